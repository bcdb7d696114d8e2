"""CPU: the draw track (qpn_decode_frame_sampling; draw_track= of batch_fast_generate / generate_live; loaders.uv_draw_track; run_decode's
--<control>_voiced / _unvoiced flags) -- what is checked before a device is looked at: the ABI's argument rules on a handle created without a GPU, the
Python surface's ValueErrors in front of the device layer, the voiced / unvoiced track builder, and the frame a generated sample draws with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_spec as FS
from qpnet_amd import _lib, loaders
from qpnet_amd.config import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0
GOOD = (0.7, 40, 0.9, 0.05)


@pytest.fixture()
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0      # (without a GPU: a geometry-only handle)
    yield L, hp
    L.qpn_destroy(hp)


def _recs(recs):
    return (_lib.QpnFrameDraw * len(recs))(*[_lib.QpnFrameDraw(*r) for r in recs])


def test_abi_refuses_bad_records_naming_field_row_and_frame(handle):
    L, hp = handle
    Q = TINY.n_quantize
    bad = {"temperature": [(0.0, 0, 1.0, 0.0), (-1.0, 0, 1.0, 0.0), (float("nan"), 0, 1.0, 0.0), (float("inf"), 0, 1.0, 0.0), (1e-45, 0, 1.0, 0.0)],
           "top_k": [(1.0, -1, 1.0, 0.0), (1.0, Q + 1, 1.0, 0.0)],
           "top_p": [(1.0, 0, 0.0, 0.0), (1.0, 0, 1.5, 0.0), (1.0, 0, float("nan"), 0.0)],
           "min_p": [(1.0, 0, 1.0, -0.1), (1.0, 0, 1.0, 1.5), (1.0, 0, 1.0, float("nan"))]}
    n_rows, n_frames = 3, 5
    for field, recs in bad.items():
        for rec in recs:
            for row, frame in ((0, 0), (1, 4), (2, 3)):
                table = [GOOD] * (n_rows * n_frames)
                table[row * n_frames + frame] = rec
                assert L.qpn_decode_frame_sampling(hp, n_rows, n_frames, _recs(table)) == EINVAL, (field, rec)
                msg = L.qpn_last_error().decode()
                assert field in msg and ("row %d frame %d: " % (row, frame)) in msg, msg
                # the per-value message is qpn_decode_sampling_ex's, with the row and the frame in front
                assert L.qpn_decode_sampling_ex(hp, *rec) == EINVAL
                assert msg == "row %d frame %d: %s" % (row, frame, L.qpn_last_error().decode())
    assert L.qpn_decode_frame_sampling(hp, -1, 5, _recs([GOOD] * 5)) == EINVAL and "n_rows" in L.qpn_last_error().decode()
    assert L.qpn_decode_frame_sampling(hp, 1, 0, _recs([GOOD])) == EINVAL and "n_frames" in L.qpn_last_error().decode()
    assert L.qpn_decode_frame_sampling(hp, 2, 5, None) == EINVAL and "NULL" in L.qpn_last_error().decode()
    assert L.qpn_decode_frame_sampling(None, 0, 0, None) == EINVAL


def test_abi_accepts_a_good_track_and_switches_off(handle):
    L, hp = handle
    Q = TINY.n_quantize
    assert L.qpn_decode_frame_sampling(hp, 0, 0, None) == OK                     # off on a handle that never had one
    assert L.qpn_decode_frame_sampling(hp, 2, 3, _recs([GOOD, (1.0, 0, 1.0, 0.0), (100.0, Q, 1.0, 1.0)] * 2)) == OK
    assert L.qpn_decode_frame_sampling(hp, 1, 1, _recs([GOOD])) == OK            # replaces the table
    assert L.qpn_decode_frame_sampling(hp, 0, 7, _recs([GOOD])) == OK            # 0 rows: off, whatever the rest
    assert L.qpn_decode_frame_sampling(hp, 0, 0, None) == OK


def test_record_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "qpnet_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} qpn_frame_draw;", hdr)
    assert m, "qpn_frame_draw is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "float temperature; int32_t top_k; float top_p, min_p;"
    assert re.search(r"int qpn_decode_frame_sampling\(qpn_handle\* ?h?, int n_rows, int64_t n_frames, const qpn_frame_draw\* h_track\);", hdr)
    assert [n for n, _ in _lib.QpnFrameDraw._fields_] == ["temperature", "top_k", "top_p", "min_p"]
    assert C.sizeof(_lib.QpnFrameDraw) == 16 and _lib.QpnFrameDraw.top_k.offset == 4 and _lib.QpnFrameDraw.min_p.offset == 12
    assert "qpn_decode_frame_sampling" in {n for n, _, _ in _lib.SYMBOLS}


def test_python_surface_refuses_bad_tracks_before_any_device_work():
    """CPU tensors: a call that reached the device layer would raise RuntimeError (no CPU fallback); a bad track raises ValueError first."""
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    B, F = 2, 4
    args = (torch.zeros(B, 1, dtype=torch.long), torch.zeros(B, 39, F), [10, 10], np.ones((B, 440)))
    ok_t = np.full((B, F), 0.7, dtype=np.float32)
    bad = (dict(draw_track=dict(temperature=np.ones((B, F + 1)))), dict(draw_track=dict(temperature=np.ones((B + 1, F)))), dict(draw_track=dict(top_k=np.zeros(F - 1, dtype=int))),      # bad shapes
           dict(draw_track=dict(top_p=np.ones((B, F, 1)))), dict(draw_track=dict(min_p=0.1)), dict(draw_track=dict(top_p=torch.ones(F + 2))),
           dict(draw_track=dict(temperature=ok_t), temperature=0.7), dict(draw_track=dict(top_k=np.zeros(F, dtype=int)), top_k=5),                                           # a key given twice
           dict(draw_track=dict(top_p=np.ones(F)), top_p=[0.9, 0.9]), dict(draw_track=dict(min_p=np.zeros(F)), min_p=0.05),
           dict(draw_track=dict(temperature=ok_t), mode="argmax"), dict(draw_track={}, mode="argmax"),                                                                      # argmax draws nothing
           dict(draw_track=dict(temp=ok_t)), dict(draw_track=[ok_t]), dict(draw_track=dict(top_k=np.ones(F))), dict(draw_track=dict(temperature=np.array(["a"] * F))))       # not a track
    for kw in bad:
        with pytest.raises(ValueError):
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(ValueError):
            m.generate_live(*args, **kw)
    with pytest.raises(ValueError, match="temperature / top_k / top_p / min_p shape the draw of mode='sampling'; mode='argmax' takes none of them"):
        m.batch_fast_generate(*args, mode="argmax", draw_track=dict(top_k=np.zeros(F, dtype=int)))      # (the error the other controls raise)
    with pytest.raises(ValueError, match="given twice"):
        m.batch_fast_generate(*args, draw_track=dict(temperature=ok_t), temperature=0.7)
    # a bad value names the key, the row and the frame
    for key, good, badv in (("temperature", 1.0, 0.0), ("temperature", 1.0, float("nan")), ("top_k", 0, -1), ("top_k", 0, TINY.n_quantize + 1), ("top_p", 1.0, 0.0), ("top_p", 1.0, 1.5),
                            ("min_p", 0.0, -0.1), ("min_p", 0.0, float("nan"))):
        v = np.full((B, F), good, dtype=np.int64 if key == "top_k" else np.float64)
        v[1, 2] = badv
        with pytest.raises(ValueError, match=r"%s.* row 1 frame 2: " % key):
            m.batch_fast_generate(*args, draw_track={key: v})
        with pytest.raises(ValueError, match=r"%s.* row 1 frame 2: " % key):
            m.generate_live(*args, draw_track={key: v})
        shared = v[1].copy()                                                    # (F,): every row -- the first row that has it is named
        with pytest.raises(ValueError, match=r"%s.* row 0 frame 2: " % key):
            m.batch_fast_generate(*args, draw_track={key: shared})
    good = (dict(draw_track=dict(temperature=ok_t)), dict(draw_track=dict(top_k=np.array([0, 5, 40, 1]))), dict(draw_track=dict(top_p=torch.full((B, F), 0.9), min_p=[0.0, 0.05, 0.0, 0.1])),
            dict(draw_track=dict(temperature=ok_t), top_k=5, top_p=[0.9, 1.0], row_seeds=[3, 4]), dict(draw_track={}), dict(draw_track=None))
    for kw in good:
        with pytest.raises(RuntimeError, match="no CPU fallback"):               # good values go on to the device layer
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate_live(*args, **kw)
    with pytest.raises(TypeError):                                               # keyword-only, behind row_seeds
        m.batch_fast_generate(*args, None, "sampling", False, dict(temperature=ok_t))


def test_uv_draw_track_follows_feature_column_zero():
    h = np.random.RandomState(3).standard_normal((2, 5, 6)).astype(np.float32)
    h[0, 0] = [1, 1, 1, 0, 0, 0]                                                 # a voiced-to-unvoiced edge between frames 2 and 3
    h[1, 0] = [0, 1, 0.51, 0.5, 1, 0]                                            # > 0.5 is voiced: 0.5 itself is not
    voiced, unvoiced = dict(temperature=0.7, top_k=40), dict(temperature=1.0, top_k=0)
    t = loaders.uv_draw_track(h, voiced, unvoiced)
    assert sorted(t) == ["temperature", "top_k"] and t["temperature"].dtype == np.float32 and t["top_k"].dtype == np.int32
    np.testing.assert_array_equal(t["temperature"], np.float32([[0.7, 0.7, 0.7, 1, 1, 1], [1, 0.7, 0.7, 1, 0.7, 1]]))
    np.testing.assert_array_equal(t["top_k"], [[40, 40, 40, 0, 0, 0], [0, 40, 40, 0, 40, 0]])
    import torch
    t2 = loaders.uv_draw_track(torch.from_numpy(h), dict(top_p=0.8, min_p=0.0), dict(top_p=1.0, min_p=0.02))
    np.testing.assert_array_equal(t2["top_p"][0], np.float32([0.8, 0.8, 0.8, 1, 1, 1]))
    np.testing.assert_array_equal(t2["min_p"][0], np.float32([0, 0, 0, 0.02, 0.02, 0.02]))
    assert loaders.uv_draw_track(h, {}, {}) == {}
    for bad in ((dict(temperature=1.0), {}), (dict(temp=1.0), dict(temp=1.0))):
        with pytest.raises(ValueError):
            loaders.uv_draw_track(h, *bad)
    with pytest.raises(ValueError):
        loaders.uv_draw_track(h[0], voiced, unvoiced)


def test_run_decode_has_the_flags_off_by_default():
    from qpnet_amd import runners
    need = ["--feats", "f", "--stats", "s", "--config", "c", "--outdir", "o", "--checkpoint", "k"]
    a = runners._decode_args().parse_args(need + ["--temperature", "0.8", "--top_k", "7"])
    for name in ("temperature", "top_k", "top_p", "min_p"):
        assert getattr(a, name + "_voiced") is None and getattr(a, name + "_unvoiced") is None
    plain, voiced, unvoiced = runners.uv_decode_controls(a)
    assert plain == dict(temperature=0.8, top_k=7, top_p=1.0, min_p=0.0) and voiced == {} and unvoiced == {}      # the call it always made
    a = runners._decode_args().parse_args(need + ["--temperature", "0.8", "--temperature_voiced", "0.6", "--top_k_unvoiced", "0", "--top_k", "30", "--min_p_voiced", "0.1", "--min_p_unvoiced", "0.2"])
    plain, voiced, unvoiced = runners.uv_decode_controls(a)
    assert plain == dict(top_p=1.0)                                              # a control that has a track leaves its keyword at the default
    assert voiced == dict(temperature=0.6, top_k=30, min_p=0.1) and unvoiced == dict(temperature=0.8, top_k=0, min_p=0.2)      # the unset side: the plain flag's value


@pytest.mark.parametrize("U", [0, 4])
@pytest.mark.parametrize("n_x", [1, 3])
def test_frame_of_a_sample_is_the_reference_current_index(n_x, U, ):
    """The reference (qpnet.py:343-359, 443-451): h is upsampled (frame f fills columns f U .. f U + U - 1), padded on the left by n_pad replicated columns like x,
    and step i reads column current_index = samples.size(-1) - 1 of it, samples being the padded seed plus the i samples generated so far."""
    n_pad, n = 7, 21
    last_c = n_x - 1 + (n - 1)                                                   # the un-padded column of the last step
    per = U if U > 0 else 1
    for F in (-(-(last_c + 1) // per), -(-last_c // per)):                       # exactly covering the last step / one column short of it
        cols = np.repeat(np.arange(F), per)                                      # frame of every column of the upsampled h
        padded = np.concatenate([np.full(n_pad, cols[0]), cols])                 # F.pad(h, (n_pad, 0), "replicate")
        for i in range(n):
            current_index = (n_pad + n_x + i) - 1
            want = padded[min(current_index, len(padded) - 1)]                   # (past the features: the last frame)
            assert FS.frame_of(i, n_x, U, F) == want, (n_x, U, F, i)
        for f in range(F):
            i0 = FS.first_step_of(f, n_x, U)
            assert FS.frame_of(i0, n_x, U, F) >= f and (i0 == 0 or FS.frame_of(i0 - 1, n_x, U, F) < f)
