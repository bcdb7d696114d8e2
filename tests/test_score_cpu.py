"""CPU: the argument checks of qpn_score_logits (made before a device is looked for), the chunk walk of per-file scoring (loaders.score_chunks), the
float64 specification itself on hand-made rows, and the host-side refusals of the scoring API."""
import ctypes as C
import itertools

import numpy as np
import pytest

from qpnet_amd import _lib, loaders
from qpnet_amd.config import TINY
import score_spec as SP


def _call(lg=1, tg=1, stride=8, B=2, BL=8, Q=256, out=1):
    """qpn_score_logits with fake non-null pointers (never dereferenced: every check comes before the device is looked for) -> (rc, message)"""
    L = _lib.lib()
    rc = L.qpn_score_logits(C.c_void_p(4096 if lg else 0), C.c_void_p(8192 if tg else 0), stride, B, BL, Q, C.c_void_p(12288 if out else 0), None)
    return rc, L.qpn_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(lg=0), "d_logits"), (dict(tg=0), "d_targets"), (dict(out=0), "d_out"),
    (dict(B=0), "B "), (dict(B=-3), "B "), (dict(BL=0, stride=0), "BL "), (dict(Q=0), "Q "), (dict(Q=65537), "Q "),
    (dict(stride=7), "tgt_stride"), (dict(B=1 << 16, BL=1 << 15, stride=1 << 15), "B * BL"), (dict(B=1 << 20, BL=1 << 20, stride=1 << 20), "B * BL"),
])
def test_bad_arguments_are_named_before_a_device_is_looked_for(kw, name):
    rc, msg = _call(**kw)
    assert rc == -1 and msg.startswith(name), (rc, msg)


def test_the_largest_row_count_and_q_pass_the_argument_checks():
    """B * BL = 2^31 - 1 and Q = 65536, Q = 1 are valid: what comes back is not QPN_EINVAL (without a GPU: the no-device error)"""
    import torch
    if torch.cuda.is_available():
        return                                        # (a GPU would run the launch on the fake pointers)
    for kw in (dict(B=1, BL=(1 << 31) - 1, stride=(1 << 31) - 1), dict(Q=65536), dict(Q=1)):
        rc, msg = _call(**kw)
        assert rc == -2 and "no CPU fallback" in msg, (kw, rc, msg)


def test_valid_arguments_without_a_gpu_fail_loudly():
    import torch
    if torch.cuda.is_available():
        return
    L = _lib.lib()
    lg, tg, out = (C.c_float * (2 * 3 * 64))(), (C.c_int64 * (2 * 5))(), (C.c_float * (2 * 3 * 4))()
    rc = L.qpn_score_logits(C.addressof(lg), C.addressof(tg), 5, 2, 3, 64, C.addressof(out), None)
    assert rc == -2 and b"no CPU fallback" in L.qpn_last_error()


def test_python_api_refuses_cpu_tensors():
    import torch
    from qpnet_amd import train
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    T, F = 2 * TINY.upsampling_factor, 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score(torch.zeros(1, T, dtype=torch.long), torch.zeros(1, TINY.n_aux, F), torch.ones(1, T), [10], torch.zeros(1, T, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.score_logits(torch.zeros(1, 4, 256), torch.zeros(1, 4, dtype=torch.long))
    assert train.Score._fields == ("nll", "entropy", "argmax", "rank")


def test_the_dropin_module_exports_the_class_that_scores():
    import importlib.util
    import os
    import qpnet_amd.qpnet as mine
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpnet_amd", "dropin", "qpnet.py")
    spec = importlib.util.spec_from_file_location("_dropin_qpnet_for_score", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.QPNet is mine.QPNet and callable(mod.QPNet.score)


def test_run_validate_has_the_per_utterance_flag_off_by_default():
    from qpnet_amd import runners
    base = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--resultdir", "r", "--config", "c", "--checkpoint", "k"]
    assert runners._validate_args().parse_args(base).per_utterance is False
    assert runners._validate_args().parse_args(base + ["--per_utterance"]).per_utterance is True


# ---------------------------------------------------------------- the chunk walk
def _check_walk(n_frames, rf, bl_max, max_length, U):
    chunks = loaders.score_chunks(n_frames, rf, bl_max, max_length, U)
    E = (n_frames - 1) * U
    if E <= rf:
        assert chunks == []
        return 0
    covered = []
    for frame0, frames, bl, keep in chunks:
        a, T = frame0 * U, frames * U                       # frame aligned by construction: the walk hands out frames
        assert frame0 >= 0 and frame0 + frames <= n_frames - 1 and a + T <= E      # (one sample past the inputs exists: a + T <= E < n_frames U)
        assert T - bl == rf and T <= max_length and keep <= bl_max and 1 <= keep <= bl
        assert bl - keep <= U - 1                           # at most U - 1 leading rows are computed and dropped
        # rows of the chunk's Score are the target positions a + rf + 1 .. a + T; the last `keep` of them are kept
        covered.extend(range(a + T - keep + 1, a + T + 1))
    assert covered == list(range(rf + 1, E + 1)), (n_frames, rf, bl_max, max_length, U)
    return len(chunks)


@pytest.mark.parametrize("U", [1, 7, 110])
def test_score_chunks_cover_every_scored_sample_once_and_in_order(U):
    rfs = sorted({0, 1, U, 3 * U, 3 * U + 1, 5 * U - 1, 2 * U + U // 2})         # both = 0 and != 0 (mod U) where U > 1
    multi = binding = 0
    for rf in rfs:
        pairs = [(U, rf + 2 * U), (2 * U + 1, rf + 2 * U), (3 * U, rf + 5 * U + 3), (4 * U + U // 2, rf + 2 * U + 1), (1000 * U, rf + 3 * U), (1000 * U, 10 ** 6),
                 (5 * U, 10 ** 6)]
        for (bl_max, max_length), n_frames in itertools.product(pairs, range(1, 61)):
            n = _check_walk(n_frames, rf, bl_max, max_length, U)
            multi += n > 1
            binding += n > 0 and max_length - rf < bl_max
    assert multi > 100 and binding > 100                     # several chunks, and walks on which max_length (not batch_length) bounds the chunk, both occur


@pytest.mark.parametrize("U", [1, 7, 110])
def test_score_chunks_refuse_geometries_that_cannot_progress(U):
    for rf in (0, U, 3 * U + 1):
        with pytest.raises(ValueError, match="max_length"):
            loaders.score_chunks(40, rf, 20 * U, rf + 2 * U - 1, U)
        assert loaders.score_chunks(40, rf, 20 * U, rf + 2 * U, U)
    with pytest.raises(ValueError, match="batch_length"):
        loaders.score_chunks(40, 5, U - 1, 10 ** 6, U)


@pytest.mark.parametrize("U", [1, 7, 110])
def test_score_chunks_of_a_file_without_a_scored_sample_are_empty(U):
    for rf in (U, 3 * U + 1, 5 * U):
        n_last = rf // U + 1                                 # the largest n_frames with (n_frames - 1) U <= rf
        for n_frames in range(0, n_last + 1):
            assert loaders.score_chunks(n_frames, rf, 20 * U, 10 ** 6, U) == []
        assert len(loaders.score_chunks(n_last + 1, rf, 20 * U, 10 ** 6, U)) == 1


# ---------------------------------------------------------------- the specification on rows whose answers are known in closed form
def test_spec_on_closed_form_rows():
    from qpnet_amd.train import Score
    assert Score._fields == ("nll", "entropy", "argmax", "rank")          # the spec returns its four arrays in the API's order: the suites zip the two
    Q = 8
    eq = np.zeros((1, Q), np.float32)
    nll, ent, am, rk = SP.score(eq, [3])
    assert abs(nll[0] - np.log(Q)) < 1e-12 and abs(ent[0] - np.log(Q)) < 1e-12 and am[0] == 0 and rk[0] == 0
    tie = np.array([[1, 5, 2, 5, -np.inf, 0, 5, 1]], np.float32)
    nll, ent, am, rk = SP.score(np.repeat(tie, 4, 0), [3, 0, 4, 2])
    assert am.tolist() == [1, 1, 1, 1] and rk.tolist() == [0, 4, 7, 3] and np.isfinite(ent).all() and nll[2] == np.inf
    nll, ent, am, rk = SP.score(np.repeat(tie, 2, 0), [-1, Q])
    assert np.isinf(nll).all() and rk.tolist() == [Q, Q] and am.tolist() == [1, 1] and np.isfinite(ent).all()
    two = np.array([[0.0, np.log(3.0)]])
    nll, ent, am, rk = SP.score(two, [0])
    assert abs(nll[0] - np.log(4.0)) < 1e-12 and abs(ent[0] - (0.25 * np.log(4.0) + 0.75 * np.log(4.0 / 3.0))) < 1e-12 and rk[0] == 1
