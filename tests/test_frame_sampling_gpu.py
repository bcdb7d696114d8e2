"""GPU: the draw track (qpn_decode_frame_sampling; draw_track= of batch_fast_generate and generate_live) on every decode kernel, bit for bit against the
restatement of tests/frame_spec.py: sample i of a row is the controlled draw (tests/nucleus_spec.py) with the unchanged uniform and the record of frame
f(i) = min(F - 1, (n_x - 1 + i) / U).

1. Closed loop: every pick of a call with the logits output is the restated draw on the call's own logits, which are the oracle's teacher-forced logits.
2. Law C: a track that is constant in every row is the per-row call with those constants (and, one constant for all rows, the uniform call).
3. Law K: what a track holds from frame f* on, and in other rows, does not reach a sample drawn before the row enters f*.
4. Edges (seed lengths, upsampling_factor 0) and compositions (live output, cancel, the re-run after a give-up, the call after, the enqueue's checks).
Every row of every call here starts in the left padding (the receptive field is longer than the seeds)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_spec as FS
import util
from qpnet_amd import synth
from test_sampling_controls_gpu import _KERNELS, _setup, _rows_in_input_order, _teacher_forced_logits

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
RECS = [(1.0, 0, 1.0, 0.0), (0.7, 40, 0.95, 0.01), (1.3, 100, 0.9, 0.05), (0.5, 20, 0.8, 0.02)]      # consecutive entries differ in all four values
EINVAL, ESTATE = -1, -5


def _cycle_track(cfg, B, F, shift=0):
    """row b holds RECS[(f + b + shift) % 4] in frame f: every row changes all four values at every frame, and no two neighbouring rows hold the same record in a frame"""
    Q = cfg.n_quantize
    return FS.track_of([[(T, min(k, Q - 1), tp, mp) for T, k, tp, mp in (RECS[(f + b + shift) % 4] for f in range(F))] for b in range(B)])


def _call(m, xb, hb, ns, bd, want_logits=False, **kw):
    """qpn_decode behind _decode_args, with the logits output where asked -> (rows in input order, logits (B, max_n, Q) or None)"""
    import torch
    from qpnet_amd import _lib
    a = m._decode_args(xb, hb, list(ns), bd, "sampling", False, **kw)
    call = list(a["call"])
    logits = None
    if want_logits:
        logits = torch.empty((a["B"], max(a["max_n"], 1), m.n_quantize), dtype=torch.float32, device=a["dev"])
        call[15] = logits.data_ptr()
    try:
        with torch.cuda.device(a["dev"]):
            _lib.check(a["L"].qpn_decode(*call))
            m.last_decode_plan = a["L"].qpn_last_decode_plan(a["hd"]).decode()
    finally:
        _lib.check(a["L"].qpn_decode_frame_sampling(a["hd"], 0, 0, None))
    out = a["out"].cpu().numpy()
    return [out[b, :n].copy() for b, n in enumerate(a["ns"])], (logits.cpu().numpy() if want_logits else None)


def _seeded_batch(cfg, utts, n_x):
    """util.decode_batch with seeds of n_x samples: n_x - 1 more known samples in front of the usual one, as many fewer to generate"""
    bx, bh, bd, ns = util.decode_batch(cfg, utts)
    if n_x > 1:
        more = np.random.RandomState(7 + n_x).randint(0, cfg.n_quantize, size=(bx.shape[0], n_x - 1)).astype(np.int64)
        bx = np.ascontiguousarray(np.concatenate([more, bx], axis=1))
        ns = [n - (n_x - 1) for n in ns]
    return bx, bh, bd, ns


def _assert_restated(kernel, m, oracle, cfg, flat, batch, rows, logits, track, seed_of, stream_of, check, n_x):
    bx, bh, bd, ns = batch
    U, F = cfg.upsampling_factor, bh.shape[2]
    for b in check:
        y = rows[b]
        assert len(y) == ns[b] and 0 <= y.min() and y.max() < cfg.n_quantize
        lg = _teacher_forced_logits(oracle, cfg, flat, batch, b, y) if logits is None else logits[b, :ns[b]]
        want = FS.draw_track_steps(lg, seed_of(b), stream_of(b), FS.row_of(track, b), n_x, U, F)
        diff = np.nonzero(want != y)[0]
        assert diff.size == 0, "%s row %d (%s): first difference at step %d of %d (frame %d): kernel %d, spec %d" % (
            kernel, b, m.last_decode_plan, diff[0], len(y), FS.frame_of(int(diff[0]), n_x, U, F), y[diff[0]], want[diff[0]])
        if logits is not None:      # the call's own logits are the oracle's teacher-forced logits of its picks, bit for bit (what the closed-loop tests of the other controls rest on)
            ref = _teacher_forced_logits(oracle, cfg, flat, batch, b, y)
            assert np.array_equal(lg.view(np.uint32), ref.view(np.uint32)), "%s row %d: logits differ from the oracle's, max abs diff %g" % (kernel, b, np.abs(lg - ref).max())


@pytest.mark.parametrize("kernel", list(_KERNELS))
def test_closed_loop_with_a_track_on_every_kernel(kernel, cuda, oracle, monkeypatch):
    """Seeds of three samples, five and four frames: every row changes all four values at each of its frames (four and three changes), the first one
    U - 2 steps in, the last one on entering its last frame; rows are shifted against each other, and in pipe2's batch the two rows that alternate in a
    five-role group hold different records at every step."""
    import torch
    cfg, flat, m, plan, _, _ = _setup(kernel, cuda, monkeypatch)
    B, n_x = _KERNELS[kernel][3], 3
    batch = _seeded_batch(cfg, [(61 + b, 5 if b % 2 == 0 else 4, (1.0, 0.5)[b % 2]) for b in range(B)], n_x)
    bx, bh, bd, ns = batch
    U, F = cfg.upsampling_factor, bh.shape[2]
    assert F == 5 and FS.first_step_of(1, n_x, U) == U - 2 and all(FS.frame_of(n - 1, n_x, U, F) == n_f - 1 for n, n_f in zip(ns[:2], (5, 4)))
    track = _cycle_track(cfg, B, F)
    m.sampling_seed = SEED
    rows, logits = _call(m, torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), ns, bd, want_logits=True, draw_track=track)
    assert plan in m.last_decode_plan, m.last_decode_plan
    check = range(B) if B <= 2 else [0, 1, 2, 3, B - 2, B - 1]      # (pipe2: the longest rows and the shortest, which share groups)
    _assert_restated(kernel, m, oracle, cfg, flat, batch, rows, logits, track, lambda b: SEED, lambda b: b, check, n_x)
    for b in check:      # the records are felt: the row is not what its first frame's record alone would draw
        const = FS.draw_track_steps(logits[b, :ns[b]], SEED, b, {k: np.repeat(v[b, :1], F) for k, v in track.items()}, n_x, U, F)
        assert not np.array_equal(const, rows[b])


@pytest.mark.parametrize("kernel", list(_KERNELS))
def test_law_c_a_constant_track_is_the_per_row_call(kernel, cuda, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B, F, Q = len(ns), bh.shape[2], cfg.n_quantize
    m.sampling_seed = SEED
    ctl = [(T, min(k, Q - 1), tp, mp) for T, k, tp, mp in (RECS[1 + b % 3] for b in range(B))]
    track = FS.track_of([[ctl[b]] * F for b in range(B)])
    got = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", draw_track=track), ns)
    assert plan in m.last_decode_plan, m.last_decode_plan
    per_row = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=[c[0] for c in ctl], top_k=[c[1] for c in ctl],
                                                         top_p=[c[2] for c in ctl], min_p=[c[3] for c in ctl]), ns)
    for b in range(B):
        np.testing.assert_array_equal(got[b], per_row[b], err_msg="%s row %d %r" % (kernel, b, ctl[b]))
    # ... with row seeds: key and counter word come from the row's record, the values from the track
    seeds = [(0xC0FFEE0000000001 + 0x9E3779B97F4A7C15 * (b + 1)) % (1 << 64) | (1 << 63) for b in range(B)]
    got = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", draw_track=track, row_seeds=seeds), ns)
    per_row_s = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=[c[0] for c in ctl], top_k=[c[1] for c in ctl],
                                                           top_p=[c[2] for c in ctl], min_p=[c[3] for c in ctl], row_seeds=seeds), ns)
    for b in range(B):
        np.testing.assert_array_equal(got[b], per_row_s[b], err_msg="%s row %d %r with row seeds" % (kernel, b, ctl[b]))
    assert not np.array_equal(per_row_s[0], per_row[0])
    # one record for all rows, (F,) arrays shared by the rows: the uniform call
    c = ctl[0]
    shared = {k: np.repeat(v[0, :1], F) for k, v in track.items()}
    got = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", draw_track=shared), ns)
    uni = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=c[0], top_k=c[1], top_p=c[2], min_p=c[3]), ns)
    for b in range(B):
        np.testing.assert_array_equal(got[b], uni[b], err_msg="%s row %d %r against the uniform call" % (kernel, b, c))
    # a key the track does not hold takes the call's value of that name: two keys from the track, two from the scalars
    half = {k: shared[k] for k in ("temperature", "top_p")}
    got = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", draw_track=half, top_k=c[1], min_p=c[3]), ns)
    for b in range(B):
        np.testing.assert_array_equal(got[b], uni[b], err_msg="%s row %d: missing keys" % (kernel, b))


@pytest.mark.parametrize("kernel", [n for n in _KERNELS if n != "pipe2"])
def test_law_k_later_frames_and_other_rows_do_not_reach_earlier_samples(kernel, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B, F, U, Q = len(ns), bh.shape[2], cfg.upsampling_factor, cfg.n_quantize
    assert B == 2 and F == 4
    m.sampling_seed = SEED
    first = _cycle_track(cfg, B, F)
    f_star = 2
    second = {k: v.copy() for k, v in _cycle_track(cfg, B, F, shift=1).items()}      # row 1: another record in every frame
    for k in FS.KEYS:
        second[k][0, :f_star] = first[k][0, :f_star]                                  # row 0: the same up to f*, then top_k = 1 with whatever else
    second["top_k"][0, f_star:] = 1
    assert all((first[k][1] != second[k][1]).all() for k in FS.KEYS)
    a_rows, _ = _call(m, xb, hb, ns, bd, draw_track=first)
    b_rows, b_logits = _call(m, xb, hb, ns, bd, want_logits=True, draw_track=second)
    assert plan in m.last_decode_plan, m.last_decode_plan
    i_star = FS.first_step_of(f_star, 1, U)
    assert 0 < i_star < ns[0] and FS.frame_of(i_star, 1, U, F) == f_star and FS.frame_of(i_star - 1, 1, U, F) == f_star - 1
    np.testing.assert_array_equal(b_rows[0][:i_star], a_rows[0][:i_star], err_msg="%s: samples before the tracks part" % kernel)
    lg = b_logits[0, i_star:ns[0]]
    untied = (lg == lg.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert untied.sum() > 0.9 * len(lg)
    np.testing.assert_array_equal(b_rows[0][i_star:][untied], lg.argmax(axis=1)[untied], err_msg="%s: top_k = 1 from frame %d on" % (kernel, f_star))
    assert not np.array_equal(b_rows[0][i_star:], a_rows[0][i_star:]) and not np.array_equal(b_rows[1], a_rows[1])
    # row 0 keeps its track, row 1 changes everywhere: row 0 does not notice
    third = {k: np.stack([first[k][0], second[k][1]]) for k in FS.KEYS}
    c_rows, _ = _call(m, xb, hb, ns, bd, draw_track=third)
    np.testing.assert_array_equal(c_rows[0], a_rows[0], err_msg="%s: row 0 with another track in row 1" % kernel)
    np.testing.assert_array_equal(c_rows[1], b_rows[1])


@pytest.mark.parametrize("n_x", [1, 3, 5])
@pytest.mark.parametrize("kernel", ["pipe", "one-cu", "tiny"])
def test_seed_lengths_shift_the_frame_of_a_sample(kernel, n_x, cuda, oracle, monkeypatch):
    """c(i) = n_x - 1 + i: with longer seeds a row enters every frame earlier (and the warm-up over a seed of >= 3 samples pairs its steps with the frame before)"""
    import torch
    cfg, flat, m, plan, _, _ = _setup(kernel, cuda, monkeypatch)
    batch = _seeded_batch(cfg, [(61, 4, 1.0), (62, 3, 0.5)], n_x)
    bx, bh, bd, ns = batch
    track = _cycle_track(cfg, 2, bh.shape[2])
    m.sampling_seed = SEED
    rows, _ = _call(m, torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), ns, bd, draw_track=track)
    assert plan in m.last_decode_plan, m.last_decode_plan
    _assert_restated(kernel, m, oracle, cfg, flat, batch, rows, None, track, lambda b: SEED, lambda b: b, range(2), n_x)


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_upsampling_factor_zero_one_record_per_sample(cfgname, cuda, oracle):
    """upsampling_factor = 0 (the configuration of test_decode_gpu.test_upsampling_factor_zero_decode_vs_oracle): the features arrive at sample rate, f(i) = min(F - 1, i)"""
    import torch
    from qpnet_amd.config import TINY, PAPER
    cfg_u = TINY if cfgname == "tiny" else PAPER
    cfg0 = dataclasses.replace(cfg_u, upsampling_factor=0)
    flat = synth.make_weights(cfg0, 19)
    m = util.build_model(cfg0, flat, cuda)
    x, h, d, n = synth.decode_inputs(cfg_u, 4, 23, 1.0)
    h0 = np.ascontiguousarray(np.repeat(h, cfg_u.upsampling_factor, axis=1))
    F = h0.shape[1]
    assert F == n + 1
    rs = np.random.RandomState(5)
    pick = rs.randint(0, 4, size=F)                                  # another record at (nearly) every sample
    track = FS.track_of([[RECS[j] for j in pick]])
    m.sampling_seed = 99
    batch = (x[None], h0[None], d[None], [n])
    rows, _ = _call(m, torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h0[None]).to(cuda), [n], d[None], draw_track=track)
    _assert_restated(cfgname, m, oracle, cfg0, flat, batch, rows, None, track, lambda b: 99, lambda b: b, [0], 1)


def test_generate_live_and_cancel_with_a_track(cuda, monkeypatch):
    """generate_live(draw_track=): its pieces, concatenated, are batch_fast_generate's rows; with on_close="cancel" what was handed over of a row is a prefix
    of the full row; the setter is refused while the call is in flight; the call after is the call of a model that never had a track."""
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("pipe", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED
    plain = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)      # (before any track)
    plain_plan = m.last_decode_plan
    track = _cycle_track(cfg, 2, bh.shape[2])
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", draw_track=track), ns)
    got = [[] for _ in ns]
    first = True
    for b, start, piece in m.generate_live(xb, hb, list(ns), bd, every=64, mode="sampling", draw_track=track):
        if first:
            first = False
            rec = (_lib.QpnFrameDraw * 8)(*[_lib.QpnFrameDraw(1.0, 0, 1.0, 0.0)] * 8)
            assert _lib.lib().qpn_decode_frame_sampling(m._handle, 2, 4, rec) == ESTATE      # a decode is in flight
            assert _lib.lib().qpn_decode_frame_sampling(m._handle, 0, 0, None) == ESTATE
        assert start == sum(len(p) for p in got[b])
        got[b].append(piece)
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(got[b]), want[b])
        assert not np.array_equal(want[b], plain[b])
    gen = m.generate_live(xb, hb, list(ns), bd, every=32, on_close="cancel", mode="sampling", draw_track=track)
    got = [[] for _ in ns]
    for b, start, piece in gen:
        got[b].append(piece)
        break
    gen.close()
    counts = m.last_decode_counts
    assert counts is not None and len(counts) == len(ns)
    for b in range(len(ns)):
        have = np.concatenate(got[b]) if got[b] else np.zeros(0, dtype=np.int64)
        assert len(have) <= counts[b] <= ns[b]
        np.testing.assert_array_equal(have, want[b][:len(have)])
    again = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)
    assert m.last_decode_plan == plain_plan
    for b in range(len(ns)):
        np.testing.assert_array_equal(again[b], plain[b])


def test_rerun_after_a_give_up_draws_with_the_same_track():
    """The fault-injection hook exists only in the -DQPN_TESTING build: the scenario runs in a child process of its own bound to it (tests/frame_sampling_giveup_child.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0", QPN_TEST_PIPE_GIVES_UP="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "frame_sampling_giveup_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FRAME_SAMPLING_GIVEUP_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_enqueue_refuses_a_call_that_does_not_match_the_track(cuda, monkeypatch):
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("tiny", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    L = _lib.lib()
    B, F = len(ns), bh.shape[2]
    a = m._decode_args(xb, hb, list(ns), bd, "sampling", False)          # (clears the track; B = 2, F = 4)
    neutral = _lib.QpnFrameDraw(1.0, 0, 1.0, 0.0)
    try:
        _lib.check(L.qpn_decode_frame_sampling(a["hd"], B + 1, F, (_lib.QpnFrameDraw * ((B + 1) * F))(*[neutral] * ((B + 1) * F))))
        assert L.qpn_decode_enqueue(*a["call"]) == EINVAL and "n_rows" in L.qpn_last_error().decode()
        assert L.qpn_decode(*a["call"]) == EINVAL and "n_rows" in L.qpn_last_error().decode()
        _lib.check(L.qpn_decode_frame_sampling(a["hd"], B, F + 1, (_lib.QpnFrameDraw * (B * (F + 1)))(*[neutral] * (B * (F + 1)))))
        assert L.qpn_decode_enqueue(*a["call"]) == EINVAL and "n_frames" in L.qpn_last_error().decode()
        # QPN_MODE_ARGMAX calls ignore the track
        g = m._decode_args(xb, hb, list(ns), bd, "argmax", False)
        _lib.check(L.qpn_decode_frame_sampling(g["hd"], B + 1, F, (_lib.QpnFrameDraw * ((B + 1) * F))(*[neutral] * ((B + 1) * F))))
        import torch
        with torch.cuda.device(g["dev"]):
            _lib.check(L.qpn_decode(*g["call"]))
        out = g["out"].cpu().numpy()
        greedy = [out[b, :n].copy() for b, n in enumerate(ns)]
    finally:
        _lib.check(L.qpn_decode_frame_sampling(a["hd"], 0, 0, None))
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="argmax"), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(greedy[b], want[b])
