"""GPU: gradient accumulation in the fused trainer -- k_grad_accum behind qpn_grad_accumulate, the one-call micro-step qpn_train_step_acc,
FusedTrainer(accum_steps=K) on one rank and in the data-parallel shape, and run_train --accum_steps.

A window of K chunks is the sum a data-parallel step takes over K ranks, taken over time: the yardstick is the one tests/test_parallel_gpu.py holds two ranks to
(oracle/train_oracle.py on the UNION batch of every update, the same chunks: TINY, weights seed 3, synth.train_inputs(TINY, bl, 900 + ci, 30000) with bl = 300,
410, 350, 280).  The backward's float atomics make two runs of one chunk differ in the last bits, so whatever is held bit for bit here is computed from the buffers
the very call under test left behind."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY
import util

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ERANGE = -1, -4
BLS = [300, 410, 350, 280]
WSEED, LR = 3, 1e-4
N = TINY.n_params


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def handle(cuda):
    """one TINY handle for the C-ABI tests"""
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _chunk_np(ci):
    return synth.train_inputs(TINY, BLS[ci], 900 + ci, 30000)


def _oracle_chunk(flat, ci):
    from oracle import train_oracle as TO
    x, h, t, d, b = _chunk_np(ci)
    lg, caches = TO.forward(TINY, flat, x, h, d, b)
    BL = int(b[0])
    loss, dl = TO.ce_loss(lg, t[:, -BL:])
    return dict(loss=float(loss), g=TO.backward(TINY, flat, caches, dl), caches=caches, dl=dl, rows=x.shape[0] * BL)


def _union(per, gs=None):
    """the float64 row-weighted mean of the chunks' gradients: the gradient of the mean CE over all the window's rows"""
    gs = [p["g"] for p in per] if gs is None else gs
    return sum(g.astype(np.float64) * p["rows"] for g, p in zip(gs, per)) / sum(p["rows"] for p in per)


@pytest.fixture(scope="module")
def ref():
    """the oracle's trajectory, computed once and left unchanged: two windows of two chunks from make_weights(TINY, 3); per window the chunks' losses and gradients at
    the window's starting weights, their union gradient, and the weights after TO.Adam's step on it"""
    from oracle import train_oracle as TO
    flat = synth.make_weights(TINY, WSEED).copy()
    opt = TO.Adam(flat.size, lr=LR)
    wins = []
    for w in range(2):
        per = [_oracle_chunk(flat, 2 * w + k) for k in range(2)]
        un = _union(per)
        win = dict(start=flat.copy(), per=per, union=un)
        opt.step(flat, un.astype(F))
        win["after"] = flat.copy()
        wins.append(win)
    return wins


def _applied(L, hp):
    n = C.c_int64(-1)
    _lib.check(L.qpn_train_applied_updates(hp, C.byref(n), _stream()))
    return int(n.value)


# ---------------------------------------------------------------- 1. the kernel against numpy
def _off_tensor(cuda, a, off):
    """a device copy of `a` that starts `off` floats into its allocation"""
    import torch
    t = torch.empty(a.size + off, dtype=torch.float32, device=cuda)
    t[off:].copy_(torch.from_numpy(a))
    v = t[off:]
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


# block edges, a short last quad and none, TINY's n + 4, more than one stride of the grid (3 * 2^20 + 1 floats: 786 433 quads over at most 256 CUs * 8 * 256 threads)
@pytest.mark.parametrize("cnt", [1, 3, 255, 256, 257, 52595, 3 * 2 ** 20 + 1])
def test_kernel_against_numpy(cnt, cuda, handle):
    """acc and g independently 16-byte aligned or one float into their allocation (the float4 form needs both aligned): first = 1 onto an accumulator full of NaNs
    leaves exactly g; first = 0 with a second vector leaves numpy's float32 a + b, bit for bit; g is never written; d_acc == d_grad is refused."""
    import torch
    L, hp = handle
    rs = np.random.RandomState(4000 + cnt % 977)
    a = (rs.standard_normal(cnt) * 3.0).astype(F)
    b = (rs.standard_normal(cnt) * 3.0 * 10.0 ** rs.randint(-3, 4, cnt)).astype(F)       # (magnitudes apart: the add rounds)
    want = a + b
    assert want.dtype == F
    for oa in (0, 1):
        for og in (0, 1):
            acc = _off_tensor(cuda, np.full(cnt, np.nan, F), oa)
            ga, gb = _off_tensor(cuda, a, og), _off_tensor(cuda, b, og)
            _lib.check(L.qpn_grad_accumulate(hp, acc.data_ptr(), ga.data_ptr(), cnt, 1, _stream()))
            assert torch.equal(acc, ga)
            _lib.check(L.qpn_grad_accumulate(hp, acc.data_ptr(), gb.data_ptr(), cnt, 0, _stream()))
            got = acc.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (oa, og, int(np.sum(got.view(np.uint32) != want.view(np.uint32))))
            assert np.array_equal(ga.cpu().numpy(), a) and np.array_equal(gb.cpu().numpy(), b)
            assert L.qpn_grad_accumulate(hp, acc.data_ptr(), acc.data_ptr(), cnt, 0, _stream()) == EINVAL and b"d_acc is d_grad" in L.qpn_last_error()
            assert np.array_equal(acc.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- 2. the one-call path, bit for bit
class _Bufs:
    """the caller-owned buffers of qpn_train_step_acc for TINY from weights `w0`; the accumulator starts full of NaNs (micro-step 0 must overwrite it)"""

    def __init__(self, cuda, w0):
        import torch
        self.cuda = cuda
        self.flat = torch.from_numpy(w0.copy()).to(cuda)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.ema = self.flat.clone()
        self.g = torch.zeros(N + 4, dtype=torch.float32, device=cuda)
        self.acc = torch.full((N + 4,), float("nan"), dtype=torch.float32, device=cuda)
        self.keep = []

    def call(self, L, hp, chunk, micro, count, mode, clip, decay, step=1, acc=True):
        import torch
        x, h, t, d, b = chunk
        B, T = x.shape
        BL = int(b[0])
        maxd = int(np.ceil(d).max())
        xt, ht, tt, dt = _to(self.cuda, x, h, t, d)
        logits = torch.empty((B, BL, TINY.n_quantize), dtype=torch.float32, device=self.cuda)
        dlogits = torch.empty_like(logits)
        self.keep = [xt, ht, tt, dt, logits, dlogits]
        loss, valid, norm = C.c_double(0.0), C.c_int(0), C.c_double(0.0)
        rc = L.qpn_train_step_acc(hp, self.flat.data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr(),
                                  tt.data_ptr(), tt.shape[1], logits.data_ptr(), dlogits.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), N,
                                  step, LR, 0.9, 0.999, 1e-8, 0.0, mode, C.byref(loss), C.byref(valid), clip, C.byref(norm),
                                  self.ema.data_ptr() if decay else None, decay, self.acc.data_ptr() if acc else None, micro, count, _stream())
        return rc, loss.value, valid.value, norm.value


@pytest.mark.parametrize("mode", [1, 2])
def test_one_call_window_bit_for_bit(mode, cuda, handle, ref):
    """K = 3 (bl = 300, 410, 350), clipping at half the expected norm, ema_decay 0.9.  After every call d_grad and d_acc are read back: the accumulator is the
    sequential float32 sum (g0 + g1) + g2 of the calls' own gradient buffers, trailer included -- {the three chunks' rows, 0, 0, 0} --; weights, moments and average
    stay put until the closing call and then equal, bit for bit, qpn_adam_step_avg(d_grad = a copy of the accumulator, den = that copy + n, same clip / decay) on
    copies of the state the window started from; one update was applied; the norm comes with the closing micro-step's loss only (mode 1: one call late, out of
    the pinned slot; mode 2: in the call).  Every micro-step's loss is the oracle's for its chunk at the window's starting weights (1e-4).
    (train_inputs cuts a chunk of bl = 410 to 402 rows: the rows are what the chunk says, b[0].)"""
    import torch
    L, hp = handle
    w0 = synth.make_weights(TINY, WSEED)
    per = ref[0]["per"] + [_oracle_chunk(w0, 2)]
    un = _union(per)
    expect = float(np.sqrt((un ** 2).sum()))
    clip = 0.5 * expect
    bufs = _Bufs(cuda, w0)
    start = [t.clone() for t in (bufs.flat, bufs.m, bufs.v, bufs.ema)]
    before = _applied(L, hp)
    gs, accs, outs = [], [], []
    for k in range(3):
        rc, loss, valid, norm = bufs.call(L, hp, _chunk_np(k), k, 3, mode, clip, 0.9)
        assert rc == 0, L.qpn_last_error()
        gs.append(bufs.g.cpu().numpy()); accs.append(bufs.acc.cpu().numpy())
        outs.append((loss, valid, norm))
        if k < 2:
            assert all(torch.equal(a, b) for a, b in zip((bufs.flat, bufs.m, bufs.v, bufs.ema), start)), "micro-step %d moved the state" % k
            assert _applied(L, hp) == before
    # each call's buffer: rows * gradient, then {rows, 0, 0, 0}
    from oracle import train_oracle as TO
    rows = [p["rows"] for p in per]
    for k in range(3):
        np.testing.assert_array_equal(gs[k][N:], np.array([rows[k], 0, 0, 0], F))
        util.assert_grads_match_oracle(TO, TINY, w0, per[k]["caches"], per[k]["dl"], gs[k][:N] / F(rows[k]), og=per[k]["g"])
    s = gs[0].copy()
    assert np.array_equal(accs[0].view(np.uint32), s.view(np.uint32))
    s = s + gs[1]
    assert np.array_equal(accs[1].view(np.uint32), s.view(np.uint32))
    s = s + gs[2]
    assert s.dtype == F and np.array_equal(accs[2].view(np.uint32), s.view(np.uint32))
    np.testing.assert_array_equal(accs[2][N:], np.array([sum(rows), 0, 0, 0], F))
    # the closing call's update
    assert _applied(L, hp) == before + 1
    acc2 = torch.from_numpy(accs[2]).to(cuda)
    w2, m2, v2, e2 = [t.clone() for t in start]
    _lib.check(L.qpn_adam_step_avg(hp, w2.data_ptr(), acc2.data_ptr(), m2.data_ptr(), v2.data_ptr(), N, 1, LR, 0.9, 0.999, 1e-8, 0.0,
                                   acc2.data_ptr() + 4 * N, clip, e2.data_ptr(), 0.9, _stream()))
    assert torch.equal(bufs.flat, w2) and torch.equal(bufs.m, m2) and torch.equal(bufs.v, v2) and torch.equal(bufs.ema, e2)
    assert not torch.equal(bufs.flat, start[0]) and not torch.equal(bufs.ema, start[3])
    # losses and the norm
    if mode == 2:
        losses = [o[0] for o in outs]
        assert [o[1] for o in outs] == [1, 1, 1]
        assert outs[0][2] == 0.0 and outs[1][2] == 0.0
        got_norm = outs[2][2]
    else:
        assert outs[0][1] == 0 and outs[1][1] == 1 and outs[2][1] == 1
        assert outs[0][2] == 0.0 and outs[1][2] == 0.0 and outs[2][2] == 0.0          # (the losses these calls returned are micro-step 0's and 1's)
        last, lv, gn, gv = C.c_double(0.0), C.c_int(0), C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_loss_collect(hp, 1, C.byref(last), C.byref(lv)))
        _lib.check(L.qpn_train_grad_norm_lagged(hp, C.byref(gn), C.byref(gv)))
        assert lv.value == 1 and gv.value == 1
        losses = [outs[1][0], outs[2][0], last.value]
        got_norm = gn.value
    for k in range(3):
        print("micro-step %d: loss %.7f oracle %.7f" % (k, losses[k], per[k]["loss"]))
        assert abs(losses[k] - per[k]["loss"]) < 1e-4
    print("norm %.8g, oracle's union gradient %.8g, clip %.4g" % (got_norm, expect, clip))
    np.testing.assert_allclose(got_norm, expect, rtol=1e-5, atol=0)
    assert got_norm > clip
    assert L.qpn_train_status(hp, _stream()) == 0


def test_null_accumulator_with_a_window_of_one_is_the_plain_step(cuda, handle):
    """d_acc = NULL, micro = 0, micro_count = 1 forwards to qpn_train_step_avg: the gradient buffer holds the plain mean-CE gradient (no row weight, the trailer words
    are not written) and one update is applied by the call."""
    L, hp = handle
    w0 = synth.make_weights(TINY, WSEED)
    bufs = _Bufs(cuda, w0)
    bufs.g[N:] = 7.0
    before = _applied(L, hp)
    rc, loss, valid, _ = bufs.call(L, hp, _chunk_np(0), 0, 1, 2, 0.0, 0.0, acc=False)
    assert rc == 0 and valid == 1
    assert _applied(L, hp) == before + 1
    g = bufs.g.cpu().numpy()
    np.testing.assert_array_equal(g[N:], np.full(4, 7.0, F))
    from oracle import train_oracle as TO
    og = _oracle_chunk(w0, 0)
    assert abs(loss - og["loss"]) < 1e-4
    util.assert_grads_match_oracle(TO, TINY, w0, og["caches"], og["dl"], g[:N], og=og["g"])


@pytest.mark.parametrize("want_loss", [True, "lagged", False])
def test_the_trainers_one_call_site_is_the_avg_step(want_loss, cuda, handle, ref):
    """FusedTrainer(max_grad_norm, ema_decay) with accum_steps = 1 steps through qpn_train_step_acc(d_acc = NULL, 0, 1); three steps of it against three calls of
    qpn_train_step_avg over the C ABI from the same weights on the same chunks, clipping at half the first chunk's oracle norm, decay 0.9.
    Two runs of one forward + backward differ in the order of their float atomics (the upsampling bias, the adaptive blocks' scatter; tests/test_train_gpu.py holds
    such runs to 2e-6 on the weights), so the two sequences are compared in two parts.  What a step does with ITS gradient is bit for bit: after every trainer step
    qpn_adam_step_avg -- the Adam launch of qpn_train_step_avg -- on copies of the state the step started from, given the gradient buffer the step left, the step's
    number, clip and decay, yields torch.equal weights, moments and average, and the same norm (the bit pattern of last_grad_norm where the step reports one).
    Across the two runs: step_count and which steps return a loss / a norm are the same; losses and norms agree to 1e-6 relative, weights, moments and average
    to test_train_gpu.py's bounds for two runs of the same steps.  (Measured: the two runs' weights differ by up to 1.5e-8 and are not bit-equal in any of the
    three modes -- nor are two runs of the parent commit's library, profiles/adam_step.txt --, their norms by 1e-11 relative, their losses not at all.)"""
    import torch
    from qpnet_amd.train import FusedTrainer
    L, hp = handle
    w0 = synth.make_weights(TINY, WSEED)
    clip = 0.5 * float(np.sqrt((ref[0]["per"][0]["g"].astype(np.float64) ** 2).sum()))
    mode = 1 if want_loss == "lagged" else (2 if want_loss else 0)
    # the C ABI's sequence
    bufs = _Bufs(cuda, w0)
    c_out = []
    for k in range(3):
        x, h, t, d, b = _chunk_np(k)
        xt, ht, tt, dt = _to(cuda, x, h, t, d)
        B, BL = x.shape[0], int(b[0])
        logits = torch.empty((B, BL, TINY.n_quantize), dtype=torch.float32, device=cuda)
        dlogits = torch.empty_like(logits)
        loss, valid, norm = C.c_double(0.0), C.c_int(0), C.c_double(0.0)
        _lib.check(L.qpn_train_step_avg(hp, bufs.flat.data_ptr(), B, x.shape[1], ht.shape[2], dt.shape[1], BL, int(np.ceil(d).max()), xt.data_ptr(), ht.data_ptr(),
                                        dt.data_ptr(), tt.data_ptr(), tt.shape[1], logits.data_ptr(), dlogits.data_ptr(), bufs.g.data_ptr(), bufs.m.data_ptr(),
                                        bufs.v.data_ptr(), N, k + 1, LR, 0.9, 0.999, 1e-8, 0.0, mode, C.byref(loss), C.byref(valid), clip, C.byref(norm),
                                        bufs.ema.data_ptr(), 0.9, _stream()))
        c_out.append((loss.value if valid.value else None, norm.value if valid.value else None))
    if mode == 1:
        loss, valid, norm, nv = C.c_double(0.0), C.c_int(0), C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_loss_collect(hp, 1, C.byref(loss), C.byref(valid)))
        _lib.check(L.qpn_train_grad_norm_lagged(hp, C.byref(norm), C.byref(nv)))
        assert valid.value == 1 and nv.value == 1
        c_out.append((loss.value, norm.value))
    assert L.qpn_train_status(hp, _stream()) == 0
    # the trainer's
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, max_grad_norm=clip, ema_decay=0.9)
    assert tr.last_grad_norm is None
    t_out = []
    state = [torch.from_numpy(w0.copy()).to(cuda), torch.zeros(N, device=cuda), torch.zeros(N, device=cuda), torch.from_numpy(w0.copy()).to(cuda)]
    for k in range(3):
        loss = tr.step(*_chunk(cuda, k), want_loss=want_loss)
        assert tr.step_count == k + 1 and tr.micro_step == 0 and tr.acc is None
        t_out.append((loss, tr.last_grad_norm))
        # this step's Adam launch, replayed on the state it started from
        _lib.check(L.qpn_adam_step_avg(hp, state[0].data_ptr(), tr.g.data_ptr(), state[1].data_ptr(), state[2].data_ptr(), N, k + 1, LR, 0.9, 0.999, 1e-8, 0.0,
                                       None, clip, state[3].data_ptr(), 0.9, _stream()))
        replay, nv = C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_grad_norm(hp, C.byref(replay), C.byref(nv), _stream()))
        assert nv.value == 1 and replay.value > clip
        for what, a, r in zip(("w", "m", "v", "ema"), (m.flat_parameters(), tr.m, tr.v, tr.ema), state):
            assert torch.equal(a, r), "step %d: %s differs from qpn_adam_step_avg on the step's own gradient" % (k, what)
        if mode == 2:
            assert np.float64(tr.last_grad_norm).tobytes() == np.float64(replay.value).tobytes()
        t_norm_of_step = replay.value
        if mode == 1 and k > 0:
            assert np.float64(tr.last_grad_norm).tobytes() == np.float64(prev_norm).tobytes()      # (the norm that came with the previous step's loss)
        prev_norm = t_norm_of_step
    if mode == 1:
        loss = tr.flush_loss()
        assert np.float64(tr.last_grad_norm).tobytes() == np.float64(prev_norm).tobytes()
        t_out.append((loss, tr.last_grad_norm))
    tr.check_status()
    assert tr.step_count == 3 and tr.state_dict()["state"][0]["step"] == 3
    # the two sequences next to each other
    print("C ABI:", c_out, "\ntrainer:", t_out)
    assert [(o[0] is None, o[1] is None) for o in t_out] == [(o[0] is None, o[1] is None) for o in c_out]
    if mode == 0:
        assert all(o == (None, None) for o in t_out)
    for tv, cv in zip(t_out, c_out):
        for a, r in zip(tv, cv):
            if r is not None:
                np.testing.assert_allclose(a, r, rtol=1e-6, atol=0)
    got = [t.cpu().numpy() for t in (m.flat_parameters(), tr.m, tr.v, tr.ema)]
    want = [t.cpu().numpy() for t in (bufs.flat, bufs.m, bufs.v, bufs.ema)]
    print("bit-equal across the two runs (w, m, v, ema):", [bool(np.array_equal(a, r)) for a, r in zip(got, want)],
          "max |dw| %.2e" % np.abs(got[0] - want[0]).max())
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got[3], want[3], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-5 * np.abs(want[1]).max())
    np.testing.assert_allclose(got[2], want[2], rtol=0, atol=4e-5 * np.abs(want[2]).max())
    assert not np.array_equal(got[0], w0) and not np.array_equal(got[3], w0)


def test_a_flag_of_an_earlier_micro_step_skips_the_closing_update(cuda, handle):
    """the C ABI alone, loss_mode 2 (the status is read, and cleared, in every call): micro-step 0 carries a target equal to n_quantize -- clamped and flagged, the
    call reports QPN_ERANGE -- and a caller that goes on with the window anyway finds the flag in the accumulator's trailer: the closing call applies nothing and
    reports QPN_ERANGE naming an earlier micro-step."""
    import torch
    L, hp = handle
    w0 = synth.make_weights(TINY, WSEED)
    bufs = _Bufs(cuda, w0)
    start = [t.clone() for t in (bufs.flat, bufs.m, bufs.v, bufs.ema)]
    before = _applied(L, hp)
    x, h, t, d, b = _chunk_np(0)
    t = t.copy(); t[0, -5] = TINY.n_quantize
    rc, _, _, _ = bufs.call(L, hp, (x, h, t, d, b), 0, 2, 2, 0.0, 0.9)
    assert rc == ERANGE and b"target class" in L.qpn_last_error()
    assert float(bufs.acc[N + 1]) == 1.0
    rc, _, _, _ = bufs.call(L, hp, _chunk_np(1), 1, 2, 2, 0.0, 0.9)
    assert rc == ERANGE and b"earlier micro-step" in L.qpn_last_error(), L.qpn_last_error()
    np.testing.assert_array_equal(bufs.acc[N:].cpu().numpy()[1:], np.array([1, 0, 0], F))
    assert all(torch.equal(a, b_) for a, b_ in zip((bufs.flat, bufs.m, bufs.v, bufs.ema), start)) and _applied(L, hp) == before
    assert L.qpn_train_status(hp, _stream()) == 0


# ---------------------------------------------------------------- 3. FusedTrainer(accum_steps=2) against the oracle
def _chunk(cuda, ci):
    x, h, t, d, b = _chunk_np(ci)
    return _to(cuda, x, h, t, d, b)


def _check_window_gradients(tr, win):
    """the micro-steps' gradients were checked one by one against their chunks (kept in win["matched"]: the oracle gradients that matched, ReLU sides included);
    here the accumulator divided by its trailer against the union gradient"""
    from oracle import train_oracle as TO
    acc = tr.acc.cpu().numpy()
    rows = [p["rows"] for p in win["per"]]
    np.testing.assert_array_equal(acc[N:], np.array([sum(rows), 0, 0, 0], F))
    un = _union(win["per"], win["matched"]).astype(F)
    util.assert_grads_match_oracle(TO, TINY, win["start"], win["per"][0]["caches"], win["per"][0]["dl"], acc[:N] / acc[N], og=un)


def _run_two_windows(cuda, ref, **kw):
    """two windows of K = 2 through FusedTrainer, held to the oracle: every micro-step's loss (1e-4), the first window's gradients, the final weights"""
    from oracle import train_oracle as TO
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, WSEED)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, accum_steps=2, **kw)
    for w in range(2):
        win = dict(ref[w], matched=[])
        for k in range(2):
            assert tr.micro_step == k
            loss = tr.step(*_chunk(cuda, 2 * w + k), want_loss=True)
            p = win["per"][k]
            print("window %d micro-step %d: loss %.7f oracle %.7f" % (w, k, loss, p["loss"]))
            assert abs(loss - p["loss"]) < 1e-4
            assert tr.last_grad_norm is None and tr.step_count == w + k
            if w == 0:       # (the second window starts from weights an update away from the oracle's: its gradients are held through the final weights)
                g = tr.g.cpu().numpy()
                np.testing.assert_array_equal(g[N:], np.array([p["rows"], 0, 0, 0], F))
                win["matched"].append(util.assert_grads_match_oracle(TO, TINY, win["start"], p["caches"], p["dl"], g[:N] / F(p["rows"]), og=p["g"]))
        assert tr.micro_step == 0
        if w == 0:
            _check_window_gradients(tr, win)
    tr.check_status()
    assert tr.step_count == 2
    w = m.flat_parameters().cpu().numpy()
    print("max |w - oracle| %.3e" % np.abs(w - ref[1]["after"]).max())
    util.assert_weights_after_adam(w, ref[1]["after"], LR, 2)
    np.testing.assert_allclose(w, ref[1]["after"], atol=4e-6, rtol=0)          # (the two-rank test's bound on the same computation)
    return tr, m, w


def test_two_windows_equal_the_union_batch_oracle(cuda, ref):
    """the single-process half of test_two_ranks_on_one_gpu_equal_union_batch_oracle: its chunks, its weights, its oracle (per update the float64 row-weighted mean
    of the two chunk gradients, then TO.Adam), its bounds -- 1e-4 on every loss, 4e-6 on the final weights -- and util.assert_weights_after_adam at lr 1e-4 over the
    two updates.  Both runs start from the same weights and see the same chunks, as in test_world2_without_exchange_equals_world1; the first window's gradients are
    compared at exactly those weights, so no ReLU side is decided by a weight difference.  Two updates, not four: the weights are far from four plain steps'."""
    from qpnet_amd.train import FusedTrainer
    tr, m, w = _run_two_windows(cuda, ref)
    assert tr.state_dict()["state"][0]["step"] == 2
    m4 = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    t4 = FusedTrainer(m4, lr=LR)
    for ci in range(4):
        t4.step(*_chunk(cuda, ci), want_loss=False)
    t4.check_status()
    assert t4.step_count == 4
    far = np.abs(w - m4.flat_parameters().cpu().numpy()).max()
    print("max |w (2 updates of 2 chunks) - w (4 plain steps)| %.3e" % far)
    assert far > 0.5 * LR                                                       # (Adam moves an element by ~lr per update: two updates apart)


# ---------------------------------------------------------------- 4. skip
@pytest.mark.parametrize("want_loss", [True, False])
def test_a_flagged_micro_step_skips_the_window(want_loss, cuda):
    """K = 2, clipping and averaging on.  After one clean window, micro-step 0 of the next gets a target equal to n_quantize (clamped and flagged).
    want_loss=True: the status is read in the step -- it raises QPN_ERANGE at once and the window is abandoned.  want_loss=False: the window runs to its end, the
    closing Adam launch skips on the device and check_status() raises.  Either way weights, moments, average and the applied-update count are those of before,
    micro_step is 0, step_count is the one clean update, and a following clean window applies exactly one more."""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=1e-3, accum_steps=2, max_grad_norm=0.05, ema_decay=0.9)
    L, hp = m._native(cuda)
    for k in range(2):
        tr.step(*_chunk(cuda, k), want_loss=want_loss)
    tr.check_status()
    assert tr.step_count == 1 and tr.micro_step == 0
    state = lambda: (m.flat_parameters(), tr.m, tr.v, tr.ema)
    before, applied = [t.clone() for t in state()], _applied(L, hp)
    xt, ht, tt, dt, bt = _chunk(cuda, 2)
    tt = tt.clone(); tt[0, -3] = TINY.n_quantize
    if want_loss:
        with pytest.raises(_lib.QpnError) as err:
            tr.step(xt, ht, tt, dt, bt, want_loss=True)
    else:
        tr.step(xt, ht, tt, dt, bt, want_loss=False)
        assert tr.micro_step == 1
        tr.step(*_chunk(cuda, 3), want_loss=False)
        assert tr.micro_step == 0
        with pytest.raises(_lib.QpnError) as err:
            tr.check_status()
    assert err.value.code == ERANGE
    assert tr.micro_step == 0 and tr.step_count == 1
    assert all(torch.equal(a, b) for a, b in zip(state(), before)) and _applied(L, hp) == applied
    for k in range(2):
        tr.step(*_chunk(cuda, k), want_loss=want_loss)
        assert tr.micro_step == (k + 1) % 2
    tr.check_status()
    assert _applied(L, hp) == applied + 1 and tr.step_count == 2
    assert not any(torch.equal(a, b) for a, b in zip(state(), before))
    assert bool(torch.isfinite(m.flat_parameters()).all()) and bool(torch.isfinite(tr.ema).all())


# ---------------------------------------------------------------- 5. the trainer's options together
def _omd(decay):
    return F(1.0) - F(decay)


@pytest.mark.parametrize("want_loss", [True, "lagged"])
def test_clipping_and_averaging_act_once_per_window(want_loss, cuda, ref):
    """FusedTrainer(accum_steps=2, max_grad_norm=c, ema_decay=0.9), c = half the first window's norm.  last_grad_norm is None with the loss of a micro-step that does
    not close a window and, with a closing one's, the float64 norm of the oracle's union gradient at the window's starting weights (rtol 1e-5, the bound
    tests/test_grad_clip_gpu.py holds the trainer's norm to against an independent backward).  The average follows the float64 recurrence over the weights after
    each UPDATE, within two fp32 roundings an update (tests/test_ema_gpu.py), and does not move in between; state_dict() counts updates."""
    import torch
    from qpnet_amd.train import FusedTrainer
    decay = 0.9
    w0 = synth.make_weights(TINY, WSEED)
    c = 0.5 * float(np.sqrt((ref[0]["union"] ** 2).sum()))
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, accum_steps=2, max_grad_norm=c, ema_decay=decay)
    lagged = want_loss == "lagged"
    got, expect, snaps = [], [], []
    for w in range(2):
        start = m.flat_parameters().cpu().numpy() if w else w0
        per = ref[0]["per"] if w == 0 else [_oracle_chunk(start, 2 + k) for k in range(2)]
        un = _union(per)
        for k in range(2):
            e_before = tr.ema.clone() if tr.ema is not None else None
            loss = tr.step(*_chunk(cuda, 2 * w + k), want_loss=want_loss)
            got.append((loss, tr.last_grad_norm))
            expect.append((per[k]["loss"], float(np.sqrt((un ** 2).sum())) if k == 1 else None))
            if k == 0 and e_before is not None:
                assert torch.equal(tr.ema, e_before)
        snaps.append(m.flat_parameters().cpu().numpy())
    if lagged:
        assert got[0] == (None, None)
        got = got[1:] + [(tr.flush_loss(), tr.last_grad_norm)]
        assert tr.flush_loss() is None and tr.last_grad_norm is None
    tr.check_status()
    for i, ((loss, norm), (oloss, onorm)) in enumerate(zip(got, expect)):
        print("micro-step %d: loss %.7f (oracle %.7f) norm %s (oracle %s)" % (i, loss, oloss, norm, onorm))
        assert abs(loss - oloss) < 1e-4
        if onorm is None:
            assert norm is None
        else:
            np.testing.assert_allclose(norm, onorm, rtol=1e-5, atol=0)
            assert norm > c
    assert tr.step_count == 2 and tr.micro_step == 0
    sd = tr.state_dict()
    assert all(int(st["step"]) == 2 for st in sd["state"].values()) and len(sd["state"]) == len(list(m.parameters()))
    e = np.asarray(w0, dtype=np.float64).copy()
    for s in snaps:
        e = e + (s.astype(np.float64) - e) * float(_omd(decay))
    tol = 2 * 2 * 2.0 ** -23 * float(np.abs(e).max())
    err = np.abs(tr.ema.cpu().numpy().astype(np.float64) - e).max()
    print("max |e - recurrence over the two updates| %.3e (bound %.3e)" % (err, tol))
    assert err <= tol
    assert np.abs(tr.ema.cpu().numpy() - snaps[-1]).max() > 100 * tol
    # (clipped at half the norm: the first update is not the unclipped one)
    assert np.abs(snaps[0] - ref[0]["after"]).max() > 1e-6


# ---------------------------------------------------------------- 6. the data-parallel shape
def test_world2_exchanges_the_accumulator_once_per_window(cuda, ref, monkeypatch):
    """FusedTrainer(world_size=2, accum_steps=2) without a process group (the exchange is the identity, as in test_world2_without_exchange_equals_world1): the
    call-by-call path.  parallel.exchange is called exactly once per window, on the accumulator; nothing goes out as an early bucket; the results are held to the
    bounds of the single-rank test."""
    from qpnet_amd import parallel
    calls = []
    inner = parallel.exchange

    def counting(buf, group=None):
        calls.append((buf.data_ptr(), buf.numel()))
        return inner(buf, group)

    monkeypatch.setattr(parallel, "exchange", counting)
    tr, m, w = _run_two_windows(cuda, ref, world_size=2)
    assert calls == [(tr.acc.data_ptr(), N + 4)] * 2
    assert tr.last_buckets == (0, 0) and tr._two_buckets is False


def test_capture_with_a_window_is_refused(cuda, monkeypatch):
    """a step on a capturing stream raises before anything is enqueued and leaves the window where it was (the stream's capture state is stood in for: what is
    held is the trainer's refusal, not the runtime's capture)"""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=LR, accum_steps=2)
    chunk = _chunk(cuda, 0)
    maxd = int(torch.max(chunk[3].ceil()))
    tr.step(*chunk, want_loss=False, maxd=maxd)
    assert tr.micro_step == 1
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="accum_steps"):
            tr.step(*chunk, want_loss=False, maxd=maxd)
    assert tr.micro_step == 1
    tr.step(*chunk, want_loss=False, maxd=maxd)
    tr.check_status()
    assert tr.micro_step == 0 and tr.step_count == 1


# ---------------------------------------------------------------- 7. the runner
def _corpus(root):
    """the corpus of tests/test_runners_gpu.py"""
    from qpnet_amd import loaders
    from scipy.io import wavfile
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    rs = np.random.RandomState(5)
    feats = []
    for i in range(3):
        h = synth.make_features(45 + 3 * i, 700 + i)
        wavfile.write("%s/wav/u%02d.wav" % (root, i), 22050, (rs.uniform(-0.8, 0.8, (45 + 3 * i) * TINY.upsampling_factor + 11) * 32767).astype(np.int16))
        np.save("%s/feat/u%02d.npy" % (root, i), h)
        feats.append(h)
    st = loaders.calc_stats(feats)
    np.savez(root + "/stats.npz", mean=st.mean_, scale=st.scale_)
    return root


GEO = ["--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2", "--dilationF_repeat", "1", "--dilationA_depth", "1",
       "--dilationA_repeat", "1", "--feature_format", "npy", "--batch_length", "1500", "--max_length", "4000", "--verbose", "1"]


def test_run_train_counts_updates(cuda, tmp_path, monkeypatch, caplog):
    """run_train --accum_steps 2 --iters 4 --checkpoint_interval 2: eight batches are stepped, checkpoints fall on window boundaries and count updates ("iterations"
    2 and 4, the optimiser's step numbers the same), their keys are today's, the interval's loss is the mean of the micro-step losses; resuming from the
    2-iteration checkpoint steps four more batches and ends at the same "iterations".  --accum_steps 1 is a run without the flag: the same files, and the same
    log up to its timings and the last digits of a loss."""
    import torch
    import yaml
    from qpnet_amd import runners, train
    root = _corpus(str(tmp_path / "corpus"))
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz"]
    steps = []
    inner = train.FusedTrainer.step

    def counting(self, *a, **kw):
        out = inner(self, *a, **kw)
        steps.append((self.micro_step, self.step_count, out))
        return out

    monkeypatch.setattr(train.FusedTrainer, "step", counting)
    flushed = []
    inner_flush = train.FusedTrainer.flush_loss

    def flushing(self):
        flushed.append(inner_flush(self))
        return flushed[-1]

    monkeypatch.setattr(train.FusedTrainer, "flush_loss", flushing)

    def run(exp, extra):
        os.makedirs(exp)
        del steps[:]
        del flushed[:]
        caplog.clear()
        with caplog.at_level(logging.INFO):
            assert runners.run_train(common + GEO + ["--expdir", exp, "--config", exp + "/model.conf", "--iters", "4", "--checkpoint_interval", "2",
                                                     "--intervals", "2"] + extra) == 0
        return list(steps), list(flushed), [r.getMessage() for r in caplog.records if r.name == "root"]

    exp = str(tmp_path / "acc")
    st, fl, log = run(exp, ["--accum_steps", "2", "--resume", exp + "/none.pkl"])
    assert len(st) == 8 and [s[0] for s in st] == [1, 0] * 4 and [s[1] for s in st] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert sorted(f for f in os.listdir(exp) if f.startswith("checkpoint")) == ["checkpoint-2.pkl", "checkpoint-4.pkl", "checkpoint-final.pkl"]
    for it in (2, 4):
        ck = torch.load("%s/checkpoint-%d.pkl" % (exp, it), map_location="cpu", weights_only=False)
        assert list(ck.keys()) == ["model", "optimizer", "iterations"] and ck["iterations"] == it
        assert all(int(s["step"]) == it for s in ck["optimizer"]["state"].values())
    assert list(torch.load(exp + "/checkpoint-final.pkl", map_location="cpu", weights_only=False).keys()) == ["model"]
    rec = yaml.safe_load(open(exp + "/loss-final.yml"))
    assert len(rec) == 2 and all(np.isfinite(rec))
    # lagged losses: step i returns step i - 1's, the interval's last one comes with the flush -- the report of the first interval is the mean of its four micro-steps
    lines = [l for l in log if "average loss" in l]
    assert len(lines) == 2 and lines[0].startswith("(iter:2)") and lines[1].startswith("(iter:4)")
    assert st[0][2] is None and st[4][2] is None and len(fl) == 2
    for k, line in enumerate(lines):
        four = [s[2] for s in st[4 * k + 1:4 * k + 4]] + [fl[k]]
        assert all(v is not None for v in four)
        assert abs(float(re.search(r"average loss = ([0-9.]+)", line).group(1)) - sum(four) / 4) < 1e-6 and abs(rec[k] - sum(four) / 4) < 1e-9
    # resume
    exp2 = str(tmp_path / "resumed")
    st2, _, _ = run(exp2, ["--accum_steps", "2", "--resume", exp + "/checkpoint-2.pkl"])
    assert len(st2) == 4 and [s[1] for s in st2] == [2, 3, 3, 4]
    ck = torch.load(exp2 + "/checkpoint-4.pkl", map_location="cpu", weights_only=False)
    assert ck["iterations"] == 4 and all(int(s["step"]) == 4 for s in ck["optimizer"]["state"].values())
    assert not os.path.exists(exp2 + "/checkpoint-2.pkl")
    # --accum_steps 1 against no flag
    outs = []
    for name, extra in (("one", ["--accum_steps", "1"]), ("plain", [])):
        e = str(tmp_path / name)
        s, _, lg = run(e, extra + ["--resume", e + "/none.pkl"])
        assert len(s) == 4 and [v[0] for v in s] == [0] * 4 and [v[1] for v in s] == [1, 2, 3, 4]
        files = sorted(os.listdir(e))
        cks = {f: torch.load(e + "/" + f, map_location="cpu", weights_only=False) for f in files if f.endswith(".pkl")}
        outs.append((files, cks, [re.sub(r"[0-9]+\.[0-9]+", "#", l).replace(e, "EXP") for l in lg], yaml.safe_load(open(e + "/loss-final.yml"))))
    (f1, c1, l1, r1), (f0, c0, l0, r0) = outs
    assert f1 == f0 and l1 == l0
    np.testing.assert_allclose(r1, r0, rtol=0, atol=1e-5)
    for f in c0:
        assert list(c1[f].keys()) == list(c0[f].keys()) and c1[f].get("iterations") == c0[f].get("iterations")
        a = torch.cat([v.reshape(-1).float() for v in c1[f]["model"].values()]); b = torch.cat([v.reshape(-1).float() for v in c0[f]["model"].values()])
        assert float((a - b).abs().max()) <= 2e-6                              # (two runs of one backward: the bound tests/test_ema_gpu.py holds a resumed run to)
