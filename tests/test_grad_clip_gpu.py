"""GPU: gradient-norm clipping inside the library's optimiser step (qpn_adam_step_clip / qpn_train_step_clip; FusedTrainer / FlatAdam / run_train
`max_grad_norm`) == `torch.nn.utils.clip_grad_norm_(parameters, c)` followed by Adam.step.

Adam's update is nearly invariant to a constant scale of the gradient (tests/test_parallel_gpu.py says so about the row-count scaling): after ONE step from
zero moments a clipped and an unclipped run differ only through eps.  Clipping shows in the moments (m scales with coef, v with coef^2) and in the weights
once clipped and unclipped steps have mixed in the moments -- so every test here checks m and v, and the multi-step ones hold both kinds of step and
assert that the result is far from the unclipped run's."""
import ctypes as C
import logging
import os
import struct

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY
import util

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, STEP = 1e-3, 0.9, 0.999, 1e-8, 1e-3, 3
F = np.float32


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


@pytest.fixture(scope="module")
def handle(cuda):
    """one TINY handle for the C-ABI tests on hand-made buffers (no forward is run on it)"""
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, seed, s=0.01):
    """w, g = N(0,1) * s, non-zero moments (v >= 0)"""
    rs = np.random.RandomState(seed)
    w = (rs.standard_normal(n) * 0.1).astype(F)
    g = (rs.standard_normal(n) * s).astype(F)
    m = (rs.standard_normal(n) * s * 0.3).astype(F)
    v = ((rs.standard_normal(n) * s) ** 2 * 0.5).astype(F)
    return w, g, m, v


def _dev(cuda, arrs, off):
    """device copies; off = 1: every buffer starts one float into its allocation (a base that is not 16-byte aligned)"""
    import torch
    out = []
    for a in arrs:
        t = torch.empty(a.size + off, dtype=torch.float32, device=cuda)
        t[off:].copy_(torch.from_numpy(a))
        out.append(t[off:])
        assert out[-1].data_ptr() % 16 == (4 * off) % 16
    return out


def _clip_call(L, hp, w, g, m, v, n, max_norm, den=None, step=STEP, wd=WD):
    _lib.check(L.qpn_adam_step_clip(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, wd,
                                    den.data_ptr() if den is not None else None, max_norm, _stream()))


def _norm(L, hp):
    norm, valid = C.c_double(-1.0), C.c_int(-1)
    _lib.check(L.qpn_train_grad_norm(hp, C.byref(norm), C.byref(valid), _stream()))
    return norm.value, valid.value


def _applied(L, hp):
    n = C.c_int64(-1)
    _lib.check(L.qpn_train_applied_updates(hp, C.byref(n), _stream()))
    return int(n.value)


def _ref_adam(w, g, m, v, coef, den=None, step=STEP, wd=WD):
    """k_adam's formula restated in numpy fp32 (same operations in the same order), the gradient scaled by `coef` in front of the weight-decay term"""
    b1, b2 = F(B1), F(B2)
    bc1 = F(1.0 - float(b1) ** step)
    bc2s = F(np.sqrt(1.0 - float(b2) ** step))
    gi = g if den is None else g / F(den)
    gi = gi * F(coef)
    gi = gi + F(wd) * w
    mi = m + (gi - m) * (F(1.0) - b1)
    vi = v * b2 + (F(1.0) - b2) * gi * gi
    denom = np.sqrt(vi) / bc2s + F(EPS)
    wi = w - (F(LR) / bc1) * (mi / denom)
    assert wi.dtype == F and mi.dtype == F and vi.dtype == F
    return wi, mi, vi


def _coef(total, max_norm):
    return F(min(1.0, float(F(max_norm)) / (total + 1e-6)))


SIZES = [1, 3, 255, 256, 257, 52591, 504495, 3 * 2 ** 20 + 1]


@pytest.mark.parametrize("n,off", [(n, 0) for n in SIZES] + [(n, 1) for n in SIZES if n >= 257])
def test_clip_step_matches_numpy(n, off, cuda, handle):
    """qpn_adam_step_clip on hand-made buffers against the numpy restatement, clipped (max = 0.5 |g|) and not (max = 2 |g|), without and with a
    denominator buffer {700, 0}; the norm from qpn_train_grad_norm against the fp64 norm.  Bounds: weights atol 2e-6 (test_flat_adam_matches_torch_adam), m
    1e-5 max|m|, v 4e-5 max|v| (test_train_gpu.py's moment comparison).  The norm: rtol 1e-7 (n 2^-53 of accumulation, a square root, one rounding), 1e-6 with the
    denominator's division."""
    import torch
    L, hp = handle
    w0, g0, m0, v0 = _buffers(n, 1000 + n % 977)
    for den in (None, 700.0):
        gin = g0 if den is None else (g0 * F(den)).astype(F)                # the exchanged buffer holds the SUM: den * g
        geff = gin if den is None else gin / F(den)                          # what a den-free run would be given
        total = float(np.sqrt((geff.astype(np.float64) ** 2).sum()))
        total_dev = float(np.sqrt((gin.astype(np.float64) ** 2).sum())) / (den or 1.0)
        assert total > 0
        dden = torch.tensor([den, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda) if den else None
        got = {}
        for kind, max_norm in (("clipped", 0.5 * total), ("free", 2.0 * total)):
            w, g, m, v = _dev(cuda, (w0, gin, m0, v0), off)
            _clip_call(L, hp, w, g, m, v, n, max_norm, dden)
            norm, valid = _norm(L, hp)
            assert valid == 1
            np.testing.assert_allclose(norm, total_dev, rtol=1e-7, atol=0)
            np.testing.assert_allclose(norm, total, rtol=1e-6 if den else 1e-7, atol=0)
            coef = _coef(total, max_norm)
            assert (coef < 0.51) if kind == "clipped" else (coef == 1.0)
            wr, mr, vr = _ref_adam(w0, geff, m0, v0, coef)
            wg, mg, vg = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
            print("n %d off %d den %s %s: norm rel err %.2e, max err w %.2e m %.2e (of max) v %.2e (of max)" % (
                n, off, den, kind, abs(norm - total) / total, np.abs(wg - wr).max(), np.abs(mg - mr).max() / np.abs(mr).max(), np.abs(vg - vr).max() / np.abs(vr).max()))
            np.testing.assert_allclose(wg, wr, rtol=0, atol=2e-6)
            np.testing.assert_allclose(mg, mr, rtol=0, atol=1e-5 * np.abs(mr).max())
            np.testing.assert_allclose(vg, vr, rtol=0, atol=4e-5 * np.abs(vr).max())
            np.testing.assert_array_equal(g.cpu().numpy(), gin)               # the gradient buffer itself is not modified
            got[kind] = mg
        # clipping is visible where it must be: the first moment, by far more than its bound
        assert np.abs(got["clipped"] - got["free"]).max() > 100 * 1e-5 * np.abs(got["free"]).max()


@pytest.mark.parametrize("n", [257, 52591])
def test_off_or_not_binding_leaves_the_bits_of_adam_step_ex(n, cuda, handle):
    """max_grad_norm = 0 is qpn_adam_step_ex; 1e30 clips by coef = 1.0f exactly, and a product with 1.0f is exact: weights and both moments are
    torch.equal to qpn_adam_step_ex's on copies of the same buffers.  With 0 no norm is reported."""
    import torch
    L, hp = handle
    arrs = _buffers(n, 77)
    w, g, m, v = _dev(cuda, arrs, 0)
    _lib.check(L.qpn_adam_step_ex(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, STEP, LR, B1, B2, EPS, WD, None, _stream()))
    for max_norm in (1e30, 0.0):
        w2, g2, m2, v2 = _dev(cuda, arrs, 0)
        _clip_call(L, hp, w2, g2, m2, v2, n, max_norm)
        norm, valid = _norm(L, hp)
        assert valid == (1 if max_norm else 0)
        assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v)
    assert not torch.equal(w, torch.from_numpy(arrs[0]).to(cuda))               # (the step did move them)


@pytest.mark.parametrize("n", [504495, 3 * 2 ** 20 + 1])
def test_norm_and_update_are_bit_identical_from_run_to_run(n, cuda, handle):
    """three calls from identical copies: the norm is the same bit pattern (fixed grid, fixed reduction order, no floating-point atomics) and so are the buffers;
    the same holds from another base alignment (data-parallel ranks hold the same values wherever their allocators put them)."""
    import torch
    L, hp = handle
    arrs = _buffers(n, 5)
    total = float(np.sqrt((arrs[1].astype(np.float64) ** 2).sum()))
    outs = []
    for off in (0, 0, 0, 1):
        w, g, m, v = _dev(cuda, arrs, off)
        _clip_call(L, hp, w, g, m, v, n, 0.5 * total)
        norm, valid = _norm(L, hp)
        assert valid == 1
        outs.append((struct.pack("<d", norm), w, m, v))
    for o in outs[1:]:
        assert o[0] == outs[0][0]
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2]) and torch.equal(o[3], outs[0][3])


def test_non_finite_norm_skips_the_step_and_is_reported(cuda, handle):
    """one inf (then one NaN) in g: weights and both moments untouched, the applied-update counter stays, qpn_train_status returns QPN_ERANGE
    ("non-finite gradient norm"); the next clean call applies.  With max_grad_norm = 0 the same buffer raises no flag, as before.  A zero gradient is an
    ordinary step with coef = 1."""
    import torch
    L, hp = handle
    n = 52591
    arrs = _buffers(n, 31)
    total = float(np.sqrt((arrs[1].astype(np.float64) ** 2).sum()))
    # (the handle's training state exists from the first clipping call on)
    w, g, m, v = _dev(cuda, arrs, 0)
    _clip_call(L, hp, w, g, m, v, n, 0.5 * total)
    assert L.qpn_train_status(hp, _stream()) == 0
    for poison in (np.inf, np.nan):
        w, g, m, v = _dev(cuda, arrs, 0)
        g[n // 3] = poison
        before = _applied(L, hp)
        _clip_call(L, hp, w, g, m, v, n, 0.5 * total)
        norm, valid = _norm(L, hp)
        assert valid == 1 and not np.isfinite(norm)
        for t, a in zip((w, m, v), (arrs[0], arrs[2], arrs[3])):
            assert torch.equal(t, torch.from_numpy(a).to(cuda))
        assert _applied(L, hp) == before
        assert L.qpn_train_status(hp, _stream()) == -4
        assert b"non-finite" in L.qpn_last_error()
        # ... reported once; a clean call behind it applies and counts
        g[n // 3] = 0.0
        _clip_call(L, hp, w, g, m, v, n, 0.5 * total)
        assert _applied(L, hp) == before + 1
        assert not torch.equal(w, torch.from_numpy(arrs[0]).to(cuda))
        assert L.qpn_train_status(hp, _stream()) == 0
        # clipping off: the poisoned buffer is stepped as it always was, and nothing is flagged
        g[n // 3] = poison
        _clip_call(L, hp, w, g, m, v, n, 0.0)
        assert L.qpn_train_status(hp, _stream()) == 0
        assert _applied(L, hp) == before + 2
    # total = 0: coef = min(1, max / 1e-6) = 1
    w, g, m, v = _dev(cuda, (arrs[0], np.zeros(n, F), arrs[2], arrs[3]), 0)
    w2, g2, m2, v2 = _dev(cuda, (arrs[0], np.zeros(n, F), arrs[2], arrs[3]), 0)
    before = _applied(L, hp)
    _clip_call(L, hp, w, g, m, v, n, 0.25)
    norm, valid = _norm(L, hp)
    assert valid == 1 and norm == 0.0
    _lib.check(L.qpn_adam_step_ex(hp, w2.data_ptr(), g2.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, STEP, LR, B1, B2, EPS, WD, None, _stream()))
    assert _applied(L, hp) == before + 2 and L.qpn_train_status(hp, _stream()) == 0
    assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2)


# ---------------------------------------------------------------- through the trainers
# chunks whose gradient norms at synth.make_weights(TINY, 12) are, in this order, low / high / middle / high / low (found with the numpy oracle, oracle/train_oracle.py:
# five plain Adam steps at lr 1e-3 give norms 0.0905, 0.1571, 0.1149, 0.1665, 0.0846 -- 0.79, 1.37, 1, 1.45, 0.74 of their median; with weight_decay 1e-3
# 0.0905, 0.1563, 0.1138, 0.1655, 0.0819 -- 0.795, 1.37, 1, 1.45, 0.72)
CHUNKS = [(144, 676), (383, 631), (12, 640), (295, 607), (378, 648)]
WSEED = 12


def _chunk(cuda, k):
    seed, bl = CHUNKS[k]
    x, h, t, d, b = synth.train_inputs(TINY, bl, seed, 30000)
    return _to(cuda, x, h, t, d, b)


def _torch_loop(cuda, monkeypatch, nsteps, clip, lr=1e-3, wd=0.0):
    """the reference-side loop on the drop-in module, torch's own Adam (step hooks off): -> norms (clip_grad_norm_'s return values), flat weights, flat m, flat v"""
    import torch
    monkeypatch.setenv("QPN_DROPIN_FUSED_ADAM", "0")
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=wd)
    norms = []
    for k in range(nsteps):
        xt, ht, tt, dt, bt = _chunk(cuda, k)
        out = m(xt, ht, dt, bt)
        loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, TINY.n_quantize), tt[:, -out.shape[1]:].reshape(-1))
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), clip if clip is not None else 1e30)))
        opt.step()
    assert not opt.__dict__.get("_qpn_adopt")
    ps = list(m.parameters())
    cat = lambda key: torch.cat([opt.state[p][key].reshape(-1) for p in ps]).cpu().numpy()
    return norms, torch.cat([p.detach().reshape(-1) for p in ps]).cpu().numpy(), cat("exp_avg"), cat("exp_avg_sq"), [p.numel() for p in ps]


def _fused_run(cuda, nsteps, clip, lr=1e-3, wd=0.0, **kw):
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=lr, weight_decay=wd, max_grad_norm=clip, **kw)
    norms, losses = [], []
    for k in range(nsteps):
        losses.append(tr.step(*_chunk(cuda, k), want_loss=True))
        norms.append(tr.last_grad_norm)
    tr.check_status()
    return tr, m, norms, losses


# The five-step comparison against torch runs with the optimiser settings of the comparison its weight bound comes from (tests/test_train_gpu.py,
# test_stock_adam_stepped_by_the_library_equals_torchs_own: lr 1e-3, weight_decay 1e-3, atol 2e-6).  Weight decay is part of what that bound rests on: it keeps every
# element's effective gradient (g + wd w ~ 1e-4) far above Adam's eps = 1e-8.  Without it the bound is not reachable on these chunks by ANY pair of backward
# implementations, clipping or no clipping: the first chunk's gradient of auxF_1x1_sigmoid.1.weight[...] (flat element 26447) is 5.95e-9, next to eps, where the first
# update lr g / (|g| + eps) moves by lr eps / (|g| + eps)^2 = 4e4 per unit of gradient -- at that slope a difference of 7e-11 (1e-7 of that tensor's largest gradient: fp32 reassociation) between
# the one-call step's backward and the module's autograd backward is all that 2.85e-6 of weight takes (computed from the slope, not read off the device).  Measured on an MI355X, five steps at lr 1e-3, max |dw| torch loop
# against FusedTrainer: 2.85e-6 clipped and 2.88e-6 UNCLIPPED with weight_decay 0 (the same element; each side repeats itself to 1.3e-7), 1.07e-6 clipped with
# weight_decay 1e-3.  With weight decay the comparison also holds the order "clip, then weight decay" against torch's own, which the C-ABI test holds against numpy only.
WD5 = 1e-3


@pytest.fixture(scope="module")
def clip_level(cuda):
    """c = the median of the five unclipped norms of the torch loop (computed once, shared)"""
    mp = pytest.MonkeyPatch()
    try:
        norms = _torch_loop(cuda, mp, 5, None, wd=WD5)[0]
    finally:
        mp.undo()
    c = float(np.median(norms))
    print("unclipped norms", norms, "c", c)
    assert sum(v > 1.2 * c for v in norms) >= 2 and sum(v < 0.8 * c for v in norms) >= 2, norms
    return c


def test_fused_trainer_clips_like_clip_grad_norm_then_adam(cuda, monkeypatch, clip_level):
    """FusedTrainer(max_grad_norm=c), five steps at lr 1e-3 (weight_decay 1e-3: see WD5), against clip_grad_norm_(c) + torch.optim.Adam on the drop-in module: weights atol 2e-6 and moments 1e-5 / 4e-5
    of the tensor's largest (the bounds of test_stock_adam_stepped_by_the_library_equals_torchs_own), every step's last_grad_norm against clip_grad_norm_'s return
    value at rtol 1e-5 (two runs of one backward differ by float-atomics order, ~1e-6 of the largest gradient) -- and far from the unclipped run."""
    c = clip_level
    tnorms, tw, tm, tv, sizes = _torch_loop(cuda, monkeypatch, 5, c, wd=WD5)
    tr, m, norms, losses = _fused_run(cuda, 5, c, wd=WD5)
    assert tr.step_count == 5 and all(np.isfinite(losses))
    print("torch norms", tnorms, "fused norms", norms)
    np.testing.assert_allclose(norms, tnorms, rtol=1e-5, atol=0)
    w = m.flat_parameters().cpu().numpy()
    fm, fv = tr.m.cpu().numpy(), tr.v.cpu().numpy()
    print("max |dw| %.3e" % np.abs(w - tw).max())
    np.testing.assert_allclose(w, tw, rtol=0, atol=2e-6)
    o = 0
    for n in sizes:
        for a, b, f in ((tm[o:o + n], fm[o:o + n], 1e-5), (tv[o:o + n], fv[o:o + n], 4e-5)):
            np.testing.assert_allclose(b, a, rtol=0, atol=f * max(float(np.abs(a).max()), 1e-30))
        o += n
    tr0, m0, norms0, _ = _fused_run(cuda, 5, None, wd=WD5)
    assert norms0 == [None] * 5 and tr0.last_grad_norm is None
    w0 = m0.flat_parameters().cpu().numpy()
    print("clipped vs unclipped max |dw| %.3e" % np.abs(w - w0).max())
    assert np.abs(w - w0).max() > 1e-5
    assert np.abs(fm - tr0.m.cpu().numpy()).max() > 100 * 1e-5 * np.abs(fm).max()


def test_grad_norm_is_delivered_with_its_loss_in_every_loss_mode(cuda, clip_level):
    """two steps per want_loss mode: "lagged" returns step 1's pair at step 2 and step 2's at flush_loss(); True returns each step's own; False none."""
    from qpnet_amd.train import FusedTrainer
    c = clip_level
    _, _, ref_norms, ref_losses = _fused_run(cuda, 2, c)
    assert all(v is not None and v > 0 for v in ref_norms)
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=1e-3, max_grad_norm=c)
    assert tr.step(*_chunk(cuda, 0), want_loss="lagged") is None and tr.last_grad_norm is None
    l1 = tr.step(*_chunk(cuda, 1), want_loss="lagged"); n1 = tr.last_grad_norm
    l2 = tr.flush_loss(); n2 = tr.last_grad_norm
    assert tr.flush_loss() is None and tr.last_grad_norm is None
    tr.check_status()
    np.testing.assert_allclose([l1, l2], ref_losses, rtol=0, atol=1e-6)
    np.testing.assert_allclose([n1, n2], ref_norms, rtol=1e-5, atol=0)
    assert abs(n1 - n2) > 1e-3 * n1                                        # (the two chunks' norms are far apart: a norm delivered a step off would show)
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=1e-3, max_grad_norm=c)
    for k in range(2):
        assert tr.step(*_chunk(cuda, k), want_loss=False) is None and tr.last_grad_norm is None
    tr.check_status()
    assert tr.step_count == 2


def _chunk2(cuda, k):      # B = 2, one short chunk (seeds whose two rows share a batch length)
    return _to(cuda, *synth.train_inputs(TINY, 400, (91, 100)[k], 30000, batch_size=2))


def _two_lagged_steps(cuda, c, second_by_calls):
    """one handle, clipping on: a one-call step in lagged mode, then one more -- one call again, or made call by call over the C ABI (FusedTrainer._step_calls) --, then
    flush_loss(): -> what the second step and the flush returned, [(loss, norm), (loss, norm)]"""
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    tr = FusedTrainer(m, lr=1e-3, max_grad_norm=c)
    assert tr.step(*_chunk2(cuda, 0), want_loss="lagged") is None and tr.last_grad_norm is None
    if second_by_calls:      # (the path a data-parallel or capturing trainer takes: the same arguments, one C-ABI call per piece)
        tr._step_call = lambda L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, loss: \
            tr._step_calls(L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, False, False, loss)
    l1 = tr.step(*_chunk2(cuda, 1), want_loss="lagged")
    n1 = tr.last_grad_norm
    l2 = tr.flush_loss(); n2 = tr.last_grad_norm
    assert tr.flush_loss() is None and tr.last_grad_norm is None
    tr.check_status()
    assert tr.step_count == 2
    return [(l1, n1), (l2, n2)]


def test_one_call_step_and_call_by_call_step_share_the_report_slots(cuda, clip_level):
    """The one-call step's last kernel and the copies of qpn_train_loss_enqueue / qpn_train_status_enqueue write ONE pair of pinned slots (train_report.h): a lagged
    one-call step followed by a lagged step made call by call returns the first step's loss and norm at the second step and the second's at flush_loss(), the values
    two one-call steps return (losses atol 1e-6, norms rtol 1e-5: the bounds of test_grad_norm_is_delivered_with_its_loss_in_every_loss_mode, float-atomics order)."""
    c = clip_level
    ref = _two_lagged_steps(cuda, c, False)
    got = _two_lagged_steps(cuda, c, True)
    print("one call + one call", ref, "one call + call by call", got)
    assert all(v is not None for pair in ref + got for v in pair)
    np.testing.assert_allclose([p[0] for p in got], [p[0] for p in ref], rtol=0, atol=1e-6)
    np.testing.assert_allclose([p[1] for p in got], [p[1] for p in ref], rtol=1e-5, atol=0)
    assert abs(ref[0][0] - ref[1][0]) > 1e-5 and abs(ref[0][1] - ref[1][1]) > 1e-4 * ref[0][1]      # (the two steps' values lie ten bounds apart: a pair delivered a step off, or a loss with the other step's norm, would show)


def test_world2_with_the_identity_exchange_clips_like_world1(cuda):
    """No process group: world_size=2 holds n_r g_r | n_r and divides by n_r on the device, so the clipped step must reproduce world_size=1's (the norm is that of the AVERAGED
    gradient).  The per-step weight re-sync and the bounds are test_world2_without_exchange_equals_world1's; the norms agree to rtol 1e-6 (the denominator's division)."""
    import torch
    from qpnet_amd.train import FusedTrainer
    c = 0.12                    # between the chunks' norms (0.09, 0.157, 0.115 at these weights)
    flat = synth.make_weights(TINY, WSEED)
    m1 = util.build_model(TINY, flat, cuda).train()
    m2 = util.build_model(TINY, flat, cuda).train()
    t1 = FusedTrainer(m1, lr=1e-4, world_size=1, max_grad_norm=c)
    t2 = FusedTrainer(m2, lr=1e-4, world_size=2, max_grad_norm=c)
    norms = []
    for step in range(3):
        xt, ht, tt, dt, bt = _chunk(cuda, step)
        if step:
            assert float((m2.flat_parameters() - m1.flat_parameters()).abs().max()) <= 2e-7
            with torch.no_grad():
                m2._flat.copy_(m1._flat)
        l1 = t1.step(xt, ht, tt, dt, bt)
        l2 = t2.step(xt, ht, tt, dt, bt)
        assert abs(l1 - l2) < 1e-6
        norms.append(t1.last_grad_norm)
        # (two runs of one backward differ by float-atomics order, ~1e-6 of the largest gradient: the norm of n g / n against that of g)
        np.testing.assert_allclose(t2.last_grad_norm, t1.last_grad_norm, rtol=1e-6, atol=0)
        mm1 = t1.m.cpu().numpy().astype(np.float64); mm2 = t2.m.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(mm2, mm1, rtol=0, atol=2e-6 * np.abs(mm1).max())
        vv1 = t1.v.cpu().numpy().astype(np.float64); vv2 = t2.v.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(vv2, vv1, rtol=0, atol=4e-6 * np.abs(vv1).max())
    print("norms", norms)
    assert max(norms) > 1.2 * c and min(norms) < 0.85 * c                 # both kinds of step
    np.testing.assert_allclose(m2.flat_parameters().cpu().numpy(), m1.flat_parameters().cpu().numpy(), atol=2e-7, rtol=0)
    # ... and the clipped first moment is far from an unclipped trainer's
    t0 = FusedTrainer(util.build_model(TINY, flat, cuda).train(), lr=1e-4, world_size=2)
    for step in range(3):
        t0.step(*_chunk(cuda, step))
    assert t0.last_grad_norm is None
    assert np.abs(t0.m.cpu().numpy() - t2.m.cpu().numpy()).max() > 100 * 2e-6 * np.abs(t0.m.cpu().numpy()).max()


def test_flat_adam_clips_like_clip_grad_norm_then_adam(cuda, monkeypatch):
    """FlatAdam(max_grad_norm=c) in the reference-style loop == clip_grad_norm_(c) + torch.optim.Adam over three steps (atol 2e-6); an inf in a .grad leaves the parameters
    alone, raises QpnError(-4) at the next status collection and leaves the optimiser usable."""
    import torch
    from qpnet_amd.train import FlatAdam
    c = 0.12
    tnorms, tw, tm, tv, _ = _torch_loop(cuda, monkeypatch, 3, c)
    assert max(tnorms) > 1.2 * c and min(tnorms) < 0.85 * c
    m = util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()
    opt = FlatAdam(m, lr=1e-3, max_grad_norm=c)

    def backward(k):
        xt, ht, tt, dt, bt = _chunk(cuda, k)
        out = m(xt, ht, dt, bt)
        loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, TINY.n_quantize), tt[:, -out.shape[1]:].reshape(-1))
        opt.zero_grad()
        loss.backward()
    for k in range(3):
        backward(k)
        opt.step()
    m.check_status()
    w = m.flat_parameters().cpu().numpy()
    print("max |dw| %.3e" % np.abs(w - tw).max())
    np.testing.assert_allclose(w, tw, rtol=0, atol=2e-6)
    np.testing.assert_allclose(opt._m.cpu().numpy(), tm, rtol=0, atol=1e-5 * np.abs(tm).max())
    np.testing.assert_allclose(opt._v.cpu().numpy(), tv, rtol=0, atol=4e-5 * np.abs(tv).max())
    # a non-finite gradient
    backward(3)
    before = m.flat_parameters().clone()
    list(m.parameters())[5].grad.view(-1)[0] = float("inf")
    opt.step()
    assert torch.equal(m.flat_parameters(), before)
    with pytest.raises(_lib.QpnError) as e:
        m.check_status()
    assert e.value.code == -4 and "non-finite" in str(e.value)
    assert torch.equal(m.flat_parameters(), before)
    backward(4)
    opt.step()
    m.check_status()
    assert opt._steps == 4 and not torch.equal(m.flat_parameters(), before)      # (the skipped step does not count: the bias correction goes on from 3 applied updates)


def test_run_train_reports_the_norm_and_clips(cuda, tmp_path, caplog):
    """run_train --max_grad_norm below the run's norms: it finishes, every report line carries the interval's largest norm and a non-zero clipped count, and the
    final checkpoint differs from the same run without the flag (whose report lines are what they always were)."""
    import torch
    from qpnet_amd import loaders, runners
    from scipy.io import wavfile
    # (the corpus and geometry of tests/test_runners_gpu.py's smallest case)
    root = str(tmp_path / "corpus")
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
    geo = ["--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2", "--dilationF_repeat", "1", "--dilationA_depth", "1",
           "--dilationA_repeat", "1", "--feature_format", "npy", "--batch_length", "1500", "--max_length", "4000", "--verbose", "1"]
    finals, lines = [], []
    for tag, extra in (("clip", ["--max_grad_norm", "0.01"]), ("plain", [])):
        exp = str(tmp_path / tag)
        os.makedirs(exp)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            args = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz"] + geo + \
                   ["--expdir", exp, "--config", exp + "/model.conf", "--iters", "4", "--checkpoint_interval", "100", "--intervals", "2", "--resume", exp + "/none.pkl"] + extra
            assert runners.run_train(args) == 0
        lines.append([r.getMessage() for r in caplog.records if "average loss" in r.getMessage()])
        sd = torch.load(exp + "/checkpoint-final.pkl", map_location="cpu")["model"]
        finals.append(torch.cat([v.reshape(-1).float() for v in sd.values()]))
    assert len(lines[0]) == 2 and len(lines[1]) == 2
    for ln in lines[0]:
        assert "max grad norm = " in ln and "2 of 2 steps clipped" in ln, ln
        assert float(ln.split("max grad norm = ")[1].split(",")[0]) > 0.01
    for ln in lines[1]:
        assert "grad norm" not in ln and ln.endswith("sec / batch)"), ln
    assert float((finals[0] - finals[1]).abs().max()) > 1e-5
