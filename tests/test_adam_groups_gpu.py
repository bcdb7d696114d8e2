"""GPU: parameter groups inside the fused Adam launch (qpn_adam_groups; FlatAdam(params=...), FusedTrainer(param_groups=...), run_update --freeze).

The C-ABI tests run on hand-made buffers on a TINY handle, as tests/test_grad_clip_gpu.py's do, against k_adam's formula restated in numpy fp32 with
per-element lr / weight_decay arrays: the library is built with -ffp-contract=off, so the restatement is bit-exact and every comparison of weights, moments and
averaged weights is array_equal.  The norm of a clipped grouped launch is compared, bit for bit, with the norm qpn_adam_step_clip reports for the same
gradient with its frozen elements set to +0."""
import ctypes as C

import numpy as np
import pytest

from qpnet_amd import _lib, loaders, synth
from qpnet_amd.config import TINY, ADAM_FROZEN
import util

pytestmark = pytest.mark.gpu

B1, B2, EPS, STEP, DECAY = 0.9, 0.999, 1e-8, 3, 0.99
F = np.float32
FR = ADAM_FROZEN
LRS, WDS = [1e-3, 3e-4, 2e-2], [0.0, 1e-2, 1e-3]          # three groups with distinct (lr, wd)
CALL_LR, CALL_WD = 7e-2, 0.3                              # the launch's own two values: ignored while groups are on (far from every group's)


def _edge_table():
    """n = 5003: one-element segments, ends on and next to wave and block boundaries, block 2 (512..768) frozen, a one-element run 1030..1040 that
    alternates groups, a frozen last segment"""
    ends = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 768, 1024, 1030] + list(range(1031, 1041)) + [4096, 5003]
    groups = []
    for s, e in enumerate(ends):
        groups.append(FR if e in (768, 5003, 64) else (s % 2 if 1030 < e <= 1040 else s % 3))
    return ends, groups


def _front_table():
    """the first segment frozen and spanning block 0"""
    return [300, 1000, 2600, 5003], [FR, 1, 0, 2]


TABLES = {"edge": _edge_table(), "front": _front_table()}
N = 5003


def _per_elem(ends, groups):
    q = np.repeat(np.array(groups), np.diff([0] + list(ends)))
    lr = np.array(LRS + [0.0], F)[q]          # (index -1: the frozen elements' entry, never used)
    wd = np.array(WDS + [0.0], F)[q]
    return q, lr, wd


@pytest.fixture(scope="module")
def handle(cuda):
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _set(L, hp, ends, groups, lrs=LRS, wds=WDS):
    n = len(lrs)
    _lib.check(L.qpn_adam_groups(hp, n, (C.c_float * n)(*lrs), (C.c_float * n)(*wds), len(ends), (C.c_int64 * len(ends))(*ends),
                                 (C.c_int32 * len(groups))(*groups), _stream()))


def _off(L, hp):
    _lib.check(L.qpn_adam_groups(hp, 0, None, None, 0, None, None, None))


@pytest.fixture(scope="module")
def arrs():
    """w, g, m (non-zero), v (>= 0), e: made once, never written"""
    rs = np.random.RandomState(77)
    n = 52591
    out = ((rs.standard_normal(n) * 0.1).astype(F), (rs.standard_normal(n) * 0.01).astype(F), (rs.standard_normal(n) * 0.003).astype(F),
           ((rs.standard_normal(n) * 0.01) ** 2 * 0.5).astype(F), (rs.standard_normal(n) * 0.1).astype(F))
    for a in out:
        a.setflags(write=False)
    return out


def _dev(cuda, arrays, off=0):
    """device copies; off = 1: every buffer starts one float into its allocation"""
    import torch
    out = []
    for a in arrays:
        t = torch.empty(a.size + off, dtype=torch.float32, device=cuda)
        t[off:].copy_(torch.from_numpy(np.array(a)))
        out.append(t[off:])
    return out


def _call(L, hp, w, g, m, v, n, lr=CALL_LR, wd=CALL_WD, den=None, max_norm=0.0, e=None, expect=0):
    rc = L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, STEP, lr, B1, B2, EPS, wd,
                             den.data_ptr() if den is not None else None, max_norm, e.data_ptr() if e is not None else None, DECAY if e is not None else 0.0, _stream())
    assert rc == expect, (rc, L.qpn_last_error())


def _norm(L, hp):
    norm, valid = C.c_double(-1.0), C.c_int(-1)
    _lib.check(L.qpn_train_grad_norm(hp, C.byref(norm), C.byref(valid), _stream()))
    assert valid.value == 1
    return norm.value


def _applied(L, hp):
    n = C.c_int64(-1)
    _lib.check(L.qpn_train_applied_updates(hp, C.byref(n), _stream()))
    return int(n.value)


def _ref_adam(w, g, m, v, lr, wd, coef=1.0, den=None, step=STEP):
    """tests/test_grad_clip_gpu.py's _ref_adam with per-element lr / wd arrays (fp32): k_adam's operations in k_adam's order"""
    b1, b2 = F(B1), F(B2)
    bc1 = F(1.0 - float(b1) ** step)
    bc2s = F(np.sqrt(1.0 - float(b2) ** step))
    gi = g if den is None else g / F(den)
    gi = gi * F(coef)
    gi = gi + wd * w
    mi = m + (gi - m) * (F(1.0) - b1)
    vi = v * b2 + (F(1.0) - b2) * gi * gi
    denom = np.sqrt(vi) / bc2s + F(EPS)
    wi = w - (lr / bc1) * (mi / denom)
    assert wi.dtype == F and mi.dtype == F and vi.dtype == F
    return wi, mi, vi


def _coef(total, max_norm):
    c = float(F(max_norm)) / (total + 1e-6)
    return F(c) if c < 1.0 else F(1.0)


def _expected(w0, g0, m0, v0, e0, q, lr, wd, coef=1.0, den=None, ema=False):
    """the grouped launch restated: the update where q >= 0, the inputs where frozen; the average moves everywhere"""
    tr = q >= 0
    wr, mr, vr = _ref_adam(w0, g0, m0, v0, lr, wd, coef, den)
    wr, mr, vr = np.where(tr, wr, w0), np.where(tr, mr, m0), np.where(tr, vr, v0)
    er = e0 + (wr - e0) * (F(1.0) - F(DECAY)) if ema else e0
    return wr, mr, vr, er


def _zeroed_norm(L, hp, cuda, w0, g0, m0, v0, q, den, max_norm, ends, groups):
    """the norm the launch WITHOUT groups reports for the gradient with its frozen elements set to +0 (on scratch copies); the groups are put back afterwards"""
    _off(L, hp)
    gz = np.where(q >= 0, g0, F(0.0)).astype(F)
    w, g, m, v = _dev(cuda, (w0, gz, m0, v0))
    _call(L, hp, w, g, m, v, w0.size, den=den, max_norm=max_norm)
    norm = _norm(L, hp)
    _set(L, hp, ends, groups)
    return norm


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("table", ["edge", "front"])
def test_grouped_launch_matches_numpy_on_the_edge_tables(table, off, cuda, handle, arrs):
    """1: plain, clipped (0.5 |g| and 2 |g|), with the data-parallel denominator, with averaging -- w, m, v, e bit for bit; frozen elements untouched; the norm
    that of the zeroed gradient; one applied update per call"""
    import torch
    L, hp = handle
    ends, groups = TABLES[table]
    assert ends[-1] == N and groups[-1 if table == "edge" else 0] == FR
    q, lr, wd = _per_elem(ends, groups)
    assert (q[512:768] == FR).all() if table == "edge" else (q[:300] == FR).all()
    assert set(q.tolist()) == {FR, 0, 1, 2}
    w0, g0, m0, v0, e0 = (a[:N] for a in arrs)
    gnorm = float(np.sqrt((np.where(q >= 0, g0, 0).astype(np.float64) ** 2).sum()))
    _set(L, hp, ends, groups)
    try:
        # (the clipped call first: it creates the handle's training state, where the applied-update count lives)
        variants = [("clipped", None, 0.5 * gnorm, False), ("plain", None, 0.0, False), ("free", None, 2.0 * gnorm, False), ("den", 700.0, 0.0, False),
                    ("den-clipped", 700.0, 0.5 * gnorm, False), ("avg", None, 0.0, True), ("avg-clipped", None, 0.5 * gnorm, True)]
        for name, den, max_norm, ema in variants:
            gin = g0 if den is None else (g0 * F(den)).astype(F)
            geff = gin
            dden = torch.tensor([den, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda) if den else None
            coef = 1.0
            w, g, m, v, e = _dev(cuda, (w0, gin, m0, v0, e0), off)
            before = _applied(L, hp)
            _call(L, hp, w, g, m, v, N, den=dden, max_norm=max_norm, e=e if ema else None)
            assert _applied(L, hp) == before + 1, name
            if max_norm > 0.0:
                norm = _norm(L, hp)
                np.testing.assert_allclose(norm, gnorm, rtol=1e-6)                       # (the norm of the trainable elements ...)
                assert norm == _zeroed_norm(L, hp, cuda, w0, gin, m0, v0, q, dden, max_norm, ends, groups), name      # ... bit for bit the zeroed gradient's
                coef = _coef(norm, max_norm)
                assert (coef < 0.51) if "clipped" in name else (coef == 1.0)
            wr, mr, vr, er = _expected(w0, geff, m0, v0, e0, q, lr, wd, coef, den, ema)
            got = [t.cpu().numpy() for t in (w, m, v, e)]
            for what, a, r, inp in zip("wmve", got, (wr, mr, vr, er), (w0, m0, v0, e0)):
                assert np.array_equal(a, r), "%s %s: %d elements differ, first at %d" % (name, what, (a != r).sum(), int(np.argmax(a != r)))
                if what != "e":
                    assert np.array_equal(a[q < 0], inp[q < 0]) and (a[q >= 0] != inp[q >= 0]).mean() > 0.99, (name, what)
            assert np.array_equal(g.cpu().numpy(), gin)
            if ema:
                assert (got[3] != e0).mean() > 0.99                                          # the average moves on frozen elements too
    finally:
        _off(L, hp)


@pytest.mark.parametrize("clip", [False, True])
def test_grouped_result_is_the_ungrouped_launches_stitched(clip, cuda, handle, arrs):
    """2: segment by segment the grouped result equals today's launch run once per group, on fresh copies, with that group's (lr, wd)"""
    import torch
    L, hp = handle
    ends, groups = TABLES["edge"]
    q, _, _ = _per_elem(ends, groups)
    w0, g0, m0, v0, e0 = (a[:N] for a in arrs)
    gz = np.where(q >= 0, g0, F(0.0)).astype(F)          # (clipping: the ungrouped launch must see the grouped launch's norm)
    max_norm = 0.5 * float(np.sqrt((gz.astype(np.float64) ** 2).sum())) if clip else 0.0
    dden = torch.tensor([3.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda)
    _off(L, hp)
    per_group = []
    for k in range(3):
        w, g, m, v, e = _dev(cuda, (w0, gz, m0, v0, e0))
        _call(L, hp, w, g, m, v, N, lr=LRS[k], wd=WDS[k], den=dden, max_norm=max_norm, e=e)
        per_group.append([t.cpu().numpy() for t in (w, m, v, e)])
    _set(L, hp, ends, groups)
    try:
        w, g, m, v, e = _dev(cuda, (w0, g0, m0, v0, e0))
        _call(L, hp, w, g, m, v, N, den=dden, max_norm=max_norm, e=e)
        got = [t.cpu().numpy() for t in (w, m, v, e)]
    finally:
        _off(L, hp)
    lo = 0
    for hi, k in zip(ends, groups):
        for i, inp in enumerate((w0, m0, v0)):
            want = inp[lo:hi] if k == FR else per_group[k][i][lo:hi]
            assert np.array_equal(got[i][lo:hi], want), (lo, hi, k, "wmv"[i])
        if k != FR:
            assert np.array_equal(got[3][lo:hi], per_group[k][3][lo:hi]), (lo, hi, k, "e")
        lo = hi


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 52591])
def test_one_group_with_the_calls_own_values_is_the_ungrouped_launch(n, cuda, handle, arrs):
    """3: one group over [0, n) -- plain, and clipped with averaging"""
    import torch
    L, hp = handle
    a = [x[:n] for x in arrs]
    gn = float(np.sqrt((a[1].astype(np.float64) ** 2).sum()))
    for max_norm, ema in ((0.0, False), (0.5 * gn, True)):
        _off(L, hp)
        w, g, m, v, e = _dev(cuda, a)
        _call(L, hp, w, g, m, v, n, lr=LRS[1], wd=WDS[1], max_norm=max_norm, e=e if ema else None)
        norm = _norm(L, hp) if max_norm else None
        _set(L, hp, [n], [0], [LRS[1]], [WDS[1]])
        try:
            w2, g2, m2, v2, e2 = _dev(cuda, a)
            _call(L, hp, w2, g2, m2, v2, n, lr=LRS[1], wd=WDS[1], max_norm=max_norm, e=e2 if ema else None)
            assert norm is None or _norm(L, hp) == norm
        finally:
            _off(L, hp)
        assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2) and torch.equal(e, e2)
        assert not torch.equal(w, torch.from_numpy(np.array(a[0])).to(cuda))


def test_non_finite_gradients(cuda, handle, arrs):
    """4: an inf in a frozen element's gradient is not seen (the clipped step is applied, the norm is finite); in a trainable element it skips the step: nothing
    written, the applied-update count stays, the next status report is QPN_ERANGE"""
    import torch
    L, hp = handle
    ends, groups = TABLES["edge"]
    q, lr, wd = _per_elem(ends, groups)
    w0, g0, m0, v0, e0 = (a[:N] for a in arrs)
    gnorm = float(np.sqrt((np.where(q >= 0, g0, 0).astype(np.float64) ** 2).sum()))
    _set(L, hp, ends, groups)
    try:
        assert q[600] == FR and q[5002] == FR and q[700] == FR
        gin = g0.copy(); gin[600] = np.inf; gin[5002] = np.nan; gin[700] = -np.inf
        w, g, m, v = _dev(cuda, (w0, gin, m0, v0))
        before = _applied(L, hp)
        _call(L, hp, w, g, m, v, N, max_norm=0.5 * gnorm)
        norm = _norm(L, hp)
        assert np.isfinite(norm) and abs(norm - gnorm) <= 1e-6 * gnorm
        assert _applied(L, hp) == before + 1 and L.qpn_train_status(hp, _stream()) == 0
        wr, mr, vr, _ = _expected(w0, g0, m0, v0, e0, q, lr, wd, _coef(norm, 0.5 * gnorm))
        assert np.array_equal(w.cpu().numpy(), wr) and np.array_equal(m.cpu().numpy(), mr) and np.array_equal(v.cpu().numpy(), vr)
        # ... and in a trainable element
        assert q[100] >= 0
        gin = g0.copy(); gin[100] = np.inf
        w, g, m, v = _dev(cuda, (w0, gin, m0, v0))
        _call(L, hp, w, g, m, v, N, max_norm=0.5 * gnorm)
        for t, a in zip((w, m, v), (w0, m0, v0)):
            assert np.array_equal(t.cpu().numpy(), a)
        assert _applied(L, hp) == before + 1
        assert L.qpn_train_status(hp, _stream()) == -4 and b"non-finite" in L.qpn_last_error()
        assert L.qpn_train_status(hp, _stream()) == 0
    finally:
        _off(L, hp)


def test_table_lifetime(cuda, handle, arrs):
    """5: the same table with a new lr is used by the next launch; n_groups = 0 brings the ungrouped bits back; a launch with another n is QPN_EINVAL"""
    L, hp = handle
    ends, groups = TABLES["front"]
    q, _, wd = _per_elem(ends, groups)
    w0, g0, m0, v0, e0 = (a[:N] for a in arrs)
    try:
        _set(L, hp, ends, groups)
        lrs2 = [5e-3, 6e-3, 7e-3]
        _set(L, hp, ends, groups, lrs2)                              # (equal table: values only)
        w, g, m, v = _dev(cuda, (w0, g0, m0, v0))
        _call(L, hp, w, g, m, v, N)
        wr, mr, vr, _ = _expected(w0, g0, m0, v0, e0, q, np.array(lrs2 + [0.0], F)[q], wd)
        assert np.array_equal(w.cpu().numpy(), wr) and np.array_equal(m.cpu().numpy(), mr) and np.array_equal(v.cpu().numpy(), vr)
        # a raw table that only splits a segment is the same table
        _set(L, hp, [100] + ends, [FR] + groups, LRS)
        w, g, m, v = _dev(cuda, (w0, g0, m0, v0))
        _call(L, hp, w, g, m, v, N)
        assert np.array_equal(w.cpu().numpy(), _expected(w0, g0, m0, v0, e0, q, np.array(LRS + [0.0], F)[q], wd)[0])
        # another n
        for n in (N - 1, N + 1, 256):
            w, g, m, v = _dev(cuda, (arrs[0][:N + 1], arrs[1][:N + 1], arrs[2][:N + 1], arrs[3][:N + 1]))
            _call(L, hp, w, g, m, v, n, expect=-1)
            assert b"qpn_adam_groups" in L.qpn_last_error() and np.array_equal(w.cpu().numpy(), arrs[0][:N + 1])
            _call(L, hp, w, g, m, v, n, max_norm=1.0, expect=-1)
        # off: the launch it always was, with the call's own values
        _off(L, hp)
        w, g, m, v = _dev(cuda, (w0, g0, m0, v0))
        _call(L, hp, w, g, m, v, N, lr=LRS[2], wd=WDS[2])
        wr, mr, vr = _ref_adam(w0, g0, m0, v0, F(LRS[2]), F(WDS[2]))
        assert np.array_equal(w.cpu().numpy(), wr) and np.array_equal(m.cpu().numpy(), mr) and np.array_equal(v.cpu().numpy(), vr)
    finally:
        _off(L, hp)


def test_grouped_step_on_a_non_blocking_stream_with_late_buffers(cuda, handle, arrs):
    """9: the table is set up front; behind a gate on a non-blocking stream the real gradient replaces a decoy, then the per-step value call and the grouped,
    clipped, averaging launch are enqueued while the gate is still closed: the result is that of the real gradient and the new values"""
    import torch
    L, hp = handle
    ends, groups = TABLES["edge"]
    q, _, wd = _per_elem(ends, groups)
    w0, g0, m0, v0, e0 = (a[:N] for a in arrs)
    gnorm = float(np.sqrt((np.where(q >= 0, g0, 0).astype(np.float64) ** 2).sum()))
    lrs2 = [2e-3, 4e-3, 8e-3]
    try:
        _set(L, hp, ends, groups)
        w, g, m, v, e = _dev(cuda, (w0, (g0 * F(-3.0)).astype(F), m0, v0, e0))          # g: the decoy
        real = torch.from_numpy(np.array(g0)).to(cuda)
        s0 = torch.cuda.Stream(cuda)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s0):
            torch.cuda._sleep(1000); t0.record(); torch.cuda._sleep(2000000); t1.record()
        s0.synchronize()
        cycles = int(2000000 * 40.0 / max(t0.elapsed_time(t1), 1e-3))                    # a gate of ~40 ms
        torch.cuda.synchronize()
        s = torch.cuda.Stream(cuda)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            g.copy_(real)
            _set(L, hp, ends, groups, lrs2)
            _call(L, hp, w, g, m, v, N, max_norm=0.5 * gnorm, e=e)
            closed = not s.query()
            norm = _norm(L, hp)
        assert closed, "the value call and the launch are documented not to drain the stream, yet the gate had opened when they returned"
        wr, mr, vr, er = _expected(w0, g0, m0, v0, e0, q, np.array(lrs2 + [0.0], F)[q], wd, _coef(norm, 0.5 * gnorm), None, True)
        for t, r in zip((w, m, v, e), (wr, mr, vr, er)):
            assert np.array_equal(t.cpu().numpy(), r)
    finally:
        _off(L, hp)


# ---------------------------------------------------------------- the model-level paths: TINY, lr 1e-3, chunks of synth.train_inputs
# weight decay 1e-3 in every group, as in the comparison the 2e-6 bound comes from where the one-call step's backward is involved (tests/test_grad_clip_gpu.py: it
# keeps every element's effective gradient far above Adam's eps, where two correct backward implementations otherwise part by more than the bound)
LR, WD, WSEED = 1e-3, 1e-3, 11
FROZEN_PATS = ["causal.*", "upsampling.*", "dil*", "res*", "skip*"]
TRAINER_GROUPS = [{"params": FROZEN_PATS, "frozen": True}, {"params": "conv_post_2.*", "lr_scale": 0.5}]


def _to(dev, *a):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]


@pytest.fixture(scope="module")
def chunks(cuda):
    return [_to(cuda, *synth.train_inputs(TINY, 700, 80 + i, 30000)) for i in range(4)]


def _model(cuda):
    return util.build_model(TINY, synth.make_weights(TINY, WSEED), cuda).train()


def _is_trainable(k):
    return k.startswith("aux") or k.startswith("conv_post_")


def _torch_groups(m):
    named = dict(m.named_parameters())
    return [{"params": [p for k, p in named.items() if k.startswith("aux") or k.startswith("conv_post_1.")]},
            {"params": [p for k, p in named.items() if k.startswith("conv_post_2.")], "lr": float(F(LR) * F(0.5))}]


def _loop_step(m, opt, chunk):
    import torch
    xt, ht, tt, dt, bt = chunk
    out = m(xt, ht, dt, bt)
    loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, TINY.n_quantize), tt[:, -out.shape[1]:].reshape(-1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


def _state(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _check_frozen_and_moved(w, w_init):
    for k in w:
        if _is_trainable(k):
            assert not np.array_equal(w[k], w_init[k]), k + " has not moved"
            assert (w[k] != w_init[k]).mean() > 0.9, k
        else:
            assert np.array_equal(w[k], w_init[k]), k + " is frozen and has changed"


@pytest.fixture(scope="module")
def torch_run(cuda, chunks):
    """three steps of torch.optim.Adam's own update (the step hooks off) with the groups: made once"""
    import torch
    mp = pytest.MonkeyPatch()
    mp.setenv("QPN_DROPIN_FUSED_ADAM", "0")
    try:
        m = _model(cuda)
        init = _state(m)
        opt = torch.optim.Adam(_torch_groups(m), lr=LR, weight_decay=WD)
        for i in range(3):
            _loop_step(m, opt, chunks[i])
        return init, _state(m)
    finally:
        mp.undo()


@pytest.mark.parametrize("kind", ["trainer", "flat_adam"])
def test_three_steps_with_groups_match_torch_adam_with_those_groups(kind, cuda, chunks, torch_run):
    """6: everything frozen except aux* and conv_post_*, conv_post_2.* at half the rate: weights to atol 2e-6 of torch's (the bound of
    test_flat_adam_matches_torch_adam for three steps at this lr), frozen tensors bitwise their initial values, trainable tensors moved"""
    from qpnet_amd.train import FlatAdam, FusedTrainer
    init, want = torch_run
    m = _model(cuda)
    if kind == "trainer":
        tr = FusedTrainer(m, lr=LR, weight_decay=WD, param_groups=TRAINER_GROUPS)
        for i in range(3):
            tr.step(*chunks[i])
        tr.check_status()
        assert tr.n_trainable == sum(v.size for k, v in init.items() if _is_trainable(k)) and tr.n_trainable + tr.n_frozen == TINY.n_params
    else:
        opt = FlatAdam(m, _torch_groups(m), lr=LR, weight_decay=WD)
        for i in range(3):
            _loop_step(m, opt, chunks[i])
        m.check_status()
    got = _state(m)
    worst = max(float(np.abs(got[k] - want[k]).max()) for k in got)
    print("ADAM_GROUPS %s vs torch.optim.Adam with the same groups, three steps: max |dw| = %.3e" % (kind, worst))
    _check_frozen_and_moved(got, init)
    for k in got:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=2e-6, err_msg=k)
    # the groups are visible: conv_post_2 moved about half as far as it does at the full rate
    step2 = np.abs(got["conv_post_2.weight"] - init["conv_post_2.weight"]).mean()
    step1 = np.abs(got["conv_post_1.weight"] - init["conv_post_1.weight"]).mean()
    assert 0.3 < step2 / step1 < 0.7, (step1, step2)


@pytest.mark.parametrize("path", ["accum2", "world2"])
def test_groups_on_the_other_host_paths(path, cuda, chunks):
    """7: accum_steps = 2, and world_size = 2 under the identity exchange (no process group, as test_world2_without_exchange_equals_world1 sets it up).  After two
    updates the frozen tensors are bitwise unchanged and the others have moved; after the FIRST update -- both runs start from the same weights and see the same
    chunks; from the second on the frozen tensors differ between the runs, and with them every gradient -- the default group's tensors are within 2e-6 of the
    run of the same path without groups"""
    from qpnet_amd.train import FusedTrainer
    kw = dict(accum_steps=2) if path == "accum2" else dict(world_size=2)
    per_update = 2 if path == "accum2" else 1
    first = {}
    for name, groups, updates in (("plain", None, 1), ("grouped", TRAINER_GROUPS, 2)):
        m = _model(cuda)
        init = _state(m)
        tr = FusedTrainer(m, lr=LR, weight_decay=WD, param_groups=groups, **kw)
        for u in range(updates):
            for i in range(per_update):
                tr.step(*chunks[u * per_update + i])
            tr.check_status()
            assert tr.step_count == u + 1
            if u == 0:
                first[name] = _state(m)
        if groups is not None:
            _check_frozen_and_moved(first[name], init)
            _check_frozen_and_moved(_state(m), init)
            assert not np.array_equal(_state(m)["conv_post_1.weight"], first[name]["conv_post_1.weight"])
    worst = 0.0
    for k in first["plain"]:
        if k.startswith("aux") or k.startswith("conv_post_1."):
            worst = max(worst, float(np.abs(first["grouped"][k] - first["plain"][k]).max()))
            np.testing.assert_allclose(first["grouped"][k], first["plain"][k], rtol=0, atol=2e-6, err_msg=k)
    print("ADAM_GROUPS %s: default-group tensors, grouped vs ungrouped run after one update: max |dw| = %.3e" % (path, worst))


def test_checkpoint_round_trip_with_groups(cuda, chunks, tmp_path):
    """8: saved after two steps, loaded into a fresh grouped trainer: steps 3-4 reproduce the straight run's losses to 1e-6 (test_trainer_checkpoint_resumes_like_
    torch_adam's bound); the file's optimizer state loads into a torch.optim.Adam built with the same groups"""
    import torch
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FusedTrainer
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR, weight_decay=WD, param_groups=TRAINER_GROUPS)
    for i in range(2):
        tr.step(*chunks[i])
    path = loaders.save_checkpoint(str(tmp_path), m, tr, 2)
    ref_losses = [tr.step(*chunks[i]) for i in (2, 3)]
    w_ref = _state(m)
    m2 = QPNet(**TINY.kwargs()).to(cuda).train()
    tr2 = FusedTrainer(m2, lr=5e-2, weight_decay=WD, param_groups=TRAINER_GROUPS)
    assert loaders.load_checkpoint(path, m2, tr2) == 2 and tr2.step_count == 2 and abs(tr2.lr - LR) < 1e-9
    np.testing.assert_allclose([tr2.step(*chunks[i]) for i in (2, 3)], ref_losses, rtol=0, atol=1e-6)
    w2 = _state(m2)
    for k in w2:
        if _is_trainable(k):
            np.testing.assert_allclose(w2[k], w_ref[k], rtol=0, atol=2e-6, err_msg=k)
        else:
            assert np.array_equal(w2[k], w_ref[k]), k
    ck = torch.load(path, weights_only=False)
    m3 = QPNet(**TINY.kwargs())
    opt = torch.optim.Adam(_torch_groups(m3), lr=LR, weight_decay=WD)
    opt.load_state_dict(ck["optimizer"])
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2 and len(sd["state"]) == sum(len(g["params"]) for g in sd["param_groups"])
    # torch numbers conv_post_2.bias last (the last tensor of the last group): its state is the file's last entry
    st = opt.state[dict(m3.named_parameters())["conv_post_2.bias"]]
    last = ck["optimizer"]["state"][len(sd["state"]) - 1]
    assert float(st["step"]) == 2.0 and st["exp_avg"].shape == (TINY.n_quantize,) and torch.equal(st["exp_avg"].cpu(), last["exp_avg"].cpu()) and float(st["exp_avg"].abs().max()) > 0


def test_run_update_with_freeze(cuda, tmp_path):
    """10: run_update --freeze for a handful of iterations: the frozen keys of the written checkpoint are bitwise those of --pretrain, the others differ"""
    import argparse
    import torch
    from qpnet_amd import runners
    from test_runners_gpu import _corpus
    root = _corpus(str(tmp_path / "corpus"))
    conf = str(tmp_path / "model.conf")
    loaders.save_model_conf(conf, argparse.Namespace(feature_type="world", feature_format="npy", dense_factor=8, **TINY.kwargs()))
    pre = loaders.save_checkpoint(str(tmp_path / "si"), _model(cuda), None, 0)
    exp = str(tmp_path / "sd")
    assert runners.run_update(["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz", "--expdir", exp, "--config", conf,
                               "--pretrain", pre, "--iters", "4", "--batch_length", "1500", "--max_length", "4000", "--intervals", "2", "--verbose", "0",
                               "--resume", exp + "/none.pkl", "--lr", "1e-3", "--freeze", ",".join(FROZEN_PATS), "--lr_scale", "conv_post_2.*=0.5"]) == 0
    a = torch.load(pre, map_location="cpu")["model"]
    b = torch.load(exp + "/checkpoint-final.pkl", map_location="cpu")["model"]
    assert list(a) == list(b)
    for k in a:
        if _is_trainable(k):
            assert not torch.equal(a[k], b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind", ["trainer", "flat_adam", "stock_adam"])
def test_an_optimiser_without_groups_after_a_grouped_one_trains_everything(kind, cuda, chunks):
    """The groups are sticky on the module's native handle.  Freeze for one step with a grouped trainer, then build an optimiser WITHOUT groups on the same
    module -- a FusedTrainer, a FlatAdam, a stock torch.optim.Adam the step hooks adopt: its step moves the formerly frozen tensors with its own lr, and equals (2e-6,
    the bound of the other one-step comparisons here) the same step on a module that starts from the same weights and never had groups"""
    import torch
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FlatAdam, FusedTrainer

    def second_step(m):
        if kind == "trainer":
            tr = FusedTrainer(m, lr=LR, weight_decay=WD)
            tr.step(*chunks[1])
            tr.check_status()
        else:
            opt = FlatAdam(m, lr=LR, weight_decay=WD) if kind == "flat_adam" else torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
            _loop_step(m, opt, chunks[1])
            m.check_status()
            if kind == "stock_adam":
                assert opt.__dict__.get("_qpn_adopt"), "the step hooks did not adopt the stock Adam: this case would prove nothing"

    m = _model(cuda)
    init = _state(m)
    tr = FusedTrainer(m, lr=LR, weight_decay=WD, param_groups=TRAINER_GROUPS)
    tr.step(*chunks[0])
    tr.check_status()
    after_grouped = _state(m)
    _check_frozen_and_moved(after_grouped, init)
    ref = QPNet(**TINY.kwargs())
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in after_grouped.items()})
    ref = ref.to(cuda).train()
    second_step(m)
    second_step(ref)
    got, want = _state(m), _state(ref)
    worst = 0.0
    for k in got:
        assert (got[k] != after_grouped[k]).mean() > 0.9, k + " did not move under the optimiser without groups"
        worst = max(worst, float(np.abs(got[k] - want[k]).max()))
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=2e-6, err_msg=k)
    print("ADAM_GROUPS %s without groups behind a grouped trainer vs a module that never had groups: max |dw| = %.3e" % (kind, worst))
    # ... and a grouped optimiser built after that one puts its groups back
    tr2 = FusedTrainer(m, lr=LR, weight_decay=WD, param_groups=TRAINER_GROUPS)
    tr2.step(*chunks[2])
    tr2.check_status()
    _check_frozen_and_moved(_state(m), got)
