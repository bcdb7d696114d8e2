"""GPU: the loss options -- k_ce_hard<NV, true> / k_weight_mass / k_ce_soft<NV, true> (qpn_ce_loss_opts, qpn_distill_loss_opts) bit for bit against qpn_ce_loss / qpn_distill_loss
where the options are neutral or powers of two, and against the float64 spec (tests/loss_opts_spec.py) elsewhere; the armed forward-with-loss
(qpn_train_loss_opts) against its pieces; FusedTrainer(ignore_index=, label_smoothing=, loss_norm=).step(sample_weights=) against a loop of forward,
train.cross_entropy and backward; the compositions (accumulation, world_size 2, distillation, h_grad, a non-blocking stream); run_train's two flags.

    w_r = weights[r], 0 where y == ignore_index;   CE_r = lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q;   L = (1 / N) sum_r w_r CE_r
    dL/dz_r = (w_r / N) (softmax(z) - (1 - eps) onehot(y) - eps / Q);   N = rows or sum_r w_r                  ("Loss options")

Every check prints its figures before it asserts."""
import ctypes as C
import dataclasses
import logging
import os

import numpy as np
import pytest
import yaml

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY, PAPER
import loss_opts_spec as spec
import test_distill_gpu as DG
import test_streams_gpu as ST
import util

pytestmark = pytest.mark.gpu

B0, BL0 = 2, 37                       # 74 rows: five workgroups of 16, the last with empty wave slots; no multiple of 4 or 16
STRIDE0 = BL0 + 4                     # tgt_stride 41: the targets are the last 37 columns
ROWS = B0 * BL0
gate = ST.gate                        # the calibrated torch.cuda._sleep gate of tests/test_streams_gpu.py (a module-scoped fixture)
_to, _stream, _RefAdam, _chunk, _two_row_batch, _teacher_logits = DG._to, DG._stream, DG._RefAdam, DG._chunk, DG._two_row_batch, DG._teacher_logits


def _opts(w=None, ign=None, eps=0.0, norm=0):
    return _lib.QpnLossOpts(w.data_ptr() if w is not None else None, w.numel() if w is not None else 0, 0 if ign is None else 1, 0 if ign is None else ign, eps, norm)


# every instance family of train_loss.hip: the register forms NV = 1 .. 4 (Q = 256 NV), the float4 loop form (Q % 256 == 0, Q > 1024) and the scalar loop form
@pytest.fixture(scope="module", params=[256, 512, 96, 768, 1024, 1280], ids=["Q256-NV1", "Q512-NV2", "Q96-scalar", "Q768-NV3", "Q1024-NV4", "Q1280-vecloop"])
def case(request):
    """one handle and one set of inputs per class count, shared by the kernel tests (and left unchanged by them): random logits with |z| <= 10, one peaked row;
    the plain kernels' outputs, computed once"""
    import torch
    Q = request.param
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(500 + Q)
    z = rs.uniform(-10, 10, (B0, BL0, Q)).astype(np.float32)
    t = rs.uniform(-10, 10, (B0, BL0, Q)).astype(np.float32)
    z[0, 3] = -10.0; z[0, 3, Q // 3] = 10.0
    y = rs.randint(0, Q, (B0, STRIDE0)).astype(np.int64)
    y[0, STRIDE0 - BL0 + 3] = Q // 3
    y[1, -1] = Q - 1; y[1, -2] = 0                     # the last columns, the ends of the class range
    L = _lib.lib()
    hp = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(L.qpn_create(C.byref(_lib.make_config(dataclasses.replace(TINY, n_quantize=Q))), C.byref(hp)))
    zt, tt, yt = _to(dev, z, t, y)
    c = dict(Q=Q, dev=dev, L=L, hp=hp, z=zt, t=tt, y=yt, z64=z.reshape(ROWS, Q).astype(np.float64), y_rows=y[:, -BL0:].reshape(ROWS), rs=rs)
    dce, one = torch.full_like(zt, 7.0), C.c_double(0)
    with torch.cuda.device(dev):
        _lib.check(L.qpn_ce_loss(hp, zt.data_ptr(), yt.data_ptr(), STRIDE0, B0, BL0, dce.data_ptr(), C.byref(one), _stream(dev)))
        _lib.check(L.qpn_train_status(hp, _stream(dev)))
    c["dl_plain"], c["loss_plain"] = dce, one.value
    # the yardstick of the float64 comparisons: qpn_ce_loss's own error on these logits
    _, g64, _ = spec.loss_and_grad(c["z64"], c["y_rows"])
    c["yard"] = float(np.abs(dce.cpu().numpy().reshape(ROWS, Q).astype(np.float64) * ROWS - g64 * ROWS).max())
    dd, p3 = torch.full_like(zt, 7.0), (C.c_double * 3)()
    with torch.cuda.device(dev):
        _lib.check(L.qpn_distill_loss(hp, zt.data_ptr(), tt.data_ptr(), yt.data_ptr(), STRIDE0, B0, BL0, 0.5, 2.0, dd.data_ptr(), p3, _stream(dev)))
        _lib.check(L.qpn_train_status(hp, _stream(dev)))
    c["dd_plain"], c["dloss_plain"] = dd, list(p3)
    yield c
    L.qpn_destroy(hp)


def _ce(c, w=None, ign=None, eps=0.0, norm=0, z=None, y=None, check=True):
    """qpn_ce_loss_opts -> (dL/dlogits, loss, effective mass, status rc)"""
    import torch
    z = c["z"] if z is None else z
    y = c["y"] if y is None else y
    dl, p2, o = torch.full_like(z, 7.0), (C.c_double * 2)(), _opts(w, ign, eps, norm)
    with torch.cuda.device(c["dev"]):
        _lib.check(c["L"].qpn_ce_loss_opts(c["hp"], z.data_ptr(), y.data_ptr(), STRIDE0, B0, BL0, C.byref(o), dl.data_ptr(), p2, _stream(c["dev"])))
        rc = c["L"].qpn_train_status(c["hp"], _stream(c["dev"]))
    if check:
        assert rc == 0, c["L"].qpn_last_error().decode()
    return dl, p2[0], p2[1], rc


def _dist(c, w=None, ign=None, norm=0, z=None, t=None, y=None):
    """qpn_distill_loss_opts (alpha 0.5, T 2) -> (dL/dlogits, [total, CE, T^2 KL, mass])"""
    import torch
    z, t, y = (c["z"] if z is None else z), (c["t"] if t is None else t), (c["y"] if y is None else y)
    dl, p4, o = torch.full_like(z, 7.0), (C.c_double * 4)(), _opts(w, ign, 0.0, norm)
    with torch.cuda.device(c["dev"]):
        _lib.check(c["L"].qpn_distill_loss_opts(c["hp"], z.data_ptr(), t.data_ptr(), y.data_ptr(), STRIDE0, B0, BL0, 0.5, 2.0, C.byref(o), dl.data_ptr(), p4, _stream(c["dev"])))
        _lib.check(c["L"].qpn_train_status(c["hp"], _stream(c["dev"])))
    return dl, list(p4)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _pow2_weights(c):
    import torch
    w = np.random.RandomState(7).choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], np.float32), (B0, BL0))
    w[0, 0], w[0, 1], w[1, -1] = 0.0, 2.0, 0.25                 # every value is there, the first and the last row among them
    return torch.from_numpy(w).to(c["dev"])


# ---------------------------------------------------------------- 1. bitwise, no tolerance
def test_neutral_options_give_the_plain_kernels_bits(case):
    import torch
    c = case
    ones = torch.ones((B0, BL0), device=c["dev"])
    dl, loss, mass, _ = _ce(c, ones)
    print("BITS Q=%d ones: loss %.15f plain %.15f mass %.1f" % (c["Q"], loss, c["loss_plain"], mass))
    assert torch.equal(_bits(dl), _bits(c["dl_plain"])) and abs(loss - c["loss_plain"]) < 1e-12 and mass == ROWS
    dl, loss, mass, _ = _ce(c, None, ign=-100)                    # an ignore_index no target has: the same
    assert torch.equal(_bits(dl), _bits(c["dl_plain"])) and abs(loss - c["loss_plain"]) < 1e-12 and mass == ROWS
    dd, p4 = _dist(c, ones)
    assert torch.equal(_bits(dd), _bits(c["dd_plain"])) and all(abs(a - b) < 1e-12 for a, b in zip(p4[:3], c["dloss_plain"])) and p4[3] == ROWS


def test_power_of_two_weights_scale_the_rows_exactly(case):
    import torch
    c = case
    w = _pow2_weights(c)
    zero = (w == 0).reshape(-1)
    assert int(zero.sum()) >= 5
    for name, dl, plain in (("ce", _ce(c, w)[0], c["dl_plain"]), ("distill", _dist(c, w)[0], c["dd_plain"])):
        want = plain * w[:, :, None]
        rows_d, rows_w = dl.reshape(ROWS, -1), want.reshape(ROWS, -1)
        assert torch.equal(rows_d[~zero], rows_w[~zero]), name        # dlogits[r] == w_r * dlogits_plain[r], exactly
        assert not bool(_bits(rows_d[zero]).any()), name               # zero rows: every bit clear, exact +0
    # the loss: sum_r w_r CE_r over the row count, from qpn_ce_loss's own float64-accurate row terms
    ce, _ = spec.row_terms(c["z64"], c["y_rows"])
    loss = _ce(c, w)[1]
    assert abs(loss - float((w.cpu().numpy().reshape(-1).astype(np.float64) * ce).sum() / ROWS)) < 1e-4


# ---------------------------------------------------------------- 2. against float64
def _hole_weights(c, seed=11):
    """uniform in [0, 2) with a zero block that covers one whole workgroup (rows 16 .. 31) and straddles the next (.. 39)"""
    import torch
    w = np.random.RandomState(seed).uniform(0.0, 2.0, ROWS).astype(np.float32)
    w[16:40] = 0.0
    return torch.from_numpy(w.reshape(B0, BL0)).to(c["dev"]), w.astype(np.float64)


@pytest.mark.parametrize("norm", ["rows", "weights"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_opts_against_float64(case, eps, norm):
    """loss within 1e-4 (test_distill_loss_against_float64's bound); max |dL/dz N - float64| / max w within 4 x qpn_ce_loss's own error on the same logits, 8 x with
    smoothing (that test's two bounds, for one and two terms); the reported mass within 1e-12 relative.  Measured: profiles/loss_options.txt"""
    c = case
    wt, w64 = _hole_weights(c)
    L64, g64, m64 = spec.loss_and_grad(c["z64"], c["y_rows"], weights=w64, label_smoothing=eps, norm=norm)
    dl, loss, mass, _ = _ce(c, wt, eps=eps, norm=1 if norm == "weights" else 0)
    N = ROWS if norm == "rows" else m64
    err = float(np.abs(dl.cpu().numpy().reshape(ROWS, -1).astype(np.float64) * N - g64 * N).max()) / float(w64.max())
    bound = 8.0 if eps > 0 else 4.0
    print("LOSS_OPTS Q=%d eps=%g norm=%s: loss %.9f float64 %.9f; max |dL/dz N - float64| / max w = %.3e, qpn_ce_loss's own %.3e, ratio %.2f (bound %g); mass %.12f float64 %.12f"
          % (c["Q"], eps, norm, loss, L64, err, c["yard"], err / c["yard"], bound, mass, m64))
    assert abs(loss - L64) < 1e-4
    assert c["yard"] > 0 and err <= bound * c["yard"]
    assert abs(mass - m64) <= 1e-12 * m64
    assert not bool(_bits(dl.reshape(ROWS, -1)[16:40]).any())


# ---------------------------------------------------------------- 3. ignore_index
@pytest.mark.parametrize("ign", [-100, 3])
def test_ignore_index_equals_torch_mean_in_float64(case, ign):
    import torch
    import torch.nn.functional as F
    c = case
    Q = c["Q"]
    y = c["y"].clone()
    tail = y[:, -BL0:]
    tail[torch.from_numpy(np.random.RandomState(5).rand(B0, BL0) < 0.3).to(c["dev"])] = ign
    tail[0, 0] = ign
    y_rows = tail.reshape(-1).cpu()
    live = y_rows != ign
    assert 10 < int(live.sum()) < ROWS
    z64 = torch.from_numpy(c["z64"]).requires_grad_(True)
    ref = F.cross_entropy(z64, y_rows, ignore_index=ign)
    ref.backward()
    dl, loss, mass, _ = _ce(c, None, ign=ign, norm=1, y=y)
    err = float((dl.cpu().reshape(ROWS, Q).double() - z64.grad).abs().max()) * mass
    print("IGNORE Q=%d ignore_index=%d: loss %.9f torch float64 %.9f, mass %g of %d rows, max |dL/dz N - float64| = %.3e (qpn_ce_loss's own %.3e)"
          % (Q, ign, loss, float(ref.detach()), mass, ROWS, err, c["yard"]))
    assert mass == float(live.sum()) and abs(loss - float(ref.detach())) < 1e-4 and err <= 4.0 * c["yard"]
    # a target outside [0, Q) in an ignored row (-100 is one itself) or in a zero-weight row raises no status ...
    w = torch.ones((B0, BL0), device=c["dev"]); w[1, 7] = 0.0
    y2 = y.clone(); y2[1, STRIDE0 - BL0 + 7] = Q + 5
    dl2, loss2, mass2, rc = _ce(c, w, ign=ign, norm=1, y=y2, check=False)
    assert rc == 0 and not bool(_bits(dl2[1, 7]).any())
    # ... the same target in a live row still sets value 2
    j = int(np.nonzero(live.numpy().reshape(B0, BL0)[1])[0][0])
    y3 = y.clone(); y3[1, STRIDE0 - BL0 + j] = Q + 5
    _, _, _, rc = _ce(c, None, ign=ign, norm=1, y=y3, check=False)
    assert rc == -4 and "target class" in c["L"].qpn_last_error().decode()


# ---------------------------------------------------------------- 4. masked rows are not read
def test_zero_weight_rows_are_not_read(case):
    import torch
    c = case
    wt, _ = _hole_weights(c)
    wt = wt.clone(); wt[1, -1] = 0.0
    dead = (wt == 0)
    z, t, y = c["z"].clone(), c["t"].clone(), c["y"].clone()
    z[dead] = float("nan"); t[dead] = float("inf")
    tail = y[:, -BL0:]
    tail[dead] = torch.tensor([1 << 40, -7], device=c["dev"]).repeat(int(dead.sum()) // 2 + 1)[:int(dead.sum())]
    for eps, norm in ((0.0, 0), (0.1, 1)):
        a, la, ma, _ = _ce(c, wt, eps=eps, norm=norm)
        b, lb, mb, _ = _ce(c, wt, eps=eps, norm=norm, z=z, y=y)              # (status checked clean inside)
        assert torch.equal(_bits(a), _bits(b)) and abs(la - lb) < 1e-12 and ma == mb and np.isfinite(lb)
    a, pa = _dist(c, wt)
    b, pb = _dist(c, wt, z=z, t=t, y=y)
    assert torch.equal(_bits(a), _bits(b)) and all(abs(u - v) < 1e-12 for u, v in zip(pa, pb))


# ---------------------------------------------------------------- 5. degenerate and bad weights
def test_all_zero_weights_under_norm_weights(case):
    import torch
    c = case
    w = torch.zeros((B0, BL0), device=c["dev"])
    dl, loss, mass, _ = _ce(c, w, eps=0.1, norm=1)
    assert loss == 0.0 and mass == 0.0 and not bool(_bits(dl).any())
    dd, p4 = _dist(c, w, norm=1)
    assert p4[0] == 0.0 and p4[3] == 0.0 and not bool(_bits(dd).any())
    y = torch.full_like(c["y"], -100)
    dl, loss, mass, _ = _ce(c, None, ign=-100, norm=1, y=y)
    assert loss == 0.0 and mass == 0.0 and not bool(_bits(dl).any())


@pytest.mark.parametrize("bad", [float("nan"), -0.5, float("inf")], ids=["nan", "negative", "inf"])
def test_a_bad_weight_is_flagged_and_counts_as_zero(case, bad):
    import torch
    c = case
    wt, w64 = _hole_weights(c)
    wt = wt.clone(); wt[0, 5] = bad
    w64 = w64.copy(); w64[5] = 0.0
    for norm in (0, 1):
        dl, loss, mass, rc = _ce(c, wt, norm=norm, check=False)
        msg = c["L"].qpn_last_error().decode()
        L64, _, m64 = spec.loss_and_grad(c["z64"], c["y_rows"], weights=w64, norm="weights" if norm else "rows")
        print("BAD WEIGHT Q=%d %r norm=%d: rc %d, loss %.9f float64 with the weight at 0 %.9f" % (c["Q"], bad, norm, rc, loss, L64))
        assert rc == -4 and "sample weights" in msg
        assert abs(loss - L64) < 1e-4 and abs(mass - m64) <= 1e-12 * m64 and not bool(_bits(dl[0, 5]).any())
    _, _, _, rc = _ce(c, _hole_weights(c)[0])                                 # reported once: the word is clean again
    assert rc == 0


def test_a_bad_weight_skips_the_update(cuda):
    """test_a_non_finite_teacher_value_skips_the_update with a NaN among the sample weights: QpnError(-4) naming the sample weights, parameters and moments untouched by
    the flagged step and by the clean one enqueued behind it; training goes on"""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), cuda).train()
    tr = FusedTrainer(m, lr=1e-3)
    x, h, t, d, b = synth.train_inputs(TINY, 600, 41, 30000)
    xt, ht, tt, dt = _to(cuda, x, h, t, d)
    maxd = int(np.ceil(d).max())
    w = torch.rand((x.shape[0], int(b[0])), device=cuda)
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, sample_weights=w)
    tr.flush_loss(); tr.check_status()
    w0, m0, v0 = m.flat_parameters().clone(), tr.m.clone(), tr.v.clone()
    bad = w.clone(); bad[0, 17] = float("nan")
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, sample_weights=bad)
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, sample_weights=w)
    tr.flush_loss()
    with pytest.raises(_lib.QpnError, match="sample weights") as e:
        tr.check_status()
    assert e.value.code == -4
    assert torch.equal(m.flat_parameters(), w0) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0) and tr.step_count == 1
    loss = tr.step(xt, ht, tt, dt, b, want_loss=True, maxd=maxd, sample_weights=w)
    assert np.isfinite(loss) and not torch.equal(m.flat_parameters(), w0) and tr.step_count == 2
    neg = w.clone(); neg[0, 3] = -1.0
    with pytest.raises(_lib.QpnError, match="sample weights"):
        tr.step(xt, ht, tt, dt, b, want_loss=True, maxd=maxd, sample_weights=neg)          # checked in the call: its Adam launch applied nothing
    assert tr.step_count == 2


# ---------------------------------------------------------------- 6. repeatability
def test_two_calls_give_the_same_bits(case):
    import torch
    c = case
    wt, _ = _hole_weights(c)
    for norm in (0, 1):
        a, la, ma, _ = _ce(c, wt, eps=0.1, norm=norm)
        b, lb, mb, _ = _ce(c, wt, eps=0.1, norm=norm)
        assert torch.equal(_bits(a), _bits(b)) and not bool((a == 7.0).any()) and abs(la - lb) < 1e-12 and abs(ma - mb) <= 1e-12 * ma
        a, _ = _dist(c, wt, norm=norm)
        b, _ = _dist(c, wt, norm=norm)
        assert torch.equal(_bits(a), _bits(b)) and not bool((a == 7.0).any())


# ---------------------------------------------------------------- 7. the armed forward-with-loss equals the pieces
def _step_weights(cuda, B, BL, seed=3):
    """uniform in [0, 2), a zero block that covers whole workgroups, on the device"""
    import torch
    w = torch.rand((B, BL), generator=torch.Generator().manual_seed(seed)) * 2.0
    w[0, 100:180] = 0.0
    w[-1, -1] = 0.0
    return w.to(cuda)


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_armed_forward_equals_the_pieces(cfgname, cuda):
    """qpn_train_loss_opts + qpn_train_forward_loss against qpn_train_forward, then qpn_ce_loss_opts on those logits: same logits and dL/dlogits bit for bit, the loss
    up to the order of the partial sums, the backward's flat gradient within 1e-6 max(1, |g|max); the same with want_logits = 2, and with norm = weights"""
    import torch
    from qpnet_amd.train import ensure_flat
    cfg = TINY if cfgname == "tiny" else PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 23), cuda)
    xt, ht, tt, dt, BL, maxd = _two_row_batch(cfg, 700 if cfgname == "tiny" else 1500, cuda)
    L, hd = m._native(cuda)
    flat = ensure_flat(m, cuda)
    B, T = xt.shape; Q = cfg.n_quantize
    w = _step_weights(cuda, B, BL)
    stream = _stream(cuda)
    args = (hd, flat.data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr())
    for norm, want in ((0, 1), (0, 2), (1, 2)):
        o = _opts(w, ign=int(tt[0, -3]), eps=0.1, norm=norm)
        lg0 = torch.empty((B, BL, Q), device=cuda); dl0 = torch.empty_like(lg0)
        lg1 = torch.full((B, BL, Q), 7.0, device=cuda); dl1 = torch.empty_like(lg0)
        p0, l1 = (C.c_double * 2)(), C.c_double(0)
        _lib.check(L.qpn_train_forward(*args, lg0.data_ptr(), stream))
        _lib.check(L.qpn_ce_loss_opts(hd, lg0.data_ptr(), tt.data_ptr(), tt.shape[1], B, BL, C.byref(o), dl0.data_ptr(), p0, stream))
        _lib.check(L.qpn_train_loss_opts(hd, C.byref(o)))
        _lib.check(L.qpn_train_forward_loss(*args, tt.data_ptr(), tt.shape[1], lg1.data_ptr(), want, dl1.data_ptr(), stream))
        _lib.check(L.qpn_train_loss(hd, C.byref(l1), stream))
        _lib.check(L.qpn_train_status(hd, stream))
        print("ARMED %s norm=%d want_logits=%d: loss %.12f, pieces %.12f (mass %.6f)" % (cfgname, norm, want, l1.value, p0[0], p0[1]))
        assert torch.equal(lg0, lg1) and torch.equal(_bits(dl0), _bits(dl1)) and abs(p0[0] - l1.value) < 1e-12 and 0 < p0[1] < B * BL
        g0 = torch.empty(flat.numel(), device=cuda); g1 = torch.empty_like(g0)
        _lib.check(L.qpn_train_backward(hd, dl1.data_ptr(), g1.data_ptr(), stream))
        _lib.check(L.qpn_train_forward(*args, lg0.data_ptr(), stream))
        _lib.check(L.qpn_train_backward(hd, dl0.data_ptr(), g0.data_ptr(), stream))
        _lib.check(L.qpn_train_status(hd, stream))
        assert float((g0 - g1).abs().max()) <= 1e-6 * max(1.0, float(g0.abs().max()))


# ---------------------------------------------------------------- 8. one shot, and the default is untouched
@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_one_shot_and_the_default_is_untouched(cfgname, cuda):
    import torch
    from qpnet_amd.train import ensure_flat
    cfg = TINY if cfgname == "tiny" else PAPER
    xt, ht, tt, dt, BL, maxd = _two_row_batch(cfg, 700 if cfgname == "tiny" else 1500, cuda)
    B, T = xt.shape; Q = cfg.n_quantize
    w = _step_weights(cuda, B, BL)
    stream = _stream(cuda)
    L = _lib.lib()

    def fwd_loss(m, want=0):
        hd = m._native(cuda)[1]
        flat = ensure_flat(m, cuda)
        lg = torch.full((B, BL, Q), 7.0, device=cuda); dl = torch.full_like(lg, 7.0)
        rc = L.qpn_train_forward_loss(hd, flat.data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr(),
                                      tt.data_ptr(), tt.shape[1], lg.data_ptr(), want, dl.data_ptr(), stream)
        if rc:
            return rc, lg, dl, None
        loss = C.c_double(0)
        _lib.check(L.qpn_train_loss(hd, C.byref(loss), stream))
        _lib.check(L.qpn_train_status(hd, stream))
        return 0, lg, dl, loss.value
    never = util.build_model(cfg, synth.make_weights(cfg, 23), cuda)
    _, _, dl_plain, loss_plain = fwd_loss(never)
    m = util.build_model(cfg, synth.make_weights(cfg, 23), cuda)
    hd = m._native(cuda)[1]
    o = _opts(w, eps=0.1)
    _lib.check(L.qpn_train_loss_opts(hd, C.byref(o)))
    _, _, dl_armed, loss_armed = fwd_loss(m)
    assert not torch.equal(dl_armed, dl_plain) and abs(loss_armed - loss_plain) > 1e-3
    rc, lg, dl, loss = fwd_loss(m)                                     # one shot: this one is the plain cross entropy again
    assert rc == 0 and torch.equal(_bits(dl), _bits(dl_plain)) and loss == loss_plain
    if cfgname == "paper":
        assert float(lg.min()) == 7.0                                  # ... inside the post-net tile, as ever: the logits buffer is left alone
    # an entirely default struct arms nothing: the fused tile again
    _lib.check(L.qpn_train_loss_opts(hd, C.byref(_opts())))
    rc, lg, dl, loss = fwd_loss(m)
    assert rc == 0 and torch.equal(_bits(dl), _bits(dl_plain)) and loss == loss_plain and (cfgname != "paper" or float(lg.min()) == 7.0)
    # a plain forward computes no loss and leaves the arm alone
    _lib.check(L.qpn_train_loss_opts(hd, C.byref(o)))
    lg0 = torch.empty((B, BL, Q), device=cuda)
    _lib.check(L.qpn_train_forward(hd, ensure_flat(m, cuda).data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr(), lg0.data_ptr(), stream))
    rc, _, dl, loss = fwd_loss(m)
    assert rc == 0 and torch.equal(_bits(dl), _bits(dl_armed)) and abs(loss - loss_armed) < 1e-12
    # a wrong n_weights
    short = w.reshape(-1)[:B * BL - 1]
    _lib.check(L.qpn_train_loss_opts(hd, C.byref(_opts(short, eps=0.1))))
    rc, lg, dl, _ = fwd_loss(m)
    torch.cuda.synchronize()
    assert rc == -1 and "n_weights" in L.qpn_last_error().decode() and float(lg.min()) == 7.0 and float(lg.max()) == 7.0 and float(dl.min()) == 7.0
    rc, _, dl, loss = fwd_loss(m)
    assert rc == 0 and torch.equal(_bits(dl), _bits(dl_plain)) and loss == loss_plain


# ---------------------------------------------------------------- 9. the trainer against the loop
LR = 1e-3


def _ref_grad(model, chunk, w, teacher_logits=None, want_h_grad=False, **kw):
    """forward, train.cross_entropy (or distill_loss with weights), backward on the drop-in module: (loss, flat gradient[, h.grad])"""
    import torch
    from qpnet_amd.train import cross_entropy, distill_loss
    xt, ht, tt, dt, bt = chunk
    for p in model.parameters():
        p.grad = None
    if want_h_grad:
        ht = ht.clone().requires_grad_(True)
    out = model(xt, ht, dt, bt)
    if teacher_logits is not None:
        loss = distill_loss(out, teacher_logits, tt, 0.5, 2.0, sample_weights=w, **kw)
    else:
        loss = cross_entropy(out, tt, sample_weights=w, **kw)
    loss.backward()
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()
    return (float(loss.detach()), g, ht.grad.clone()) if want_h_grad else (float(loss.detach()), g)


def _chunk_weights(cuda, chunk, seed):
    import torch
    B, BL = chunk[0].shape[0], int(chunk[4][0])
    w = torch.rand((B, BL), generator=torch.Generator().manual_seed(seed)) * 2.0
    w[:, 50:120] = 0.0
    return w.to(cuda)


@pytest.mark.parametrize("variant", ["smoothing-rows", "ignore-weights"])
def test_fused_trainer_equals_the_loop(variant, cuda):
    """three steps of FusedTrainer(label_smoothing=0.1).step(sample_weights=...) against model(...), train.cross_entropy, backward and torch's Adam on the same chunks:
    loss within 1e-4 per step, weights within 2e-6 at lr 1e-3 (the distillation test's bounds); the plain trainer ends more than 0.5 lr away.  ignore-weights:
    loss_norm="weights", ignore_index=-100 and some targets set to -100"""
    import torch
    from qpnet_amd.train import FusedTrainer
    ign = variant == "ignore-weights"
    kw = dict(label_smoothing=0.1, ignore_index=-100 if ign else None)
    w0 = synth.make_weights(TINY, 11)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, loss_norm="weights" if ign else "rows", **kw)
    ref = util.build_model(TINY, w0, cuda).train()
    opt = _RefAdam(ref, cuda, LR)
    chunks = []
    for step in range(3):
        chunk = _chunk(TINY, cuda, 80 + step)
        if ign:
            chunk[2] = chunk[2].clone()
            chunk[2][:, -300:-200] = -100
            chunk[2][:, -1] = -100
        chunks.append(chunk)
        w = _chunk_weights(cuda, chunk, 20 + step)
        loss = tr.step(*chunk, sample_weights=w)
        rl, g = _ref_grad(ref, chunk, w, norm="weights" if ign else "rows", **kw)
        opt.step(g)
        print("TRAINER %s step %d: loss %.7f, the loop's %.7f" % (variant, step, loss, rl))
        assert abs(loss - rl) < 1e-4
    tr.check_status()
    w, wr = m.flat_parameters().cpu().numpy(), ref.flat_parameters().cpu().numpy()
    print("TRAINER %s: max |w - w_loop| %.3e, moved %.3e" % (variant, np.abs(w - wr).max(), np.abs(w - w0).max()))
    np.testing.assert_allclose(w, wr, atol=2e-6, rtol=0)
    assert np.abs(w - w0).max() > 1e-4
    if not ign:                                     # (the plain criterion flags a target of -100)
        m3 = util.build_model(TINY, w0, cuda).train()
        t3 = FusedTrainer(m3, lr=LR)
        for chunk in chunks:
            t3.step(*chunk)
        assert np.abs(m3.flat_parameters().cpu().numpy() - w).max() > 0.5 * LR


def test_cross_entropy_takes_the_references_flattened_pair(cuda):
    """criterion(output.view(-1, Q), t.view(-1)) as the reference calls it: the same loss and gradient as the (B, BL, Q) form, and the plain criterion's with no option"""
    import torch
    from qpnet_amd.train import cross_entropy
    rs = np.random.RandomState(3)
    z = torch.from_numpy(rs.uniform(-5, 5, (2, 33, 256)).astype(np.float32)).to(cuda)
    y = torch.from_numpy(rs.randint(0, 256, (2, 33))).to(cuda)
    za, zb, zc = (z.clone().requires_grad_(True) for _ in range(3))
    la = cross_entropy(za, y, label_smoothing=0.1); la.backward()
    lb = cross_entropy(zb.view(-1, 256), y.view(-1), label_smoothing=0.1); lb.backward()
    assert float(la) == float(lb) and torch.equal(za.grad, zb.grad)
    lc = cross_entropy(zc.view(-1, 256), y.view(-1)); (2.0 * lc).backward()
    ref = torch.nn.functional.cross_entropy(z.double().view(-1, 256), y.view(-1))
    gref = torch.autograd.functional.jacobian(lambda v: torch.nn.functional.cross_entropy(v.view(-1, 256), y.view(-1)), z.double())
    assert abs(float(lc) - float(ref)) < 1e-5 and float((zc.grad.double() - 2.0 * gref).abs().max()) < 1e-7


# ---------------------------------------------------------------- 10. composition
def test_accumulation_window_equals_the_row_weighted_update(cuda):
    """accum_steps = 2, every micro-step armed with its own weights: two windows of two chunks of unequal batch_length against the row-weighted mean of the loop's
    gradients, then Adam -- tests/test_grad_accum_gpu.py's 4e-6 at lr = 1e-4"""
    from qpnet_amd.train import FusedTrainer
    lr = 1e-4
    w0 = synth.make_weights(TINY, 11)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=lr, accum_steps=2, label_smoothing=0.1)
    ref = util.build_model(TINY, w0, cuda).train()
    opt = _RefAdam(ref, cuda, lr)
    for win in range(2):
        gs, ns = [], []
        for k in range(2):
            chunk = _chunk(TINY, cuda, 90 + 2 * win + k, bl=600 + 150 * k)
            w = _chunk_weights(cuda, chunk, 30 + 2 * win + k)
            assert tr.micro_step == k
            loss = tr.step(*chunk, sample_weights=w)
            rl, g = _ref_grad(ref, chunk, w, label_smoothing=0.1)
            assert abs(loss - rl) < 1e-4
            gs.append(g.double()); ns.append(chunk[0].shape[0] * int(chunk[4][0]))
        assert tr.micro_step == 0 and tr.step_count == win + 1
        opt.step(((ns[0] * gs[0] + ns[1] * gs[1]) / (ns[0] + ns[1])).float())
    tr.check_status()
    w, wr = m.flat_parameters().cpu().numpy(), ref.flat_parameters().cpu().numpy()
    print("ACCUM: max |w - w_ref| %.3e" % np.abs(w - wr).max())
    np.testing.assert_allclose(w, wr, atol=4e-6, rtol=0)
    assert np.abs(w - w0).max() > 1e-4


def test_world2_without_exchange_equals_world1(cuda):
    """no process group, the exchange is the identity: world_size = 2 (forward-with-loss, backward_ex, Adam call by call) reproduces the one-call step"""
    import torch
    from qpnet_amd.train import FusedTrainer
    flat = synth.make_weights(TINY, 5)
    m1 = util.build_model(TINY, flat, cuda).train()
    m2 = util.build_model(TINY, flat, cuda).train()
    t1 = FusedTrainer(m1, lr=1e-4, world_size=1, label_smoothing=0.1, ignore_index=5)
    t2 = FusedTrainer(m2, lr=1e-4, world_size=2, label_smoothing=0.1, ignore_index=5)
    for step in range(3):
        chunk = _chunk(TINY, cuda, 70 + step, bl=600 + 37 * step)
        w = _chunk_weights(cuda, chunk, 40 + step)
        if step:
            assert float((m2.flat_parameters() - m1.flat_parameters()).abs().max()) <= 2e-7
            with torch.no_grad():
                m2._flat.copy_(m1._flat)
        l1 = t1.step(*chunk, sample_weights=w)
        l2 = t2.step(*chunk, sample_weights=w)
        assert abs(l1 - l2) < 1e-6
        n = m1.flat_parameters().numel()
        nrow = chunk[0].shape[0] * int(chunk[4][0])
        g1 = t1.g[:n].cpu().numpy().astype(np.float64); g2 = t2.g[:n].cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(t2.g[n:].cpu().numpy(), np.array([nrow, 0, 0, 0], np.float32))
        np.testing.assert_allclose(g2, g1 * nrow, rtol=0, atol=2e-6 * np.abs(g1).max() * nrow)
    w1, w2 = m1.flat_parameters().cpu().numpy(), m2.flat_parameters().cpu().numpy()
    np.testing.assert_allclose(w2, w1, atol=2e-7, rtol=0)
    assert np.abs(w1 - flat).max() > 1e-5


def test_distillation_with_weights_equals_the_loop(cuda):
    """distill= plus weights and ignore_index: one step against the loop with distill_loss(..., sample_weights=, ignore_index=) at the trainer test's bounds"""
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, 11)
    m = util.build_model(TINY, w0, cuda).train()
    ref = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, distill={"alpha": 0.5, "temperature": 2.0}, ignore_index=7)
    opt = _RefAdam(ref, cuda, LR)
    chunk = _chunk(TINY, cuda, 81)
    w = _chunk_weights(cuda, chunk, 50)
    tl = _teacher_logits(cuda, chunk[0].shape[0], int(chunk[4][0]), TINY.n_quantize)
    loss = tr.step(*chunk, teacher_logits=tl, sample_weights=w)
    rl, g = _ref_grad(ref, chunk, w, teacher_logits=tl, ignore_index=7)
    opt.step(g)
    tr.check_status()
    wa, wr = m.flat_parameters().cpu().numpy(), ref.flat_parameters().cpu().numpy()
    print("DISTILL+WEIGHTS: loss %.7f, the loop's %.7f, max |w - w_loop| %.3e" % (loss, rl, np.abs(wa - wr).max()))
    assert abs(loss - rl) < 1e-4
    np.testing.assert_allclose(wa, wr, atol=2e-6, rtol=0)
    m3 = util.build_model(TINY, w0, cuda).train()
    FusedTrainer(m3, lr=LR, distill={"alpha": 0.5, "temperature": 2.0}).step(*chunk, teacher_logits=tl)
    assert np.abs(m3.flat_parameters().cpu().numpy() - wa).max() > 0.5 * LR


def test_h_grad_with_weights(cuda):
    """step(h_grad=, sample_weights=): the frames reached only by zero-weight rows are exact zeros (without the weights they are not); the rest match the loop's h.grad
    within tests/test_input_grad_gpu.py's bound, 1e-4 max |dh|"""
    import torch
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, 11)
    chunk = _chunk(TINY, cuda, 83, bl=1500)
    xt, ht, tt, dt, bt = chunk
    B, BL, U, F = xt.shape[0], int(bt[0]), TINY.upsampling_factor, ht.shape[2]
    maxd = int(torch.max(dt.ceil()))
    t0 = 900
    w = torch.rand((B, BL), generator=torch.Generator().manual_seed(4)).to(cuda) + 0.5
    w[:, :t0] = 0.0
    rf = TINY.receptiveA_field * maxd + TINY.receptiveF_field + TINY.receptiveCausal_field
    f0 = (F * U - BL + t0 - rf - 2) // U              # frames [0, f0) lie wholly below the first position a live row reads
    ffirst = (F * U - BL - rf) // U + 1               # ... and from ffirst on, rows of the chunk reach them
    assert f0 - ffirst >= 3, (f0, ffirst)
    plain, buf = torch.full_like(ht, 7.0), torch.full_like(ht, 7.0)
    FusedTrainer(util.build_model(TINY, w0, cuda).train(), lr=LR).step(*chunk, h_grad=plain)
    tr = FusedTrainer(util.build_model(TINY, w0, cuda).train(), lr=LR, label_smoothing=0.1)
    tr.step(*chunk, h_grad=buf, sample_weights=w)
    tr.check_status()
    ref = util.build_model(TINY, w0, cuda).train()
    _, _, dh = _ref_grad(ref, chunk, w, want_h_grad=True, label_smoothing=0.1)
    err, top = float((buf - dh).abs().max()), float(dh.abs().max())
    print("H_GRAD: frames [0, %d) exact zeros (plain there: max %.3e), max |dh - dh_loop| %.3e = %.3f of the bound" % (f0, float(plain[:, :, ffirst:f0].abs().max()), err, err / (1e-4 * top)))
    assert float(plain[:, :, ffirst:f0].abs().max()) > 0.0
    assert not bool((buf[:, :, :f0] != 0).any())
    assert top > 0 and err <= 1e-4 * top


def test_step_on_a_stream_with_late_weights(cuda, gate):
    """in the manner of tests/test_streams_gpu.py: on a non-blocking stream the weights buffer holds a decoy (all ones) until, behind a gate, the real weights are
    copied over it on that stream; step(want_loss=False) returns while the gate is closed, and the gradient it leaves is the one of the real weights (a reference
    trainer on the default stream) within 1e-6 max(1, |g|max); the decoy's gradient is more than 100 x that away"""
    import torch
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, 11)
    chunk = _chunk(TINY, cuda, 84)
    real = _chunk_weights(cuda, chunk, 60)
    grads = {}
    for name, w in (("real", real), ("decoy", torch.ones_like(real))):
        t = FusedTrainer(util.build_model(TINY, w0, cuda).train(), lr=1e-4, label_smoothing=0.1)
        t.step(*chunk, sample_weights=w)
        grads[name] = t.g[:-4].clone()
    bound = 1e-6 * max(1.0, float(grads["real"].abs().max()))
    assert float((grads["real"] - grads["decoy"]).abs().max()) > 100 * bound
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=1e-4, label_smoothing=0.1)
    buf = torch.ones_like(real)
    tr.step(*chunk, sample_weights=buf)               # the first call of a handle allocates: on the decoy, on the default stream
    tr.check_status()
    with torch.no_grad():
        m._flat.copy_(torch.from_numpy(w0).to(cuda))
    s = ST._start(cuda)
    with torch.cuda.stream(s):
        torch.cuda._sleep(gate.cycles)
        buf.copy_(real)
        tr.step(*chunk, want_loss=False, sample_weights=buf)
        ST._still_closed(s, "FusedTrainer.step(want_loss=False, sample_weights=...)")
        g = tr.g[:-4].clone()
    s.synchronize()
    tr.check_status()
    err = float((g - grads["real"]).abs().max())
    print("LATE WEIGHTS: max |g - g_real| %.3e (bound %.3e), the decoy's is %.3e away" % (err, bound, float((grads["real"] - grads["decoy"]).abs().max())))
    assert err <= bound


# ---------------------------------------------------------------- 11. capture
def test_a_captured_step_is_refused(cuda, monkeypatch):
    """a step with options on a capturing stream raises before anything is enqueued and leaves the handle unarmed (the capture state is stood in for, as in
    test_capture_with_a_window_is_refused: what is held is the trainer's refusal); the library's own refusal of an armed forward while capturing is QPN_ESTATE"""
    import torch
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, 11)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, label_smoothing=0.1)
    chunk = _chunk(TINY, cuda, 41, bl=600)
    w = _chunk_weights(cuda, chunk, 70)
    tr.step(*chunk, sample_weights=w)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="captured"):
            tr.step(*chunk, want_loss=False, sample_weights=w)
        with pytest.raises(RuntimeError, match="captured"):
            FusedTrainer(m).step(*chunk, want_loss=False, sample_weights=w)
    assert tr.step_count == 1
    # unarmed: a plain trainer on the same model and weights takes the same step as one on a model that never saw an option
    with torch.no_grad():
        m._flat.copy_(torch.from_numpy(w0).to(cuda))
    never = util.build_model(TINY, w0, cuda).train()
    la, lb = FusedTrainer(m, lr=LR).step(*chunk), FusedTrainer(never, lr=LR).step(*chunk)
    assert la == lb and float((m.flat_parameters() - never.flat_parameters()).abs().max()) <= 2e-7      # (an armed step's loss would differ in the third digit)
    assert np.isfinite(tr.step(*chunk, sample_weights=w)) and tr.step_count == 2


# ---------------------------------------------------------------- 12. the runner
def test_run_train_with_loss_options(cuda, tmp_path, caplog):
    """run_train --unvoiced_weight 0.25 --label_smoothing 0.05 on the three-utterance corpus of test_run_train_with_a_teacher: runs, logs both options, and its first
    losses differ from the plain run's; --unvoiced_weight 1 --label_smoothing 0 gives the plain run's loss values exactly (nothing is armed).  One loss per
    record (--intervals 1).  "Exactly" holds for the first loss, which no update precedes; the later ones pass through Adam updates whose backward sums with float
    atomics -- two plain runs differ there in the tenth digit (5.543925722 against 5.543925721 when this test was written) -- and are held to 1e-6, two units of the
    float32 loss at 5.5.  "Differ": by more than 1e-5, far above that noise (measured 5.5e-4 on the first record: smoothing barely moves an untrained model's loss)"""
    from qpnet_amd import runners
    root = DG._corpus(str(tmp_path / "corpus"))
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz", "--feature_format", "npy", "--batch_length", "1500",
              "--max_length", "4000", "--dilationA_depth", "1", "--dilationA_repeat", "1", "--dilationF_repeat", "1", "--n_resch", "32", "--n_skipch", "32",
              "--dilationF_depth", "2", "--iters", "3", "--intervals", "1", "--checkpoint_interval", "3"]

    def run(name, extra, verbose="0"):
        exp = str(tmp_path / name)
        assert runners.run_train(common + ["--expdir", exp, "--config", exp + "/model.conf", "--verbose", verbose, "--resume", exp + "/none.pkl"] + extra) == 0
        return yaml.safe_load(open(exp + "/loss-final.yml"))
    plain = run("plain", [])
    with caplog.at_level(logging.INFO):
        armed = run("armed", ["--unvoiced_weight", "0.25", "--label_smoothing", "0.05"], verbose="1")
    line = [r.getMessage() for r in caplog.records if "loss options:" in r.getMessage()]
    assert len(line) == 1 and "label_smoothing = 0.05" in line[0] and "unvoiced_weight = 0.25" in line[0], line
    neutral = run("neutral", ["--unvoiced_weight", "1", "--label_smoothing", "0"])
    print("RUNNER: plain %s, with options %s, neutral options %s" % (plain, armed, neutral))
    assert len(armed) == 3 and all(np.isfinite(armed)) and all(v > 0 for v in armed)
    assert abs(armed[0] - plain[0]) > 1e-5
    assert neutral[0] == plain[0] and len(neutral) == len(plain) and all(abs(a - b) <= 1e-6 for a, b in zip(neutral, plain))
    import torch
    from qpnet_amd import loaders
    a = torch.load(os.path.join(str(tmp_path / "armed"), "checkpoint-final.pkl"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(str(tmp_path / "plain"), "checkpoint-final.pkl"), map_location="cpu", weights_only=False)
    assert list(a.keys()) == list(b.keys()) and list(a["model"].keys()) == list(b["model"].keys())
    assert vars(loaders.load_model_conf(str(tmp_path / "armed") + "/model.conf")).keys() == vars(loaders.load_model_conf(str(tmp_path / "plain") + "/model.conf")).keys()
