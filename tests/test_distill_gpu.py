"""GPU: knowledge distillation -- the soft-target loss kernel (qpn_distill_loss / k_ce_distill) against the float64 formula, the armed forward-with-loss
(qpn_train_distill) against its pieces, FusedTrainer(distill=...) against a loop of forward, train.distill_loss and backward, and run_train --teacher.

    L_row = (1 - alpha) CE(z, y) + alpha T^2 KL(softmax(t / T) || softmax(z / T))
    dL/dz = (1 - alpha) (softmax(z) - onehot(y)) + alpha T (softmax(z / T) - softmax(t / T))            ("Soft-target loss")

The reference is that formula in torch float64 on the CPU, from the same float32 inputs (_spec below).  Every check prints its figures before it asserts."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import yaml

from qpnet_amd import _lib, loaders, synth
from qpnet_amd.config import TINY, PAPER
import util

pytestmark = pytest.mark.gpu

B0, BL0 = 2, 37                       # 74 rows: five workgroups of 16, the last with empty wave slots
STRIDE0 = BL0 + 5
COMBOS = [(1.0, 1.0), (0.5, 2.0), (0.3, 0.5)]


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _spec(z, t, y, alpha, T):
    """the formula in float64: z, t (rows, Q) float32 CPU tensors, y (rows,) int64 -> (total, hard CE mean, T^2 KL mean, dL/dz per row -- NOT over the row count)"""
    import torch
    z, t = z.double(), t.double()
    rows, Q = z.shape
    lp = torch.log_softmax(z, 1)
    ce = -lp[torch.arange(rows), y]
    lpz, lpt = torch.log_softmax(z / T, 1), torch.log_softmax(t / T, 1)
    kl = (lpt.exp() * (lpt - lpz)).sum(1)
    onehot = torch.zeros_like(z); onehot[torch.arange(rows), y] = 1.0
    g = (1.0 - alpha) * (lp.exp() - onehot) + alpha * T * (lpz.exp() - lpt.exp())
    c, k = float(ce.mean()), float(T * T * kl.mean())
    return (1.0 - alpha) * c + alpha * k, c, k, g


@pytest.fixture(scope="module", params=[256, 96], ids=["Q256-vector", "Q96-scalar"])
def loss_case(request):
    """one handle and one set of inputs per class count, shared by the kernel tests: random logits with |z| <= 10, one peaked student row, one row where t == z"""
    import torch
    Q = request.param
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(300 + Q)
    z = rs.uniform(-10, 10, (B0, BL0, Q)).astype(np.float32)
    t = rs.uniform(-10, 10, (B0, BL0, Q)).astype(np.float32)
    z[0, 3] = -10.0; z[0, 3, Q // 3] = 10.0            # peaked: softmax = (1 - 2e-7 Q, 2e-9 ...)
    t[1, 5] = z[1, 5]                                   # this row's KL term and its gradient are exact zeros
    y = rs.randint(0, Q, (B0, STRIDE0)).astype(np.int64)
    y[0, STRIDE0 - BL0 + 3] = Q // 3
    L = _lib.lib()
    hp = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(L.qpn_create(C.byref(_lib.make_config(dataclasses.replace(TINY, n_quantize=Q))), C.byref(hp)))
    zt, tt, yt = _to(dev, z, t, y)
    yield dict(Q=Q, dev=dev, L=L, hp=hp, z=zt, t=tt, y=yt, z_cpu=torch.from_numpy(z).reshape(-1, Q), t_cpu=torch.from_numpy(t).reshape(-1, Q),
               y_cpu=torch.from_numpy(y[:, -BL0:]).reshape(-1))
    L.qpn_destroy(hp)


def _distill(c, teacher, alpha, T, want_parts=True):
    import torch
    dl = torch.full_like(c["z"], 7.0)
    parts = (C.c_double * 3)()
    with torch.cuda.device(c["dev"]):
        _lib.check(c["L"].qpn_distill_loss(c["hp"], c["z"].data_ptr(), teacher.data_ptr(), c["y"].data_ptr(), STRIDE0, B0, BL0, alpha, T, dl.data_ptr(),
                                           parts if want_parts else None, _stream(c["dev"])))
        _lib.check(c["L"].qpn_train_status(c["hp"], _stream(c["dev"])))
    return dl, list(parts)


@pytest.mark.parametrize("alpha,T", COMBOS, ids=["a1-T1", "a.5-T2", "a.3-T.5"])
def test_distill_loss_against_float64(loss_case, alpha, T):
    """all three loss components within 1e-4 (the project's loss tolerance); dL/dlogits * rows within 4 max(1, T) x the error qpn_ce_loss's own dL/dlogits * rows
    has against float64 on the same student logits (the extra term carries the factor T and two more exponentials per class; the yardstick is the existing
    kernel).  Measured on an MI355X: MEASUREMENTS.md, "Soft-target loss"."""
    import torch
    c = loss_case
    rows = B0 * BL0
    tot, ce, kl, g = _spec(c["z_cpu"], c["t_cpu"], c["y_cpu"], alpha, T)
    dl, parts = _distill(c, c["t"], alpha, T)
    print("DISTILL Q=%d alpha=%g T=%g: loss %.9f / %.9f / %.9f, float64 %.9f / %.9f / %.9f" % (c["Q"], alpha, T, parts[0], parts[1], parts[2], tot, ce, kl))
    # the yardstick: the existing cross-entropy kernel against float64
    dce = torch.empty_like(c["z"])
    with torch.cuda.device(c["dev"]):
        _lib.check(c["L"].qpn_ce_loss(c["hp"], c["z"].data_ptr(), c["y"].data_ptr(), STRIDE0, B0, BL0, dce.data_ptr(), None, _stream(c["dev"])))
    _, _, _, gce = _spec(c["z_cpu"], c["z_cpu"], c["y_cpu"], 1e-30, 1.0)          # (alpha -> 0: the plain cross entropy's gradient)
    yard = float((dce.cpu().reshape(-1, c["Q"]).double() * rows - gce).abs().max())
    err = float((dl.cpu().reshape(-1, c["Q"]).double() * rows - g).abs().max())
    print("DISTILL Q=%d alpha=%g T=%g: max |dL/dz * rows - float64| = %.3e, qpn_ce_loss's own %.3e, ratio %.2f (bound %g)"
          % (c["Q"], alpha, T, err, yard, err / yard, 4 * max(1.0, T)))
    assert abs(parts[0] - tot) < 1e-4 and abs(parts[1] - ce) < 1e-4 and abs(parts[2] - kl) < 1e-4
    assert yard > 0 and err <= 4 * max(1.0, T) * yard
    # without the host pointer the total stays on the device for qpn_train_loss
    dl2, _ = _distill(c, c["t"], alpha, T, want_parts=False)
    one = C.c_double(0)
    with torch.cuda.device(c["dev"]):
        _lib.check(c["L"].qpn_train_loss(c["hp"], C.byref(one), _stream(c["dev"])))
    assert torch.equal(dl, dl2) and abs(one.value - parts[0]) < 1e-12


@pytest.mark.parametrize("T", [1.0, 2.0, 0.5])
def test_teacher_equal_to_the_student_is_a_zero(loss_case, T):
    """teacher logits bitwise the student's and alpha = 1: |loss| <= 1e-6 and |dL/dlogits * rows| <= 1e-6 T everywhere (KL from log-probabilities)"""
    c = loss_case
    dl, parts = _distill(c, c["z"], 1.0, T)
    worst = float(dl.abs().max()) * B0 * BL0
    print("DISTILL Q=%d T=%g teacher == student: loss %.3e, max |dL/dz * rows| %.3e" % (c["Q"], T, parts[0], worst))
    assert abs(parts[0]) <= 1e-6 and abs(parts[2]) <= 1e-6 and worst <= 1e-6 * T


def test_two_calls_give_the_same_bits(loss_case):
    import torch
    c = loss_case
    a, pa = _distill(c, c["t"], 0.5, 2.0)
    b, pb = _distill(c, c["t"], 0.5, 2.0)
    assert torch.equal(a, b) and not bool((a == 7.0).any())
    assert abs(pa[0] - pb[0]) < 1e-12


def _two_row_batch(cfg, bl, cuda):
    x, h, t, d, b = synth.train_inputs(cfg, bl, 77, bl + 3000)
    x, h, t, d = np.repeat(x, 2, 0), np.repeat(h, 2, 0), np.repeat(t, 2, 0).copy(), np.repeat(d, 2, 0)
    x[1, -9:] = (x[1, -9:] + 11) % cfg.n_quantize                    # two different rows in the batch
    t[1, -5] = (t[1, -5] + 7) % cfg.n_quantize
    return _to(cuda, x, h, t, d) + [int(b[0]), int(np.ceil(d).max())]


def _teacher_logits(cuda, B, BL, Q, seed=9):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn((B, BL, Q), generator=g)).to(cuda)


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_armed_forward_equals_the_pieces(cfgname, cuda):
    """qpn_train_distill + qpn_train_forward_loss against qpn_train_forward, then qpn_distill_loss on those logits: same logits and dL/dlogits bit for bit, the loss
    up to the order of the partial sums, and the backward's flat gradient within 1e-6 max(1, |g|max) (test_fused_forward_loss_equals_forward_then_ce's bound)"""
    import torch
    from qpnet_amd.train import ensure_flat
    cfg = TINY if cfgname == "tiny" else PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 23), cuda)
    xt, ht, tt, dt, BL, maxd = _two_row_batch(cfg, 700 if cfgname == "tiny" else 1500, cuda)
    L, hd = m._native(cuda)
    flat = ensure_flat(m, cuda)
    B, T = xt.shape; Q = cfg.n_quantize
    tl = _teacher_logits(cuda, B, BL, Q)
    stream = _stream(cuda)
    alpha, temp = 0.5, 2.0
    lg0 = torch.empty((B, BL, Q), device=cuda); dl0 = torch.empty_like(lg0)
    lg1 = torch.full((B, BL, Q), 7.0, device=cuda); dl1 = torch.empty_like(lg0)
    p0, l1 = (C.c_double * 3)(), C.c_double(0)
    args = (hd, flat.data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr())
    _lib.check(L.qpn_train_forward(*args, lg0.data_ptr(), stream))
    _lib.check(L.qpn_distill_loss(hd, lg0.data_ptr(), tl.data_ptr(), tt.data_ptr(), tt.shape[1], B, BL, alpha, temp, dl0.data_ptr(), p0, stream))
    _lib.check(L.qpn_train_distill(hd, tl.data_ptr(), tl.numel(), alpha, temp))
    _lib.check(L.qpn_train_forward_loss(*args, tt.data_ptr(), tt.shape[1], lg1.data_ptr(), 1, dl1.data_ptr(), stream))
    _lib.check(L.qpn_train_loss(hd, C.byref(l1), stream))
    _lib.check(L.qpn_train_status(hd, stream))
    print("ARMED %s: loss %.12f, pieces %.12f (CE %.6f, T^2 KL %.6f)" % (cfgname, l1.value, p0[0], p0[1], p0[2]))
    assert torch.equal(lg0, lg1) and torch.equal(dl0, dl1)
    assert abs(p0[0] - l1.value) < 1e-12 and p0[2] > 0 and abs(p0[0] - ((1 - alpha) * p0[1] + alpha * p0[2])) < 1e-12
    g0 = torch.empty(flat.numel(), device=cuda); g1 = torch.empty_like(g0)
    _lib.check(L.qpn_train_backward(hd, dl1.data_ptr(), g1.data_ptr(), stream))
    _lib.check(L.qpn_train_forward(*args, lg0.data_ptr(), stream))
    _lib.check(L.qpn_train_backward(hd, dl0.data_ptr(), g0.data_ptr(), stream))
    torch.cuda.synchronize()
    assert float((g0 - g1).abs().max()) <= 1e-6 * max(1.0, float(g0.abs().max()))
    # as the fused step enqueues it (want_logits = 0, the backward follows): the armed forward writes the logits all the same, the backward computes the post-net itself
    lg2 = torch.full((B, BL, Q), 7.0, device=cuda); dl2 = torch.empty_like(lg0); g2 = torch.empty_like(g0)
    _lib.check(L.qpn_train_distill(hd, tl.data_ptr(), tl.numel(), alpha, temp))
    _lib.check(L.qpn_train_forward_loss(*args, tt.data_ptr(), tt.shape[1], lg2.data_ptr(), 2, dl2.data_ptr(), stream))
    _lib.check(L.qpn_train_backward(hd, dl2.data_ptr(), g2.data_ptr(), stream))
    _lib.check(L.qpn_train_status(hd, stream))
    assert torch.equal(lg2, lg0) and torch.equal(dl2, dl0)
    assert float((g0 - g2).abs().max()) <= 1e-6 * max(1.0, float(g0.abs().max()))


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_one_shot_and_the_default_is_untouched(cfgname, cuda):
    """the forward-with-loss after an armed one gives dL/dlogits and loss bit-identical to a never-armed model's (every loss slot of these shapes receives two
    partial sums at most: their order cannot show); a plain forward leaves the arm alone; a wrong n returns QPN_EINVAL, launches nothing and leaves the handle unarmed"""
    import torch
    from qpnet_amd.train import ensure_flat
    cfg = TINY if cfgname == "tiny" else PAPER
    xt, ht, tt, dt, BL, maxd = _two_row_batch(cfg, 700 if cfgname == "tiny" else 1500, cuda)
    B, T = xt.shape; Q = cfg.n_quantize
    tl = _teacher_logits(cuda, B, BL, Q)
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
    _lib.check(L.qpn_train_distill(hd, tl.data_ptr(), tl.numel(), 0.5, 2.0))
    _, _, dl_armed, loss_armed = fwd_loss(m)
    assert not torch.equal(dl_armed, dl_plain) and abs(loss_armed - loss_plain) > 1e-3
    rc, lg, dl, loss = fwd_loss(m)                                     # one shot: this one is the plain cross entropy again
    assert rc == 0 and torch.equal(dl, dl_plain) and loss == loss_plain
    if cfgname == "paper":
        assert float(lg.min()) == 7.0                                  # ... inside the post-net tile, as ever: the logits buffer is left alone
    # a plain forward computes no loss and leaves the arm alone
    _lib.check(L.qpn_train_distill(hd, tl.data_ptr(), tl.numel(), 0.5, 2.0))
    lg0 = torch.empty((B, BL, Q), device=cuda)
    _lib.check(L.qpn_train_forward(hd, ensure_flat(m, cuda).data_ptr(), B, T, ht.shape[2], dt.shape[1], BL, maxd, xt.data_ptr(), ht.data_ptr(), dt.data_ptr(), lg0.data_ptr(), stream))
    rc, _, dl, loss = fwd_loss(m)
    assert rc == 0 and torch.equal(dl, dl_armed) and abs(loss - loss_armed) < 1e-12
    # a wrong n
    _lib.check(L.qpn_train_distill(hd, tl.data_ptr(), tl.numel() - Q, 0.5, 2.0))
    rc, lg, dl, _ = fwd_loss(m)
    torch.cuda.synchronize()
    assert rc == -1 and " n = " in L.qpn_last_error().decode() and float(lg.min()) == 7.0 and float(lg.max()) == 7.0 and float(dl.min()) == 7.0
    rc, _, dl, loss = fwd_loss(m)
    assert rc == 0 and torch.equal(dl, dl_plain) and loss == loss_plain


LR = 1e-3


def _ref_grad(model, teacher, chunk, cuda, alpha, temp):
    """forward, train.distill_loss, backward on the drop-in module: (loss, flat gradient)"""
    import torch
    from qpnet_amd.train import distill_loss
    xt, ht, tt, dt, bt = chunk
    with torch.no_grad():
        tl = teacher(xt, ht, dt, bt).clone()
    for p in model.parameters():
        p.grad = None
    out = model(xt, ht, dt, bt)
    loss = distill_loss(out, tl, tt, alpha, temp)
    loss.backward()
    return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()


class _RefAdam:
    """torch.optim.Adam on a flat copy of the weights, written back into the module: the update of a loop `opt.step()` without any of the library's optimiser code"""
    def __init__(self, model, cuda, lr):
        import torch
        from qpnet_amd.train import ensure_flat
        self.model, self.cuda = model, cuda
        self.w = ensure_flat(model, cuda).clone().requires_grad_()
        self.opt = torch.optim.Adam([self.w], lr=lr)

    def step(self, g):
        import torch
        from qpnet_amd.train import ensure_flat
        self.w.grad = g.clone()
        self.opt.step()
        with torch.no_grad():
            ensure_flat(self.model, self.cuda).copy_(self.w)


def _chunk(cfg, cuda, seed, bl=700):
    x, h, t, d, b = synth.train_inputs(cfg, bl, seed, 30000)
    return _to(cuda, x, h, t, d) + [b]


BIGGER = dataclasses.replace(TINY, n_resch=48, dilationF_depth=4)       # a larger fixed stack (receptive field 15 against 3) at another width


@pytest.mark.parametrize("tname", ["same-geometry", "larger-stack"])
def test_fused_trainer_equals_the_loop(tname, cuda):
    """three steps of FusedTrainer(distill={"teacher": ...}) against forward, distill_loss autograd, backward and torch's Adam on the same chunks, within
    test_flat_adam_matches_torch_adam's 2e-6 at its lr; the teacher's weights are the same bits before and after.  larger-stack: the chunks are cut for the teacher"""
    import torch
    from qpnet_amd.train import FusedTrainer
    tcfg = TINY if tname == "same-geometry" else BIGGER
    assert tcfg.receptiveF_field >= TINY.receptiveF_field
    alpha, temp = 0.5, 2.0
    w0 = synth.make_weights(TINY, 11)
    teacher = util.build_model(tcfg, synth.make_weights(tcfg, 31), cuda)
    tw0 = teacher.flat_parameters().clone()
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=LR, distill={"teacher": teacher, "alpha": alpha, "temperature": temp})
    ref = util.build_model(TINY, w0, cuda).train()
    teacher2 = util.build_model(tcfg, synth.make_weights(tcfg, 31), cuda)
    opt = _RefAdam(ref, cuda, LR)
    for step in range(3):
        chunk = _chunk(tcfg, cuda, 80 + step)
        loss = tr.step(*chunk)
        rl, g = _ref_grad(ref, teacher2, chunk, cuda, alpha, temp)
        opt.step(g)
        print("TRAINER %s step %d: loss %.7f, the loop's %.7f" % (tname, step, loss, rl))
        assert abs(loss - rl) < 1e-4
    tr.check_status()
    w, wr = m.flat_parameters().cpu().numpy(), ref.flat_parameters().cpu().numpy()
    print("TRAINER %s: max |w - w_loop| %.3e, moved %.3e" % (tname, np.abs(w - wr).max(), np.abs(w - w0).max()))
    np.testing.assert_allclose(w, wr, atol=2e-6, rtol=0)
    assert np.abs(w - w0).max() > 1e-4
    assert torch.equal(teacher.flat_parameters(), tw0) and not any(p.grad is not None for p in teacher.parameters())
    # the soft-target term is in the update: the plain trainer ends somewhere else
    m3 = util.build_model(TINY, w0, cuda).train()
    t3 = FusedTrainer(m3, lr=LR)
    for step in range(3):
        t3.step(*_chunk(tcfg, cuda, 80 + step))
    assert np.abs(m3.flat_parameters().cpu().numpy() - w).max() > 0.5 * LR


def test_accumulation_window_equals_the_row_weighted_update(cuda):
    """accum_steps = 2, every micro-step armed: two windows of two chunks of unequal batch_length against the one-window equivalent of tests/test_grad_accum_gpu.py --
    per update the row-weighted mean of the two chunks' gradients (here: of the loop's distill_loss gradients), then Adam -- within that file's 4e-6 at lr = 1e-4"""
    import torch
    from qpnet_amd.train import FusedTrainer
    alpha, temp, lr = 0.3, 0.5, 1e-4
    w0 = synth.make_weights(TINY, 11)
    teacher = util.build_model(TINY, synth.make_weights(TINY, 31), cuda)
    teacher2 = util.build_model(TINY, synth.make_weights(TINY, 31), cuda)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=lr, accum_steps=2, distill={"teacher": teacher, "alpha": alpha, "temperature": temp})
    ref = util.build_model(TINY, w0, cuda).train()
    opt = _RefAdam(ref, cuda, lr)
    for w in range(2):
        gs, ns = [], []
        for k in range(2):
            chunk = _chunk(TINY, cuda, 90 + 2 * w + k, bl=600 + 150 * k)
            assert tr.micro_step == k
            loss = tr.step(*chunk)
            rl, g = _ref_grad(ref, teacher2, chunk, cuda, alpha, temp)
            assert abs(loss - rl) < 1e-4
            gs.append(g.double()); ns.append(chunk[0].shape[0] * int(chunk[4][0]))
        assert tr.micro_step == 0 and tr.step_count == w + 1
        opt.step(((ns[0] * gs[0] + ns[1] * gs[1]) / (ns[0] + ns[1])).float())
    tr.check_status()
    w, wr = m.flat_parameters().cpu().numpy(), ref.flat_parameters().cpu().numpy()
    print("ACCUM: max |w - w_ref| %.3e" % np.abs(w - wr).max())
    np.testing.assert_allclose(w, wr, atol=4e-6, rtol=0)
    assert np.abs(w - w0).max() > 1e-4


def test_world2_without_exchange_equals_world1_with_a_teacher(cuda):
    """test_world2_without_exchange_equals_world1 with distill set: no process group, the exchange is the identity -- world_size = 2 (forward-with-loss, backward_ex,
    Adam call by call) reproduces the one-call step, loss and weights"""
    import torch
    from qpnet_amd.train import FusedTrainer
    flat = synth.make_weights(TINY, 5)
    teacher = util.build_model(TINY, synth.make_weights(TINY, 31), cuda)
    m1 = util.build_model(TINY, flat, cuda).train()
    m2 = util.build_model(TINY, flat, cuda).train()
    dd = {"teacher": teacher, "alpha": 0.5, "temperature": 2.0}
    t1 = FusedTrainer(m1, lr=1e-4, world_size=1, distill=dd)
    t2 = FusedTrainer(m2, lr=1e-4, world_size=2, distill=dd)
    for step in range(3):
        chunk = _chunk(TINY, cuda, 70 + step, bl=600 + 37 * step)
        if step:
            assert float((m2.flat_parameters() - m1.flat_parameters()).abs().max()) <= 2e-7
            with torch.no_grad():
                m2._flat.copy_(m1._flat)
        l1 = t1.step(*chunk)
        l2 = t2.step(*chunk)
        assert abs(l1 - l2) < 1e-6
        n = m1.flat_parameters().numel()
        nrow = chunk[0].shape[0] * int(chunk[4][0])
        g1 = t1.g[:n].cpu().numpy().astype(np.float64); g2 = t2.g[:n].cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(t2.g[n:].cpu().numpy(), np.array([nrow, 0, 0, 0], np.float32))
        np.testing.assert_allclose(g2, g1 * nrow, rtol=0, atol=2e-6 * np.abs(g1).max() * nrow)
    w1, w2 = m1.flat_parameters().cpu().numpy(), m2.flat_parameters().cpu().numpy()
    np.testing.assert_allclose(w2, w1, atol=2e-7, rtol=0)
    assert np.abs(w1 - flat).max() > 1e-5


def test_a_non_finite_teacher_value_skips_the_update(cuda):
    """test_a_flagged_step_leaves_parameters_and_moments_alone with one inf in teacher_logits=: QpnError(-4) naming the teacher logits within two steps, parameters
    and moments untouched by the flagged step and by the clean one enqueued behind it; training goes on"""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), cuda).train()
    tr = FusedTrainer(m, lr=1e-3, distill={"alpha": 0.5, "temperature": 2.0})
    x, h, t, d, b = synth.train_inputs(TINY, 600, 41, 30000)
    xt, ht, tt, dt = _to(cuda, x, h, t, d)
    maxd = int(np.ceil(d).max())
    tl = _teacher_logits(cuda, x.shape[0], int(b[0]), TINY.n_quantize)
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, teacher_logits=tl)
    tr.flush_loss(); tr.check_status()
    w0, m0, v0 = m.flat_parameters().clone(), tr.m.clone(), tr.v.clone()
    bad = tl.clone(); bad[0, 17, 5] = float("inf")
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, teacher_logits=bad)
    tr.step(xt, ht, tt, dt, b, want_loss="lagged", maxd=maxd, teacher_logits=tl)
    tr.flush_loss()
    with pytest.raises(_lib.QpnError, match="teacher logits") as e:
        tr.check_status()
    assert e.value.code == -4
    assert torch.equal(m.flat_parameters(), w0) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0)
    assert tr.step_count == 1
    loss = tr.step(xt, ht, tt, dt, b, want_loss=True, maxd=maxd, teacher_logits=tl)
    assert np.isfinite(loss) and not torch.equal(m.flat_parameters(), w0) and tr.step_count == 2
    nan = tl.clone(); nan[0, 3, 200] = float("nan")
    with pytest.raises(_lib.QpnError, match="teacher logits"):
        tr.step(xt, ht, tt, dt, b, want_loss=True, maxd=maxd, teacher_logits=nan)          # checked in the call: its Adam launch applied nothing
    assert tr.step_count == 2


def test_a_captured_step_is_refused(cuda, monkeypatch):
    """a step with the soft-target loss on a capturing stream raises before anything is enqueued (the stream's capture state is stood in for, as in
    test_capture_with_a_window_is_refused: what is held is the trainer's refusal, not the runtime's capture)"""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), cuda).train()
    tr = FusedTrainer(m, distill={"alpha": 0.5, "temperature": 2.0})
    chunk = _chunk(TINY, cuda, 41, bl=600)
    tl = _teacher_logits(cuda, 1, int(chunk[4][0]), TINY.n_quantize)
    tr.step(*chunk, teacher_logits=tl)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="captured"):
            tr.step(*chunk, want_loss=False, teacher_logits=tl)
    assert tr.step_count == 1
    assert np.isfinite(tr.step(*chunk, teacher_logits=tl)) and tr.step_count == 2


def _corpus(root, n=3, frames=45):
    from scipy.io import wavfile
    U = TINY.upsampling_factor
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    rs = np.random.RandomState(5)
    feats = []
    for i in range(n):
        h = synth.make_features(frames + 3 * i, 700 + i)
        x = (rs.uniform(-0.8, 0.8, (frames + 3 * i) * U + 11) * 32767).astype(np.int16)
        wavfile.write("%s/wav/u%02d.wav" % (root, i), 22050, x)
        np.save("%s/feat/u%02d.npy" % (root, i), h)
        feats.append(h)
    st = loaders.calc_stats(feats)
    np.savez(root + "/stats.npz", mean=st.mean_, scale=st.scale_)
    return root


def test_run_train_with_a_teacher(cuda, tmp_path, caplog):
    """python -m qpnet_amd.run_train --teacher on the runner tests' synthetic corpus: a teacher with a larger fixed stack trained for two iterations, then a student
    against it -- finite losses, the start-up line, and checkpoints that hold exactly the keys of a run without a teacher"""
    import logging
    import torch
    from qpnet_amd import runners
    root = _corpus(str(tmp_path / "corpus"))
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz", "--feature_format", "npy", "--batch_length", "1500",
              "--max_length", "4000", "--dilationA_depth", "1", "--dilationA_repeat", "1", "--dilationF_repeat", "1"]
    small = ["--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2"]
    big, plain, exp = str(tmp_path / "big"), str(tmp_path / "plain"), str(tmp_path / "exp")
    assert runners.run_train(common + ["--n_resch", "48", "--n_skipch", "32", "--dilationF_depth", "4", "--expdir", big, "--config", big + "/model.conf", "--iters", "2",
                                       "--intervals", "1", "--ema_decay", "0.9", "--verbose", "0", "--resume", big + "/none.pkl"]) == 0
    assert runners.run_train(common + small + ["--expdir", plain, "--config", plain + "/model.conf", "--iters", "4", "--checkpoint_interval", "2", "--intervals", "2",
                                               "--verbose", "0", "--resume", plain + "/none.pkl"]) == 0
    with caplog.at_level(logging.INFO):
        assert runners.run_train(common + small + ["--expdir", exp, "--config", exp + "/model.conf", "--iters", "4", "--checkpoint_interval", "2", "--intervals", "2",
                                                   "--verbose", "1", "--resume", exp + "/none.pkl", "--teacher", big + "/checkpoint-final.pkl",
                                                   "--teacher_config", big + "/model.conf", "--teacher_ema", "--distill_alpha", "0.5", "--distill_temperature", "2"]) == 0
    line = [r.getMessage() for r in caplog.records if "distillation:" in r.getMessage()]
    assert len(line) == 1 and "alpha = 0.5" in line[0] and "T = 2" in line[0] and "distillation total" in line[0] and "(1, 15, 1)" in line[0] and "(1, 3, 1)" in line[0], line
    rec, rec0 = yaml.safe_load(open(exp + "/loss-final.yml")), yaml.safe_load(open(plain + "/loss-final.yml"))
    print("RUNNER: distillation totals %s, plain cross entropies %s" % (rec, rec0))
    assert len(rec) == 2 and all(np.isfinite(rec)) and all(v > 0 for v in rec)
    for name in ("checkpoint-2.pkl", "checkpoint-4.pkl", "checkpoint-final.pkl"):
        a = torch.load(os.path.join(exp, name), map_location="cpu", weights_only=False)
        b = torch.load(os.path.join(plain, name), map_location="cpu", weights_only=False)
        assert list(a.keys()) == list(b.keys()), name
        assert list(a["model"].keys()) == list(b["model"].keys()) and all(torch.isfinite(v).all() for v in a["model"].values())
        if a.get("optimizer"):
            assert list(a["optimizer"].keys()) == list(b["optimizer"].keys())
    assert vars(loaders.load_model_conf(exp + "/model.conf")).keys() == vars(loaders.load_model_conf(plain + "/model.conf")).keys()
