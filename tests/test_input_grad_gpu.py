"""GPU parity of the feature gradient: h.grad from the training backward on every kernel path, FusedTrainer.step(h_grad=...), and the arm / disarm entry.

Yardstick, bound, inputs and the ReLU-kink condition: tests/input_grad_common.py (float64 oracle/train_torch.py::forward_row + torch.autograd.grad;
|dh - dh64| <= 1e-4 * max|dh64|, 2e-4 on the wide stacks; no input has a post-net unit within 4e-6 of zero -- tests/test_input_grad_cpu.py asserts it).  Logits,
loss and parameter gradients go through the helpers of tests/test_train_edges_gpu.py / tests/test_aux_geometry_gpu.py at their bounds.  Every check prints its
error as a fraction of the bound before it asserts (pytest -s / -rA shows them)."""
import os

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY
import util
import input_grad_common as IC
import test_train_edges_gpu as E
import test_aux_geometry_gpu as G
from test_streams_gpu import gate, _Late, _prime, _start, _still_closed          # noqa: F401  (gate: the module-scoped fixture, used below)

pytestmark = pytest.mark.gpu

F = np.float32
ALL = IC.CASES + IC.U0_CASES
FUSED_IDS = ["hoist-A39-U110-B2", "w160-A17-U120-B2"]


def _env(case, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)


def _compare(case):
    return G._compare_wide if case["wide"] else E._compare


def _model(o, cuda):
    m = util.build_model(o.cfg, o.flat, cuda).train()
    m.read_back_maxd = True                                   # the exact ceil(max d): N1 = recA * maxd + recF + BL, what IC.unreached counts with
    return m


def _forward(m, o, cuda):
    import torch
    xt, ht, tt, dt, bt = E._to(cuda, o.x, o.h, o.t, o.d, o.b)
    ht.requires_grad_()
    logits = m(xt, ht, dt, bt)
    loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, o.cfg.n_quantize), tt[:, -o.BL:].reshape(-1))
    return ht, logits, loss


def _flat_grad(m):
    import torch
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy()


def _fixture(cid, golden_dir):
    key = IC.FIXTURE_OF.get(cid)
    return None if key is None else np.load(os.path.join(golden_dir, "input_grad.npz"))[key + "_dh"]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- the autograd path, one case per kernel-selection row
@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_h_grad_autograd_vs_yardstick(case, cuda, golden_dir, monkeypatch):
    """model(x, h, d, b) -> CrossEntropyLoss -> backward(): h.grad against the float64 yardstick (and the reference's own h.grad where it is recorded), exact zeros where
    no row reaches; logits, loss and every parameter gradient as before.  Then the same backward once more through the C ABI into a buffer full of NaN: finite
    everywhere, the same gradient (a repeated backward of one forward runs a launch per layer: another kernel in front of the same contraction)."""
    import torch
    _env(case, monkeypatch)
    cid = case["id"]
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m = _model(o, cuda)
    ht, logits, loss = _forward(m, o, cuda)
    loss.backward()
    assert ht.grad is not None and ht.grad.shape == ht.shape and ht.grad.dtype == torch.float32
    dh = ht.grad.cpu().numpy()
    m.check_status()
    IC.check(cid + " autograd", dh, dh64, IC.rel(case))
    ref = _fixture(cid, golden_dir)
    if ref is not None:
        IC.check(cid + " autograd vs the reference's h.grad", dh, ref.astype(np.float64), IC.rel(case))
    mask = IC.unreached(o)
    assert np.array_equal(dh[mask], np.zeros(int(mask.sum()), F))
    _compare(case)(cid + " autograd (h requires grad)", o, logits.detach().cpu().numpy(), loss.item(), _flat_grad(m))
    # ... once more, straight through the ABI, into NaN
    L, hd = m._native(cuda)
    buf = torch.full_like(ht, float("nan"))
    dl, scratch = torch.from_numpy(np.array(o.dl)).to(cuda), torch.empty_like(m._flat)
    _lib.check(L.qpn_train_input_grad(hd, buf.data_ptr(), buf.numel()))
    _lib.check(L.qpn_train_backward(hd, dl.data_ptr(), scratch.data_ptr(), _stream()))
    dh2 = buf.cpu().numpy()
    IC.check(cid + " repeated backward into NaN", dh2, dh64, IC.rel(case))
    assert np.array_equal(dh2[mask], np.zeros(int(mask.sum()), F))


# ---------------------------------------------------------------- an upstream gradient that is not a cross entropy's
@pytest.mark.parametrize("cid", FUSED_IDS)
def test_h_grad_of_another_upstream_gradient(cid, cuda):
    import torch
    case = IC.BY_ID[cid]
    o = IC.input_of(cid)
    g = IC.fixed_g(o)
    want, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, g=g)
    m = _model(o, cuda)
    xt, ht, dt, bt = E._to(cuda, o.x, o.h, o.d, o.b)
    ht.requires_grad_()
    logits = m(xt, ht, dt, bt)
    (logits * torch.from_numpy(g).to(cuda)).sum().backward()
    m.check_status()
    IC.check(cid + " sum(g * logits)", ht.grad.cpu().numpy(), want, IC.rel(case))


# ---------------------------------------------------------------- a second backward of the same forward
def test_second_backward_of_one_forward_accumulates(cuda):
    cid = "hoist-A39-U110-B2"
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m = _model(o, cuda)
    ht, logits, loss = _forward(m, o, cuda)
    loss.backward(retain_graph=True)
    first = ht.grad.clone()
    g1 = _flat_grad(m)
    loss.backward()
    m.check_status()
    second = (ht.grad - first).cpu().numpy()
    IC.check(cid + " first backward", first.cpu().numpy(), dh64, IC.REL)
    IC.check(cid + " second backward (h.grad - first)", second, dh64, IC.REL)
    IC.check(cid + " accumulated h.grad", ht.grad.cpu().numpy(), 2.0 * dh64, IC.REL)
    np.testing.assert_allclose(_flat_grad(m), 2.0 * g1, rtol=0, atol=2e-4 * np.abs(g1).max())        # the parameters accumulate next to it, as torch does


# ---------------------------------------------------------------- only h requires a gradient
@pytest.mark.parametrize("cid", ["hoist-A39-U110-B2", "k176-A39-U5"])
def test_only_the_features_require_a_gradient(cid, cuda):
    """saliency: every parameter frozen, model.eval(); the backward runs whole (there is no input-only backward), the parameters get nothing"""
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m = _model(o, cuda).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    ht, logits, loss = _forward(m, o, cuda)
    assert logits.requires_grad
    loss.backward()
    IC.check(cid + " frozen parameters, eval()", ht.grad.cpu().numpy(), dh64, IC.REL)
    assert all(p.grad is None for p in m.parameters())
    m.check_status()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), o.lg, atol=2e-5, rtol=0)


# ---------------------------------------------------------------- FusedTrainer.step(h_grad=buf)
def _armed_step(o, cuda, lr):
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=lr)
    xt, ht, tt, dt = E._to(cuda, o.x, o.h, o.t, o.d)
    buf = torch.full_like(ht, float("nan"))
    loss = tr.step(xt, ht, tt, dt, o.b, want_loss=True, maxd=o.maxd, h_grad=buf)
    tr.check_status()
    return m, tr, loss, buf.cpu().numpy()


@pytest.mark.parametrize("cid", FUSED_IDS)
def test_fused_step_h_grad_is_taken_before_the_update(cid, cuda):
    """lr = 1e-2: the buffer holds d(mean CE) / dh at the weights the forward saw; the yardstick at the weights the step left is shown to lie outside the bound"""
    case = IC.BY_ID[cid]
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m, tr, loss, dh = _armed_step(o, cuda, 1e-2)
    assert abs(loss - o.loss) < 1e-4
    IC.check(cid + " fused step (lr 1e-2), weights before the step", dh, dh64, IC.rel(case))
    mask = IC.unreached(o)
    assert np.array_equal(dh[mask], np.zeros(int(mask.sum()), F))
    after, _ = IC.yardstick(o.cfg, m.flat_parameters().cpu().numpy(), o.x, o.h, o.d, o.BL, o.maxd, t=o.t)
    off = np.abs(after - dh64).max() / (IC.rel(case) * np.abs(dh64).max())
    print("DH   %-52s the yardstick at the weights after the step is %.0f x the bound away" % (cid, off))
    assert off > 20 and np.abs(dh - after).max() > 20 * IC.rel(case) * np.abs(dh64).max()


@pytest.mark.parametrize("cid", FUSED_IDS)
def test_armed_fused_step_leaves_the_same_weights_and_moments(cid, cuda):
    """an armed step on a freshly built model at lr = 1e-4, held to oracle/train_oracle.py::train_step the way test_train_edges_gpu._fused holds an unarmed one:
    loss, the step's gradient, the weights after the update (paper widths); the moments are the Adam launch's function of that gradient"""
    from oracle import train_oracle as TO
    case = IC.BY_ID[cid]
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m, tr, loss, dh = _armed_step(o, cuda, 1e-4)
    IC.check(cid + " fused step (lr 1e-4)", dh, dh64, IC.rel(case))
    g = tr.g[:o.flat.size].cpu().numpy()
    og = _compare(case)(cid + " armed fused step", o, None, loss, g)
    if not case["wide"]:
        wo = o.flat.copy()
        TO.Adam(wo.size).step(wo, og)
        util.assert_weights_after_adam(m.flat_parameters().cpu().numpy(), wo, 1e-4, 1, far=2.0, significant=util.significant_elements(o.cfg, [og]), sig_max=1e-6)
    opt = TO.Adam(g.size)
    opt.step(o.flat.copy(), g)
    np.testing.assert_allclose(tr.m.cpu().numpy(), opt.m, rtol=1e-5, atol=1e-12)
    # (the kernel forms 1 - beta2 in float32 from float32(0.999), the oracle rounds the float64 difference: float32(0.999) is up to 2^-25 = 3e-8 off, 3e-5 of 0.001)
    np.testing.assert_allclose(tr.v.cpu().numpy(), opt.v, rtol=1e-4, atol=1e-20)


def test_accumulation_micro_steps_each_get_their_own_chunks_gradient(cuda):
    """accum_steps = 2, chunks of different batch_length: every micro-step's buffer is ITS chunk's mean-CE gradient (the row-count weighting B * BL of the
    accumulated parameter gradient must not leak into it), and the closing update matches the oracle's Adam step on the union gradient, as
    tests/test_grad_accum_gpu.py checks it"""
    import torch
    from oracle import train_oracle as TO
    from qpnet_amd.train import FusedTrainer
    w0 = synth.make_weights(TINY, IC.ACC_WSEED)
    m = util.build_model(TINY, w0, cuda).train()
    tr = FusedTrainer(m, lr=1e-4, accum_steps=2)
    matched, rows = [], []
    for k in range(2):
        o = IC.acc_chunk(k)
        want, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, t=o.t)
        xt, ht, tt, dt = E._to(cuda, o.x, o.h, o.t, o.d)
        buf = torch.full_like(ht, float("nan"))
        loss = tr.step(xt, ht, tt, dt, o.b, want_loss=True, maxd=o.maxd, h_grad=buf)
        assert abs(loss - o.loss) < 1e-4
        IC.check("accumulation micro-step %d (BL %d)" % (k, o.BL), buf.cpu().numpy(), want, IC.REL)
        n = o.x.shape[0] * o.BL
        g = tr.g.cpu().numpy()
        np.testing.assert_array_equal(g[w0.size:], np.array([n, 0, 0, 0], F))
        matched.append(util.assert_grads_match_oracle(TO, TINY, o.flat, o.caches, o.dl, g[:w0.size] / F(n), og=o.og))
        rows.append(n)
    tr.check_status()
    assert tr.step_count == 1 and tr.micro_step == 0
    union = (sum(g.astype(np.float64) * n for g, n in zip(matched, rows)) / sum(rows)).astype(F)
    wo = w0.copy()
    TO.Adam(wo.size, lr=1e-4).step(wo, union)
    w = m.flat_parameters().cpu().numpy()
    util.assert_weights_after_adam(w, wo, 1e-4, 1)
    np.testing.assert_allclose(w, wo, atol=4e-6, rtol=0)


def test_a_captured_step_refuses_the_request(cuda, monkeypatch):
    import torch
    from qpnet_amd.train import FusedTrainer
    o = IC.acc_chunk(0)
    m = util.build_model(TINY, o.flat, cuda).train()
    tr = FusedTrainer(m)
    xt, ht, tt, dt = E._to(cuda, o.x, o.h, o.t, o.d)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        tr.step(xt, ht, tt, dt, o.b, maxd=o.maxd, h_grad=torch.empty_like(ht))
    assert tr.step_count == 0


# ---------------------------------------------------------------- arming
def test_arm_is_one_shot_disarm_disarms_and_a_wrong_n_is_refused(cuda):
    import torch
    cid = "hoist-A39-U110-B2"
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    m = _model(o, cuda)
    ht, logits, loss = _forward(m, o, cuda)
    L, hd = m._native(cuda)
    dl, scratch = torch.from_numpy(np.array(o.dl)).to(cuda), torch.empty_like(m._flat)
    buf = torch.full_like(ht, float("nan"))

    def backward():
        return L.qpn_train_backward(hd, dl.data_ptr(), scratch.data_ptr(), _stream())

    # armed, then disarmed: the backward writes nothing
    _lib.check(L.qpn_train_input_grad(hd, buf.data_ptr(), buf.numel()))
    _lib.check(L.qpn_train_input_grad(hd, None, 0))
    assert backward() == 0
    assert torch.isnan(buf).all()
    # a wrong n: that backward is refused, naming n, before it launches anything; the arm is dropped with it
    scratch.fill_(float("nan"))
    _lib.check(L.qpn_train_input_grad(hd, buf.data_ptr(), buf.numel() - 1))
    assert backward() == -1
    msg = L.qpn_last_error().decode()
    assert "n = %d" % (buf.numel() - 1) in msg and "%d" % buf.numel() in msg, msg
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and torch.isnan(scratch).all()
    assert backward() == 0                                    # the next, unarmed, backward works
    assert torch.isnan(buf).all() and torch.isfinite(scratch).all()
    np.testing.assert_allclose(scratch.cpu().numpy(), o.og, rtol=0, atol=2e-4 * np.abs(o.og).max())
    # one shot
    _lib.check(L.qpn_train_input_grad(hd, buf.data_ptr(), buf.numel()))
    assert backward() == 0
    IC.check(cid + " armed backward through the ABI", buf.cpu().numpy(), dh64, IC.REL)
    buf.fill_(float("nan"))
    assert backward() == 0
    assert torch.isnan(buf).all()
    m.check_status()


# ---------------------------------------------------------------- a non-blocking stream, inputs that arrive late
def test_fused_step_h_grad_on_a_stream_with_late_inputs(cuda, gate):
    """tests/test_streams_gpu.py's pattern: the device buffers hold a decoy until a gate on the step's own non-blocking stream opens; the step returns with the gate
    closed, and the buffer it fills holds the REAL input's gradient -- the side stream's launch is ordered behind the copies too"""
    import torch
    from qpnet_amd.train import FusedTrainer
    cid = "hoist-A39-U110-B2"
    o, dh64 = IC.input_of(cid), IC.dh64_ce(cid)
    dx, dhh, dt_, dd, db = util.distinct_rows_batch(o.cfg, 300, 61, 2500, 2)
    assert int(db[0]) == o.BL and int(np.ceil(dd).max()) == o.maxd
    decoy, _ = IC.yardstick(o.cfg, o.flat, dx, dhh, dd, o.BL, o.maxd, t=dt_)
    assert np.abs(decoy - dh64).max() > 100 * IC.REL * np.abs(dh64).max()
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4)
    late = _Late(cuda, (o.x, o.h, o.t, o.d), (dx, dhh, dt_, dd))
    xb, hb, tb, db_ = late.buf
    _prime(tr, late, o, cuda)                                   # set-up on the default stream: handle, workspace, code objects, the trainer's buffers
    buf = torch.full_like(hb, float("nan"))
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        tr.step(xb, hb, tb, db_, o.b, want_loss=False, maxd=o.maxd, h_grad=buf)
        _still_closed(s, "FusedTrainer.step(want_loss=False, h_grad=...)")
        got = buf.clone()
    s.synchronize()
    tr.check_status()
    IC.check(cid + " on a non-blocking stream, late inputs", got.cpu().numpy(), dh64, IC.REL)
