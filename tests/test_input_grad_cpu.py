"""The feature gradient (h.grad) without a GPU: the yardstick of tests/test_input_grad_gpu.py against the reference's own h.grad, the condition its inputs
have to meet, what the yardstick tells apart, and the argument checks of the arm / disarm entry and of FusedTrainer.step(h_grad=...).

Yardstick, bound and the kink condition: tests/input_grad_common.py.  Every check prints its figures before it asserts (pytest -s / -rA shows them)."""
import ctypes as C
import os

import numpy as np
import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY
import util
import input_grad_common as IC

ALL_IDS = [c["id"] for c in IC.CASES + IC.U0_CASES]


@pytest.mark.parametrize("cid", IC.FIXTURE_IDS)
def test_yardstick_reproduces_the_reference_h_grad(cid, golden_dir):
    """float64 forward_row + autograd against h.grad of the reference module itself (float32, CPU: tests/golden/input_grad.npz), within the bound of the GPU tests;
    the float32 noise of both -- the reference's and the yardstick's own at float32 -- is measured against the float64 yardstick and printed"""
    g = np.load(os.path.join(golden_dir, "input_grad.npz"))
    o = IC.input_of(cid)
    dh64 = IC.dh64_ce(cid)
    ref = g[cid + "_dh"]
    dh32, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, t=o.t, dtype="float32")
    scale = np.abs(dh64).max()
    print("DH   %-28s float32 noise against the float64 yardstick: the reference's %.2e, the yardstick's own %.2e of max|dh| = %.3e"
          % (cid, np.abs(ref - dh64).max() / scale, np.abs(dh32 - dh64).max() / scale, scale))
    IC.check(cid + " reference fixture vs float64 yardstick", ref, dh64, IC.REL)
    IC.check(cid + " float32 yardstick vs float64 yardstick", dh32, dh64, IC.REL)
    assert abs(float(g[cid + "_loss"]) - o.loss) < 1e-4


@pytest.mark.parametrize("cid", ALL_IDS)
def test_no_input_has_a_unit_near_a_relu_kink(cid):
    """every input of the GPU file: no post-net pre-activation of the numpy oracle's forward within kink_eps = 4e-6 of zero (no side to enumerate, no case to skip),
    the features cover the rows, and the exact-zero region is what the case's comment says"""
    o = IC.input_of(cid)
    c = IC.BY_ID[cid]
    assert IC.near_kink_units(o) == 0, (cid, IC.near_kink_units(o))
    N1 = o.cfg.receptiveA_field * o.maxd + o.cfg.receptiveF_field + o.BL
    F, U = o.h.shape[2], o.cfg.upsampling_factor
    assert (F * U if U > 0 else F) >= N1
    lead = int(IC.unreached(o)[0, 0].sum())
    if c["u0"]:
        assert F > N1 and lead == F - N1               # sample-rate features longer than the chunk's rows: leading columns no row reaches
    elif c["lead"]:
        assert lead > 16 and lead % 4 != 0           # whole tiles of k_dh_frames (four frames each) of zeros and a mixed one
    if U == 16:
        assert (F * U - N1) % U != 0
    dh = IC.dh64_ce(cid)
    assert not dh[IC.unreached(o)].any() and dh.any()


def test_the_other_inputs_of_the_gpu_file_meet_the_condition_too():
    """the accumulation test's two chunks (unequal batch_length) and what makes the exact-zero check bite: frames in front of the rows on each of the three kernels"""
    for k in range(2):
        assert IC.near_kink_units(IC.acc_chunk(k)) == 0, k
    assert IC.acc_chunk(0).BL != IC.acc_chunk(1).BL
    lead = {c["id"]: int(IC.unreached(IC.input_of(c["id"]))[0, 0].sum()) for c in IC.CASES + IC.U0_CASES}
    assert lead["hoist-A64-U16-B2-lead21"] > 16 and lead["w256-A65-U80"] >= 1 and lead["u0-tiny"] >= 1 and lead["u0-paper"] >= 1, lead


@pytest.mark.parametrize("cid", ["hoist-A39-U110-B2", "w160-A17-U120-B2"])
def test_the_yardstick_tells_the_mistakes_apart(cid):
    """in the yardstick alone: a dh without the last upsampling tap, without one layer's aux term, or weighted by the row count B * BL (the gscale of the
    data-parallel and accumulation steps) is off by far more than the bound"""
    o = IC.input_of(cid)
    c = IC.BY_ID[cid]
    dh = IC.dh64_ce(cid)
    scale, bound = np.abs(dh).max(), IC.rel(c) * np.abs(dh).max()
    U = o.cfg.upsampling_factor
    kw = dict(t=o.t)
    no_tap, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, zero_saved=[("upsampling.conv.weight", U - 1)], **kw)
    last = len(o.cfg.dilationsA) - 1
    no_layer, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, zero_saved=["auxA_1x1_sigmoid.%d.weight" % last, "auxA_1x1_tanh.%d.weight" % last], **kw)
    no_first, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, zero_saved=["auxF_1x1_sigmoid.0.weight", "auxF_1x1_tanh.0.weight"], **kw)
    scaled = dh * (o.x.shape[0] * o.BL)
    for what, v in (("last upsampling tap dropped", no_tap), ("last layer's aux term dropped", no_layer), ("first layer's aux term dropped", no_first), ("times gscale = B * BL", scaled)):
        e = np.abs(v - dh).max()
        print("DH   %-22s %-32s off by %.2e of max|dh| = %.0f x the bound" % (cid, what, e / scale, e / bound))
        assert e > 20 * bound, (what, e, bound)
    # ... and the mean-CE gradient at weights one Adam step of lr = 1e-2 further is another one (what a dh launched BEHIND the step's Adam would be)
    from oracle import train_oracle as TO
    w1 = o.flat.copy()
    TO.Adam(w1.size, lr=1e-2).step(w1, np.array(o.og))
    after, _ = IC.yardstick(o.cfg, w1, o.x, o.h, o.d, o.BL, o.maxd, **kw)
    e = np.abs(after - dh).max()
    print("DH   %-22s %-32s off by %.2e of max|dh| = %.0f x the bound" % (cid, "weights after an lr = 1e-2 step", e / scale, e / bound))
    assert e > 20 * bound


def test_the_upstream_gradient_case_is_not_a_cross_entropy():
    """sum(g * logits) with the fixed normal g: another dh than the mean CE's, by orders of magnitude"""
    cid = "hoist-A39-U110-B2"
    o = IC.input_of(cid)
    dg, _ = IC.yardstick(o.cfg, o.flat, o.x, o.h, o.d, o.BL, o.maxd, g=IC.fixed_g(o))
    assert np.abs(dg).max() > 100 * np.abs(IC.dh64_ce(cid)).max()


def test_header_declares_and_library_exports_the_entry():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "qpnet_hip.h")) as f:
        assert "int qpn_train_input_grad(qpn_handle* h, float* d_dh, int64_t n);" in f.read()
    assert any(name == "qpn_train_input_grad" for name, _, _ in _lib.SYMBOLS)
    assert hasattr(_lib.lib(), "qpn_train_input_grad")


def test_arm_and_disarm_argument_checks_on_a_handle_without_a_gpu():
    """checked before the device is looked at: a null handle and n < 1 with a destination are QPN_EINVAL, disarming always succeeds, and a backward without a
    device still reports the device (the arm is gone with it)"""
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    buf = (C.c_float * 8)()
    try:
        assert L.qpn_train_input_grad(None, buf, 8) == -1 and b"null handle" in L.qpn_last_error()
        assert L.qpn_train_input_grad(None, None, 0) == -1
        for n in (0, -5):
            assert L.qpn_train_input_grad(hp, buf, n) == -1 and b"n must be" in L.qpn_last_error(), n
        assert L.qpn_train_input_grad(hp, buf, 8) == 0
        assert L.qpn_train_input_grad(hp, None, 0) == 0
        assert L.qpn_train_input_grad(hp, None, -3) == 0          # disarming: n is not looked at
        assert L.qpn_train_input_grad(hp, buf, 8) == 0
        import torch
        if not torch.cuda.is_available():
            assert L.qpn_train_backward(hp, buf, buf, None) == -2     # QPN_ENODEV, as ever
    finally:
        L.qpn_destroy(hp)


def _cpu_batch():
    import torch
    from qpnet_amd import synth
    x, h, t, d, b = synth.train_inputs(TINY, 100, 3, 1500)
    return [torch.from_numpy(a) for a in (x, h, t, d)] + [b]


def test_fused_trainer_refuses_a_bad_h_grad_before_any_device_work():
    """wrong type, dtype, shape, layout or device: ValueError -- raised in front of the device check that refuses CPU tensors (RuntimeError), so no device work came first"""
    import torch
    from qpnet_amd import synth
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu")
    tr = FusedTrainer(m)
    x, h, t, d, b = _cpu_batch()
    bad = [("Tensor", np.zeros(tuple(h.shape), np.float32)), ("float32", torch.zeros(h.shape, dtype=torch.float64)), ("shaped like h", torch.zeros(h.shape[0], h.shape[1], h.shape[2] + 1)),
           ("shaped like h", torch.zeros(h.shape[0], h.shape[2], h.shape[1])), ("contiguous", torch.zeros(h.shape[0], h.shape[1], 2 * h.shape[2])[:, :, ::2]),
           ("CUDA tensor", torch.zeros(h.shape))]
    for why, hg in bad:
        with pytest.raises(ValueError, match=why):
            tr.step(x, h, t, d, b, h_grad=hg)
    assert m._handle is None and tr.step_count == 0 and tr.m is None          # nothing was created, counted or allocated
    with pytest.raises(RuntimeError, match="AMD GPU only"):                    # without the request: the refusal it always was
        tr.step(x, h, t, d, b)


def test_the_module_refuses_cpu_tensors_as_before_when_h_requires_grad():
    from qpnet_amd import synth
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu").train()
    x, h, t, d, b = _cpu_batch()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, h.clone().requires_grad_(), d, b)
