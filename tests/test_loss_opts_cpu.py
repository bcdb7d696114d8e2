"""The loss options without a GPU: the argument checks of qpn_ce_loss_opts / qpn_distill_loss_opts / qpn_train_loss_opts on a handle created without a device, the
ValueErrors of train.cross_entropy, FusedTrainer(ignore_index=, label_smoothing=, loss_norm=) and step(sample_weights=), the runner's flags, the uv -> row weight
mapping against a per-row loop, the float64 spec against torch, and the register report of the new kernels (no scratch memory)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from qpnet_amd import _lib, loaders, synth
from qpnet_amd.config import TINY
import loss_opts_spec as spec
import test_kernel_resources
import util

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(1 << 20)          # a stand-in device address (16-byte aligned): the checks below never read through it
NAN, INF = float("nan"), float("inf")


def _err():
    return _lib.lib().qpn_last_error().decode()


def _opts(w=None, n=0, use_ign=0, ign=0, eps=0.0, norm=0):
    return _lib.QpnLossOpts(w, n, use_ign, ign, eps, norm)


@pytest.fixture()
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    yield L, hp
    L.qpn_destroy(hp)


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(ROOT, "include", "qpnet_hip.h")) as f:
        hdr = f.read()
    assert "int qpn_train_loss_opts(qpn_handle* h, const qpn_loss_opts* opts);" in hdr
    assert re.search(r"typedef struct \{ const float\* d_weights; int64_t n_weights; int use_ignore; int64_t ignore_index;\s+float label_smoothing; int norm;", hdr)
    for name in ("qpn_ce_loss_opts", "qpn_distill_loss_opts", "qpn_train_loss_opts"):
        assert any(n == name for n, _, _ in _lib.SYMBOLS) and hasattr(_lib.lib(), name)
    # the ctypes mirror has the C struct's layout (x86-64 / LP64: 8, 8, 4 (+4), 8, 4, 4)
    assert C.sizeof(_lib.QpnLossOpts) == 40 and _lib.QpnLossOpts.ignore_index.offset == 24 and _lib.QpnLossOpts.norm.offset == 36


BAD_OPTS = [(dict(w=P, n=0), "n_weights"), (dict(w=P, n=-3), "n_weights"), (dict(eps=NAN), "label_smoothing"), (dict(eps=1.0), "label_smoothing"),
            (dict(eps=-0.01), "label_smoothing"), (dict(eps=INF), "label_smoothing"), (dict(norm=2), "norm"), (dict(norm=-1), "norm"),
            (dict(w=C.c_void_p((1 << 20) + 2), n=20), "4-byte")]


def test_arm_argument_checks_on_a_handle_without_a_gpu(handle):
    """checked before the device is looked at, QPN_EINVAL naming the argument; a default struct arms nothing; disarming always succeeds"""
    L, hp = handle
    assert L.qpn_train_loss_opts(None, C.byref(_opts(eps=0.1))) == -1 and "null handle" in _err()
    assert L.qpn_train_loss_opts(None, None) == -1 and "null handle" in _err()
    for kw, word in BAD_OPTS:
        assert L.qpn_train_loss_opts(hp, C.byref(_opts(**kw))) == -1 and word in _err(), (kw, _err())
    assert L.qpn_train_loss_opts(hp, C.byref(_opts())) == 0                          # entirely default: QPN_OK, nothing armed ...
    assert L.qpn_train_distill(hp, P, 8, 0.5, 2.0) == 0                              # ... so a teacher behind it is not "smoothing with a teacher"
    assert L.qpn_train_loss_opts(hp, C.byref(_opts(eps=0.1))) == -1 and "label_smoothing" in _err() and "teacher" in _err()
    assert L.qpn_train_loss_opts(hp, C.byref(_opts(w=P, n=20, use_ign=1, ign=-100, norm=1))) == 0      # weights + ignore compose with a teacher
    assert L.qpn_train_distill(hp, None, 0, 0.0, 1.0) == 0
    assert L.qpn_train_loss_opts(hp, C.byref(_opts(eps=0.999))) == 0
    assert L.qpn_train_distill(hp, P, 8, 0.5, 2.0) == -1 and "label_smoothing" in _err()       # the other order: the teacher is refused
    assert L.qpn_train_loss_opts(hp, None) == 0                                      # disarm
    assert L.qpn_train_distill(hp, P, 8, 0.5, 2.0) == 0 and L.qpn_train_distill(hp, None, 0, 0.0, 1.0) == 0
    assert L.qpn_train_loss_opts(hp, C.byref(_opts(w=P, n=20))) == 0
    import torch
    if not torch.cuda.is_available():
        assert L.qpn_train_forward_loss(hp, P, 1, 100, 1, 100, 10, 1, P, P, P, P, 10, P, 0, P, None) == -2      # QPN_ENODEV, as ever (the arm is gone with it)
    assert L.qpn_train_loss_opts(hp, None) == 0


def test_loss_argument_checks_on_a_handle_without_a_gpu(handle):
    L, hp = handle
    ok = dict(h=hp, lg=P, tg=P, stride=12, B=2, BL=10, dl=P)

    def call(opts="default", **kw):
        v = dict(ok, **kw)
        o = _opts(w=P, n=20, eps=0.1) if opts == "default" else opts
        return L.qpn_ce_loss_opts(v["h"], v["lg"], v["tg"], v["stride"], v["B"], v["BL"], None if o is None else C.byref(o), v["dl"], None, None)
    for kw, word in ((dict(h=None), "null handle"), (dict(lg=None), "d_logits"), (dict(tg=None), "d_targets"), (dict(opts=None), "opts"),
                     (dict(B=0), "B must"), (dict(BL=0), "BL must"), (dict(stride=9), "tgt_stride"), (dict(opts=_opts(w=P, n=19)), "n_weights"),
                     (dict(lg=C.c_void_p((1 << 20) + 8)), "16-byte")):
        assert call(**kw) == -1 and word in _err(), (kw, _err())
    for kw, word in BAD_OPTS:
        assert call(opts=_opts(**kw)) == -1 and word in _err(), (kw, _err())

    def dcall(o, a=0.5, T=2.0, tl=P):
        return L.qpn_distill_loss_opts(hp, P, tl, P, 12, 2, 10, a, T, None if o is None else C.byref(o), P, None, None)
    assert dcall(None) == -1 and "opts" in _err()
    assert dcall(_opts(w=P, n=20), tl=None) == -1 and "d_teacher" in _err()
    assert dcall(_opts(w=P, n=20), a=0.0) == -1 and "alpha" in _err()
    assert dcall(_opts(w=P, n=20, eps=0.1)) == -1 and "label_smoothing" in _err() and "teacher" in _err()
    assert dcall(_opts(w=P, n=21)) == -1 and "n_weights" in _err()
    for kw, word in BAD_OPTS:
        assert dcall(_opts(**kw)) == -1 and word in _err(), (kw, _err())
    import torch
    if not torch.cuda.is_available():
        assert call() == -2 and call(opts=_opts()) == -2 and call(dl=None) == -2     # valid calls: QPN_ENODEV, there is no CPU fallback
        assert dcall(_opts(w=P, n=20, use_ign=1, ign=3, norm=1)) == -2


def _cpu_batch():
    import torch
    x, h, t, d, b = synth.train_inputs(TINY, 100, 3, 1500)
    return [torch.from_numpy(a) for a in (x, h, t, d)] + [b]


def test_fused_trainer_refuses_bad_loss_options_at_construction():
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu")
    same = util.build_model(TINY, synth.make_weights(TINY, 12), "cpu")
    FusedTrainer(m, ignore_index=-100, label_smoothing=0.1, loss_norm="weights")
    FusedTrainer(m, label_smoothing=0.1, accum_steps=2, world_size=2)                 # "rows" combines over both
    for eps in (-0.1, 1.0, 2.0, NAN, INF, "0.1", None, 1.0 - 1e-9):                   # (1 - 1e-9 rounds to 1.0f)
        with pytest.raises(ValueError, match="label_smoothing"):
            FusedTrainer(m, label_smoothing=eps)
    for norm in ("mean", "row", 0, None, "Weights"):
        with pytest.raises(ValueError, match="norm"):
            FusedTrainer(m, loss_norm=norm)
    for ign in (1.5, "3", True, 2 ** 63):
        with pytest.raises(ValueError, match="ignore_index"):
            FusedTrainer(m, ignore_index=ign)
    with pytest.raises(ValueError, match="accum_steps=1 and world_size=1"):
        FusedTrainer(m, loss_norm="weights", accum_steps=2)
    with pytest.raises(ValueError, match="accum_steps=1 and world_size=1"):
        FusedTrainer(m, loss_norm="weights", world_size=2)
    with pytest.raises(ValueError, match="label_smoothing"):
        FusedTrainer(m, label_smoothing=0.1, distill={"teacher": same, "alpha": 0.5, "temperature": 2.0})
    FusedTrainer(m, ignore_index=3, distill={"teacher": same, "alpha": 0.5, "temperature": 2.0})
    assert m._handle is None and same._handle is None


def test_fused_trainer_refuses_bad_sample_weights_before_any_device_work():
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu")
    x, h, t, d, b = _cpu_batch()
    B, BL = x.shape[0], int(b[0])
    tr = FusedTrainer(m, label_smoothing=0.1)
    bad = [("Tensor", np.ones((B, BL), np.float32)), ("float32", torch.ones((B, BL), dtype=torch.float64)), ("shape", torch.ones((B, BL + 1))),
           ("shape", torch.ones((B * BL,))), ("shape", torch.ones((BL, B))), ("contiguous", torch.ones((B, 2 * BL))[:, ::2]), ("CUDA tensor", torch.ones((B, BL)))]
    for trainer in (tr, FusedTrainer(m)):
        for why, w in bad:
            with pytest.raises(ValueError, match=why):
                trainer.step(x, h, t, d, b, sample_weights=w)
    assert m._handle is None and tr.step_count == 0 and tr.m is None
    with pytest.raises(RuntimeError, match="AMD GPU only"):                # options set, CPU tensors: the refusal it always was, nothing was armed
        tr.step(x, h, t, d, b)
    assert m._handle is None


def test_cross_entropy_and_distill_loss_argument_errors_without_a_gpu():
    import torch
    from qpnet_amd.train import cross_entropy, distill_loss
    z, y = torch.zeros((2, 5, 16)), torch.zeros((2, 7), dtype=torch.int64)
    for kw, word in ((dict(norm="mean"), "norm"), (dict(label_smoothing=1.0), "label_smoothing"), (dict(label_smoothing=-1e-3), "label_smoothing"),
                     (dict(label_smoothing=NAN), "label_smoothing"), (dict(ignore_index=0.5), "ignore_index"), (dict(sample_weights=torch.ones((2, 6))), "sample_weights"),
                     (dict(sample_weights=[1.0] * 10), "sample_weights"), (dict(sample_weights=torch.ones((2, 5), dtype=torch.int64)), "sample_weights")):
        with pytest.raises(ValueError, match=word):
            cross_entropy(z, y, **kw)
    with pytest.raises(ValueError, match="expected"):
        cross_entropy(z, y[:, :4])                                         # targets shorter than BL
    with pytest.raises(ValueError, match="expected"):
        cross_entropy(z.view(10, 16), y)                                   # flattened logits need flattened targets
    with pytest.raises(ValueError, match="no CPU fallback"):
        cross_entropy(z, y, sample_weights=torch.ones((2, 5)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        cross_entropy(z.view(10, 16), y[:, -5:].reshape(-1))               # the reference's flattened pair is a valid shape
    with pytest.raises(ValueError, match="sample_weights"):
        distill_loss(z, z, y, 0.5, 2.0, sample_weights=torch.ones((3, 5)))
    with pytest.raises(ValueError, match="ignore_index"):
        distill_loss(z, z, y, 0.5, 2.0, ignore_index="x")


def _argv(tmp_path, extra):
    return ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", str(tmp_path / "exp"), "--config", str(tmp_path / "exp" / "model.conf")] + extra


def test_runner_flags_and_their_exits(tmp_path):
    from qpnet_amd import runners
    for update in (False, True):
        a = runners._train_args(update).parse_args(_argv(tmp_path, ["--pretrain", "x.pkl"] if update else []))
        assert (a.label_smoothing, a.unvoiced_weight) == (0.0, 1.0)
        a = runners._train_args(update).parse_args(_argv(tmp_path, (["--pretrain", "x.pkl"] if update else []) + ["--label_smoothing", "0.05", "--unvoiced_weight", "0.25"]))
        assert (a.label_smoothing, a.unvoiced_weight) == (0.05, 0.25)
    geo = ["--n_resch", "64", "--dilationF_repeat", "1"]
    for extra, word in ((["--label_smoothing", "1"], "--label_smoothing"), (["--label_smoothing", "-0.5"], "--label_smoothing"), (["--label_smoothing", "nan"], "--label_smoothing"),
                        (["--unvoiced_weight", "-1"], "--unvoiced_weight"), (["--unvoiced_weight", "inf"], "--unvoiced_weight"), (["--unvoiced_weight", "nan"], "--unvoiced_weight")):
        with pytest.raises(SystemExit, match=word):
            runners.run_train(_argv(tmp_path, geo + extra))
    assert not os.path.exists(str(tmp_path / "exp"))                                # nothing was started


def _row_loop(h, BL, U, W):
    """the mapping written out: output row t of a chunk is the chunk's position n - BL + t of the (upsampled) features, n positions in all"""
    B, _, F = h.shape
    n = F * U if U > 0 else F
    out = np.empty((B, BL), np.float32)
    for b in range(B):
        for t in range(BL):
            p = n - BL + t
            frame = p // U if U > 0 else p
            out[b, t] = 1.0 if h[b, 0, frame] == 1.0 else W
    return out


@pytest.mark.parametrize("U,F,BL", [(110, 9, 777), (110, 4, 440), (110, 3, 1), (0, 500, 333), (0, 64, 64), (7, 30, 100)])
def test_unvoiced_row_weights_against_a_per_row_loop(U, F, BL):
    """a chunk that starts mid-frame (BL no multiple of U: its first row lies inside a frame), U = 110 and U = 0"""
    rng = np.random.default_rng(U * 1000 + BL)
    h = rng.standard_normal((3, 5, F)).astype(np.float32)
    h[:, 0, :] = rng.integers(0, 2, (3, F)).astype(np.float32)
    for W in (0.25, 0.0, 3.0):
        got = loaders.unvoiced_row_weights(h, BL, U, W)
        assert got.dtype == np.float32 and got.shape == (3, BL)
        np.testing.assert_array_equal(got, _row_loop(h, BL, U, W))
    assert set(np.unique(loaders.unvoiced_row_weights(h, BL, U, 0.25))) <= {np.float32(0.25), np.float32(1.0)}
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match="unvoiced_weight"):
            loaders.unvoiced_row_weights(h, BL, U, bad)
    with pytest.raises(ValueError, match="batch_length"):
        loaders.unvoiced_row_weights(h, (F * U if U > 0 else F) + 1, U, 0.5)


def test_calc_stats_keeps_the_uv_column_binary():
    """what the mapping relies on: the scaler leaves column 0 at mean 0 / scale 1"""
    rng = np.random.default_rng(3)
    f = rng.standard_normal((200, 6))
    f[:, 0] = rng.integers(0, 2, 200)
    sc = loaders.calc_stats([f])
    assert sc.mean_[0] == 0.0 and sc.scale_[0] == 1.0
    np.testing.assert_array_equal(sc(f)[:, 0], f[:, 0])


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.7])
def test_spec_equals_torch_cross_entropy_in_float64(eps):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(17)
    R, Q = 61, 37
    z = rng.standard_normal((R, Q)) * 4.0
    y = rng.integers(0, Q, R)
    zt, yt = torch.from_numpy(z).requires_grad_(True), torch.from_numpy(y)
    # reduction="none": the row terms
    ce, g = spec.row_terms(z, y, eps)
    ref = F.cross_entropy(zt, yt, label_smoothing=eps, reduction="none")
    np.testing.assert_allclose(ce, ref.detach().numpy(), rtol=0, atol=1e-13)
    w = rng.uniform(0.0, 2.0, R)
    (ref * torch.from_numpy(w)).sum().backward()
    np.testing.assert_allclose(g * w[:, None], zt.grad.numpy(), rtol=0, atol=1e-14)
    L, dz, mass = spec.loss_and_grad(z, y, weights=w, label_smoothing=eps, norm="rows")
    assert abs(L - float((ref.detach() * torch.from_numpy(w)).sum()) / R) < 1e-13 and abs(mass - w.sum()) < 1e-12
    np.testing.assert_allclose(dz, zt.grad.numpy() / R, rtol=0, atol=1e-15)
    # mean with ignore_index: norm = "weights"
    for ign in (-100, 3):
        y2 = y.copy()
        y2[rng.random(R) < 0.3] = ign
        zt2 = torch.from_numpy(z).requires_grad_(True)
        ref2 = F.cross_entropy(zt2, torch.from_numpy(y2), ignore_index=ign, label_smoothing=eps)
        ref2.backward()
        L2, dz2, mass2 = spec.loss_and_grad(z, y2, ignore_index=ign, label_smoothing=eps, norm="weights")
        assert abs(L2 - float(ref2.detach())) < 1e-13 and mass2 == float((y2 != ign).sum())
        np.testing.assert_allclose(dz2, zt2.grad.numpy(), rtol=0, atol=1e-15)
    L0, dz0, m0 = spec.loss_and_grad(z, y, weights=np.zeros(R), norm="weights")
    assert L0 == 0.0 and m0 == 0.0 and not dz0.any()


def test_new_loss_kernels_keep_everything_in_registers():
    """hipcc's resource report of every instance of k_ce_hard<NV, true> and k_ce_soft<NV, true> and of k_weight_mass: 0 bytes of scratch memory; k_ce_soft's
    unweighted instances stay five; the plain criterion k_ce_hard<0, false> keeps its 8 waves per SIMD"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    kernels = test_kernel_resources._report("train_loss.hip")
    for stem, count, min_occ in (("k_ce_hardILi%dELb1E", 5, 3), ("k_ce_softILi%dELb1E", 5, 3), ("k_weight_mass", 1, 3), ("k_ce_softILi%dELb0E", 5, 3), ("k_ce_hardILi0ELb0E", 1, 8)):
        frags = tuple(stem % nv for nv in range(5)) if "%d" in stem else (stem,)
        hits = {k: v for k, v in kernels.items() if any(f in k for f in frags)}
        assert len(hits) == count, (stem, sorted(kernels))
        for name, r in sorted(hits.items()):
            print("LOSS_OPTS_KERNEL %s: %d VGPRs, %d bytes of scratch per lane, %d waves per SIMD"
                  % (name, r.get("VGPRs", -1), r.get("ScratchSize [bytes/lane]", -1), r.get("Occupancy [waves/SIMD]", -1)))
            assert r.get("ScratchSize [bytes/lane]", -1) == 0, name
            assert r.get("Occupancy [waves/SIMD]", -1) >= min_occ, name          # (a streaming kernel lives on loads in flight: k_ce_soft's rule)
    assert sum("k_ce_hard" in k for k in kernels) == 6 and sum("k_ce_soft" in k for k in kernels) == 10, sorted(kernels)
