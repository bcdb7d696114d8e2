"""Knowledge distillation without a GPU: the argument checks of qpn_distill_loss / qpn_train_distill on a handle created without a device, the ValueErrors of
FusedTrainer(distill=...) and step(teacher_logits=...), the runner's --teacher flags, the chunks train_generator cuts for two models at once, and the
register report of k_ce_soft's unweighted instances (no scratch memory)."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from cases import generator_corpus
from qpnet_amd import _lib, harness, loaders, synth
from qpnet_amd.config import TINY, PAPER, DEFAULT
import test_kernel_resources
import util

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().qpn_last_error().decode()


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(ROOT, "include", "qpnet_hip.h")) as f:
        hdr = f.read()
    assert "int qpn_train_distill(qpn_handle* h, const float* d_teacher, int64_t n, float alpha, float temperature);" in hdr
    assert "int qpn_distill_loss(qpn_handle* h, const float* d_logits, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL," in hdr
    for name in ("qpn_train_distill", "qpn_distill_loss"):
        assert any(n == name for n, _, _ in _lib.SYMBOLS) and hasattr(_lib.lib(), name)


@pytest.fixture()
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    yield L, hp
    L.qpn_destroy(hp)


P = C.c_void_p(1 << 20)          # a stand-in device address (16-byte aligned): the checks below never read through it
NAN, INF = float("nan"), float("inf")


def test_arm_argument_checks_on_a_handle_without_a_gpu(handle):
    """checked before the device is looked at, QPN_EINVAL naming the argument; disarming always succeeds"""
    L, hp = handle
    assert L.qpn_train_distill(None, P, 8, 0.5, 1.0) == -1 and "null handle" in _err()
    assert L.qpn_train_distill(None, None, 0, 0.5, 1.0) == -1 and "null handle" in _err()
    for n in (0, -5):
        assert L.qpn_train_distill(hp, P, n, 0.5, 1.0) == -1 and "n must be" in _err(), n
    for a in (0.0, -0.25, 1.0000001, 2.0, NAN, INF):
        assert L.qpn_train_distill(hp, P, 8, a, 1.0) == -1 and "alpha" in _err(), a
    for T in (0.0, -1.0, NAN, INF, -INF):
        assert L.qpn_train_distill(hp, P, 8, 0.5, T) == -1 and "temperature" in _err(), T
    assert L.qpn_train_distill(hp, C.c_void_p((1 << 20) + 4), 8, 0.5, 1.0) == -1 and "d_teacher" in _err()
    assert L.qpn_train_distill(hp, P, 8, 1.0, 1.0) == 0                  # alpha = 1 is inside (0, 1]
    assert L.qpn_train_distill(hp, P, 8, 1e-6, 1e-3) == 0
    assert L.qpn_train_distill(hp, None, 0, 0.5, 1.0) == 0
    assert L.qpn_train_distill(hp, None, -3, NAN, -1.0) == 0             # disarming: nothing else is looked at
    assert L.qpn_train_distill(hp, P, 8, 0.5, 2.0) == 0
    import torch
    if not torch.cuda.is_available():
        assert L.qpn_train_forward_loss(hp, P, 1, 100, 1, 100, 10, 1, P, P, P, P, 10, P, 0, P, None) == -2      # QPN_ENODEV, as ever (the arm is gone with it)


def test_loss_argument_checks_on_a_handle_without_a_gpu(handle):
    L, hp = handle
    ok = dict(h=hp, lg=P, tl=P, tg=P, stride=12, B=2, BL=10, a=0.5, T=2.0, dl=P)

    def call(**kw):
        v = dict(ok, **kw)
        return L.qpn_distill_loss(v["h"], v["lg"], v["tl"], v["tg"], v["stride"], v["B"], v["BL"], v["a"], v["T"], v["dl"], None, None)
    for kw, word in ((dict(h=None), "null handle"), (dict(lg=None), "d_logits"), (dict(tl=None), "d_teacher"), (dict(tg=None), "d_targets"),
                     (dict(B=0), "B must"), (dict(BL=0), "BL must"), (dict(stride=9), "tgt_stride"),
                     (dict(a=0.0), "alpha"), (dict(a=1.5), "alpha"), (dict(a=NAN), "alpha"), (dict(a=-1.0), "alpha"),
                     (dict(T=0.0), "temperature"), (dict(T=-2.0), "temperature"), (dict(T=NAN), "temperature"), (dict(T=INF), "temperature"),
                     (dict(tl=C.c_void_p((1 << 20) + 8)), "16-byte")):
        assert call(**kw) == -1 and word in _err(), (kw, _err())
    import torch
    if not torch.cuda.is_available():
        assert call() == -2                                              # a valid call: QPN_ENODEV, there is no CPU fallback
        assert call(dl=None) == -2


def _cpu_batch():
    import torch
    x, h, t, d, b = synth.train_inputs(TINY, 100, 3, 1500)
    return [torch.from_numpy(a) for a in (x, h, t, d)] + [b]


def test_fused_trainer_refuses_a_bad_distill_setting_at_construction():
    """ValueError before any device work: geometry the two models must share, alpha / temperature by the C call's rules after rounding to float32"""
    import dataclasses
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu")
    same = util.build_model(TINY, synth.make_weights(TINY, 12), "cpu")
    deeper = util.build_model(dataclasses.replace(TINY, dilationF_depth=3, n_resch=48), synth.make_weights(dataclasses.replace(TINY, dilationF_depth=3, n_resch=48), 12), "cpu")
    FusedTrainer(m, distill={"teacher": same, "alpha": 0.5, "temperature": 2.0})
    FusedTrainer(m, distill={"teacher": deeper, "alpha": 1.0, "temperature": 0.5})            # another stack and width: fine
    FusedTrainer(m, distill={"alpha": 0.5, "temperature": 2.0})                               # no teacher: step(teacher_logits=...) brings the logits
    for key, val in (("n_quantize", 128), ("n_aux", TINY.n_aux + 1), ("upsampling_factor", TINY.upsampling_factor + 10)):
        cfg = dataclasses.replace(TINY, **{key: val})
        other = util.build_model(cfg, synth.make_weights(cfg, 12), "cpu")
        with pytest.raises(ValueError, match=key):
            FusedTrainer(m, distill={"teacher": other, "alpha": 0.5, "temperature": 1.0})
    for a in (0.0, -0.1, 1.5, float("nan"), 1e-50, 1.0 + 1e-7):           # (1e-50 rounds to 0.0f; 1 + 1e-7 to the float32 above 1)
        with pytest.raises(ValueError, match="alpha"):
            FusedTrainer(m, distill={"teacher": same, "alpha": a, "temperature": 1.0})
    FusedTrainer(m, distill={"teacher": same, "alpha": 1.0 + 1e-9, "temperature": 1.0})       # rounds to 1.0f: inside
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39):        # (1e39 rounds to +inf)
        with pytest.raises(ValueError, match="temperature"):
            FusedTrainer(m, distill={"teacher": same, "alpha": 0.5, "temperature": T})
    for bad, word in (({"teacher": same, "alpha": 0.5}, "temperature"), ({"teacher": same, "temperature": 1.0}, "alpha"), ("yes", "dict"),
                      ({"teacher": same, "alpha": 0.5, "temperature": 1.0, "beta": 3}, "unknown"), ({"teacher": m, "alpha": 0.5, "temperature": 1.0}, "student itself"),
                      ({"teacher": object(), "alpha": 0.5, "temperature": 1.0}, "QPNet")):
        with pytest.raises(ValueError, match=word):
            FusedTrainer(m, distill=bad)
    assert m._handle is None and same._handle is None


def test_fused_trainer_refuses_bad_teacher_logits_before_any_device_work():
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), "cpu")
    x, h, t, d, b = _cpu_batch()
    B, BL, Q = x.shape[0], int(b[0]), TINY.n_quantize
    tr = FusedTrainer(m, distill={"alpha": 0.5, "temperature": 2.0})
    bad = [("Tensor", np.zeros((B, BL, Q), np.float32)), ("float32", torch.zeros((B, BL, Q), dtype=torch.float64)), ("shape", torch.zeros((B, BL + 1, Q))),
           ("shape", torch.zeros((B, Q, BL))), ("shape", torch.zeros((B * BL, Q))), ("contiguous", torch.zeros((B, BL, 2 * Q))[:, :, ::2]), ("CUDA tensor", torch.zeros((B, BL, Q)))]
    for why, tl in bad:
        with pytest.raises(ValueError, match=why):
            tr.step(x, h, t, d, b, teacher_logits=tl)
    with pytest.raises(ValueError, match="teacher_logits"):               # neither a teacher nor logits
        tr.step(x, h, t, d, b)
    plain = FusedTrainer(m)
    with pytest.raises(ValueError, match="distill"):                      # logits without alpha / temperature
        plain.step(x, h, t, d, b, teacher_logits=torch.zeros((B, BL, Q)))
    assert m._handle is None and tr.step_count == 0 and tr.m is None
    with pytest.raises(RuntimeError, match="AMD GPU only"):                # without the feature: the refusal it always was
        plain.step(x, h, t, d, b)


def _conf(cfg):
    return argparse.Namespace(feature_type="world", feature_format="npy", dense_factor=8, **cfg.kwargs())


def _argv(tmp_path, extra):
    return ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", str(tmp_path / "exp"), "--config", str(tmp_path / "exp" / "model.conf")] + extra


def test_runner_flags_and_their_exits(tmp_path):
    """--teacher & co.: defaults, the flags leave the Namespace a run pickles as its model configuration, and every misuse is a SystemExit before training starts"""
    from qpnet_amd import runners
    p = runners._train_args(False)
    a = p.parse_args(_argv(tmp_path, []))
    assert (a.teacher, a.teacher_config, a.distill_alpha, a.distill_temperature, a.teacher_ema) == (None, None, 0.5, 1.0, False)
    before = {k: v for k, v in vars(a).items() if k not in runners._DISTILL_FLAGS}
    assert runners._distill_of(a, None) is None
    assert vars(a) == before                                                       # what the run writes as model.conf is what it always wrote
    up = runners._train_args(True).parse_args(_argv(tmp_path, ["--pretrain", "x.pkl", "--teacher", "t.pkl", "--teacher_config", "t.conf", "--teacher_ema",
                                                               "--distill_alpha", "0.25", "--distill_temperature", "4"]))
    assert (up.teacher, up.teacher_config, up.distill_alpha, up.distill_temperature, up.teacher_ema) == ("t.pkl", "t.conf", 0.25, 4.0, True)
    ck, tconf = str(tmp_path / "teacher.pkl"), str(tmp_path / "teacher.conf")
    open(ck, "wb").close()
    loaders.save_model_conf(tconf, _conf(DEFAULT))
    geo = ["--n_resch", "64", "--dilationF_repeat", "1"]
    with pytest.raises(SystemExit, match="--teacher_config"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher", ck]))
    with pytest.raises(SystemExit, match="need --teacher"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher_config", tconf]))
    with pytest.raises(SystemExit, match="need --teacher"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher_ema"]))
    with pytest.raises(SystemExit, match="does not exist"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher", str(tmp_path / "none.pkl"), "--teacher_config", tconf]))
    for flag, val, word in (("--n_quantize", "128", "n_quantize"), ("--n_aux", "40", "n_aux"), ("--upsampling_factor", "80", "upsampling_factor")):
        with pytest.raises(SystemExit, match=word):
            runners.run_train(_argv(tmp_path, geo + [flag, val, "--teacher", ck, "--teacher_config", tconf]))
    with pytest.raises(SystemExit, match="alpha"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher", ck, "--teacher_config", tconf, "--distill_alpha", "0"]))
    with pytest.raises(SystemExit, match="temperature"):
        runners.run_train(_argv(tmp_path, geo + ["--teacher", ck, "--teacher_config", tconf, "--distill_temperature", "-1"]))
    assert not os.path.exists(str(tmp_path / "exp"))                                # nothing was started
    # a compatible pair: the teacher's configuration comes back loaded
    a = p.parse_args(_argv(tmp_path, geo + ["--teacher", ck, "--teacher_config", tconf, "--distill_temperature", "2"]))
    dd = runners._distill_of(a, argparse.Namespace(**vars(a)))
    assert dd["checkpoint"] == ck and dd["alpha"] == 0.5 and dd["temperature"] == 2.0 and dd["use_ema"] is False and dd["conf"].n_resch == DEFAULT.n_resch
    assert not any(hasattr(a, k) for k in runners._DISTILL_FLAGS)


def _sk_scaler(mean, scale):
    from sklearn.preprocessing import StandardScaler
    sc = StandardScaler()
    sc.mean_, sc.scale_ = mean, scale
    return sc.transform


@pytest.mark.parametrize("pair", [(TINY, PAPER), (PAPER, DEFAULT), (TINY, DEFAULT)], ids=["tiny-paper", "paper-default", "tiny-default"])
def test_chunks_cut_for_the_joint_fields_are_long_enough_for_both_models(pair):
    """train_generator given the element-wise maximum of two models' receptive fields: every chunk has T - BL >= each model's own receptive field under the chunk's
    largest dilated factor (what qpn_train_forward asks of a chunk), and the maximum is needed -- the smaller model's own fields cut chunks too short for the other"""
    from qpnet_amd.runners import joint_fields, _fields_of
    a, b = pair
    fields = joint_fields(a, b)
    assert fields == tuple(max(u, v) for u, v in zip(_fields_of(a), _fields_of(b)))
    pcm, feats, mean, scale = generator_corpus(64, [60, 45, 80, 52], [7, -130, 0, 250], (60.0, 300.0))
    utts = [(p.astype(np.float32) / 32768, f) for p, f in zip(pcm, feats)]

    def chunks(f, n=12):
        np.random.seed(5)
        gen = loaders.train_generator(utts, f[0], f[1], f[2], 22050, wav_transform=loaders.mu_law_transform(256), feat_transform=_sk_scaler(mean, scale),
                                      dense_factor=8, batch_length=1500, max_length=9000, batch_size=1, f0_threshold=0, upsampling_factor=110, shuffle=True)
        return [next(gen) for _ in range(n)]
    short = 0
    for f, joint in ((fields, True), (_fields_of(a), False)):
        for bx, bh, bt, bd, bb in chunks(f):
            T, BL = bx.shape[1], int(bb[0])
            for cfg in (a, b):
                rf = harness.receptive_field(cfg.receptiveCausal_field, cfg.receptiveF_field, cfg.receptiveA_field, np.asarray(bd))
                if joint:
                    assert T - BL >= rf, (T, BL, rf)
                    assert bd.shape[1] >= rf + BL - 1 and bh.shape[2] * 110 >= rf + BL - 1
                else:
                    short += T - BL < rf
    assert short > 0


def test_distill_kernel_keeps_everything_in_registers():
    """hipcc's resource report of every unweighted instance of k_ce_soft (rows of 256 .. 1024 classes in registers, and the looping one): 0 bytes of scratch
    memory, and at least three waves per SIMD -- a streaming kernel lives on loads in flight"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    kernels = test_kernel_resources._report("train_loss.hip")
    hits = {k: v for k, v in kernels.items() if any("k_ce_softILi%dELb0E" % nv in k for nv in range(5))}          # (k_ce_soft<NV, false>, as mangled)
    assert len(hits) == 5, sorted(kernels)
    for name, r in sorted(hits.items()):
        print("K_CE_SOFT %s: %d VGPRs, %d bytes of scratch per lane, %d waves per SIMD"
              % (name, r.get("VGPRs", -1), r.get("ScratchSize [bytes/lane]", -1), r.get("Occupancy [waves/SIMD]", -1)))
        assert r.get("ScratchSize [bytes/lane]", -1) == 0, name
        assert r.get("Occupancy [waves/SIMD]", -1) >= 3, name
