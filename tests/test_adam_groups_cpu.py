"""CPU: parameter groups of the fused Adam step (qpn_adam_groups) -- the pure table header under sanitizers, the C ABI's argument checks on a handle without
a GPU, the name-pattern -> table function, and the state_dict() layout of the grouped optimisers (tests/test_adam_groups_gpu.py holds the numerics).

tests/adam_groups_sweep.cpp includes only qpnet_amd/csrc/adam_groups.h: built with AddressSanitizer and UBSan as a program of its own and run as a child
process, as tests/test_train_plan_cpu.py does with its sweep."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY, PAPER, QPNetConfig, ADAM_FROZEN, adam_group_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -2


def test_table_header_sweep_under_sanitizers(tmp_path):
    """every element of hand-made and random tables gets the raw table's group through the normal form and the per-block index; every rejection rule rejects"""
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path / "adam_groups_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "adam_groups_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAM_GROUPS_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    words = r.stdout.split("ADAM_GROUPS_SWEEP_OK")[1].split()
    assert int(words[0]) >= 400 and int(words[2]) >= 100000 and int(words[4]) >= 20


# ---------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _call(L, hp, n_groups, lr, wd, seg_end, seg_group, n_seg=None):
    f = lambda a: None if a is None else (C.c_float * len(a))(*a)
    e = None if seg_end is None else (C.c_int64 * len(seg_end))(*seg_end)
    g = None if seg_group is None else (C.c_int32 * len(seg_group))(*seg_group)
    rc = L.qpn_adam_groups(hp, n_groups, f(lr), f(wd), len(seg_end) if n_seg is None else n_seg, e, g, None)
    return rc, L.qpn_last_error().decode()


GOOD = dict(n_groups=2, lr=[1e-3, 0.0], wd=[0.0, 1e-2], seg_end=[10, 20, 52591], seg_group=[0, ADAM_FROZEN, 1])
NAN, INF = float("nan"), float("inf")
BAD = [
    (dict(n_groups=-1), "n_groups"), (dict(n_groups=9), "n_groups"),
    (dict(lr=None), "h_lr"), (dict(wd=None), "h_weight_decay"), (dict(seg_end=None, n_seg=3), "h_seg_end"), (dict(seg_group=None), "h_seg_group"),
    (dict(lr=[NAN, 1e-3]), "h_lr[0]"), (dict(lr=[1e-3, INF]), "h_lr[1]"), (dict(lr=[-1e-3, 1e-3]), "h_lr[0]"),
    (dict(wd=[NAN, 0.0]), "h_weight_decay[0]"), (dict(wd=[0.0, INF]), "h_weight_decay[1]"), (dict(wd=[0.0, -0.5]), "h_weight_decay[1]"),
    (dict(n_seg=0), "n_seg"), (dict(n_seg=-1), "n_seg"), (dict(n_seg=2 ** 20 + 1), "n_seg"),
    (dict(seg_end=[0, 20, 30]), "h_seg_end[0]"), (dict(seg_end=[10, 10, 30]), "strictly ascending"), (dict(seg_end=[10, 30, 20]), "strictly ascending"),
    (dict(seg_group=[0, 2, 1]), "h_seg_group[1]"), (dict(seg_group=[-2, 0, 1]), "h_seg_group[0]"),
    (dict(seg_group=[ADAM_FROZEN] * 3), "no trainable segment"),
]


@pytest.mark.parametrize("change,word", BAD, ids=[w + "-" + "-".join(c) for c, w in BAD])
def test_bad_arguments_are_refused_before_the_device_naming_the_argument(change, word, handle):
    L, hp = handle
    rc, err = _call(L, hp, **dict(GOOD, **change))
    assert rc == EINVAL and word in err, (rc, err)


def test_valid_table_needs_a_device_and_off_does_not(handle):
    import torch
    L, hp = handle
    assert L.qpn_version() >= 1006
    assert _call(L, hp, 0, None, None, [], None, n_seg=0)[0] == 0              # off: nothing else is looked at, no device needed
    assert L.qpn_adam_groups(hp, 0, None, None, -5, None, None, None) == 0
    rc, err = _call(L, hp, **GOOD)
    if torch.cuda.is_available():
        assert rc == 0, err
        assert _call(L, hp, 0, None, None, [], None, n_seg=0)[0] == 0
    else:
        assert rc == ENODEV, (rc, err)
    assert L.qpn_adam_groups(None, 0, None, None, 0, None, None, None) == EINVAL


# ---------------------------------------------------------------- name patterns -> table
UP0 = QPNetConfig(n_resch=32, n_skipch=32, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=1, dilationA_repeat=1, upsampling_factor=0)
ADAPT = [(["causal.*", "dil*", "res*", "skip*"], ADAM_FROZEN), ("conv_post_2.*", 1)]


def _brute(cfg, key_group):
    """group of every element, from the layout alone"""
    out = []
    for k, shp in cfg.param_layout():
        out += [key_group[k]] * int(np.prod(shp))
    return np.array(out)


@pytest.mark.parametrize("cfg", [TINY, PAPER, UP0], ids=["tiny", "paper", "up0"])
def test_pattern_table_tiles_the_flat_vector(cfg):
    seg_end, seg_group, key_group = adam_group_table(cfg, ADAPT, 0)
    assert seg_end[-1] == cfg.n_params and seg_end[0] >= 1
    assert all(b > a for a, b in zip(seg_end, seg_end[1:])) and all(a != b for a, b in zip(seg_group, seg_group[1:]))
    assert list(key_group) == [k for k, _ in cfg.param_layout()]
    per_elem = np.repeat(seg_group, np.diff([0] + seg_end))
    assert np.array_equal(per_elem, _brute(cfg, key_group))
    import fnmatch
    for k, g in key_group.items():
        frozen = any(fnmatch.fnmatch(k, p) for p in ADAPT[0][0])
        assert g == (ADAM_FROZEN if frozen else 1 if k.startswith("conv_post_2.") else 0), k
    assert set(seg_group) == {ADAM_FROZEN, 0, 1}
    # no entries: one segment of the default group
    assert adam_group_table(cfg, [], 0)[:2] == ([cfg.n_params], [0])


@pytest.mark.parametrize("cfg", [TINY, PAPER], ids=["tiny", "paper"])
def test_one_element_bias_frozen_alone_is_a_segment_of_its_own(cfg):
    offs, n = cfg.param_offsets()
    o = offs["upsampling.conv.bias"][0]
    seg_end, seg_group, _ = adam_group_table(cfg, [("upsampling.conv.bias", ADAM_FROZEN)], 0)
    assert seg_end == [o, o + 1, n] and seg_group == [0, ADAM_FROZEN, 0]


def test_pattern_errors():
    with pytest.raises(ValueError, match=r"nothing\.\*.*matches no parameter"):
        adam_group_table(TINY, [(["conv_post_1.*", "nothing.*"], 1)], 0)
    with pytest.raises(ValueError, match=r"upsampling"):                     # (no upsampling layer in this geometry)
        adam_group_table(UP0, [("upsampling.*", ADAM_FROZEN)], 0)
    with pytest.raises(ValueError) as e:
        adam_group_table(TINY, [("conv_post_*", 1), ("*.bias", ADAM_FROZEN)], 0)
    msg = str(e.value)
    assert "conv_post_" in msg and ".bias" in msg and "'conv_post_*'" in msg and "'*.bias'" in msg and "two groups" in msg
    # two patterns of ONE entry may overlap
    adam_group_table(TINY, [(["conv_post_*", "conv_post_1.*"], 1)], 0)


# ---------------------------------------------------------------- optimisers on a CPU-constructed module
def _model():
    from qpnet_amd.qpnet import QPNet
    return QPNet(**TINY.kwargs())


def _torch_groups(m):
    named = dict(m.named_parameters())
    g1 = [p for k, p in named.items() if k.startswith("aux") or k.startswith("conv_post_1.")]
    g2 = [p for k, p in named.items() if k.startswith("conv_post_2.")]
    return [{"params": g1, "weight_decay": 1e-3}, {"params": g2, "lr": 5e-4}]


def _fill(m):
    """distinct, recognisable moments over the whole flat vector"""
    import torch
    n = sum(p.numel() for p in m.parameters())
    return torch.arange(n, dtype=torch.float32) * 1e-6, torch.arange(n, dtype=torch.float32) * 1e-9 + 1.0


def test_flat_adam_state_dict_is_that_of_torch_adam_with_the_same_groups():
    import torch
    from qpnet_amd.train import FlatAdam
    m = _model()
    fa = FlatAdam(m, _torch_groups(m), lr=1e-3)
    ta = torch.optim.Adam(_torch_groups(m), lr=1e-3)
    assert fa.param_groups[1]["lr"] == 5e-4 and fa.param_groups[0]["weight_decay"] == 1e-3 and fa.param_groups[0]["lr"] == 1e-3
    # the moments filled: ours by hand, torch's by a step on zero gradients
    fa._m, fa._v = _fill(m)
    fa._steps = 1
    for g in ta.param_groups:
        for p in g["params"]:
            p.grad = torch.zeros_like(p)
    ta.step()
    a, b = fa.state_dict(), ta.state_dict()
    assert len(a["param_groups"]) == len(b["param_groups"]) == 2
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert ga["params"] == gb["params"]
        for k in ("lr", "betas", "eps", "weight_decay"):
            assert ga[k] == gb[k]
        assert set(ga) <= set(gb)
    assert sorted(a["state"]) == sorted(b["state"]) == list(range(len(a["param_groups"][0]["params"]) + len(a["param_groups"][1]["params"])))
    for k in a["state"]:
        assert set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert a["state"][k]["exp_avg"].shape == b["state"][k]["exp_avg"].shape
    # entry k is the tensor torch numbers k: group order, then the group's own order
    params = list(m.parameters())
    pos = {id(p): i for i, p in enumerate(params)}
    offs = np.cumsum([0] + [p.numel() for p in params])
    k = 0
    for g in _torch_groups(m):
        for p in g["params"]:
            o = offs[pos[id(p)]]
            assert torch.equal(a["state"][k]["exp_avg"].reshape(-1), fa._m[o:o + p.numel()])
            k += 1
    # ... and each side loads the other's
    ta.load_state_dict(a)
    fb = FlatAdam(m, _torch_groups(m), lr=1e-3)
    fb.load_state_dict(a)
    assert torch.equal(fb._v, torch.where(_mask(fa, m), fa._v, torch.zeros(())))
    assert fb._steps == 1


def _mask(fa, m):
    """True on the elements some group holds"""
    import torch
    mask = torch.zeros(sum(p.numel() for p in m.parameters()), dtype=torch.bool)
    lo = 0
    for hi, g in zip(fa._groups.seg_end_list, fa._groups.seg_group_list):
        mask[lo:hi] = g >= 0
        lo = hi
    return mask


def test_flat_adam_group_rules():
    import torch
    from qpnet_amd.train import FlatAdam
    m = _model()
    gs = _torch_groups(m)
    with pytest.raises(ValueError, match="betas / eps must agree"):
        FlatAdam(m, [gs[0], dict(gs[1], betas=(0.8, 0.999))])
    with pytest.raises(ValueError, match="betas / eps must agree"):
        FlatAdam(m, [gs[0], dict(gs[1], eps=1e-6)])
    with pytest.raises(ValueError, match="not a parameter of this model"):
        FlatAdam(m, [{"params": [torch.nn.Parameter(torch.zeros(3))]}])
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="at most 8"):
        FlatAdam(m, [{"params": [p]} for p in ps[:9]])
    # parameters in no group are frozen: the table says so
    fa = FlatAdam(m, gs)
    assert fa._groups.seg_end_list[-1] == TINY.n_params and ADAM_FROZEN in fa._groups.seg_group_list
    assert fa._groups.n_trainable == sum(p.numel() for g in gs for p in g["params"]) and fa._groups.n_trainable + fa._groups.n_frozen == TINY.n_params


TRAINER_GROUPS = [{"params": ["causal.*", "dil*", "res*", "skip*", "upsampling.*"], "frozen": True}, {"params": "conv_post_2.*", "lr_scale": 0.5}]


def test_trainer_state_dict_with_groups_and_the_load_errors():
    import torch
    from qpnet_amd.train import FusedTrainer
    m = _model()
    tr = FusedTrainer(m, lr=1e-3, weight_decay=1e-4, param_groups=TRAINER_GROUPS)
    n = TINY.n_params
    tr.m, tr.v, tr.step_count = torch.zeros(n), torch.ones(n), 2
    sd = tr.state_dict()
    named = [k for k, _ in m.named_parameters()]
    dflt = [k for k in named if k.startswith("aux") or k.startswith("conv_post_1.")]
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(dflt), 2]
    assert sd["param_groups"][0]["lr"] == float(np.float32(1e-3)) and sd["param_groups"][1]["lr"] == float(np.float32(1e-3) * np.float32(0.5))
    assert sd["param_groups"][0]["weight_decay"] == sd["param_groups"][1]["weight_decay"] == 1e-4
    assert sorted(sd["state"]) == list(range(len(dflt) + 2))
    assert tr.n_trainable + tr.n_frozen == n and tr.n_frozen == sum(p.numel() for k, p in m.named_parameters() if k not in dflt and not k.startswith("conv_post_2."))
    # loads into a torch.optim.Adam built with the same groups, and into a trainer with them
    pd = dict(m.named_parameters())
    ta = torch.optim.Adam([{"params": [pd[k] for k in dflt]}, {"params": [pd["conv_post_2.weight"], pd["conv_post_2.bias"]]}], lr=1e-3)
    ta.load_state_dict(sd)
    tr2 = FusedTrainer(_model(), lr=5e-3, param_groups=TRAINER_GROUPS)
    tr2.load_state_dict(sd)
    assert tr2.step_count == 2 and abs(tr2.lr - 1e-3) < 1e-9
    # torch's rule: another number of groups, or a group of another size
    with pytest.raises(ValueError, match="different number of parameter groups"):
        FusedTrainer(_model(), param_groups=TRAINER_GROUPS[:1]).load_state_dict(sd)
    with pytest.raises(ValueError, match="different number of parameter groups"):
        tr2.load_state_dict(FusedTrainer(_model()).state_dict())
    with pytest.raises(ValueError, match="doesn't match the size"):
        FusedTrainer(_model(), param_groups=[TRAINER_GROUPS[0], {"params": "conv_post_2.bias", "lr_scale": 0.5}]).load_state_dict(sd)


def test_trainer_group_validation():
    from qpnet_amd.train import FusedTrainer
    with pytest.raises(ValueError, match="matches no parameter"):
        FusedTrainer(_model(), param_groups=[{"params": "nope*", "frozen": True}])
    with pytest.raises(ValueError, match="two groups"):
        FusedTrainer(_model(), param_groups=[{"params": "conv_post_*", "frozen": True}, {"params": "*.bias", "lr_scale": 2.0}])
    with pytest.raises(ValueError, match="every parameter is frozen"):
        FusedTrainer(_model(), param_groups=[{"params": "*", "frozen": True}])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lr_scale"):
            FusedTrainer(_model(), param_groups=[{"params": "conv_post_2.*", "lr_scale": bad}])
        with pytest.raises(ValueError, match="weight_decay"):
            FusedTrainer(_model(), param_groups=[{"params": "conv_post_2.*", "weight_decay": bad}])
    with pytest.raises(ValueError, match="param_groups entries"):
        FusedTrainer(_model(), param_groups=[{"params": "conv_post_2.*", "lr": 1e-3}])
    keys = [k for k, _ in _model().named_parameters()]
    with pytest.raises(ValueError, match="at most 8"):
        FusedTrainer(_model(), param_groups=[{"params": k, "lr_scale": 2.0} for k in keys[:8]])


def test_without_groups_the_state_dict_is_what_it_was():
    """byte for byte: the serialised state of an ungrouped trainer / FlatAdam equals the one built by the layout rule that predates groups (one group, every
    parameter in order, state keyed 0 .. P-1)"""
    import io
    import torch
    from qpnet_amd.train import FusedTrainer, FlatAdam, _ADAM_GROUP_DEFAULTS
    m = _model()
    n = TINY.n_params
    mm, vv = torch.arange(n, dtype=torch.float32) * 1e-6, torch.arange(n, dtype=torch.float32) * 1e-9
    tr = FusedTrainer(m, lr=1e-4)
    tr.m, tr.v, tr.step_count = mm, vv, 3
    fa = FlatAdam(m, lr=1e-4)
    fa._m, fa._v, fa._steps = mm, vv, 3
    state, o = {}, 0
    params = list(m.parameters())
    for i, p in enumerate(params):
        k = p.numel()
        state[i] = {"step": torch.tensor(3.0), "exp_avg": mm[o:o + k].view(p.shape).clone(), "exp_avg_sq": vv[o:o + k].view(p.shape).clone()}
        o += k
    group = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    group.update(_ADAM_GROUP_DEFAULTS)
    group["params"] = list(range(len(params)))
    want = {"state": state, "param_groups": [group]}

    def blob(sd):
        b = io.BytesIO()
        torch.save(sd, b)
        return b.getvalue()
    assert blob(tr.state_dict()) == blob(want) and blob(fa.state_dict()) == blob(want)
    assert list(tr.state_dict()["param_groups"][0]) == list(want["param_groups"][0])


_REQUIRED = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e", "--config", "c"]


@pytest.mark.parametrize("update", [False, True])
def test_runner_flags(update):
    from qpnet_amd import runners
    extra = ["--pretrain", "p"] if update else []
    args = runners._train_args(update).parse_args(_REQUIRED + extra)
    assert args.freeze is None and args.lr_scale == [] and runners._param_groups_of(args) is None
    args = runners._train_args(update).parse_args(_REQUIRED + extra + ["--freeze", "causal.*,dil*", "--lr_scale", "conv_post_2.*=0.5", "--lr_scale", "aux*,conv_post_1.*=2"])
    assert runners._param_groups_of(args) == [{"params": ["causal.*", "dil*"], "frozen": True}, {"params": ["conv_post_2.*"], "lr_scale": 0.5},
                                               {"params": ["aux*", "conv_post_1.*"], "lr_scale": 2.0}]
    for bad in ("conv_post_2.*", "=0.5", "conv_post_2.*=fast"):
        with pytest.raises(SystemExit):
            runners._param_groups_of(runners._train_args(update).parse_args(_REQUIRED + extra + ["--lr_scale", bad]))


def test_constants_are_the_same_in_both_headers_in_python_and_in_the_library(handle):
    """QPN_ADAM_MAX_GROUPS / QPN_ADAM_FROZEN are written down in include/qpnet_hip.h, qpnet_amd/csrc/adam_groups.h and qpnet_amd/config.py: the three agree, and
    the library behaves by them (MAX groups accepted, MAX + 1 refused; FROZEN a valid group id, FROZEN - 1 not)"""
    import re
    import torch
    from qpnet_amd import config, train
    vals = []
    for rel in ("include/qpnet_hip.h", "qpnet_amd/csrc/adam_groups.h"):
        text = open(os.path.join(ROOT, rel)).read()
        vals.append(tuple(int(re.search(r"#define %s \(?(-?\d+)\)?" % name, text).group(1)) for name in ("QPN_ADAM_MAX_GROUPS", "QPN_ADAM_FROZEN")))
    assert vals[0] == vals[1] == (config.ADAM_MAX_GROUPS, config.ADAM_FROZEN) == (train.ADAM_MAX_GROUPS, train.ADAM_FROZEN)
    L, hp = handle
    M, FRZ = config.ADAM_MAX_GROUPS, config.ADAM_FROZEN
    passed = 0 if torch.cuda.is_available() else ENODEV
    table = dict(seg_end=[10, 20, 30], seg_group=[M - 1, FRZ, 0])
    assert _call(L, hp, M, [1e-3] * M, [0.0] * M, **table)[0] == passed
    rc, err = _call(L, hp, M + 1, [1e-3] * (M + 1), [0.0] * (M + 1), **table)
    assert rc == EINVAL and "n_groups" in err
    rc, err = _call(L, hp, M, [1e-3] * M, [0.0] * M, seg_end=[10, 20, 30], seg_group=[M - 1, FRZ - 1, 0])
    assert rc == EINVAL and "h_seg_group[1]" in err
    assert L.qpn_adam_groups(hp, 0, None, None, 0, None, None, None) == 0


def test_flat_adam_add_param_group_rebuilds_the_table():
    import torch
    from qpnet_amd.train import FlatAdam
    m = _model()
    gs = _torch_groups(m)
    fa = FlatAdam(m, gs, lr=1e-3)
    before = (fa._groups.n_groups, fa._groups.n_trainable, list(fa._groups.seg_group_list))
    named = dict(m.named_parameters())
    extra = [named["causal.conv.weight"], named["causal.conv.bias"]]
    fa.add_param_group({"params": extra, "lr": 2e-4})
    assert len(fa.param_groups) == 3 and fa._groups.n_groups == 3 and len(fa._groups.positions) == 3
    assert fa._groups.n_trainable == before[1] + sum(p.numel() for p in extra)
    assert fa._groups.seg_group_list[0] == 2 and fa._groups.seg_end_list[0] == sum(p.numel() for p in extra)
    sd = fa.state_dict()
    ta = torch.optim.Adam(_torch_groups(m), lr=1e-3)
    ta.add_param_group({"params": extra, "lr": 2e-4})
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ta.state_dict()["param_groups"]] and sd["param_groups"][2]["lr"] == 2e-4
    # a group the constructor would refuse is refused here too, and leaves the optimiser as it was
    with pytest.raises(ValueError, match="betas / eps must agree"):
        fa.add_param_group({"params": [named["upsampling.conv.bias"]], "eps": 1e-3})
    with pytest.raises(ValueError, match="not a parameter of this model"):
        fa.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    assert len(fa.param_groups) == 3 and fa._groups.n_groups == 3
    # without groups the optimiser is what it always was
    plain = FlatAdam(m, lr=1e-3)
    assert plain._groups is None and len(plain.param_groups) == 1


def test_trainer_load_with_groups_takes_the_files_weight_decay_and_lr():
    import torch
    from qpnet_amd.train import FusedTrainer
    n = TINY.n_params
    src = FusedTrainer(_model(), lr=2e-3, weight_decay=3e-4, param_groups=TRAINER_GROUPS)
    src.m, src.v, src.step_count = torch.zeros(n), torch.ones(n), 5
    sd = src.state_dict()
    dst = FusedTrainer(_model(), lr=7e-2, weight_decay=0.5, param_groups=TRAINER_GROUPS)
    dst.load_state_dict(sd)
    assert dst.step_count == 5 and abs(dst.lr - 2e-3) < 1e-9 and dst.wd == 3e-4
    assert dst._group_values()[0] == src._group_values()[0] and dst._group_values()[1] == src._group_values()[1]
    # no default group in the file (every tensor claimed): lr comes back through the first scale that is not 0, the trainer's weight_decay stays
    allg = [{"params": ["causal.*", "upsampling.*", "dil*", "res*", "skip*", "aux*", "conv_post_1.*"], "lr_scale": 0.0}, {"params": "conv_post_2.*", "lr_scale": 0.25, "weight_decay": 0.0}]
    src = FusedTrainer(_model(), lr=2e-3, weight_decay=3e-4, param_groups=allg)
    src.m, src.v, src.step_count = torch.zeros(n), torch.ones(n), 1
    dst = FusedTrainer(_model(), lr=7e-2, weight_decay=0.5, param_groups=allg)
    dst.load_state_dict(src.state_dict())
    assert abs(dst.lr - 2e-3) < 1e-9 and dst.wd == 0.5
