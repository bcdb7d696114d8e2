"""CPU: the gradient-norm clipping option's arguments and what it must not change (tests/test_grad_clip_gpu.py holds the numerics)."""
import pytest

from qpnet_amd.config import TINY

_REQUIRED = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e", "--config", "c"]


@pytest.mark.parametrize("update", [False, True])
def test_runner_arguments(update):
    from qpnet_amd import runners
    extra = ["--pretrain", "p"] if update else []
    args = runners._train_args(update).parse_args(_REQUIRED + extra)
    assert args.max_grad_norm == 0.0 and isinstance(args.max_grad_norm, float)
    args = runners._train_args(update).parse_args(_REQUIRED + extra + ["--max_grad_norm", "2.5"])
    assert args.max_grad_norm == 2.5


def _model():
    from qpnet_amd.qpnet import QPNet
    return QPNet(**TINY.kwargs())


@pytest.mark.parametrize("kind", ["trainer", "flat_adam"])
def test_max_grad_norm_validation(kind):
    from qpnet_amd.train import FlatAdam, FusedTrainer
    make = (lambda **kw: FusedTrainer(_model(), **kw)) if kind == "trainer" else (lambda **kw: FlatAdam(_model(), **kw))
    for off in (None, 0, 0.0):
        assert make(max_grad_norm=off).max_grad_norm == 0.0
    assert make().max_grad_norm == 0.0
    assert make(max_grad_norm=5).max_grad_norm == 5.0
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            make(max_grad_norm=bad)


def test_state_dict_does_not_carry_the_setting():
    """max_grad_norm is a trainer setting: checkpoints keep torch.optim.Adam's layout, key for key."""
    import torch
    from qpnet_amd.train import FlatAdam, FusedTrainer
    sds = []
    for clip in (None, 3.0):
        m = _model()
        tr = FusedTrainer(m, lr=1e-4, max_grad_norm=clip)
        n = sum(p.numel() for p in m.parameters())
        tr.m, tr.v, tr.step_count = torch.zeros(n), torch.ones(n), 2
        sds.append(tr.state_dict())
        assert tr.last_grad_norm is None
    a, b = sds
    assert set(a) == set(b) == {"state", "param_groups"}
    assert set(a["state"]) == set(b["state"]) and all(set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} for i in a["state"])
    assert len(b["param_groups"]) == 1 and set(a["param_groups"][0]) == set(b["param_groups"][0])
    ref = torch.optim.Adam(_model().parameters()).state_dict()["param_groups"][0]
    assert set(b["param_groups"][0]) <= set(ref) and "max_grad_norm" not in b["param_groups"][0]
    fa, fb = FlatAdam(_model()).state_dict(), FlatAdam(_model(), max_grad_norm=3.0).state_dict()
    assert set(fa["param_groups"][0]) == set(fb["param_groups"][0]) and "max_grad_norm" not in fb["param_groups"][0]
    # ... and a checkpoint made with clipping on loads into a trainer without it
    FusedTrainer(_model()).load_state_dict(b)
