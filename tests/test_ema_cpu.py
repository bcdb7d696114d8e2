"""CPU: the averaged-weights (EMA) option of the fused optimiser step -- what can be held without a GPU: the argument checks of qpn_adam_step_avg /
qpn_train_step_avg come back BEFORE the device check (a geometry-only handle), the checkpoint format (loaders.save_checkpoint / save_final /
load_checkpoint with a trainer that keeps an average), and the command-line flags."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

from qpnet_amd import _lib, loaders, runners, synth
from qpnet_amd.config import TINY
from qpnet_amd.qpnet import QPNet
from qpnet_amd.train import FlatAdam, FusedTrainer

EINVAL, ENODEV = -1, -2
# (d_ema given, ema_decay, what the message must name)
BAD = [(True, 0.0, b"ema_decay"), (True, 1.0, b"ema_decay"), (True, -0.1, b"ema_decay"), (True, float("nan"), b"ema_decay"), (False, 0.9, b"d_ema")]


@pytest.fixture()
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0      # geometry-only without a GPU
    yield L, hp
    L.qpn_destroy(hp)


def _adam_avg(L, hp, a, ema, decay):
    return L.qpn_adam_step_avg(hp, a, a, a, a, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0.0, ema, decay, None)


def _step_avg(L, hp, a, ema, decay):
    loss, valid = C.c_double(0.0), C.c_int(0)
    return L.qpn_train_step_avg(hp, a, 1, 10, 1, 10, 5, 1, a, a, a, a, 10, a, a, a, a, a, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                0, C.byref(loss), C.byref(valid), 0.0, None, ema, decay, None)


@pytest.mark.parametrize("call", [_adam_avg, _step_avg])
def test_ema_argument_errors_come_before_the_device_check(call, handle):
    """decay 0 with a buffer, 1.0, -0.1, NaN, and a decay without a buffer: QPN_EINVAL naming the argument -- on any machine, because the check precedes
    everything about the device or the handle's state.  Without a GPU a VALID pair then gets as far as the device check (QPN_ENODEV): the order is observable."""
    L, hp = handle
    buf = (C.c_float * 16)(*([0.25] * 16))
    a = C.addressof(buf)
    for given, decay, word in BAD:
        assert call(L, hp, a, a if given else None, decay) == EINVAL, (given, decay)
        assert word in L.qpn_last_error(), (given, decay, L.qpn_last_error())
    assert list(buf) == [0.25] * 16
    if not torch.cuda.is_available():
        for ema, decay in ((a, 0.9), (None, 0.0)):
            assert call(L, hp, a, ema, decay) == ENODEV
            assert b"no CPU fallback" in L.qpn_last_error()


def _model(seed=3):
    m = QPNet(**TINY.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(TINY, synth.make_weights(TINY, seed)).items()})
    return m


def _adam_state(model):
    """a torch.optim.Adam state_dict after one step on made-up gradients (what a resumed trainer holds)"""
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g) * 1e-3
    opt.step()
    for p in model.parameters():
        p.grad = None
    return opt.state_dict()


def _an_average(model, seed=9):
    g = torch.Generator().manual_seed(seed)
    return {k: v.detach() + 0.01 * torch.randn(v.shape, generator=g) for k, v in model.state_dict().items()}


def _same_tree(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys())
        for k in a:
            _same_tree(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b)
        for x, y in zip(a, b):
            _same_tree(x, y)
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    else:
        assert a == b


@pytest.mark.parametrize("make", [lambda m, **kw: FusedTrainer(m, **kw), lambda m, **kw: FlatAdam(m, lr=1e-4, **kw)])
def test_checkpoint_round_trip_on_a_cpu_model(make, tmp_path):
    """save -> load -> ema_state_dict() returns the average that went in, keys, shapes and order the model's; "model" / "optimizer" / "iterations" are what a file
    written without the average holds (the parent's save_checkpoint: exactly those three keys); the final file likewise."""
    model = _model()
    tr = make(model, ema_decay=0.999)
    tr.load_state_dict(_adam_state(model))
    avg = _an_average(model)
    tr.load_ema(avg)
    assert tr.ema.dtype == torch.float32 and tr.ema.numel() == TINY.n_params and tr.ema.device.type == "cpu"
    path = loaders.save_checkpoint(str(tmp_path / "a"), model, tr, 7)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["model", "optimizer", "iterations", "ema", "ema_decay"] and ck["ema_decay"] == 0.999
    torch.save({"model": model.state_dict(), "optimizer": tr.state_dict(), "iterations": 7}, str(tmp_path / "parent.pkl"))      # the parent's three entries
    parent = torch.load(str(tmp_path / "parent.pkl"), map_location="cpu", weights_only=False)
    _same_tree({k: ck[k] for k in parent}, parent)
    assert list(ck["ema"].keys()) == list(ck["model"].keys())
    for k in ck["model"]:
        assert ck["ema"][k].shape == ck["model"][k].shape and torch.equal(ck["ema"][k], avg[k])
    # resume into fresh objects
    m2 = _model(4)
    tr2 = make(m2, ema_decay=0.999)
    assert loaders.load_checkpoint(path, m2, tr2) == 7
    _same_tree(dict(m2.state_dict()), dict(model.state_dict()))
    _same_tree(dict(tr2.ema_state_dict()), dict(avg))
    _same_tree(tr2.state_dict()["state"], tr.state_dict()["state"])
    # use_ema: the model receives the average, not the live weights
    m3 = _model(5)
    loaders.load_checkpoint(path, m3, None, use_ema=True)
    _same_tree(dict(m3.state_dict()), dict(avg))
    assert not torch.equal(m3.state_dict()["conv_post_2.weight"], model.state_dict()["conv_post_2.weight"])
    # the final file
    fin = torch.load(loaders.save_final(str(tmp_path / "a"), model, tr), map_location="cpu", weights_only=False)
    assert list(fin.keys()) == ["model", "ema", "ema_decay"]
    _same_tree(dict(fin["model"]), dict(model.state_dict()))
    _same_tree(dict(fin["ema"]), dict(avg))


def test_files_without_averaging_hold_exactly_the_old_keys(tmp_path):
    model = _model()
    tr = FusedTrainer(model)
    assert tr.ema_state_dict() == {} and FlatAdam(model).ema_state_dict() == {}
    ck = torch.load(loaders.save_checkpoint(str(tmp_path), model, tr, 3), map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["model", "optimizer", "iterations"]
    assert list(torch.load(loaders.save_final(str(tmp_path), model, tr), map_location="cpu", weights_only=False).keys()) == ["model"]
    assert list(torch.load(loaders.save_final(str(tmp_path), model), map_location="cpu", weights_only=False).keys()) == ["model"]
    ck = torch.load(loaders.save_checkpoint(str(tmp_path), model, None, 4), map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["model", "optimizer", "iterations"] and ck["optimizer"] is None


def test_use_ema_on_a_file_without_the_average_raises(tmp_path):
    model = _model()
    path = loaders.save_checkpoint(str(tmp_path), model, FusedTrainer(model), 3)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(KeyError, match="no averaged weights"):
        loaders.load_checkpoint(path, _model(4), None, use_ema=True)
    with pytest.raises(KeyError, match="no averaged weights"):
        loaders.load_checkpoint(loaders.save_final(str(tmp_path), model), _model(4), None, use_ema=True)
    _same_tree(dict(model.state_dict()), before)


def test_resume_without_the_average_seeds_it_from_the_loaded_weights(tmp_path, caplog):
    """a trainer with averaging on, resumed from a file that holds none: a warning, and the average is the loaded weights (the seed the first step would take)."""
    model = _model()
    path = loaders.save_checkpoint(str(tmp_path), model, FusedTrainer(model), 3)
    m2 = _model(4)
    tr = FusedTrainer(m2, ema_decay=0.9)
    tr.load_ema(_an_average(m2))                     # (something else, so that the re-seed shows)
    with caplog.at_level(logging.WARNING):
        assert loaders.load_checkpoint(path, m2, tr) == 3
    assert any("no averaged weights" in r.getMessage() for r in caplog.records)
    assert tr.ema is None                            # seeded at the next step ...
    _same_tree(dict(tr.ema_state_dict()), dict(model.state_dict()))      # ... and until then it reads as the weights


def test_load_ema_checks_keys_and_shapes_and_needs_averaging_on():
    model = _model()
    tr = FusedTrainer(model, ema_decay=0.5)
    avg = _an_average(model)
    bad = dict(avg); bad.pop("conv_post_2.bias")
    with pytest.raises(ValueError, match="keys"):
        tr.load_ema(bad)
    bad = dict(avg); bad["conv_post_2.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match="conv_post_2.bias"):
        tr.load_ema(bad)
    with pytest.raises(RuntimeError, match="ema_decay is off"):
        FusedTrainer(model).load_ema(avg)
    with pytest.raises(RuntimeError, match="ema_decay is off"):
        FlatAdam(model).load_ema(avg)


def test_flags_parse():
    train = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e", "--config", "c"]
    assert runners._train_args(False).parse_args(train).ema_decay == 0.0
    assert runners._train_args(False).parse_args(train + ["--ema_decay", "0.9999"]).ema_decay == 0.9999
    assert runners._train_args(True).parse_args(train + ["--pretrain", "p", "--ema_decay", "0.5"]).ema_decay == 0.5
    val = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--resultdir", "r", "--config", "c", "--checkpoint", "k"]
    assert runners._validate_args().parse_args(val).ema is False and runners._validate_args().parse_args(val + ["--ema"]).ema is True
    dec = ["--feats", "f", "--stats", "s", "--config", "c", "--outdir", "o", "--checkpoint", "k"]
    assert runners._decode_args().parse_args(dec).ema is False and runners._decode_args().parse_args(dec + ["--ema"]).ema is True


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan"), float("inf"), 1.0 - 1e-12])
def test_constructors_refuse_a_decay_outside_the_open_interval(bad):
    """(1 - 1e-12 is 1.0f as the fp32 number the kernel is given: refused here, not by the C call of the first step)"""
    model = _model()
    with pytest.raises(ValueError, match="ema_decay"):
        FusedTrainer(model, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdam(model, ema_decay=bad)


def test_constructors_take_none_and_zero_as_off():
    model = _model()
    for off in (None, 0, 0.0):
        assert FusedTrainer(model, ema_decay=off).ema_decay == 0.0 and FlatAdam(model, ema_decay=off).ema_decay == 0.0
    tr = FusedTrainer(model, ema_decay=0.9)
    assert tr.ema_decay == 0.9 and tr.ema is None
    with pytest.raises(RuntimeError, match="ema_decay is off"):
        FusedTrainer(model).forward_loss(torch.zeros(1, 4, dtype=torch.long), None, None, None, [1], weights="ema")
