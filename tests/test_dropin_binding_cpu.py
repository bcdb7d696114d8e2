"""The reference's own task scripts bind the drop-in module.

runQP.py puts src/utils:src/nets on PYTHONPATH and the scripts do `from qpnet import ...` (qpnet_train.py:35-37, qpnet_decode.py:32-34).
With qpnet_amd/dropin in FRONT of src/nets the names they bind must be this repo's, and everything they do with them on the host --
construct from the argparse namespace, .apply(initialize), read the receptive fields, wrap in DataParallel, write and resume a checkpoint
(qpnet_train.py:400-423,463-465,338-353,481-499) -- must work on the drop-in class and match what the reference class does.
What the reference does is recorded in tests/golden/dropin.json (tests/golden/make_dropin_golden.py imports the scripts to write it).
Construction / state only: no kernel runs on the CPU, the library has no CPU path."""
import copy
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "qpnet_amd", "dropin")


@pytest.fixture
def dropin(monkeypatch):
    """`import qpnet` with the drop-in directory first on the path, as the scripts' PYTHONPATH has it"""
    monkeypatch.syspath_prepend(DROPIN)
    saved = sys.modules.pop("qpnet", None)
    try:
        yield importlib.import_module("qpnet")
    finally:
        sys.modules.pop("qpnet", None)
        if saved is not None:
            sys.modules["qpnet"] = saved


def test_reference_scripts_bind_the_dropin_module(dropin, golden_dir, tmp_path):
    import qpnet_amd.qpnet as mine
    from qpnet_amd import loaders
    g = json.load(open(os.path.join(golden_dir, "dropin.json")))
    assert dropin.__file__.startswith(DROPIN), dropin.__file__
    for script, names in g["imports"].items():
        for n in names:
            assert getattr(dropin, n) is getattr(mine, n), (script, n)
    # the network as qpnet_train.py builds it from its argparse namespace
    model = dropin.QPNet(**g["kwargs"])
    model.apply(dropin.initialize)
    model.train()
    assert float(model.upsampling.conv.weight.min()) == 1.0 and float(model.causal.conv.bias.abs().max()) == 0.0     # initialize reached the holders
    for a, v in g["attributes"].items():
        assert getattr(model, a) == v, a
    assert list(model.dilationsF) == g["dilationsF"] and list(model.dilationsA) == g["dilationsA"]
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == g["state_dict"]
    assert [[k, list(p.shape)] for k, p in model.named_parameters()] == g["parameters"]     # Adam's state is indexed in this order
    # setups for multi GPUs (qpnet_train.py:416-423), over the devices this machine has (none: a plain wrapper; DataParallel moves the module to the first)
    dp = torch.nn.DataParallel(copy.deepcopy(model), list(range(torch.cuda.device_count())))
    dp.receptiveF_field = dp.module.receptiveF_field
    dp.receptiveA_field = dp.module.receptiveA_field
    dp.receptiveCausal_field = dp.module.receptiveCausal_field
    assert (dp.receptiveCausal_field, dp.receptiveF_field, dp.receptiveA_field) == (1, 45, 15)
    # a checkpoint laid out as the reference trainer writes it, and the resume path's load in both directions
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4)
    path = loaders.save_checkpoint(str(tmp_path), model, optimizer, g["checkpoint"]["iterations"])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(os.listdir(tmp_path)) == g["checkpoint"]["files"]
    assert sorted(ck.keys()) == g["checkpoint"]["keys"] and ck["iterations"] == g["checkpoint"]["iterations"]
    assert list(ck["model"].keys()) == g["checkpoint"]["model_keys"]
    assert sorted(ck["optimizer"].keys()) == g["checkpoint"]["optimizer_keys"]
    assert [len(pg["params"]) for pg in ck["optimizer"]["param_groups"]] == g["checkpoint"]["optimizer_params"]
    # a state dict with the reference class's names and shapes loads strictly into the drop-in class, and the decode script's construction takes it
    ref_sd = {k: torch.full(s, 0.5) for k, s in g["state_dict"]}
    model.load_state_dict(ref_sd)
    m2 = dropin.QPNet(**g["kwargs"])
    m2.load_state_dict(ck["model"]); m2.eval()
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in ref_sd.items())
    optimizer.load_state_dict(ck["optimizer"])
    # mu-law round trip on the drop-in's functions against the reference's tables
    x = np.asarray(g["mu_law"]["x"])
    assert np.array_equal(dropin.encode_mu_law(x, 256), np.asarray(g["mu_law"]["encoded"]))
    assert np.array_equal(dropin.decode_mu_law(np.arange(256), 256), np.asarray(g["mu_law"]["decoded"]))
