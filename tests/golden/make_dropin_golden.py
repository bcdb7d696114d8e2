#!/usr/bin/env python3
"""Record what the reference's task scripts bind and write through `qpnet` into tests/golden/dropin.json, by IMPORTING them.

    python tests/golden/make_dropin_golden.py <reference checkout>/src

Runs only where the reference checkout exists.  The fixture is plain data -- the names qpnet_train.py / qpnet_decode.py import from
`qpnet`, the reference class's receptive fields, dilations, state-dict and parameter names with their shapes, the layout of the
checkpoint its trainer writes and the mu-law tables -- which tests/test_dropin_binding_cpu.py checks the drop-in module against."""
import json
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))

# the network qpnet_train.py builds from its argparse defaults (runQP's 'default' model)
KWARGS = dict(n_quantize=256, n_aux=39, n_resch=512, n_skipch=256, dilationF_depth=4, dilationF_repeat=3,
              dilationA_depth=4, dilationA_repeat=1, kernel_size=2, upsampling_factor=110)


def main(src):
    warnings.filterwarnings("ignore")
    for name in ("h5py", "torchvision"):                   # the scripts only import them
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    if not hasattr(tv, "transforms"):
        tv.transforms = types.ModuleType("torchvision.transforms"); sys.modules["torchvision.transforms"] = tv.transforms
    sys.path[:0] = [os.path.join(src, "utils"), os.path.join(src, "nets"), os.path.join(src, "bin")]
    import numpy as np
    import torch
    import qpnet as ref
    import qpnet_train as rt
    import qpnet_decode as rd
    # the names each script holds that are the reference module's own functions / classes
    imports = {mod.__name__: sorted(n for n, v in vars(mod).items() if vars(ref).get(n) is v and getattr(v, "__module__", None) == ref.__name__)
               for mod in (rt, rd)}
    model = ref.QPNet(**KWARGS)
    model.apply(rt.initialize)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    with tempfile.TemporaryDirectory() as td:
        rt._save_checkpoint(td, model, opt, 7)
        files = sorted(os.listdir(td))
        ck = torch.load(os.path.join(td, files[0]), map_location="cpu", weights_only=False)
    x = np.linspace(-1, 1, 101)
    out = {
        "kwargs": KWARGS,
        "imports": imports,
        "attributes": {a: int(getattr(model, a)) for a in ("receptiveCausal_field", "receptiveF_field", "receptiveA_field",
                                                            "n_quantize", "n_aux", "upsampling_factor")},
        "dilationsF": [int(v) for v in model.dilationsF], "dilationsA": [int(v) for v in model.dilationsA],
        "state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()],
        "parameters": [[k, list(p.shape)] for k, p in model.named_parameters()],
        "checkpoint": {"files": files, "keys": sorted(ck.keys()), "iterations": ck["iterations"],
                       "model_keys": list(ck["model"].keys()), "optimizer_keys": sorted(ck["optimizer"].keys()),
                       "optimizer_params": [len(g["params"]) for g in ck["optimizer"]["param_groups"]]},
        "mu_law": {"x": x.tolist(), "encoded": [int(v) for v in ref.encode_mu_law(x, 256)],
                   "decoded": [float(v) for v in ref.decode_mu_law(np.arange(256), 256)]},
    }
    with open(os.path.join(HERE, "dropin.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
