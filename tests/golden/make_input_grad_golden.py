#!/usr/bin/env python3
"""Generate tests/golden/input_grad.npz by IMPORTING the Python reference, the way make_golden.py does: the reference's own h.grad of the mean cross entropy
(QPNet.forward is plain torch there, so h.requires_grad_() + loss.backward() is all it takes), on the CPU in float32, for two of the inputs of
tests/input_grad_common.py.  Runs only in the build container (needs /root/reference); the file holds arrays only (a few KB): inputs are regenerated from seeds.

    python tests/golden/make_input_grad_golden.py
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src/nets")

import torch  # noqa: E402
import qpnet as ref  # noqa: E402  (the reference module)

from qpnet_amd import synth  # noqa: E402
import input_grad_common as IC  # noqa: E402

torch.set_num_threads(8)


def build_ref(cfg, flat):
    m = ref.QPNet(**cfg.kwargs())
    assert list(m.state_dict().keys()) == [k for k, _ in cfg.param_layout()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
    return m.train()


if __name__ == "__main__":
    out = {}
    for cid in IC.FIXTURE_IDS:
        o = IC.input_of(cid)
        m = build_ref(o.cfg, o.flat)
        h = torch.from_numpy(np.array(o.h)).requires_grad_()
        logits = m(torch.from_numpy(np.array(o.x)), h, torch.from_numpy(np.array(o.d)), torch.from_numpy(np.array(o.b)))
        loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, o.cfg.n_quantize), torch.from_numpy(np.array(o.t[:, -o.BL:])).reshape(-1))
        loss.backward()
        out[cid + "_dh"] = h.grad.numpy().astype(np.float32)
        out[cid + "_loss"] = np.float64(loss.item())
        print(cid, "loss", loss.item(), "max|dh| %.3e" % np.abs(out[cid + "_dh"]).max(), out[cid + "_dh"].shape)
    np.savez_compressed(os.path.join(HERE, "input_grad.npz"), **out)
    print("input_grad.npz written")
