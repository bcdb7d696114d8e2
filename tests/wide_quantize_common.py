"""What the CPU and GPU tests of sampling at n_quantize > 256 share: the four width sets on TINY's layers, their weights and inputs, and the C oracle's
sampled stream of each (computed once per process)."""
import dataclasses
import functools

import numpy as np

from qpnet_amd import synth
from qpnet_amd.config import TINY

SEED = 0x1234567890ABCDEF
ROW = 1
# (n_resch, n_skipch, n_quantize): per = 5 (an odd count), 8, 16 (the cap) on the one-CU interpreter; 512 channels take several workgroups per utterance
WIDTHS = ((64, 48, 320), (64, 64, 512), (64, 64, 1024), (512, 64, 512))
IDS = ["C%d-S%d-Q%d" % w for w in WIDTHS]


def cfg_of(csq):
    return dataclasses.replace(TINY, n_resch=csq[0], n_skipch=csq[1], n_quantize=csq[2])


@functools.lru_cache(maxsize=None)
def weights(csq, seed=31):
    return synth.make_weights(cfg_of(csq), seed)


@functools.lru_cache(maxsize=None)
def oracle_stream(csq):
    """-> dict(samples (329,), logits (329, Q)): the oracle's sampling decode of row ROW under SEED"""
    from oracle import cpu_oracle
    cfg = cfg_of(csq)
    x, h, d, n = synth.decode_inputs(cfg, 3, 61, 1.0)
    assert n == 329
    r = cpu_oracle.decode(cfg, weights(csq), h, d, x, n, mode="sampling", seed=SEED, row=ROW, want_logits=True)
    return dict(samples=np.asarray(r["samples"]), logits=np.asarray(r["logits"], dtype=np.float32))
