"""Inputs of the saturated-regime tests (tests/test_saturation_cpu.py, tests/test_saturation_gpu.py, tools/saturation_parity_noise.py): networks whose gates
saturate and whose softmax is peaked, the way a trained vocoder's are -- util.trained_like_weights on the geometries of tests/test_train_edges_gpu.py -- with
the numpy oracle's forward, loss and gradient computed once per input and shared, and the figures that say what regime an input is in."""
import functools

import numpy as np

from qpnet_amd.config import PAPER, TINY, QPNetConfig
import util
import test_train_edges_gpu as E

SCENARIOS = {
    "gates": dict(gate_gain=4.0),
    "forced": dict(forced=True),
    "peaked": dict(post_gain=40.0, logit_bias=True),
    "all": dict(gate_gain=4.0, forced=True, post_gain=40.0, logit_bias=True),
}
WIDE = QPNetConfig(n_quantize=256, n_resch=64, n_skipch=512, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1)   # the wide post-net tiles
COOPB = QPNetConfig(n_resch=256, n_skipch=256, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=2)     # the batched cooperative decode
CFGS = dict(E.CFGS, wide=(WIDE, 7))
TRAIN_CASES = [(c, s) for c in ("paper", "c128", "tiny") for s in SCENARIOS] + [("wide", "peaked"), ("wide", "all")]
BL = 81                   # one full 80-row post-net tile and one row; five 16-row stack tiles and one row
FLT_MIN = np.float32(1.17549435e-38)
PLANTED = ((0, (2, 3, 41, 42)), (-1, (10, 11, 50, 51)), (37, (20, 21, 60, 61)))       # class, columns of the last BL: the dominant, the runner-up, the suppressed class


@functools.lru_cache(maxsize=None)
def train_input(cfgname, scenario):
    """the two distinct rows of test_train_edges_gpu's chunk with batch_length cut to BL, under the scenario's weights; where the softmax is peaked each row's
    targets contain the dominant class, the runner-up and the suppressed class"""
    cfg, wseed = CFGS[cfgname]
    x, h, t, d, b = util.distinct_rows_batch(cfg, 500, 61, 2500, 2)
    kw = SCENARIOS[scenario]
    t = t.copy()
    if kw.get("logit_bias"):
        for q, cols in PLANTED:
            for c in cols:
                t[:, t.shape[1] - BL + c] = q % cfg.n_quantize
    flat = util.trained_like_weights(cfg, wseed, **kw)
    return E._with_oracle(cfgname, x.copy(), h.copy(), t, d.copy(), np.full_like(b, BL), cfg=cfg, flat=flat)


def gate_stats(o):
    """over every gate of the oracle's forward: sigma exactly 0, a float32 denormal, exactly 1; |tanh| exactly 1; the shares of saturated sigma (< 1e-3 or
    > 1 - 1e-3) and of |tanh| > 0.999"""
    sg = np.concatenate([lc["sg"].ravel() for c in o.caches for lc in c["layers"]])
    th = np.abs(np.concatenate([lc["th"].ravel() for c in o.caches for lc in c["layers"]]))
    assert sg.dtype == np.float32 and th.dtype == np.float32
    return dict(zero=int((sg == 0).sum()), denormal=int(((sg > 0) & (sg < FLT_MIN)).sum()), one=int((sg == 1).sum()), tanh_one=int((th == 1).sum()),
                sat_sigma=float(((sg < 1e-3) | (sg > 1 - 1e-3)).mean()), sat_tanh=float((th > 0.999).mean()))


def softmax_stats(o):
    """per row of the batch_size * BL softmax rows: the target's probability, whether the target is the largest / the second largest class"""
    lg = o.lg.reshape(-1, o.lg.shape[-1]).astype(np.float64)
    t = o.t[:, -o.BL:].reshape(-1)
    p = np.exp(lg - lg.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    order = np.argsort(-lg, axis=1, kind="stable")
    return dict(p_target=p[np.arange(t.size), t], dominant=int((order[:, 0] == t).sum()), runner_up=int((order[:, 1] == t).sum()),
                spread=float((lg.max(1) - lg.min(1)).max()), p_max=float(p.max()))


def near_kink_units(o, kink_eps=4e-6):
    return int(sum((np.abs(c[key]) < kink_eps).sum() for c in o.caches for key in ("s0", "y0")))


def f64_distance(o):
    """the float32 oracle's own distance to the same oracle in float64 on the float32 run's ReLU sides (tools/edge_parity_noise.py): logits as a fraction of
    2e-5 * max(1, max|logits|), loss of 1e-4 * max(1, |loss|), the worst gradient tensor of its bound in util.assert_grads_match_oracle, and that tensor's name"""
    from oracle import train_oracle as TO
    with TO.precision(np.float64):
        f64 = o.flat.astype(np.float64)
        lg64, c64 = TO.forward(o.cfg, f64, o.x, o.h.astype(np.float64), o.d, o.b)
        loss64, dl64 = TO.ce_loss(lg64, o.t[:, -o.BL:])
        for c, c32 in zip(c64, o.caches):
            for key in ("s0", "y0"):
                v = c[key].copy()
                flip = (v > 0) != (c32[key] > 0)
                v[flip] = np.where(c32[key][flip] > 0, 1e-300, -1e-300)
                c[key] = v
        g64 = TO.backward(o.cfg, f64, c64, dl64)
    offs, _ = o.cfg.param_offsets()
    scale = np.abs(g64).max()
    frac, name = max((np.abs(o.og[a:a + int(np.prod(s))] - g64[a:a + int(np.prod(s))]).max() / (2e-5 * scale + 1e-4 * np.abs(g64[a:a + int(np.prod(s))]).max()), k)
                     for k, (a, s) in offs.items())
    e_lg = float(np.abs(o.lg - lg64).max()) / (2e-5 * max(1.0, float(np.abs(lg64).max())))
    return dict(logits=e_lg, loss=abs(o.loss - loss64) / (1e-4 * max(1.0, abs(loss64))), grad=float(frac), tensor=name, lg64=lg64, finite=bool(np.isfinite(g64).all()))


# ---------------------------------------------------------------- decode
DECODE_CFGS = {"paper": PAPER, "c128": E.C128, "coopb": COOPB}
DECODE_UTTS = [(61, 4, 1.0), (62, 3, 0.5)]           # two ragged rows: 439 and 329 samples
DECODE_WSEED = 29


@functools.lru_cache(maxsize=None)
def decode_weights(cfgname, kind):
    """"clamped": a logit spread beyond the exp-argument clamp of the streaming spec at every step; "stochastic": a softmax peaked enough for an exactly-zero tail
    and flat enough that the draw is not the argmax.  No logit bias: it makes the stream a constant."""
    cfg = DECODE_CFGS[cfgname] if cfgname in DECODE_CFGS else CFGS[cfgname][0]
    post = 100.0 if kind == "clamped" else (16.0 if cfg is TINY else 8.0)
    flat = util.trained_like_weights(cfg, DECODE_WSEED, gate_gain=4.0, forced=True, post_gain=post)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def decode_reference(cfgname, kind, mode, f32_factors, seed=5):
    """the C oracle's streams of the ragged batch (completion order), computed once and shared"""
    from oracle import cpu_oracle
    cfg = DECODE_CFGS[cfgname]
    bx, bh, bd, ns = util.decode_batch(cfg, DECODE_UTTS)
    outs = cpu_oracle.batch_fast_generate(cfg, decode_weights(cfgname, kind), bx, bh, list(ns), bd.astype(np.float32) if f32_factors else bd, mode=mode, seed=seed)
    for a in outs:
        a.setflags(write=False)
    return tuple(outs)
