"""What the loss options cost in the fused step: FusedTrainer.step on the paper-size bench chunk, in ONE process, the variants interleaved block by block:

    fused          the step as it is (cross entropy inside the post-net tile, the post-net's backward in the same launch)
    ce_separate    the same step under QPN_CE_SEPARATE=1 -- the route an armed step takes (the forward writes the logits, k_ce_hard<0, false> behind it, the backward computes the
                   post-net itself): what leaving the fused tile costs, without any option
    weights        step(sample_weights=w), w uniform in [0, 2): k_ce_hard<NV, true> in the plain kernel's place
    weights_half   the same with half the rows at weight 0 (alternating blocks of 64 rows: whole workgroups skip their logits)
    smoothing      FusedTrainer(label_smoothing=0.1): k_ce_hard<NV, true> with its extra wave sum
    norm_weights   FusedTrainer(loss_norm="weights").step(sample_weights=w): k_weight_mass in front of k_ce_hard<NV, true>
    weights_distill  distill= with precomputed teacher logits plus sample_weights: k_ce_soft<NV, true> in k_ce_soft<NV, false>'s place

`fused` and `ce_separate` have a model of their own (the launch-plan knobs are read when a model's training state is created); the armed variants are trainers of their
own on ONE more model, all from the same weights, stepping through the same chunks.  Three training states, not seven: every training state owns a side stream for the
weight-gradient kernels, and with more of them than the process has hardware queues (4 by default) one variant's side stream shares a queue with its main stream and loses
the overlap -- measured with a model per variant, that one variant, whichever came sixth, ran at 0.82 of the fused step with a kernel trace showing its weight-gradient
kernels in front of the stack backward, not beside it.  Prints steps/s (median of the timed blocks), the spread of each variant's blocks and the ratios to `fused` and to `ce_separate`.

    python tools/loss_opts_rate.py [--rounds 6]

Warm-up as in bench.py: every trainer is stepped until the device has been busy for 40 ms, then a block of each variant is run untimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK = 300                                     # steps per timed block (~0.25 s)
ALPHA, TEMP, EPS = 0.5, 2.0, 0.1
NAMES = ["fused", "ce_separate", "weights", "weights_half", "smoothing", "norm_weights", "weights_distill"]


def setup(dev):
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FusedTrainer
    cfg = PAPER

    def model(seed):
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, synth.make_weights(cfg, seed)).items()})
        return m.to(dev)
    nchunks = 4
    host = [synth.train_inputs(cfg, 20000, 5000 + 17 * i, 30000, f0_lo=45.0, f0_hi=300.0, pin_f0_floor=True) for i in range(nchunks)]
    batches = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in hb] for hb in host]
    maxds = [int(np.ceil(hb[3]).max()) for hb in host]
    teacher = model(29).eval()
    with torch.no_grad():                        # the precomputed logits: the teacher's own, one tensor per chunk
        tls = [teacher(b[0], b[1], b[3], hb[4]).clone().contiguous() for b, hb in zip(batches, host)]
    gen = torch.Generator().manual_seed(3)
    ws, halves = [], []
    for hb in host:
        B, BL = hb[0].shape[0], int(hb[4][0])
        w = torch.rand((B, BL), generator=gen) * 2.0
        half = w.clone()
        half[:, (torch.arange(BL) // 64) % 2 == 1] = 0.0
        ws.append(w.to(dev)); halves.append(half.to(dev))
    kwargs = {"fused": {}, "ce_separate": {}, "weights": {}, "weights_half": {}, "smoothing": {"label_smoothing": EPS}, "norm_weights": {"loss_norm": "weights"},
              "weights_distill": {"distill": {"alpha": ALPHA, "temperature": TEMP}}}
    armed = model(13).train()
    trainers = {name: FusedTrainer(armed if name not in ("fused", "ce_separate") else model(13).train(), lr=1e-4, **kwargs[name]) for name in NAMES}

    def step(name, i):
        k = i % nchunks
        x, h, t, d, b = batches[k]
        kw = {}
        if name in ("weights", "norm_weights", "weights_distill"):
            kw["sample_weights"] = ws[k]
        elif name == "weights_half":
            kw["sample_weights"] = halves[k]
        if name == "weights_distill":
            kw["teacher_logits"] = tls[k]
        return trainers[name].step(x, h, t, d, host[k][4], want_loss=False, maxd=maxds[k], **kw)
    # the first step of a trainer creates its model's training state, which reads the environment once
    for name in NAMES:
        if name == "ce_separate":
            os.environ["QPN_CE_SEPARATE"] = "1"
        try:
            step(name, 0)
        finally:
            os.environ.pop("QPN_CE_SEPARATE", None)
    torch.cuda.synchronize()
    return trainers, step


def measure(rounds, dev):
    import torch
    trainers, step = setup(dev)
    for name in NAMES:
        t0, n = time.perf_counter(), 1
        while (time.perf_counter() - t0) * 1e3 < 40.0:
            step(name, n); n += 1
        torch.cuda.synchronize()
    rates = {name: [] for name in NAMES}
    for r in range(rounds + 1):                    # (round 0: every variant untimed)
        order = NAMES if r % 2 else NAMES[::-1]
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(BLOCK):
                step(name, i)
            torch.cuda.synchronize()
            if r:
                rates[name].append(BLOCK / (time.perf_counter() - t0))
    for name in NAMES:
        trainers[name].check_status()
    med = {name: float(np.median(v)) for name, v in rates.items()}
    return {"geometry": "paper", "chunk": "B=1, batch_length 20000", "block_steps": BLOCK, "rounds": rounds, "alpha": ALPHA, "temperature": TEMP, "label_smoothing": EPS,
            "steps_per_s": med, "over_fused": {name: med[name] / med["fused"] for name in NAMES},
            "over_ce_separate": {name: med[name] / med["ce_separate"] for name in NAMES},
            "spread_pct": {name: 100.0 * (max(v) - min(v)) / med[name] for name, v in rates.items()}, "all": rates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loss_opts_rate.py needs an AMD GPU: there is nothing to time without one")
    res = measure(args.rounds, torch.device("cuda", 0))
    print("# FusedTrainer.step, paper-size geometry, %s, %d rounds of %d-step blocks interleaved in one process, %s"
          % (res["chunk"], res["rounds"], res["block_steps"], torch.cuda.get_device_name(0)))
    print("# label_smoothing = %g; distillation alpha = %g, T = %g; steps/s = median of the timed blocks, spread = (max - min) / median of a variant's own blocks" % (EPS, ALPHA, TEMP))
    for name in NAMES:
        print("%-16s %9.1f steps/s   %.3f x fused   %.3f x ce_separate   spread %.1f %%"
              % (name, res["steps_per_s"][name], res["over_fused"][name], res["over_ce_separate"][name], res["spread_pct"][name]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
