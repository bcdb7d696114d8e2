"""What the soft-target loss costs in the fused step: FusedTrainer.step on the paper-size bench chunk, in ONE process, the variants interleaved block by block:

    fused        the step as it is (cross entropy inside the post-net tile, the post-net's backward in the same launch)
    ce_separate  the same step under QPN_CE_SEPARATE=1 -- the route an armed step takes (the forward writes the logits, k_ce_hard<0, false> behind it, the backward computes the
                 post-net itself): what leaving the fused tile costs, without the soft-target term
    armed        FusedTrainer(distill={"alpha", "temperature"}).step(teacher_logits=...) with precomputed teacher logits: k_ce_soft in the plain kernel's place
    teacher      (--teacher, default on) FusedTrainer(distill={"teacher": a second paper-size model, ...}): the armed step plus the teacher's forward

Each variant has a trainer and a model of its own (the launch-plan knobs are read when a model's training state is created), all from the same weights, stepping
through the same chunks.  Prints steps/s (median of the timed blocks), the spread of each variant's blocks and the ratios to `fused`.

    python tools/distill_rate.py [--rounds 6] [--no-teacher]

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
ALPHA, TEMP = 0.5, 2.0


def setup(dev, with_teacher):
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
    names = ["fused", "ce_separate", "armed"] + (["teacher"] if with_teacher else [])
    trainers = {}
    for name in names:
        m = model(13).train()
        dd = None if name in ("fused", "ce_separate") else ({"alpha": ALPHA, "temperature": TEMP} if name == "armed" else {"teacher": teacher, "alpha": ALPHA, "temperature": TEMP})
        trainers[name] = FusedTrainer(m, lr=1e-4, distill=dd)

    def step(name, i):
        x, h, t, d, b = batches[i % nchunks]
        kw = {"teacher_logits": tls[i % nchunks]} if name == "armed" else {}
        return trainers[name].step(x, h, t, d, host[i % nchunks][4], want_loss=False, maxd=maxds[i % nchunks], **kw)
    # the first step of a trainer creates its model's training state, which reads the environment once
    for name in names:
        if name == "ce_separate":
            os.environ["QPN_CE_SEPARATE"] = "1"
        try:
            step(name, 0)
        finally:
            os.environ.pop("QPN_CE_SEPARATE", None)
    torch.cuda.synchronize()
    return names, trainers, step


def measure(rounds, dev, with_teacher):
    import torch
    names, trainers, step = setup(dev, with_teacher)
    for name in names:
        t0, n = time.perf_counter(), 1
        while (time.perf_counter() - t0) * 1e3 < 40.0:
            step(name, n); n += 1
        torch.cuda.synchronize()
    rates = {name: [] for name in names}
    for r in range(rounds + 1):                    # (round 0: every variant untimed)
        order = names if r % 2 else names[::-1]
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(BLOCK):
                step(name, i)
            torch.cuda.synchronize()
            if r:
                rates[name].append(BLOCK / (time.perf_counter() - t0))
    for name in names:
        trainers[name].check_status()
    med = {name: float(np.median(v)) for name, v in rates.items()}
    return {"geometry": "paper", "chunk": "B=1, batch_length 20000", "block_steps": BLOCK, "rounds": rounds, "alpha": ALPHA, "temperature": TEMP,
            "steps_per_s": med, "over_fused": {name: med[name] / med["fused"] for name in names},
            "spread_pct": {name: 100.0 * (max(v) - min(v)) / med[name] for name, v in rates.items()}, "all": rates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--no-teacher", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("distill_rate.py needs an AMD GPU: there is nothing to time without one")
    res = measure(args.rounds, torch.device("cuda", 0), not args.no_teacher)
    print("# FusedTrainer.step, paper-size geometry, %s, %d rounds of %d-step blocks interleaved in one process, %s"
          % (res["chunk"], res["rounds"], res["block_steps"], torch.cuda.get_device_name(0)))
    print("# alpha = %g, T = %g; steps/s = median of the timed blocks, spread = (max - min) / median of a variant's own blocks" % (ALPHA, TEMP))
    for name in res["steps_per_s"]:
        print("%-12s %9.1f steps/s   %.3f x fused   spread %.1f %%" % (name, res["steps_per_s"][name], res["over_fused"][name], res["spread_pct"][name]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
