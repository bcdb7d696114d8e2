"""What per-row sampling records (qpn_decode_row_sampling; row_seeds= and per-row controls) cost per generated sample, on one GPU:
    python tools/row_sampling_rate.py [--repeats 7] [--uniform-only] [--out profiles/row_sampling.txt]

Paper-size model at B = 20 x 600 frames and the repo-default model at B = 20 x 100 frames, mode="sampling".  Four calls ALTERNATE inside one process
(call 1 of each, then call 2 of each, ...) so that clock and temperature drift hits them alike:
  (a) the default call;
  (b) a uniform call with temperature 0.7, top_k 64, top_p 0.9;
  (c) the per-row call with those same values in every row plus row_seeds;
  (d) a per-row call whose rows cycle through the four settings of tests/test_row_sampling_gpu.py, plus row_seeds.
Per call: microseconds per sample step (device time of the call's launches, qpn_last_decode_kernel_ms, over the longest row's samples), min / median / max
over the repeats; (c) and (d) against (b) of the same run; and the spread of the repeated (a) and (b) calls, which is what a difference has to exceed to
mean anything.  --uniform-only times (a) and (b) alone: the same inputs on a tree without the records (this file copied into a checkout of the parent).

profiles/row_sampling.txt is one GPU visit: the output of this tool on this tree and, behind comment lines that say so, of --uniform-only in a checkout of
the parent commit built there, in fresh processes that alternate between the two trees (tree, parent, tree, parent)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNIFORM = dict(temperature=0.7, top_k=64, top_p=0.9)
CYCLE = [(1.0, 0, 1.0, 0.0), (0.7, 40, 1.0, 0.0), (1.0, 0, 0.9, 0.05), (0.5, 64, 0.8, 0.0)]


def mmm(v):
    v = sorted(v)
    return "min %8.4f  median %8.4f  max %8.4f" % (v[0], float(np.median(v)), v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--uniform-only", dest="uniform_only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_sampling.txt"))
    args = ap.parse_args()
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER, DEFAULT
    from qpnet_amd.qpnet import QPNet
    dev = torch.device("cuda:0")
    lines = ["# per-row sampling records, us per sample step (device time of the launches / samples of the longest row): %s, mode=sampling, %d alternating calls each%s"
             % (torch.cuda.get_device_name(0), args.repeats, " (--uniform-only)" if args.uniform_only else "")]
    for name, cfg, B, frames in (("paper-size", PAPER, 20, 600), ("repo-default", DEFAULT, 20, 100)):
        flat = synth.make_weights(cfg, 13)
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
        m = m.to(dev).eval()
        m.sampling_seed = 1234
        bx, bh, bd, ns = synth.decode_batch(cfg, [(100 + b, frames, 1.0) for b in range(B)])
        xb, hb = torch.from_numpy(bx).to(dev), torch.from_numpy(bh).to(dev)
        seeds = [(0x9E3779B97F4A7C15 * (b + 1)) % (1 << 64) for b in range(B)]
        cyc = [CYCLE[b % 4] for b in range(B)]
        calls = [("(a) default draw", {}), ("(b) uniform T 0.7, top_k 64, top_p 0.9", UNIFORM)]
        if not args.uniform_only:
            calls += [("(c) per row: (b)'s values + row_seeds", dict(temperature=[0.7] * B, top_k=[64] * B, top_p=[0.9] * B, row_seeds=seeds)),
                      ("(d) per row: four settings + row_seeds", dict(temperature=[c[0] for c in cyc], top_k=[c[1] for c in cyc], top_p=[c[2] for c in cyc],
                                                                      min_p=[c[3] for c in cyc], row_seeds=seeds))]
        plans = {}

        def call(label, kw):
            outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", **kw)
            assert sum(len(o) for o in outs) == sum(ns)
            plans[label] = m.last_decode_plan
            return m.last_decode_kernel_ms * 1e3 / max(ns)

        for label, kw in calls:          # warm-up: allocations, code objects
            call(label, kw)
        us = {label: [] for label, _ in calls}
        for _ in range(args.repeats):
            for label, kw in calls:
                us[label].append(call(label, kw))
        med = {label: float(np.median(v)) for label, v in us.items()}
        lines.append("")
        lines.append("== %s model, B = %d, %d samples per row; plan: %s" % (name, B, ns[0], plans[calls[0][0]]))
        assert len(set(plans.values())) == 1, plans
        for label, _ in calls[:2]:
            v = us[label]
            lines.append("   spread (max - min) of the %s calls: %.4f us = %.2f %% of their median" % (label[:3], max(v) - min(v), 100 * (max(v) - min(v)) / med[label]))
        b_label = calls[1][0]
        for label, _ in calls:
            tail = "" if label in (calls[0][0], b_label) else "   vs (b): %+.4f us (%+.2f %%)" % (med[label] - med[b_label], 100 * (med[label] - med[b_label]) / med[b_label])
            lines.append("   %-42s us/step: %s%s" % (label, mmm(us[label]), tail))
        del m
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
