"""What the sampling controls (temperature, top_k, top_p, min_p) cost per generated sample, on one GPU:
    python tools/sampling_controls_cost.py [--repeats 5] [--default-only] [--out profiles/sampling_controls.txt]

Paper-size model at B = 20 x 600 frames and the repo-default model at B = 20 x 100 frames, mode="sampling".  The settings -- the default
draw, temperature 0.7, top_k 64, both, min_p 0.05, top_p 0.9, and top_p 0.9 on top of temperature 0.7 and top_k 64 -- ALTERNATE inside one
process (call 1 of each, then call 2 of each, ...) so that clock and temperature drift hits them alike.  Per setting: microseconds per sample step (device time of the call's launches, qpn_last_decode_kernel_ms,
over the longest row's samples), min / median / max over the repeats, the difference of the medians to the default draw, and the spread of
the repeated default calls, which is what a difference has to exceed to mean anything.
--default-only times the default draw alone (the same inputs on a build without the controls).

profiles/sampling_controls.txt is one GPU visit: the output of this tool on this tree; then, behind comment lines that say so, the output (less
its header line) of a copy of this tool run with --default-only in a checkout of the parent commit, built there; then the decode figures
of `python bench.py --mode decode --full` (samples/s of the timed greedy steps, and of the sampling-mode run) on both trees; then default calls
alone in fresh processes that alternate between the two trees, which shows what a process's placement on the chip is worth.
profiles/top_p_min_p.txt is another visit: this tool (--out) on the tree that added top_p and min_p and the parent's copy of it in a checkout of
the parent, built there, in fresh processes that alternate between the two trees."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("default draw", {}), ("temperature 0.7", dict(temperature=0.7)), ("top_k 64", dict(top_k=64)),
            ("temperature 0.7, top_k 64", dict(temperature=0.7, top_k=64)), ("min_p 0.05", dict(min_p=0.05)), ("top_p 0.9", dict(top_p=0.9)),
            ("temperature 0.7, top_k 64, top_p 0.9", dict(temperature=0.7, top_k=64, top_p=0.9))]


def mmm(v):
    v = sorted(v)
    return "min %8.4f  median %8.4f  max %8.4f" % (v[0], float(np.median(v)), v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--default-only", dest="default_only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_controls.txt"))
    args = ap.parse_args()
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER, DEFAULT
    from qpnet_amd.qpnet import QPNet
    dev = torch.device("cuda:0")
    settings = SETTINGS[:1] if args.default_only else SETTINGS
    lines = ["# sampling controls, us per sample step (device time of the launches / samples of the longest row): %s, mode=sampling, %d alternating calls per setting"
             % (torch.cuda.get_device_name(0), args.repeats)]
    for name, cfg, B, frames in (("paper-size", PAPER, 20, 600), ("repo-default", DEFAULT, 20, 100)):
        flat = synth.make_weights(cfg, 13)
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
        m = m.to(dev).eval()
        m.sampling_seed = 1234
        bx, bh, bd, ns = synth.decode_batch(cfg, [(100 + b, frames, 1.0) for b in range(B)])
        xb, hb = torch.from_numpy(bx).to(dev), torch.from_numpy(bh).to(dev)

        def call(kw):
            outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", **kw)
            assert sum(len(o) for o in outs) == sum(ns)
            return m.last_decode_kernel_ms * 1e3 / max(ns)

        for _, kw in settings:          # warm-up: allocations, code objects
            call(kw)
        us = {label: [] for label, _ in settings}
        for _ in range(args.repeats):
            for label, kw in settings:
                us[label].append(call(kw))
        base = float(np.median(us[settings[0][0]]))
        d = us[settings[0][0]]
        lines.append("")
        lines.append("== %s model, B = %d, %d samples per row; plan: %s" % (name, B, ns[0], m.last_decode_plan))
        lines.append("   spread (max - min) of the default calls: %.4f us = %.2f %% of their median" % (max(d) - min(d), 100 * (max(d) - min(d)) / base))
        for label, _ in settings:
            med = float(np.median(us[label]))
            lines.append("   %-36s us/step: %s   vs default: %+.4f us (%+.2f %%)" % (label, mmm(us[label]), med - base, 100 * (med - base) / base))
        del m
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
