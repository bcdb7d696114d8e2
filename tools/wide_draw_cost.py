"""What the wide draw (sampling at n_quantize > 256, sample_wave_wide of decode_dev.h) costs per generated sample, on one GPU:
    python tools/wide_draw_cost.py [--repeats 5] [--out profiles/wide_draw_cost.txt]

TINY's layers at (n_resch, n_skipch, n_quantize) = (64, 64, 512) and (64, 64, 1024) on the one-CU kernel, and (512, 256, 512) on the batched cooperative
kernel ((512, 64, 512), which the per-utterance cooperative kernel takes, is timed too).  Per geometry: greedy decode, the default draw, and the draw with
temperature 0.7, top_k 40, top_p 0.9 ALTERNATE inside one process (call 1 of each, then call 2 of each, ...) so that clock and temperature drift hits
them alike.  Per setting: microseconds per sample step (device time of the call's launches, qpn_last_decode_kernel_ms, over the longest row's samples),
min / median / max over the repeats, and the difference of the medians to greedy decode.  There is nothing to compare the figures with (the parent
refuses these calls): they are written down, no threshold applies.  The sibling of tools/sampling_controls_cost.py."""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("greedy", dict(mode="argmax")), ("default draw", dict(mode="sampling")),
            ("temperature 0.7, top_k 40, top_p 0.9", dict(mode="sampling", temperature=0.7, top_k=40, top_p=0.9))]
GEOMETRIES = [((64, 64, 512), 4, 5), ((64, 64, 1024), 4, 5), ((512, 64, 512), 3, 3), ((512, 256, 512), 3, 3)]      # (C, S, Q), batch rows, feature frames per row


def mmm(v):
    v = sorted(v)
    return "min %8.4f  median %8.4f  max %8.4f" % (v[0], float(np.median(v)), v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_draw_cost.txt"))
    args = ap.parse_args()
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import TINY
    from qpnet_amd.qpnet import QPNet
    dev = torch.device("cuda:0")
    lines = ["# wide draw, us per sample step (device time of the launches / samples of the longest row): %s, %d alternating calls per setting"
             % (torch.cuda.get_device_name(0), args.repeats)]
    for (C_, S_, Q_), B, frames in GEOMETRIES:
        cfg = dataclasses.replace(TINY, n_resch=C_, n_skipch=S_, n_quantize=Q_)
        flat = synth.make_weights(cfg, 13)
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
        m = m.to(dev).eval()
        m.sampling_seed = 1234
        bx, bh, bd, ns = synth.decode_batch(cfg, [(100 + b, frames, 1.0) for b in range(B)])
        xb, hb = torch.from_numpy(bx).to(dev), torch.from_numpy(bh).to(dev)
        plans = {}

        def call(label, kw):
            outs = m.batch_fast_generate(xb, hb, list(ns), bd, **kw)
            assert sum(len(o) for o in outs) == sum(ns)
            plans[label] = m.last_decode_plan
            return m.last_decode_kernel_ms * 1e3 / max(ns)

        for label, kw in SETTINGS:          # warm-up: allocations, code objects
            call(label, kw)
        us = {label: [] for label, _ in SETTINGS}
        for _ in range(args.repeats):
            for label, kw in SETTINGS:
                us[label].append(call(label, kw))
        base = float(np.median(us["greedy"]))
        lines.append("")
        lines.append("== TINY's layers at (n_resch, n_skipch, n_quantize) = (%d, %d, %d), B = %d, %d samples per row; plan: %s" % (C_, S_, Q_, B, ns[0], plans["default draw"]))
        for label, _ in SETTINGS:
            med = float(np.median(us[label]))
            lines.append("   %-38s us/step: %s   vs greedy: %+.4f us (%+.2f %%)" % (label, mmm(us[label]), med - base, 100 * (med - base) / base))
        del m
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
