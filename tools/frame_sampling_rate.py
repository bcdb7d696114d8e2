"""What a draw track (qpn_decode_frame_sampling; draw_track=) costs per generated sample, on one GPU:
    python tools/frame_sampling_rate.py [--repeats 5] [--frames 200] [--no-track] [--out profiles/frame_sampling.txt]
    python tools/frame_sampling_rate.py --one-call default|track      (one short B = 20 call and its plan: the program of a rocprofv3 --kernel-trace --stats run)

Paper-size model, mode="sampling", B = 20 (one utterance per five-role group) and B = 96 (two per group on 48 resident groups).  The calls ALTERNATE inside one process (call 1 of
each, then call 2 of each, ...) so that clock and temperature drift hits them alike:
  (a) the default call;
  (b) a uniform call with temperature 0.7, top_k 64, top_p 0.9;
  (c) the per-row call with those same values in every row: the natural baseline of a track, the same draw with key and values from a record;
  (d) the track that holds those values in every frame of every row (Law C: the samples of (c));
  (e) a track that alternates every 25 frames between (b)'s values and the neutral ones, rows shifted against each other: what run_decode's voiced / unvoiced flags make.
Per call: microseconds per sample step (device time of the call's launches, qpn_last_decode_kernel_ms, over the longest row's samples), min / median / max over the
repeats; (d) and (e) against (c) of the same run; and the spread of the repeated calls, which is what a difference has to exceed to mean anything.
--no-track times (a), (b), (c) alone: the same inputs on a tree without tracks (this file copied into a checkout of the parent commit)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNIFORM = dict(temperature=0.7, top_k=64, top_p=0.9)


def mmm(v):
    v = sorted(v)
    return "min %8.4f  median %8.4f  max %8.4f" % (v[0], float(np.median(v)), v[-1])


def model_and_batch(B, frames, dev):
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER
    from qpnet_amd.qpnet import QPNet
    cfg = PAPER
    flat = synth.make_weights(cfg, 13)
    m = QPNet(**cfg.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
    m = m.to(dev).eval()
    m.sampling_seed = 1234
    bx, bh, bd, ns = synth.decode_batch(cfg, [(100 + b, frames, 1.0) for b in range(B)])
    return m, torch.from_numpy(bx).to(dev), torch.from_numpy(bh).to(dev), bd, ns


def tracks(B, F):
    const = dict(temperature=np.full((B, F), 0.7, np.float32), top_k=np.full((B, F), 64, np.int32), top_p=np.full((B, F), 0.9, np.float32))
    on = ((np.arange(F)[None, :] + 7 * np.arange(B)[:, None]) // 25) % 2 == 0
    alt = dict(temperature=np.where(on, 0.7, 1.0).astype(np.float32), top_k=np.where(on, 64, 0).astype(np.int32), top_p=np.where(on, 0.9, 1.0).astype(np.float32))
    return const, alt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-track", dest="no_track", action="store_true")
    ap.add_argument("--one-call", dest="one_call", choices=["default", "track"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_sampling.txt"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    if args.one_call:
        m, xb, hb, bd, ns = model_and_batch(20, 20, dev)
        kw = dict(draw_track=tracks(20, hb.shape[2])[1]) if args.one_call == "track" else {}
        m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", **kw)
        print("one %s call, B = 20 x %d samples; plan: %s" % (args.one_call, ns[0], m.last_decode_plan))
        return 0
    lines = ["# draw track, us per sample step (device time of the launches / samples of the longest row): %s, paper-size model, mode=sampling, %d alternating calls each%s"
             % (torch.cuda.get_device_name(0), args.repeats, " (--no-track)" if args.no_track else "")]
    for B in (20, 96):
        m, xb, hb, bd, ns = model_and_batch(B, args.frames, dev)
        const, alt = tracks(B, hb.shape[2])
        calls = [("(a) default draw", {}), ("(b) uniform T 0.7, top_k 64, top_p 0.9", UNIFORM),
                 ("(c) per row: (b)'s values in every row", dict(temperature=[0.7] * B, top_k=[64] * B, top_p=[0.9] * B))]
        if not args.no_track:
            calls += [("(d) track: (b)'s values in every frame", dict(draw_track=const)), ("(e) track: (b)'s values / neutral, 25 frames each", dict(draw_track=alt))]
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
        lines.append("== B = %d, %d samples per row; plan: %s" % (B, ns[0], plans[calls[0][0]]))
        assert len(set(plans.values())) == 1, plans
        for label, _ in calls[:3]:
            v = us[label]
            lines.append("   spread (max - min) of the %s calls: %.4f us = %.2f %% of their median" % (label[:3], max(v) - min(v), 100 * (max(v) - min(v)) / med[label]))
        c_label = calls[2][0]
        for label, _ in calls:
            tail = "" if label in [c[0] for c in calls[:3]] else "   vs (c): %+.4f us (%+.2f %%)" % (med[label] - med[c_label], 100 * (med[label] - med[c_label]) / med[c_label])
            lines.append("   %-50s us/step: %s%s" % (label, mmm(us[label]), tail))
        del m
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
