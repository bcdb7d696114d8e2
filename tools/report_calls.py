"""The host side of the one-call training step, call for call and as a rate: FusedTrainer.step on the repository-default geometry (the bench chunk).

    python tools/report_calls.py                      # one-call step rate in lagged mode: JSON, steps/s of each timed block and their median
    python tools/report_calls.py --trace [--out DIR]  # runs itself under `rocprofv3 --hip-trace` (a fresh child process, the HIP API trace alone) and writes
                                                      # DIR/report_calls.txt: the ordered HIP runtime calls of 20 steps in each of loss modes 0, 1 and 2,
                                                      # once plain and once with clipping and accum_steps=2

QPN_LIB=<path> selects the library, so two builds can be compared: the --trace files of two builds that make the same calls are the same bytes.  The file
holds every distinct call name once and, per segment, the sequence of calls as indices into that table (launches, async copies, event records, synchronisations
and waits, memsets, attribute calls -- everything the process's main thread asked of the runtime but device guards, error polls and the compiler's registration
calls; torch's own calls between the steps are included, they are the same on both sides).
The child marks a segment's start with three hipDeviceSynchronize calls in a row."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENTS = [(mode, variant) for variant in ("plain", "clip_accum2") for mode in (False, "lagged", True)]
STEPS, BLOCK, MAX_NORM = 20, 12, 0.05
NOISE = ("hipGetDevice", "hipSetDevice", "hipGetLastError", "hipDevicePrimaryCtxGetState", "hipGetDeviceCount")      # device guards and error polls: left out of the lists


def setup(dev, variant):
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import DEFAULT
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FusedTrainer
    cfg = DEFAULT
    m = QPNet(**cfg.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, synth.make_weights(cfg, 13)).items()})
    m = m.to(dev).train()
    kw = dict(max_grad_norm=MAX_NORM, accum_steps=2) if variant == "clip_accum2" else {}
    tr = FusedTrainer(m, lr=1e-4, **kw)
    host = [synth.train_inputs(cfg, 20000, 5000 + 17 * i, 30000, f0_lo=45.0, f0_hi=300.0, pin_f0_floor=True) for i in range(2)]
    batches = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in hb] for hb in host]
    maxds = [int(np.ceil(hb[3]).max()) for hb in host]

    def step(i, want_loss):
        x, h, t, d, b = batches[i % 2]
        return tr.step(x, h, t, d, host[i % 2][4], want_loss=want_loss, maxd=maxds[i % 2])
    return tr, step


def rate(dev, rounds):
    import torch
    tr, step = setup(dev, "plain")
    step(0, "lagged"); torch.cuda.synchronize()
    t0, n = time.perf_counter(), 1
    while (time.perf_counter() - t0) * 1e3 < 40.0:
        step(n, "lagged"); n += 1
    rates = []
    for r in range(rounds + 1):                    # (round 0 untimed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(BLOCK):
            step(i, "lagged")
        torch.cuda.synchronize()
        if r:
            rates.append(BLOCK / (time.perf_counter() - t0))
    tr.flush_loss(); tr.check_status()
    return {"tool": "report_calls", "lib": os.environ.get("QPN_LIB", "product"), "geometry": "default", "loss_mode": "lagged", "block_steps": BLOCK,
            "steps_per_s": float(np.median(rates)), "all": rates}


def traced_child(dev):
    import torch
    for mode, variant in SEGMENTS:
        tr, step = setup(dev, variant)
        for _ in range(3):
            torch.cuda.synchronize()
        for i in range(STEPS):
            step(i, mode)
        torch.cuda.synchronize()
        if mode == "lagged":
            tr.flush_loss()
        tr.check_status()


def trace(out):
    d = os.path.join(out, "report_calls_trace")
    cmd = ["rocprofv3", "--hip-trace", "--output-format", "csv", "-d", d, "-o", "calls", "--", sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    fs = glob.glob(os.path.join(d, "**", "*hip_api_trace.csv"), recursive=True)
    if not fs:
        raise RuntimeError("no hip_api_trace.csv under " + d)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda x: int(x["Start_Timestamp"]))
    marks = [x["Thread_Id"] for x in rows if x["Function"] == "hipDeviceSynchronize"]
    main = max(set(marks), key=marks.count)
    calls = [x["Function"] for x in rows if x["Thread_Id"] == main and not x["Function"].startswith("__hip") and x["Function"] not in NOISE]
    starts = [i + 3 for i in range(len(calls) - 2) if calls[i:i + 3] == ["hipDeviceSynchronize"] * 3 and (i == 0 or calls[i - 1] != "hipDeviceSynchronize")]
    if len(starts) != len(SEGMENTS):
        raise RuntimeError("%d segment marks in the trace, %d expected" % (len(starts), len(SEGMENTS)))
    names = sorted(set(calls))
    path = os.path.join(out, "report_calls.txt")
    with open(path, "w") as f:
        f.write("names " + " ".join(names) + "\n")
        for k, (mode, variant) in enumerate(SEGMENTS):
            seg = calls[starts[k]:(starts[k + 1] - 3 if k + 1 < len(starts) else len(calls))]
            # a segment runs from its mark to the next trainer's set-up; the set-up's own calls (building the next model) are part of it on both sides
            f.write("segment want_loss=%s %s calls=%d launches=%d : %s\n" % (mode, variant, len(seg), sum("Launch" in c for c in seg), " ".join(str(names.index(c)) for c in seg)))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "trace"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("report_calls.py needs an AMD GPU: there is nothing to trace or time without one")
    dev = torch.device("cuda", 0)
    if args.child:
        return traced_child(dev)
    if args.trace:
        os.makedirs(args.out, exist_ok=True)
        print(trace(args.out))
    else:
        print(json.dumps(rate(dev, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
