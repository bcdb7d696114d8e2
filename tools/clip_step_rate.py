"""What gradient-norm clipping costs in the fused step: FusedTrainer.step on the bench chunk with and without max_grad_norm, in ONE process, the two
variants interleaved block by block (the same trainer, weights and buffers: only `max_grad_norm` changes between blocks), for the paper-size geometry
(bench.py's headline workload) and the repo-default one.  Prints steps/s of both and their ratio per geometry; with --profile it then runs itself once
more under `rocprofv3 --kernel-trace --stats` (a fresh child process, clipping on) and prints the durations of k_grad_sumsq, k_adam<clip> and k_adam<no clip>.

    python tools/clip_step_rate.py [--geometry paper,default] [--rounds 5] [--profile] [--out DIR]

Warm-up as in bench.py: the trainer is stepped until the device has been busy for 40 ms, then a block of each variant is run untimed."""
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

BLOCK = {"paper": 300, "default": 12}          # steps per timed block (~0.2 s / ~0.4 s)
MAX_NORM = 0.05                                 # binds on some chunks and not on others; the cost does not depend on it


def setup(name, dev):
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER, DEFAULT
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FusedTrainer
    cfg = PAPER if name == "paper" else DEFAULT
    flat = synth.make_weights(cfg, 13)
    m = QPNet(**cfg.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
    m = m.to(dev).train()
    tr = FusedTrainer(m, lr=1e-4)
    nchunks = 4 if name == "paper" else 2
    host = [synth.train_inputs(cfg, 20000, 5000 + 17 * i, 30000, f0_lo=45.0, f0_hi=300.0, pin_f0_floor=True) for i in range(nchunks)]
    batches = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in hb] for hb in host]
    maxds = [int(np.ceil(hb[3]).max()) for hb in host]

    def step(i, clip):
        tr.max_grad_norm = MAX_NORM if clip else 0.0
        x, h, t, d, b = batches[i % nchunks]
        return tr.step(x, h, t, d, host[i % nchunks][4], want_loss=False, maxd=maxds[i % nchunks])
    return tr, step


def measure(name, rounds, dev):
    import torch
    tr, step = setup(name, dev)
    step(0, False); torch.cuda.synchronize()
    t0, n = time.perf_counter(), 1
    while (time.perf_counter() - t0) * 1e3 < 40.0:
        step(n, False); n += 1
    K = BLOCK[name]
    rates = {False: [], True: []}
    for r in range(rounds + 1):                    # (round 0: both variants untimed)
        for clip in ((False, True) if r % 2 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(K):
                step(i, clip)
            torch.cuda.synchronize()
            if r:
                rates[clip].append(K / (time.perf_counter() - t0))
    tr.check_status()
    off, on = float(np.median(rates[False])), float(np.median(rates[True]))
    return {"geometry": name, "block_steps": K, "rounds": rounds, "steps_per_s_off": off, "steps_per_s_on": on, "on_over_off": on / off,
            "off_all": rates[False], "on_all": rates[True]}


def profiled_child(name, dev):
    import torch
    tr, step = setup(name, dev)
    for i in range(30 if name == "paper" else 4):
        step(i, True)
    torch.cuda.synchronize()
    tr.check_status()


def profile(name, out):
    d = os.path.join(out, "clip_trace_" + name)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "clip", "--",
           sys.executable, os.path.abspath(__file__), "--child", name]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    fs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not fs:
        raise RuntimeError("no kernel_stats.csv under " + d)
    rows = list(csv.DictReader(open(fs[0])))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    res = {"geometry": name, "all_kernels_us_per_step": None, "kernels": {}}
    for x in rows:
        # (the Adam kernel is one template, reported as `void k_adam<CLIP, EMA, GROUPED>(...)`: its first argument tells the clipping instance from the plain one)
        for k, label in (("k_grad_sumsq", "k_grad_sumsq"), ("k_adam<true", "k_adam<clip>"), ("k_adam<false", "k_adam<no clip>")):
            if k in x["Name"].replace(" ", ""):
                res["kernels"][label] = {"calls": int(x["Calls"]), "average_us": float(x["AverageNs"]) / 1e3, "min_us": float(x["MinNs"]) / 1e3,
                                         "max_us": float(x["MaxNs"]) / 1e3, "share_of_kernel_time_pct": 100.0 * float(x["TotalDurationNs"]) / total}
    calls = res["kernels"].get("k_adam<clip>", {}).get("calls")
    if calls:
        res["all_kernels_us_per_step"] = total / calls / 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="paper,default")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clip_step_rate.py needs an AMD GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    if args.child:
        return profiled_child(args.child, dev)
    for name in args.geometry.split(","):
        print(json.dumps(measure(name, args.rounds, dev)), flush=True)
    if args.profile:
        for name in args.geometry.split(","):
            print(json.dumps(profile(name, args.out)), flush=True)


if __name__ == "__main__":
    main()
