"""What the feature gradient costs in the fused step: FusedTrainer.step on the bench chunk with and without `h_grad`, in ONE process, the two variants
interleaved block by block (the same trainer, weights and buffers: only the request changes between blocks), for the paper-size geometry (bench.py's
headline workload) and the repo-default one.  Prints steps/s of both and their ratio per geometry.

    python tools/input_grad_rate.py [--geometry paper,default] [--rounds 5] [--profile] [--parent DIR] [--out DIR]

--profile     runs itself once more under `rocprofv3 --kernel-trace --stats` (a fresh child process, every step armed) and prints the durations of the
              feature-gradient kernels (k_dh_frames / k_dh_up / k_dh_copy) next to the launches they run beside (k_aux_tail / k_up_bwd, the weight gradients).
--parent DIR  a built checkout of the parent commit: (a) the UNARMED step of this tree and of that one, timed in alternating fresh child processes of the same
              session (median and spread of each, the way profiles/step_ends_ab.txt compares two trees); (b) the kernel names and calls per step of an unarmed
              step on both trees, from a kernel trace each, and whether the two lists are identical.

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
if "--tree" in sys.argv:                            # (a child timing another checkout imports THAT tree's package)
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))
else:
    sys.path.insert(0, ROOT)

BLOCK = {"paper": 300, "default": 12}          # steps per timed block (~0.2 s / ~0.4 s)
TRACED_STEPS = {"paper": 30, "default": 4}
DH_KERNELS = ("k_dh_frames", "k_dh_up", "k_dh_copy")
BESIDE = ("k_aux_tail", "k_up_bwd", "k_wgrad", "k_gemm_tn")


def setup(name, dev, with_buffers=True):
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
    bufs = [torch.empty_like(b[1]) for b in batches] if with_buffers else None

    def step(i, armed):
        x, h, t, d, b = batches[i % nchunks]
        kw = {"h_grad": bufs[i % nchunks]} if armed else {}
        return tr.step(x, h, t, d, host[i % nchunks][4], want_loss=False, maxd=maxds[i % nchunks], **kw)
    return tr, step


def _warm(step):
    import torch
    step(0, False); torch.cuda.synchronize()
    t0, n = time.perf_counter(), 1
    while (time.perf_counter() - t0) * 1e3 < 40.0:
        step(n, False); n += 1


def measure(name, rounds, dev):
    import torch
    tr, step = setup(name, dev)
    _warm(step)
    K = BLOCK[name]
    rates = {False: [], True: []}
    for r in range(rounds + 1):                    # (round 0: both variants untimed)
        for armed in ((False, True) if r % 2 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(K):
                step(i, armed)
            torch.cuda.synchronize()
            if r:
                rates[armed].append(K / (time.perf_counter() - t0))
    tr.check_status()
    off, on = float(np.median(rates[False])), float(np.median(rates[True]))
    return {"geometry": name, "block_steps": K, "rounds": rounds, "steps_per_s_unarmed": off, "steps_per_s_armed": on, "armed_over_unarmed": on / off,
            "unarmed_all": rates[False], "armed_all": rates[True]}


def unarmed_child(name, rounds, dev):
    """steps/s of the plain step of whichever tree --tree names (no h_grad anywhere: runs on the parent commit too)"""
    import torch
    tr, step = setup(name, dev, with_buffers=False)
    _warm(step)
    K = BLOCK[name]
    rates = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            step(i, False)
        torch.cuda.synchronize()
        if r:
            rates.append(K / (time.perf_counter() - t0))
    tr.check_status()
    print(json.dumps({"steps_per_s": float(np.median(rates)), "all": rates}), flush=True)


def traced_child(name, armed, dev):
    import torch
    tr, step = setup(name, dev, with_buffers=armed)
    for i in range(TRACED_STEPS[name]):
        step(i, armed)
    torch.cuda.synchronize()
    tr.check_status()


def _trace(name, out, tag, tree, armed):
    d = os.path.join(out, "input_grad_trace_%s_%s" % (name, tag))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dh", "--",
           sys.executable, os.path.abspath(__file__), "--child", "armed" if armed else "unarmed", "--geometry", name, "--tree", tree]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    fs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not fs:
        raise RuntimeError("no kernel_stats.csv under " + d)
    return list(csv.DictReader(open(fs[0])))


def _short(kernel_name):
    return kernel_name.split("(")[0].strip()


def profile(name, out):
    rows = _trace(name, out, "armed", ROOT, True)
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    steps = TRACED_STEPS[name]
    res = {"geometry": name, "all_kernels_us_per_step": total / steps / 1e3, "kernels": {}}
    for x in rows:
        if any(k in x["Name"] for k in DH_KERNELS + BESIDE):
            res["kernels"][_short(x["Name"])] = {"calls_per_step": int(x["Calls"]) / steps, "average_us": float(x["AverageNs"]) / 1e3, "min_us": float(x["MinNs"]) / 1e3,
                                                 "max_us": float(x["MaxNs"]) / 1e3, "share_of_kernel_time_pct": 100.0 * float(x["TotalDurationNs"]) / total}
    return res


def names(name, out, parent):
    """kernel names and calls of TRACED_STEPS unarmed steps (set-up launches included: the same on both trees) on this tree and on the parent's"""
    lists = {}
    for tag, tree in (("this", ROOT), ("parent", parent)):
        lists[tag] = sorted((_short(x["Name"]), int(x["Calls"])) for x in _trace(name, out, "names_" + tag, tree, False))
    return {"geometry": name, "unarmed_steps_traced": TRACED_STEPS[name], "identical": lists["this"] == lists["parent"],
            "this_tree": ["%s x%d" % kc for kc in lists["this"]], "parent": ["%s x%d" % kc for kc in lists["parent"]]}


def ab(name, rounds, parent):
    """the unarmed step of both trees in alternating fresh processes"""
    res = {"this": [], "parent": []}
    for r in range(rounds):
        for tag in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            tree = ROOT if tag == "this" else parent
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "rate", "--geometry", name, "--rounds", "3", "--tree", tree],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError("child failed (%d): %s" % (p.returncode, (p.stdout + p.stderr)[-2000:]))
            res[tag].append(json.loads(p.stdout.strip().splitlines()[-1])["steps_per_s"])
    a, b = res["this"], res["parent"]
    return {"geometry": name, "processes_per_tree": rounds, "unarmed_steps_per_s_this_tree": a, "unarmed_steps_per_s_parent": b,
            "median_this_tree": float(np.median(a)), "median_parent": float(np.median(b)), "this_over_parent": float(np.median(a) / np.median(b)),
            "spread_this_tree": float((max(a) - min(a)) / np.median(a)), "spread_parent": float((max(b) - min(b)) / np.median(b))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="paper,default")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_rate.py needs an AMD GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    if args.child == "rate":
        return unarmed_child(args.geometry, args.rounds, dev)
    if args.child:
        return traced_child(args.geometry, args.child == "armed", dev)
    for name in args.geometry.split(","):
        print(json.dumps(measure(name, args.rounds, dev)), flush=True)
    if args.profile:
        for name in args.geometry.split(","):
            print(json.dumps(profile(name, args.out)), flush=True)
    if args.parent:
        parent = os.path.abspath(args.parent)
        for name in args.geometry.split(","):
            print(json.dumps(ab(name, args.rounds, parent)), flush=True)
        for name in args.geometry.split(","):
            print(json.dumps(names(name, args.out, parent)), flush=True)


if __name__ == "__main__":
    main()
