"""Kernel time of qpn_score_logits next to qpn_ce_loss (no dL/dlogits) on the same logits, on one GPU:
    python tools/score_rate.py [--rows 19954] [--q 256] [--launches 50] [--repeats 9] [--out profiles/score.txt]

The flagship chunk's logits: 19 954 rows x 256 classes fp32 (20.4 MB) and int64 targets.  Two settings, the two calls ALTERNATING inside one process in both:
  hot    every launch reads the same buffer: 20 MB stay in the caches between launches (what a scorer launched right behind the forward sees)
  cold   the launches rotate over enough buffers to exceed the 256 MB last-level cache several times over: every launch reads from HBM
Per setting and call: device time per launch = (event time over `launches` back-to-back launches) / launches -- the gaps between dependent launches on one
stream are in it, so it bounds the kernel time from above; min / median / max over the repeats.  GB/s = the bytes the call must move (logits + targets
read, records written for the scorer; logits + targets read for the loss) over that time.  A kernel-trace run of this tool (--launches 20 --repeats 1 under a
tracing profiler) gives the kernels' own durations; profiles/score.txt holds both.  The file records what was found: it is no pass/fail bound."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mmm(v):
    v = sorted(v)
    return "min %7.2f  median %7.2f  max %7.2f" % (v[0], float(np.median(v)), v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=19954)
    ap.add_argument("--q", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cold-mb", dest="cold_mb", type=int, default=1536, help="footprint of the rotating buffers of the cold setting")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.txt"))
    args = ap.parse_args()
    import dataclasses
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import TINY
    if not torch.cuda.is_available():
        raise SystemExit("tools/score_rate.py measures on a GPU: none here")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    rows, Q, N = args.rows, args.q, args.launches
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(dataclasses.replace(TINY, n_quantize=Q))), C.byref(hp)))      # (qpn_ce_loss takes Q from its handle)
    n_cold = max(2, -(-args.cold_mb * (1 << 20) // (rows * Q * 4)))
    g = torch.Generator(device=dev); g.manual_seed(7)
    bufs = [3.0 * torch.randn((1, rows, Q), device=dev, generator=g) for _ in range(n_cold)]
    tgt = torch.randint(0, Q, (1, rows), device=dev, generator=g)
    out = torch.empty((rows, 4), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def score(i):
        _lib.check(L.qpn_score_logits(bufs[i].data_ptr(), tgt.data_ptr(), rows, 1, rows, Q, out.data_ptr(), stream))

    def ce(i):
        _lib.check(L.qpn_ce_loss(hp, bufs[i].data_ptr(), tgt.data_ptr(), rows, 1, rows, None, None, stream))

    calls = [("qpn_score_logits", score, rows * (Q * 4 + 8 + 16)), ("qpn_ce_loss (loss only)", ce, rows * (Q * 4 + 8))]
    for _, fn, _ in calls:                      # warm-up: code objects, the handle's training state
        for i in range(n_cold):
            fn(i)
    torch.cuda.synchronize()
    # the two agree on the loss (the scorer's rows are k_ce's arithmetic)
    loss = C.c_double(0.0)
    _lib.check(L.qpn_ce_loss(hp, bufs[0].data_ptr(), tgt.data_ptr(), rows, 1, rows, None, C.byref(loss), stream))
    score(0)
    mine = float(out[:, 0].double().sum()) / rows
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {(s, name): [] for s in ("hot", "cold") for name, _, _ in calls}
    for _ in range(args.repeats):
        for setting in ("hot", "cold"):
            for name, fn, _ in calls:
                e0.record()
                for k in range(N):
                    fn(0 if setting == "hot" else k % n_cold)
                e1.record()
                e1.synchronize()
                us[(setting, name)].append(e0.elapsed_time(e1) * 1e3 / N)
    L.qpn_destroy(hp)
    lines = ["# qpn_score_logits against qpn_ce_loss without dL/dlogits: %d rows x %d classes fp32, %s" % (rows, Q, torch.cuda.get_device_name(0)),
             "# device time per launch (events around %d back-to-back launches, / %d), %d alternating repeats; cold: %d buffers of %.1f MB in rotation"
             % (N, N, args.repeats, n_cold, rows * Q * 4 / 1e6),
             "# mean nll of the scorer %.12f, loss of qpn_ce_loss %.12f (relative difference %.1e)" % (mine, loss.value, abs(mine - loss.value) / abs(loss.value))]
    for setting in ("hot", "cold"):
        lines.append("")
        lines.append("== %s" % setting)
        for name, _, nbytes in calls:
            v = us[(setting, name)]
            lines.append("   %-26s us/launch: %s   %7.1f MB moved   %7.0f GB/s at the median" % (name, mmm(v), nbytes / 1e6, nbytes / float(np.median(v)) / 1e3))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
