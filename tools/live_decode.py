"""Live decode output (QPNet.generate_live) against the blocking call (batch_fast_generate), on one GPU:
    python tools/live_decode.py [--repeats 5] [--frames 200] [--unarmed-only] [--cancel] > profiles/live_decode.txt

Paper-size model at B = 1 and B = 20 and the repo-default model at B = 1, 200-frame utterances (21 999 samples each), greedy.  Per case:
  - the time from the return of the enqueue to the first piece, and the pieces per call, with a publish every 64 / 256 / 1024 samples;
  - the time of a whole call, armed (every = 64, 256, 1024; the generator drained by a consumer that only counts) against unarmed
    (batch_fast_generate).  The variants ALTERNATE inside one process -- repeat 1 of each, then repeat 2 of each, ... -- so that clock and
    temperature drift hits them alike; min / median / max over the repeats, host wall time of the call and device time of its launches.
--unarmed-only times the blocking call alone (the same inputs on a build without live output).
--cancel adds, per case and publish interval, calls that are stopped through the C ABI (qpn_decode_cancel) right after their first count has
appeared: the time from the return of qpn_decode_cancel to the first poll that reports *running == 0, the time to the return of
qpn_decode_finish, the longest row's count at the request and its final count.

profiles/live_decode.txt is TWO runs in one GPU visit: the output of this tool on this tree, then, behind a comment line that says so, the output (less its
header line) of a copy of this tool run with --unarmed-only in a checkout of the parent commit, built there: the blocking call before live output existed.
Its "decode cancel" part is two runs of the same kind: this tool with --cancel on this tree, then the parent commit's copy of the tool (all four variants, no
--cancel: the parent cannot) in a checkout of the parent commit, built there."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mmm(v):
    v = sorted(v)
    return "min %9.3f  median %9.3f  max %9.3f" % (v[0], float(np.median(v)), v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--unarmed-only", dest="unarmed_only", action="store_true")
    ap.add_argument("--cancel", action="store_true")
    args = ap.parse_args()
    import torch
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER, DEFAULT
    from qpnet_amd.qpnet import QPNet
    dev = torch.device("cuda:0")
    print("# live decode output vs the blocking call: %s, %d-frame utterances, greedy, %d alternating repeats per variant"
          % (torch.cuda.get_device_name(0), args.frames, args.repeats))
    variants = [0] if args.unarmed_only else [0, 64, 256, 1024]
    for name, cfg, B in (("paper-size", PAPER, 1), ("paper-size", PAPER, 20), ("repo-default", DEFAULT, 1)):
        flat = synth.make_weights(cfg, 13)
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
        m = m.to(dev).eval()
        bx, bh, bd, ns = synth.decode_batch(cfg, [(100 + b, args.frames, 1.0) for b in range(B)])
        xb, hb = torch.from_numpy(bx).to(dev), torch.from_numpy(bh).to(dev)

        def call(every):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if every == 0:
                outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode="argmax")
                got = sum(len(o) for o in outs)
            else:
                got = sum(len(s) for _, _, s in m.generate_live(xb, hb, list(ns), bd, mode="argmax", every=every))
            dt = time.perf_counter() - t0
            assert got == sum(ns)
            return dt * 1e3, m.last_decode_kernel_ms

        def cancelled_call(every):
            """-> ms from the return of qpn_decode_cancel to *running == 0, ms to the return of qpn_decode_finish, the longest row's count at the request, its final count"""
            import ctypes as C
            from qpnet_amd import _lib
            a = m._decode_args(xb, hb, list(ns), bd, "argmax", False)
            L, hd = a["L"], a["hd"]
            done, cancelled = (C.c_int64 * B)(), C.c_int()
            mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
            pargs = (hd, done, C.byref(mirror), C.byref(stride), C.byref(running))
            torch.cuda.synchronize()
            _lib.check(L.qpn_decode_live(hd, every))
            _lib.check(L.qpn_decode_enqueue(*a["call"]))
            while True:
                _lib.check(L.qpn_decode_poll(*pargs))
                if max(done) > 0:
                    break
            at_request = max(done)
            _lib.check(L.qpn_decode_cancel(hd))
            t0 = time.perf_counter()
            while True:                 # (no sleep between the polls: the poll is what is being timed)
                _lib.check(L.qpn_decode_poll(*pargs))
                if not running.value:
                    break
            t_run = time.perf_counter()
            _lib.check(L.qpn_decode_finish(hd, a["stream"]))
            t_fin = time.perf_counter()
            _lib.check(L.qpn_decode_final_counts(hd, done, C.byref(cancelled)))
            _lib.check(L.qpn_decode_live(hd, 0))
            assert cancelled.value == 1 and max(done) < max(ns), (cancelled.value, max(done))
            return (t_run - t0) * 1e3, (t_fin - t0) * 1e3, at_request, max(done)

        for every in variants:          # warm-up: allocations, code objects
            call(every)
        wall = {v: [] for v in variants}
        kern = {v: [] for v in variants}
        first = {v: [] for v in variants}
        pieces = {v: [] for v in variants}
        for _ in range(args.repeats):
            for every in variants:
                w, k = call(every)
                wall[every].append(w); kern[every].append(k)
                if every:
                    first[every].append(m._live_first_piece_s * 1e3); pieces[every].append(m._live_mirror_pieces)
        stops = {v: [cancelled_call(v) for _ in range(args.repeats + 1)][1:] for v in variants if v and args.cancel}      # (the first one: warm-up)
        print("\n== %s model, B = %d, %d samples per row; plan: %s" % (name, B, ns[0], m.last_decode_plan))
        base = float(np.median(wall[0]))
        print("   unarmed spread (max - min) of the call time: %.3f ms = %.2f %% of its median" % (max(wall[0]) - min(wall[0]), 100 * (max(wall[0]) - min(wall[0])) / base))
        for every in variants:
            tag = "unarmed        " if every == 0 else "armed every=%-4d" % every
            print("   %s call ms: %s   launches ms: %s" % (tag, mmm(wall[every]), mmm(kern[every])))
            if every:
                print("   %s median call time vs unarmed: %+.3f ms (%+.2f %%)   first piece after enqueue ms: %s   pieces per call: %d..%d"
                      % (" " * len(tag), float(np.median(wall[every])) - base, 100 * (float(np.median(wall[every])) - base) / base,
                         mmm(first[every]), min(pieces[every]), max(pieces[every])))
        for every, st in stops.items():
            print("   cancel every=%-4d request -> running == 0 ms: %s   request -> finish returned ms: %s   count at the request %d..%d, final count %d..%d"
                  % (every, mmm([r[0] for r in st]), mmm([r[1] for r in st]), min(r[2] for r in st), max(r[2] for r in st), min(r[3] for r in st), max(r[3] for r in st)))
        del m
    return 0


if __name__ == "__main__":
    sys.exit(main())
