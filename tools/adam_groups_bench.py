"""Dev: what parameter groups cost inside the Adam launch (qpn_adam_groups) -> profiles/adam_groups.txt.

Times, with HIP events, in ONE process, the launches taken in turn (the order rotates from round to round, so that clock and cache state are shared), after a warm-up:
  plain       the launch without groups (k_adam)
  one-group   the grouped launch with one group over [0, n)
  adaptation  the grouped launch with the adaptation table: everything frozen except aux* and conv_post_*, conv_post_2.* a group of its own
at n = the paper-size and the repo-default parameter count.  28 bytes move per updated element (w, m, v read and written, g read); a frozen element moves none.

    python tools/adam_groups_bench.py [--reps 300] [--out profiles/adam_groups.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FROZEN = ["causal.*", "upsampling.*", "dil*", "res*", "skip*"]


def main():
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER, DEFAULT, ADAM_FROZEN, adam_group_table
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_groups.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = ["# tools/adam_groups_bench.py: %d launches each after %d warm-up rounds, taken in turn in one process, HIP events around every launch; median (min) in us" % (args.reps, args.warmup),
             "# device: %s" % torch.cuda.get_device_name(dev)]
    for name, cfg in (("paper", PAPER), ("default", DEFAULT)):
        n = cfg.n_params
        w, g, m, v = (torch.randn(n, device=dev) * s for s in (0.1, 0.01, 0.003, 0.0))
        v = v + 1e-4
        stream = torch.cuda.current_stream(dev).cuda_stream
        seg_end, seg_group, key_group = adam_group_table(cfg, [(FROZEN, ADAM_FROZEN), ("conv_post_2.*", 1)], 0)
        n_train = sum(int(np.prod(shp)) for k, shp in cfg.param_layout() if key_group[k] >= 0)
        tables = {"plain": None, "one-group": ([n], [0]), "adaptation": (seg_end, seg_group)}
        lr, wd = (C.c_float * 2)(1e-4, 5e-5), (C.c_float * 2)(0.0, 0.0)
        handles = {}                                     # the groups are sticky on a handle: one handle per table, nothing is switched between launches
        for k, t in tables.items():
            hp = C.c_void_p()
            _lib.check(L.qpn_create(C.byref(_lib.make_config(cfg)), C.byref(hp)))
            if t is not None:
                _lib.check(L.qpn_adam_groups(hp, 2, lr, wd, len(t[0]), (C.c_int64 * len(t[0]))(*t[0]), (C.c_int32 * len(t[1]))(*t[1]), stream))
            handles[k] = hp

        def launch(kind):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.qpn_adam_step(handles[kind], w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3, 1e-4, 0.9, 0.999, 1e-8, 0.0, stream))
            e1.record()
            return e0, e1

        times = {k: [] for k in tables}
        for r in range(args.warmup + args.reps):
            order = list(tables)
            order = order[r % 3:] + order[:r % 3]            # (every launch follows every other equally often: what the one before left in the caches is shared out)
            evs = [(k, launch(k)) for k in order]
            torch.cuda.synchronize()
            if r >= args.warmup:
                for k, (e0, e1) in evs:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        for hp in handles.values():
            L.qpn_destroy(hp)
        base = float(np.median(times["plain"]))
        lines.append("n = %d (%s): %d segments in the adaptation table, %d trainable elements (%.1f %%)" % (n, name, len(seg_end), n_train, 100.0 * n_train / n))
        for k in tables:
            t = np.array(times[k])
            moved = 28.0 * (n_train if k == "adaptation" else n)
            lines.append("  %-11s %9.2f (%9.2f) us   %5.2f x plain   %7.1f GB/s of weight, moment and gradient traffic" % (
                k, np.median(t), t.min(), np.median(t) / base, moved / np.median(t) / 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
