"""Dev: what per-tensor statistics (qpn_tensor_stats: train_stats.hip) cost.      python tools/tensor_stats_rate.py --calls [--geometry paper|default] | --loop [--rounds 3] [--steps 1500]

--calls: 200 qpn_tensor_stats calls each at the paper-size and the repo-default parameter counts, on the models' own tensor tables and buffers made like a step's
(run it under `rocprofv3 --kernel-trace --stats`, one geometry per run, for the two kernels' times; it prints the call's wall time -- launches, drain, read-back -- and the byte floor
16 n / HBM rate itself).
--loop: the run_train loop as bench.runner_loop_rate restates it (loader -> depth-2 prefetch thread -> FusedTrainer.step(want_loss="lagged"), the loss flushed every
100 steps) on the paper-size model, WITHOUT the report (what the loop always did: the parent commit's behaviour) and WITH it every 100 steps (flush, check_status,
tensor_stats, one JSON line to a scratch file: run_train --stats_interval 100), in alternating rounds."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes/s: the spec and the measured float4 copy rate of an MI355X


def _host_line():
    try:
        info = [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")]
        return "host: %s x %d, affinity %d cpus, load %s" % (info[0], len(info), len(os.sched_getaffinity(0)), open("/proc/loadavg").read().strip())
    except Exception as e:
        return "host: ? %s" % e


def calls(n_calls, which):
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER, DEFAULT
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    for name, cfg in (("paper", PAPER), ("default", DEFAULT)):
        if which not in ("both", name):
            continue
        hp = C.c_void_p()
        _lib.check(L.qpn_create(C.byref(_lib.make_config(cfg)), C.byref(hp)))
        ends, o = [], 0
        for _, shp in cfg.param_layout():
            o += int(np.prod(shp))
            ends.append(o)
        n, nt = o, len(ends)
        gen = torch.Generator(device=dev).manual_seed(1)
        w = torch.randn(n, device=dev, generator=gen) * 0.1
        g = torch.randn(n + 4, device=dev, generator=gen) * 0.01
        m = torch.randn(n, device=dev, generator=gen) * 0.003
        v = (torch.randn(n, device=dev, generator=gen) * 0.01) ** 2
        table, out = (C.c_int64 * nt)(*ends), (_lib.QpnTensorStat * nt)()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def call():
            _lib.check(L.qpn_tensor_stats(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3, 0.9, 0.999, 1e-8, None, nt, table, out, stream))
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            call()
        dt = (time.perf_counter() - t0) / n_calls
        items = sum(-(-(e - s) // 2048) for s, e in zip([0] + ends[:-1], ends))
        print("%s: n = %d, %d tensors, %d work items; the call (two launches, drain, %d bytes read back): %.1f us wall; byte floor 16 n = %.2f MB: %.2f us at %.1f TB/s, %.2f us at %.2f TB/s"
              % (name, n, nt, items, 40 * nt, dt * 1e6, 16 * n / 1e6, 16 * n / HBM_PEAK * 1e6, HBM_PEAK / 1e12, 16 * n / HBM_COPY * 1e6, HBM_COPY / 1e12), flush=True)
        L.qpn_destroy(hp)


def loop(rounds, steps):
    import torch
    from qpnet_amd import loaders, synth
    from qpnet_amd.config import PAPER as cfg
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.runners import PinnedStager, Prefetcher
    from qpnet_amd.train import FusedTrainer
    dev = torch.device("cuda", 0)
    flat = synth.make_weights(cfg, 13)
    m = QPNet(**cfg.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()})
    m = m.to(dev).train()
    tr = FusedTrainer(m, lr=1e-4)
    U = cfg.upsampling_factor
    rs = np.random.RandomState(0)
    utts = []
    for i in range(24):
        nf = int(rs.randint(600, 1200))                 # 3-6 s utterances (bench.runner_loop_rate's corpus)
        utts.append((rs.uniform(-1, 1, nf * U + 5).astype(np.float32), synth.make_features(nf, 400 + i, 45.0, 300.0)))
    mean, scale = synth.scaler_stats()
    fields = (cfg.receptiveCausal_field, cfg.receptiveF_field, cfg.receptiveA_field)
    wav_t, feat_t = loaders.mu_law_transform(cfg.n_quantize), (lambda h: (h - mean) / scale)

    def batches():
        np.random.seed(1)
        gen = loaders.train_generator(utts, *fields, 22050, wav_transform=wav_t, feat_transform=feat_t, batch_length=20000, max_length=30000, upsampling_factor=U, shuffle=True)
        stage = PinnedStager(dev)
        for bx, bh, bt, bd, bb in gen:
            dv = stage({"x": bx, "h": bh, "t": bt, "d": bd})
            yield dv["x"], dv["h"], dv["t"], dv["d"], bb, int(np.ceil(float(bd.max())))

    def run(stats_interval, sink):
        stream = Prefetcher(batches())
        for _ in range(20):
            bx, bh, bt, bd, bb, maxd = next(stream)
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
        tr.flush_loss()
        torch.cuda.synchronize()
        t_stats, n_stats = 0.0, 0
        t0 = time.perf_counter()
        for i in range(steps):
            bx, bh, bt, bd, bb, maxd = next(stream)
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
            if (i + 1) % 100 == 0:
                tr.flush_loss()
                tr.check_status()
            if stats_interval and (i + 1) % stats_interval == 0:
                a = time.perf_counter()
                sink.write(json.dumps({"iter": i + 1, "tensors": tr.tensor_stats()}) + "\n")
                t_stats += time.perf_counter() - a; n_stats += 1
        tr.flush_loss()
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0), t_stats / max(n_stats, 1) * 1e6

    print(_host_line())
    with tempfile.TemporaryFile("w") as sink:
        for r in range(rounds):
            for name, interval in (("no report         ", 0), ("report every 100  ", 100)):
                rate, per = run(interval, sink)
                print("round %d %s: %.0f steps/s = %.1f us per iteration%s (load %s)"
                      % (r, name, rate, 1e6 / rate, "; tensor_stats() + the JSON line: %.0f us per report" % per if interval else "", open("/proc/loadavg").read().split()[0]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--n_calls", type=int, default=200)
    ap.add_argument("--geometry", default="both", choices=["both", "paper", "default"], help="--calls: one geometry only (a kernel trace per size)")
    args = ap.parse_args()
    if not (args.calls or args.loop):
        ap.error("--calls and / or --loop")
    if args.calls:
        calls(args.n_calls, args.geometry)
    if args.loop:
        loop(args.rounds, args.steps)
