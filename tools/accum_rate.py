"""Gradient accumulation: what it costs, measured on the GPU.

    python tools/accum_rate.py --kernel                          # k_grad_accum alone, HIP events: bytes moved per second at the paper-size and the
                                                                 # repo-default parameter count, first = 1 and first = 0
    python tools/accum_rate.py --window --accum_steps K          # bench.py's training workload (paper-size model, its four chunks) through FusedTrainer(accum_steps=K),
                                                                 # and through run_train's loop (generator -> pinned staging -> prefetch thread -> lagged losses): chunks / s
    python tools/accum_rate.py --window --root <other checkout>  # the same loops on another checkout's package (a build of the parent commit: K = 1 only)

Every invocation prints one JSON line.  Compare versions by running them alternately in one session (other work shares the host); a run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HBM_BYTES_PER_S = 6.29e12          # the float4-copy rate the microarchitecture notes quote for the MI355X (8.0 TB/s on paper)


def _kernel(args):
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER, DEFAULT
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(PAPER)), C.byref(hp)))
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = []
    for name, n in (("paper", PAPER.n_params), ("default", DEFAULT.n_params)):
        cnt = n + 4
        acc = torch.zeros(cnt, dtype=torch.float32, device=dev)
        g = torch.full((cnt,), 1e-3, dtype=torch.float32, device=dev)
        for first in (1, 0):
            reps = args.reps
            for _ in range(20):
                _lib.check(L.qpn_grad_accumulate(hp, acc.data_ptr(), g.data_ptr(), cnt, first, stream))
            torch.cuda.synchronize()
            # (a) back to back on one stream: what a launch costs where it sits, between two kernels of a step (launch boundary included)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                L.qpn_grad_accumulate(hp, acc.data_ptr(), g.data_ptr(), cnt, first, stream)
            e1.record(); torch.cuda.synchronize()
            chain_us = e0.elapsed_time(e1) * 1e3 / reps
            # (b) one launch between two events, the median of many
            single = []
            for _ in range(min(reps, 200)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); L.qpn_grad_accumulate(hp, acc.data_ptr(), g.data_ptr(), cnt, first, stream); b.record()
                b.synchronize()
                single.append(a.elapsed_time(b) * 1e3)
            nbytes = cnt * 4 * (2 if first else 3)
            out.append({"model": name, "floats": cnt, "first": first, "bytes": nbytes, "us_back_to_back": round(chain_us, 3), "us_single_median": round(float(np.median(single)), 3),
                        "TB_per_s_back_to_back": round(nbytes / chain_us / 1e6, 3), "of_hbm_rate": round(nbytes / chain_us / 1e6 / (HBM_BYTES_PER_S / 1e12), 3)})
    L.qpn_destroy(hp)
    return {"what": "k_grad_accum alone", "hbm_TB_per_s": HBM_BYTES_PER_S / 1e12, "reps": args.reps, "rows": out}


def _window(args):
    import torch
    from qpnet_amd import synth, loaders
    from qpnet_amd.config import PAPER
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.train import FusedTrainer
    from qpnet_amd.runners import PinnedStager, Prefetcher
    dev = torch.device("cuda", 0)
    cfg, K = PAPER, args.accum_steps
    kw = {"accum_steps": K} if K > 1 else {}                      # (K = 1: the constructor call every checkout accepts)

    def model():
        m = QPNet(**cfg.kwargs())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, synth.make_weights(cfg, 13)).items()})
        return m.to(dev).train()

    # ---- FusedTrainer directly: bench.py's chunks, want_loss=False, the device kept busy before the timed window as bench.py does
    m = model()
    tr = FusedTrainer(m, lr=1e-4, **kw)
    host = [synth.train_inputs(cfg, 20000, 5000 + 17 * i, 30000, f0_lo=45.0, f0_hi=300.0, pin_f0_floor=True) for i in range(4)]
    batches = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in hb] for hb in host]
    maxds = [int(np.ceil(hb[3]).max()) for hb in host]

    def step(i):
        x, h, t, d, _ = batches[i % 4]
        tr.step(x, h, t, d, host[i % 4][4], want_loss=False, maxd=maxds[i % 4])
    step(0); torch.cuda.synchronize()
    t0, i = time.perf_counter(), 1
    while (time.perf_counter() - t0) < 0.04 or i % K:
        step(i); i += 1
    for j in range(args.warmup * K):
        step(j)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for j in range(args.steps * K):
        step(j)
    torch.cuda.synchronize()
    direct = args.steps * K / (time.perf_counter() - t0)
    tr.check_status()
    updates = tr.step_count
    # ---- run_train's loop (bench.py's runner_loop_rate with the window inside an iteration, as runners.run_train has it)
    m = model()
    tr = FusedTrainer(m, lr=1e-4, **kw)
    U = cfg.upsampling_factor
    rs = np.random.RandomState(0)
    utts = []
    for k in range(24):
        nf = int(rs.randint(600, 1200))
        utts.append((rs.uniform(-1, 1, nf * U + 5).astype(np.float32), synth.make_features(nf, 400 + k, 45.0, 300.0)))
    mean, scale = synth.scaler_stats()
    np.random.seed(1)
    gen = loaders.train_generator(utts, cfg.receptiveCausal_field, cfg.receptiveF_field, cfg.receptiveA_field, 22050,
                                  wav_transform=loaders.mu_law_transform(cfg.n_quantize), feat_transform=lambda h: (h - mean) / scale,
                                  batch_length=20000, max_length=30000, upsampling_factor=U, shuffle=True)
    stage = PinnedStager(dev)

    def staged():
        for bx, bh, bt, bd, bb in gen:
            dv = stage({"x": bx, "h": bh, "t": bt, "d": bd})
            yield dv["x"], dv["h"], dv["t"], dv["d"], bb, int(np.ceil(float(bd.max())))
    stream = Prefetcher(staged())

    def iteration():
        got = 0
        for _ in range(K):
            bx, bh, bt, bd, bb, maxd = next(stream)
            got += tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd) is not None
        return got
    for _ in range(5):
        iteration()
    tr.flush_loss()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    got = 0
    for it in range(args.runner_iters):
        got += iteration()
        if (it + 1) % 100 == 0:
            got += tr.flush_loss() is not None
    got += tr.flush_loss() is not None
    torch.cuda.synchronize()
    runner = args.runner_iters * K / (time.perf_counter() - t0)
    tr.check_status()
    assert got == args.runner_iters * K, (got, args.runner_iters * K)
    return {"what": "chunks per second, paper-size model, bench.py's chunk", "root": args.root or ".", "accum_steps": K, "trainer_chunks_per_s": round(direct, 1),
            "run_train_loop_chunks_per_s": round(runner, 1), "timed_chunks": args.steps * K, "runner_chunks": args.runner_iters * K, "updates_applied_in_trainer_run": updates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--window", action="store_true")
    ap.add_argument("--accum_steps", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300, help="timed updates of the FusedTrainer loop (K chunks each)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runner_iters", type=int, default=300, help="timed updates of the run_train-style loop (K chunks each)")
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--root", default=None, help="another checkout whose qpnet_amd package (built) is measured instead of this one's")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_rate.py measures on the GPU: none here")
    if args.kernel:
        print(json.dumps(_kernel(args)), flush=True)
    if args.window:
        print(json.dumps(_window(args)), flush=True)


if __name__ == "__main__":
    main()
