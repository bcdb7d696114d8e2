"""Dev: the run_train loop fed by the host loader against the same loop fed by the device-resident corpus (loaders.DeviceCorpus / device_train_generator), on
the paper-size model and the in-memory corpus of bench.runner_loop_rate: steps/s of each loop in alternating rounds, where an iteration spends its host time
(main thread: waiting for the batch / inside step(); loader thread: per batch), the fused step alone on resident inputs as the ceiling, and the corpus's build
time and bytes.      python tools/device_corpus_rate.py [--rounds 3] [--steps 1500] [--host_only]
--host_only: the host loop alone (runs on a tree from before the device corpus: the side-by-side figure of the parent commit)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--host_only", action="store_true")
    args = ap.parse_args()
    import torch
    from qpnet_amd import loaders, synth
    from qpnet_amd.config import PAPER as cfg
    from qpnet_amd.qpnet import QPNet
    from qpnet_amd.runners import PinnedStager, Prefetcher
    from qpnet_amd.train import FusedTrainer
    try:
        info = [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")]
        print("host: %s x %d, affinity %d cpus, load %s" % (info[0], len(info), len(os.sched_getaffinity(0)), open("/proc/loadavg").read().strip()))
    except Exception as e:
        print("host: ?", e)
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
    tgen = [0.0, 0]

    def timed(gen):
        it = iter(gen)
        while True:
            t0 = time.perf_counter()
            b = next(it)
            tgen[0] += time.perf_counter() - t0; tgen[1] += 1
            yield b

    def host_batches():
        np.random.seed(1)
        gen = loaders.train_generator(utts, *fields, 22050, wav_transform=wav_t, feat_transform=feat_t, batch_length=20000, max_length=30000, upsampling_factor=U, shuffle=True)
        stage = PinnedStager(dev)
        for bx, bh, bt, bd, bb in gen:
            dv = stage({"x": bx, "h": bh, "t": bt, "d": bd})
            yield dv["x"], dv["h"], dv["t"], dv["d"], bb, int(np.ceil(float(bd.max())))
    corpus = None
    if not args.host_only:
        t0 = time.perf_counter()
        corpus = loaders.DeviceCorpus(utts, U, 22050, 8, 0, wav_t, feat_t, dev)
        print("device corpus: %d utterances, %d frames, %d bytes, built in %.3f s" % (corpus.n_utterances, corpus.n_frames, corpus.nbytes, time.perf_counter() - t0))

    def device_batches():
        np.random.seed(1)
        return loaders.device_train_generator(corpus, *fields, 20000, 1, 30000, True, None, None)

    def loop(make, steps):
        stream = Prefetcher(timed(make()))
        for _ in range(20):
            bx, bh, bt, bd, bb, maxd = next(stream)
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
        tr.flush_loss()
        torch.cuda.synchronize()
        tgen[0], tgen[1] = 0.0, 0
        w_next = w_step = 0.0
        t0 = time.perf_counter()
        for i in range(steps):
            a = time.perf_counter()
            bx, bh, bt, bd, bb, maxd = next(stream)
            b = time.perf_counter()
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
            w_next += b - a; w_step += time.perf_counter() - b
            if (i + 1) % 100 == 0:
                tr.flush_loss()
        tr.flush_loss()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return steps / dt, w_next / steps * 1e6, w_step / steps * 1e6, tgen[0] / max(tgen[1], 1) * 1e6

    def resident(steps):
        """the fused step alone: one chunk resident on the device, nothing made or copied per step"""
        np.random.seed(1)
        bx, bh, bt, bd, bb, maxd = next(host_batches())
        torch.cuda.synchronize()
        for _ in range(20):
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
        tr.flush_loss(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            tr.step(bx, bh, bt, bd, bb, want_loss="lagged", maxd=maxd)
        tr.flush_loss(); torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)
    loops = [("host loader  ", host_batches)] + ([] if args.host_only else [("device corpus", device_batches)])
    for r in range(args.rounds):
        for name, make in loops:
            rate, w_next, w_step, per_batch = loop(make, args.steps)
            print("round %d %s: %.0f steps/s = %.0f us per iteration: main thread waits %.0f us for the batch, %.0f us in step(); loader thread %.0f us per batch"
                  % (r, name, rate, 1e6 / rate, w_next, w_step, per_batch), flush=True)
        print("round %d resident chunk: %.0f steps/s (load %s)" % (r, resident(args.steps), open("/proc/loadavg").read().split()[0]), flush=True)


if __name__ == "__main__":
    main()
