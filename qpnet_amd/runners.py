"""Task entry points over the native hot path: train / SD-update / validate / decode.

Same command-line flags and on-disk artefacts as the reference task scripts
  src/bin/qpnet_train.py    (main loop :517-567, resume :481-499, checkpoints :338-353)
  src/bin/qpnet_update.py   (--pretrain / --resume :444-464)
  src/bin/qpnet_validate.py (validation_result.yml :409-437)
  src/bin/qpnet_decode.py   (per-GPU split :258-259,322-331; wav writing :315-320)
but the loop body is the fused step behind the C ABI (FusedTrainer) and multi-GPU is one process per GPU
(torch.distributed / RCCL): rank r consumes chunks r, r+N, ... of the generator stream and the flat gradient is
all-reduced once per step (with --accum_steps K: once per window of K chunks, and an iteration is one update); decode splits the utterance list over ranks with no
communication.

    python -m qpnet_amd.run_train    --waveforms .. --feats .. --stats .. --expdir .. --config .. [--n_gpus N]
    python -m qpnet_amd.run_update   ... --pretrain checkpoint-final.pkl
    python -m qpnet_amd.run_validate ... --checkpoint .. --resultdir .. [--per_utterance]
    python -m qpnet_amd.run_decode   --feats .. --stats .. --config .. --checkpoint .. --outdir out/feat_id.wav

With --n_gpus N > 1 and no torchrun environment the entry point re-launches itself as N ranks (before any GPU call).
"""
import argparse
import json
import logging
import os
import queue
import subprocess
import sys
import threading
import time

import numpy as np
import torch
import yaml

from . import loaders


# ---------------------------------------------------------------- shared plumbing
def _setup_logging(verbose):
    level = logging.INFO if verbose == 1 else logging.DEBUG if verbose > 1 else logging.WARN
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s",
                        datefmt="%m/%d/%Y %I:%M:%S")


def _fix_seed(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


def launch_ranks(n_gpus, module, argv):
    """Re-launch `python -m module argv` as n_gpus ranks under torch.distributed.run (the parent never touches the GPU);
    returns the children's exit code, or None when this process already is a rank / runs single-GPU."""
    if n_gpus <= 1 or "RANK" in os.environ:
        return None
    port = 29500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", module] + list(argv)
    return subprocess.call(cmd)


def dist_context():
    """(rank, world, device): initialises the process group when launched as ranks (backend nccl = RCCL; gloo when
    QPN_DIST_BACKEND=gloo, used by one-GPU rehearsals)."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("qpnet_amd needs an AMD GPU: there is no CPU fallback for the hot path")
    backend = os.environ.get("QPN_DIST_BACKEND", "nccl")
    dev_index = 0 if os.environ.get("QPN_BENCH_ONE_GPU") else local
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    return rank, world, dev


class PinnedStager:
    """Host-to-device copies of the loader's batches through a small ring of REUSED pinned staging buffers.

    `tensor.to(device)` from pageable memory goes through the runtime's own bounce buffers and blocks the calling thread: measured
    1150 chunks/s of 0.5 MB on the GPU box (tools/loader_rate.py) -- no faster than one GPU consumes them.  Staging into pinned memory
    first makes the copy a plain DMA (non_blocking=True really is): the ring is `depth` deep because a buffer may only be reused once the
    copy that read it has completed (an event per slot)."""

    def __init__(self, device, depth=4):
        self.device, self.depth = device, depth
        self.slots = [None] * depth                        # one pinned byte buffer per slot (grown on demand)
        self.events = [None] * depth
        self.i = 0
        # the copies run on a stream of their own: on the compute stream a 0.5 MB chunk is a DMA packet BETWEEN two of the step's kernels (the queue is in
        # order: ~25 us of every 705 us step with the compute units idle, tools/step_timeline.py on the run_train loop).  QPN_STAGE_STREAM=0: the caller's stream.
        self.copy_stream = torch.cuda.Stream(device) if (torch.device(device).type == "cuda" and os.environ.get("QPN_STAGE_STREAM", "1") != "0") else None

    def __call__(self, named):
        """named: {name: cpu tensor} -> {name: device tensor}.  ONE asynchronous copy on the current stream: the tensors are packed into the slot's
        pinned buffer at 256-byte offsets and land in one device buffer the results are views of (a chunk's four small tensors as four copies cost
        four in-stream DMA packets of ~5 us each between the step's kernels; tools/runner_prof.py)."""
        k = self.i
        if self.events[k] is not None:
            self.events[k].synchronize()                  # the copy that last read this slot is done
        offs, total = {}, 0
        for name, t in named.items():
            offs[name] = total
            total += (t.numel() * t.element_size() + 255) // 256 * 256
        buf = self.slots[k]
        if buf is None or buf.numel() < total:
            buf = torch.empty(max(total, 1) * 5 // 4, dtype=torch.uint8).pin_memory()
            self.slots[k] = buf
        for name, t in named.items():
            n = t.numel() * t.element_size()
            buf[offs[name]:offs[name] + n].view(t.dtype).view(t.shape).copy_(t)
        cs = self.copy_stream
        if cs is not None:
            with torch.cuda.stream(cs):
                dbuf = buf[:total].to(self.device, non_blocking=True)
        else:
            dbuf = buf[:total].to(self.device, non_blocking=True)
        out = {name: dbuf[offs[name]:offs[name] + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for name, t in named.items()}
        ev = torch.cuda.Event()
        ev.record(cs if cs is not None else torch.cuda.current_stream(self.device))
        self.events[k] = ev
        if cs is not None:
            # whoever consumes the batch joins the copy: FusedTrainer.step / forward_loss and QPNet.forward look at ALL their inputs (train.join_staged)
            for t in out.values():
                t.__dict__["_qpn_staged"] = (ev, dbuf)
        self.i = (self.i + 1) % self.depth
        return out


class Prefetcher:
    """Runs a generator on a daemon thread, `depth` items ahead (the reference wraps its generators in a depth-2
    background queue, utils.py:165-214)."""
    _END = object()

    def __init__(self, gen, depth=2):
        depth = int(os.environ.get("QPN_PREFETCH_DEPTH", depth))
        self.q = queue.Queue(maxsize=depth)
        self.err = None
        self.t = threading.Thread(target=self._run, args=(gen,), daemon=True)
        self.t.start()

    def _run(self, gen):
        try:
            for item in gen:
                self.q.put(item)
        except BaseException as e:      # surfaced on the consumer side
            self.err = e
        self.q.put(self._END)

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if item is self._END:
            if self.err is not None:
                raise self.err
            raise StopIteration
        return item


class _FileUtterance:
    """One (wav, feature file) pair of the corpus: called, it reads both (waveform in [-1, 1), features); `plan()` is what the sharded generator needs to lay
    the chunk stream out WITHOUT the waveform -- its length from the wav header (a memory map: no sample is read) and the features (the f0 column sets the
    dilated factors) -- so that a data-parallel rank reads the samples of the utterances its own chunks reach into only (loaders.train_generator)."""

    def __init__(self, wav, feat, feature_type):
        self.wav, self.feat, self.feature_type = wav, feat, feature_type
        self._x = self._h = None                       # memory maps of the wav samples / .npy features, opened by the first plan() / part() and kept

    def __call__(self):
        return loaders.read_wav(self.wav)[1], loaders.read_features(self.feat, self.feature_type)

    def _maps(self):
        if self._x is None:
            from scipy.io import wavfile
            self._x = wavfile.read(self.wav, mmap=True)[1]
            if self.feat.endswith(".npy"):
                self._h = np.load(self.feat, mmap_mode="r")
        return self._x, self._h

    def plan(self):
        x, h = self._maps()
        return int(x.shape[0]), (np.array(h) if h is not None else loaders.read_features(self.feat, self.feature_type))

    def part(self, s0, s1, f0, f1):
        """samples [s0, s1) as read_wav scales them and feature rows [f0, f1): the wav through a memory map (only the pages of the slice are read), .npy
        features likewise; an .h5 dataset is read whole (150 KB at 39 features x 5 ms frames) and sliced."""
        x, h = self._maps()
        xs = np.array(x[s0:s1], dtype=np.float32) / 32768
        if f1 <= f0:
            return xs, np.zeros((0, 0), dtype=np.float32)
        return xs, (np.array(h[f0:f1]) if h is not None else loaders.read_features(self.feat, self.feature_type)[f0:f1])


def _utterance_loaders(wav_list, feat_list, feature_type):
    """loaders (waveform in [-1,1), features) per utterance: files are read when the generator reaches them."""
    return [_FileUtterance(w, f, feature_type) for w, f in zip(wav_list, feat_list)]


def _batches(args, conf, model, shuffle, epochs, device, rank=0, world=1, fields=None, unvoiced_weight=None, device_corpus=None):
    """Training / validation batches on `device`.  unvoiced_weight (None: off): a seventh element, the chunk's (B, batch_length) sample weights
    (loaders.unvoiced_row_weights), staged with the chunk.  fields: (receptiveCausal_field, receptiveF_field, receptiveA_field) to cut the chunks for (None: the model's).  With world > 1 rank r takes chunks r, r+N, ... of the generator's
    stream (same seed on every rank: identical shuffles and chunk boundaries) INSIDE the generator: a rank encodes,
    scales, takes ceil(max d) of and copies to its GPU only its own chunks.  device_corpus ({"max_bytes": bound or None}; None: off): the corpus is encoded,
    scaled and uploaded once (loaders.DeviceCorpus, every rank the whole of it) and the same stream of batches is cut on the GPU (loaders.device_train_generator)."""
    wavs, feats = loaders.file_lists(args.waveforms, args.feats, conf.feature_format)
    logging.info("number of utterances = %d." % len(wavs))
    scaler = loaders.read_scaler_stats(args.stats, conf.feature_type)
    fs = loaders.read_wav(wavs[0])[0]
    if device_corpus is not None:
        t0 = time.time()
        # (plain loads, not _FileUtterance's maps: nothing of a file stays open once its utterance is packed)
        utts = [lambda w=w, f=f: (loaders.read_wav(w)[1], loaders.read_features(f, conf.feature_type)) for w, f in zip(wavs, feats)]
        corpus = loaders.DeviceCorpus(utts, conf.upsampling_factor, fs, conf.dense_factor, args.f0_threshold, loaders.mu_law_transform(conf.n_quantize), scaler,
                                      device, device_corpus.get("max_bytes"))
        logging.info("device corpus: %d utterances, %d frames, %d bytes on %s, built in %.2f s." % (corpus.n_utterances, corpus.n_frames, corpus.nbytes, device, time.time() - t0))
        return loaders.device_train_generator(corpus, *(fields or _fields_of(model)), args.batch_length, args.batch_size, args.max_length, shuffle, epochs,
                                              (rank, world) if world > 1 else None, unvoiced_weight)
    gen = loaders.train_generator(
        _utterance_loaders(wavs, feats, conf.feature_type), *(fields or _fields_of(model)), fs, wav_transform=loaders.mu_law_transform(conf.n_quantize), feat_transform=scaler,
        dense_factor=conf.dense_factor, batch_length=args.batch_length, batch_size=args.batch_size, max_length=args.max_length,
        f0_threshold=args.f0_threshold, upsampling_factor=conf.upsampling_factor, shuffle=shuffle, epochs=epochs,
        shard=(rank, world) if world > 1 else None)

    stage = PinnedStager(device)

    def with_maxd():            # ceil(max d) is known on the host here: the fused step then needs no device read-back
        for bx, bh, bt, bd, bb in gen:
            maxd = int(np.ceil(float(bd.max())))
            if unvoiced_weight is None:
                dv = stage({"x": bx, "h": bh, "t": bt, "d": bd})
                yield (dv["x"], dv["h"], dv["t"], dv["d"], bb, maxd)
            else:
                bw = torch.from_numpy(loaders.unvoiced_row_weights(bh.numpy(), int(bb[0]), conf.upsampling_factor, unvoiced_weight))
                dv = stage({"x": bx, "h": bh, "t": bt, "d": bd, "w": bw})
                yield (dv["x"], dv["h"], dv["t"], dv["d"], bb, maxd, dv["w"])
    return with_maxd()


def _fields_of(m):
    """(receptiveCausal_field, receptiveF_field, receptiveA_field) of a model or a configuration: what train_generator sizes its chunks from"""
    return (m.receptiveCausal_field, m.receptiveF_field, m.receptiveA_field)


def joint_fields(a, b):
    """the element-wise maximum of two models' receptive fields: a chunk cut for it is long enough for both (the training forward takes a chunk longer than its
    own receptive field + batch_length, inputs aligned at the end)"""
    return tuple(max(u, v) for u, v in zip(_fields_of(a), _fields_of(b)))


_DISTILL_FLAGS = ("teacher", "teacher_config", "distill_alpha", "distill_temperature", "teacher_ema")


def _distill_of(args, conf):
    """--teacher & co. -> None (no teacher: the run is what it always was), or {"checkpoint", "conf", "alpha", "temperature", "use_ema"} with the teacher's model
    configuration loaded and checked against the student's `conf`.  Every error is a SystemExit, before anything is trained.  The flags are taken OUT of `args`:
    the Namespace a training run pickles as its model configuration holds what it always held."""
    v = {k: getattr(args, k) for k in _DISTILL_FLAGS}
    for k in _DISTILL_FLAGS:
        delattr(args, k)
    if not v["teacher"]:
        if v["teacher_config"] or v["teacher_ema"]:
            raise SystemExit("--teacher_config / --teacher_ema need --teacher CHECKPOINT")
        return None
    if not v["teacher_config"]:
        raise SystemExit("--teacher %s needs --teacher_config MODEL_CONF (the teacher's geometry is not stored in its checkpoint)" % v["teacher"])
    for path in (v["teacher"], v["teacher_config"]):
        if not os.path.exists(path):
            raise SystemExit("--teacher: %s does not exist" % path)
    from .config import QPNetConfig
    from .train import _check_distill_scalars, check_distill_geometry
    try:
        alpha, temp = _check_distill_scalars(v["distill_alpha"], v["distill_temperature"])
        tconf = loaders.load_model_conf(v["teacher_config"])
        check_distill_geometry(conf, tconf)
        QPNetConfig(**loaders.model_kwargs(tconf))
    except (ValueError, AttributeError) as e:
        raise SystemExit("--teacher %s: %s" % (v["teacher"], e))
    return {"checkpoint": v["teacher"], "conf": tconf, "alpha": alpha, "temperature": temp, "use_ema": bool(v["teacher_ema"])}


def _build_model(conf, device):
    from .qpnet import QPNet, initialize
    model = QPNet(**loaders.model_kwargs(conf))
    model.apply(initialize)
    return model.to(device)


# ---------------------------------------------------------------- train / update
def _is_non_finite_norm(e):
    """the status error of a step whose gradient norm was inf / NaN (--max_grad_norm): the device applied nothing, the run may go on."""
    return getattr(e, "code", None) == -4 and "non-finite gradient norm" in str(e)


def _train_args(update):
    p = argparse.ArgumentParser()
    for name in ("waveforms", "feats", "stats", "expdir", "config"):
        p.add_argument("--" + name, required=True, type=str)
    if update:
        p.add_argument("--pretrain", required=True, type=str, help="SI model to adapt")
    else:
        for name, dflt in (("n_quantize", 256), ("n_aux", 39), ("n_resch", 512), ("n_skipch", 256), ("dilationF_depth", 4),
                           ("dilationF_repeat", 3), ("dilationA_depth", 4), ("dilationA_repeat", 1), ("kernel_size", 2),
                           ("dense_factor", 8), ("upsampling_factor", 110)):
            p.add_argument("--" + name, default=dflt, type=int)
        p.add_argument("--feature_type", default="world", type=str)
        p.add_argument("--feature_format", default="h5", type=str)
    p.add_argument("--batch_length", default=20000, type=int)
    p.add_argument("--batch_size", default=1, type=int)
    p.add_argument("--max_length", default=30000, type=int)
    p.add_argument("--f0_threshold", default=0, type=int)
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--weight_decay", default=0.0, type=float)
    p.add_argument("--max_grad_norm", default=0.0, type=float, help="clip the gradient norm inside the fused step (torch's clip_grad_norm_); 0: off")
    p.add_argument("--ema_decay", default=0.0, type=float, help="keep an exponential moving average of the weights inside the fused step, written to the checkpoints as \"ema\" (decode / validate with --ema); 0: off")
    p.add_argument("--accum_steps", default=1, type=int, help="gradient accumulation: one Adam update per K batches of the stream (an iteration is then one update: --iters, --intervals, --checkpoint_interval and the checkpoints count updates); 1: off")
    p.add_argument("--freeze", default=None, type=str, metavar="PATTERN[,PATTERN...]",
                   help="do not update the parameters whose state_dict names match (fnmatch), e.g. \"causal.*,dil*,res*,skip*\" adapts the conditioning path and the post-net only")
    p.add_argument("--lr_scale", default=[], action="append", metavar="PATTERNS=SCALE",
                   help="train the parameters whose names match PATTERN[,PATTERN...] at lr * SCALE (repeatable: a group of its own each)")
    p.add_argument("--teacher", default=None, type=str, metavar="CHECKPOINT",
                   help="knowledge distillation: train against this checkpoint's predicted distributions (the soft-target loss inside the fused step); the reported loss is then the distillation total")
    p.add_argument("--teacher_config", default=None, type=str, metavar="MODEL_CONF", help="the teacher's model configuration (required with --teacher)")
    p.add_argument("--distill_alpha", default=0.5, type=float, help="weight of the soft-target term, in (0, 1]; the hard cross entropy gets 1 - alpha")
    p.add_argument("--distill_temperature", default=1.0, type=float, help="temperature both distributions are softened with, > 0")
    p.add_argument("--teacher_ema", action="store_true", help="take the teacher checkpoint's averaged weights (a run with --ema_decay wrote them)")
    p.add_argument("--label_smoothing", default=0.0, type=float, metavar="EPS", help="label smoothing of the cross entropy inside the fused step, in [0, 1); 0: off")
    p.add_argument("--unvoiced_weight", default=1.0, type=float, metavar="W",
                   help="weight of the samples of unvoiced frames in the loss (voiced ones weigh 1; finite, >= 0; the loss stays a mean over the row count); 1: off")
    p.add_argument("--device_corpus", action="store_true", help="keep the encoded, scaled corpus on the GPU and cut every chunk there (the same stream of batches; "
                   "every rank holds the whole corpus); off: the host loader")
    p.add_argument("--device_corpus_max_gb", default=None, type=float, metavar="G", help="with --device_corpus: refuse a corpus above G GB on the device (default: half of the free device memory)")
    p.add_argument("--iters", default=3000 if update else 200000, type=int)
    p.add_argument("--checkpoint_interval", default=10000, type=int)
    p.add_argument("--intervals", default=100, type=int)
    p.add_argument("--stats_interval", default=0, type=int, metavar="N", help="every N iterations rank 0 appends the per-tensor statistics of the latest update (gradient, weight and "
                   "update norms: FusedTrainer.tensor_stats, a synchronous call) as one JSON line to <expdir>/tensor_stats.jsonl; 0: off")
    p.add_argument("--seed", default=1, type=int)
    p.add_argument("--resume", default=None, nargs="?", type=str)
    p.add_argument("--n_gpus", default=1, type=int)
    p.add_argument("--verbose", default=1, type=int)
    return p


def _param_groups_of(args):
    """--freeze / --lr_scale -> FusedTrainer's param_groups (None when neither is given)"""
    groups = []
    if args.freeze:
        groups.append({"params": [w for w in args.freeze.split(",") if w], "frozen": True})
    for spec in args.lr_scale:
        pats, sep, scale = spec.rpartition("=")
        if not sep or not pats:
            raise SystemExit("--lr_scale takes PATTERN[,PATTERN...]=SCALE, got %r" % spec)
        try:
            groups.append({"params": [w for w in pats.split(",") if w], "lr_scale": float(scale)})
        except ValueError:
            raise SystemExit("--lr_scale %r: %r is not a number" % (spec, scale))
    return groups or None


def run_train(argv=None, update=False):
    argv = sys.argv[1:] if argv is None else argv
    args = _train_args(update).parse_args(argv)
    sconf = None if not (args.teacher and args.teacher_config) else (loaders.load_model_conf(args.config) if update else argparse.Namespace(**vars(args)))
    distill = _distill_of(args, sconf)          # (--teacher & co.: checked, and taken out of args, before any rank is launched)
    # (the loss options are taken out of args as well: args is the model configuration run_train writes)
    label_smoothing, unvoiced_weight = args.__dict__.pop("label_smoothing"), args.__dict__.pop("unvoiced_weight")
    # (... and the loader's: --device_corpus changes where the batches are made, not the model)
    device_corpus, max_gb = args.__dict__.pop("device_corpus"), args.__dict__.pop("device_corpus_max_gb")
    if max_gb is not None and not device_corpus:
        raise SystemExit("--device_corpus_max_gb needs --device_corpus")
    if max_gb is not None and not (max_gb > 0.0 and np.isfinite(max_gb)):
        raise SystemExit("--device_corpus_max_gb must be finite and > 0, got %r" % (max_gb,))
    device_corpus = {"max_bytes": None if max_gb is None else int(max_gb * 1e9)} if device_corpus else None
    # (... and the report's: --stats_interval changes what is written next to the model, not the model)
    stats_interval = args.__dict__.pop("stats_interval")
    if stats_interval < 0:
        raise SystemExit("--stats_interval must be >= 0, got %r" % (stats_interval,))
    if not (0.0 <= label_smoothing < 1.0):
        raise SystemExit("--label_smoothing must lie in [0, 1), got %r" % (label_smoothing,))
    if not (unvoiced_weight >= 0.0 and np.isfinite(unvoiced_weight)):
        raise SystemExit("--unvoiced_weight must be finite and >= 0, got %r" % (unvoiced_weight,))
    if label_smoothing > 0.0 and distill is not None:
        raise SystemExit("--label_smoothing cannot be combined with --teacher (the soft targets already smooth)")
    if unvoiced_weight == 1.0:
        unvoiced_weight = None                  # (off: no weights are made or staged, nothing is armed)
    rc = launch_ranks(args.n_gpus, "qpnet_amd.run_update" if update else "qpnet_amd.run_train", argv)
    if rc is not None:
        return rc
    _setup_logging(args.verbose)
    rank, world, dev = dist_context()
    os.makedirs(args.expdir, exist_ok=True)
    _fix_seed(args.seed)                       # same seed on every rank: identical shuffles, so the chunk stream is shared
    if update:
        conf = loaders.load_model_conf(args.config)
    else:
        conf = args
        if args.upsampling_factor <= 0:
            logging.warning("upsampling_factor should larger than 0!")
            return 0
        if rank == 0:
            loaders.save_model_conf(args.config, args)
    from .train import FusedTrainer
    from . import parallel
    model = _build_model(conf, dev).train()
    teacher = fields = None
    if distill is not None:
        # the teacher: built from its own configuration, loaded once, never written (no optimiser, no entry in the checkpoints: --resume needs the flags again)
        from .qpnet import QPNet
        teacher = QPNet(**loaders.model_kwargs(distill["conf"])).to(dev).eval()
        loaders.load_checkpoint(distill["checkpoint"], teacher, None, use_ema=distill["use_ema"])
        teacher.requires_grad_(False)
        fields = joint_fields(model, teacher)           # every chunk is long enough for both models
        logging.info("distillation: teacher %s%s, receptive fields (causal, fixed, adaptive) student %s teacher %s -> chunks cut for %s; alpha = %g, T = %g; "
                     "the reported loss is the distillation total (1 - alpha) CE + alpha T^2 KL."
                     % (distill["checkpoint"], " (averaged weights)" if distill["use_ema"] else "", _fields_of(model), _fields_of(teacher), fields,
                        distill["alpha"], distill["temperature"]))
    trainer = FusedTrainer(model, lr=args.lr, weight_decay=args.weight_decay, world_size=world, max_grad_norm=args.max_grad_norm, ema_decay=args.ema_decay,
                           accum_steps=args.accum_steps, param_groups=_param_groups_of(args),
                           distill=None if teacher is None else {"teacher": teacher, "alpha": distill["alpha"], "temperature": distill["temperature"]},
                           label_smoothing=label_smoothing)
    if label_smoothing > 0.0 or unvoiced_weight is not None:
        logging.info("loss options: label_smoothing = %g, unvoiced_weight = %g (samples of unvoiced frames; voiced ones weigh 1); the reported loss is "
                     "sum_r w_r CE_r over the row count." % (label_smoothing, 1.0 if unvoiced_weight is None else unvoiced_weight))
    logging.info("trainable parameters = %d, frozen parameters = %d." % (trainer.n_trainable, trainer.n_frozen))
    clipping = trainer.max_grad_norm > 0.0
    K = trainer.accum_steps                    # batches per iteration: an iteration is one UPDATE (a window of K micro-steps), so checkpoints fall on window boundaries
    norm_max, n_clipped, n_seen = 0.0, 0, 0    # (clipping on) the interval's largest gradient norm, how many of its steps were clipped, how many losses it collected
    n_got = 0                                  # (K > 1) the micro-step losses that arrived in the interval: its reported loss is their mean

    def note_norm(g):
        # (a non-finite norm is the largest there is: max() would drop a NaN)
        nonlocal norm_max, n_clipped
        if g is not None:
            norm_max = float("nan") if g != g or norm_max != norm_max else max(norm_max, g)
            n_clipped += bool(g > trainer.max_grad_norm)

    def note_loss(v):
        # (K > 1: only a window-closing micro-step has a norm -- the None of the others is no step of the clipping statistics)
        nonlocal loss, n_got, n_seen
        loss += v; n_got += 1
        if clipping and (K == 1 or trainer.last_grad_norm is not None):
            n_seen += 1; note_norm(trainer.last_grad_norm)
    iterations, loss_record = 0, []
    flossyml = os.path.join(args.expdir, "loss-final.yml")
    if args.resume and os.path.exists(args.resume):
        iterations = loaders.load_checkpoint(args.resume, model, trainer)
        logging.info("restored from %d-iter checkpoint." % iterations)
        if os.path.exists(flossyml):
            with open(flossyml, encoding="utf-8") as yf:
                loss_record = yaml.safe_load(yf) or []
    elif update:
        loaders.load_checkpoint(args.pretrain, model, None)
        logging.info("updating based on %s." % args.pretrain)
    from .train import ensure_flat
    parallel.broadcast_parameters(ensure_flat(model, dev))
    stream = Prefetcher(_batches(args, conf, model, True, None, dev, rank, world, fields=fields, unvoiced_weight=unvoiced_weight, device_corpus=device_corpus))      # rank r: chunks r, r+N, r+2N, ...
    loss = total = 0.0
    logging.info("training start!")
    # The reference reads loss.item() at every step (qpnet_train.py:533) and reports its average over `intervals` steps (:536-541).  Here a step
    # returns the loss of the step BEFORE it (copied out behind that step's kernels: the device never idles while the host enqueues) and the last
    # one of an interval is fetched at the report: the same averages, the per-batch debug line one step late.  QPN_RUN_TRAIN_SYNC_LOSS=1: in-step.
    lagged = os.environ.get("QPN_RUN_TRAIN_SYNC_LOSS", "0") != "1"
    for i in range(iterations, args.iters):
        start = time.time()
        while True:                             # the K batches of this iteration's window (K = 1: the one batch)
            bx, bh, bt, bd, bb, maxd, *bw = next(stream)
            try:
                batch_loss = trainer.step(bx, bh, bt, bd, bb, want_loss="lagged" if lagged else True, maxd=maxd, sample_weights=bw[0] if bw else None)
            except Exception as e:
                if not (clipping and _is_non_finite_norm(e)):
                    raise
                batch_loss = None               # the device skipped that update (and those enqueued behind it): training goes on from the last clean state
                logging.warning("(iter:%d) %s" % (i + 1, e))
            if batch_loss is not None:
                note_loss(batch_loss)
                logging.debug("batch loss = %.3f" % batch_loss)
            if trainer.micro_step == 0:         # the window closed (or a status error abandoned it: the iteration ends with it)
                break
        total += time.time() - start
        stats_due = stats_interval > 0 and (i + 1) % stats_interval == 0
        if (i + 1) % args.intervals == 0 or (i + 1) % args.checkpoint_interval == 0 or i + 1 == args.iters or stats_due:
            last = trainer.flush_loss() if lagged else None
            if last is not None:
                note_loss(last)
            # the device-side checks of the last steps (a dilated factor outside the layer input, a target outside [0, n_quantize), an abandoned
            # stack launch: the reference asserts in every step, qpnet.py:294, qpnet_train.py:525) are collected HERE -- before an interval
            # is reported, before a checkpoint and before the final model are written: nothing flagged reaches the disk
            try:
                trainer.check_status()
            except Exception as e:
                if not (clipping and _is_non_finite_norm(e)):
                    raise
                logging.warning("(iter:%d) %s" % (i + 1, e))
        if stats_due and rank == 0 and trainer.step_count > 0 and trainer.micro_step == 0:
            # per-tensor statistics of the latest applied update (behind the checks above: what a flagged step left is reported as what it is), one JSON line
            with open(os.path.join(args.expdir, "tensor_stats.jsonl"), "a", encoding="utf-8") as sf:
                sf.write(json.dumps({"iter": i + 1, "tensors": trainer.tensor_stats()}) + "\n")
        if (i + 1) % args.intervals == 0:
            if clipping:
                # (a step that raised for a non-finite norm took the loss it would have returned with it: the average is over the losses that arrived)
                n_upd = n_seen if 0 < n_seen < args.intervals else args.intervals
                n_loss = n_upd if K == 1 else max(n_got, 1)
                logging.info("(iter:%d) average loss = %.6f (%.3f sec / batch) max grad norm = %.6g, %d of %d steps clipped"
                             % (i + 1, loss / n_loss, total / (args.intervals * K), norm_max, n_clipped, n_upd))
                norm_max, n_clipped, n_seen = 0.0, 0, 0
            else:
                n_loss = args.intervals if K == 1 else max(n_got, 1)
                logging.info("(iter:%d) average loss = %.6f (%.3f sec / batch)" % (i + 1, loss / n_loss, total / (args.intervals * K)))
            loss_record.append(loss / n_loss)
            loss = total = 0.0
            n_got = 0
        if (i + 1) % args.checkpoint_interval == 0 and rank == 0:
            loaders.save_checkpoint(args.expdir, model, trainer, i + 1)
    if world > 1:
        # every rank applied the same Adam step to the same summed gradient: the replicas must still be bit-identical (a rank that consumed a different
        # chunk count, a diverged knob or a lost collective shows here, before the final model is written)
        drift = parallel.replica_drift(ensure_flat(model, dev))
        if drift != 0.0:
            raise RuntimeError("data-parallel replicas drifted apart: max |w_r - w_0| = %g" % drift)
        if trainer.ema is not None:
            # ... and the same kernel moved every rank's average by the same weights
            drift = parallel.replica_drift(trainer.ema)
            if drift != 0.0:
                raise RuntimeError("data-parallel replicas' averaged weights drifted apart: max |e_r - e_0| = %g" % drift)
        logging.info("replicas identical on %d ranks." % world)
    if rank == 0:
        loaders.save_final(args.expdir, model, trainer)
        logging.info("final checkpoint created.")
        with open(flossyml, "w", encoding="utf-8") as yf:
            yaml.safe_dump([float(v) for v in loss_record], yf)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


def run_update(argv=None):
    return run_train(argv, update=True)


# ---------------------------------------------------------------- validate
def _validate_args():
    p = argparse.ArgumentParser()
    for name in ("waveforms", "feats", "stats", "resultdir", "config", "checkpoint"):
        p.add_argument("--" + name, required=True, type=str)
    p.add_argument("--batch_length", default=20000, type=int)
    p.add_argument("--batch_size", default=1, type=int)
    p.add_argument("--max_length", default=30000, type=int)
    p.add_argument("--f0_threshold", default=0, type=int)
    p.add_argument("--seed", default=1, type=int)
    p.add_argument("--n_gpus", default=1, type=int)
    p.add_argument("--verbose", default=1, type=int)
    p.add_argument("--ema", action="store_true", help="score the checkpoint's averaged weights (a run with --ema_decay wrote them)")
    p.add_argument("--per_utterance", action="store_true", help="after the pass above, score every file of the list on its own (batch size 1) and write per-file "
                   "nll / bits / top-1 / top-5 / entropy to <resultdir>/validation_utterances.yml")
    return p


def _score_entry(n, nll, ent, top1, top5):
    """one record of validation_utterances.yml from the sums over n samples"""
    return {"samples": int(n), "nll": float(nll / n), "bits": float(nll / n / np.log(2.0)), "top1": float(top1 / n), "top5": float(top5 / n),
            "entropy": float(ent / n)}


def score_utterances(args, conf, model, trainer, dev):
    """run_validate --per_utterance: every file of the list teacher-forced on its own, chunk by chunk (loaders.score_chunks; inputs made as the training
    generator makes them), through FusedTrainer.score -> {"total": entry, "utterances": {file id: entry}, "skipped": [file ids]}.  Of a file of n_frames
    frames the samples rf + 1 .. (n_frames - 1) U are scored, rf the receptive field under the file's own largest dilated factor; a file too short to
    have one is skipped.  The sums are float64 on the device: one read-back per file."""
    wavs, feats = loaders.file_lists(args.waveforms, args.feats, conf.feature_format)
    scaler = loaders.read_scaler_stats(args.stats, conf.feature_type)
    wav_transform = loaders.mu_law_transform(conf.n_quantize)
    U = int(conf.upsampling_factor)
    from . import harness
    utts, skipped, tot = {}, [], np.zeros(5)
    for wav, feat in zip(wavs, feats):
        fid = os.path.splitext(os.path.basename(wav))[0]
        fs, x = loaders.read_wav(wav)
        x, h = harness.validate_length(x, np.asarray(loaders.read_features(feat, conf.feature_type)), U)
        chunks = []
        if h.shape[0] > 0:
            d = harness.dilated_factor(harness.batch_f0(h, args.f0_threshold), fs, conf.dense_factor)
            rf = harness.receptive_field(model.receptiveCausal_field, model.receptiveF_field, model.receptiveA_field, d)
            chunks = loaders.score_chunks(h.shape[0], rf, args.batch_length, args.max_length, U)
        if not chunks:
            logging.warning("%s: too short to score (%d frames), skipped." % (fid, h.shape[0]))
            skipped.append(fid)
            continue
        xq = torch.from_numpy(np.asarray(wav_transform(x))).long()
        hs = torch.from_numpy(np.asarray(scaler(h))).float()
        acc = torch.zeros(5, dtype=torch.float64, device=dev)
        for frame0, frames, bl, keep in chunks:
            a, T = frame0 * U, frames * U
            dc = np.repeat(d[frame0:frame0 + frames], U)
            s = trainer.score(xq[a:a + T][None].to(dev), hs[frame0:frame0 + frames].transpose(0, 1)[None].to(dev), xq[a + 1:a + T + 1][None].to(dev),
                              torch.from_numpy(dc).float()[None].to(dev), [bl], maxd=int(np.ceil(float(dc.max()))))
            tg = xq[a + T + 1 - keep:a + T + 1].to(dev)
            acc += torch.stack([s.nll[0, -keep:].double().sum(), s.entropy[0, -keep:].double().sum(), (s.argmax[0, -keep:] == tg).sum().double(),
                                (s.rank[0, -keep:] < 5).sum().double(), torch.tensor(float(keep), dtype=torch.float64, device=dev)])
        nll, ent, top1, top5, n = acc.tolist()
        if not np.isfinite(nll):
            raise ValueError("%s: a target sample lies outside [0, n_quantize = %d) (its nll is %r)" % (fid, conf.n_quantize, nll))
        utts[fid] = _score_entry(n, nll, ent, top1, top5)
        tot += (nll, ent, top1, top5, n)
        logging.info("%s: %d samples, nll = %.6f, top1 = %.4f" % (fid, n, utts[fid]["nll"], utts[fid]["top1"]))
    return {"total": _score_entry(tot[4], tot[0], tot[1], tot[2], tot[3]) if tot[4] > 0 else {"samples": 0}, "utterances": utts, "skipped": skipped}


def run_validate(argv=None):
    args = _validate_args().parse_args(sys.argv[1:] if argv is None else argv)
    _setup_logging(args.verbose)
    # validation is one forward-only pass over the list (reference qpnet_validate.py:409-437): a single process.  --n_gpus is
    # accepted for command-line compatibility; under a multi-rank launcher rank 0 evaluates and writes the yml, the other
    # ranks leave at once (no process group is created, nothing to tear down)
    if int(os.environ.get("RANK", "0")) != 0:
        return 0
    if args.n_gpus > 1:
        logging.warning("validation runs on one GPU; --n_gpus %d ignored" % args.n_gpus)
    if not torch.cuda.is_available():
        raise RuntimeError("qpnet_amd needs an AMD GPU: there is no CPU fallback for the hot path")
    local = 0 if os.environ.get("QPN_BENCH_ONE_GPU") else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    _fix_seed(args.seed)
    conf = loaders.load_model_conf(args.config)
    from .train import FusedTrainer
    model = _build_model(conf, dev).eval()
    loaders.load_checkpoint(args.checkpoint, model, None, use_ema=args.ema)
    logging.info("load %s%s." % (args.checkpoint, " (averaged weights)" if args.ema else ""))
    trainer = FusedTrainer(model)
    flossyml = os.path.join(args.resultdir, "validation_result.yml")
    results = {}
    if os.path.exists(flossyml):
        with open(flossyml, encoding="utf-8") as yf:
            results = yaml.safe_load(yf) or {}
    loss, n = 0.0, 0
    for bx, bh, bt, bd, bb, maxd in _batches(args, conf, model, False, 1, dev):
        v = trainer.forward_loss(bx, bh, bt, bd, bb, maxd=maxd)
        loss += v; n += 1
        logging.info("(batch:%d) batch loss = %.6f" % (n, v))
    results[str(os.path.basename(args.checkpoint))] = float(loss / max(n, 1))
    os.makedirs(args.resultdir, exist_ok=True)
    with open(flossyml, "w", encoding="utf-8") as yf:
        yaml.safe_dump(results, yf)
    if args.per_utterance:
        futtyml = os.path.join(args.resultdir, "validation_utterances.yml")
        per_file = {}
        if os.path.exists(futtyml):
            with open(futtyml, encoding="utf-8") as yf:
                per_file = yaml.safe_load(yf) or {}
        per_file[str(os.path.basename(args.checkpoint))] = score_utterances(args, conf, model, trainer, dev)
        with open(futtyml, "w", encoding="utf-8") as yf:
            yaml.safe_dump(per_file, yf)
    return 0


# ---------------------------------------------------------------- decode
def _decode_args():
    p = argparse.ArgumentParser()
    for name in ("feats", "stats", "config", "outdir", "checkpoint"):
        p.add_argument("--" + name, required=True, type=str)
    p.add_argument("--fs", default=22050, type=int)
    p.add_argument("--batch_size", default=1, type=int)
    p.add_argument("--extra_memory", default=False, type=lambda s: str(s).lower() in ("1", "true", "yes", "y", "t", "on"))
    p.add_argument("--intervals", default=1000, type=int)
    p.add_argument("--seed", default=100, type=int)
    p.add_argument("--n_gpus", default=1, type=int)
    p.add_argument("--verbose", default=1, type=int)
    p.add_argument("--f0_factor", default=1.0, type=float)
    p.add_argument("--f0_dim_index", default=1, type=int)
    p.add_argument("--mode", default="sampling", choices=["sampling", "argmax"], help="the reference script always samples")
    p.add_argument("--ema", action="store_true", help="decode with the checkpoint's averaged weights (a run with --ema_decay wrote them)")
    p.add_argument("--temperature", default=1.0, type=float, help="sampling mode: draw from softmax(logits / temperature); 1: the reference's draw")
    p.add_argument("--top_k", default=0, type=int, help="sampling mode: draw among the classes with the top_k largest logits only (ties kept); 0: off")
    p.add_argument("--top_p", default=1.0, type=float, help="sampling mode: draw among the most probable classes whose mass reaches this fraction (ties kept); 1: off")
    p.add_argument("--min_p", default=0.0, type=float, help="sampling mode: draw among the classes at least this fraction as probable as the most probable one; 0: off")
    for name, typ in (("temperature", float), ("top_k", int), ("top_p", float), ("min_p", float)):
        for part in ("voiced", "unvoiced"):      # unset: the plain flag's value.  With none of the eight set the call is the one it always was
            p.add_argument("--%s_%s" % (name, part), default=None, type=typ, help="sampling mode: --%s of the samples whose feature frame is %s (feature column 0, the "
                           "uv flag; loaders.uv_draw_track); unset: the value of --%s" % (name, part, name))
    p.add_argument("--per_file_seed", action="store_true", help="sampling mode: every file draws from a stream of its own, keyed by --seed and the file's id "
                   "(loaders.row_seed): its wav does not depend on --batch_size, --n_gpus or the other files of the list; off: the reference-like per-call stream")
    return p


def uv_decode_controls(args):
    """run_decode's draw flags -> (plain, voiced, unvoiced): the keyword arguments of the four plain controls, and the two dicts of loaders.uv_draw_track for the
    controls that have a --<name>_voiced or --<name>_unvoiced flag set (the side left unset takes the plain flag's value; the plain keyword is then left at its default,
    the track carries the value).  None set: both dicts empty, and the call is the one the plain flags make."""
    plain, voiced, unvoiced = {}, {}, {}
    for name in ("temperature", "top_k", "top_p", "min_p"):
        v, u, base = getattr(args, name + "_voiced"), getattr(args, name + "_unvoiced"), getattr(args, name)
        if v is None and u is None:
            plain[name] = base
        else:
            voiced[name] = base if v is None else v
            unvoiced[name] = base if u is None else u
    return plain, voiced, unvoiced


def run_decode(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = _decode_args().parse_args(argv)
    rc = launch_ranks(args.n_gpus, "qpnet_amd.run_decode", argv)
    if rc is not None:
        return rc
    _setup_logging(args.verbose)
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if os.environ.get("QPN_BENCH_ONE_GPU") else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)            # replicas only: no process group, no collective
    dev = torch.device("cuda", local)
    outdir = os.path.dirname(args.outdir)
    if outdir:
        os.makedirs(outdir, exist_ok=True)
    _fix_seed(args.seed)
    conf = loaders.load_model_conf(args.config)
    ext = "." + conf.feature_format
    feat_list = loaders.find_files(args.feats, "*" + ext) if os.path.isdir(args.feats) else loaders.read_txt(args.feats)
    mine = np.array_split(np.array(feat_list, dtype=object), world)[rank].tolist()      # qpnet_decode.py:258-259
    scaler = loaders.read_scaler_stats(args.stats, conf.feature_type)
    with torch.no_grad():
        model = _build_model(conf, dev).eval()
        loaders.load_checkpoint(args.checkpoint, model, None, use_ema=args.ema)
        feats = [loaders.read_features(f, conf.feature_type) for f in mine]
        ids = [os.path.basename(f).replace(ext, "") for f in mine]
        from .qpnet import encode_mu_law
        gen = loaders.decode_generator(feats, args.fs, ids, wav_transform=lambda x: encode_mu_law(x, conf.n_quantize),
                                       feat_transform=scaler, dense_factor=conf.dense_factor, batch_size=args.batch_size,
                                       upsampling_factor=conf.upsampling_factor, f0_factor=args.f0_factor,
                                       f0_dim_index=args.f0_dim_index, extra_memory=args.extra_memory, device=dev)
        per_file = args.per_file_seed and args.mode == "sampling"      # (argmax draws nothing)
        if per_file:
            logging.info("per-file seeds on: every file draws from its own stream (seed %d and its id), whatever its batch." % args.seed)
        plain, voiced, unvoiced = uv_decode_controls(args)
        if voiced:
            logging.info("voiced / unvoiced sampling on: %s in voiced frames, %s in unvoiced ones." % (voiced, unvoiced))
        for feat_ids, bx, bh, ns, bd in gen:
            logging.info("decoding start!")
            row_seeds = [loaders.row_seed(args.seed, i) for i in feat_ids] if per_file else None      # (input order: feat_ids lists the batch rows)
            track = loaders.uv_draw_track(bh, voiced, unvoiced) if voiced else None
            outs = model.batch_fast_generate(bx, bh, ns, bd, intervals=args.intervals, mode=args.mode, extra_memory=args.extra_memory, row_seeds=row_seeds, draw_track=track, **plain)
            for feat_id, samples in zip(feat_ids, outs):
                name = args.outdir.replace("feat_id", feat_id)
                loaders.write_wav(name, args.fs, samples, conf.n_quantize)
                logging.info("wrote %s." % name)
    return 0
