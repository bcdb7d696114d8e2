"""In-memory counterparts of the reference's batch generators and checkpoint helpers.

Same batching / chunking semantics as the reference task scripts, but over arrays instead of .wav/.h5 files
(the file formats of rank 4 are at the end of this module):

  decode_generator  <- src/bin/qpnet_decode.py:122-209  (sort by length, array_split batching, F0 scaling,
                       d = fs/(f0*dense) extended x U, scaler, zero pad_list, n_samples = F*U - 1)
  train_generator   <- src/bin/qpnet_train.py:200-335   (running x/h/d buffers over utterances, receptive field from the
                       buffer's max d, batch_length shrunk to max_length and to a multiple of U, chunks of RF+BL samples
                       that overlap by RF, x[:-1] / x[1:] input-target shift)
  DeviceCorpus / plan_device_batches / device_train_generator: train_generator's stream cut on the GPU out of a corpus that is encoded, scaled and
                       uploaded once (no counterpart in the reference; csrc/corpus.hip)
  save_checkpoint / load_checkpoint <- src/bin/qpnet_train.py:338-353,481-499,557-563 ({"model","optimizer","iterations"})
"""
import hashlib
import logging
import math
import os

import numpy as np
import torch

from . import harness
from .qpnet import encode_mu_law


def row_seed(seed, feat_id):
    """The Philox key of one file under run_decode --per_file_seed: the first eight bytes (little-endian) of SHA-256 of "<seed>:<feat_id>".  It depends
    on the run's seed and the file's id alone -- not on Python's per-process hash(), the batch, the rank or the rest of the list -- so it is the same
    in every process and on every machine."""
    return int.from_bytes(hashlib.sha256(("%d:%s" % (seed, feat_id)).encode("utf-8")).digest()[:8], "little")


def decode_generator(feats, fs, feat_ids=None, wav_transform=None, feat_transform=None, dense_factor=8, batch_size=32,
                     upsampling_factor=80, f0_factor=1.0, f0_dim_index=1, extra_memory=False, device=None):
    """feats: list of (F_i, n_aux) float arrays.  Yields (feat_ids, batch_x, batch_h, n_samples_list, batch_d) exactly as
    the reference generator does (batch_d is a numpy float64 array unless extra_memory)."""
    if feat_ids is None:
        feat_ids = ["utt%04d" % i for i in range(len(feats))]
    idx = np.argsort([f.shape[0] for f in feats])                     # sort with the feature length (:152-155)
    order = [int(i) for i in idx]
    n_batch = math.ceil(len(order) / batch_size)
    for part in np.array_split(np.array(order, dtype=np.int64), n_batch):   # (:157-160)
        bx, bh, bd, ids, ns = [], [], [], [], []
        for i in part.tolist():
            x = np.zeros((1))
            h = np.array(feats[i], copy=True)
            # `if f0_factor is not 1.0` in the reference is an identity test that is true for any parsed float,
            # so F0 is always scaled and d always rebuilt (:172-175)
            h[:, f0_dim_index] = h[:, f0_dim_index] * f0_factor
            d = harness.dilated_factor(harness.batch_f0(h), fs, dense_factor)
            d = harness.extend_time(np.expand_dims(d, -1), upsampling_factor)
            if wav_transform is not None:
                x = wav_transform(x)
            if feat_transform is not None:
                h = feat_transform(h)
            bx.append(x); bh.append(h); bd.append(d); ids.append(feat_ids[i]); ns.append(h.shape[0] * upsampling_factor - 1)
        batch_x = torch.from_numpy(np.stack(bx, axis=0)).long()
        batch_h = torch.from_numpy(harness.pad_list(bh)).float().transpose(1, 2)
        batch_d = harness.pad_list(bd)
        batch_d = torch.from_numpy(batch_d).float().squeeze(-1) if extra_memory else batch_d.squeeze(-1)
        if device is not None:
            batch_x, batch_h = batch_x.to(device), batch_h.to(device)
            if extra_memory:
                batch_d = batch_d.to(device)
        yield ids, batch_x, batch_h, ns, batch_d


class _SampleWindow:
    """The trainer's running window over the concatenated utterance stream, kept as a queue of per-utterance segments
    (samples, frame-rate dilated factors + their suffix maxima, features) and consumed from the front by a frame offset.
    Appending an utterance is O(1): nothing is concatenated until a chunk is actually cut (`front`), and the largest
    dilated factor still in the window -- which sets the receptive field after every append -- comes from the suffix
    maxima instead of a pass over the sample-rate array.  Every utterance holds exactly U samples per frame
    (harness.validate_length), so the window's sample offset is always U times its frame offset."""

    def __init__(self, n_feat, feat_dtype, U):
        import collections
        self.U = int(U)
        self.segs = collections.deque()                 # [x (F*U,) f32 | None, d (F,) f64, sufmax (F,) f64, h (F, D) | None, load, part]
        self.f0 = 0                                     # frames of the first segment already consumed
        self.n_frames = 0                               # live frames / samples in the window
        self.h_dtype = np.result_type(np.float32, feat_dtype)
        self.n_feat = n_feat

    @property
    def n_samples(self):
        return self.n_frames * self.U

    def append(self, x, h, d_frames, sufmax=None, load=None, part=None):
        """One utterance.  x / h may be None with `load` a callable returning the (validated) pair: the PLAN of the stream -- where chunks begin and end,
        which receptive field each has -- needs only the frame count and the dilated factors; samples and features are fetched when a chunk
        that is actually cut (`front`) reaches into the utterance (a data-parallel rank cuts every world-th chunk only).  `part(s0, s1, f0, f1)`, when the
        utterance's source has it, returns just samples [s0, s1) and feature rows [f0, f1): a rank whose chunks are a world-th of the stream then reads a
        world-th of the BYTES, however long the utterances are (its consecutive chunks lie `world` chunks apart: nothing of a whole-utterance load is reused)."""
        d = np.asarray(d_frames, dtype=np.float64)      # float32 buffer + float64 factors promote to float64 upstream too
        if x is not None:
            assert len(x) == len(d) * self.U == h.shape[0] * self.U
        if len(d) == 0:
            return
        if sufmax is None:
            sufmax = np.fmax.accumulate(d[::-1])[::-1]  # (fmax: a NaN factor is ignored, as by the reference's np.nanmax; all-NaN tails stay NaN)
        self.segs.append([None if x is None else np.asarray(x, dtype=np.float32), d, sufmax,
                          None if h is None else h.astype(self.h_dtype, copy=False), load, part])
        self.n_frames += len(d)

    def max_factor(self):
        """largest dilated factor among the live samples (what np.nanmax over the reference's d_buffer returns)."""
        m = np.nan
        for k, seg in enumerate(self.segs):
            m = np.fmax(m, seg[2][self.f0 if k == 0 else 0])
        return float(m)                                 # (NaN only when every live factor is NaN: np.nanmax's answer as well)

    def front(self, frames, samples):
        """first `frames` feature rows and `samples` (= frames*U + 1) samples / sample-rate factors of the window."""
        U = self.U
        xs, ds, hs = [], [], []
        need_s, need_f, off = samples, frames, self.f0
        for seg in self.segs:
            if need_s <= 0:
                break
            d = seg[1]
            take_s = min(need_s, len(d) * U - off * U)
            take_fd = -(-take_s // U)                   # frames whose factors those samples repeat
            take_f = min(need_f, len(d) - off) if need_f > 0 else 0
            if seg[0] is None and seg[5] is not None:   # planned only, and its source can hand out a slice: exactly what this chunk needs of it
                xp, hp = seg[5](off * U, off * U + take_s, off, off + take_f)
                assert len(xp) == take_s and hp.shape[0] == take_f, "an utterance changed between the plan and the load"
                xs.append(np.asarray(xp, dtype=np.float32))
                if take_f > 0:
                    hs.append(hp.astype(self.h_dtype, copy=False))
            else:
                if seg[0] is None:                      # planned only so far: fetch the utterance now (kept until the window has moved past it)
                    x, h = seg[4]()
                    assert len(x) == len(d) * U == h.shape[0] * U, "an utterance changed between the plan and the load"
                    seg[0], seg[3] = np.asarray(x, dtype=np.float32), h.astype(self.h_dtype, copy=False)
                xs.append(seg[0][off * U:off * U + take_s])
                if take_f > 0:
                    hs.append(seg[3][off:off + take_f])
            ds.append(np.repeat(d[off:off + take_fd], U)[:take_s])
            need_f -= take_f
            need_s -= take_s
            off = 0
        cat = lambda parts: parts[0] if len(parts) == 1 else np.concatenate(parts)      # noqa: E731
        return cat(xs), cat(hs), cat(ds)

    def advance(self, frames, samples):
        assert samples == frames * self.U
        self.n_frames -= frames
        self.f0 += frames
        while self.segs and self.f0 >= len(self.segs[0][1]):
            self.f0 -= len(self.segs[0][1])
            self.segs.popleft()


class _UtterancePlan:
    """What the chunk plan needs of every utterance -- frame count after validate_length, per-frame dilated factors and their suffix maxima, the feature
    dtype / width -- computed ONCE per utterance and kept for the later epochs (a few KB each).  Source, cheapest first: the item's own `plan()` hook
    (runners' file-backed loaders: the wav header and the feature file, no waveform), else one full load of the item."""

    def __init__(self, utterances, U, f0_threshold, fs, dense_factor):
        self.utts, self.U, self.f0_threshold, self.fs, self.dense = utterances, int(U), f0_threshold, fs, dense_factor
        self.meta = {}
        self.loads = 0                                  # full loads of an utterance (samples + features) so far: what a sharded rank should need few of
        self.parts = 0                                  # partial loads (the item's `part` hook)

    def load(self, i):
        item = self.utts[i]
        x, h = item() if callable(item) else item
        if callable(item):
            self.loads += 1
        return harness.validate_length(np.array(x, dtype=np.float32), np.asarray(h), self.U)

    def _entry(self, n_wav, h):
        frames = h.shape[0]
        shortfall = frames * self.U - n_wav             # (harness.validate_length on the lengths alone)
        if shortfall > 0:
            frames = max(frames - (shortfall // self.U + 1), 0)
        d = np.asarray(harness.dilated_factor(harness.batch_f0(h[:frames], self.f0_threshold), self.fs, self.dense), dtype=np.float64)
        return (frames, d, np.fmax.accumulate(d[::-1])[::-1] if frames else d, h.shape[1], h.dtype)

    def part_hook(self, i):
        item = self.utts[i]
        hook = getattr(item, "part", None) if callable(item) else None
        if hook is None:
            return None

        def part(s0, s1, f0, f1):
            self.parts += 1
            return hook(s0, s1, f0, f1)
        return part

    def get(self, i):
        """-> (entry, loaded pair or None)"""
        e = self.meta.get(i)
        if e is not None:
            return e, None
        item = self.utts[i]
        hook = getattr(item, "plan", None) if callable(item) else None
        if hook is not None:
            n_wav, h = hook()
            e, pair = self._entry(int(n_wav), np.asarray(h)), None
        else:
            pair = self.load(i)
            e = self._entry(len(pair[0]), pair[1])
        self.meta[i] = e
        return e, pair


def train_generator(utterances, model_receptiveCausal, model_receptiveF, model_receptiveA, fs, wav_transform=None,
                    feat_transform=None, dense_factor=8, batch_length=20000, batch_size=1, max_length=23070,
                    f0_threshold=0, upsampling_factor=80, shuffle=True, device=None, epochs=None, shard=None):
    """Chunked teacher-forcing batches over a stream of utterances (reference generator: src/bin/qpnet_train.py:200-335).

    utterances: list of (x float waveform in [-1,1], h (F, n_aux)) pairs, or zero-argument callables returning such a
    pair (lazy file loading).  Yields (batch_x, batch_h, batch_t, batch_d, batch_b); endless unless `epochs` is given.

    Behaviour kept from the reference (pinned by tests/test_loaders_cpu.py): utterances are concatenated into one stream
    that survives epoch boundaries; after each appended utterance the receptive field is taken from the largest dilated
    factor still in the window, the batch length is cut to fit max_length and a whole number of frames, and chunks of
    RF + BL (+1 sample for the input/target shift) are cut while MORE than `slots_left` chunks' worth of frames and
    samples remain, each advancing the window by BL (so consecutive chunks overlap by RF).

    shard = (rank, world): data-parallel ranks walk the SAME stream (same seed, same chunk boundaries) but only batch
    numbers rank, rank + world, ... are materialised and yielded; for the others the window just advances -- no mu-law
    encoding, scaling or tensor is made for a chunk another rank consumes, and the stream is laid out from per-utterance
    metadata (frames + dilated factors, computed once per utterance -- through the item's `plan()` hook when it has one --
    and cached over the epochs): an utterance's samples and features are loaded only when one of this rank's own chunks
    reaches into it (no counterpart in the reference, whose only multi-GPU path is a dead DataParallel wrapper,
    qpnet_train.py:416-423).  An item with a `part(s0, s1, f0, f1)` hook (runners' file-backed
    loaders) is read in slices: exactly the samples / feature rows a chunk needs.  `train_generator.last_stats` counts the full ("loads") and
    partial ("parts") loads of the most recent generator."""
    U = int(upsampling_factor)
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    n_batches = 0                                       # batches cut so far, over all ranks
    n_files = len(utterances)
    order = np.random.permutation(n_files) if shuffle else np.arange(n_files)
    win = None
    epoch = 0
    # With world > 1 the stream is PLANNED from per-utterance metadata (frames, dilated factors: _UtterancePlan, cached across epochs) and an utterance's
    # samples / features are loaded only when one of THIS rank's chunks reaches into it (every rank used to load, validate and take the
    # factors of every utterance, so a rank's host work per step grew with the world size).  world == 1 touches every utterance anyway: loaded on append.
    plan = _UtterancePlan(utterances, U, f0_threshold, fs, dense_factor) if world > 1 else None
    stats = {"loads": 0, "parts": 0}                    # (train_generator.last_stats: full / partial utterance loads of the most recent generator, for tests / tools)
    train_generator.last_stats = stats
    while epochs is None or epoch < epochs:
        rows = []                                       # (x, h, t, d, bl) of the batch being filled
        slots_left = batch_size
        for i in order:
            if plan is None:
                item = utterances[int(i)]
                x, h = item() if callable(item) else item
                stats["loads"] += 1
                x, h = harness.validate_length(np.array(x, dtype=np.float32), np.asarray(h), U)
                d = harness.dilated_factor(harness.batch_f0(h, f0_threshold), fs, dense_factor)
                if win is None:
                    win = _SampleWindow(h.shape[1], h.dtype, U)
                win.append(x, h, d)
            else:
                (nfr, d, sufmax, n_feat, h_dtype), pair = plan.get(int(i))
                if win is None:
                    win = _SampleWindow(n_feat, h_dtype, U)

                def load(i=int(i)):
                    out = plan.load(i)
                    stats["loads"] = plan.loads
                    return out
                if pair is not None:                    # (the plan had to load it: keep what was loaded)
                    stats["loads"] = plan.loads
                    win.append(pair[0], pair[1], d, sufmax)
                else:
                    win.append(None, None, d, sufmax, load, plan.part_hook(int(i)))
            rf = harness.receptive_field(model_receptiveCausal, model_receptiveF, model_receptiveA, win.max_factor())
            bl, frames, samples = harness.chunk_plan(rf, batch_length, max_length, U)
            hop_frames = bl // U
            while win.n_frames > slots_left * frames and win.n_samples > slots_left * samples:
                mine = n_batches % world == rank
                if mine:
                    xs, hs, ds = win.front(frames, samples)
                    if plan is not None:
                        stats["parts"] = plan.parts
                    if wav_transform is not None:
                        xs = wav_transform(xs)
                    if feat_transform is not None:
                        hs = feat_transform(hs)
                    xs = torch.from_numpy(np.asarray(xs)).long()
                    rows.append((xs[:-1], torch.from_numpy(np.asarray(hs)).float().transpose(0, 1), xs[1:],
                                 torch.from_numpy(np.asarray(ds)).float()[:-1], bl))
                else:
                    rows.append(None)
                slots_left -= 1
                win.advance(hop_frames, hop_frames * U)
                if len(rows) == batch_size:
                    if mine:
                        out = tuple(torch.stack([r[k] for r in rows]) for k in range(4)) + (torch.tensor([r[4] for r in rows]),)
                        if device is not None:
                            out = tuple(o.to(device) for o in out)
                        yield out
                    rows, slots_left = [], batch_size
                    n_batches += 1
        if shuffle:
            order = order[np.random.permutation(n_files)]      # the reference re-shuffles the ALREADY shuffled list (:331-335)
        epoch += 1


# ---------------------------------------------------------------- device-resident corpus (no counterpart in the reference; its generator is qpnet_train.py:200-335)
# one segment of a batch row as qpn_cut_chunks reads it (qpn_corpus_seg, include/qpnet_hip.h): 32 bytes
CORPUS_SEG_DTYPE = np.dtype([("sample0", "<i8"), ("frame0", "<i8"), ("factor0", "<i8"), ("n_samples", "<i4"), ("n_frames", "<i4")])
_UPLOAD_PIECE = 32 << 20                               # bytes of the pinned buffer the corpus goes to the device through


class DeviceCorpus:
    """The whole training corpus, encoded and scaled ONCE, in three device arenas with the utterances back to back:
        samples  int16   (n_samples,)        wav_transform of the waveform (mu-law class indices), cast as train_generator's .long() casts it
        feats    float32 (n_frames, n_aux)   feat_transform of the features, cast as train_generator's .float() casts it
        factors  float32 (n_frames,)         harness.dilated_factor(harness.batch_f0(h, f0_threshold), fs, dense_factor), one per frame
    utterances: the items train_generator takes, (x, h) pairs or zero-argument callables returning one.  Each is loaded once, trimmed by
    harness.validate_length and transformed whole: both transforms are element-wise, so any slice of the arenas is bit for bit what train_generator makes of
    that slice.  Kept on the host: what plan_device_batches needs and no more -- per utterance its frame count, its arena offsets, its float64 factors and
    their suffix maxima (a few KB each); no memory map or file handle outlives the packing of its utterance.  A corpus larger than max_bytes (default: half
    of the device memory free at construction) is a ValueError before anything is allocated on the device; it is raised as soon as the utterances packed so
    far exceed the bound.  With data-parallel ranks every rank holds the whole corpus.  device: a cuda device, or the CPU (plan_device_batches and host
    copies of the arenas for tests; device_train_generator needs the GPU: there is no CPU fallback for the cut)."""

    def __init__(self, utterances, upsampling_factor, fs, dense_factor, f0_threshold=0, wav_transform=None, feat_transform=None, device=None, max_bytes=None):
        U = int(upsampling_factor)
        if U < 1:
            raise ValueError("DeviceCorpus needs upsampling_factor >= 1, got %d (one feature vector per sample has no frame grid to cut chunks on)" % U)
        self.U, self.fs, self.dense_factor, self.f0_threshold = U, fs, dense_factor, f0_threshold
        self.device = torch.device("cpu" if device is None else device)
        if max_bytes is None and self.device.type == "cuda":
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        self.max_bytes = max_bytes
        xs, hs, ds = [], [], []
        self.meta = []                                  # per utterance: (frames, first arena sample, first arena frame, float64 factors, their suffix maxima)
        n_samples = n_frames = 0
        self.n_aux = None
        for item in utterances:
            x, h = item() if callable(item) else item
            x, h = harness.validate_length(np.array(x, dtype=np.float32), np.asarray(h), U)
            frames = h.shape[0]
            d = np.asarray(harness.dilated_factor(harness.batch_f0(h, f0_threshold), fs, dense_factor), dtype=np.float64)
            self.meta.append((frames, n_samples, n_frames, d, np.fmax.accumulate(d[::-1])[::-1] if frames else d))
            if frames == 0:
                continue
            xq = wav_transform(x) if wav_transform is not None else x
            xq = torch.from_numpy(np.ascontiguousarray(xq)).long().numpy()
            if xq.min() < 0 or xq.max() > 32767:
                raise ValueError("utterance %d: sample value %d does not fit the int16 arena (class indices in [0, 32767] expected)"
                                 % (len(self.meta) - 1, int(xq.min() if xq.min() < 0 else xq.max())))
            hq = h.astype(np.result_type(np.float32, h.dtype), copy=False)
            if feat_transform is not None:
                hq = feat_transform(hq)
            hq = torch.from_numpy(np.ascontiguousarray(hq)).float().numpy()
            if self.n_aux is None:
                self.n_aux = hq.shape[1]
            elif hq.shape[1] != self.n_aux:
                raise ValueError("utterance %d has %d features per frame, the ones before it %d" % (len(self.meta) - 1, hq.shape[1], self.n_aux))
            xs.append(xq.astype(np.int16)); hs.append(hq); ds.append(d.astype(np.float32))
            n_samples += frames * U
            n_frames += frames
            nbytes = 2 * n_samples + 4 * n_frames * (self.n_aux + 1)
            if max_bytes is not None and nbytes > max_bytes:
                raise ValueError("the corpus needs more than %d bytes on the device (%d after %d of %d utterances), above max_bytes = %d"
                                 % (nbytes, nbytes, len(self.meta), len(utterances), max_bytes))
        if n_frames == 0:
            raise ValueError("the corpus holds no frame")
        self.n_utterances, self.n_frames, self.n_samples = len(self.meta), n_frames, n_samples
        self.nbytes = 2 * n_samples + 4 * n_frames * (self.n_aux + 1)
        self.samples = self._upload(xs, np.int16, (n_samples,))
        self.feats = self._upload(hs, np.float32, (n_frames, self.n_aux))
        self.factors = self._upload(ds, np.float32, (n_frames,))

    def _upload(self, parts, dtype, shape):
        """the concatenation of `parts` as one device tensor; to a GPU it goes in pieces of at most _UPLOAD_PIECE bytes through two pinned buffers"""
        tdtype = {np.int16: torch.int16, np.float32: torch.float32}[dtype]
        out = torch.empty(shape, dtype=tdtype, device=self.device)
        flat = out.view(-1)
        if self.device.type != "cuda":
            pos = 0
            for a in parts:
                flat[pos:pos + a.size] = torch.from_numpy(a.reshape(-1))
                pos += a.size
            parts.clear()
            return out
        per = _UPLOAD_PIECE // np.dtype(dtype).itemsize
        pins = [torch.empty(per, dtype=tdtype).pin_memory() for _ in range(2)]
        events = [None, None]
        pos = fill = k = 0

        def flush():
            nonlocal pos, fill, k
            if fill:
                flat[pos:pos + fill].copy_(pins[k][:fill], non_blocking=True)
                events[k] = torch.cuda.Event()
                events[k].record(torch.cuda.current_stream(self.device))
                pos += fill
                fill, k = 0, 1 - k
                if events[k] is not None:
                    events[k].synchronize()            # the copy that last read the buffer about to be filled is done
        for a in parts:
            a = torch.from_numpy(a.reshape(-1))
            done = 0
            while done < a.numel():
                n = min(per - fill, a.numel() - done)
                pins[k][fill:fill + n] = a[done:done + n]
                fill += n; done += n
                if fill == per:
                    flush()
        flush()
        torch.cuda.current_stream(self.device).synchronize()
        parts.clear()
        return out


def plan_device_batches(corpus, model_receptiveCausal, model_receptiveF, model_receptiveA, batch_length=20000, batch_size=1, max_length=23070,
                        shuffle=True, epochs=None, shard=None):
    """The window walk of train_generator over a DeviceCorpus, as a plan: no sample or feature is touched.  Same np.random.permutation calls in the same order,
    the window survives epoch boundaries, the receptive field is re-evaluated after every append from the suffix maxima, harness.chunk_plan and the same
    `while` condition decide where chunks are cut, and the window advances by bl // U frames.  Yields one tuple per batch of the stream, over all ranks:
        (rows, frames, bl, mine, maxd)
    mine: the batch is this rank's (shard = (rank, world); always True without).  For a foreign batch the window only advances: rows is None and maxd 0.
    rows: per batch row a list of segments (sample0, n_samples, frame0, n_frames, factor0) in ARENA terms (the fields of qpn_corpus_seg), together
    frames * U + 1 samples and `frames` feature rows.  maxd: ceil of the largest float32 factor among the frames the batch covers (what runners._batches
    takes from the chunk's tensor).  The rows of a batch are always cut under one receptive field: the `while` condition asks for more than slots_left chunks'
    worth of frames and a chunk advances the window by less than its length, so a batch that is begun is completed before the next utterance is appended."""
    import collections
    U = corpus.U
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    n_files = len(corpus.meta)
    order = np.random.permutation(n_files) if shuffle else np.arange(n_files)
    win = collections.deque()                           # utterances with live frames, oldest first
    first, live = 0, 0                                  # frames of win[0] already consumed; live frames in the window
    n_batches = epoch = 0

    def front(frames):
        segs, need_s, need_f, off, dmax = [], frames * U + 1, frames, first, 0.0
        for i in win:
            if need_s <= 0:
                break
            nfr, s0, f0, d = corpus.meta[i][:4]
            take_s = min(need_s, (nfr - off) * U)
            take_f = min(need_f, nfr - off) if need_f > 0 else 0
            segs.append((s0 + off * U, take_s, f0 + off, take_f, f0 + off))
            if take_f > 0:
                dmax = max(dmax, float(d[off:off + take_f].max()))
            need_s -= take_s; need_f -= take_f; off = 0
        assert need_s == 0 and need_f == 0
        return segs, dmax
    while epochs is None or epoch < epochs:
        rows, dmaxs = [], []
        slots_left = batch_size
        for i in order:
            i = int(i)
            if corpus.meta[i][0] > 0:
                win.append(i)
                live += corpus.meta[i][0]
            m = np.nan                                  # (fmax: as _SampleWindow.max_factor)
            for k, j in enumerate(win):
                m = np.fmax(m, corpus.meta[j][4][first if k == 0 else 0])
            rf = harness.receptive_field(model_receptiveCausal, model_receptiveF, model_receptiveA, float(m))
            bl, frames, samples = harness.chunk_plan(rf, batch_length, max_length, U)
            hop_frames = bl // U
            while live > slots_left * frames and live * U > slots_left * samples:
                mine = n_batches % world == rank
                if mine:
                    segs, dmax = front(frames)
                    rows.append(segs); dmaxs.append(dmax)
                slots_left -= 1
                live -= hop_frames
                first += hop_frames
                while win and first >= corpus.meta[win[0]][0]:
                    first -= corpus.meta[win.popleft()][0]
                if slots_left == 0:
                    if mine:
                        yield rows, frames, bl, True, int(np.ceil(float(np.float32(max(dmaxs)))))
                    else:
                        yield None, frames, bl, False, 0
                    rows, dmaxs, slots_left = [], [], batch_size
                    n_batches += 1
        if shuffle:
            order = order[np.random.permutation(n_files)]
        epoch += 1


def corpus_segment_table(rows, frames, U):
    """The rows of one batch (lists of (sample0, n_samples, frame0, n_frames, factor0), as plan_device_batches yields them) -> (records, row_first): the
    CORPUS_SEG_DTYPE array and the int32 index qpn_cut_chunks takes.  Rows of unequal length -- any row that does not hold frames * U + 1 samples and `frames`
    feature rows, where train_generator would fail in torch.stack -- raise ValueError, before anything is launched."""
    T = int(frames) * int(U)
    for b, r in enumerate(rows):
        ns, nf = sum(s[1] for s in r), sum(s[3] for s in r)
        if ns != T + 1 or nf != frames:
            raise ValueError("the rows of a batch must have equal length: row %d holds %d samples and %d feature rows, %d and %d expected" % (b, ns, nf, T + 1, frames))
    recs = np.array([(s0, f0, fd0, ns, nf) for r in rows for (s0, ns, f0, nf, fd0) in r], dtype=CORPUS_SEG_DTYPE)
    return recs, np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)


def device_train_generator(corpus, model_receptiveCausal, model_receptiveF, model_receptiveA, batch_length=20000, batch_size=1, max_length=23070,
                           shuffle=True, epochs=None, shard=None, unvoiced_weight=None):
    """train_generator's stream (same seed, same chunks, same order) cut on the GPU out of a DeviceCorpus: per batch the host sends the segment table (a few
    dozen bytes) and qpn_cut_chunks writes the tensors.  Yields (batch_x, batch_h, batch_t, batch_d, batch_b, maxd[, batch_w]) for this rank's batches:
    batch_b is the CPU tensor train_generator yields, maxd what runners._batches adds, batch_w (with unvoiced_weight) unvoiced_row_weights; the others are
    views of ONE device buffer, bit for bit train_generator's tensors moved to the device.  The work is enqueued on a stream of the generator's own (it runs
    on the prefetch thread): the table goes through a small ring of pinned buffers (an event per slot, as runners.PinnedStager), the launch follows it on that
    stream, and the outputs carry `_qpn_staged` = (event, buffer): the consumer joins them through train.join_staged like any staged copy."""
    import ctypes as C
    from . import _lib
    if corpus.device.type != "cuda":
        raise RuntimeError("device_train_generator needs the corpus on an AMD GPU: there is no CPU fallback for the cut")
    if unvoiced_weight is not None and not (float(unvoiced_weight) >= 0.0 and np.isfinite(float(unvoiced_weight))):
        raise ValueError("unvoiced_weight must be finite and >= 0, got %r" % (unvoiced_weight,))
    L = _lib.lib()
    dev, U, n_aux = corpus.device, corpus.U, corpus.n_aux
    stream = torch.cuda.Stream(dev)
    depth = 4
    pins, events, slot = [None] * depth, [None] * depth, 0
    pad = lambda n: (n + 255) // 256 * 256              # noqa: E731
    for rows, frames, bl, mine, maxd in plan_device_batches(corpus, model_receptiveCausal, model_receptiveF, model_receptiveA, batch_length, batch_size,
                                                            max_length, shuffle, epochs, shard):
        if not mine:
            continue
        B, T = len(rows), frames * U
        recs, row_first = corpus_segment_table(rows, frames, U)
        n_segs = len(recs)
        o_first = n_segs * CORPUS_SEG_DTYPE.itemsize    # the table: n_segs records, then row_first[B + 1]
        n_table = o_first + 4 * (B + 1)
        if events[slot] is not None:
            events[slot].synchronize()                  # the copy that last read this slot is done
        pin = pins[slot]
        if pin is None or pin.numel() < n_table:
            pin = pins[slot] = torch.empty(max(2 * n_table, 4096), dtype=torch.uint8).pin_memory()
        host = pin.numpy()
        host[:o_first].view(CORPUS_SEG_DTYPE)[:] = recs
        host[o_first:n_table].view(np.int32)[:] = row_first
        offs, total = {}, 0
        for name, n in (("x", 8 * B * T), ("t", 8 * B * T), ("d", 4 * B * T), ("h", 4 * B * n_aux * frames)) + ((("w", 4 * B * bl),) if unvoiced_weight is not None else ()):
            offs[name] = (total, n)
            total += pad(n)
        with torch.cuda.stream(stream):
            table = pin[:n_table].to(dev, non_blocking=True)
            buf = torch.empty(total, dtype=torch.uint8, device=dev)
            ptr = lambda name: buf.data_ptr() + offs[name][0]      # noqa: E731
            _lib.check(L.qpn_cut_chunks(corpus.samples.data_ptr(), corpus.n_samples, corpus.feats.data_ptr(), corpus.factors.data_ptr(), corpus.n_frames, n_aux,
                                        pin.data_ptr(), pin.data_ptr() + o_first, table.data_ptr(), table.data_ptr() + o_first, n_segs,
                                        B, frames, U, bl, C.c_float(0.0 if unvoiced_weight is None else float(unvoiced_weight)),
                                        ptr("x"), ptr("t"), ptr("h"), ptr("d"), ptr("w") if unvoiced_weight is not None else None, stream.cuda_stream))
            ev = torch.cuda.Event()
            ev.record(stream)
        events[slot] = ev
        slot = (slot + 1) % depth
        view = lambda name, dtype, shape: buf[offs[name][0]:offs[name][0] + offs[name][1]].view(dtype).view(shape)      # noqa: E731
        out = [view("x", torch.int64, (B, T)), view("h", torch.float32, (B, n_aux, frames)), view("t", torch.int64, (B, T)), view("d", torch.float32, (B, T))]
        if unvoiced_weight is not None:
            out.append(view("w", torch.float32, (B, bl)))
        for t in out:
            t.__dict__["_qpn_staged"] = (ev, buf)
        yield tuple(out[:4]) + (torch.tensor([bl] * B), maxd) + tuple(out[4:])


def score_chunks(n_frames, rf, batch_length, max_length, U):
    """The chunk walk of per-file scoring (run_validate --per_utterance) over ONE utterance of n_frames frames (n_frames * U samples after
    harness.validate_length) whose receptive field is rf -> [(frame0, frames, bl, keep)].

    The targets scored are sample positions rf + 1 .. E, E = (n_frames - 1) * U: the first rf samples are context only (as at the head of the training
    stream), and the last frame is not scored (a chunk carries one sample past its inputs).  A chunk starts at the frame-aligned sample a = frame0 * U,
    has T = frames * U inputs and F = frames feature rows, and the library scores its last bl = T - rf targets -- the geometry the training generator
    has always cut (T - bl == rf, T <= max_length).  The walk keeps `prev`, the last position already scored (rf at first): the next chunk starts at the
    frame that holds sample prev - rf and ends at the largest frame boundary `end` <= E with end - prev <= batch_length and end - a <= max_length; of
    its bl rows the LAST keep = end - prev are new, the at most U - 1 rows in front of them were scored by the chunk before (or are context).
    Empty when E <= rf (nothing to score).  ValueError when no chunk can make progress: max_length < rf + 2 U, or batch_length < U."""
    n_frames, rf, batch_length, max_length, U = int(n_frames), int(rf), int(batch_length), int(max_length), int(U)
    if U < 1 or rf < 0:
        raise ValueError("score_chunks: U >= 1 and rf >= 0 expected (got U = %d, rf = %d)" % (U, rf))
    if max_length < rf + 2 * U:
        raise ValueError("score_chunks: max_length = %d is below rf + 2 U = %d: a chunk that starts on a frame could score nothing new" % (max_length, rf + 2 * U))
    if batch_length < U:
        raise ValueError("score_chunks: batch_length = %d is below U = %d: no frame boundary within a chunk's reach" % (batch_length, U))
    E = (n_frames - 1) * U
    out = []
    prev = rf
    while prev < E:
        a = ((prev - rf) // U) * U
        end = (min(E, prev + batch_length, a + max_length) // U) * U
        assert end > prev and end - a >= rf + 1
        out.append((a // U, (end - a) // U, end - a - rf, end - prev))
        prev = end
    return out


def mu_law_transform(n_quantize=256):
    """wav_transform of the reference scripts: encode_mu_law(x, n_quantize)."""
    return lambda x: encode_mu_law(x, n_quantize)


def _ema_entries(optimizer):
    """{"ema": ..., "ema_decay": ...} of an optimizer object that keeps averaged weights (train.FusedTrainer / FlatAdam with ema_decay), else {}."""
    get = getattr(optimizer, "ema_state_dict", None)
    ema = get() if get is not None else None
    return {"ema": ema, "ema_decay": float(optimizer.ema_decay)} if ema else {}


def save_checkpoint(checkpoint_dir, model, optimizer, iterations):
    """reference _save_checkpoint (qpnet_train.py:338-353).  An optimizer that keeps averaged weights adds "ema" (a second state dict, the model's keys) and
    "ema_decay" at the top level; "model", "optimizer" and "iterations" are what they always were (the reference's loader reads ["model"] only)."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    path = os.path.join(checkpoint_dir, "checkpoint-%d.pkl" % iterations)
    ck = {"model": model.state_dict(), "optimizer": optimizer.state_dict() if optimizer is not None else None,
          "iterations": iterations}
    ck.update(_ema_entries(optimizer))
    torch.save(ck, path)
    return path


def save_final(checkpoint_dir, model, optimizer=None):
    """reference final model file: {"model": state_dict} only (qpnet_train.py:557-563); with the trainer given and averaging on, "ema" / "ema_decay" as in
    save_checkpoint."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    path = os.path.join(checkpoint_dir, "checkpoint-final.pkl")
    ck = {"model": model.state_dict()}
    ck.update(_ema_entries(optimizer))
    torch.save(ck, path)
    return path


def load_checkpoint(path, model, optimizer=None, map_location="cpu", use_ema=False):
    """reference --resume (qpnet_train.py:481-499): restores model (+optimizer, iteration count).
    use_ema=True: the model receives the file's averaged weights ("ema") instead of "model" (decoding / validating with the average); a file without them is an error.
    An optimizer that keeps averaged weights gets the file's back (load_ema); from a file without any it seeds them from the loaded weights."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    if use_ema:
        if not ck.get("ema"):
            raise KeyError("%s holds no averaged weights (no 'ema' entry: it was not written by a run with --ema_decay)" % path)
        model.load_state_dict(ck["ema"])
    else:
        model.load_state_dict(ck["model"])
    if optimizer is not None and ck.get("optimizer") is not None:
        optimizer.load_state_dict(ck["optimizer"])
    if optimizer is not None and getattr(optimizer, "ema_decay", 0.0) and hasattr(optimizer, "load_ema"):
        if ck.get("ema"):
            optimizer.load_ema(ck["ema"])
        else:
            logging.warning("%s holds no averaged weights: the average starts from the loaded weights." % path)
            optimizer.load_ema(None)
    return int(ck.get("iterations", 0))


# ---------------------------------------------------------------- on-disk formats
def samples_to_int16(samples, n_quantize=256):
    """mu-law class ids -> int16 PCM exactly as the reference decode script writes it (qpnet_decode.py:316-319):
    decode_mu_law, x 32768, clip to [-32768, 32767], truncate to int16."""
    from .qpnet import decode_mu_law
    wav = decode_mu_law(np.asarray(samples), n_quantize)
    return np.clip(wav * 32768, -32768, 32767).astype(np.int16)


def write_wav(path, fs, samples, n_quantize=256):
    """Write one decoded utterance as 16-bit PCM (scipy.io.wavfile, as the reference does)."""
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    wavfile.write(path, fs, samples_to_int16(samples, n_quantize))
    return path


def read_wav(path):
    """(fs, float32 waveform in [-1, 1)) the way the trainer reads it (qpnet_train.py:250-251: int16 / 32768)."""
    from scipy.io import wavfile
    fs, x = wavfile.read(path)
    return fs, np.array(x, dtype=np.float32) / 32768


def _h5py():
    """h5py, or -- where only the HDF5 C library is installed (this image) -- the same few calls on libhdf5 itself (qpnet_amd/_hdf5.py): either
    way the files are real HDF5, the format the reference's feature extraction writes and its trainers read (utils.py:43-128)."""
    try:
        import h5py
        return h5py
    except ImportError:
        pass
    try:
        from . import _hdf5
        _hdf5._lib()
        return _hdf5
    except ImportError as e:
        raise ImportError("neither h5py nor an HDF5 library (libhdf5, QPN_LIBHDF5=<path>) is available for the reference's .h5 feature files "
                          "(utils.py:43-92); use feature_format 'npy' or pass arrays to decode_generator / train_generator instead") from e


def read_hdf5(hdf5_name, hdf5_path):
    """reference utils.read_hdf5 (utils.py:43-68): dataset values, e.g. read_hdf5(f, "/world")."""
    h5py = _h5py()
    if not os.path.exists(hdf5_name):
        raise FileNotFoundError("There is no such a hdf5 file. (%s)" % hdf5_name)
    with h5py.File(hdf5_name, "r") as f:
        if hdf5_path not in f:
            raise KeyError("There is no such a data in hdf5 file. (%s)" % hdf5_path)
        return f[hdf5_path][()]


def check_hdf5(hdf5_name, hdf5_path):
    """reference utils.check_hdf5 (utils.py:19-40): the file exists and holds that dataset."""
    if not os.path.exists(hdf5_name):
        return False
    with _h5py().File(hdf5_name, "r") as f:
        return hdf5_path in f


def shape_hdf5(hdf5_name, hdf5_path):
    """reference utils.shape_hdf5 (utils.py:71-88): the dataset's shape without reading it (the reference exits where this raises)."""
    if not check_hdf5(hdf5_name, hdf5_path):
        raise KeyError("There is no such a file or dataset. (%s, %s)" % (hdf5_name, hdf5_path))
    with _h5py().File(hdf5_name, "r") as f:
        return tuple(f[hdf5_path].shape)


def write_hdf5(hdf5_name, hdf5_path, write_data, is_overwrite=True):
    """reference utils.write_hdf5 (utils.py:71-116)."""
    h5py = _h5py()
    write_data = np.array(write_data)
    os.makedirs(os.path.dirname(os.path.abspath(hdf5_name)) or ".", exist_ok=True)
    with h5py.File(hdf5_name, "a") as f:
        if hdf5_path in f:
            if not is_overwrite:
                raise KeyError("Dataset in hdf5 file already exists. (%s)" % hdf5_path)
            del f[hdf5_path]
        f.create_dataset(hdf5_path, data=write_data)


def read_features(path, feature_type="world"):
    """(F, n_aux) acoustic features of one utterance: the `/world` dataset of an .h5 file (layout
    [uv, cont_f0, mcep.., codeap..], feature_extract.py:337-343), or a plain .npy array of the same layout."""
    if path.endswith(".npy"):
        return np.load(path)
    return read_hdf5(path, "/%s" % feature_type)


class FeatureScaler:
    """The StandardScaler the task scripts rebuild from the stats file (qpnet_train.py:433-440): transform = (x - mean) / scale."""

    def __init__(self, mean, scale):
        self.mean_ = np.asarray(mean, dtype=np.float64)
        self.scale_ = np.asarray(scale, dtype=np.float64)
        self.n_features_in_ = self.mean_.shape[0]

    def transform(self, x):
        return (np.asarray(x) - self.mean_) / self.scale_

    __call__ = transform


def read_scaler_stats(path, feature_type="world"):
    """`/world/mean`, `/world/scale` of the stats file calc_stats.py writes (:19-37; the uv dimension has mean 0 / scale 1),
    or an .npz with arrays `mean` and `scale`."""
    if path.endswith(".npz"):
        z = np.load(path)
        return FeatureScaler(z["mean"], z["scale"])
    return FeatureScaler(read_hdf5(path, "/%s/mean" % feature_type), read_hdf5(path, "/%s/scale" % feature_type))


def calc_stats(feature_arrays):
    """mean / scale over a list of (F, n_aux) feature arrays the way calc_stats.py does: population statistics of every
    dimension but the first (uv), which keeps mean 0 / scale 1; zero variance -> scale 1 (sklearn's rule)."""
    n, s1, s2 = 0, 0.0, 0.0
    for f in feature_arrays:
        f = np.asarray(f, dtype=np.float64)[:, 1:]
        n += f.shape[0]; s1 = s1 + f.sum(0); s2 = s2 + (f * f).sum(0)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    scale = np.sqrt(var)
    scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
    return FeatureScaler(np.concatenate([[0.0], mean]), np.concatenate([[1.0], scale]))


def save_model_conf(path, args):
    """the trainer pickles its argparse.Namespace as the model config (qpnet_train.py:389)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    torch.save(args, path)
    return path


def load_model_conf(path):
    """model.conf = a pickled argparse.Namespace (read with a bare torch.load at qpnet_decode.py:245; torch >= 2.6 needs
    weights_only=False for it).  Returns the Namespace."""
    return torch.load(path, map_location="cpu", weights_only=False)


_MODEL_KEYS = ("n_quantize", "n_aux", "n_resch", "n_skipch", "dilationF_depth", "dilationF_repeat",
               "dilationA_depth", "dilationA_repeat", "kernel_size", "upsampling_factor")


def model_kwargs(conf):
    """QPNet constructor kwargs out of a model config Namespace (qpnet_decode.py:275-285)."""
    return {k: getattr(conf, k) for k in _MODEL_KEYS}


def read_txt(path):
    """one entry per line (utils.read_txt, utils.py:151-162)."""
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def find_files(directory, pattern="*.wav"):
    import fnmatch
    out = []
    for root, _, names in os.walk(directory, followlinks=True):
        out += [os.path.join(root, n) for n in fnmatch.filter(names, pattern)]
    return sorted(out)


def file_lists(waveforms, feats, feature_format="h5"):
    """(wav_list, feat_list) from a directory pair or a pair of list files (qpnet_train.py:442-455)."""
    if os.path.isdir(waveforms):
        wavs = find_files(waveforms, "*.wav")
        return wavs, [os.path.join(feats, os.path.basename(w).replace(".wav", "." + feature_format)) for w in wavs]
    if os.path.isfile(waveforms):
        wavs, fts = read_txt(waveforms), read_txt(feats)
        assert len(wavs) == len(fts)
        return wavs, fts
    raise FileNotFoundError("--waveforms should be directory or list: %s" % waveforms)


def unvoiced_row_weights(batch_h, batch_length, upsampling_factor, unvoiced_weight):
    """Per-row sample weights of a chunk from its voiced / unvoiced flag: feature column 0 is uv (1 voiced, 0 unvoiced; calc_stats keeps it at mean 0 / scale 1,
    so the scaled feature is still 0 / 1).  batch_h: (B, n_aux, F) features as the training forward takes them -> (B, batch_length) float32, 1 for the rows of voiced
    frames and `unvoiced_weight` for the others.  Rows are aligned as the forward aligns h with its output rows: the chunk's LAST batch_length positions of the
    upsampled features (position p lies in frame p // upsampling_factor), or of the features themselves with upsampling_factor = 0 (one feature vector per sample)."""
    uv = np.asarray(batch_h, dtype=np.float32)[:, 0, :]
    BL, U, F = int(batch_length), int(upsampling_factor), uv.shape[1]
    w = float(unvoiced_weight)
    if not (w >= 0.0 and np.isfinite(w)):
        raise ValueError("unvoiced_weight must be finite and >= 0, got %r" % (unvoiced_weight,))
    n = F * U if U > 0 else F
    if BL < 1 or BL > n:
        raise ValueError("batch_length %d does not fit the %d positions the features cover" % (BL, n))
    pos = np.arange(n - BL, n)
    if U > 0:
        pos //= U
    return np.where(uv[:, pos] > 0.5, np.float32(1.0), np.float32(w)).astype(np.float32)


def uv_draw_track(batch_h, voiced, unvoiced):
    """A voiced / unvoiced draw track for QPNet.batch_fast_generate(draw_track=...) from the features' flag, under the convention of unvoiced_row_weights: feature
    column 0 is uv (1 voiced, 0 unvoiced; calc_stats keeps it at mean 0 / scale 1, so the scaled feature is still 0 / 1), and > 0.5 is voiced.  batch_h: (B, n_aux, F)
    features as the decode call takes them (array or tensor); voiced, unvoiced: dicts with the same keys among "temperature", "top_k", "top_p", "min_p" -> {key: (B, F)
    array} holding voiced[key] in the voiced frames and unvoiced[key] in the others (int32 for top_k, float32 otherwise).  Frames are the features' own: the decode
    kernels look a sample's frame up themselves."""
    if hasattr(batch_h, "detach"):
        batch_h = batch_h.detach().cpu().numpy()
    h = np.asarray(batch_h, dtype=np.float32)
    if h.ndim != 3 or h.shape[1] < 1:
        raise ValueError("batch_h must be (B, n_aux, F) features, got shape %r" % (h.shape,))
    keys = ("temperature", "top_k", "top_p", "min_p")
    if set(voiced) != set(unvoiced) or not set(voiced) <= set(keys):
        raise ValueError("voiced and unvoiced must hold the same keys among %s, got %r and %r" % (", ".join(keys), sorted(voiced), sorted(unvoiced)))
    is_voiced = h[:, 0, :] > 0.5
    return {k: np.where(is_voiced, voiced[k], unvoiced[k]).astype(np.int32 if k == "top_k" else np.float32) for k in keys if k in voiced}
