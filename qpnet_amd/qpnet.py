"""Host-side mirror of the reference module ``src/nets/qpnet.py`` (bigpon/QPNet).

Same public names, constructor kwargs, attributes, state_dict keys/shapes and call
signatures, but NO torch compute op on the hot path: ``forward`` and
``batch_fast_generate`` hand raw device pointers to the hand-written HIP kernels of
``libqpnet_hip.so`` through the C ABI in ``include/qpnet_hip.h``.  torch is used for device
memory, streams and autograd plumbing only.  There is no CPU fallback: calling the hot path
without the built library or without a GPU raises.

    encode_mu_law / decode_mu_law   <- reference qpnet.py:22-45   (host numpy, as in the reference)
    initialize                      <- reference qpnet.py:47-58
    QPNet                           <- reference qpnet.py:160-686
"""
import logging
import sys
import time

import numpy as np
import torch
from torch import nn

from .config import QPNetConfig
from . import _lib


def encode_mu_law(x, mu=256):
    """mu-law companding to integer classes 0..mu-1 (reference qpnet.py:22-32)."""
    mu = mu - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    return np.floor((fx + 1) / 2 * mu + 0.5).astype(np.int64)


def decode_mu_law(y, mu=256):
    """inverse of encode_mu_law (reference qpnet.py:34-45)."""
    mu = mu - 1
    fx = (y - 0.5) / mu * 2 - 1
    return np.sign(fx) / mu * ((1 + mu) ** np.abs(fx) - 1)


def initialize(m):
    """Xavier-uniform conv weights, zero bias; upsampling kernel 1 / bias 0 (reference qpnet.py:47-58).
    Works with ``model.apply(initialize)`` because parameters are held by stock nn.Conv1d /
    nn.ConvTranspose2d containers (holders only - their forward is never called)."""
    if isinstance(m, nn.Conv1d):
        nn.init.xavier_uniform_(m.weight)
        nn.init.constant_(m.bias, 0.0)
    if isinstance(m, nn.ConvTranspose2d):
        nn.init.constant_(m.weight, 1.0)
        nn.init.constant_(m.bias, 0.0)


class _TapConv(nn.Module):
    """parameter holder: ``.conv`` = 2-tap (dilated) causal conv weights (C_out, C_in, 2)."""

    def __init__(self, cin, cout, ksize, dilation=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, ksize, padding=0, dilation=dilation)


class _PitchTapPair(nn.Module):
    """parameter holder: ``.convC`` (current sample) and ``.convP`` (pitch-dependent past sample)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.convC = nn.Conv1d(cin, cout, 1)
        self.convP = nn.Conv1d(cin, cout, 1)


class _FrameUpsampler(nn.Module):
    """parameter holder: ``.conv`` = (1,1,1,U) transposed-conv kernel + scalar bias."""

    def __init__(self, factor):
        super().__init__()
        self.conv = nn.ConvTranspose2d(1, 1, kernel_size=(1, factor), stride=(1, factor))


def live_pieces(delivered, done):
    """The step between two polls of a live decode: `delivered[b]` samples of row b have been handed on, `done[b]` are
    reported final.  -> [(row, start, stop), ...] for the rows with something new, in row order, and `delivered` is advanced
    in place.  A report below what has been delivered (a re-run starts its counts at zero) brings nothing and takes nothing
    back: the row's next piece starts where the last one ended, once the report has caught up."""
    pieces = []
    for b, d in enumerate(done):
        d = int(d)
        if d > delivered[b]:
            pieces.append((b, delivered[b], d))
            delivered[b] = d
    return pieces


class QPNet(nn.Module):
    """Quasi-Periodic WaveNet vocoder; drop-in for the reference class (qpnet.py:160)."""

    def __init__(self, n_quantize=256, n_aux=39, n_resch=512, n_skipch=256,
                 dilationF_depth=4, dilationF_repeat=3, dilationA_depth=4, dilationA_repeat=1,
                 kernel_size=2, upsampling_factor=110):
        super().__init__()
        cfg = QPNetConfig(n_quantize, n_aux, n_resch, n_skipch, dilationF_depth, dilationF_repeat,
                          dilationA_depth, dilationA_repeat, kernel_size, upsampling_factor)
        # unsupported geometries fail HERE, not at the first forward / decode (the library validates without a GPU)
        import ctypes as _C
        if _lib.lib().qpn_param_count(_C.byref(_lib.make_config(cfg))) < 0:
            raise ValueError("qpnet_amd.QPNet: " + _lib.lib().qpn_last_error().decode("utf-8", "replace"))
        self.cfg = cfg
        self.n_quantize, self.n_aux, self.n_resch, self.n_skipch = n_quantize, n_aux, n_resch, n_skipch
        self.kernel_size, self.upsampling_factor = kernel_size, upsampling_factor
        self.dilationF_depth, self.dilationF_repeat = dilationF_depth, dilationF_repeat
        self.dilationA_depth, self.dilationA_repeat = dilationA_depth, dilationA_repeat
        self.receptiveCausal_field = cfg.receptiveCausal_field
        self.dilationsF = cfg.dilationsF
        self.receptiveF_field = cfg.receptiveF_field
        self.dilationsA = cfg.dilationsA
        self.receptiveA_field = cfg.receptiveA_field
        self.n_ch = n_resch
        C, S, Q, A = n_resch, n_skipch, n_quantize, n_aux
        # registration order == state_dict order == flat parameter order (config.param_layout)
        self.causal = _TapConv(Q, C, kernel_size)
        if upsampling_factor > 0:
            self.upsampling = _FrameUpsampler(upsampling_factor)
        self.dilF_sigmoid = nn.ModuleList(_TapConv(C, C, kernel_size, d) for d in self.dilationsF)
        self.dilF_tanh = nn.ModuleList(_TapConv(C, C, kernel_size, d) for d in self.dilationsF)
        self.auxF_1x1_sigmoid = nn.ModuleList(nn.Conv1d(A, C, 1) for _ in self.dilationsF)
        self.auxF_1x1_tanh = nn.ModuleList(nn.Conv1d(A, C, 1) for _ in self.dilationsF)
        self.skipF_1x1 = nn.ModuleList(nn.Conv1d(C, S, 1) for _ in self.dilationsF)
        self.resF_1x1 = nn.ModuleList(nn.Conv1d(C, C, 1) for _ in self.dilationsF)
        self.dilA_sigmoid = nn.ModuleList(_PitchTapPair(C, C) for _ in self.dilationsA)
        self.dilA_tanh = nn.ModuleList(_PitchTapPair(C, C) for _ in self.dilationsA)
        self.auxA_1x1_sigmoid = nn.ModuleList(nn.Conv1d(A, C, 1) for _ in self.dilationsA)
        self.auxA_1x1_tanh = nn.ModuleList(nn.Conv1d(A, C, 1) for _ in self.dilationsA)
        self.skipA_1x1 = nn.ModuleList(nn.Conv1d(C, S, 1) for _ in self.dilationsA)
        self.resA_1x1 = nn.ModuleList(nn.Conv1d(C, C, 1) for _ in self.dilationsA)
        self.conv_post_1 = nn.Conv1d(S, S, 1)
        self.conv_post_2 = nn.Conv1d(S, Q, 1)
        assert [k for k, _ in self.named_parameters()] == [k for k, _ in cfg.param_layout()]
        self._handle = None
        self._handle_dev = None
        self._qpn_sync_status = False
        self.status_check = "backward"     # "backward": loss.backward() waits for the forward's device-side check (raised before ANY optimizer steps); "lazy": never waits (train.QPNetFunction.backward)
        self.last_decode_kernel_ms = 0.0
        self.last_decode_plan = ""
        self.sampling_seed = None          # set to an int to pin the sampling-mode random stream
        self._n_generate_calls = 0
        self.last_sampling_seed = None
        self.last_row_seeds = None         # the Philox key of every row (input order) of the last decode call that drew per row (per-row controls or row_seeds=); None after a uniform call
        self.last_decode_counts, self.last_decode_cancelled = None, False   # generate_live: every row's final count (input order) / whether the call stopped short on request
        self._live_first_piece_s, self._live_mirror_pieces = None, 0      # generate_live (diagnostics): enqueue return -> first piece, pieces of the last call that were read from the mirror while the call was in flight

    # ------------------------------------------------------------------ native handle
    def _native(self, device):
        """libqpnet_hip handle bound to `device` (created lazily, one per module)."""
        if device.type != "cuda":
            raise RuntimeError("qpnet_amd.QPNet runs on an AMD GPU only (tensors are on %s); there is no CPU fallback" % device)
        L = _lib.lib()
        if self._handle is None or self._handle_dev != device:
            self._release()
            import ctypes as C
            hp = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(L.qpn_create(C.byref(_lib.make_config(self.cfg)), C.byref(hp)))
            self._handle, self._handle_dev = hp, device
        return L, self._handle

    @property
    def last_train_plan(self):
        """What the latest training forward (and its backward, once run) of this module launched, as text (qpn_train_last_plan); "" before the first one."""
        if self._handle is None:
            return ""
        return _lib.lib().qpn_train_last_plan(self._handle).decode("utf-8", "replace")

    def _replicate_for_data_parallel(self):
        """torch.nn.DataParallel with more than one device (the reference wraps the model so, src/bin/qpnet_train.py:416-423, but forces one GPU:
        runQP.py:84-88) would call this once per replica.  The module's state -- the native handle, its workspace with the forward's activations, the
        flat parameter buffer the parameters are views of -- belongs to ONE device and is not carried by replicate(): refuse instead of training on
        replicas that silently share or lose it.  Multi-GPU here is one process per GPU (python -m qpnet_amd.run_train --n_gpus N: RCCL all-reduce of
        the flat gradient); DataParallel over a single device never replicates and works."""
        raise RuntimeError("qpnet_amd.QPNet cannot be replicated by torch.nn.DataParallel over several devices (its native handle and flat parameter "
                           "buffer are per-device state); use one process per GPU: python -m qpnet_amd.run_train --n_gpus N")

    def check_status(self):
        """Raise what the device-side checks of the training forwards so far have found (a dilated factor outside the layer input --
        the reference's gather assert, qpnet.py:294 -- or a target outside [0, n_quantize)); collected without a stream drain.
        backward(), FlatAdam.step() and the next forward call it too; call it after the last forward of a loop that has none of them."""
        if self._handle is not None:
            with torch.cuda.device(self._handle_dev):
                _lib.check(_lib.lib().qpn_train_status_collect(self._handle))

    def _release(self):
        if self._handle is not None:
            try:
                self.check_status()
            except Exception as e:          # (a destructor must not raise: say it)
                import logging
                logging.warning("qpnet_amd: unreported device-side status at release: %s", e)
            _lib.lib().qpn_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def flat_parameters(self):
        """fp32 parameter vector in state_dict order (the layout qpn_set_weights expects)."""
        return torch.cat([p.detach().reshape(-1) for p in self.parameters()]).float().contiguous()

    def _bind_decode_weights(self, L, hd, dev, stream):
        """qpn_set_weights on the model's flat parameter buffer.  The parameters are views of ONE flat buffer
        (train.ensure_flat: built once, re-built only if .to()/.cuda() replaced the storages), so a decode call costs no
        2-96 MB concatenation; the library's tile re-pack is stream-ordered with no host synchronisation (one gather pass
        over the weights, ~0.1 ms for the 96 MB geometry) and is done on every call -- cheaper than any scheme that has to
        notice writes made through `p.data`, which torch's version counters do not see."""
        from .train import ensure_flat
        flat = ensure_flat(self, dev)
        _lib.check(L.qpn_set_weights(hd, flat.data_ptr(), flat.numel(), stream))
        return flat

    # ------------------------------------------------------------------ training forward
    def forward(self, x, h, dilated_factors, blength):
        """Teacher-forced forward (reference qpnet.py:239-312): x (B,T) long, h (B,n_aux,F),
        dilated_factors (B,T) float, blength (B) -> (B, batch_length, n_quantize) logits.
        Differentiable in the parameters and in `h` (h.requires_grad_(): backward fills h.grad as the reference's autograd does, exact zeros in the
        frames in front of the chunk's receptive field); `dilated_factors` gets no gradient (the pitch tap is a rounding: zero almost everywhere,
        in the reference too).  There is no input-only backward: with every parameter frozen the whole backward still runs."""
        from . import train   # native training path (autograd.Function over the C ABI)
        return train.qpnet_forward(self, x, h, dilated_factors, blength)

    def score(self, x, h, dilated_factors, blength, targets):
        """Teacher-forced scoring: forward(x, h, dilated_factors, blength) without a graph, then one record per sample of the chunk's last `blength`
        targets (targets (B, >= blength) long, its last columns used as the loss uses batch_t) -> train.Score(nll, entropy, argmax, rank), each
        (B, blength).  For audio the model generated itself this is its log likelihood; see train.score_logits for the records."""
        from . import train
        for name, v in (("x", x), ("h", h), ("dilated_factors", dilated_factors), ("targets", targets)):
            if v.device.type != "cuda":
                raise RuntimeError("qpnet_amd.QPNet runs on an AMD GPU only (%s is on %s); there is no CPU fallback" % (name, v.device))
        with torch.no_grad():
            logits = self.forward(x, h, dilated_factors, blength)
            train.join_staged(targets, x.device)
            return train.score_logits(logits, targets)

    # ------------------------------------------------------------------ autoregressive decode
    def batch_fast_generate(self, x, h, n_samples_list, dilated_factors,
                            intervals=None, mode="sampling", extra_memory=False, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, row_seeds=None, draw_track=None):
        """Batch fast generation (reference qpnet.py:314-559).

        x (B,T0) long seed, h (B,n_aux,F) float, n_samples_list list[int] (consumed exactly like
        the reference does), dilated_factors (B,T): numpy float64 when extra_memory is False,
        float tensor otherwise.  Returns the list of int64 ndarrays in completion order
        (ascending length, ties in input order).

        temperature, top_k (keyword-only, not in the reference; mode="sampling" only): the draw is taken from softmax(logits / temperature)
        over the classes whose logit is at least the top_k-th largest (ties with it kept; 0 = every class), inside the decode kernel
        (qpn_decode_sampling).  min_p in [0, 1] then keeps the classes whose probability is at least min_p times the most probable class's
        (0 = off), and top_p in (0, 1] the most probable of those whose mass reaches the fraction top_p of the whole, ties with the last one
        kept (1 = off; qpn_decode_sampling_ex): two cuts that follow the width of the distribution where top_k's count
        is fixed.  The defaults are the reference's draw.  The values hold for this call only.

        Per row (qpn_decode_row_sampling): each of the four accepts a sequence of B values instead of a scalar (B >= 2: a batch of one row takes
        scalars, as it always did, and a sequence there is a ValueError), and row_seeds B integers in [0, 2^64) (any B); both always refer to the
        INPUT rows, whatever order the results come back in.  With row_seeds, row b draws from the stream
        (seed = row_seeds[b], stream 0): its samples depend on its own inputs, values and seed only, not on its place in the batch, the batch
        size or the launch plan.  Without row_seeds but with a per-row control, row b draws from (call seed, stream b), the stream of a uniform
        call.  All scalars and no row_seeds is the uniform call: same kernels, same bytes.  last_row_seeds records the keys that were used.

        At frame rate (qpn_decode_frame_sampling): draw_track is a dict with any of the keys "temperature", "top_k", "top_p", "min_p", each an array or tensor
        of shape (B, F) -- rows in INPUT order, F = h.shape[2] -- or (F,), which every row shares.  Generated sample i of a row is drawn with the values of the
        frame whose features that step reads, f(i) = min(F - 1, (x.shape[1] - 1 + i) // upsampling_factor) (upsampling_factor 0: min(F - 1, x.shape[1] - 1 + i));
        the uniforms are those of the same call without a track.  A key the dict does not hold takes the call's scalar or per-row value of that name; a key given
        both ways is a ValueError.  A track whose rows are constant gives the samples of the per-row call with those constants, bit for bit, and what a track
        holds from frame f on cannot change a sample drawn before the row reaches f.  loaders.uv_draw_track builds a voiced / unvoiced one."""
        a = self._decode_args(x, h, n_samples_list, dilated_factors, mode, extra_memory, temperature, top_k, top_p, min_p, row_seeds, draw_track)
        L, hd, dev, B, ns, max_n, out, stream = a["L"], a["hd"], a["dev"], a["B"], a["ns"], a["max_n"], a["out"], a["stream"]
        t_start = a["t_start"]
        with torch.cuda.device(dev):
            try:
                _lib.check(L.qpn_decode(*a["call"]))
            finally:
                if a["track"]:
                    L.qpn_decode_frame_sampling(hd, 0, 0, None)      # this call's track goes with it: nothing is left over for a caller of the C interface either
            self.last_decode_kernel_ms = float(L.qpn_last_decode_kernel_ms(hd))
            self.last_decode_plan = L.qpn_last_decode_plan(hd).decode("utf-8", "replace")
        out_np = out.cpu().numpy()
        if intervals is not None and intervals > 0 and max_n > 0:
            # progress lines of the reference loop (qpnet.py:519-524).  The whole call is one persistent launch, so they are
            # written once it has returned, with the measured mean time per sample (the estimate the reference prints is
            # the same quantity taken over the last `intervals` samples)
            per = (time.time() - t_start) / max_n
            for i in range(intervals, max_n + 1, intervals):
                logging.info("%d/%d estimated time = %.3f sec (%.3f sec / sample)" % (i, max_n, (max_n - i) * per, per))
        # completion order + in-place consumption of n_samples_list (reference qpnet.py:527-557)
        order = sorted(range(B), key=lambda i: ns[i])
        result = [out_np[i, :ns[i]].copy() for i in order]
        keep = ns[order[-1]]
        del n_samples_list[:]
        n_samples_list.append(keep)
        return result

    def _sampling_controls(self, mode, temperature, top_k, top_p=1.0, min_p=0.0):
        """temperature / top_k / top_p / min_p of a decode call, checked on the host before anything touches the device -> (float, int, float, float).
        top_p and min_p are rounded to float32 first, which is what the library sees: the rounded value is what is checked and returned."""
        try:
            t = float(temperature)
        except (TypeError, ValueError):
            raise ValueError("temperature must be a number, not %r" % (temperature,))
        with np.errstate(all="ignore"):
            ok = np.isfinite(np.float32(t)) and t > 0 and np.isfinite(np.float32(1.0) / np.float32(t))
        if not ok:
            raise ValueError("temperature must be a finite float32 > 0 whose reciprocal is finite, not %r" % (temperature,))
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 0 <= int(top_k) <= self.n_quantize:
            raise ValueError("top_k must be an int in 0..n_quantize = %d (0: off), not %r" % (self.n_quantize, top_k))
        cuts = []
        for name, v, lo_open in (("top_p", top_p, True), ("min_p", min_p, False)):
            try:
                with np.errstate(all="ignore"):
                    f = float(np.float32(float(v)))
            except (TypeError, ValueError):
                raise ValueError("%s must be a number, not %r" % (name, v))
            if not ((0.0 < f if lo_open else 0.0 <= f) and f <= 1.0):      # (NaN fails both)
                raise ValueError("%s must be a float32 in %s0, 1] (%s: off), not %r" % (name, "(" if lo_open else "[", "1" if lo_open else "0", v))
            cuts.append(f)
        if mode == "argmax" and (t != 1.0 or int(top_k) != 0 or cuts != [1.0, 0.0]):
            raise ValueError("temperature / top_k / top_p / min_p shape the draw of mode='sampling'; mode='argmax' takes none of them")
        return t, int(top_k), cuts[0], cuts[1]

    def _row_controls(self, mode, B, temperature, top_k, top_p, min_p, row_seeds):
        """The draw of a decode call, checked on the host before anything touches the device -> (the four uniform values, None) for a uniform call (all
        scalars, no row_seeds), or ((1.0, 0, 1.0, 0.0), [(seed or None, temperature, top_k, top_p, min_p)] * B in input order) for a per-row call."""
        vals = tuple(v.tolist() if isinstance(v, torch.Tensor) and v.dim() >= 1 else v for v in (temperature, top_k, top_p, min_p))      # (a 1-D tensor is a sequence like any other)
        if isinstance(row_seeds, torch.Tensor):
            row_seeds = row_seeds.tolist()
        seq = [isinstance(v, (list, tuple, np.ndarray)) and np.ndim(v) >= 1 for v in vals]
        if not any(seq) and row_seeds is None:
            return self._sampling_controls(mode, temperature, top_k, top_p, min_p), None
        if mode == "argmax":
            raise ValueError("per-row temperature / top_k / top_p / min_p and row_seeds shape the draw of mode='sampling'; mode='argmax' takes none of them")
        cols = []
        for name, v, is_seq in zip(("temperature", "top_k", "top_p", "min_p"), vals, seq):
            if is_seq:
                if B < 2:       # a batch of one row has no rows to tell apart: its controls stay the scalars they always were, and a list there stays the error it was
                    raise ValueError("%s must be a number for a batch of one row (a sequence gives one value per row of a batch of two or more), not %r" % (name, v))
                v = v.tolist() if isinstance(v, np.ndarray) and v.ndim == 1 else list(v)
                if len(v) != B:
                    raise ValueError("%s has %d values for a batch of %d rows (one per input row, or a scalar)" % (name, len(v), B))
                if name == "top_k" and any(isinstance(k, float) for k in v):
                    raise ValueError("top_k must hold ints, not %r" % (v,))
            cols.append(v if is_seq else [v] * B)
        if row_seeds is not None:
            seeds = row_seeds.tolist() if isinstance(row_seeds, np.ndarray) else list(row_seeds)
            if len(seeds) != B:
                raise ValueError("row_seeds has %d values for a batch of %d rows (one per input row)" % (len(seeds), B))
            for b, sd in enumerate(seeds):
                if isinstance(sd, bool) or not isinstance(sd, (int, np.integer)) or not 0 <= int(sd) < (1 << 64):
                    raise ValueError("row %d: row_seeds must hold ints in [0, 2^64), not %r" % (b, sd))
            seeds = [int(sd) for sd in seeds]
        else:
            seeds = [None] * B
        rows = []
        for b in range(B):
            try:
                rows.append((seeds[b],) + self._sampling_controls(mode, cols[0][b], cols[1][b], cols[2][b], cols[3][b]))
            except ValueError as e:
                raise ValueError("row %d: %s" % (b, e)) from None
        return (1.0, 0, 1.0, 0.0), rows

    _TRACK_KEYS = ("temperature", "top_k", "top_p", "min_p")
    _TRACK_DEFAULTS = {"temperature": 1.0, "top_k": 0, "top_p": 1.0, "min_p": 0.0}

    def _track_controls(self, mode, B, F, draw_track, temperature, top_k, top_p, min_p):
        """draw_track of a decode call, checked on the host before anything touches the device -> None (no track), or {key: (B, F) ndarray, float32 or int32}
        holding the keys the dict gave.  The four arguments are the call's own values of those names: a key given both ways is refused."""
        if draw_track is None:
            return None
        if not isinstance(draw_track, dict):
            raise ValueError("draw_track must be a dict with any of the keys %s, not %r" % (", ".join(self._TRACK_KEYS), type(draw_track).__name__))
        unknown = [k for k in draw_track if k not in self._TRACK_KEYS]
        if unknown:
            raise ValueError("draw_track has no key %r (its keys: %s)" % (unknown[0], ", ".join(self._TRACK_KEYS)))
        if mode == "argmax":
            raise ValueError("temperature / top_k / top_p / min_p shape the draw of mode='sampling'; mode='argmax' takes none of them")
        out = {}
        for name, arg in zip(self._TRACK_KEYS, (temperature, top_k, top_p, min_p)):
            if name not in draw_track:
                continue
            if not (isinstance(arg, (int, float, np.integer, np.floating)) and arg == self._TRACK_DEFAULTS[name]):
                raise ValueError("%s is given twice: in draw_track and as the argument %s=%r (one of them only)" % (name, name, arg))
            src = draw_track[name]
            src = src.detach().cpu().numpy() if isinstance(src, torch.Tensor) else np.asarray(src)
            if src.dtype.kind not in "iuf":
                raise ValueError("draw_track[%r] must hold numbers, not dtype %s" % (name, src.dtype))
            if src.shape == (F,):
                v = np.broadcast_to(src, (B, F))
            elif src.shape == (B, F):
                v = src
            else:
                raise ValueError("draw_track[%r] has shape %r: expected (B, F) = (%d, %d), or (F,) = (%d,) for every row (F: the frames of h)" % (name, tuple(src.shape), B, F, F))
            with np.errstate(all="ignore"):
                if name == "top_k":
                    if v.dtype.kind == "f":
                        raise ValueError("draw_track['top_k'] must hold ints, not dtype %s" % v.dtype)
                    bad = (v < 0) | (v > self.n_quantize)
                    rule = "must be an int in 0..n_quantize = %d (0: off)" % self.n_quantize
                    v = np.where(bad, 0, v).astype(np.int32)
                else:
                    v = v.astype(np.float32)      # (what the library sees: the rounded value is what is checked)
                    if name == "temperature":
                        bad = ~(np.isfinite(v) & (v > 0) & np.isfinite(np.float32(1.0) / v))
                        rule = "must be a finite float32 > 0 whose reciprocal is finite"
                    elif name == "top_p":
                        bad = ~((v > 0) & (v <= 1))
                        rule = "must be a float32 in (0, 1] (1: off)"
                    else:
                        bad = ~((v >= 0) & (v <= 1))
                        rule = "must be a float32 in [0, 1] (0: off)"
            if bad.any():
                b, fr = (int(i) for i in np.argwhere(bad)[0])
                raise ValueError("draw_track[%r] row %d frame %d: %s, not %r" % (name, b, fr, rule, src[fr] if src.ndim == 1 else src[b, fr]))
            out[name] = np.ascontiguousarray(v)
        return out

    def _decode_args(self, x, h, n_samples_list, dilated_factors, mode, extra_memory, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, row_seeds=None, draw_track=None):
        """What batch_fast_generate and generate_live do before the library call: mode check, maxd, dtype and device moves, the
        output buffer, the sampling seed, binding the weights.  -> dict; "call" is the argument tuple of qpn_decode / qpn_decode_enqueue, the rest
        keeps the tensors behind its pointers alive."""
        if mode not in ("sampling", "argmax"):
            logging.error("mode should be sampling or argmax")
            sys.exit(1)
        B = len(n_samples_list)
        track = self._track_controls(mode, B, int(h.shape[2]), draw_track, temperature, top_k, top_p, min_p)
        (temperature, top_k, top_p, min_p), rows = self._row_controls(mode, B, temperature, top_k, top_p, min_p, row_seeds)
        import ctypes as C
        dev = x.device
        L, hd = self._native(dev)
        _lib.check(L.qpn_decode_sampling_ex(hd, temperature, top_k, top_p, min_p))      # this call's values, set before every enqueue: nothing is left over from the last call
        assert x.shape[0] == B and h.shape[0] == B
        # maxd exactly as the reference computes it (qpnet.py:347-350)
        if extra_memory:
            maxd = int(torch.max(dilated_factors.ceil()))
            d_dev = dilated_factors.to(dev, torch.float32).contiguous()
            d_is_f32 = 1
        else:
            dnp = np.asarray(dilated_factors)
            maxd = int(np.nanmax(np.ceil(dnp)))
            d_dev = torch.from_numpy(np.ascontiguousarray(dnp, dtype=np.float64)).to(dev)
            d_is_f32 = 0
        assert d_dev.dim() == 2 and d_dev.shape[0] == B
        xd = x.to(dev, torch.int64).contiguous()
        hd_ = h.to(dev, torch.float32).contiguous()
        assert hd_.shape[1] == self.n_aux
        ns = [int(n) for n in n_samples_list]
        max_n = max(ns)
        out = torch.empty((B, max(max_n, 1)), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        # sampling: a counter-based generator keyed by torch's seed (torch.manual_seed(args.seed) in the reference
        # decode script, qpnet_decode.py:236-239) plus a per-call counter; draws are reproducible, but they are not
        # torch.distributions.Categorical's stream (parity with the reference is statistical in this mode)
        seed = self.sampling_seed if self.sampling_seed is not None else (torch.initial_seed() + self._n_generate_calls) % (1 << 64)
        self._n_generate_calls += 1
        self.last_sampling_seed = seed
        # ... and this call's per-row records, set or cleared before every enqueue for the same reason.  A row without a seed of its own draws from
        # (call seed, stream = its input row): the stream of the uniform call
        if rows is None:
            _lib.check(L.qpn_decode_row_sampling(hd, 0, None))
            self.last_row_seeds = None
        else:
            rec = (_lib.QpnRowDraw * B)(*[_lib.QpnRowDraw(seed if sd is None else sd, b if sd is None else 0, t, k, tp, mp) for b, (sd, t, k, tp, mp) in enumerate(rows)])
            _lib.check(L.qpn_decode_row_sampling(hd, B, rec))
            self.last_row_seeds = [seed if sd is None else sd for sd, _, _, _, _ in rows]
        # ... and this call's draw track, likewise.  A key the dict does not hold is filled with the call's own value of that name: the row's, or the scalar
        rec_t = None
        if track is None:
            _lib.check(L.qpn_decode_frame_sampling(hd, 0, 0, None))
        else:
            F = int(h.shape[2])
            rec_t = np.empty((B, F), dtype=np.dtype([("temperature", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("min_p", "<f4")]))
            for j, (name, scalar) in enumerate(zip(self._TRACK_KEYS, (temperature, top_k, top_p, min_p))):
                if name in track:
                    rec_t[name] = track[name]
                elif rows is not None:
                    rec_t[name] = np.asarray([r[1 + j] for r in rows])[:, None]
                else:
                    rec_t[name] = scalar
            _lib.check(L.qpn_decode_frame_sampling(hd, B, F, rec_t.ctypes.data_as(C.POINTER(_lib.QpnFrameDraw))))
        t_start = time.time()           # (the clock of batch_fast_generate's progress lines starts here, in front of the weight binding)
        arr = (C.c_int64 * B)(*ns)
        call = (hd, B, xd.shape[1], hd_.shape[2], d_dev.shape[1], xd.data_ptr(), hd_.data_ptr(), d_dev.data_ptr(), d_is_f32,
                arr, maxd, 1 if mode == "sampling" else 0, seed, None, out.data_ptr(), None, stream)
        with torch.cuda.device(dev):
            flat = self._bind_decode_weights(L, hd, dev, stream)
        return dict(L=L, hd=hd, dev=dev, B=B, ns=ns, max_n=max_n, out=out, stream=stream, call=call, t_start=t_start, track=track is not None, keep=(xd, hd_, d_dev, arr, flat, rec_t))

    # ------------------------------------------------------------------ live decode output
    def generate_live(self, x, h, n_samples_list, dilated_factors, intervals=None, mode="sampling",
                      extra_memory=False, every=256, poll_s=0.001, on_close="finish", *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, row_seeds=None, draw_track=None):
        """batch_fast_generate as a generator that hands samples over while the decode kernel runs: yields (row, start, samples)
        -- row = index in the input order, samples = a fresh int64 ndarray holding that row's samples [start, start + len) --
        as soon as a poll of the library (qpn_decode_poll) shows new finished samples of a row.  A row's pieces are contiguous
        and in order; concatenated they are what batch_fast_generate returns for that row.  The kernel publishes a row's
        progress every `every` samples and at its end.  After the last piece the call is finished and raises what
        batch_fast_generate raises (a QpnError for a dilated factor outside the rings, ...).  Same arguments and seed rule as
        batch_fast_generate, except that n_samples_list is not consumed.  Polling happens in the caller's thread (no background
        thread), with time.sleep(poll_s) between polls that brought nothing; with `intervals` the reference's progress line
        (qpnet.py:519-524) is written as the longest row passes each multiple.  Closing or dropping the generator early finishes
        the call and leaves the model usable: with on_close="finish" (the default) the kernel runs to its end first; with
        on_close="cancel" the call is asked to stop (qpn_decode_cancel) and returns after about one or two publish intervals
        (`every` samples of the longest-running row each) plus the drain of the launch.  A generator that is iterated to its end
        never cancels.  After the generator has ended, either way, last_decode_counts holds every row's final count in input
        order (samples below it are valid; n_samples for a call that ran to its end) and last_decode_cancelled whether the call
        stopped short on request.  temperature / top_k / top_p / min_p / row_seeds / draw_track: as in batch_fast_generate, per-row sequences included."""
        if on_close not in ("finish", "cancel"):
            raise ValueError("on_close must be 'finish' or 'cancel', not %r" % (on_close,))
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        if mode in ("sampling", "argmax"):
            self._track_controls(mode, len(n_samples_list), int(h.shape[2]), draw_track, temperature, top_k, top_p, min_p)
            self._row_controls(mode, len(n_samples_list), temperature, top_k, top_p, min_p, row_seeds)          # (bad values are refused here, at the call, not at the first next())
        self._native(x.device)          # (CPU tensors are refused here, at the call, not at the first next())
        return self._live_pieces(x, h, list(n_samples_list), dilated_factors, intervals, mode, extra_memory, int(every), float(poll_s), on_close == "cancel", temperature, top_k, top_p, min_p, row_seeds, draw_track)

    def _live_pieces(self, x, h, n_samples_list, dilated_factors, intervals, mode, extra_memory, every, poll_s, cancel_on_close, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, row_seeds=None,
                     draw_track=None):
        import ctypes as C
        a = self._decode_args(x, h, n_samples_list, dilated_factors, mode, extra_memory, temperature, top_k, top_p, min_p, row_seeds, draw_track)
        L, hd, dev, B, ns, max_n, out, stream = a["L"], a["hd"], a["dev"], a["B"], a["ns"], a["max_n"], a["out"], a["stream"]
        done = (C.c_int64 * B)()
        mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
        delivered = [0] * B
        longest = max(range(B), key=lambda b: ns[b])
        next_line, t_line = (intervals if intervals is not None and intervals > 0 else 0), time.time()
        in_flight = enqueued = False

        def progress(b, stop):          # the reference's progress line, as the longest row passes each multiple of `intervals`
            nonlocal next_line, t_line
            while next_line and b == longest and next_line <= stop:
                now = time.time()
                per = (now - t_line) / intervals
                logging.info("%d/%d estimated time = %.3f sec (%.3f sec / sample)" % (next_line, max_n, (max_n - next_line) * per, per))
                t_line = now
                next_line += intervals

        try:
            with torch.cuda.device(dev):
                _lib.check(L.qpn_decode_live(hd, every))
                _lib.check(L.qpn_decode_enqueue(*a["call"]))
                in_flight = enqueued = True
                self.last_decode_counts, self.last_decode_cancelled = None, False
                t_enqueued = time.time()
                self._live_first_piece_s, self._live_mirror_pieces = None, 0      # (diagnostics: tools/live_decode.py)
                self.last_decode_plan = L.qpn_last_decode_plan(hd).decode("utf-8", "replace")
            while any(delivered[b] < ns[b] for b in range(B)):
                with torch.cuda.device(dev):
                    _lib.check(L.qpn_decode_poll(hd, done, C.byref(mirror), C.byref(stride), C.byref(running)))
                pieces = live_pieces(delivered, [min(int(done[b]), ns[b]) for b in range(B)])
                if pieces:
                    rows = np.ctypeslib.as_array(mirror, shape=(B, max(int(stride.value), 1)))
                for b, start, stop in pieces:
                    progress(b, stop)
                    if self._live_first_piece_s is None:
                        self._live_first_piece_s = time.time() - t_enqueued
                    self._live_mirror_pieces += 1
                    yield b, start, rows[b, start:stop].astype(np.int64)
                if not pieces:
                    if not running.value:
                        break           # the launch gave up short of the end: finish re-runs it, the rest comes from its output
                    time.sleep(poll_s)
            with torch.cuda.device(dev):
                in_flight = False
                _lib.check(L.qpn_decode_finish(hd, stream))
                self.last_decode_kernel_ms = float(L.qpn_last_decode_kernel_ms(hd))
                self.last_decode_plan = L.qpn_last_decode_plan(hd).decode("utf-8", "replace")
            if any(delivered[b] < ns[b] for b in range(B)):
                out_np = out.cpu().numpy()
                for b, start, stop in live_pieces(delivered, ns):
                    progress(b, stop)
                    yield b, start, out_np[b, start:stop].copy()
        finally:
            with torch.cuda.device(dev):
                if in_flight:
                    if cancel_on_close:
                        L.qpn_decode_cancel(hd)          # every row stops at one of its next publish points; finish then waits for the drain only
                    L.qpn_decode_finish(hd, stream)      # (abandoned, or an error on the way: what it reports has nobody to go to)
                if enqueued:
                    cancelled = C.c_int()
                    if L.qpn_decode_final_counts(hd, done, C.byref(cancelled)) == 0:
                        self.last_decode_counts, self.last_decode_cancelled = [int(done[b]) for b in range(B)], bool(cancelled.value)
                L.qpn_decode_live(hd, 0)
                if a["track"]:
                    L.qpn_decode_frame_sampling(hd, 0, 0, None)      # (the call is finished by now: this call's track goes with it)

    # test/diagnostic helper (not part of the reference surface): teacher-forced streaming logits
    def _stream_logits(self, x, h, dilated_factors, teacher, n_samples):
        import ctypes as C
        dev = x.device
        L, hd = self._native(dev)
        dnp = np.asarray(dilated_factors)
        maxd = int(np.nanmax(np.ceil(dnp)))
        d_dev = torch.from_numpy(np.ascontiguousarray(dnp, dtype=np.float64)).to(dev)
        B = x.shape[0]
        out = torch.empty((B, n_samples), dtype=torch.int64, device=dev)
        logits = torch.empty((B, n_samples, self.n_quantize), dtype=torch.float32, device=dev)
        tch = teacher.to(dev, torch.int64).contiguous()
        xd = x.to(dev, torch.int64).contiguous(); hh = h.to(dev, torch.float32).contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            self._bind_decode_weights(L, hd, dev, stream)
            arr = (C.c_int64 * B)(*([n_samples] * B))
            _lib.check(L.qpn_decode(hd, B, xd.shape[1], hh.shape[2], d_dev.shape[1], xd.data_ptr(), hh.data_ptr(),
                                    d_dev.data_ptr(), 0, arr, maxd, 0, 0, tch.data_ptr(), out.data_ptr(),
                                    logits.data_ptr(), stream))
        return out, logits
