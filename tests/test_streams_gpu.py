"""GPU: every path of the library on a NON-BLOCKING stream, with inputs that arrive late on that stream.

Every other GPU test hands the library the legacy null stream and synchronises between making an input and the call, so a launch, memset or copy that went
to stream 0, or a missed fork / join of the side stream, could not show.  Here every case runs under `torch.cuda.stream(s)`, s = torch.cuda.Stream (torch
makes it non-blocking: nothing orders it against stream 0), behind a GATE that makes the race deterministic:

    the device buffers the library reads hold a DECOY -- a second valid input of the same shapes and geometry (another seed of the same generator, the
    pitch floor pinned so that ceil(max d) and the receptive field agree, classes in [0, Q), factors within the rings): reading it flags nothing and
    indexes nothing out of range, it only gives another answer;
    on s: torch.cuda._sleep(cycles), the device-to-device copies of the REAL input over the decoy, the library call, clones of what the call left on
    the device; then s.synchronize() and the comparison.

Work that is not ordered behind the copies on s reads the decoy.  `cycles` is calibrated once per module (the tick torch.cuda._sleep counts differs
between builds) to GATE_MS; a call that is documented not to drain its stream must return while the gate is still closed (`not s.query()`), or the case
fails: a gate that has already opened proves nothing.  Set-up (model, native handle and its workspace, trainer buffers, staging copies, one call on the
decoy where the first call of a handle allocates) runs on the default stream and is synchronised before s.wait_stream(default stream).

Teeth: every case asserts, on the CPU oracle alone, that the decoy's result is at least 100 x the comparison bound away from the real one (decode: that
at least 10 % of the samples differ), so a too-early read cannot pass.  No new tolerances: training against oracle/train_oracle.py at the small-chunk
bounds of test_train_edges_gpu._compare and util.assert_weights_after_adam as test_train_edges_gpu._fused uses it, the optimiser options against the numpy
restatements of test_grad_clip_gpu / test_ema_gpu at their bounds, decode bit for bit against oracle/qpnet_oracle.c, the standalone kernels against
tests/sampling_spec.py and tests/golden/kat.npz.  MEASUREMENTS.md, "Stream independence", has the calibrated gate and what two deliberate mutations did."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import PAPER, TINY, QPNetConfig
import sampling_spec as SS
import test_decode_gpu as D
import test_ema_gpu as EM
import test_grad_clip_gpu as GC
import test_train_edges_gpu as E
import util

pytestmark = pytest.mark.gpu

F = np.float32
GATE_MS = 40.0                        # the calibration's aim; the measured gate must lie in [20, 200] ms (~50 x the host time to enqueue a step)
# synth.train_inputs(cfg, 500, seed, 2500, f0_lo=60, pin_f0_floor=True, batch_size=2): seed 61 is test_train_edges_gpu's shared two-row chunk.  The others
# were chosen with the oracle (ceil(max d) = 46 like seed 61's; losses at the shared weights 5.6147 (61), 5.5988 (62), 5.5854 (66), 5.5845 (67) on PAPER:
# every pair used as real / decoy below is more than 100 x 1e-4 apart; 5.5619 (61) and 5.5868 (64) on the generic geometry)
REAL, DECOY, SECOND, THIRD = 61, 66, 62, 67
DECOY_SEED = {"paper": DECOY, "c128": 64}


# ---------------------------------------------------------------- the gate
@pytest.fixture(scope="module")
def gate(cuda):
    """cycles of torch.cuda._sleep for GATE_MS, measured with events on a non-blocking stream (and measured again at the calibrated value)"""
    import torch
    s = torch.cuda.Stream(cuda)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(n):
        with torch.cuda.stream(s):
            e0.record(); torch.cuda._sleep(n); e1.record()
        s.synchronize()
        return e0.elapsed_time(e1)

    timed(1000)                       # (the sleep kernel's code object)
    n = 100000
    while timed(n) < 2.0 and n < 10 ** 11:
        n *= 10
    cycles = int(n * GATE_MS / timed(n))
    ms = timed(cycles)
    print("STREAMS gate: torch.cuda._sleep(%d) lasts %.1f ms (%.0f ticks per microsecond)" % (cycles, ms, cycles / ms / 1e3))
    assert 20.0 <= ms <= 200.0, ms
    return types.SimpleNamespace(cycles=cycles, ms=ms)


class _Late:
    """device buffers that hold the decoy, and synchronised staging tensors with the real input, array by array"""

    def __init__(self, cuda, real, decoy):
        import torch
        assert len(real) == len(decoy)
        for r, d in zip(real, decoy):
            assert r.shape == d.shape and r.dtype == d.dtype and not np.array_equal(r, d)
        self.buf = [torch.from_numpy(np.array(a)).to(cuda) for a in decoy]
        self.stage = [[torch.from_numpy(np.array(a)).to(cuda) for a in real]]

    def more(self, cuda, arrs):
        """another real input for the same buffers (its decoy is whatever the buffers hold by then: the input before it) -> its index"""
        import torch
        self.stage.append([torch.from_numpy(np.array(a)).to(cuda) for a in arrs])
        return len(self.stage) - 1

    def deliver(self, gate, k=0):
        """on the current stream: the gate, then the real input over the decoy"""
        import torch
        torch.cuda._sleep(gate.cycles)
        for b, r in zip(self.buf, self.stage[k]):
            b.copy_(r)


def _start(cuda):
    """end of set-up: everything so far is complete, and a fresh non-blocking stream starts behind it"""
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream(cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    return s


def _still_closed(s, what):
    assert not s.query(), "%s is documented not to drain its stream, yet the gate in front of it had opened when it returned: this run proves nothing" % what


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- training: inputs, oracles, teeth
@functools.lru_cache(maxsize=None)
def _chunk(cfgname, seed):
    """a two-row chunk of `cfgname` with its oracle (computed once, never written)"""
    if seed == E.DSEED[2]:
        return E._oracle(cfgname, 2)
    return E._with_oracle(cfgname, *util.distinct_rows_batch(E.CFGS[cfgname][0], 500, seed, 2500, 2))


def _teeth(o, dec):
    """the decoy is a valid input of the same geometry whose oracle result is >= 100 x the bounds of test_train_edges_gpu._compare away from the real one's"""
    for a, b in ((o.x, dec.x), (o.h, dec.h), (o.t, dec.t), (o.d, dec.d)):
        assert a.shape == b.shape and a.dtype == b.dtype
    assert dec.maxd == o.maxd and dec.BL == o.BL
    Q = o.cfg.n_quantize
    assert 0 <= min(dec.x.min(), dec.t.min()) and max(dec.x.max(), dec.t.max()) < Q and dec.d.min() > 0.5
    scale = float(np.abs(o.og).max())
    far = (float(np.abs(dec.lg - o.lg).max()) / 2e-5, abs(dec.loss - o.loss) / 1e-4, float(np.abs(dec.og - o.og).max()) / ((2e-5 + 1e-4) * scale))
    print("STREAMS teeth: decoy away from the real result by %.0f x (logits) %.0f x (loss) %.0f x (gradient) the bound" % far)
    assert min(far) >= 100.0, far


def _weights_after_adam(o, og, w, lr=1e-4, dec=None):
    """the parameters after the step against the oracle's Adam on the oracle gradient that matched, as test_train_edges_gpu._fused(weights_too=True) does;
    dec: ... and the decoy's update is > 100 x sig_max away on an element that counts"""
    from oracle import train_oracle as TO
    wo = o.flat.copy()
    TO.Adam(wo.size, lr=lr).step(wo, og)
    sig = util.significant_elements(o.cfg, [og])
    if dec is not None:
        wd = o.flat.copy()
        TO.Adam(wd.size, lr=lr).step(wd, dec.og)
        assert np.abs(wd - wo)[sig].max() >= 100 * 1e-6
    util.assert_weights_after_adam(w, wo, lr, 1, far=2.0, significant=sig, sig_max=1e-6)


def _train_late(cuda, o, dec):
    return _Late(cuda, (o.x, o.h, o.t, o.d), (dec.x, dec.h, dec.t, dec.d))


def _prime(tr, late, o, cuda):
    """What belongs to a trainer's set-up, on the default stream: the native handle with its workspace and the kernels' code objects (one validation forward,
    on the decoy), the trainer's buffers, and the applied-update base FusedTrainer.step reads once per trainer (qpn_train_applied_updates drains its stream)."""
    import torch
    from qpnet_amd.train import ensure_flat
    xb, hb, tb, db = late.buf
    tr.forward_loss(xb, hb, tb, db, o.b, maxd=o.maxd)
    L, hd = tr.model._native(cuda)
    tr._buffers(ensure_flat(tr.model, cuda))
    n = C.c_int64(0)
    _lib.check(L.qpn_train_applied_updates(hd, C.byref(n), torch.cuda.current_stream(cuda).cuda_stream))
    tr._applied_base = (tr.step_count, int(n.value))
    return L, hd


def _loss_on(L, hd, s):
    v = C.c_double(0.0)
    _lib.check(L.qpn_train_loss(hd, C.byref(v), s.cuda_stream))
    return v.value


# ---------------------------------------------------------------- 1. the autograd path
ARRANGEMENTS = {"paper": ("paper", {}), "paper,QPN_STACK_QUEUE=0": ("paper", {"QPN_STACK_QUEUE": "0"}), "paper,QPN_TRAIN_GEMM=1": ("paper", {"QPN_TRAIN_GEMM": "1"}),
                "c128": ("c128", {})}


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_autograd_path_on_a_stream_with_late_inputs(arrangement, cuda, gate, monkeypatch):
    """forward, CrossEntropyLoss and loss.backward() inside the stream context: the specialised tiles with both stack queues and the side stream, a launch per
    layer, the LDS-tiled GEMM path, the generic tiles.  The forward must return with the gate closed (its status check is enqueued, not waited for); the
    backward waits for that check by default, i.e. for the gate."""
    import torch
    cfgname, env = ARRANGEMENTS[arrangement]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o, dec = _chunk(cfgname, REAL), _chunk(cfgname, DECOY_SEED[cfgname])
    _teeth(o, dec)
    m = util.build_model(o.cfg, o.flat, cuda).train()
    late = _train_late(cuda, o, dec)
    xb, hb, tb, db = late.buf
    with torch.no_grad():
        m(xb, hb, db, o.b)                                          # set-up: the handle, its workspace (left full of the decoy's activations), the code objects
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        logits = m(xb, hb, db, o.b)
        _still_closed(s, "QPNet.forward")
        loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, o.cfg.n_quantize), tb[:, -o.BL:].reshape(-1))
        loss.backward()
        got = logits.detach().clone(), loss.detach().clone(), torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
    s.synchronize()
    m.check_status()
    E._compare("streams %s autograd" % arrangement, o, _np(got[0]), float(got[1]), _np(got[2]))


# ---------------------------------------------------------------- 2. the fused step
@pytest.mark.parametrize("want_loss", [False, "lagged", True], ids=["none", "lagged", "in-step"])
def test_fused_step_on_a_stream_with_late_inputs(want_loss, cuda, gate):
    """FusedTrainer.step (qpn_train_step) in its three loss modes: the loss, the step's gradient and the weights after it.  Modes 0 and 1 must return with the
    gate closed.  Mode 2 drains the stream in the call; it runs WITHOUT the set-up call, so the handle's first-call initialisation happens on the stream too."""
    import torch
    from qpnet_amd.train import FusedTrainer
    o, dec = _chunk("paper", REAL), _chunk("paper", DECOY)
    _teeth(o, dec)
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4)
    late = _train_late(cuda, o, dec)
    xb, hb, tb, db = late.buf
    if want_loss is not True:
        _prime(tr, late, o, cuda)
    L, hd = m._native(cuda)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        loss = tr.step(xb, hb, tb, db, o.b, want_loss=want_loss, maxd=o.maxd)
        if want_loss is not True:
            _still_closed(s, "qpn_train_step with loss_mode %d" % (1 if want_loss else 0))
        g, w = tr.g.clone(), m._flat.clone()
    s.synchronize()
    if want_loss == "lagged":
        assert loss is None
        loss = tr.flush_loss()
    elif want_loss is False:
        assert loss is None
        loss = _loss_on(L, hd, s)                                   # (the partial sums the step left on the device)
    tr.check_status()
    og = E._compare("streams fused step, want_loss=%r" % (want_loss,), o, None, loss, _np(g)[:o.flat.size])
    _weights_after_adam(o, og, _np(w), dec=dec)


# ---------------------------------------------------------------- 3. clipping and the averaged weights on
def _norm64(g):
    return float(np.sqrt((np.asarray(g, np.float64) ** 2).sum()))


def _check_optimiser(label, o, dec, og, w0, g_dev, den, max_norm, w, mo, vo, norm, ema=None, decay=0.0):
    """The optimiser launch of a step against test_grad_clip_gpu._ref_adam restated from the gradient buffer the step itself left (weights atol 2e-6, m 1e-5 and v
    4e-5 of their largest, as there), the average against test_ema_gpu._ema_ref from the device's own new weights; the norm against the fp64 norm of the same
    buffer (rtol 1e-7; 1e-6 with a denominator) and of the ORACLE gradient (rtol 1e-5: the bound test_grad_clip_gpu holds the norms of two implementations of
    one backward to).  Teeth: the decoy's norm and first moment are > 100 x those bounds away."""
    total = _norm64(g_dev) / (den or 1.0)
    want = _norm64(og)
    print("STREAMS %s: norm %.9g, of the buffer %.9g (rel %.1e), of the oracle gradient %.9g (rel %.1e); max_grad_norm %.4g" %
          (label, norm, total, abs(norm - total) / total, want, abs(norm - want) / want, max_norm))
    np.testing.assert_allclose(norm, total, rtol=1e-6 if den else 1e-7, atol=0)
    np.testing.assert_allclose(norm, want, rtol=1e-5, atol=0)
    coef = GC._coef(total, max_norm)
    assert coef < 0.51                                              # (clipping binds)
    z = np.zeros_like(w0)
    wr, mr, vr = GC._ref_adam(w0, g_dev, z, z, coef, den=den, step=1)
    np.testing.assert_allclose(w, wr, rtol=0, atol=2e-6)
    np.testing.assert_allclose(mo, mr, rtol=0, atol=1e-5 * np.abs(mr).max())
    np.testing.assert_allclose(vo, vr, rtol=0, atol=4e-5 * np.abs(vr).max())
    assert abs(_norm64(dec.og) - want) >= 100 * 1e-5 * want
    md = GC._ref_adam(w0, dec.og, z, z, GC._coef(_norm64(dec.og), max_norm), step=1)[1]
    assert np.abs(md - GC._ref_adam(w0, og, z, z, GC._coef(want, max_norm), step=1)[1]).max() >= 100 * 1e-5 * np.abs(mr).max()
    if ema is not None:
        r, bound = EM._ema_ref(w, w0, decay)
        err = np.abs(ema.astype(np.float64) - r.astype(np.float64))
        assert (err <= bound).all(), (err / bound).max()
        assert (np.abs(ema.astype(np.float64) - w0.astype(np.float64)) > 100 * bound).any()


@pytest.mark.parametrize("want_loss", [False, "lagged", True], ids=["none", "lagged", "in-step"])
def test_clipped_averaged_step_on_a_stream_with_late_inputs(want_loss, cuda, gate):
    """qpn_train_step_avg with max_grad_norm binding (half the oracle gradient's norm) and ema_decay 0.9: loss and gradient against the oracle, the norm, both
    moments, the weights and the average.  Optimiser settings of test_grad_clip_gpu (lr 1e-3, weight_decay 1e-3), whose restatement and bounds are used."""
    import torch
    from qpnet_amd.train import FusedTrainer
    o, dec = _chunk("paper", REAL), _chunk("paper", DECOY)
    _teeth(o, dec)
    max_norm, decay = 0.5 * _norm64(o.og), 0.9
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=GC.LR, weight_decay=GC.WD, max_grad_norm=max_norm, ema_decay=decay)
    late = _train_late(cuda, o, dec)
    xb, hb, tb, db = late.buf
    L, hd = _prime(tr, late, o, cuda)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        loss = tr.step(xb, hb, tb, db, o.b, want_loss=want_loss, maxd=o.maxd)
        if want_loss is not True:
            _still_closed(s, "qpn_train_step_avg with loss_mode %d" % (1 if want_loss else 0))
        g, w, mo, vo, ema = tr.g.clone(), m._flat.clone(), tr.m.clone(), tr.v.clone(), tr.ema.clone()
    s.synchronize()
    if want_loss == "lagged":
        assert loss is None and tr.last_grad_norm is None
        loss = tr.flush_loss()
        norm = tr.last_grad_norm
    elif want_loss is False:
        assert loss is None and tr.last_grad_norm is None
        loss = _loss_on(L, hd, s)
        nv, v = C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_grad_norm(hd, C.byref(nv), C.byref(v), s.cuda_stream))
        assert v.value == 1
        norm = nv.value
    else:
        norm = tr.last_grad_norm
    tr.check_status()
    n = o.flat.size
    og = E._compare("streams clipped averaged step, want_loss=%r" % (want_loss,), o, None, loss, _np(g)[:n])
    _check_optimiser("clipped averaged step", o, dec, og, o.flat, _np(g)[:n], None, max_norm, _np(w), _np(mo), _np(vo), norm, _np(ema), decay)


# ---------------------------------------------------------------- 4. accumulation
def test_accumulation_window_on_a_stream_with_late_chunks(cuda, gate):
    """accum_steps = 2, lagged losses: micro-step 0 reads the real chunk behind a gate (the buffers held the decoy), micro-step 1 a second real chunk behind a gate of
    its own (the buffers then hold the first chunk: reading early would accumulate it twice).  Micro-step 0 ends in the accumulate kernel, which carries the status word
    and the loss to pinned memory.  Against the union-batch oracle as in test_grad_accum_gpu.test_two_windows_equal_the_union_batch_oracle: every micro-step's loss and
    row-weighted gradient, the accumulator over its trailer against the row-weighted mean, the weights against the oracle's Adam on that mean."""
    import torch
    from oracle import train_oracle as TO
    from qpnet_amd.train import FusedTrainer
    o, dec, o2 = _chunk("paper", REAL), _chunk("paper", DECOY), _chunk("paper", SECOND)
    _teeth(o, dec)
    _teeth(o2, o)
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4, accum_steps=2)
    late = _train_late(cuda, o, dec)
    k2 = late.more(cuda, (o2.x, o2.h, o2.t, o2.d))
    xb, hb, tb, db = late.buf
    _prime(tr, late, o, cuda)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        assert tr.step(xb, hb, tb, db, o.b, want_loss="lagged", maxd=o.maxd) is None
        _still_closed(s, "qpn_train_step_acc (micro-step 0) with loss_mode 1")
        g0 = tr.g.clone()
        late.deliver(gate, k2)
        loss0 = tr.step(xb, hb, tb, db, o2.b, want_loss="lagged", maxd=o2.maxd)      # (waits for micro-step 0's loss, not for this micro-step)
        _still_closed(s, "qpn_train_step_acc (micro-step 1) with loss_mode 1")
        g1, acc, w = tr.g.clone(), tr.acc.clone(), m._flat.clone()
    s.synchronize()
    loss1 = tr.flush_loss()
    tr.check_status()
    assert tr.step_count == 1 and tr.micro_step == 0
    n, rows = o.flat.size, [o.x.shape[0] * o.BL, o2.x.shape[0] * o2.BL]
    matched = []
    for k, (oo, g, loss) in enumerate(((o, _np(g0), loss0), (o2, _np(g1), loss1))):
        np.testing.assert_array_equal(g[n:], np.array([rows[k], 0, 0, 0], F))
        matched.append(E._compare("streams accumulation micro-step %d" % k, oo, None, loss, g[:n] / F(rows[k])))
    acc = _np(acc)
    np.testing.assert_array_equal(acc[n:], np.array([sum(rows), 0, 0, 0], F))
    union = (sum(g.astype(np.float64) * r for g, r in zip(matched, rows)) / sum(rows)).astype(F)
    util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, acc[:n] / acc[n], og=union)
    # (what a window that read the first chunk twice would hold is that chunk's own gradient)
    assert np.abs(matched[0] - union).max() >= 100 * (2e-5 + 1e-4) * np.abs(union).max()
    _weights_after_adam(o, union, _np(w))


# ---------------------------------------------------------------- 5. the early bucket
def test_early_bucket_stream_orders_itself_against_the_callers_stream(cuda, gate, monkeypatch):
    """world_size = 2 without a process group (the identity exchange of test_grad_clip_gpu.test_world2_with_the_identity_exchange_clips_like_world1), two buckets:
    the tail of the gradient goes out on the trainer's own early-bucket stream, which waits for the backward's event and is joined by the caller's stream.  The
    step must be the world_size = 1 step: loss, gradient (n g | n), the clipped norm of the averaged gradient, moments and weights."""
    import torch
    from qpnet_amd.train import FusedTrainer
    monkeypatch.setenv("QPN_EXCHANGE_BUCKETS", "2")
    o, dec = _chunk("paper", REAL), _chunk("paper", DECOY)
    _teeth(o, dec)
    max_norm = 0.5 * _norm64(o.og)
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=GC.LR, weight_decay=GC.WD, world_size=2, max_grad_norm=max_norm)
    late = _train_late(cuda, o, dec)
    xb, hb, tb, db = late.buf
    _prime(tr, late, o, cuda)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        assert tr.step(xb, hb, tb, db, o.b, want_loss="lagged", maxd=o.maxd) is None
        _still_closed(s, "the data-parallel step with a lagged loss")
        g, w, mo, vo = tr.g.clone(), m._flat.clone(), tr.m.clone(), tr.v.clone()
    s.synchronize()
    loss = tr.flush_loss()
    norm = tr.last_grad_norm
    tr.check_status()
    assert tr._two_buckets and tr.last_buckets[0] > 0 and tr.last_buckets[1] > 0, tr.last_buckets
    n, rows = o.flat.size, o.x.shape[0] * o.BL
    g = _np(g)
    np.testing.assert_array_equal(g[n:], np.array([rows, 0, 0, 0], F))
    og = E._compare("streams world_size=2, two buckets", o, None, loss, g[:n] / F(rows))
    _check_optimiser("world_size=2, two buckets", o, dec, og, o.flat, g[:n], float(rows), max_norm, _np(w), _np(mo), _np(vo), norm)


# ---------------------------------------------------------------- 6. one handle, two streams
def test_three_lagged_steps_switching_streams_vs_the_torch_port(cuda, gate):
    """Step 1 on s1, step 2 on s2 after s2.wait_stream(s1), step 3 on s1 after s1.wait_stream(s2), each behind its own gate (a step's decoy is the chunk before it,
    still in the buffers; the first one's is the decoy chunk): the lagged loss and status slots keep one event per slot, recorded on whichever stream the call was
    given.  Every loss arrives one step late and equals oracle/train_torch.py's within 1e-4; the weights after the three steps as in
    test_train_gpu.test_three_fused_steps_at_the_bench_shape_vs_the_torch_port, at this small shape.  Teeth: at every step the torch port's loss of the decoy, at the
    same weights, is >= 100 x 1e-4 away."""
    import torch
    from oracle import train_torch as TT
    from qpnet_amd.train import FusedTrainer
    # (ascending losses at the shared weights: the chunk a step has just trained on -- the next step's decoy -- has by then a loss ~0.017 lower still)
    chunks = [_chunk("paper", sd) for sd in (THIRD, SECOND, REAL)]
    decoys = [_chunk("paper", REAL)] + chunks[:2]
    o = chunks[0]
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4)
    late = _train_late(cuda, o, decoys[0])
    for c in chunks[1:]:
        assert c.maxd == o.maxd and c.BL == o.BL
        late.more(cuda, (c.x, c.h, c.t, c.d))
    xb, hb, tb, db = late.buf
    _prime(tr, late, o, cuda)
    ref = TT.Trainer(o.cfg, o.flat, lr=1e-4)
    want, grads = [], []
    for c, dc in zip(chunks, decoys):
        dloss, _ = ref.loss_and_grad(dc.x, dc.h, dc.t, dc.d, dc.b)
        loss, grad = ref.loss_and_grad(c.x, c.h, c.t, c.d, c.b)
        assert abs(dloss - loss) >= 100 * 1e-4, (dloss, loss)
        want.append(loss); grads.append(grad.copy())
        ref.opt.step()
    s1 = _start(cuda)
    s2 = torch.cuda.Stream(cuda)
    got, prev = [], None
    for k, s in enumerate((s1, s2, s1)):
        if prev is not None:
            s.wait_stream(prev)
        with torch.cuda.stream(s):
            late.deliver(gate, k)
            got.append(tr.step(xb, hb, tb, db, o.b, want_loss="lagged", maxd=o.maxd))
            _still_closed(s, "qpn_train_step with loss_mode 1 (step %d)" % (k + 1))
        prev = s
    got.append(tr.flush_loss())
    s1.synchronize(); s2.synchronize()
    tr.check_status()
    print("STREAMS three lagged steps on s1, s2, s1: losses", got[1:], "torch port", want)
    assert got[0] is None
    np.testing.assert_allclose(got[1:], want, atol=1e-4, rtol=0)
    util.assert_weights_after_adam(_np(m.flat_parameters()), ref.flat.detach().numpy(), 1e-4, 3, far=2.0,
                                   significant=util.significant_elements(o.cfg, grads), sig_max=3e-5, sig_frac=0.02)


def test_a_flagged_step_is_reported_and_cleared_across_a_stream_switch(cuda, gate):
    """The graceful path of test_train_gpu.test_fused_step_reports_a_bad_chunk_at_the_next_step -- a status word, not a fault -- over two streams.  Step 1 on s1
    carries one target equal to Q behind its gate (its decoy is clean: a step that read early would raise no flag), step 2 is clean, on s2.  Neither may change
    a parameter (bit-equal); the report arrives with the third call at the latest; the first clean step after the report is applied, counted by
    qpn_train_applied_updates, and equals the oracle's step from the unchanged weights.  In between the caller hands the trainer back from s2 to s1 and keeps
    s2 busy with work of its own (a sleep kernel standing for a prefetch): clearing the sticky word must be ordered on the stream the trainer is called on,
    in front of the next step -- behind other work on the stream of an earlier call it would land after that step's Adam launch had looked at the word."""
    import torch
    from qpnet_amd.train import FusedTrainer
    o, dec, o2, o3 = _chunk("paper", REAL), _chunk("paper", DECOY), _chunk("paper", SECOND), _chunk("paper", THIRD)
    _teeth(o3, o2)
    Q = o.cfg.n_quantize
    bad = o.t.copy()
    bad[0, -5] = Q
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4)
    late = _Late(cuda, (o.x, o.h, bad, o.d), (dec.x, dec.h, dec.t, dec.d))
    k2, k3 = late.more(cuda, (o2.x, o2.h, o2.t, o2.d)), late.more(cuda, (o3.x, o3.h, o3.t, o3.d))
    xb, hb, tb, db = late.buf
    L, hd = _prime(tr, late, o, cuda)
    applied0 = tr._applied_base[1]
    w0 = m.flat_parameters().clone()
    s1 = _start(cuda)
    s2 = torch.cuda.Stream(cuda)
    with torch.cuda.stream(s1):
        late.deliver(gate)
        tr.step(xb, hb, tb, db, o.b, want_loss=False, maxd=o.maxd)                     # flagged on the device, not yet seen
        _still_closed(s1, "qpn_train_step with loss_mode 0 (the flagged step)")
        w1 = m._flat.clone()
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        late.deliver(gate, k2)
        tr.step(xb, hb, tb, db, o.b, want_loss=False, maxd=o.maxd)                     # clean, behind the flagged one: skipped on the device
        _still_closed(s2, "qpn_train_step with loss_mode 0 (the clean step behind it)")
        w2 = m._flat.clone()
    s1.wait_stream(s2)                                                                 # the trainer goes back to s1 ...
    with torch.cuda.stream(s2):
        torch.cuda._sleep(4 * gate.cycles)                                             # ... and s2 goes on with work of its own, longer than the next step's gate
    with torch.cuda.stream(s1):
        with pytest.raises(_lib.QpnError) as e:
            tr.step(xb, hb, tb, db, o.b, want_loss=False, maxd=o.maxd)                 # raised before anything of this step is enqueued
        assert e.value.code == -4 and "target class" in str(e.value)
        assert tr.step_count == 0
        late.deliver(gate, k3)
        tr.step(xb, hb, tb, db, o.b, want_loss=False, maxd=o.maxd)
        _still_closed(s1, "qpn_train_step with loss_mode 0 (the first step after the report)")
        g, w = tr.g.clone(), m._flat.clone()
    s1.synchronize()
    assert torch.equal(w1, w0) and torch.equal(w2, w0)
    n = C.c_int64(-1)
    _lib.check(L.qpn_train_applied_updates(hd, C.byref(n), s1.cuda_stream))
    assert n.value == applied0 + 1 and tr.step_count == 1, (n.value, applied0, tr.step_count)
    loss = _loss_on(L, hd, s1)
    s2.synchronize()
    tr.check_status()
    og = E._compare("streams first clean step after the report", o3, None, loss, _np(g)[:o.flat.size])
    _weights_after_adam(o3, og, _np(w), dec=o2)


# ---------------------------------------------------------------- decode
DECODE_UTTS, DECOY_UTTS = [(61, 4, 1.0), (62, 3, 0.5)], [(71, 4, 1.0), (72, 3, 0.5)]
DECODE_CASES = [(k, "argmax") for k in D._TIE_KERNELS] + [("pipe", "sampling"), ("coopb", "sampling")]
DECODE_IDS = ["%s-%s" % c for c in DECODE_CASES]
SAMPLING_SEED = 5
LOGITS_SEED = 0x9E3779B97F4A7C15           # qpn_sample_logits' seed (test_sampling_controls_gpu's)


def _rows(oracle, cfg, flat, bx, bh, bd, ns, mode):
    """the oracle's streams in INPUT order"""
    outs = oracle.batch_fast_generate(cfg, flat, bx, bh, list(ns), bd, mode=mode, seed=SAMPLING_SEED)
    order = sorted(range(len(ns)), key=lambda i: ns[i])
    rows = [None] * len(ns)
    for pos, i in enumerate(order):
        rows[i] = outs[pos]
    return rows


SEED_SAMPLES = 100                    # the seed x of a call: long enough that the greedy streams depend on it (a single seed sample moves under 1 % of them)


@functools.lru_cache(maxsize=None)
def _decode_inputs(kernel):
    """(cfg, weights, decoy weights, real (x, h, d32, d64), decoy (x, h, d32, d64), ns): two ragged rows of 4 and 3 frames behind a seed of SEED_SAMPLES samples.
    The decoy: other seed samples, other features and pitch contours, the factors clipped to the real batch's ceil(max d) with one factor ON it (the rings
    have the real batch's lengths)"""
    geo = D._TIE_KERNELS[kernel][0]
    cfg = PAPER if geo is None else QPNetConfig(**geo)
    _, bh, bd, ns = util.decode_batch(cfg, DECODE_UTTS)
    _, dh, dd, dns = util.decode_batch(cfg, DECOY_UTTS)
    assert list(dns) == list(ns) and dd.shape == bd.shape and dh.shape == bh.shape
    rs = np.random.RandomState(3)
    bx, dx = (rs.randint(0, cfg.n_quantize, (len(ns), SEED_SAMPLES)).astype(np.int64) for _ in range(2))
    ns = [n - SEED_SAMPLES + 1 for n in ns]
    maxd = int(np.nanmax(np.ceil(bd)))
    dd = np.where(dd > 0, np.minimum(dd, float(maxd) - 0.25), 0.0)
    dd[1, 7] = float(maxd)
    assert int(np.nanmax(np.ceil(dd))) == maxd and dd[dd > 0].min() > 0.5
    f32 = lambda a: a.astype(F)
    return cfg, synth.make_weights(cfg, 29), synth.make_weights(cfg, 30), (bx, bh, f32(bd), bd), (dx, dh, f32(dd), dd), ns


@functools.lru_cache(maxsize=None)
def _decode_want(kernel, mode):
    """The oracle's streams of the real input (input order), after the teeth: the decoy's streams differ from them in >= 10 % of every row's samples, and with any ONE
    of x, h, d -- or the weights -- replaced by the decoy's every row still differs in three samples at least (the comparison is bit for bit): each late input counts
    by itself.  (Once per kernel and mode.)"""
    from oracle import cpu_oracle as oracle
    cfg, flat, dflat, real, decoy, ns = _decode_inputs(kernel)
    want = _rows(oracle, cfg, flat, real[0], real[1], real[2], ns, mode)
    whole = _rows(oracle, cfg, flat, decoy[0], decoy[1], decoy[2], ns, mode)
    assert min(float((a != b).mean()) for a, b in zip(whole, want)) >= 0.10
    counts = []
    for k in range(3):
        mixed = [decoy[j] if j == k else real[j] for j in range(3)]
        counts.append(min(int((a != b).sum()) for a, b in zip(_rows(oracle, cfg, flat, mixed[0], mixed[1], mixed[2], ns, mode), want)))
    counts.append(min(int((a != b).sum()) for a, b in zip(_rows(oracle, cfg, dflat, real[0], real[1], real[2], ns, mode), want)))
    print("STREAMS decode teeth, %s %s: of %s samples a row, the whole decoy moves %s; only x / h / d / the weights the decoy's: at least %d / %d / %d / %d" %
          ((kernel, mode, ns, [int((a != b).sum()) for a, b in zip(whole, want)]) + tuple(counts)))
    assert min(counts) >= 3, counts
    return want


def _decode_setup(kernel, mode, cuda, oracle, monkeypatch, late_weights=False):
    """model, late inputs, and the call's arguments as QPNet._decode_args prepares them, after one blocking decode of the DECOY on the default stream: it sizes the
    handle's buffers (growing one frees the old one, which waits for the device), loads the code objects, names the plan -- and must give the decoy's own stream"""
    import torch
    from qpnet_amd.train import ensure_flat
    geo, env, plan = D._TIE_KERNELS[kernel]
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, flat, dflat, real, decoy, ns = _decode_inputs(kernel)
    want = _decode_want(kernel, mode)
    w_first = dflat if late_weights else flat
    m = util.build_model(cfg, w_first, cuda)
    m.sampling_seed = SAMPLING_SEED
    late = _Late(cuda, real[:3], decoy[:3])
    if late_weights:
        late.buf.append(ensure_flat(m, cuda))
        late.stage[0].append(torch.from_numpy(flat.copy()).to(cuda))
    xb, hb, db = late.buf[:3]
    outs = m.batch_fast_generate(xb, hb, list(ns), db, mode=mode, extra_memory=True)
    assert plan in m.last_decode_plan, m.last_decode_plan
    own = _rows(oracle, cfg, w_first, decoy[0], decoy[1], decoy[2], ns, mode)
    for pos, i in enumerate(sorted(range(len(ns)), key=lambda i: ns[i])):
        np.testing.assert_array_equal(outs[pos], own[i], err_msg="the decoy's own stream, row %d" % i)
    a = m._decode_args(xb, hb, list(ns), db, mode, True)
    assert a["keep"][0].data_ptr() == xb.data_ptr() and a["keep"][1].data_ptr() == hb.data_ptr() and a["keep"][2].data_ptr() == db.data_ptr()
    return m, late, a, ns, want, plan


def _assert_streams(out, ns, want, what):
    out = _np(out)
    for b, n in enumerate(ns):
        np.testing.assert_array_equal(out[b, :n], want[b], err_msg="%s: row %d" % (what, b))


@pytest.mark.parametrize("kernel,mode", DECODE_CASES, ids=DECODE_IDS)
def test_blocking_decode_on_a_stream_with_late_inputs(kernel, mode, cuda, gate, oracle, monkeypatch):
    """x, h and float32 d arrive behind the gate; the known-sample prelude, the ring clear, the status clear and the auxiliary projection go to the call's stream ahead
    of the persistent launch.  Driven through the C ABI (qpn_decode) with the arguments QPNet._decode_args prepared during set-up: batch_fast_generate(extra_memory=True)
    itself reads ceil(max d) back from the device before it calls the library, which waits for the gate.  It runs as well, second, under the same stream with the
    decoy put back and the real input late again -- by then a check of the stream it picks up and of its result, not a race."""
    import torch
    m, late, a, ns, want, plan = _decode_setup(kernel, mode, cuda, oracle, monkeypatch)
    L, hd = a["L"], a["hd"]
    decoy = [b.clone() for b in late.buf]
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_decode(*(a["call"][:-1] + (s.cuda_stream,))))
        out = a["out"].clone()
    s.synchronize()
    assert plan in L.qpn_last_decode_plan(hd).decode(), L.qpn_last_decode_plan(hd)
    _assert_streams(out, ns, want, "%s %s through qpn_decode" % (kernel, mode))
    with torch.cuda.stream(s):
        for b, d in zip(late.buf, decoy):
            b.copy_(d)
        late.deliver(gate)
        outs = m.batch_fast_generate(late.buf[0], late.buf[1], list(ns), late.buf[2], mode=mode, extra_memory=True)
    assert plan in m.last_decode_plan, m.last_decode_plan
    order = sorted(range(len(ns)), key=lambda i: ns[i])
    for pos, i in enumerate(order):
        np.testing.assert_array_equal(outs[pos], want[i], err_msg="%s %s through batch_fast_generate: row %d" % (kernel, mode, i))


@pytest.mark.parametrize("kernel,mode", DECODE_CASES, ids=DECODE_IDS)
def test_blocking_decode_with_late_weights(kernel, mode, cuda, gate, oracle, monkeypatch):
    """... and the flat weights themselves arrive behind the gate, over decoy weights from another seed: the pack and bias-fold launches of qpn_set_weights are ordered on
    the stream too.  qpn_set_weights and qpn_decode through the C ABI with QPNet._decode_args' arguments (see above); qpn_set_weights must return with the gate closed."""
    import torch
    m, late, a, ns, want, plan = _decode_setup(kernel, mode, cuda, oracle, monkeypatch, late_weights=True)
    L, hd = a["L"], a["hd"]
    flat = late.buf[3]
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_set_weights(hd, flat.data_ptr(), flat.numel(), s.cuda_stream))
        _still_closed(s, "qpn_set_weights")
        _lib.check(L.qpn_decode(*(a["call"][:-1] + (s.cuda_stream,))))
        out = a["out"].clone()
    s.synchronize()
    assert plan in L.qpn_last_decode_plan(hd).decode(), L.qpn_last_decode_plan(hd)
    _assert_streams(out, ns, want, "%s %s, late weights" % (kernel, mode))


@pytest.mark.parametrize("kernel,mode", DECODE_CASES, ids=DECODE_IDS)
def test_asynchronous_decode_returns_while_the_gate_is_closed(kernel, mode, cuda, gate, oracle, monkeypatch):
    """qpn_decode_enqueue returns while s is still gated; qpn_decode_finish waits; the output is cloned on s"""
    import torch
    m, late, a, ns, want, plan = _decode_setup(kernel, mode, cuda, oracle, monkeypatch)
    L, hd = a["L"], a["hd"]
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_decode_enqueue(*(a["call"][:-1] + (s.cuda_stream,))))
        _still_closed(s, "qpn_decode_enqueue")
        _lib.check(L.qpn_decode_finish(hd, s.cuda_stream))
        out = a["out"].clone()
    s.synchronize()
    assert plan in L.qpn_last_decode_plan(hd).decode(), L.qpn_last_decode_plan(hd)
    _assert_streams(out, ns, want, "%s %s through qpn_decode_enqueue / qpn_decode_finish" % (kernel, mode))


@pytest.mark.parametrize("kernel,mode", DECODE_CASES, ids=DECODE_IDS)
def test_live_decode_on_a_stream(kernel, mode, cuda, gate, oracle, monkeypatch):
    """generate_live iterated to its end under s, x and h late, the factors as float64 numpy (their host-to-device copy on s waits for the gate: what is checked is the
    stream the call, its polls and its finish run on): every row's pieces are contiguous and concatenate to the oracle's stream"""
    import torch
    geo, env, plan = D._TIE_KERNELS[kernel]
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, flat, _, real, decoy, ns = _decode_inputs(kernel)
    want = _rows(oracle, cfg, flat, real[0], real[1], real[3], ns, mode)
    assert min(float((a != b).mean()) for a, b in zip(_rows(oracle, cfg, flat, decoy[0], decoy[1], real[3], ns, mode), want)) >= 0.10
    m = util.build_model(cfg, flat, cuda)
    m.sampling_seed = SAMPLING_SEED
    late = _Late(cuda, real[:2], decoy[:2])
    s = _start(cuda)
    got = [[] for _ in ns]
    with torch.cuda.stream(s):
        late.deliver(gate)
        for b, start, piece in m.generate_live(late.buf[0], late.buf[1], list(ns), real[3], mode=mode, every=64):
            assert start == sum(len(p) for p in got[b]), "row %d: a piece starts at %d, %d samples delivered" % (b, start, sum(len(p) for p in got[b]))
            got[b].append(piece)
    s.synchronize()
    assert plan in m.last_decode_plan, m.last_decode_plan
    assert m.last_decode_counts == list(ns) and not m.last_decode_cancelled
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(got[b]), want[b], err_msg="%s %s live: row %d" % (kernel, mode, b))


# ---------------------------------------------------------------- the standalone kernels
@pytest.fixture(scope="module")
def handle(cuda):
    """one TINY handle for the C-ABI calls on hand-made buffers"""
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _unaligned(late):
    """every buffer of `late` moved one float into an allocation of its own (a base that is not 16-byte aligned)"""
    import torch
    for i, b in enumerate(late.buf):
        t = torch.empty(b.numel() + 1, dtype=b.dtype, device=b.device)
        t[1:].copy_(b)
        late.buf[i] = t[1:]
        assert late.buf[i].data_ptr() % 16 == 4


def test_adam_step_avg_and_the_norm_with_late_buffers(cuda, gate, handle):
    """qpn_adam_step_avg at n = 257 from an unaligned base, with a clipping denominator buffer {700, 0, 0, 0}, clipping binding and the average: weights, gradient, both
    moments, the average AND the denominator arrive behind the gate.  Then qpn_train_grad_norm.  Restatements and bounds of test_grad_clip_gpu.test_clip_step_matches_numpy
    and test_ema_gpu.test_one_call_against_numpy."""
    import torch
    L, hp = handle
    n, den, dden, decay = 257, 700.0, 300.0, 0.9
    w0, g0, m0, v0, e0 = EM._buffers(n, 2257)
    real = (w0, (g0 * F(den)).astype(F), m0, v0, e0, np.array([den, 0, 0, 0], F))
    dw, dg, dm, dv, de = EM._buffers(n, 3257)
    decoy = (dw, (dg * F(dden)).astype(F), dm, dv, de, np.array([dden, 0, 0, 0], F))
    total = _norm64(g0 * F(den) / F(den))
    max_norm = 0.5 * total
    late = _Late(cuda, real, decoy)
    _unaligned(late)
    w, g, mo, vo, e, dd = late.buf
    # set-up: the training state of the handle (the partial sums and the norm word live in it) and the kernels' code objects, on copies of the decoy
    c = [b.clone() for b in late.buf]
    _lib.check(L.qpn_adam_step_avg(hp, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), n, GC.STEP, GC.LR, GC.B1, GC.B2, GC.EPS, GC.WD,
                                   c[5].data_ptr(), max_norm, c[4].data_ptr(), decay, torch.cuda.current_stream(cuda).cuda_stream))
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), mo.data_ptr(), vo.data_ptr(), n, GC.STEP, GC.LR, GC.B1, GC.B2, GC.EPS, GC.WD,
                                       dd.data_ptr(), max_norm, e.data_ptr(), decay, s.cuda_stream))
        _still_closed(s, "qpn_adam_step_avg")
        got = [t.clone() for t in (w, g, mo, vo, e)]
        norm, valid = C.c_double(-1.0), C.c_int(-1)
        _lib.check(L.qpn_train_grad_norm(hp, C.byref(norm), C.byref(valid), s.cuda_stream))
    s.synchronize()
    assert L.qpn_train_status(hp, s.cuda_stream) == 0
    wg, gg, mg, vg, eg = (_np(t) for t in got)
    assert valid.value == 1
    np.testing.assert_allclose(norm.value, _norm64(real[1]) / den, rtol=1e-7, atol=0)
    np.testing.assert_allclose(norm.value, total, rtol=1e-6, atol=0)
    coef = GC._coef(total, max_norm)
    assert coef < 0.51
    wr, mr, vr = GC._ref_adam(w0, real[1], m0, v0, coef, den=den)
    np.testing.assert_allclose(wg, wr, rtol=0, atol=2e-6)
    np.testing.assert_allclose(mg, mr, rtol=0, atol=1e-5 * np.abs(mr).max())
    np.testing.assert_allclose(vg, vr, rtol=0, atol=4e-5 * np.abs(vr).max())
    np.testing.assert_array_equal(gg, real[1])
    r, bound = EM._ema_ref(wg, e0, decay)
    assert (np.abs(eg.astype(np.float64) - r.astype(np.float64)) <= bound).all()
    # teeth: the decoy's result is far from the real one; so is the real gradient's norm over the decoy's denominator (while clipping binds, the clipped update
    # itself does not depend on the denominator: a denominator read too early shows in the norm)
    dtotal = _norm64(decoy[1]) / dden
    wd, md, vd = GC._ref_adam(dw, decoy[1], dm, dv, GC._coef(dtotal, max_norm), den=dden)
    assert np.abs(wd - wr).max() >= 100 * 2e-6 and np.abs(md - mr).max() >= 100 * 1e-5 * np.abs(mr).max() and np.abs(vd - vr).max() >= 100 * 4e-5 * np.abs(vr).max()
    assert abs(dtotal - total) >= 100 * 1e-6 * total and abs(total * den / dden - total) >= 100 * 1e-6 * total
    assert (np.abs(EM._ema_ref(wd, de, decay)[0].astype(np.float64) - r) > 100 * bound).any()


def test_grad_accumulate_with_late_buffers(cuda, gate, handle):
    """qpn_grad_accumulate with first = 1 (the accumulator holds NaNs, the gradient buffer a decoy until the gate opens), then with first = 0 and a second vector
    late in the same buffer: exactly g, then numpy's float32 a + b, bit for bit (test_grad_accum_gpu.test_kernel_against_numpy), from unaligned bases"""
    import torch
    L, hp = handle
    cnt = 1029
    rs = np.random.RandomState(4101)
    a, decoy = (rs.standard_normal(cnt) * 3.0).astype(F), (rs.standard_normal(cnt) * 3.0).astype(F)
    b = (rs.standard_normal(cnt) * 3.0 * 10.0 ** rs.randint(-3, 4, cnt)).astype(F)
    want = a + b
    assert ((decoy + b) != want).mean() >= 0.10 and ((a + a) != want).mean() >= 0.10 and (decoy != a).mean() >= 0.10
    late = _Late(cuda, (a,), (decoy,))
    kb = late.more(cuda, (b,))
    _unaligned(late)
    g, = late.buf
    acc = torch.full((cnt + 1,), float("nan"), dtype=torch.float32, device=cuda)[1:]
    c = acc.clone()
    _lib.check(L.qpn_grad_accumulate(hp, c.data_ptr(), g.data_ptr(), cnt, 1, torch.cuda.current_stream(cuda).cuda_stream))      # (set-up: the code object)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_grad_accumulate(hp, acc.data_ptr(), g.data_ptr(), cnt, 1, s.cuda_stream))
        _still_closed(s, "qpn_grad_accumulate (first = 1)")
        first = acc.clone()
        late.deliver(gate, kb)
        _lib.check(L.qpn_grad_accumulate(hp, acc.data_ptr(), g.data_ptr(), cnt, 0, s.cuda_stream))
        _still_closed(s, "qpn_grad_accumulate (first = 0)")
        second = acc.clone()
    s.synchronize()
    assert np.array_equal(_np(first).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(_np(second).view(np.uint32), want.view(np.uint32))


def test_ce_loss_with_late_logits_and_targets(cuda, gate, handle):
    """qpn_ce_loss without a host loss pointer (with one it reads the loss in the call): dL/dlogits and the loss against train_oracle.ce_loss at the bounds of
    test_saturation_gpu.test_ce_loss_on_hand_made_rows; the target rows are longer than batch_length"""
    import torch
    from oracle import train_oracle as TO
    L, hp = handle
    B, BL, Q, pad = 2, 37, TINY.n_quantize, 3
    rs = np.random.RandomState(77)
    lg, dlg = (2.0 * rs.standard_normal((B, BL, Q))).astype(F), (2.0 * rs.standard_normal((B, BL, Q))).astype(F)
    t, dt = rs.randint(0, Q, (B, pad + BL)).astype(np.int64), rs.randint(0, Q, (B, pad + BL)).astype(np.int64)
    ref_loss, ref_dl = TO.ce_loss(lg, t[:, pad:])
    bound_loss, bound_dl = 1e-4 * max(1.0, abs(ref_loss)), 2e-5 / (B * BL)
    for a, b in ((dlg, dt), (dlg, t), (lg, dt)):                    # the decoy, and either input alone the decoy's
        l2, d2 = TO.ce_loss(a, b[:, pad:])
        assert abs(l2 - ref_loss) >= 100 * bound_loss and np.abs(d2 - ref_dl).max() >= 100 * bound_dl
    late = _Late(cuda, (lg, t), (dlg, dt))
    lb, tb = late.buf
    dl = torch.full((B, BL, Q), float("nan"), device=cuda)
    scratch = dl.clone()
    _lib.check(L.qpn_ce_loss(hp, lb.data_ptr(), tb.data_ptr(), tb.shape[1], B, BL, scratch.data_ptr(), None, torch.cuda.current_stream(cuda).cuda_stream))      # (set-up: the code object)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_ce_loss(hp, lb.data_ptr(), tb.data_ptr(), tb.shape[1], B, BL, dl.data_ptr(), None, s.cuda_stream))
        _still_closed(s, "qpn_ce_loss")
        got = dl.clone()
    s.synchronize()
    loss = _loss_on(L, hp, s)
    assert L.qpn_train_status(hp, s.cuda_stream) == 0
    print("STREAMS ce: loss %.7f (ref %.7f)" % (loss, ref_loss))
    assert abs(loss - ref_loss) <= bound_loss
    np.testing.assert_allclose(_np(got), ref_dl, atol=bound_dl, rtol=0)


def test_sample_logits_with_late_rows(cuda, gate, oracle):
    """qpn_sample_logits with the controls on (temperature 0.7, top_k 40), bit for bit against tests/sampling_spec.py"""
    import torch
    n, Q, T, k, step0 = 300, 256, 0.7, 40, 70003
    rs = np.random.RandomState(4242)
    rows, decoy = (4.0 * rs.standard_normal((n, Q))).astype(F), (4.0 * rs.standard_normal((n, Q))).astype(F)
    u = SS.uniforms(LOGITS_SEED, 2, range(step0, step0 + n))
    want = SS.draw(rows, u, T, k)
    assert (SS.draw(decoy, u, T, k) != want).mean() >= 0.10
    late = _Late(cuda, (rows,), (decoy,))
    lg, = late.buf
    out = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    L = _lib.lib()
    scratch = out.clone()
    _lib.check(L.qpn_sample_logits(lg.data_ptr(), n, Q, LOGITS_SEED, 2, step0, T, k, scratch.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream))      # (set-up: the code object)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_sample_logits(lg.data_ptr(), n, Q, LOGITS_SEED, 2, step0, T, k, out.data_ptr(), s.cuda_stream))
        _still_closed(s, "qpn_sample_logits")
        got = out.clone()
    s.synchronize()
    np.testing.assert_array_equal(_np(got), want)


@pytest.mark.parametrize("tag,decoy_tag", [("h", "1"), ("1", "x"), ("x", "h")])
def test_dilated_index_exports_with_late_factors(tag, decoy_tag, cuda, gate, golden_dir):
    """qpn_dilated_index_{train, gen_f32, gen_f64} on tests/golden/kat.npz, the factors late over another tag's (whose own index tensors are in the file: the decoy's
    result differs from the real one in every tenth entry at least)"""
    import torch
    L = _lib.lib()
    kat = np.load(golden_dir + "/kat.npz")
    d64, x64 = kat["didx_d64_" + tag], kat["didx_d64_" + decoy_tag]
    B, n = d64.shape
    late = _Late(cuda, (d64.astype(F), d64), (x64.astype(F), x64))
    t32, t64 = late.buf
    calls = []
    for k in range(4):
        for name, src, dtype in (("train_f32", t32, torch.int64), ("gen_f32", t32, torch.int64), ("gen_f64", t64, torch.int32)):
            want, other = kat["didx_%s_%s_%d" % (name, tag, k)], kat["didx_%s_%s_%d" % (name, decoy_tag, k)]
            assert (want != other).mean() >= 0.10
            calls.append((name, k, src, torch.empty((B, n), dtype=dtype, device=cuda), want))

    def run(name, k, src, out, stream):
        if name == "train_f32":
            _lib.check(L.qpn_dilated_index_train(src.data_ptr(), B, n, 2 ** k, out.data_ptr(), stream))
        elif name == "gen_f32":
            _lib.check(L.qpn_dilated_index_gen_f32(src.data_ptr(), B * n, 2 ** k, out.data_ptr(), stream))
        else:
            _lib.check(L.qpn_dilated_index_gen_f64(src.data_ptr(), B * n, 2 ** k, out.data_ptr(), stream))

    for name, k, src, out, _ in calls[:3]:
        run(name, k, src, out, torch.cuda.current_stream(cuda).cuda_stream)      # (set-up: the three code objects)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        for name, k, src, out, _ in calls:
            run(name, k, src, out, s.cuda_stream)
        _still_closed(s, "the qpn_dilated_index_* exports")
    s.synchronize()
    for name, k, _, out, want in calls:
        np.testing.assert_array_equal(_np(out), want, err_msg="%s, dilation %d" % (name, 2 ** k))
