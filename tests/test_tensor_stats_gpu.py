"""GPU: per-tensor training statistics (qpn_tensor_stats, FusedTrainer.tensor_stats / FlatAdam.tensor_stats, run_train --stats_interval).

The C-ABI cases run on ONE small table, tensor sizes 1, 1, 110, 3, 256, 2 * ITEM + 3, 64 (ITEM = 2048, the work-item length of train_stats_plan.h): the smallest
table with single-element tensors, an unaligned start (the multi-item tensor begins 3 floats past a 16-byte boundary, as every tensor behind the upsampling pair of a
real model does), a tensor of several items with a short last one, and a short tail.

Expected values are a numpy float64 restatement from the fp32 inputs.  Bounds, derived, not measured:
  grad_sumsq, weight_sumsq  an fp32 square is exact in fp64, so the device sum is good to n * 2^-53 relative (n <= 4099: 5e-13); 1e-12
  update_sumsq              every u_i is a few fp32 roundings (a square root, two divisions, an addition) in the operations the restatement uses too; 4 ulp on u, 2 * 4 * 2^-24 = 5e-7
                            on its square; 2e-6
  absmax, counts            exact"""
import collections
import ctypes as C
import itertools
import json
import logging
import math
import os

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY
import test_grad_clip_gpu as GC
import util

pytestmark = pytest.mark.gpu

F = np.float32
ITEM = 2048                                   # QPN_STATS_ITEM (tests/test_tensor_stats_cpu.py holds it against the header's)
SIZES = [1, 1, 110, 3, 256, 2 * ITEM + 3, 64]
ENDS = list(itertools.accumulate(SIZES))
N = ENDS[-1]
B1, B2, EPS, STEP, DEN = 0.9, 0.999, 1e-8, 3, 3.0
Rec = collections.namedtuple("Rec", "grad_sumsq weight_sumsq update_sumsq grad_absmax weight_absmax grad_nonfinite")


def test_the_table_is_the_one_the_cases_rely_on():
    starts = [0] + ENDS[:-1]
    assert SIZES[0] == SIZES[1] == 1 and starts[5] % 4 == 3 and SIZES[5] > 2 * ITEM and SIZES[5] % ITEM == 3 and SIZES[6] < 256 and N % 4 != 0


def _fsum_sq(x):
    return math.fsum(float(a) * float(a) for a in x.astype(np.float64))


def _ref(w, g, m, v, ends, den=None, step=STEP, b2=B2, eps=EPS):
    """the records restated: float64 sums over the finite elements, the fp32 maximum, u in k_adam's fp32 operations (g, or m and v, None: zero fields)"""
    out, lo = [], 0
    bc2s = F(np.sqrt(1.0 - float(F(b2)) ** step))
    for hi in ends:
        gs = ga = gn = us = 0.0
        if g is not None:
            x = g[lo:hi]
            fin = np.isfinite(x)
            gn = int((~fin).sum())
            gs = _fsum_sq(x[fin])
            ga = F(np.abs(x[fin]).max()) if fin.any() else F(0)
            if den is not None:
                gs = gs / (float(F(den)) * float(F(den)))
                ga = ga / F(den)
        x = w[lo:hi]
        fin = np.isfinite(x)
        ws, wa = _fsum_sq(x[fin]), (F(np.abs(x[fin]).max()) if fin.any() else F(0))
        if m is not None:
            denom = np.sqrt(v[lo:hi]) / bc2s + F(eps)
            u = m[lo:hi] / denom
            assert u.dtype == F
            us = _fsum_sq(u)
        out.append(Rec(gs, ws, us, float(ga), float(wa), gn))
        lo = hi
    return out


def _call(L, hp, w, g, m, v, ends, den=None, step=STEP):
    nt = len(ends)
    out = (_lib.QpnTensorStat * nt)()
    _lib.check(L.qpn_tensor_stats(hp, w.data_ptr(), g.data_ptr() if g is not None else None, m.data_ptr() if m is not None else None,
                                  v.data_ptr() if v is not None else None, ends[-1], step, B1, B2, EPS, den.data_ptr() if den is not None else None,
                                  nt, (C.c_int64 * nt)(*ends), out, GC._stream()))
    return out


def _compare(out, ref):
    assert len(out) == len(ref)
    for t, (a, r) in enumerate(zip(out, ref)):
        for f in ("grad_sumsq", "weight_sumsq"):
            assert abs(getattr(a, f) - getattr(r, f)) <= 1e-12 * getattr(r, f), (t, f, getattr(a, f), getattr(r, f))
        assert abs(a.update_sumsq - r.update_sumsq) <= 2e-6 * r.update_sumsq, (t, a.update_sumsq, r.update_sumsq)
        assert (a.grad_absmax, a.weight_absmax, a.grad_nonfinite) == (r.grad_absmax, r.weight_absmax, r.grad_nonfinite), (t, a.grad_absmax, a.weight_absmax, a.grad_nonfinite, r)


@pytest.fixture(scope="module")
def arrs():
    """w, g, m, v by tests/test_grad_clip_gpu.py's recipe: made once, never written"""
    return GC._buffers(N, 4534)


@pytest.fixture(scope="module")
def handle(cuda):
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


CASES = list(itertools.product([False, True], [0, 1], [True, False], [True, False]))


@pytest.mark.parametrize("den,off,grad,moments", CASES, ids=["%s-off%d-%s-%s" % ("den" if c[0] else "noden", c[1], "g" if c[2] else "nog", "mv" if c[3] else "nomv") for c in CASES])
def test_c_abi_matrix_against_numpy(den, off, grad, moments, cuda, handle, arrs):
    import torch
    L, hp = handle
    w0, g0, m0, v0 = arrs
    gin = (g0 * F(DEN)).astype(F) if den else g0                       # an exchanged / accumulated buffer holds the SUM: den * g
    w, g, m, v = GC._dev(cuda, (w0, gin, m0, v0), off)
    dden = torch.tensor([DEN, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda) if den else None
    out = _call(L, hp, w, g if grad else None, m if moments else None, v if moments else None, ENDS, dden)
    ref = _ref(w0, gin if grad else None, m0 if moments else None, v0 if moments else None, ENDS, DEN if den else None)
    _compare(out, ref)
    if grad and moments:
        assert all(r.grad_sumsq > 0 and r.update_sumsq > 0 and r.grad_absmax > 0 for r in out)
    for t, a, inp in zip((w, g, m, v), (w0, gin, m0, v0), "wgmv"):     # the call only reads
        assert np.array_equal(t.cpu().numpy(), a), inp


def test_non_finite_values_are_counted_and_left_out(cuda, handle, arrs):
    """a NaN in a size-1 tensor, +inf in the last element of the multi-item tensor (and -inf among the weights of the 3-element one): the counts are 1 and 1, the
    other tensors report 0, every sum and maximum is that of the finite elements"""
    L, hp = handle
    w0, g0, m0, v0 = (a.copy() for a in arrs)
    g0[0] = np.nan
    g0[ENDS[5] - 1] = np.inf
    w0[ENDS[2]] = -np.inf
    w, g, m, v = GC._dev(cuda, (w0, g0, m0, v0), 0)
    out = _call(L, hp, w, g, m, v, ENDS)
    assert [r.grad_nonfinite for r in out] == [1, 0, 0, 0, 0, 1, 0]
    assert out[0].grad_sumsq == 0.0 and out[0].grad_absmax == 0.0
    assert all(math.isfinite(x) for r in out for x in (r.grad_sumsq, r.weight_sumsq, r.update_sumsq, r.grad_absmax, r.weight_absmax))
    _compare(out, _ref(w0, g0, m0, v0, ENDS))


def test_the_records_have_the_same_bits_from_run_to_run_and_at_any_alignment(cuda, handle, arrs):
    import torch
    L, hp = handle
    dden = torch.tensor([DEN, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda)
    bufs0, bufs1 = GC._dev(cuda, arrs, 0), GC._dev(cuda, arrs, 1)
    w, g, m, v = bufs0
    first = bytes(_call(L, hp, w, g, m, v, ENDS, dden))
    assert bytes(_call(L, hp, w, g, m, v, ENDS, dden)) == first
    w1, g1, m1, v1 = bufs1
    assert bytes(_call(L, hp, w1, g1, m1, v1, ENDS, dden)) == first
    assert bytes(_call(L, hp, w1, g, m1, v, ENDS, dden)) == first       # every buffer by its own alignment
    # another table on the same handle (the plan is replaced), then the first one again
    one = _call(L, hp, w, g, m, v, [N], dden)
    _compare(one, _ref(arrs[0], arrs[1], arrs[2], arrs[3], [N], DEN))
    assert bytes(_call(L, hp, w, g, m, v, ENDS, dden)) == first


# ---------------------------------------------------------------- the trainer
LR = 1e-3


def _model(cuda):
    return util.build_model(TINY, synth.make_weights(TINY, GC.WSEED), cuda).train()


def _snap(tr, m):
    return [t.detach().cpu().numpy().copy() for t in (m._flat, tr.m, tr.v)]


def _applied(m, cuda):
    L, hd = m._native(cuda)
    return GC._applied(L, hd)


def test_adam_launches_have_the_same_bits_with_the_call_between_them(cuda, arrs):
    """three clipping, averaging Adam launches through the C ABI on fixed gradients (the launches are bit-reproducible: tests/test_grad_clip_gpu.py), with
    qpn_tensor_stats behind each in one arm: weights, m, v, the average, the norms, the status and the applied-update count have the bits of the arm without it"""
    L = _lib.lib()
    w0, g0, m0, v0 = arrs
    grads = [g0, (g0[::-1] * F(1.5)).astype(F), (np.roll(g0, 7) * F(0.5)).astype(F)]
    arms = []
    for with_stats in (False, True):
        hp = C.c_void_p()
        _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
        try:
            w, m, v, e = GC._dev(cuda, (w0, m0, v0, w0), 0)
            norms = []
            for k, gk in enumerate(grads):
                g, = GC._dev(cuda, (gk,), 0)
                _lib.check(L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N, k + 1, GC.LR, B1, B2, EPS, GC.WD, None,
                                               0.5 * float(np.linalg.norm(g0)), e.data_ptr(), 0.9, GC._stream()))
                if with_stats:
                    _compare(_call(L, hp, w, g, m, v, ENDS, None, k + 1), _ref(w.cpu().numpy(), gk, m.cpu().numpy(), v.cpu().numpy(), ENDS, None, k + 1))
                norms.append(GC._norm(L, hp))
            applied = GC._applied(L, hp)
            assert L.qpn_train_status(hp, GC._stream()) == 0
            arms.append((norms, applied, [t.cpu().numpy() for t in (w, m, v, e)]))
        finally:
            L.qpn_destroy(hp)
    assert arms[0][0] == arms[1][0] and all(valid == 1 for _, valid in arms[0][0]) and arms[0][1] == arms[1][1] == 3
    for a, b in zip(arms[0][2], arms[1][2]):
        assert np.array_equal(a, b)


def test_tensor_stats_changes_nothing(cuda):
    """Three FusedTrainer steps (clipping, averaging) with tensor_stats() behind each.  Inside the run, bit for bit: the weights, m, v, the gradient buffer, the average,
    the applied-update count and the step count are the same bytes behind the call as in front of it, and the status stays clean.  Against three steps WITHOUT the
    call: the first loss and the counts are identical; the rest is held to the suite's bounds for two runs of the same steps -- the backward's float atomics (the
    upsampling bias, the adaptive blocks' scatter) make two runs of ONE chunk differ in the last bits whatever runs between them (tests/test_grad_accum_gpu.py,
    tests/test_runners_gpu.py: losses to 1e-6, weights to atol 2e-6), so bit equality between two trainer runs is not a property the step has to lose.  (Measured
    when this test was written: the first step's norm 0.0904526732586553 against 0.09045267322468584 in two plain arms' place.)"""
    from qpnet_amd.train import FusedTrainer
    runs = []
    for with_stats in (False, True):
        m = _model(cuda)
        tr = FusedTrainer(m, lr=LR, max_grad_norm=0.1, ema_decay=0.9)
        base, losses = None, []
        for k in range(3):
            losses.append((tr.step(*GC._chunk(cuda, k), want_loss=True), tr.last_grad_norm))
            if base is None:
                base = _applied(m, cuda) - 1
            if with_stats:
                before = [t.clone() for t in (m._flat, tr.m, tr.v, tr.g, tr.ema)] + [_applied(m, cuda), tr.step_count]
                s = tr.tensor_stats()
                assert len(s) == len(list(m.parameters()))
                tr.tensor_stats(weights="ema")
                after = [m._flat, tr.m, tr.v, tr.g, tr.ema, _applied(m, cuda), tr.step_count]
                for a, b in zip(before[:5], after[:5]):
                    assert a.data_ptr() != b.data_ptr() and torch_equal_bits(a, b)
                assert before[5:] == after[5:]
        tr.check_status()
        runs.append((losses, _applied(m, cuda) - base, tr.step_count, _snap(tr, m) + [tr.ema.cpu().numpy()]))
    assert runs[0][0][0][0] == runs[1][0][0][0]                       # the first loss: same weights, and the forward has no atomics
    for (la, na), (lb, nb) in zip(runs[0][0], runs[1][0]):
        assert abs(la - lb) < 1e-6 and abs(na - nb) <= 1e-6 * abs(na), (la, lb, na, nb)
    assert runs[0][1] == runs[1][1] == 3 and runs[0][2] == runs[1][2] == 3
    for a, b in zip(runs[0][3], runs[1][3]):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)


def torch_equal_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_against_numpy(stats, keys, ends, w, g, m, v, den, step, lrs):
    ref = _ref(w, g, m, v, ends, den, step)
    bc1 = F(1.0 - float(F(B1)) ** step)
    assert list(stats.keys()) == keys
    for key, r, lr in zip(keys, ref, lrs):
        s = stats[key]
        assert set(s) == {"grad_norm", "weight_norm", "update_norm", "update_ratio", "grad_absmax", "weight_absmax", "grad_nonfinite"}
        assert abs(s["grad_norm"] - math.sqrt(r.grad_sumsq)) <= 1e-12 * math.sqrt(r.grad_sumsq), key
        assert abs(s["weight_norm"] - math.sqrt(r.weight_sumsq)) <= 1e-12 * math.sqrt(r.weight_sumsq), key
        un = math.sqrt(r.update_sumsq) * float(F(lr) / bc1)
        assert abs(s["update_norm"] - un) <= 1e-6 * un, (key, s["update_norm"], un)      # (the square root halves update_sumsq's 2e-6)
        assert abs(s["update_ratio"] - un / math.sqrt(r.weight_sumsq)) <= 1e-6 * s["update_ratio"], key
        assert (s["grad_absmax"], s["weight_absmax"], s["grad_nonfinite"]) == (r.grad_absmax, r.weight_absmax, 0), key


def _layout(m):
    keys = list(m.state_dict().keys())
    ends = list(itertools.accumulate(p.numel() for p in m.parameters()))
    return keys, ends


def test_trainer_fields_match_numpy_and_the_weights_that_moved(cuda):
    from qpnet_amd.train import FusedTrainer
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR, max_grad_norm=0.1)
    with pytest.raises(RuntimeError, match="before the first update"):
        tr.tensor_stats()
    keys, ends = _layout(m)
    n = ends[-1]
    for k in range(2):
        before = m._flat.detach().cpu().numpy().copy() if getattr(m, "_flat", None) is not None else synth.make_weights(TINY, GC.WSEED)
        tr.step(*GC._chunk(cuda, k), want_loss=True)
        norm = tr.last_grad_norm
        stats = tr.tensor_stats()
        w, mm, vv = _snap(tr, m)
        g = tr.g[:n].cpu().numpy()
        _check_against_numpy(stats, keys, ends, w, g, mm, vv, None, k + 1, [LR] * len(keys))
        # clipping on (the first chunk's norm lies below the level, the second's above): the per-tensor sums add up to the norm the step clipped by
        total = math.fsum(s["grad_norm"] ** 2 for s in stats.values())
        assert norm > 0 and abs(total - norm * norm) <= 1e-12 * total, (total, norm * norm)
        # the reconstructed update against the weights that moved: w_after = fl(w_before - delta), each element good to ulp(max |w|) -- sqrt(numel) of them in the norm
        # (the residual 1x1 of the LAST layer feeds nothing: its gradient, its moments and its update are exact zeros -- and are reported as such)
        lo, still = 0, []
        for key, hi in zip(keys, ends):
            moved = float(np.linalg.norm(w[lo:hi].astype(np.float64) - before[lo:hi].astype(np.float64)))
            ulp = float(np.spacing(F(max(np.abs(w[lo:hi]).max(), np.abs(before[lo:hi]).max()))))
            bound = math.sqrt(hi - lo) * ulp
            assert abs(stats[key]["update_norm"] - moved) <= bound, (key, stats[key]["update_norm"], moved, bound)
            assert (stats[key]["update_norm"] > 0) == (moved > 0), (key, stats[key]["update_norm"], moved)
            if moved == 0:
                still.append(key)
            lo = hi
        assert "resA_1x1.0.weight" in still and all(key.startswith("resA_1x1.0.") for key in still), still
    tr.check_status()


def test_capturing_stream_raises(cuda, monkeypatch):
    import torch
    from qpnet_amd.train import FusedTrainer
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR)
    tr.step(*GC._chunk(cuda, 0), want_loss=True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        tr.tensor_stats()


def test_param_groups_frozen_and_scaled(cuda):
    """one frozen pattern, one lr_scale = 0.5: the frozen tensors report update_norm 0, the scaled ones half of what their m and v give at scale 1"""
    from qpnet_amd.train import FusedTrainer
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR, param_groups=[{"params": "causal.*", "frozen": True}, {"params": "conv_post_*", "lr_scale": 0.5}])
    w_before = synth.make_weights(TINY, GC.WSEED)
    tr.step(*GC._chunk(cuda, 0), want_loss=True)
    tr.check_status()
    stats = tr.tensor_stats()
    keys, ends = _layout(m)
    w, mm, vv = _snap(tr, m)
    ref = _ref(w, None, mm, vv, ends, None, 1)
    bc1 = F(1.0 - float(F(B1)))
    lo, seen = 0, collections.Counter()
    for key, hi, r in zip(keys, ends, ref):
        full = math.sqrt(r.update_sumsq) * float(F(LR) / bc1)
        moved = float(np.linalg.norm(w[lo:hi].astype(np.float64) - w_before[lo:hi].astype(np.float64)))
        if key.startswith("causal."):
            assert stats[key]["update_norm"] == 0.0 and stats[key]["update_ratio"] == 0.0 and moved == 0.0 and stats[key]["grad_norm"] > 0, key
            seen["frozen"] += 1
        elif key.startswith("conv_post_"):
            assert full > 0 and abs(stats[key]["update_norm"] - 0.5 * full) <= 1e-6 * full, (key, stats[key]["update_norm"], full)
            assert abs(moved - 0.5 * full) <= 0.01 * full, (key, moved, full)      # (and that is what moved: far from `full`)
            seen["scaled"] += 1
        else:
            assert abs(stats[key]["update_norm"] - full) <= 1e-6 * full, key
        lo = hi
    assert seen == {"frozen": 2, "scaled": 4}


def test_accumulation_window(cuda):
    """accum_steps = 2: a call inside the window raises; behind the closing micro-step the gradient fields are those of the accumulator over its summed row count"""
    from qpnet_amd.train import FusedTrainer
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR, accum_steps=2)
    tr.step(*GC._chunk(cuda, 0), want_loss=True)
    assert tr.micro_step == 1
    with pytest.raises(RuntimeError, match="before the first update|accumulation window"):
        tr.tensor_stats()
    tr.step(*GC._chunk(cuda, 1), want_loss=True)
    assert tr.micro_step == 0 and tr.step_count == 1
    stats = tr.tensor_stats()
    keys, ends = _layout(m)
    n = ends[-1]
    acc = tr.acc.cpu().numpy()
    assert acc[n] == sum(int(GC._chunk(cuda, k)[4][0]) for k in range(2)) and acc[n + 1] == 0        # the trailer: the window's summed row count (batch size 1), no flag
    w, mm, vv = _snap(tr, m)
    _check_against_numpy(stats, keys, ends, w, acc[:n], mm, vv, float(acc[n]), 1, [LR] * len(keys))
    # a window that has closed once and is open again
    tr.step(*GC._chunk(cuda, 2), want_loss=True)
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.tensor_stats()
    tr.step(*GC._chunk(cuda, 3), want_loss=True)
    tr.check_status()


def test_ema_weights_and_flat_adam(cuda):
    """weights="ema" reports the average's norms (everything else unchanged); FlatAdam.tensor_stats describes its own latest step from p.grad"""
    import torch
    from qpnet_amd.train import FusedTrainer, FlatAdam
    m = _model(cuda)
    tr = FusedTrainer(m, lr=LR, ema_decay=0.5)
    with pytest.raises(RuntimeError, match="ema_decay is off"):
        FusedTrainer(_model(cuda), lr=LR).tensor_stats(weights="ema")
    for k in range(2):
        tr.step(*GC._chunk(cuda, k), want_loss=True)
    keys, ends = _layout(m)
    live, avg = tr.tensor_stats(), tr.tensor_stats(weights="ema")
    e = tr.ema.cpu().numpy()
    ref = _ref(e, None, None, None, ends)
    for key, r in zip(keys, ref):
        assert abs(avg[key]["weight_norm"] - math.sqrt(r.weight_sumsq)) <= 1e-12 * avg[key]["weight_norm"] and avg[key]["weight_absmax"] == r.weight_absmax, key
        assert avg[key]["grad_norm"] == live[key]["grad_norm"] and avg[key]["update_norm"] == live[key]["update_norm"], key
    assert any(avg[k]["weight_norm"] != live[k]["weight_norm"] for k in keys)
    # FlatAdam: the reference-style loop
    m2 = _model(cuda)
    opt = FlatAdam(m2, lr=LR)
    with pytest.raises(RuntimeError, match="before the first update"):
        opt.tensor_stats()
    xt, ht, tt, dt, bt = GC._chunk(cuda, 0)
    out = m2(xt, ht, dt, bt)
    loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, TINY.n_quantize), tt[:, -out.shape[1]:].reshape(-1))
    loss.backward()
    opt.step()
    stats = opt.tensor_stats()
    g = torch.cat([p.grad.reshape(-1) for p in m2.parameters()]).cpu().numpy()
    _check_against_numpy(stats, keys, ends, m2._flat.detach().cpu().numpy(), g, opt._m.cpu().numpy(), opt._v.cpu().numpy(), None, 1, [LR] * len(keys))


# ---------------------------------------------------------------- the runner
def test_run_train_writes_the_report_only_when_asked(cuda, tmp_path, caplog):
    """run_train --iters 4 --stats_interval 2: tensor_stats.jsonl has two lines, every key, all values finite; without the flag the file is not written and the
    model configuration and the final weights are those of the run with it"""
    import torch
    from qpnet_amd import loaders, runners
    from scipy.io import wavfile
    # (the corpus and geometry of tests/test_runners_gpu.py's smallest case)
    root = str(tmp_path / "corpus")
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    rs = np.random.RandomState(5)
    feats = []
    for i in range(3):
        h = synth.make_features(45 + 3 * i, 700 + i)
        wavfile.write("%s/wav/u%02d.wav" % (root, i), 22050, (rs.uniform(-0.8, 0.8, (45 + 3 * i) * TINY.upsampling_factor + 11) * 32767).astype(np.int16))
        np.save("%s/feat/u%02d.npy" % (root, i), h)
        feats.append(h)
    st = loaders.calc_stats(feats)
    np.savez(root + "/stats.npz", mean=st.mean_, scale=st.scale_)
    geo = ["--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2", "--dilationF_repeat", "1", "--dilationA_depth", "1",
           "--dilationA_repeat", "1", "--feature_format", "npy", "--batch_length", "1500", "--max_length", "4000", "--verbose", "1"]
    finals, confs = [], []
    for tag, extra in (("stats", ["--stats_interval", "2"]), ("plain", [])):
        exp = str(tmp_path / tag)
        os.makedirs(exp)
        with caplog.at_level(logging.INFO):
            args = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz"] + geo + \
                   ["--expdir", exp, "--config", exp + "/model.conf", "--iters", "4", "--checkpoint_interval", "100", "--intervals", "4", "--resume", exp + "/none.pkl"] + extra
            assert runners.run_train(args) == 0
        sd = torch.load(exp + "/checkpoint-final.pkl", map_location="cpu")["model"]
        finals.append(torch.cat([v.reshape(-1).float() for v in sd.values()]))
        confs.append({k: v for k, v in vars(loaders.load_model_conf(exp + "/model.conf")).items() if k not in ("expdir", "config", "resume")})
        keys = list(sd.keys())
    path = str(tmp_path / "stats" / "tensor_stats.jsonl")
    with open(path) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["iter"] for ln in lines] == [2, 4]
    for ln in lines:
        assert list(ln["tensors"].keys()) == keys
        for key, s in ln["tensors"].items():
            assert set(s) == {"grad_norm", "weight_norm", "update_norm", "update_ratio", "grad_absmax", "weight_absmax", "grad_nonfinite"}
            # (the last layer's residual 1x1 feeds nothing: its gradient and its update are exact zeros, and its bias is still the zeros it was initialised with)
            assert all(math.isfinite(x) for x in s.values()) and s["grad_nonfinite"] == 0, (key, s)
            assert (s["weight_norm"] > 0 and s["update_norm"] > 0 and s["grad_norm"] > 0) or key.startswith("resA_1x1.0."), (key, s)
    assert sorted(os.listdir(str(tmp_path / "plain"))) == sorted(set(os.listdir(str(tmp_path / "stats"))) - {"tensor_stats.jsonl"})
    assert "stats_interval" not in confs[0] and confs[0] == confs[1]
    np.testing.assert_allclose(finals[0].numpy(), finals[1].numpy(), rtol=0, atol=2e-6)      # (two runs of the same steps: float-atomics order inside a step, tests/test_runners_gpu.py's bound)
