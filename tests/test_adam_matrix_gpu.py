"""GPU: every instance of the Adam kernel through ONE call (qpn_adam_step_avg) on one small shape -- clip x averaged weights x parameter groups, crossed with the
denominator buffer (absent, clean, flagged by a peer) and the base alignment.

n = 2051 is the smallest shape on which all of this happens at once: three workgroups of a grouped launch, the last with 3 elements and three padded pairs;
n % 4 == 3 (the tail of the sum of squares); more than one 256-element block per workgroup.  The group table puts a segment boundary into blocks 1, 3 and 4
(block 4 is the first block of the second workgroup) and freezes block 2 as a whole.

Expected values are the suite's own numpy restatements, compared the way their own tests compare them: without groups tests/test_grad_clip_gpu.py's _ref_adam
within its bounds and tests/test_ema_gpu.py's _ema_ref from the device's own new weights within its bound; with groups tests/test_adam_groups_gpu.py's
per-element form, bit for bit (the averaged weights too: its line restated from the expected new weights)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY
import test_adam_groups_gpu as GR
import test_ema_gpu as EM
import test_grad_clip_gpu as GC

pytestmark = pytest.mark.gpu

F = np.float32
N = 2051
ENDS, GROUPS = [300, 1000, 1030, 2051], [0, GR.FR, 1, 2]
DECAY = 0.9
MIXED = "mixed"


def _block_kinds(ends, groups):
    """adam_groups_build()'s per-block verdict restated: the group of a 256-element block that lies inside one segment, MIXED where a boundary crosses it"""
    seg = np.repeat(np.arange(len(ends)), np.diff([0] + list(ends)))
    return [groups[seg[b]] if seg[b] == seg[min(b + 256, ends[-1]) - 1] else MIXED for b in range(0, ends[-1], 256)]


def test_the_table_has_the_block_kinds_the_cases_rely_on():
    kinds = _block_kinds(ENDS, GROUPS)
    assert kinds == [0, MIXED, GR.FR, MIXED, MIXED, 2, 2, 2, 2]
    assert N % 4 == 3 and N - 8 * 256 == 3                    # the sum of squares' short last quad; 3 elements in the last block ...
    assert -(-len(kinds) // 4) == 3 and 3 * 4 - len(kinds) == 3      # ... of the third workgroup, whose other three pairs are padding
    assert 256 * 4 < ENDS[2] < 256 * 5                         # a boundary inside the first block of the second workgroup
    q = GR._per_elem(ENDS, GROUPS)[0]
    assert set(q.tolist()) == {GR.FR, 0, 1, 2}


@pytest.fixture(scope="module")
def handle(cuda):
    """one TINY handle; a clipping call first: it creates the handle's training state, where the status word and the applied-update count live"""
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    w, g, m, v = GC._dev(cuda, GC._buffers(8, 1), 0)
    GC._clip_call(L, hp, w, g, m, v, 8, 1.0)
    assert L.qpn_train_status(hp, GC._stream()) == 0
    yield L, hp
    L.qpn_destroy(hp)


@pytest.fixture(scope="module")
def arrs():
    """w, g, m, v by tests/test_grad_clip_gpu.py's recipe and an independent e: made once, never written"""
    return GC._buffers(N, 2051) + ((np.random.RandomState(52051).standard_normal(N) * 0.1).astype(F),)


CASES = list(itertools.product([False, True], [False, True], [False, True], ["none", "clean", "flagged"], [0, 1]))


@pytest.mark.parametrize("clip,avg,grouped,den,off", CASES, ids=["%s-%s-%s-den_%s-off%d" % ("clip" if c[0] else "noclip", "ema" if c[1] else "noema", "grp" if c[2] else "nogrp",
                                                                                            c[3], c[4]) for c in CASES])
def test_every_instance_against_numpy(clip, avg, grouped, den, off, cuda, handle, arrs):
    import torch
    L, hp = handle
    w0, g0, m0, v0, e0 = arrs
    q, lr, wd = GR._per_elem(ENDS, GROUPS)
    live = q >= 0 if grouped else np.ones(N, bool)
    dval = None if den == "none" else 3.0
    gin = g0 if dval is None else (g0 * F(dval)).astype(F)             # the exchanged buffer holds the SUM: den * g
    dden = None if dval is None else torch.tensor([dval, 1.0 if den == "flagged" else 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda)
    unfrozen = float(np.sqrt((np.where(q >= 0, g0, 0).astype(np.float64) ** 2).sum()))
    total = float(np.sqrt((np.where(live, gin, 0).astype(np.float64) ** 2).sum())) / (dval or 1.0)      # what the launch sees
    max_norm = 0.5 * unfrozen if clip else 0.0
    w, g, m, v, e = GC._dev(cuda, (w0, gin, m0, v0, e0), off)
    if grouped:
        GR._set(L, hp, ENDS, GROUPS)
    try:
        before = GC._applied(L, hp)
        _lib.check(L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N, GC.STEP, GC.LR, GC.B1, GC.B2, GC.EPS, GC.WD,
                                       dden.data_ptr() if dden is not None else None, max_norm, e.data_ptr() if avg else None, DECAY if avg else 0.0, GC._stream()))
        norm, valid = GC._norm(L, hp)
        applied = GC._applied(L, hp)
        status = L.qpn_train_status(hp, GC._stream())
        msg = L.qpn_last_error()
    finally:
        if grouped:
            GR._off(L, hp)
    wg, gg, mg, vg, eg = (t.cpu().numpy() for t in (w, g, m, v, e))
    assert np.array_equal(gg, gin)                                     # the gradient buffer is never written
    assert valid == (1 if clip else 0)
    if clip:
        np.testing.assert_allclose(norm, total, rtol=1e-6 if (dval or grouped) else 1e-7, atol=0)
    if den == "flagged":                                               # a peer's flag: nothing moves, nothing is counted, the error is reported once
        for t, a in zip((w, m, v, e), (w0, m0, v0, e0)):
            assert torch.equal(t, torch.from_numpy(np.array(a)).to(cuda))
        assert applied == before
        assert status == -4 and b"peer rank" in msg
        assert L.qpn_train_status(hp, GC._stream()) == 0
        return
    assert status == 0 and applied == before + 1
    if not avg:
        assert np.array_equal(eg, e0)
    if grouped:
        coef = GR._coef(norm, max_norm) if clip else 1.0
        assert (coef < 0.51) if clip else True
        wr, mr, vr = GR._ref_adam(w0, gin, m0, v0, lr, wd, coef, dval, step=GC.STEP)
        wr, mr, vr = np.where(live, wr, w0), np.where(live, mr, m0), np.where(live, vr, v0)
        for what, a, r, inp in zip("wmv", (wg, mg, vg), (wr, mr, vr), (w0, m0, v0)):
            assert np.array_equal(a, r), "%s: %d elements differ, first at %d" % (what, (a != r).sum(), int(np.argmax(a != r)))
            assert np.array_equal(a[~live], inp[~live]) and (a[live] != inp[live]).mean() > 0.99, what
        if avg:
            assert np.array_equal(eg, EM._ema_ref(wr, e0, DECAY)[0])     # (frozen elements: towards the weight that stays)
            assert (eg != e0).mean() > 0.99
    else:
        geff = gin if dval is None else gin / F(dval)
        coef = GC._coef(total, max_norm) if clip else F(1.0)
        assert (coef < 0.51) if clip else True
        wr, mr, vr = GC._ref_adam(w0, geff, m0, v0, coef)
        np.testing.assert_allclose(wg, wr, rtol=0, atol=2e-6)
        np.testing.assert_allclose(mg, mr, rtol=0, atol=1e-5 * np.abs(mr).max())
        np.testing.assert_allclose(vg, vr, rtol=0, atol=4e-5 * np.abs(vr).max())
        assert not np.array_equal(wg, w0)
        if avg:
            r, bound = EM._ema_ref(wg, e0, DECAY)
            err = np.abs(eg.astype(np.float64) - r.astype(np.float64))
            assert (err <= bound).all()
            assert (np.abs(eg.astype(np.float64) - e0.astype(np.float64)) > 100 * bound).any()
