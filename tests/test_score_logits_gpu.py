"""GPU: qpn_score_logits on synthetic logits against the float64 specification (tests/score_spec.py), against qpn_ce_loss on the same buffers, and on a
non-blocking stream behind a late copy of its inputs (the pattern of tests/test_streams_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY
import score_spec as SP
from test_streams_gpu import _Late, _start, _still_closed, gate      # noqa: F401  (gate: the module-scoped fixture, calibrated once here too)

pytestmark = pytest.mark.gpu

F = np.float32
QS = [256, 64, 100, 512, 2048]          # the vector path in one pass, a partly filled pass, a non-multiple of 64, two register passes, the re-read path
SHAPES = [(1, 1, 1), (1, 5, 5), (2, 37, 50), (1, 263, 263)]      # (B, BL, tgt_stride): a partly filled workgroup, the (b, t) split with a stride, a tail


def _score(cuda, lg, tg):
    """train.score_logits on host arrays -> host arrays"""
    import torch
    from qpnet_amd import train
    s = train.score_logits(torch.from_numpy(lg).to(cuda), torch.from_numpy(tg).to(cuda))
    assert [a.dtype for a in s] == [torch.float32, torch.float32, torch.int32, torch.int32]
    assert all(tuple(a.shape) == lg.shape[:2] for a in s)
    assert s.nll.data_ptr() + 4 == s.entropy.data_ptr() and s.nll.data_ptr() + 12 == s.rank.data_ptr() and s.nll.stride() == (4 * lg.shape[1], 4)      # views of one record buffer
    return tuple(a.cpu().numpy() for a in s)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_stride%d" % s for s in SHAPES])
@pytest.mark.parametrize("Q", QS)
def test_random_logits_against_the_spec(Q, shape, cuda):
    B, BL, stride = shape
    rs = np.random.RandomState(1000 * Q + BL)
    lg = (3.0 * rs.standard_normal((B, BL, Q))).astype(F)
    tg = rs.randint(0, Q, (B, stride)).astype(np.int64)
    nll, ent, am, rk = _score(cuda, lg, tg)
    w_nll, w_ent, w_am, w_rk = SP.score(lg, tg[:, stride - BL:])
    np.testing.assert_array_equal(am, w_am)
    np.testing.assert_array_equal(rk, w_rk)
    err_n, err_e = np.abs(nll - w_nll).max(), np.abs(ent - w_ent).max()
    print("SCORE_LOGITS Q=%d %s: max |nll - spec| %.3e, max |entropy - spec| %.3e" % (Q, shape, err_n, err_e))
    assert err_n <= 1e-4 and err_e <= 1e-4


def _hand_rows(Q):
    """rows whose answers are known, and their targets; rows 9 and 10 carry the out-of-range targets, between ordinary rows"""
    rs = np.random.RandomState(Q)
    base = (2.0 * rs.standard_normal(Q)).astype(F)
    hi = F(np.abs(base).max() + 1.5)
    rows, tg = [], []
    a, b = 3, Q - 2
    r = base.copy(); r[a] = r[b] = hi; rows.append(r); tg.append(b)                    # 0: two-way tie at the top, target = the later one
    r = base.copy(); r[a] = r[b] = hi; rows.append(r); tg.append(a)                    # 1: ... target = the earlier one
    r = base.copy(); r[a] = r[b] = hi; rows.append(r); tg.append(7)                    # 2: ... target below both
    rows.append(np.full(Q, F(1.25))); tg.append(Q // 2)                                 # 3: all equal
    rows.append(np.zeros(Q, F)); tg.append(Q - 1)                                       # 4: all equal (zeros)
    r = np.full(Q, F(-80.0)); r[Q // 3] = F(80.0); rows.append(r); tg.append(Q // 3)    # 5: peaked, target = the peak
    r = np.full(Q, F(-80.0)); r[Q // 3] = F(80.0); rows.append(r); tg.append(0)         # 6: peaked, target elsewhere
    r = base.copy(); r[::2] = -np.inf; rows.append(r); tg.append(1)                     # 7: half the classes at -inf, target finite
    r = base.copy(); r[1::2] = -np.inf; rows.append(r); tg.append(1)                    # 8: ... target at -inf
    rows.append(base.copy()); tg.append(-1)                                             # 9: target below the range
    rows.append(base[::-1].copy()); tg.append(Q)                                        # 10: target above the range
    rows.append(base.copy()); tg.append(5)                                              # 11: an ordinary row behind them
    return np.stack(rows)[None], np.array(tg, dtype=np.int64)[None]


@pytest.mark.parametrize("Q", [256, 100])
def test_hand_made_rows(Q, cuda):
    lg, tg = _hand_rows(Q)
    nll, ent, am, rk = (a[0] for a in _score(cuda, lg, tg))
    w_nll, w_ent, w_am, w_rk = (a[0] for a in SP.score(lg, tg))
    np.testing.assert_array_equal(am, w_am)
    np.testing.assert_array_equal(rk, w_rk)
    # ties: the lowest index wins; a tied-top target has nothing above it
    assert am[0] == am[1] == am[2] == 3 and rk[0] == rk[1] == 0 and rk[2] >= 2
    for i in (3, 4):
        assert am[i] == 0 and rk[i] == 0 and abs(nll[i] - np.log(Q)) <= 1e-5 and abs(ent[i] - np.log(Q)) <= 1e-5, (i, nll[i], ent[i])
    # peaked: finite, entropy below 1e-6
    assert np.isfinite(nll[5:7]).all() and np.isfinite(ent[5:7]).all() and (ent[5:7] < 1e-6).all() and (ent[5:7] >= 0).all()
    assert abs(nll[5]) <= 1e-6 and abs(nll[6] - 160.0) <= 1e-4 and rk[5] == 0 and rk[6] == 1 and am[5] == am[6] == Q // 3
    # -inf classes: finite and the spec's; a target AT -inf has an infinite nll and every finite class above it
    assert np.isfinite([nll[7], ent[7], ent[8]]).all() and nll[8] == np.inf and rk[8] == Q // 2
    fin = [0, 1, 2, 3, 4, 5, 6, 7, 11]
    np.testing.assert_allclose(nll[fin], w_nll[fin], atol=1e-4, rtol=0)
    np.testing.assert_allclose(ent, w_ent, atol=1e-4, rtol=0)
    # out-of-range targets: nll = +inf, rank = Q, argmax and entropy still the row's; the neighbours untouched
    for i in (9, 10):
        assert nll[i] == np.inf and rk[i] == Q and am[i] == w_am[i] and abs(ent[i] - w_ent[i]) <= 1e-4
    assert np.isfinite(nll[11]) and rk[11] == w_rk[11] and abs(nll[11] - w_nll[11]) <= 1e-4


@pytest.mark.parametrize("Q", [256, 100, 112])
def test_sum_of_nll_is_the_loss_qpn_ce_loss_reports(Q, cuda):
    """the scorer's per-row arithmetic is k_ce's: only the float64 reassociation of 600 terms separates the two.  qpn_ce_loss takes Q from its handle, and
    the training state of a handle refuses an n_quantize that is no multiple of 16: at Q = 100 there is no library loss to compare with (that refusal is
    what the case pins); Q = 112 is the scalar path (no multiple of 64 or 256) at a width the handle takes."""
    import dataclasses
    import torch
    B, BL, pad = 2, 300, 3
    rs = np.random.RandomState(31 + Q)
    lg = torch.from_numpy((3.0 * rs.standard_normal((B, BL, Q))).astype(F)).to(cuda)
    tg = torch.from_numpy(rs.randint(0, Q, (B, pad + BL)).astype(np.int64)).to(cuda)
    from qpnet_amd import train
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(dataclasses.replace(TINY, n_quantize=Q))), C.byref(hp)))
    try:
        loss = C.c_double(0.0)
        rc = L.qpn_ce_loss(hp, lg.data_ptr(), tg.data_ptr(), tg.shape[1], B, BL, None, C.byref(loss), torch.cuda.current_stream(cuda).cuda_stream)
        if Q % 16:
            assert rc == -1 and b"multiples of 16" in L.qpn_last_error(), (rc, L.qpn_last_error())
            s = train.score_logits(lg, tg)                       # (the scorer itself takes the width: against the spec in the tests above)
            assert bool(torch.isfinite(s.nll).all())
            return
        _lib.check(rc)
        s = train.score_logits(lg, tg)
        mine = float(s.nll.double().sum()) / (B * BL)
    finally:
        L.qpn_destroy(hp)
    print("SCORE_LOGITS Q=%d: sum nll / rows %.15f, qpn_ce_loss %.15f" % (Q, mine, loss.value))
    assert abs(mine - loss.value) <= 1e-9 * abs(loss.value)


def test_score_logits_with_late_logits_and_targets(cuda, gate):
    import torch
    B, BL, Q, pad = 2, 37, 256, 3
    rs = np.random.RandomState(99)
    lg, dlg = (3.0 * rs.standard_normal((B, BL, Q))).astype(F), (3.0 * rs.standard_normal((B, BL, Q))).astype(F)
    t, dt = rs.randint(0, Q, (B, pad + BL)).astype(np.int64), rs.randint(0, Q, (B, pad + BL)).astype(np.int64)
    want = SP.score(lg, t[:, pad:])
    for a, b in ((dlg, dt), (dlg, t), (lg, dt)):                    # teeth: the decoy, and either input alone the decoy's, give other records
        other = SP.score(a, b[:, pad:])
        assert (other[3] != want[3]).mean() >= 0.5 and np.abs(other[0] - want[0]).mean() >= 100 * 1e-4
    late = _Late(cuda, (lg, t), (dlg, dt))
    lb, tb = late.buf
    L = _lib.lib()
    out = torch.full((B, BL, 4), float("nan"), device=cuda)
    scratch = out.clone()
    _lib.check(L.qpn_score_logits(lb.data_ptr(), tb.data_ptr(), tb.shape[1], B, BL, Q, scratch.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream))      # (set-up: the code object)
    s = _start(cuda)
    with torch.cuda.stream(s):
        late.deliver(gate)
        _lib.check(L.qpn_score_logits(lb.data_ptr(), tb.data_ptr(), tb.shape[1], B, BL, Q, out.data_ptr(), s.cuda_stream))
        _still_closed(s, "qpn_score_logits")
        got = out.clone()
    s.synchronize()
    got = got.cpu()
    ints = got.view(torch.int32).numpy()
    np.testing.assert_array_equal(ints[..., 2], want[2])
    np.testing.assert_array_equal(ints[..., 3], want[3])
    np.testing.assert_allclose(got.numpy()[..., 0], want[0], atol=1e-4, rtol=0)
    np.testing.assert_allclose(got.numpy()[..., 1], want[1], atol=1e-4, rtol=0)
