"""CPU: sampling at n_quantize up to 1024 (Q = 64 * per, per up to 16) -- the numpy restatement of the draw for any `per` (tests/wide_draw_spec.py) against
the two restatements that stop at per = 4, against the C oracle's own sampled streams at 320, 512 and 1024 classes, and against the distribution it claims to
draw from; and the argument checks of the C ABI and of the Python surface at those class counts, none of which needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import nucleus_spec as NS
import sampling_spec as SS
import wide_draw_spec as WS
import wide_quantize_common as WQ
from qpnet_amd import _lib
from test_sampling_controls_cpu import _merged_chi2
from test_sampling_controls_gpu import _families

F32 = np.float32
SEED = 0x9E3779B97F4A7C15
EINVAL, OK = -1, 0
CONTROLS = [(1.0, 0, 1.0, 0.0), (0.7, 40, 1.0, 0.0), (1.5, 5, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (0.7, 40, 0.9, 0.01), (1.3, 63, 0.5, 0.05), (0.01, 0, 0.999, 1e-4),
            (100.0, 7, 0.1, 0.0), (1.0, 1, 1.0, 0.0), (1.0, 0, 1e-30, 0.0), (1.0, 0, 1.0, 1.0)]


@pytest.mark.parametrize("Q", [64, 128, 192, 256])
def test_restatement_equals_the_narrow_specs_bit_for_bit(Q, oracle):
    """per <= 4: sampling_spec.draw (temperature, top_k) and nucleus_spec.draw (all four) on random rows and on the crafted families of their GPU tests."""
    rs = np.random.RandomState(500 + Q)
    fams = _families(Q, 12, rs)
    fams["tied"] = NS.tied_rows(Q, 12, rs)
    fams["flat"] = (0.05 * rs.standard_normal((12, Q))).astype(F32)
    names = sorted(fams)
    rows = np.concatenate([fams[f] for f in names])
    n = 0
    for ci, (T, k, top_p, min_p) in enumerate(CONTROLS):
        k = min(k, Q)
        u = SS.uniforms(SEED, 2, range(1000 * ci, 1000 * ci + len(rows)))
        got = WS.draw(rows, u, T, k, top_p, min_p)
        np.testing.assert_array_equal(got, NS.draw(rows, u, T, k, top_p, min_p), err_msg="Q=%d T=%g k=%d top_p=%g min_p=%g" % (Q, T, k, top_p, min_p))
        if top_p == 1.0 and min_p == 0.0:
            np.testing.assert_array_equal(got, SS.draw(rows, u, T, k), err_msg="Q=%d T=%g k=%d" % (Q, T, k))
        if (T, k, top_p, min_p) == (1.0, 0, 1.0, 0.0):
            np.testing.assert_array_equal(WS.default_draw(rows, u), got)
        n += len(rows)
    assert n == len(CONTROLS) * 12 * len(names)


@pytest.mark.parametrize("csq", WQ.WIDTHS, ids=WQ.IDS)
def test_restatement_reproduces_the_oracle_stream_beyond_256_classes(csq, oracle):
    """The oracle's sample_spec is written for per = Q / 64 classes per lane: its sampled stream of row 1 (329 samples) at 320, 512 and 1024 classes is what
    the restatement draws from the run's own logits, through the default draw and through the controlled one at neutral values.  The streams are no
    degenerate ones: at least 128 distinct classes, at least 32 picks beyond class 255 (the oracle alone gives 200 / 74 at the least)."""
    r = WQ.oracle_stream(csq)
    Q = csq[2]
    y, lg = r["samples"], r["logits"]
    assert lg.shape == (329, Q) and y.shape == (329,)
    distinct, high = len(np.unique(y)), int((y >= 256).sum())
    print("oracle stream at (C, S, Q) = %s: %d distinct classes, %d picks >= 256, largest %d" % (csq, distinct, high, y.max()))
    assert distinct >= 128 and high >= 32
    u = SS.uniforms(WQ.SEED, WQ.ROW, range(len(y)))
    np.testing.assert_array_equal(WS.default_draw(lg, u), y)
    np.testing.assert_array_equal(WS.draw_steps(lg, WQ.SEED, WQ.ROW), y)
    np.testing.assert_array_equal(WS.draw_steps(lg, WQ.SEED, WQ.ROW, temperature=1.0, top_k=Q), y)


def test_restated_draw_follows_the_tempered_truncated_softmax_at_1024_classes(oracle):
    """40 000 draws over the step counter from one fixed 1024-logit row, T = 0.7, k = 100: none outside the kept set, and the counts pass a chi-square test
    against softmax(l / T) renormalised over the kept set in float64 (99.9 % quantile; fixed seed, so the test is deterministic)."""
    from scipy.stats import chi2
    Q, N, T, k = 1024, 40000, 0.7, 100
    l = (2.0 * np.random.RandomState(1234).standard_normal(Q)).astype(F32)
    keep = SS.kept_set(l, k)[0]
    assert keep.sum() == k and keep[256:].sum() >= 32          # (distinct logits: no ties; the kept set reaches past class 255)
    u = SS.uniforms(20241019, 3, range(N))
    picks = np.concatenate([WS.draw(np.broadcast_to(l, (len(c), Q)), c, T, k) for c in np.array_split(u, 8)])
    counts = np.bincount(picks, minlength=Q)
    assert counts[~keep].sum() == 0, "draws outside the kept set: classes %s" % np.nonzero(counts * ~keep)[0]
    z = l.astype(np.float64)[keep] / T
    p = np.exp(z - z.max()); p /= p.sum()
    x2, df = _merged_chi2(counts[keep], N * p)
    bound = chi2.ppf(0.999, df)
    print("Q=1024 T=%g k=%d: chi2 %.1f, df %d (chi2/df %.2f), 99.9 %% quantile %.1f" % (T, k, x2, df, x2 / df, bound))
    assert df >= 3 and x2 <= bound


# ---------------------------------------------------------------- the ABI and the Python surface, without a device
def test_stand_alone_draw_takes_the_class_counts_up_to_1024():
    """qpn_sample_logits_ex checks Q, then the controls, then its pointers, then looks for a device: null pointers say how far a call got."""
    L = _lib.lib()
    for Q in (320, 512, 1024):
        assert L.qpn_sample_logits_ex(None, 1, Q, 0, 0, 0, 1.0, 0, 1.0, 0.0, None, None) == EINVAL and b"bad arguments" in L.qpn_last_error(), Q
        assert L.qpn_sample_logits(None, 1, Q, 0, 0, 0, 0.7, 65, None, None) == EINVAL and b"bad arguments" in L.qpn_last_error(), Q
    for Q in (0, 96, 1088, 2048):
        assert L.qpn_sample_logits_ex(None, 1, Q, 0, 0, 0, 1.0, 0, 1.0, 0.0, None, None) == EINVAL and b"n_quantize" in L.qpn_last_error(), Q
        assert b"1024" in L.qpn_last_error()                   # (the message names the set)
    assert L.qpn_sample_logits_ex(None, 1, 1024, 0, 0, 0, 1.0, 1024, 1.0, 0.0, None, None) == EINVAL and b"bad arguments" in L.qpn_last_error()
    assert L.qpn_sample_logits_ex(None, 1, 1024, 0, 0, 0, 1.0, 1025, 1.0, 0.0, None, None) == EINVAL and b"top_k" in L.qpn_last_error()
    assert L.qpn_sample_logits_ex(None, 1, 512, 0, 0, 0, 1.0, 513, 1.0, 0.0, None, None) == EINVAL and b"top_k" in L.qpn_last_error()


def test_decode_setters_bound_top_k_by_the_handles_class_count():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(WQ.cfg_of((64, 64, 512)))), C.byref(hp)) == OK      # (without a GPU: a geometry-only handle)
    try:
        assert L.qpn_decode_sampling(hp, 1.0, 512) == OK and L.qpn_decode_sampling(hp, 0.7, 300) == OK
        assert L.qpn_decode_sampling_ex(hp, 0.7, 511, 0.9, 0.01) == OK
        assert L.qpn_decode_sampling(hp, 1.0, 513) == EINVAL and b"top_k" in L.qpn_last_error() and b"512" in L.qpn_last_error()
        rows = (_lib.QpnRowDraw * 2)(_lib.QpnRowDraw(1, 0, 1.0, 512, 1.0, 0.0), _lib.QpnRowDraw(2, 0, 0.7, 300, 0.9, 0.01))
        assert L.qpn_decode_row_sampling(hp, 2, rows) == OK
        rows[1].top_k = 513
        assert L.qpn_decode_row_sampling(hp, 2, rows) == EINVAL and b"top_k" in L.qpn_last_error()
        assert L.qpn_decode_row_sampling(hp, 0, None) == OK
        track = (_lib.QpnFrameDraw * 3)(_lib.QpnFrameDraw(1.0, 512, 1.0, 0.0), _lib.QpnFrameDraw(0.7, 300, 0.9, 0.01), _lib.QpnFrameDraw(1.3, 0, 1.0, 0.0))
        assert L.qpn_decode_frame_sampling(hp, 1, 3, track) == OK
        track[2].top_k = 513
        assert L.qpn_decode_frame_sampling(hp, 1, 3, track) == EINVAL and b"top_k" in L.qpn_last_error()
        assert L.qpn_decode_frame_sampling(hp, 0, 0, None) == OK
    finally:
        L.qpn_destroy(hp)


def test_python_surface_takes_top_k_up_to_the_class_count():
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**WQ.cfg_of((64, 64, 512)).kwargs())
    assert m._sampling_controls("sampling", 1.0, 300)[:2] == (1.0, 300)
    assert m._sampling_controls("sampling", 0.7, 512, 0.9, 0.01)[1] == 512
    with pytest.raises(ValueError):
        m._sampling_controls("sampling", 1.0, 513)
    (T, k, top_p, min_p), rows = m._row_controls("sampling", 2, 1.0, [300, 512], 1.0, 0.0, None)
    assert [r[2] for r in rows] == [300, 512]
    with pytest.raises(ValueError):
        m._row_controls("sampling", 2, 1.0, [300, 513], 1.0, 0.0, None)
    tr = m._track_controls("sampling", 1, 3, {"top_k": np.array([300, 512, 0])}, 1.0, 0, 1.0, 0.0)
    assert tr["top_k"].tolist() == [[300, 512, 0]]
    with pytest.raises(ValueError):
        m._track_controls("sampling", 1, 3, {"top_k": np.array([300, 513, 0])}, 1.0, 0, 1.0, 0.0)


def test_mu_law_round_trip_at_9_and_10_bits():
    """run_decode writes through loaders.samples_to_int16(samples, n_quantize): every class of a 512- or 1024-class model decodes to an int16 value that
    ascends with the class (of its own at 512 classes), and encoding the decoded waveform gives the class back."""
    from qpnet_amd import loaders
    from qpnet_amd.qpnet import decode_mu_law, encode_mu_law
    for Q in (512, 1024):
        ids = np.arange(Q)
        pcm = loaders.samples_to_int16(ids, Q)
        assert pcm.dtype == np.int16 and (np.diff(pcm.astype(np.int64)) >= 0).all() and pcm[0] < -32000 and pcm[-1] > 32000
        assert Q > 512 or len(np.unique(pcm)) == Q          # (at 1024 classes the cells around zero are narrower than one int16 step)
        # (decode_mu_law puts class y half a step below the point that encodes to y, so the round trip is taken from the middle of the class's cell)
        np.testing.assert_array_equal(encode_mu_law(decode_mu_law(ids + 0.5, Q), Q), ids)
