"""CPU: the sampling controls (temperature, top_k) -- the numpy restatement of their spec (tests/sampling_spec.py) against the C oracle and
against the distribution it claims to draw from, and the argument checks of the C ABI and of the Python surface, none of which needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import sampling_spec as SS
from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY, PAPER


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_spec_restatement_equals_the_oracle_at_default_controls(cfgname, oracle):
    """T = 1, k = 0: the restatement, fed the logits of the oracle's own sampling run, reproduces that run's stream (row 1 of a batch: the row
    enters the Philox counter).  This pins qexp, the generator, the summation order, the scan and the pick of the helper to the C spec."""
    cfg = TINY if cfgname == "tiny" else PAPER
    flat = synth.make_weights(cfg, 31)
    x, h, d, n = synth.decode_inputs(cfg, 3, 61, 1.0)
    seed = 0x1234567890ABCDEF
    r = oracle.decode(cfg, flat, h, d, x, n, mode="sampling", seed=seed, row=1, want_logits=True)
    assert n == 329 and len(np.unique(r["samples"])) > 32
    np.testing.assert_array_equal(SS.draw_steps(r["logits"], seed, 1), r["samples"])
    # the controls at their neutral values in every spelling: the same stream
    np.testing.assert_array_equal(SS.draw_steps(r["logits"], seed, 1, temperature=1.0, top_k=cfg.n_quantize), r["samples"])


def _merged_chi2(counts, expect):
    """Pearson chi-square with the cells of expectation < 5 pooled (into one cell, joined by the smallest others until it holds 5) -> (chi2, df)."""
    order = np.argsort(expect)
    counts, expect = counts[order].astype(np.float64), expect[order]
    n_small = int((expect < 5).sum())
    while 0 < n_small < len(expect) and expect[:n_small].sum() < 5:
        n_small += 1
    if n_small:
        counts = np.concatenate([[counts[:n_small].sum()], counts[n_small:]])
        expect = np.concatenate([[expect[:n_small].sum()], expect[n_small:]])
    return float(((counts - expect) ** 2 / expect).sum()), len(expect) - 1


@pytest.mark.parametrize("T,k", [(0.7, 40), (1.5, 0), (0.5, 7), (1.0, 256)])
def test_restated_draw_follows_the_tempered_truncated_softmax(T, k, oracle):
    """40 000 draws over the step counter from one fixed 256-logit row: none outside the kept set, and the counts pass a chi-square test
    against softmax(l / T) renormalised over the kept set in float64 (99.9 % quantile; fixed seed, so the test is deterministic)."""
    from scipy.stats import chi2
    Q, N = 256, 40000
    l = (2.0 * np.random.RandomState(1234).standard_normal(Q)).astype(np.float32)
    keep = SS.kept_set(l, k)[0]
    assert keep.sum() == (Q if k in (0, Q) else k)          # (distinct logits: no ties)
    u = SS.uniforms(20241019, 3, range(N))
    picks = np.concatenate([SS.draw(np.broadcast_to(l, (len(c), Q)), c, T, k) for c in np.array_split(u, 8)])
    counts = np.bincount(picks, minlength=Q)
    assert counts[~keep].sum() == 0, "draws outside the kept set: classes %s" % np.nonzero(counts * ~keep)[0]
    z = l.astype(np.float64)[keep] / T
    p = np.exp(z - z.max()); p /= p.sum()
    x2, df = _merged_chi2(counts[keep], N * p)
    bound = chi2.ppf(0.999, df)
    print("T=%g k=%d: chi2 %.1f, df %d (chi2/df %.2f), 99.9 %% quantile %.1f" % (T, k, x2, df, x2 / df, bound))
    assert df >= 3 and x2 <= bound


def test_inversions_make_the_membership_test_necessary():
    """The per-class cumulative is not monotone across lane boundaries once classes are dropped (a lane restarts from the scanned prefix, summed
    in another order), so `first class past the threshold` must also ask for membership: on random logits with k = 40 there are lane starts
    whose running sum lies below the previous lane's end."""
    l = (4.0 * np.random.RandomState(7).standard_normal((64, 256))).astype(np.float32)
    keep, e = SS.weights(l, 1.0, 40)
    e3 = e.reshape(64, 64, 4)
    v = e3[:, :, 0]
    for j in range(1, 4):
        v = v + e3[:, :, j]
    s, d = v, 1
    while d < 64:
        t = s.copy(); t[:, d:] = s[:, d:] + s[:, :-d]; s = t; d *= 2
    run_end = np.concatenate([np.zeros((64, 1), np.float32), s[:, :-1]], axis=1)
    for j in range(4):
        run_end = run_end + e3[:, :, j]
    assert (s[:, :-1] < run_end[:, :-1]).sum() > 0      # some lane's start (scanned prefix) lies below where its predecessor's running sum ended


BAD_T = [float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 1e-39]


def test_abi_checks_the_controls_without_a_gpu():
    L = _lib.lib()
    assert L.qpn_version() % 1000 >= 4
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    try:
        for t in BAD_T:
            assert L.qpn_decode_sampling(hp, t, 0) == -1 and b"temperature" in L.qpn_last_error(), t
        for k in (-1, TINY.n_quantize + 1):
            assert L.qpn_decode_sampling(hp, 1.0, k) == -1 and b"top_k" in L.qpn_last_error(), k
        assert L.qpn_decode_sampling(hp, 0.7, 64) == 0
        assert L.qpn_decode_sampling(hp, 1.0, TINY.n_quantize) == 0
        assert L.qpn_decode_sampling(hp, 1.0, 0) == 0
        assert L.qpn_decode_sampling(None, 1.0, 0) == -1
    finally:
        L.qpn_destroy(hp)
    # the stand-alone draw runs the same checks, before it looks for a device or at its pointers
    for t in BAD_T:
        assert L.qpn_sample_logits(None, 1, 256, 0, 0, 0, t, 0, None, None) == -1 and b"temperature" in L.qpn_last_error(), t
    for k in (-1, 257):
        assert L.qpn_sample_logits(None, 1, 256, 0, 0, 0, 1.0, k, None, None) == -1 and b"top_k" in L.qpn_last_error(), k
    assert L.qpn_sample_logits(None, 1, 128, 0, 0, 0, 1.0, 129, None, None) == -1 and b"top_k" in L.qpn_last_error()
    assert L.qpn_sample_logits(None, 1, 96, 0, 0, 0, 1.0, 0, None, None) == -1 and b"n_quantize" in L.qpn_last_error()
    assert L.qpn_sample_logits(None, 1, 256, 0, 0, 0, 0.7, 64, None, None) == -1 and b"bad arguments" in L.qpn_last_error()      # (null pointers)


def test_python_surface_refuses_bad_controls_before_any_device_work():
    """CPU tensors: a call that reached the device layer would raise RuntimeError (no CPU fallback); bad controls raise ValueError first."""
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    args = (torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440)))
    for kw in (dict(temperature=0), dict(temperature=float("nan")), dict(temperature=-2.0), dict(temperature=1e-39), dict(temperature="warm"),
               dict(top_k=-1), dict(top_k=257), dict(top_k=2.5), dict(mode="argmax", top_k=5), dict(mode="argmax", temperature=0.7)):
        with pytest.raises(ValueError):
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(ValueError):
            m.generate_live(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # good controls go on to the device layer
        m.batch_fast_generate(*args, temperature=0.7, top_k=64)
    with pytest.raises(TypeError):                                   # keyword-only: the reference's positional signature is unchanged
        m.batch_fast_generate(*args, None, "sampling", False, 0.7)
