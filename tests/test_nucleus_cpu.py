"""CPU: the top_p / min_p cuts of the sampling draw -- the numpy restatement of their spec (tests/nucleus_spec.py) against sampling_spec at the
neutral values, against an independently written bisection, against the distribution it claims to draw from and against other summation
orders; and the argument checks of the C ABI and of the Python surface, none of which needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import nucleus_spec as NS
import sampling_spec as SS
from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY, PAPER

F32 = np.float32


@pytest.mark.parametrize("cfgname", ["tiny", "paper"])
def test_neutral_values_are_the_draw_of_sampling_spec(cfgname, oracle):
    """top_p = 1, min_p = 0 on the oracle's own sampling runs (those of test_spec_restatement_equals_the_oracle_at_default_controls): the
    restated pick of this helper is sampling_spec's, which is the oracle's stream -- also with a temperature and a top-k cut."""
    cfg = TINY if cfgname == "tiny" else PAPER
    flat = synth.make_weights(cfg, 31)
    x, h, d, n = synth.decode_inputs(cfg, 3, 61, 1.0)
    seed = 0x1234567890ABCDEF
    r = oracle.decode(cfg, flat, h, d, x, n, mode="sampling", seed=seed, row=1, want_logits=True)
    np.testing.assert_array_equal(NS.draw_steps(r["logits"], seed, 1), r["samples"])
    np.testing.assert_array_equal(NS.draw_steps(r["logits"], seed, 1, top_p=1.0, min_p=0.0), SS.draw_steps(r["logits"], seed, 1))
    for T, k in ((0.7, 40), (1.3, 5)):
        np.testing.assert_array_equal(NS.draw_steps(r["logits"], seed, 1, 0, T, k), SS.draw_steps(r["logits"], seed, 1, 0, T, k))


def _bisect(e_row, top_p):
    """The search the kernels run, written apart from nucleus_spec: the threshold's bit pattern from bit 30 down, a candidate staying when the
    mass of the weights that reach it -- lane sums left to right, then adjacent pairs, six times -- reaches top_p * total.  -> bool (Q,)"""
    per = len(e_row) // 64
    bits = e_row.view(np.uint32)

    def S(cand):
        w = np.where(bits >= cand, e_row, F32(0.0)).reshape(64, per)
        a = w[:, 0]
        for j in range(1, per):
            a = a + w[:, j]
        for _ in range(6):
            a = a.reshape(-1, 2)
            a = a[:, 0] + a[:, 1]
        assert a.shape == (1,) and a.dtype == F32
        return a[0]

    target = F32(top_p) * S(0)
    thr, prev = 0, S(0)
    for bit in range(30, -1, -1):
        s = S(thr | (1 << bit))
        if s >= target:
            thr |= 1 << bit
    assert S(thr) >= target and prev >= S(thr)
    return bits >= np.uint32(thr)


@pytest.mark.parametrize("Q", [64, 128, 256])
def test_brute_force_nucleus_equals_the_bisection(Q, oracle):
    from test_sampling_controls_gpu import _families
    rs = np.random.RandomState(77 + Q)
    fams = _families(Q, 8, rs)
    fams["tied"] = NS.tied_rows(Q, 8, rs)
    n = cut_rows = 0
    for T, k, min_p in ((1.0, 0, 0.0), (0.7, 40, 1e-3), (0.01, 0, 0.0), (100.0, 5, 0.5)):
        for top_p in (1e-30, 0.1, 0.5, 0.9, 0.999, 0.9999999):
            for name, rows in sorted(fams.items()):
                N, e, info = NS.cut(rows, T, k, top_p, min_p)
                K, e_k = SS.weights(rows, T, k)
                M = K & (e_k >= F32(min_p))
                e_m = np.where(M, e_k, F32(0.0)).astype(F32)
                for r in range(len(rows)):
                    ws, S = NS.masses(e_m[r])
                    assert (np.diff(S) <= 0).all(), "S is not monotone"
                    want = M[r] & _bisect(e_m[r], top_p)
                    assert np.array_equal(N[r], want), "%s row %d T=%g k=%d top_p=%g min_p=%g: brute force keeps %d, bisection %d" % (
                        name, r, T, k, top_p, min_p, N[r].sum(), want.sum())
                    assert N[r, rows[r].argmax()] and not (N[r] & ~M[r]).any()
                    n += 1
                    cut_rows += int(1 < N[r].sum() < M[r].sum())
    # (coverage, not correctness: T = 0.01, top_p = 1e-30 and the peaked rows leave one class, all-equal rows all of them; the rest is 22 % of
    #  the rows at Q = 64 and more at the larger sizes, and the floor is half of that)
    assert cut_rows >= n // 9, "only %d of %d rows have a nucleus that is neither one class nor all of M" % (cut_rows, n)


@pytest.mark.parametrize("T,k,top_p,min_p", [(1.0, 0, 0.9, 0.0), (0.7, 0, 1.0, 0.05), (1.2, 64, 0.8, 0.01)])
def test_restated_draw_follows_the_softmax_renormalised_over_the_nucleus(T, k, top_p, min_p, oracle):
    """40 000 draws over the step counter from one fixed 256-logit row: none outside N, and the counts pass the pooled chi-square test of
    test_sampling_controls_cpu against softmax(l / T) renormalised over N in float64 (99.9 % quantile; fixed seed: deterministic)."""
    from scipy.stats import chi2
    from test_sampling_controls_cpu import _merged_chi2
    Q, n = 256, 40000
    l = (2.0 * np.random.RandomState(1234).standard_normal(Q)).astype(F32)
    N, e, info = NS.cut(l, T, k, top_p, min_p)
    assert 3 < info["N"][0] < (k or Q), info
    u = SS.uniforms(20241019, 3, range(n))
    picks = np.concatenate([NS.pick(np.broadcast_to(e, (len(c), Q)), np.broadcast_to(N, (len(c), Q)), c) for c in np.array_split(u, 8)])
    counts = np.bincount(picks, minlength=Q)
    keep = N[0]
    assert counts[~keep].sum() == 0, "draws outside the nucleus: classes %s" % np.nonzero(counts * ~keep)[0]
    z = l.astype(np.float64)[keep] / T
    p = np.exp(z - z.max()); p /= p.sum()
    x2, df = _merged_chi2(counts[keep], n * p)
    bound = chi2.ppf(0.999, df)
    print("T=%g k=%d top_p=%g min_p=%g: |N| %d, chi2 %.1f, df %d, 99.9 %% quantile %.1f" % (T, k, top_p, min_p, keep.sum(), x2, df, bound))
    assert df >= 3 and x2 <= bound


def test_order_witnesses_are_witnesses(oracle):
    """The committed (row, top_p) pairs: the nucleus under the spec's tree differs from the nucleus under a sequential float32 sum or under a
    float64 sum, and at the committed step the draw from that other nucleus picks another class."""
    rows = NS.witness_rows()
    seq = f64 = 0
    for r, bits, step in NS.WITNESSES:
        top_p = np.array([bits], dtype=np.uint32).view(F32)[0]
        assert 0 < top_p < 1
        N, e, _ = NS.cut(rows[r], top_p=top_p)
        others = [NS.cut(rows[r], top_p=top_p, mass=m)[:2] for m in (NS.sequential_mass, NS.float64_mass)]
        differs = [not np.array_equal(Na, N) for Na, _ in others]
        assert any(differs), "row %d top_p %r is no witness" % (r, top_p)
        seq += differs[0]; f64 += differs[1]
        u = SS.uniforms(NS.WITNESS_SEED, 2, [step])
        mine = NS.pick(e, N, u)[0]
        assert N[0, mine] and any(d and NS.pick(ea, Na, u)[0] != mine for d, (Na, ea) in zip(differs, others)), "row %d step %d: the same pick" % (r, step)
    assert seq >= 3 and f64 >= 3, (seq, f64)


BAD_TOP_P = [float("nan"), 0.0, -0.5, 1.0000001, 2.0, float("inf"), -float("inf")]
BAD_MIN_P = [float("nan"), -1e-6, -1.0, 1.0000001, float("inf")]


def test_abi_checks_top_p_and_min_p_without_a_gpu():
    L = _lib.lib()
    assert L.qpn_version() >= 1005
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    try:
        for p in BAD_TOP_P:
            assert L.qpn_decode_sampling_ex(hp, 1.0, 0, p, 0.0) == -1 and b"top_p" in L.qpn_last_error(), p
        for p in BAD_MIN_P:
            assert L.qpn_decode_sampling_ex(hp, 1.0, 0, 1.0, p) == -1 and b"min_p" in L.qpn_last_error(), p
        assert L.qpn_decode_sampling_ex(hp, float("nan"), 0, 0.9, 0.1) == -1 and b"temperature" in L.qpn_last_error()
        assert L.qpn_decode_sampling_ex(hp, 1.0, -1, 0.9, 0.1) == -1 and b"top_k" in L.qpn_last_error()
        for good in ((1.0, 0, 0.9, 0.0), (0.7, 64, 1e-30, 1.0), (1.0, 0, 1.0, 0.0), (1.0, 0, 1e-45, 0.0)):
            assert L.qpn_decode_sampling_ex(hp, *good) == 0, good
        assert L.qpn_decode_sampling(hp, 1.0, 0) == 0
        assert L.qpn_decode_sampling_ex(None, 1.0, 0, 0.9, 0.0) == -1 and b"null handle" in L.qpn_last_error()
    finally:
        L.qpn_destroy(hp)
    # the stand-alone draw runs the same checks, before it looks for a device or at its pointers
    for p in BAD_TOP_P:
        assert L.qpn_sample_logits_ex(None, 1, 256, 0, 0, 0, 1.0, 0, p, 0.0, None, None) == -1 and b"top_p" in L.qpn_last_error(), p
    for p in BAD_MIN_P:
        assert L.qpn_sample_logits_ex(None, 1, 256, 0, 0, 0, 1.0, 0, 1.0, p, None, None) == -1 and b"min_p" in L.qpn_last_error(), p
    assert L.qpn_sample_logits_ex(None, 1, 256, 0, 0, 0, 0.0, 0, 0.9, 0.0, None, None) == -1 and b"temperature" in L.qpn_last_error()
    assert L.qpn_sample_logits_ex(None, 1, 128, 0, 0, 0, 1.0, 129, 0.9, 0.0, None, None) == -1 and b"top_k" in L.qpn_last_error()
    assert L.qpn_sample_logits_ex(None, 1, 96, 0, 0, 0, 1.0, 0, 0.9, 0.0, None, None) == -1 and b"n_quantize" in L.qpn_last_error()
    assert L.qpn_sample_logits_ex(None, 1, 256, 0, 0, 0, 1.0, 0, 0.9, 0.05, None, None) == -1 and b"bad arguments" in L.qpn_last_error()      # (null pointers)


def test_python_surface_refuses_bad_top_p_and_min_p_before_any_device_work():
    """CPU tensors: a call that reached the device layer would raise RuntimeError (no CPU fallback); bad values raise ValueError first.  The value
    is rounded to float32 before it is checked: 1e-50 is 0 there, 1 + 1e-9 is 1."""
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    args = (torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440)))
    for kw in (dict(top_p=0), dict(top_p=1e-50), dict(top_p=-0.1), dict(top_p=1.001), dict(top_p=float("nan")), dict(top_p="most"), dict(top_p=None),
               dict(min_p=-1e-3), dict(min_p=1.5), dict(min_p=float("nan")), dict(min_p=float("inf")), dict(min_p=[0.1]),
               dict(mode="argmax", top_p=0.9), dict(mode="argmax", min_p=0.05)):
        with pytest.raises(ValueError):
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(ValueError):
            m.generate_live(*args, **kw)
    for kw in (dict(top_p=0.9, min_p=0.05), dict(top_p=1.0 + 1e-9, min_p=1e-50), dict(mode="argmax", top_p=1.0, min_p=0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # good values go on to the device layer
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate_live(*args, **kw)
    with pytest.raises(TypeError):                                       # keyword-only, behind top_k
        m.batch_fast_generate(*args, None, "sampling", False, 1.0, 0, 0.9)
    with pytest.raises(TypeError):
        m.generate_live(*args, None, "sampling", False, 256, 0.001, "finish", 1.0, 0, 0.9)
