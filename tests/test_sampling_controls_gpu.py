"""GPU: the sampling controls (temperature, top_k) of sampling decode, bit for bit against the numpy restatement of their spec
(tests/sampling_spec.py, pinned to the C oracle by tests/test_sampling_controls_cpu.py).

1. qpn_sample_logits puts crafted rows in front of the device function the decode kernels' picks call: ties on the k-th value, all-equal
   rows, one dominant class, -0.0 / +0.0 around the threshold, temperatures that drive every non-maximum into qexp's clamp.
2. The closed loop through batch_fast_generate on every decode kernel.  A stream that feeds back its own picks IS the teacher-forced stream
   of those picks, so the oracle's teacher-forced logits of an output row are bit for bit the logits the kernel saw, and the restated
   draw at (seed, row, step) must give the row back.
3. generate_live with controls."""
import numpy as np
import pytest

import sampling_spec as SS
import util
from qpnet_amd import synth

pytestmark = pytest.mark.gpu

KNOBS = ("QPN_DECODE_COOP", "QPN_DECODE_COOPB", "QPN_DECODE_PIPE", "QPN_PIPE_NU", "QPN_DECODE_GENERIC")
TEMPS = (1.0, 0.7, 1.5, 0.01, 100.0)
SEED = 0x9E3779B97F4A7C15


def _top_ks(Q):
    return sorted({min(k, Q) for k in (0, 1, 2, 3, 4, 5, 63, 64, 65, Q - 1, Q)})


def _sample_logits(cuda, rows, seed, row, step0, T, k):
    import torch
    from qpnet_amd import _lib
    lg = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(cuda)
    out = torch.full((lg.shape[0],), -1, dtype=torch.int64, device=cuda)
    _lib.check(_lib.lib().qpn_sample_logits(lg.data_ptr(), lg.shape[0], lg.shape[1], seed, row, step0, T, k, out.data_ptr(),
                                            torch.cuda.current_stream(cuda).cuda_stream))
    return out.cpu().numpy()


def _families(Q, n, rs):
    """name -> (n, Q) float32 rows"""
    fam = {}
    fam["normal"] = rs.standard_normal((n, Q))
    fam["wide"] = 8.0 * rs.standard_normal((n, Q))
    fam["grid"] = np.round(2.0 * rs.standard_normal((n, Q)) * 4.0) / 4.0                  # a 1/4 grid: many ties, also on the k-th value
    fam["equal"] = np.repeat(np.round(4.0 * rs.standard_normal((n, 1)), 2), Q, axis=1)
    peak = 0.5 * rs.standard_normal((n, Q))
    peak[np.arange(n), rs.randint(0, Q, n)] += 30.0
    fam["peak"] = peak
    zeros = rs.choice(np.array([-0.0, 0.0]), size=(n, Q))          # zeros of either sign around a few positive and negative classes: the k-th
    for r in range(n):                                             # value is a zero for every k between their counts, and all zeros tie with it
        pos, neg = rs.randint(0, 6), rs.randint(0, 6)
        at = rs.permutation(Q)[:pos + neg]
        zeros[r, at[:pos]] = rs.choice([0.5, 1.0, 3.0], size=pos)
        zeros[r, at[pos:]] = rs.choice([-0.5, -1.0, -3.0], size=neg)
    fam["zeros"] = zeros
    return {k: v.astype(np.float32) for k, v in fam.items()}


@pytest.mark.parametrize("Q", [256, 128, 64])
def test_sample_logits_on_crafted_rows_bitwise(Q, cuda, oracle):
    rs = np.random.RandomState(1000 + Q)
    combos = [(T, k) for T in TEMPS for k in _top_ks(Q)]
    per = 6
    fams = _families(Q, per * len(combos), rs)
    kth_ties = zero_mix = clamp_rows = 0
    bad = []
    for ci, (T, k) in enumerate(combos):
        names = sorted(fams)
        rows = np.concatenate([fams[f][ci * per:(ci + 1) * per] for f in names])
        step0 = 70000 * ci + 3                                     # (counters beyond 2^16, and past 2^21 for the last combinations)
        got = _sample_logits(cuda, rows, SEED, 2, step0, T, k)
        want = SS.draw(rows, SS.uniforms(SEED, 2, range(step0, step0 + len(rows))), T, k)
        keep = SS.kept_set(rows, k)
        assert keep[np.arange(len(rows)), want].all()
        if 0 < k < Q:
            kth_ties += int((keep.sum(axis=1) > k).sum())
            srt = np.sort(rows, axis=1)[:, Q - k]
            zero_mix += int(((srt == 0) & (np.signbit(rows) & (rows == 0)).any(axis=1) & (~np.signbit(rows) & (rows == 0)).any(axis=1)).sum())
        if T == 0.01:
            clamp_rows += int((((rows - rows.max(axis=1, keepdims=True)) * np.float32(100.0) < -87).sum(axis=1) >= Q - 8).sum())
        for r in np.nonzero(got != want)[0]:
            bad.append("T=%g k=%d %s row %d: got %d, spec %d" % (T, k, names[r // per], r % per, got[r], want[r]))
    assert kth_ties >= 100, "the crafted rows put too few ties on the k-th value: %d" % kth_ties
    assert zero_mix >= 20, "too few rows whose k-th value is a zero among zeros of both signs: %d" % zero_mix
    assert clamp_rows >= 50, "T = 0.01 should drive (nearly) every non-maximum into the clamp of qexp: %d rows" % clamp_rows
    assert not bad, "%d of %d rows differ: %s" % (len(bad), per * 6 * len(combos), "; ".join(bad[:8]))


# (row of the matrix below, step): draws whose threshold falls between the scanned prefix a lane starts from and the running sum the lane before it
# ended on, with a dropped class first in the lane.  Found once by searching the 2^24 values of u per row for such a window and then the step
# counter for a draw that has that u (seed SEED, batch row 2); the test re-derives that they are what they are said to be.
_WITNESSES = [(191, 11824), (372, 13867), (13, 15908), (209, 15984), (316, 17718), (103, 19444), (350, 22036), (178, 27887), (354, 31562), (262, 35464)]


def test_pick_asks_for_membership_where_the_cumulative_is_not_monotone(cuda, oracle):
    """Once classes are dropped the per-class cumulative is not monotone across lane boundaries, so a pick that is merely `first class past the
    threshold` takes a dropped class at these draws; the spec (and the kernel) skip it.  k = 40, T = 1: the controlled path by top_k alone."""
    rows = (4.0 * np.random.RandomState(4242).standard_normal((400, 256))).astype(np.float32)
    for r, step in _WITNESSES:
        u = SS.uniforms(SEED, 2, [step])
        want = SS.draw(rows[r:r + 1], u, 1.0, 40)
        naive = SS.draw(rows[r:r + 1], u, 1.0, 40, membership=False)
        keep = SS.kept_set(rows[r:r + 1], 40)
        assert naive[0] != want[0] and not keep[0, naive[0]] and keep[0, want[0]], "row %d step %d is no witness" % (r, step)
        got = _sample_logits(cuda, rows[r:r + 1], SEED, 2, step, 1.0, 40)
        assert got[0] == want[0], "row %d step %d: kernel %d, spec %d (without the membership test: %d)" % (r, step, got[0], want[0], naive[0])


def test_sample_logits_default_controls_equal_the_oracle_stream(cuda, oracle):
    """T = 1, k = 0 (and k = Q) on the oracle's PAPER logits: the oracle's sampling stream."""
    from qpnet_amd.config import PAPER
    cfg = PAPER
    flat = synth.make_weights(cfg, 31)
    x, h, d, n = synth.decode_inputs(cfg, 3, 61, 1.0)
    r = oracle.decode(cfg, flat, h, d, x, n, mode="sampling", seed=SEED, row=1, want_logits=True)
    np.testing.assert_array_equal(_sample_logits(cuda, r["logits"], SEED, 1, 0, 1.0, 0), r["samples"])
    np.testing.assert_array_equal(_sample_logits(cuda, r["logits"], SEED, 1, 0, 1.0, 256), r["samples"])
    half = n // 2                                                  # step0 shifts the counter, nothing else
    np.testing.assert_array_equal(_sample_logits(cuda, r["logits"][half:], SEED, 1, half, 1.0, 0), r["samples"][half:])


_WIDE = dict(n_resch=128, n_skipch=128, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1)
_KERNELS = {   # name: (geometry kwargs, None for PAPER or "tiny", environment, what last_decode_plan must say, batch rows)
    "pipe": (None, {}, "pipe rows=2", 2),
    "pipe2": (None, {"QPN_PIPE_NU": "2"}, "(2 per group)", 50),      # more rows than resident groups: two utterances per five-role group
    "one-cu": (None, {"QPN_DECODE_PIPE": "0"}, "one-cu rows=2", 2),
    "interpreter": (_WIDE, {}, "", 2),
    "coop": (None, {"QPN_DECODE_COOP": "4"}, "coop G=4", 2),
    "coopb": (dict(n_resch=256, n_skipch=256, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=2), {"QPN_DECODE_COOP": "32"}, "coopb G=32 ", 2),
    "tiny": ("tiny", {}, "one-cu rows=2", 2),
    "q128": (dict(n_quantize=128, n_resch=64, n_skipch=128, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1), {}, "", 2),
}
_CONTROLS = [(0.7, 0), (1.0, 5), (0.5, 64), (1.3, 255)]


def _setup(kernel, cuda, monkeypatch):
    import torch
    from qpnet_amd.config import PAPER, TINY, QPNetConfig
    geo, env, plan, B = _KERNELS[kernel]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = PAPER if geo is None else TINY if geo == "tiny" else QPNetConfig(**geo)
    flat = synth.make_weights(cfg, 29)
    m = util.build_model(cfg, flat, cuda)               # (a new module: its handle is created under the knobs)
    utts = [(61 + b, 4 if b % 2 == 0 else 3, (1.0, 0.5)[b % 2]) for b in range(B)]      # ragged: 439 and 329 samples
    bx, bh, bd, ns = util.decode_batch(cfg, utts)
    assert max(ns) <= 440
    return cfg, flat, m, plan, (bx, bh, bd, ns), (torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda))


def _rows_in_input_order(outs, ns):
    order = sorted(range(len(ns)), key=lambda i: ns[i])
    rows = [None] * len(ns)
    for pos, i in enumerate(order):
        rows[i] = outs[pos]
    return rows


def _teacher_forced_logits(oracle, cfg, flat, batch, b, y):
    bx, bh, bd, ns = batch
    maxd = int(np.nanmax(np.ceil(bd)))
    return oracle.decode(cfg, flat, bh[b], bd[b], bx[b], ns[b], maxd=maxd, teacher=y, want_logits=True)["logits"]


@pytest.mark.parametrize("T,k", _CONTROLS, ids=["T0.7", "k5", "T0.5k64", "T1.3k255"])
@pytest.mark.parametrize("kernel", list(_KERNELS))
def test_closed_loop_with_controls_on_every_kernel(kernel, T, k, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    k = min(k, cfg.n_quantize - 1)
    m.sampling_seed = SEED
    rows = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=T, top_k=k), ns)
    assert plan in m.last_decode_plan, m.last_decode_plan
    check = range(len(ns)) if len(ns) <= 2 else [0, 1, 2, 3, len(ns) - 2, len(ns) - 1]      # (pipe2: the longest rows and the shortest, which share groups)
    for b in check:
        y = rows[b]
        assert len(y) == ns[b] and 0 <= y.min() and y.max() < cfg.n_quantize
        lg = _teacher_forced_logits(oracle, cfg, flat, batch, b, y)
        want = SS.draw_steps(lg, SEED, b, 0, T, k)
        diff = np.nonzero(want != y)[0]
        assert diff.size == 0, "%s row %d (%s): first difference at step %d of %d: kernel %d, spec %d" % (
            kernel, b, m.last_decode_plan, diff[0], len(y), y[diff[0]], want[diff[0]])
        assert SS.kept_set(lg, k)[np.arange(len(y)), y].all()
        if b == 0 and k == 0:
            assert len(np.unique(y)) > 16                          # a draw, not a constant


@pytest.mark.parametrize("kernel", [n for n in _KERNELS if n != "pipe2"])
def test_neutral_controls_top1_and_batch_mates(kernel, cuda, oracle, monkeypatch):
    """top_k = 1 is the argmax stream (where no step has tied maxima); temperature 1 with top_k 0 is the call without the keywords, also right
    after a call that set them (nothing carries over); a row's stream does not depend on the other rows of its batch."""
    import torch
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED

    def run(**kw):
        return _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)

    greedy = run(mode="argmax")
    top1 = run(mode="sampling", temperature=0.7, top_k=1)
    for b in range(len(ns)):
        lg = _teacher_forced_logits(oracle, cfg, flat, batch, b, greedy[b])
        assert ((lg == lg.max(axis=1, keepdims=True)).sum(axis=1) == 1).all(), "tied maxima: top_k = 1 keeps both"
        np.testing.assert_array_equal(top1[b], greedy[b], err_msg="%s row %d" % (kernel, b))
    plain = run(mode="sampling")                                   # right behind a call with controls
    neutral = run(mode="sampling", temperature=1.0, top_k=0)
    full = run(mode="sampling", temperature=1.0, top_k=cfg.n_quantize)
    o = oracle.batch_fast_generate(cfg, flat, bx, bh, list(ns), bd, mode="sampling", seed=SEED)
    for b, want in enumerate(_rows_in_input_order(o, ns)):
        np.testing.assert_array_equal(plain[b], want, err_msg="%s row %d" % (kernel, b))
        np.testing.assert_array_equal(neutral[b], want)
        np.testing.assert_array_equal(full[b], want)
    # another utterance in row 0 (same length and pitch factor, so the same batch maxd): row 1 draws what it drew
    ctl = run(mode="sampling", temperature=0.7, top_k=40)
    bx2, bh2, bd2, ns2 = util.decode_batch(cfg, [(77, 4, 1.0), (62, 3, 0.5)])
    assert ns2 == ns and int(np.nanmax(np.ceil(bd2))) == int(np.nanmax(np.ceil(bd))) and not np.array_equal(bh2[0], bh[0])
    other = _rows_in_input_order(m.batch_fast_generate(torch.from_numpy(bx2).to(cuda), torch.from_numpy(bh2).to(cuda), list(ns2), bd2,
                                                       mode="sampling", temperature=0.7, top_k=40), ns2)
    np.testing.assert_array_equal(other[1], ctl[1])
    assert not np.array_equal(other[0], ctl[0]) and not np.array_equal(ctl[1], plain[1])


def test_generate_live_with_controls(cuda, monkeypatch):
    """generate_live(temperature, top_k): its pieces, concatenated, are batch_fast_generate's rows with the same controls and seed; the
    setter is refused while that call is in flight; the controls do not outlive the call."""
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("pipe", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=0.6, top_k=30), ns)
    plain = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)
    got = [[] for _ in ns]
    gen = m.generate_live(xb, hb, list(ns), bd, mode="sampling", every=64, temperature=0.6, top_k=30)
    first = True
    for b, start, piece in gen:
        if first:
            first = False
            assert _lib.lib().qpn_decode_sampling(m._handle, 0.5, 3) == -5      # QPN_ESTATE: a decode is in flight
        assert start == sum(len(p) for p in got[b])
        got[b].append(piece)
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(got[b]), want[b])
        assert not np.array_equal(want[b], plain[b])
    again = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(again[b], plain[b])
