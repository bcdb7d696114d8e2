"""GPU: sampling decode at n_quantize 320, 512 and 1024 (Q = 64 * per, per = 5, 8, 16: the wide draw of decode_dev.h), bit for bit against the numpy
restatement of the draw for any `per` (tests/wide_draw_spec.py, held to the narrow restatements and to the C oracle by tests/test_wide_quantize_cpu.py) and
against the C oracle's own sampled streams.

1. qpn_sample_logits_ex puts crafted rows in front of the device function the wide kernels' picks call.
2. The oracle's sampled stream at 512 classes, from its logits.
3. The closed loop through batch_fast_generate, sampled and greedy, on the one-CU interpreter, the per-utterance cooperative kernel and the batched one.
4. Controls in the loop (uniform, per-row records, a draw track), each held to the restatement applied to the call's own logits.
5. generate_live."""
import functools

import numpy as np
import pytest

import frame_spec as FS
import nucleus_spec as NS
import sampling_spec as SS
import util
import wide_draw_spec as WS
import wide_quantize_common as WQ
from test_nucleus_gpu import MIN_PS, TKS, TOP_PS, _sample_logits_ex
from test_sampling_controls_gpu import KNOBS, _families, _rows_in_input_order

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x9E3779B97F4A7C15
# step counters at which (SEED, batch row 2) draws u = 1 - 2^-24, the largest uniform there is: th = u * total then rounds to the float below the scanned total (or to
# the total itself), and a row whose lanes' own running sums stay below that fires no class.  Found by walking the counter; the test re-derives u and the branch.
U_MAX_STEPS = (7331401, 37308044, 49753947, 54588162)
REDUCED = ((1.0, 0.0), (0.9, 0.0), (0.5, 0.05), (1.0, 1e-4))      # (top_p, min_p) crossed with the extra top_k values


def _combos(Q):
    """the controls grid of test_nucleus_gpu, and top_k = 1, per, 65, Q - 1 and Q (at three temperatures) under four (top_p, min_p) pairs"""
    per = Q // 64
    extra = ((1.0, 1), (0.7, per), (1.3, 65), (1.0, Q - 1), (0.7, Q))
    return [(T, k, p, q) for T, k in TKS for p in TOP_PS for q in MIN_PS] + [(T, k, p, q) for T, k in extra for p, q in REDUCED]


def _wide_families(Q, n, rs):
    """name -> (n, Q) float32 rows: the families of test_sampling_controls_gpu (random rows at two scales, a grid with ties on the k-th value, all-equal rows, one
    dominant class, zeros of either sign around the k-th value), nucleus_spec's tied rows, and rows for the lane layout of the wide draw"""
    fam = _families(Q, n, rs)
    fam["tied"] = NS.tied_rows(Q, n, rs)
    fam["flat"] = (0.05 * rs.standard_normal((n, Q))).astype(F32)
    last = (0.5 * rs.standard_normal((n, Q))).astype(F32)
    last[:, Q - 1] += 40.0                                         # the whole mass in the last lane's last class
    fam["last"] = last
    first = (0.5 * rs.standard_normal((n, Q))).astype(F32)
    first[:, 0] += 40.0                                            # ... in class 0
    fam["first"] = first
    inf = (2.0 * rs.standard_normal((n, Q))).astype(F32)
    inf[rs.random_sample((n, Q)) < 0.4] = -np.inf                  # -inf entries, whole lanes of them among others
    for r in range(n):
        lane = rs.randint(0, 64)
        inf[r, lane * (Q // 64):(lane + 1) * (Q // 64)] = -np.inf
        inf[r, rs.randint(0, Q)] = 1.0                             # (never a row of nothing but -inf)
    fam["inf"] = inf
    return fam


@pytest.mark.parametrize("Q", [320, 512, 1024])
def test_sample_logits_ex_on_crafted_rows_bitwise(Q, cuda, oracle):
    combos = _combos(Q)
    rs = np.random.RandomState(7000 + Q)
    fams = _wide_families(Q, len(combos), rs)
    names = sorted(fams)
    cover = dict(strict=0, kth_ties=0, min_p=0, high=0)
    bad, n = [], 0
    for ci, (T, k, top_p, min_p) in enumerate(combos):
        rows = np.stack([fams[f][ci] for f in names])
        step0 = 50000 * ci + 5
        got = _sample_logits_ex(cuda, rows, SEED, 2, step0, T, k, top_p, min_p)
        N, e, info = WS.cut(rows, T, k, top_p, min_p)
        want = WS.pick(e, N, SS.uniforms(SEED, 2, range(step0, step0 + len(rows))))
        assert N[np.arange(len(rows)), want].all()
        cover["strict"] += int(((info["N"] > 1) & (info["N"] < info["M"])).sum())
        cover["kth_ties"] += int((info["K"] > k).sum()) if 0 < k < Q else 0
        cover["min_p"] += int((info["M"] < info["K"]).sum())
        cover["high"] += int((want >= 256).sum())
        n += len(rows)
        for r in np.nonzero(got != want)[0]:
            bad.append("T=%g k=%d top_p=%g min_p=%g %s: got %d (%s N), spec %d; |K| %d |M| %d |N| %d" % (
                T, k, top_p, min_p, names[r], got[r], "in" if 0 <= got[r] < Q and N[r, got[r]] else "NOT in", want[r], info["K"][r], info["M"][r], info["N"][r]))
    print("Q=%d: %d rows; %s" % (Q, n, cover))
    # (floors at about half of what the spec gives on these 1276 rows -- 176 to 183 strict nuclei, 229 or 230 rows with more classes kept than k, 542 to 547 rows
    #  that min_p cuts, 313 / 626 / 915 picks beyond class 255 -- so that the rows cannot silently stop reaching the branches)
    assert cover["strict"] >= 85 and cover["kth_ties"] >= 110 and cover["min_p"] >= 270 and cover["high"] >= n // 8, cover
    assert not bad, "%d of %d rows differ: %s" % (len(bad), n, "; ".join(bad[:8]))


@pytest.mark.parametrize("Q", [320, 512, 1024])
def test_highest_kept_class_when_no_class_fires(Q, cuda, oracle):
    """u = 1 - 2^-24: rows on which no running sum exceeds the threshold take the highest kept class -- Q - 1 for the default draw, the highest class of the
    kept set with a cut.  One row per launch (a launch's rows draw at consecutive counters)."""
    u = SS.uniforms(SEED, 2, U_MAX_STEPS)
    assert (u == F32(1.0) - F32(2.0 ** -24)).all()
    rows = (2.0 * np.random.RandomState(9000 + Q).standard_normal((24, Q))).astype(F32)
    reached = {}
    for name, (T, k, top_p, min_p) in dict(default=(1.0, 0, 1.0, 0.0), top_k=(0.7, 40, 1.0, 0.0), nucleus=(1.0, 0, 0.9, 0.0)).items():
        N, e, _ = WS.cut(rows, T, k, top_p, min_p)
        dry = WS.none_fires(e, N, np.repeat(u[:1], len(rows)))
        want = WS.pick(e, N, np.repeat(u[:1], len(rows)))
        reached[name] = int(dry.sum())
        for r in np.nonzero(dry)[0][:6]:
            assert want[r] == Q - 1 - int(N[r, ::-1].argmax()) and (name != "default" or want[r] == Q - 1)
            for step in U_MAX_STEPS[:2]:
                got = _sample_logits_ex(cuda, rows[r:r + 1], SEED, 2, step, T, k, top_p, min_p)[0]
                assert got == want[r], "%s row %d step %d: kernel %d, spec %d (the highest kept class)" % (name, r, step, got, want[r])
    print("Q=%d: rows on which no class fires at u = 1 - 2^-24, of 24: %s" % (Q, reached))
    assert all(v >= 1 for v in reached.values()), reached


def test_sample_logits_default_controls_equal_the_oracle_stream_at_512(cuda, oracle):
    """T = 1, k = 0 (and k = Q) on the oracle's logits at 512 classes: the oracle's sampling stream."""
    r = WQ.oracle_stream((64, 64, 512))
    lg, y = r["logits"], r["samples"]
    np.testing.assert_array_equal(_sample_logits_ex(cuda, lg, WQ.SEED, WQ.ROW, 0, 1.0, 0, 1.0, 0.0), y)
    np.testing.assert_array_equal(_sample_logits_ex(cuda, lg, WQ.SEED, WQ.ROW, 0, 1.0, 512, 1.0, 0.0), y)
    half = len(y) // 2                                             # step0 shifts the counter, nothing else
    np.testing.assert_array_equal(_sample_logits_ex(cuda, lg[half:], WQ.SEED, WQ.ROW, half, 1.0, 0, 1.0, 0.0), y[half:])


# ---------------------------------------------------------------- the closed loop
_UTTS = [(61, 3, 1.0), (62, 2, 0.5), (63, 1, 1.5), (64, 3, 1.5), (65, 2, 1.0)]      # ragged: 329 samples and fewer
# name: ((n_resch, n_skipch, n_quantize), environment, batch rows, what the plan of the call must say)
_CASES = {
    "Q320": ((64, 48, 320), {}, 2, "one-cu rows=2"),
    "Q512": ((64, 64, 512), {}, 2, "one-cu rows=2"),
    "Q1024": ((64, 64, 1024), {}, 2, "one-cu rows=2"),
    "Q320-coop": ((64, 48, 320), {"QPN_DECODE_COOP": "8"}, 2, "coop G="),
    "Q512-coop": ((64, 64, 512), {"QPN_DECODE_COOP": "8"}, 2, "coop G="),
    "Q1024-coop": ((64, 64, 1024), {"QPN_DECODE_COOP": "8"}, 2, "coop G="),
    "C512-S64-Q512": ((512, 64, 512), {}, 3, "coop G="),          # one CU cannot hold the step state; 64 skip channels are below the batched kernel's tiles
    "C512-S256-Q512": ((512, 256, 512), {}, 5, "coopb G="),       # ... 256 are not: the batched cooperative kernel, 8 logit rows per workgroup; five rows: two utterances share a group
}


def _model(case, cuda, monkeypatch):
    import torch
    csq, env, B, plan = _CASES[case]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, flat = WQ.cfg_of(csq), WQ.weights(csq)
    m = util.build_model(cfg, flat, cuda)               # (a new module: its handle is created under the knobs)
    bx, bh, bd, ns = util.decode_batch(cfg, _UTTS[:B])
    assert max(ns) <= 330 and len(set(ns)) == min(B, 3)
    return cfg, flat, m, plan, (bx, bh, bd, ns), (torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda))


@functools.lru_cache(maxsize=None)
def _oracle_rows(case, mode):
    """the oracle's streams of a case's batch in input order, computed once"""
    from oracle import cpu_oracle
    csq, _, B, _ = _CASES[case]
    cfg = WQ.cfg_of(csq)
    bx, bh, bd, ns = util.decode_batch(cfg, _UTTS[:B])
    return tuple(_rows_in_input_order(cpu_oracle.batch_fast_generate(cfg, WQ.weights(csq), bx, bh, list(ns), bd, mode=mode, seed=SEED), ns))


def _assert_plan(m, B, plan):
    assert m.last_decode_plan == util.plan_query(m, B), (m.last_decode_plan, util.plan_query(m, B))
    assert plan in m.last_decode_plan and (plan != "coop G=" or m.last_decode_plan.startswith(plan)), m.last_decode_plan
    assert plan != "coopb G=" or " x 2 " in m.last_decode_plan, m.last_decode_plan      # (two utterances in a group: the second one's logits lie Q floats behind the first's)


@pytest.mark.parametrize("case", list(_CASES))
def test_sampled_decode_equals_the_oracle(case, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, (bx, bh, bd, ns), (xb, hb) = _model(case, cuda, monkeypatch)
    m.sampling_seed = SEED
    rows = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)
    _assert_plan(m, len(ns), plan)
    print("WIDE sampled %s: %s" % (case, m.last_decode_plan))
    want = _oracle_rows(case, "sampling")
    for b in range(len(ns)):
        np.testing.assert_array_equal(rows[b], want[b], err_msg="%s (%s) row %d" % (case, m.last_decode_plan, b))
    y = np.concatenate(rows)
    assert len(np.unique(y)) >= 128 and (y >= 256).sum() >= 32      # a draw over the whole range, not a constant


@pytest.mark.parametrize("case", list(_CASES))
def test_greedy_decode_equals_the_oracle(case, cuda, oracle, monkeypatch):
    """the ground under the feature: greedy decode is generic in n_quantize"""
    cfg, flat, m, plan, (bx, bh, bd, ns), (xb, hb) = _model(case, cuda, monkeypatch)
    rows = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="argmax"), ns)
    _assert_plan(m, len(ns), plan)
    want = _oracle_rows(case, "argmax")
    for b in range(len(ns)):
        np.testing.assert_array_equal(rows[b], want[b], err_msg="%s (%s) row %d" % (case, m.last_decode_plan, b))


# ---------------------------------------------------------------- controls in the loop
def _call(m, xb, hb, ns, bd, **kw):
    """qpn_decode behind _decode_args with the logits output -> (rows in input order, logits (B, max_n, Q)): the logits every pick was drawn from"""
    import torch
    from qpnet_amd import _lib
    a = m._decode_args(xb, hb, list(ns), bd, "sampling", False, **kw)
    call = list(a["call"])
    logits = torch.empty((a["B"], max(a["max_n"], 1), m.n_quantize), dtype=torch.float32, device=a["dev"])
    call[15] = logits.data_ptr()
    try:
        with torch.cuda.device(a["dev"]):
            _lib.check(a["L"].qpn_decode(*call))
            m.last_decode_plan = a["L"].qpn_last_decode_plan(a["hd"]).decode()
    finally:
        _lib.check(a["L"].qpn_decode_frame_sampling(a["hd"], 0, 0, None))
        _lib.check(a["L"].qpn_decode_row_sampling(a["hd"], 0, None))
    out = a["out"].cpu().numpy()
    return [out[b, :n].copy() for b, n in enumerate(a["ns"])], logits.cpu().numpy()


def _teacher_forced(oracle, cfg, flat, batch, b, y):
    bx, bh, bd, ns = batch
    return oracle.decode(cfg, flat, bh[b], bd[b], bx[b], ns[b], maxd=int(np.nanmax(np.ceil(bd))), teacher=y, want_logits=True)["logits"]


_LOOP_CASES = ["Q512", "Q512-coop", "C512-S256-Q512"]


@pytest.mark.parametrize("case", _LOOP_CASES)
def test_closed_loop_with_all_four_controls(case, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _model(case, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    T, k, top_p, min_p = 0.7, 40, 0.9, 0.01
    m.sampling_seed = SEED
    rows, logits = _call(m, xb, hb, ns, bd, temperature=T, top_k=k, top_p=top_p, min_p=min_p)
    assert plan in m.last_decode_plan, m.last_decode_plan
    for b in range(len(ns)):
        y, lg = rows[b], logits[b, :ns[b]]
        N, e, info = WS.cut(lg, T, k, top_p, min_p)
        want = WS.pick(e, N, SS.uniforms(SEED, b, range(len(y))))
        diff = np.nonzero(want != y)[0]
        assert diff.size == 0, "%s row %d (%s): first difference at step %d of %d: kernel %d, spec %d" % (case, b, m.last_decode_plan, diff[0], len(y), y[diff[0]], want[diff[0]])
        assert (info["N"] < info["K"]).any() and (info["K"] >= k).all()
        if b == 0:      # the call's own logits are the oracle's teacher-forced logits of its picks, bit for bit
            ref = _teacher_forced(oracle, cfg, flat, batch, b, y)
            assert np.array_equal(lg.view(np.uint32), ref.view(np.uint32)), "logits differ from the oracle's, max abs diff %g" % np.abs(lg - ref).max()
    assert (np.concatenate(rows) >= 256).sum() >= 16


@pytest.mark.parametrize("case", _LOOP_CASES)
def test_closed_loop_with_per_row_records(case, cuda, monkeypatch):
    """distinct seeds and controls per row: row b draws from (its seed, stream 0) with its own four values"""
    cfg, flat, m, plan, batch, (xb, hb) = _model(case, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B = len(ns)
    ctl = [[(0.7, 40, 0.9, 0.01), (1.3, 300, 0.95, 0.0), (1.0, 0, 0.8, 0.02)][b % 3] for b in range(B)]
    seeds = [(0xC0FFEE0000000001 + SEED * (b + 1)) % (1 << 64) | (1 << 63) | (1 << 40) for b in range(B)]
    m.sampling_seed = 12345                                        # (ignored by the rows: each has a key of its own)
    rows, logits = _call(m, xb, hb, ns, bd, temperature=[c[0] for c in ctl], top_k=[c[1] for c in ctl], top_p=[c[2] for c in ctl], min_p=[c[3] for c in ctl], row_seeds=seeds)
    assert plan in m.last_decode_plan, m.last_decode_plan
    for b in range(B):
        want = WS.draw_steps(logits[b, :ns[b]], seeds[b], 0, 0, *ctl[b])
        diff = np.nonzero(want != rows[b])[0]
        assert diff.size == 0, "%s row %d %r (%s): first difference at step %d: kernel %d, spec %d" % (case, b, ctl[b], m.last_decode_plan, diff[0], rows[b][diff[0]], want[diff[0]])
    assert not np.array_equal(rows[0][:ns[1]], rows[1])


@pytest.mark.parametrize("case", _LOOP_CASES)
def test_closed_loop_with_a_draw_track(case, cuda, monkeypatch):
    """a track that alternates two records by frame, shifted by one frame from row to row"""
    cfg, flat, m, plan, batch, (xb, hb) = _model(case, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B, F, U = len(ns), bh.shape[2], cfg.upsampling_factor
    recs = [(0.7, 40, 0.9, 0.01), (1.2, 300, 1.0, 0.0)]
    track = FS.track_of([[recs[(f + b) % 2] for f in range(F)] for b in range(B)])
    m.sampling_seed = SEED
    rows, logits = _call(m, xb, hb, ns, bd, draw_track=track)
    assert plan in m.last_decode_plan, m.last_decode_plan
    for b in range(B):
        lg, n = logits[b, :ns[b]], ns[b]
        per_step = FS.records(FS.row_of(track, b), n, bx.shape[1], U, F)
        u = SS.uniforms(SEED, b, range(n))
        want = np.full(n, -1, dtype=np.int64)
        for rec in sorted(set(per_step)):
            at = np.array([i for i, r in enumerate(per_step) if r == rec])
            want[at] = WS.draw(lg[at], u[at], *rec)
        diff = np.nonzero(want != rows[b])[0]
        assert diff.size == 0, "%s row %d (%s): first difference at step %d (frame %d): kernel %d, spec %d" % (
            case, b, m.last_decode_plan, diff[0], FS.frame_of(int(diff[0]), bx.shape[1], U, F), rows[b][diff[0]], want[diff[0]])
        if n > U:       # the records are felt: the row is not what its first frame's record alone would draw
            assert len(set(per_step)) == 2 and not np.array_equal(WS.draw(lg, u, *per_step[0]), rows[b])


def test_generate_live_at_512_classes(cuda, monkeypatch):
    """generate_live: its pieces, concatenated, are batch_fast_generate's rows, default draw and with controls; with on_close="cancel" what was handed over of a
    row is a prefix of the full row."""
    cfg, flat, m, plan, batch, (xb, hb) = _model("Q512", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED
    for kw in (dict(mode="sampling"), dict(mode="sampling", temperature=0.8, top_k=300, top_p=0.9)):
        want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)
        got = [[] for _ in ns]
        for b, start, piece in m.generate_live(xb, hb, list(ns), bd, every=64, **kw):
            assert start == sum(len(p) for p in got[b])
            got[b].append(piece)
        for b in range(len(ns)):
            np.testing.assert_array_equal(np.concatenate(got[b]), want[b])
    np.testing.assert_array_equal(_rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling"), ns)[0], _oracle_rows("Q512", "sampling")[0])
    gen = m.generate_live(xb, hb, list(ns), bd, every=32, on_close="cancel", **kw)
    got = [[] for _ in ns]
    for b, start, piece in gen:
        got[b].append(piece)
        break
    gen.close()
    counts = m.last_decode_counts
    assert counts is not None and len(counts) == len(ns)
    for b in range(len(ns)):
        have = np.concatenate(got[b]) if got[b] else np.zeros(0, dtype=np.int64)
        assert len(have) <= counts[b] <= ns[b]
        np.testing.assert_array_equal(have, want[b][:len(have)])
