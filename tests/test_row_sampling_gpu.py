"""GPU: per-row sampling records (qpn_decode_row_sampling; row_seeds= and per-row temperature / top_k / top_p / min_p of batch_fast_generate and
generate_live), on every decode kernel, bit for bit against the numpy restatement of the draw (tests/nucleus_spec.py).

1. Restatement: row b is the restated draw at (seed_b, stream 0, step) with row b's four values on the oracle's teacher-forced logits of that row.
2. Law U: a uniform call with seed s and controls c is the per-row call with {s, b, c} in every row b.
3. Law P: with its (seed, stream) fixed, a row's samples do not depend on its row index, the batch size, the launch plan or the kernel.
4. generate_live, the re-run after a launch that gave up, and the ABI's state rules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nucleus_spec as NS
import util
from test_sampling_controls_gpu import _KERNELS, _setup, _rows_in_input_order, _teacher_forced_logits

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
CYCLE = [(1.0, 0, 1.0, 0.0), (0.7, 40, 1.0, 0.0), (1.0, 0, 0.9, 0.05), (0.5, 64, 0.8, 0.0)]
EINVAL, ESTATE = -1, -5


def _controls(cfg, B):
    return [(T, min(k, cfg.n_quantize - 1), tp, mp) for T, k, tp, mp in (CYCLE[b % 4] for b in range(B))]


def _row_seeds(B):
    """distinct 64-bit keys with high bits set (a key that lost its upper word on the way would draw another stream)"""
    s = [(0xC0FFEE0000000001 + 0x9E3779B97F4A7C15 * (b + 1)) % (1 << 64) | (1 << 63) | (1 << 40) for b in range(B)]
    assert len(set(s)) == B and len({v >> 32 for v in s}) == B
    return s


def _kw(ctl, **more):
    return dict(mode="sampling", temperature=[c[0] for c in ctl], top_k=[c[1] for c in ctl], top_p=[c[2] for c in ctl], min_p=[c[3] for c in ctl], **more)


@pytest.mark.parametrize("kernel", list(_KERNELS))
def test_rows_equal_the_restated_draw_on_every_kernel(kernel, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B = len(ns)
    ctl, seeds = _controls(cfg, B), _row_seeds(B)
    m.sampling_seed = 12345                                        # (ignored by the rows: each has a key of its own)
    rows = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **_kw(ctl, row_seeds=seeds)), ns)
    assert plan in m.last_decode_plan, m.last_decode_plan
    assert m.last_row_seeds == seeds
    check = range(B) if B <= 2 else [0, 1, 2, 3, B - 2, B - 1]      # (pipe2: the longest rows and the shortest, which share groups)
    for b in check:
        y = rows[b]
        assert len(y) == ns[b] and 0 <= y.min() and y.max() < cfg.n_quantize
        lg = _teacher_forced_logits(oracle, cfg, flat, batch, b, y)
        want = NS.draw_steps(lg, seeds[b], 0, 0, *ctl[b])
        diff = np.nonzero(want != y)[0]
        assert diff.size == 0, "%s row %d %r (%s): first difference at step %d of %d: kernel %d, spec %d" % (
            kernel, b, ctl[b], m.last_decode_plan, diff[0], len(y), y[diff[0]], want[diff[0]])
    assert not np.array_equal(rows[0][:ns[1]], rows[1][:ns[0]])


def _raw_call(m, a):
    """qpn_decode on the argument tuple _decode_args built, whatever records the handle holds now -> rows in input order"""
    import torch
    from qpnet_amd import _lib
    with torch.cuda.device(a["dev"]):
        _lib.check(a["L"].qpn_decode(*a["call"]))
    out = a["out"].cpu().numpy()
    return [out[b, :n].copy() for b, n in enumerate(a["ns"])]


@pytest.mark.parametrize("kernel", [n for n in _KERNELS if n != "pipe2"])
def test_law_u_uniform_calls_are_per_row_calls(kernel, cuda, oracle, monkeypatch):
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    B = len(ns)
    m.sampling_seed = SEED

    def run(**kw):
        return _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)

    # per-row controls, no row_seeds: row b draws from (call seed, stream b) -- row b of the uniform call with its controls
    assert B == 2
    ctl = [_controls(cfg, 4)[1], _controls(cfg, 4)[3]]             # (two non-neutral settings)
    per_row = run(**_kw(ctl))
    assert m.last_row_seeds == [SEED] * B and plan in m.last_decode_plan
    for b in range(B):
        T, k, tp, mp = ctl[b]
        uni = run(mode="sampling", temperature=T, top_k=k, top_p=tp, min_p=mp)
        assert m.last_row_seeds is None
        np.testing.assert_array_equal(per_row[b], uni[b], err_msg="%s row %d %r" % (kernel, b, ctl[b]))
        assert not np.array_equal(per_row[1 - b], uni[1 - b])         # (the other row drew with its own setting, not this one)
    # a plain call right behind a per-row call is the plain stream, the oracle's
    plain = run(mode="sampling")
    want = _rows_in_input_order(oracle.batch_fast_generate(cfg, flat, bx, bh, list(ns), bd, mode="sampling", seed=SEED), ns)
    for b in range(B):
        np.testing.assert_array_equal(plain[b], want[b], err_msg="%s row %d" % (kernel, b))
    # all-neutral records {SEED, b, neutral}, forced onto the record path through the ABI setter: the plain stream again
    a = m._decode_args(xb, hb, list(ns), bd, "sampling", False)
    rec = (_lib.QpnRowDraw * B)(*[_lib.QpnRowDraw(SEED, b, 1.0, 0, 1.0, 0.0) for b in range(B)])
    _lib.check(a["L"].qpn_decode_row_sampling(a["hd"], B, rec))
    try:
        forced = _raw_call(m, a)
    finally:
        _lib.check(a["L"].qpn_decode_row_sampling(a["hd"], 0, None))
    for b in range(B):
        np.testing.assert_array_equal(forced[b], want[b], err_msg="%s row %d (neutral records)" % (kernel, b))


def test_law_p_a_row_depends_on_its_own_inputs_and_record_only(cuda, monkeypatch):
    """Utterance A with key s and one non-neutral setting: the same samples at row 0 of [A, X], at row 1 of [X', A], in pipe2's 50-row batch at a row that
    shares a five-role group, and on the one-CU kernel.  X, X' and the 50 rows have A's mates' lengths and pitch factors, so the batch-level maxd is equal."""
    import torch
    s = 0xDEADBEEF0BADF00D
    setting = (0.7, 40, 0.9, 0.01)
    cfg, flat, m50, plan50, batch50, (xb50, hb50) = _setup("pipe2", cuda, monkeypatch)
    ns50 = batch50[3]
    B = len(ns50)
    ia = B - 1                                                     # the last of the short rows: the descriptors are sorted longest first, the last groups hold two each
    A = (61 + ia, 3, 0.5)
    maxd = int(np.nanmax(np.ceil(batch50[2])))

    def controls(B, at):
        ctl = [CYCLE[0]] * B
        ctl[at] = setting
        return ctl

    seeds = _row_seeds(B)
    seeds[ia] = s
    rows = _rows_in_input_order(m50.batch_fast_generate(xb50, hb50, list(ns50), batch50[2], **_kw(controls(B, ia), row_seeds=seeds)), ns50)
    assert plan50 in m50.last_decode_plan, m50.last_decode_plan
    # A's row shares its five-role group: one launch over the resident groups ((CUs / 40) * 8 of them, qpn_pipe_rows_resident), the descriptors sorted longest first
    # (stable) and dealt out as evenly as possible, the LAST B % groups groups taking one more (qpn_launch_decode_pipe)
    assert "waves=1 x %d (2 per group)" % B in m50.last_decode_plan, m50.last_decode_plan
    groups = min(B, (torch.cuda.get_device_properties(cuda).multi_processor_count // 40) * 8)
    base, rem = divmod(B, groups)
    k = sorted(range(B), key=lambda b: -ns50[b]).index(ia)         # (sorted is stable, like the library's sort)
    first = [gi * base + max(0, gi - (groups - rem)) for gi in range(groups)] + [B]
    gi = max(g for g in range(groups) if first[g] <= k)
    assert first[gi + 1] - first[gi] >= 2, "row %d sits alone in group %d of %d: the shared-group case is not covered" % (ia, gi, groups)
    in_group = rows[ia]

    def two_rows(kernel, utts, at, seed):
        _, _, m, plan, _, _ = _setup(kernel, cuda, monkeypatch)
        bx, bh, bd, ns = util.decode_batch(cfg, utts)
        assert int(np.nanmax(np.ceil(bd))) == maxd and sorted(ns) == sorted(set(ns50))
        sd = _row_seeds(2)
        sd[at] = seed
        out = _rows_in_input_order(m.batch_fast_generate(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), list(ns), bd,
                                                         **_kw(controls(2, at), row_seeds=sd)), ns)
        assert plan in m.last_decode_plan, m.last_decode_plan
        return out[at]

    X, X2 = (206, 4, 0.5), (220, 4, 0.5)                           # two utterances of one length and pitch factor whose largest dilated factor rounds up to the 50 rows' maxd
    first = two_rows("pipe", [A, X], 0, s)
    second = two_rows("pipe", [X2, A], 1, s)
    one_cu = two_rows("one-cu", [A, X], 0, s)
    other_key = two_rows("pipe", [A, X], 0, s + 1)
    assert len(first) == ns50[ia]
    np.testing.assert_array_equal(second, first, err_msg="row 1 of [X', A] against row 0 of [A, X]")
    np.testing.assert_array_equal(in_group, first, err_msg="row %d of the 50-row batch (two per group) against row 0 of [A, X]" % ia)
    np.testing.assert_array_equal(one_cu, first, err_msg="the one-CU kernel against the pipelined one")
    assert not np.array_equal(other_key, first)


def test_generate_live_with_row_records(cuda, monkeypatch):
    """generate_live(per-row values, row_seeds): its pieces, concatenated, are batch_fast_generate's rows; with on_close="cancel" what was handed over
    of a row is a prefix of the full row; the setter is refused while the call is in flight."""
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("pipe", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    ctl, seeds = _controls(cfg, 2)[::-1], _row_seeds(2)
    kw = _kw(ctl, row_seeds=seeds)
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)
    got = [[] for _ in ns]
    first = True
    for b, start, piece in m.generate_live(xb, hb, list(ns), bd, every=64, **kw):
        if first:
            first = False
            rec = (_lib.QpnRowDraw * 2)(_lib.QpnRowDraw(1, 0, 1.0, 0, 1.0, 0.0), _lib.QpnRowDraw(2, 0, 1.0, 0, 1.0, 0.0))
            assert _lib.lib().qpn_decode_row_sampling(m._handle, 2, rec) == ESTATE      # a decode is in flight
            assert _lib.lib().qpn_decode_row_sampling(m._handle, 0, None) == ESTATE
        assert start == sum(len(p) for p in got[b])
        got[b].append(piece)
    assert m.last_row_seeds == seeds
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(got[b]), want[b])
    # cancel: stop after the first piece; what was published is a prefix of the full row
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
    # ... and the model is usable: the same call again gives the same rows, a plain call the plain stream of its seed
    again = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(again[b], want[b])


def test_rerun_after_a_give_up_draws_with_the_same_records():
    """The fault-injection hook exists only in the -DQPN_TESTING build: the scenario runs in a child process bound to it (tests/row_sampling_giveup_child.py),
    the way test_nucleus_gpu runs its give-up scenario."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0", QPN_TEST_PIPE_GIVES_UP="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "row_sampling_giveup_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ROW_SAMPLING_GIVEUP_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_enqueue_refuses_a_batch_that_does_not_match_the_records(cuda, monkeypatch):
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("tiny", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    L = _lib.lib()
    a = m._decode_args(xb, hb, list(ns), bd, "sampling", False)          # (clears the records; B = 2)
    rec = (_lib.QpnRowDraw * 3)(*[_lib.QpnRowDraw(b + 1, 0, 1.0, 0, 1.0, 0.0) for b in range(3)])
    _lib.check(L.qpn_decode_row_sampling(a["hd"], 3, rec))
    try:
        assert L.qpn_decode_enqueue(*a["call"]) == EINVAL
        assert "n_rows" in L.qpn_last_error().decode()
        assert L.qpn_decode(*a["call"]) == EINVAL and "n_rows" in L.qpn_last_error().decode()
        # QPN_MODE_ARGMAX calls ignore the records
        g = m._decode_args(xb, hb, list(ns), bd, "argmax", False)
        _lib.check(L.qpn_decode_row_sampling(g["hd"], 3, rec))
        greedy = _raw_call(m, g)
    finally:
        _lib.check(L.qpn_decode_row_sampling(a["hd"], 0, None))
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="argmax"), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(greedy[b], want[b])
