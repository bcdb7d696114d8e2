"""GPU: the top_p / min_p cuts of sampling decode, bit for bit against the numpy restatement of their spec (tests/nucleus_spec.py, held to
sampling_spec, to a bisection and to the claimed distribution by tests/test_nucleus_cpu.py).

1. qpn_sample_logits_ex puts crafted rows in front of the device function the decode kernels' picks call.
2. The committed order witnesses: rows whose nucleus depends on the order in which the mass is summed.
3. The closed loop through batch_fast_generate on every decode kernel (see test_sampling_controls_gpu: a stream that feeds back its own picks is
   the teacher-forced stream of those picks, so the oracle's teacher-forced logits of an output row are the logits the kernel saw).
4. Neutral and extreme values, 5. generate_live, 6. the re-run after a launch that gave up."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nucleus_spec as NS
import sampling_spec as SS
import util
from test_sampling_controls_gpu import _KERNELS, _families, _rows_in_input_order, _setup, _teacher_forced_logits

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x9E3779B97F4A7C15
TOP_PS = (1e-30, 0.1, 0.5, 0.9, 0.999, 1.0)
MIN_PS = (0.0, 1e-4, 0.05, 1.0)
TKS = ((1.0, 0), (0.7, 40), (0.01, 0), (100.0, 5))
PER = 6
# per Q: rows with |N| > 1 and N a strict subset of M / rows with more than one class on w* / rows where min_p alone removes something /
# rows where top_p removes something after min_p did.  About half of what the spec gives on these rows (crafted_rows + NS.cut on the CPU:
# of 4032 rows, 256: 553, 1466, 1754, 234; 128: 565, 1445, 1777, 241; 64: 568, 1407, 1817, 268)
FLOORS = {256: (275, 730, 875, 115), 128: (280, 720, 885, 120), 64: (280, 700, 905, 130)}


def _sample_logits_ex(cuda, rows, seed, row, step0, T, k, top_p, min_p):
    import torch
    from qpnet_amd import _lib
    lg = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(cuda)
    out = torch.full((lg.shape[0],), -1, dtype=torch.int64, device=cuda)
    _lib.check(_lib.lib().qpn_sample_logits_ex(lg.data_ptr(), lg.shape[0], lg.shape[1], seed, row, step0, T, k, top_p, min_p, out.data_ptr(),
                                               torch.cuda.current_stream(cuda).cuda_stream))
    return out.cpu().numpy()


def crafted_rows(Q):
    """-> [((T, k, top_p, min_p), step0, names, rows)]: PER rows of every family (those of test_sampling_controls_gpu plus the tied one) per combination"""
    rs = np.random.RandomState(3000 + Q)
    combos = [(T, k, p, q) for T, k in TKS for p in TOP_PS for q in MIN_PS]
    fams = _families(Q, PER * len(combos), rs)
    fams["tied"] = NS.tied_rows(Q, PER * len(combos), rs)
    names = sorted(fams)
    return [(c, 50000 * ci + 5, names, np.concatenate([fams[f][ci * PER:(ci + 1) * PER] for f in names])) for ci, c in enumerate(combos)]


@pytest.mark.parametrize("Q", [256, 128, 64])
def test_sample_logits_ex_on_crafted_rows_bitwise(Q, cuda, oracle):
    cover = np.zeros(4, dtype=np.int64)
    bad, n = [], 0
    for (T, k, top_p, min_p), step0, names, rows in crafted_rows(Q):
        got = _sample_logits_ex(cuda, rows, SEED, 2, step0, T, k, top_p, min_p)
        N, e, info = NS.cut(rows, T, k, top_p, min_p)
        want = NS.pick(e, N, SS.uniforms(SEED, 2, range(step0, step0 + len(rows))))
        assert N[np.arange(len(rows)), want].all()
        cover += [((info["N"] > 1) & (info["N"] < info["M"])).sum(), (info["ties"] > 1).sum(), (info["M"] < info["K"]).sum(),
                  ((info["M"] < info["K"]) & (info["N"] < info["M"])).sum()]
        n += len(rows)
        for r in np.nonzero(got != want)[0]:
            bad.append("T=%g k=%d top_p=%g min_p=%g %s row %d: got %d (%s N), spec %d; |K| %d |M| %d |N| %d" % (
                T, k, top_p, min_p, names[r // PER], r % PER, got[r], "in" if 0 <= got[r] < Q and N[r, got[r]] else "NOT in", want[r],
                info["K"][r], info["M"][r], info["N"][r]))
    print("Q=%d: %d rows; strict nucleus %d, ties on w* %d, min_p cuts %d, top_p cuts after min_p %d" % ((Q, n) + tuple(cover)))
    assert (cover >= FLOORS[Q]).all(), "the crafted rows cover too little: %s against the floors %s" % (cover, FLOORS[Q])
    assert not bad, "%d of %d rows differ: %s" % (len(bad), n, "; ".join(bad[:8]))


def test_order_witnesses_get_the_nucleus_of_the_tree(cuda, oracle):
    """Rows whose nucleus under a sequential float32 or a float64 sum of the mass is another one (re-derived in test_nucleus_cpu): the kernel's
    pick is the spec's at the committed step, where the draw from the other nucleus picks another class."""
    rows = NS.witness_rows()
    told_apart = 0
    for r, bits, step in NS.WITNESSES:
        top_p = float(np.array([bits], dtype=np.uint32).view(F32)[0])
        u = SS.uniforms(NS.WITNESS_SEED, 2, [step])
        N, e, _ = NS.cut(rows[r], top_p=top_p)
        want = NS.pick(e, N, u)[0]
        others = {int(NS.pick(ea, Na, u)[0]) for Na, ea, _ in (NS.cut(rows[r], top_p=top_p, mass=m) for m in (NS.sequential_mass, NS.float64_mass))}
        got = _sample_logits_ex(cuda, rows[r:r + 1], NS.WITNESS_SEED, 2, step, 1.0, 0, top_p, 0.0)[0]
        assert got == want, "row %d top_p %r step %d: kernel %d, spec %d (other summation orders: %s)" % (r, top_p, step, got, want, sorted(others))
        told_apart += int(others != {int(want)})
    assert told_apart >= 1


_CONTROLS = [(1.0, 0, 0.9, 0.0), (0.7, 0, 1.0, 0.05), (1.0, 40, 0.95, 0.0), (1.3, 255, 0.999, 1e-3)]


@pytest.mark.parametrize("T,k,top_p,min_p", _CONTROLS, ids=["p0.9", "T0.7m0.05", "k40p0.95", "T1.3k255p0.999m0.001"])
@pytest.mark.parametrize("kernel", list(_KERNELS))
def test_closed_loop_with_top_p_and_min_p_on_every_kernel(kernel, T, k, top_p, min_p, cuda, oracle, monkeypatch):
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    k = min(k, cfg.n_quantize - 1)
    m.sampling_seed = SEED
    rows = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=T, top_k=k, top_p=top_p, min_p=min_p), ns)
    assert plan in m.last_decode_plan, m.last_decode_plan
    check = range(len(ns)) if len(ns) <= 2 else [0, 1, 2, 3, len(ns) - 2, len(ns) - 1]      # (pipe2: the longest rows and the shortest, which share groups)
    for b in check:
        y = rows[b]
        assert len(y) == ns[b] and 0 <= y.min() and y.max() < cfg.n_quantize
        lg = _teacher_forced_logits(oracle, cfg, flat, batch, b, y)
        N, e, info = NS.cut(lg, T, k, top_p, min_p)
        want = NS.pick(e, N, SS.uniforms(SEED, b, range(len(y))))
        diff = np.nonzero(want != y)[0]
        assert diff.size == 0, "%s row %d (%s): first difference at step %d of %d: kernel %d, spec %d" % (
            kernel, b, m.last_decode_plan, diff[0], len(y), y[diff[0]], want[diff[0]])
        assert N[np.arange(len(y)), y].all()
        if top_p <= 0.95:                                          # (synthetic weights give broad rows: min_p, or top_p = 0.999, may keep them whole)
            assert (info["N"] < info["M"]).any()


@pytest.mark.parametrize("kernel", [n for n in _KERNELS if n != "pipe2"])
def test_neutral_and_extreme_values_and_batch_mates(kernel, cuda, oracle, monkeypatch):
    """top_p = 1 with min_p = 0 is the call without the keywords, also right behind a call that set them; top_p = 1e-30 and min_p = 1 are the
    argmax stream (where no step has a second class of weight exactly 1); a row's stream does not depend on the other rows of its batch."""
    import torch
    cfg, flat, m, plan, batch, (xb, hb) = _setup(kernel, cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED

    def run(**kw):
        return _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)

    greedy = run(mode="argmax")
    for b in range(len(ns)):
        e = SS.weights(_teacher_forced_logits(oracle, cfg, flat, batch, b, greedy[b]), 1.0, 0)[1]
        assert ((e == 1).sum(axis=1) == 1).all(), "a second class of weight 1: top_p = 1e-30 and min_p = 1 keep both"
    tiny_p = run(mode="sampling", top_p=1e-30)
    full_m = run(mode="sampling", min_p=1.0)
    ctl = run(mode="sampling", top_p=0.9, min_p=0.01)
    plain = run(mode="sampling")                                   # right behind a call that set them
    neutral = run(mode="sampling", top_p=1.0, min_p=0.0)
    o = _rows_in_input_order(oracle.batch_fast_generate(cfg, flat, bx, bh, list(ns), bd, mode="sampling", seed=SEED), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(tiny_p[b], greedy[b], err_msg="%s row %d top_p=1e-30" % (kernel, b))
        np.testing.assert_array_equal(full_m[b], greedy[b], err_msg="%s row %d min_p=1" % (kernel, b))
        np.testing.assert_array_equal(plain[b], o[b], err_msg="%s row %d" % (kernel, b))
        np.testing.assert_array_equal(neutral[b], o[b])
    # another utterance in row 0 (same length and pitch factor, so the same batch maxd): row 1 draws what it drew
    bx2, bh2, bd2, ns2 = util.decode_batch(cfg, [(77, 4, 1.0), (62, 3, 0.5)])
    assert ns2 == ns and int(np.nanmax(np.ceil(bd2))) == int(np.nanmax(np.ceil(bd))) and not np.array_equal(bh2[0], bh[0])
    other = _rows_in_input_order(m.batch_fast_generate(torch.from_numpy(bx2).to(cuda), torch.from_numpy(bh2).to(cuda), list(ns2), bd2,
                                                       mode="sampling", top_p=0.9, min_p=0.01), ns2)
    np.testing.assert_array_equal(other[1], ctl[1])
    assert not np.array_equal(other[0], ctl[0]) and not np.array_equal(ctl[1], plain[1])


def test_generate_live_with_top_p_and_min_p(cuda, monkeypatch):
    """generate_live(top_p, min_p): its pieces, concatenated, are batch_fast_generate's rows with the same values and seed; the setter is
    refused while that call is in flight; the values do not outlive the call."""
    from qpnet_amd import _lib
    cfg, flat, m, plan, batch, (xb, hb) = _setup("pipe", cuda, monkeypatch)
    bx, bh, bd, ns = batch
    m.sampling_seed = SEED
    kw = dict(mode="sampling", temperature=0.9, top_p=0.85, min_p=0.02)
    want = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, **kw), ns)
    plain = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=0.9), ns)
    got = [[] for _ in ns]
    first = True
    for b, start, piece in m.generate_live(xb, hb, list(ns), bd, every=64, **kw):
        if first:
            first = False
            assert _lib.lib().qpn_decode_sampling_ex(m._handle, 1.0, 0, 0.5, 0.1) == -5      # QPN_ESTATE: a decode is in flight
        assert start == sum(len(p) for p in got[b])
        got[b].append(piece)
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(got[b]), want[b])
        assert not np.array_equal(want[b], plain[b])
    again = _rows_in_input_order(m.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", temperature=0.9), ns)
    for b in range(len(ns)):
        np.testing.assert_array_equal(again[b], plain[b])


def test_rerun_after_a_give_up_draws_with_the_same_top_p():
    """The fault-injection hook exists only in the -DQPN_TESTING build: the scenario runs in a child process bound to it (tests/nucleus_giveup_child.py),
    the way util.run_giveup_child runs the other give-up scenarios."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0", QPN_TEST_PIPE_GIVES_UP="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "nucleus_giveup_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NUCLEUS_GIVEUP_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
