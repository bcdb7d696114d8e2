"""numpy restatement of the sampling draw for Q = 64 * per with per in 1..16: the default draw, the draw with temperature and
top-k, and the top_p / min_p cuts, for the tests of n_quantize up to 1024.

Nothing here is new arithmetic.  The pieces that pin it are the ones tests/sampling_spec.py and tests/nucleus_spec.py export -- `qexp` and `uniforms` (the C
oracle's exp and generator), `kept_set` (top-k by value, ties kept), and `tree_mass` / `masses` (the balanced tree the top_p mass is summed in) -- and the
order is stated once more, for any `per`: lane i owns classes per * i .. per * i + per - 1; a lane's partial sum runs left to right over its `per` weights;
the scan over the 64 lane sums is the inclusive Hillis-Steele scan, d = 1..32; th = u * v_63; a lane's running sum starts from v_{i-1}; the first kept
class whose running sum exceeds th wins, and when none does the pick is the highest kept class.  tests/test_wide_quantize_cpu.py holds this file to
sampling_spec.draw and nucleus_spec.draw bit for bit where those are defined (per <= 4), and to the C oracle's own sampled streams beyond."""
import numpy as np

import nucleus_spec as NS
import sampling_spec as SS

F32 = np.float32
MAX_PER = 16


def _per(Q):
    assert Q % 64 == 0 and 1 <= Q // 64 <= MAX_PER, "Q = %d: the draw is defined for Q = 64 * per, per in 1..%d" % (Q, MAX_PER)
    return Q // 64


def lane_sums(e):
    """(R, Q) weights -> (R, 64): every lane's `per` weights summed left to right."""
    R, Q = e.shape
    e3 = e.reshape(R, 64, _per(Q))
    a = e3[:, :, 0].copy()
    for j in range(1, e3.shape[2]):
        a = a + e3[:, :, j]
    return a


def scan(a):
    """inclusive Hillis-Steele scan over the 64 lanes: v_i += v_{i-d} for d = 1, 2, .., 32 (every lane reads the values of the step before)."""
    v, d = a, 1
    while d < 64:
        t = v.copy()
        t[:, d:] = v[:, d:] + v[:, :-d]
        v, d = t, 2 * d
    return v


def _fire(e, keep, u):
    e = np.atleast_2d(np.asarray(e, dtype=F32))
    keep = np.atleast_2d(keep)
    R, Q = e.shape
    per = _per(Q)
    u = np.asarray(u, dtype=F32).reshape(R)
    v = scan(lane_sums(e))
    th = u * v[:, 63]
    c = np.concatenate([np.zeros((R, 1), dtype=F32), v[:, :-1]], axis=1)
    e3, k3 = e.reshape(R, 64, per), keep.reshape(R, 64, per)
    fire = np.zeros((R, 64, per), dtype=bool)
    for j in range(per):
        c = c + e3[:, :, j]
        fire[:, :, j] = k3[:, :, j] & (c > th[:, None])
    return fire.reshape(R, Q), keep


def pick(e, keep, u):
    """Step 4 on given weights (R, Q), 0.0 outside the kept set `keep` (R, Q) bool: scan, threshold, first kept class past it, else the highest kept class."""
    fire, keep = _fire(e, keep, u)
    last_kept = keep.shape[1] - 1 - keep[:, ::-1].argmax(axis=1)
    return np.where(fire.any(axis=1), fire.argmax(axis=1), last_kept).astype(np.int64)


def none_fires(e, keep, u):
    """(R,) bool: the rows whose threshold no kept class's running sum exceeds (u next to 1 and a scanned total that rounded above the lanes' own sums):
    the draws that take the `highest kept class` branch."""
    return ~_fire(e, keep, u)[0].any(axis=1)


def default_draw(logits, u):
    """The draw of a call that sets no control (the C oracle's sample_spec): e_c = qexp(l_c - m) for every class; none past the threshold: Q - 1."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    _per(l.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):
        e = SS.qexp(l - l.max(axis=1)[:, None])
    return pick(e, np.ones(l.shape, dtype=bool), u)


def cut(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """-> (N, e, info) as nucleus_spec.cut: steps 1 to 3 (temperature and top-k weights, min_p, top_p under the tree's mass), for per in 1..16."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    _per(l.shape[1])
    return NS.cut(l, temperature, top_k, top_p, min_p, mass=NS.tree_mass)


def draw(logits, u, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """The pick of every row of `logits` (R, Q) with the uniforms u (R,)."""
    N, e, _ = cut(logits, temperature, top_k, top_p, min_p)
    return pick(e, N, u)


def draw_steps(logits, seed, row, step0=0, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """Row r of `logits` drawn at counter (step0 + r, row): what a decode call with this seed picks at those steps of batch row `row`."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    return draw(l, SS.uniforms(seed, row, range(step0, step0 + l.shape[0])), temperature, top_k, top_p, min_p)
