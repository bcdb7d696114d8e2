"""numpy restatement of the top_p / min_p cuts of the sampling draw, on top of tests/sampling_spec.py, which
states steps 1 and 4 (temperature, top-k, weights; scan and pick) and is pinned to the C oracle.

Steps 2 and 3 are stated here in their brute-force form: for every distinct weight w of a row, the mass S(w) of the weights >= w in the spec's
order (lane partials left to right, then a balanced pairwise tree over the 64 lanes); w* is the largest w whose mass reaches top_p * S(0).  The
kernels find the same set by a bisection on the bit pattern; tests/test_nucleus_cpu.py holds the two to each other.  With top_p = 1 and
min_p = 0 nothing of this file runs but `pick`, which tests/test_nucleus_cpu.py holds to sampling_spec.draw."""
import numpy as np

import sampling_spec as SS

F32 = np.float32


def tree_mass(e):
    """(R, Q) float32 weights -> (R,) their sum in the spec's order: per-lane left to right, then six levels of adjacent pairs."""
    e = np.atleast_2d(np.asarray(e, dtype=F32))
    R, Q = e.shape
    per = Q // 64
    e3 = e.reshape(R, 64, per)
    a = e3[:, :, 0].copy()
    for j in range(1, per):
        a = a + e3[:, :, j]
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def masses(e_row, mass=tree_mass):
    """One row's distinct weights, ascending, and S(w) for each of them."""
    ws = np.unique(e_row)
    return ws, mass(np.where(e_row[None, :] >= ws[:, None], e_row[None, :], F32(0.0)).astype(F32))


def sequential_mass(e):
    """NOT the spec: the weights summed left to right over the whole row in float32."""
    return np.cumsum(np.atleast_2d(e), axis=1, dtype=F32)[:, -1]


def float64_mass(e):
    """NOT the spec: the weights summed in float64 (target and comparison are then float64 too)."""
    return np.atleast_2d(e).astype(np.float64).sum(axis=1)


def cut(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, mass=tree_mass):
    """-> (N, e, info): the set the draw may pick from, (R, Q) bool; the weights, 0.0 outside N; and info = dict of (R,) arrays -- `K`, `M`, `N`
    the sizes of the three sets and `ties` how many classes of N carry the weight w* (0 where top_p is off).
    `mass` is the summation order of S; anything but tree_mass is NOT the spec (the order witnesses of the tests)."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    top_p, min_p = F32(top_p), F32(min_p)
    assert 0 < top_p <= 1 and 0 <= min_p <= 1
    K, e = SS.weights(l, temperature, top_k)
    M = K & (e >= min_p) if min_p > 0 else K
    e = np.where(M, e, F32(0.0)).astype(F32)
    N = M.copy()
    ties = np.zeros(len(l), dtype=np.int64)
    if top_p < 1:
        for r in range(len(l)):
            ws, S = masses(e[r], mass)
            target = top_p * S[0]                      # (S of the smallest weight present is S(0): total; one float32 multiply)
            w = ws[np.nonzero(S >= target)[0].max()]
            N[r] = M[r] & (e[r] >= w)
            ties[r] = int((e[r] == w).sum())
        e = np.where(N, e, F32(0.0)).astype(F32)
    assert N.any(axis=1).all() and not (N & ~K).any()
    return N, e, dict(K=K.sum(axis=1), M=M.sum(axis=1), N=N.sum(axis=1), ties=ties)


def pick(e, keep, u):
    """Step 4, sampling_spec.draw's scan and membership pick, on given weights (R, Q) and kept set."""
    e = np.atleast_2d(np.asarray(e, dtype=F32))
    R, Q = e.shape
    per = Q // 64
    u = np.asarray(u, dtype=F32).reshape(R)
    e3, k3 = e.reshape(R, 64, per), np.atleast_2d(keep).reshape(R, 64, per)
    a = e3[:, :, 0].copy()
    for j in range(1, per):
        a = a + e3[:, :, j]
    v, d = a, 1
    while d < 64:
        t = v.copy()
        t[:, d:] = v[:, d:] + v[:, :-d]
        v = t
        d *= 2
    th = u * v[:, 63]
    c = np.concatenate([np.zeros((R, 1), dtype=F32), v[:, :-1]], axis=1)
    fire = np.zeros((R, 64, per), dtype=bool)
    for j in range(per):
        c = c + e3[:, :, j]
        fire[:, :, j] = k3[:, :, j] & (c > th[:, None])
    fire = fire.reshape(R, Q)
    last_kept = Q - 1 - np.atleast_2d(keep)[:, ::-1].argmax(axis=1)
    return np.where(fire.any(axis=1), fire.argmax(axis=1), last_kept).astype(np.int64)


def draw(logits, u, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, mass=tree_mass):
    """The pick of every row of `logits` (R, Q) with the uniforms u (R,)."""
    N, e, _ = cut(logits, temperature, top_k, top_p, min_p, mass)
    return pick(e, N, u)


def tied_rows(Q, n, rs):
    """(n, Q) float32 rows on a grid of seven logit values: whatever the boundary weight w* is, dozens of classes carry it."""
    return (0.75 * rs.randint(-6, 1, size=(n, Q))).astype(F32)


# Order witnesses: (row of witness_rows(), bit pattern of top_p, step).  At temperature 1, top_k 0, min_p 0 the nucleus of that row under the spec's
# tree differs from the nucleus under a left-to-right float32 sum of the row, or under a float64 sum, or both: top_p was set to S(w) / S(0) of a
# boundary weight w, or one ulp beside it, so that the last bit of the mass decides whether w's class is needed.  (Built that way, about every
# second try is a witness; random (row, top_p) pairs practically never are.)  `step` is the first step counter (seed WITNESS_SEED, batch row 2) at
# which the draw from the other nucleus picks another class.  tests/test_nucleus_cpu.py re-derives all of this.
WITNESS_SEED = 0x9E3779B97F4A7C15
WITNESSES = [(218, 0x3f7be08d, 27), (117, 0x3f53b638, 16), (282, 0x3f7fb7d0, 394), (195, 0x3f7dc8e1, 240), (327, 0x3f7ff966, 1166),
             (123, 0x3f7feaab, 10), (363, 0x3f7d9748, 98), (308, 0x3f7d4a9e, 19), (161, 0x3f7fcb32, 121), (176, 0x3f7ff2f0, 464)]


def witness_rows():
    return (4.0 * np.random.RandomState(2718).standard_normal((400, 256))).astype(F32)


def draw_steps(logits, seed, row, step0=0, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """Row r of `logits` drawn at counter (step0 + r, row): what a decode call with this seed picks at those steps of batch row `row`."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    return draw(l, SS.uniforms(seed, row, range(step0, step0 + l.shape[0])), temperature, top_k, top_p, min_p)
