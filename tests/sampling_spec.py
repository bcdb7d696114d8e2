"""numpy restatement of the sampling draw with temperature and top-k, for the tests of the sampling controls.

The C oracle states the default draw only, so the controlled draw is restated here, on top of the two pieces of the oracle that pin the
arithmetic: `qpo_qexp` (the spec's exp) and `qpo_philox_first` (the generator).  Everything else is float32 numpy in the spec's order;
tests/test_sampling_controls_cpu.py holds this restatement to the oracle's own stream at temperature 1, top_k 0.  Vectorised over rows (one
row = the Q logits of one step)."""
import ctypes as C

import numpy as np

F32 = np.float32


def _lib():
    from oracle import cpu_oracle
    L = cpu_oracle.lib()
    L.qpo_philox_first.restype = C.c_uint32
    L.qpo_philox_first.argtypes = [C.c_uint32] * 4
    return L


def qexp(x):
    """qpo_qexp, element by element over the distinct bit patterns of a float32 array."""
    x = np.ascontiguousarray(x, dtype=F32)
    bits, inv = np.unique(x.view(np.uint32).ravel(), return_inverse=True)
    f = _lib().qpo_qexp
    vals = np.array([f(v) for v in bits.view(F32).tolist()], dtype=F32)
    return vals[inv].reshape(x.shape)


def uniforms(seed, row, steps):
    """u of the draws at counter (step, row), key = seed: float32(philox >> 8) * 2^-24."""
    f = _lib().qpo_philox_first
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    raw = np.array([f(int(s) & 0xFFFFFFFF, row, k0, k1) for s in steps], dtype=np.uint32)
    return (raw >> 8).astype(F32) * F32(2.0 ** -24)


def kept_set(logits, top_k):
    """(R, Q) bool: the classes the draw may pick -- every class for top_k 0 or >= Q, else those whose logit is >= the top_k-th largest of
    the row counted with multiplicity (IEEE comparison: -0.0 == +0.0; ties with the top_k-th are all kept)."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    Q = l.shape[1]
    if top_k == 0 or top_k >= Q:
        return np.ones(l.shape, dtype=bool)
    kth = np.sort(l, axis=1)[:, Q - top_k]
    return l >= kth[:, None]


def weights(logits, temperature, top_k):
    """(keep, e): e_c = qexp((l_c - m) * invT) on the kept set, 0.0 elsewhere; invT = 1.0f / T in float32."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    keep = kept_set(l, top_k)
    inv_t = F32(1.0) / F32(temperature)
    m = l.max(axis=1)
    with np.errstate(over="ignore"):
        x = (l - m[:, None]) * inv_t                  # one float32 subtract, one float32 multiply
    e = np.where(keep, qexp(x), F32(0.0)).astype(F32)
    return keep, e


def draw(logits, u, temperature=1.0, top_k=0, membership=True):
    """The pick of every row of `logits` (R, Q) with the uniforms u (R,).  Q = 64 * per; lane i owns classes per * i .. per * i + per - 1.
    membership=False is NOT the spec: the pick without its membership test (first class past the threshold, kept or not; none: Q - 1), for
    the tests that show the test is needed."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    R, Q = l.shape
    assert Q % 64 == 0 and Q // 64 <= 4
    per = Q // 64
    u = np.asarray(u, dtype=F32).reshape(R)
    keep, e = weights(l, temperature, top_k)
    e3, k3 = e.reshape(R, 64, per), keep.reshape(R, 64, per)
    a = e3[:, :, 0].copy()                             # lane partial sums, left to right
    for j in range(1, per):
        a = a + e3[:, :, j]
    v = a
    d = 1
    while d < 64:                                      # inclusive Hillis-Steele scan over the lanes
        t = v.copy()
        t[:, d:] = v[:, d:] + v[:, :-d]
        v = t
        d *= 2
    th = u * v[:, 63]
    c = np.concatenate([np.zeros((R, 1), dtype=F32), v[:, :-1]], axis=1)      # a lane's running sum starts from the scanned v_{i-1}
    fire = np.zeros((R, 64, per), dtype=bool)
    for j in range(per):
        c = c + e3[:, :, j]
        fire[:, :, j] = (k3[:, :, j] | (not membership)) & (c > th[:, None])
    fire = fire.reshape(R, Q)
    first = fire.argmax(axis=1)                        # first class, in index order, of the kept set past the threshold
    last_kept = Q - 1 - keep[:, ::-1].argmax(axis=1) if membership else Q - 1   # none fired: the highest class of the kept set
    return np.where(fire.any(axis=1), first, last_kept).astype(np.int64)


def draw_steps(logits, seed, row, step0=0, temperature=1.0, top_k=0):
    """Row r of `logits` drawn at counter (step0 + r, row): what a decode call with this seed picks at those steps of batch row `row`."""
    l = np.atleast_2d(np.asarray(logits, dtype=F32))
    return draw(l, uniforms(seed, row, range(step0, step0 + l.shape[0])), temperature, top_k)
