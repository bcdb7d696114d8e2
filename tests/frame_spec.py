"""Restatement of the draw track (qpn_decode_frame_sampling) for its tests: which feature frame's record a generated sample draws with,
and the draw of a whole row with per-step records on top of tests/nucleus_spec.py (the controlled draw) and tests/sampling_spec.py (the uniforms)."""
import numpy as np

KEYS = ("temperature", "top_k", "top_p", "min_p")


def frame_of(i, n_x, U, F):
    """f(i) = min(F - 1, c(i) / U), c(i) = n_x - 1 + i  (U == 0: min(F - 1, c(i)))"""
    c = n_x - 1 + i
    return min(F - 1, c // U if U > 0 else c)


def first_step_of(f, n_x, U):
    """i*: the first i with f(i) >= f (for f within the frames the row reaches)"""
    return max(0, (f * U if U > 0 else f) - (n_x - 1))


def records(track_row, n, n_x, U, F):
    """track_row: {key: (F,) array} -> the n per-step records [(T, k, top_p, min_p)] of a row's generated samples"""
    fr = [frame_of(i, n_x, U, F) for i in range(n)]
    return [(float(np.float32(track_row["temperature"][f])), int(track_row["top_k"][f]), float(np.float32(track_row["top_p"][f])), float(np.float32(track_row["min_p"][f]))) for f in fr]


def draw_track_steps(logits, seed, stream, track_row, n_x, U, F):
    """Row r of `logits` (n, Q) drawn at counter (r, stream) under key `seed` with the record of frame f(r): what a decode call with this track picks."""
    import nucleus_spec as NS
    import sampling_spec as SS
    l = np.atleast_2d(np.asarray(logits, dtype=np.float32))
    n = l.shape[0]
    u = SS.uniforms(seed, stream, range(n))
    recs = records(track_row, n, n_x, U, F)
    out = np.full(n, -1, dtype=np.int64)
    for rec in sorted(set(recs)):
        at = np.array([i for i, r in enumerate(recs) if r == rec])
        out[at] = NS.draw(l[at], u[at], *rec)
    return out


def track_of(rows):
    """[[(T, k, top_p, min_p)] * F] * B -> the draw_track dict of (B, F) arrays"""
    a = np.array(rows, dtype=np.float64)
    return {"temperature": a[..., 0].astype(np.float32), "top_k": a[..., 1].astype(np.int32), "top_p": a[..., 2].astype(np.float32), "min_p": a[..., 3].astype(np.float32)}


def row_of(track, b):
    return {k: np.asarray(track[k])[b] for k in KEYS}
