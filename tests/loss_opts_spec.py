"""The loss options in float64 ("Loss options"): what k_ce_opt / k_weight_mass / k_ce_distill's weighted form are tested against.
    w_r = weights[r] (1 without), 0 where y == ignore_index;   CE_r = lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q
    g_r = softmax(z) - (1 - eps) onehot(y) - eps / Q;   L = (1 / N) sum_r w_r CE_r;   dL/dz_r = (w_r / N) g_r;   N = rows ("rows") or sum_r w_r ("weights")"""
import numpy as np


def effective_weights(targets, weights=None, ignore_index=None):
    """targets (R,) int64, weights (R,) or None -> (R,) float64"""
    w = np.ones(targets.shape[0], np.float64) if weights is None else np.asarray(weights, np.float64).copy()
    if ignore_index is not None:
        w[targets == ignore_index] = 0.0
    return w


def row_terms(logits, targets, label_smoothing=0.0, live=None):
    """logits (R, Q), targets (R,) -> (CE_r (R,), g_r (R, Q)) in float64; rows outside `live` (a bool mask; None: all) are not looked at and come back as zeros"""
    z = np.asarray(logits, np.float64)
    R, Q = z.shape
    live = np.ones(R, bool) if live is None else live
    ce, g = np.zeros(R), np.zeros((R, Q))
    idx = np.nonzero(live)[0]
    zl, y = z[idx], np.asarray(targets)[idx]
    m = zl.max(axis=1, keepdims=True)
    lse = np.log(np.exp(zl - m).sum(axis=1)) + m[:, 0]
    eps = float(label_smoothing)
    ce[idx] = lse - (1.0 - eps) * zl[np.arange(len(idx)), y] - (eps / Q) * zl.sum(axis=1)
    gl = np.exp(zl - lse[:, None]) - eps / Q
    gl[np.arange(len(idx)), y] -= 1.0 - eps
    g[idx] = gl
    return ce, g


def loss_and_grad(logits, targets, weights=None, ignore_index=None, label_smoothing=0.0, norm="rows"):
    """-> (L, dL/dlogits (R, Q), the effective sum of weights), float64.  norm "weights" with a zero sum: L = 0 and a zero gradient."""
    w = effective_weights(np.asarray(targets), weights, ignore_index)
    ce, g = row_terms(logits, targets, label_smoothing, live=w != 0.0)
    mass = float(w.sum())
    N = float(len(w)) if norm == "rows" else mass
    if N == 0.0:
        return 0.0, np.zeros_like(g), mass
    return float((w * ce).sum() / N), g * (w / N)[:, None], mass
