"""float64 numpy specification of qpn_score_logits' records (include/qpnet_hip.h), shared by the CPU and GPU suites.

Per row with logits l and target t:
    nll     = log sum_q exp(l_q) - l_t                      (+inf when t is outside [0, Q))
    entropy = -sum_q p_q log p_q, p = softmax(l), with 0 log 0 = 0 (a class at -inf contributes nothing)
    argmax  = the LOWEST index among the maxima
    rank    = #{q : l_q > l_t}, strict, on the floats as given   (Q when t is outside [0, Q))
"""
import numpy as np


def score(logits, targets):
    """logits (..., Q) float, targets (...) int -> (nll f64, entropy f64, argmax i32, rank i32), each of the leading shape.  The comparisons are made on
    the array as given (float32 logits are compared as float32 values: the widening to float64 is exact)."""
    lg = np.asarray(logits)
    Q = lg.shape[-1]
    l = lg.astype(np.float64).reshape(-1, Q)
    t = np.asarray(targets).astype(np.int64).reshape(-1)
    assert t.shape[0] == l.shape[0]
    m = l.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.exp(l - m)
        se = e.sum(axis=1)
        lse = np.log(se) + m[:, 0]
        p = e / se[:, None]
        plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    entropy = -plogp.sum(axis=1)
    argmax = np.argmax(l, axis=1).astype(np.int32)                      # (numpy returns the first occurrence)
    ok = (t >= 0) & (t < Q)
    lt = l[np.arange(l.shape[0]), np.where(ok, t, 0)]
    nll = np.where(ok, lse - lt, np.inf)
    rank = np.where(ok, (l > lt[:, None]).sum(axis=1), Q).astype(np.int32)
    shp = lg.shape[:-1]
    return nll.reshape(shp), entropy.reshape(shp), argmax.reshape(shp), rank.reshape(shp)
