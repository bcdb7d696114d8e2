"""What makes tests/test_saturation_gpu.py mean something, asserted on the oracles alone (no GPU): the inputs of tests/saturation_common.py ARE in the regime
a trained network lives in -- sigma exactly 0, a float32 denormal and exactly 1, tanh exactly +-1, a softmax whose target underflows -- their gradient is
finite, few enough post-net units sit on a ReLU kink for util.assert_grads_match_oracle to enumerate, and the two oracles (the numpy training oracle in
float64 and the C streaming spec with its exp-argument clamps, which the decode kernels are bit-exact against) agree there as well."""
import functools

import numpy as np
import pytest

import saturation_common as S
import util

GEOS = ("paper", "c128", "tiny")


def test_trained_like_weights_change_what_they_say_and_nothing_else():
    from qpnet_amd import synth
    cfg, seed = S.CFGS["paper"]
    base = synth.make_weights(cfg, seed)
    offs, _ = cfg.param_offsets()
    assert np.array_equal(util.trained_like_weights(cfg, seed), base)
    full = util.trained_like_weights(cfg, seed, gate_gain=4.0, post_gain=40.0, forced=True, logit_bias=True)
    LF, LA = len(cfg.dilationsF), len(cfg.dilationsA)
    planted = {"dilF_sigmoid.0.conv.bias", "dilF_tanh.0.conv.bias", "dilF_sigmoid.%d.conv.bias" % (LF - 1), "dilF_tanh.%d.conv.bias" % (LF - 1),
               "dilA_sigmoid.0.convC.bias", "dilA_tanh.0.convP.bias", "dilA_sigmoid.%d.convC.bias" % (LA - 1), "dilA_tanh.%d.convP.bias" % (LA - 1)}
    for k, (o, shp) in offs.items():
        n = int(np.prod(shp))
        a, b = full[o:o + n], base[o:o + n]
        if k.endswith("weight") and ("sigmoid" in k or "tanh" in k):
            assert np.array_equal(a, b * np.float32(4.0)), k
        elif k == "conv_post_2.weight":
            assert np.array_equal(a, b * np.float32(40.0)), k
        elif k == "conv_post_2.bias":
            assert (a[0], a[37], a[-1]) == (150.0, -150.0, 149.0) and (a != b).sum() == 3
        elif k in planted:
            vals = util.FORCED_SIGMOID_BIAS if "sigmoid" in k else util.FORCED_TANH_BIAS
            ch = np.nonzero(a != b)[0]
            assert sorted(a[ch]) == sorted(vals), k
            assert "tanh" in k or len({c // 16 for c in ch}) >= 2, k    # more than one 16-column tile
        else:
            assert np.array_equal(a, b), k                              # residual / skip 1x1s, the other biases, the tables: as initialised


def test_a_nan_gradient_does_not_pass_the_gradient_comparison():
    """util.assert_grads_match_oracle compared with `err > bound`, which a NaN never satisfies: a gradient with NaNs in it passed (seen on the GPU with
    tr_gate_bwd's sigma guard removed: 57 edge tests passed on an all-NaN gradient).  The oracle's own gradient passes; one NaN, or one inf, in it does not."""
    from oracle import train_oracle as TO
    o = S.train_input("tiny", "forced")
    util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, o.og.copy(), og=o.og)
    offs, _ = o.cfg.param_offsets()
    for bad in (np.nan, np.inf):
        g = o.og.copy()
        g[offs["resF_1x1.0.weight"][0] + 5] = bad
        with pytest.raises(AssertionError, match="grad mismatch in resF_1x1.0.weight"):
            util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, g, og=o.og)


@pytest.mark.parametrize("scenario", ["forced", "all"])
@pytest.mark.parametrize("cfgname", GEOS)
def test_forced_biases_reach_the_landmarks(cfgname, scenario):
    o = S.train_input(cfgname, scenario)
    g = S.gate_stats(o)
    print("SAT %-5s %-6s sigma == 0: %d  denormal: %d  == 1: %d  |tanh| == 1: %d" % (cfgname, scenario, g["zero"], g["denormal"], g["one"], g["tanh_one"]))
    assert g["zero"] >= 100 and g["denormal"] >= 100 and g["one"] >= 100 and g["tanh_one"] >= 100, g
    assert np.isfinite(o.lg).all() and np.isfinite(o.loss) and np.isfinite(o.og).all()


@pytest.mark.parametrize("scenario", ["peaked", "all"])
@pytest.mark.parametrize("cfgname", GEOS + ("wide",))
def test_peaked_softmax_underflows_the_target_and_meets_the_top_two(cfgname, scenario):
    o = S.train_input(cfgname, scenario)
    s = S.softmax_stats(o)
    Q = o.cfg.n_quantize
    assert s["p_target"].size == 2 * S.BL == 162
    print("SAT %-5s %-6s loss %.1f  spread %.0f  rows with p(target) < 1e-30: %d  target dominant: %d  runner-up: %d" %
          (cfgname, scenario, o.loss, s["spread"], (s["p_target"] < 1e-30).sum(), s["dominant"], s["runner_up"]))
    assert (s["p_target"] < 1e-30).sum() >= 100 and s["dominant"] >= 2 and s["runner_up"] >= 2
    for r in range(2):                                                  # every row of the batch has the three planted classes among its targets
        assert {0, Q - 1, 37} <= set(o.t[r, -S.BL:].tolist())
    assert np.isfinite(o.og).all()


@pytest.mark.parametrize("cfgname", GEOS)
def test_gate_gain_saturates_a_good_share_of_the_gates(cfgname):
    g = S.gate_stats(S.train_input(cfgname, "gates"))
    print("SAT %-5s gates  saturated sigma %.3f  |tanh| > 0.999 %.3f" % (cfgname, g["sat_sigma"], g["sat_tanh"]))
    assert g["sat_sigma"] >= 0.05 and g["sat_tanh"] >= 0.25


@pytest.mark.parametrize("cfgname,scenario", S.TRAIN_CASES)
def test_few_enough_units_on_a_relu_kink(cfgname, scenario):
    assert S.near_kink_units(S.train_input(cfgname, scenario)) <= 6


@pytest.mark.parametrize("cfgname,scenario", [c for c in S.TRAIN_CASES if c[0] != "wide"])
def test_streaming_spec_agrees_with_the_float64_training_oracle(cfgname, scenario, oracle):
    """oracle/qpnet_oracle.c teacher-forced on the chunk (float32, its clamped exp) against oracle/train_oracle.py in float64: the only thing that anchors the
    streaming spec's saturated behaviour to an independent implementation"""
    from oracle import train_oracle as TO
    o = S.train_input(cfgname, scenario)
    with TO.precision(np.float64):
        lg64, _ = TO.forward(o.cfg, o.flat.astype(np.float64), o.x, o.h.astype(np.float64), o.d, o.b)
    for r in range(o.x.shape[0]):
        lc = oracle.forward(o.cfg, o.flat, o.x[r], o.h[r], o.d[r], o.BL)
        bound = 2e-5 * max(1.0, float(np.abs(lg64[r]).max()))
        e = float(np.abs(lc - lg64[r]).max())
        print("SAT %-5s %-6s row %d: |C oracle - float64 numpy oracle| %.2e = %.3f of the bound" % (cfgname, scenario, r, e, e / bound))
        assert np.isfinite(lc).all() and e <= bound
        assert np.array_equal(lc.argmax(1), lg64[r].argmax(1))


@functools.lru_cache(maxsize=None)
def _decode_rows(cfgname, kind, mode):
    """per row of the ragged batch: the C oracle's stream and the logits it was drawn from"""
    from oracle import cpu_oracle
    cfg = S.DECODE_CFGS[cfgname]
    bx, bh, bd, ns = util.decode_batch(cfg, S.DECODE_UTTS)
    maxd = int(np.nanmax(np.ceil(bd)))
    return [cpu_oracle.decode(cfg, S.decode_weights(cfgname, kind), bh[i], bd[i], bx[i], ns[i], maxd=maxd, want_logits=True, mode=mode, seed=5, row=i) for i in range(len(ns))]


@pytest.mark.parametrize("cfgname", list(S.DECODE_CFGS))
def test_decode_inputs_reach_the_clamp_and_a_draw_that_is_not_the_argmax(cfgname, oracle):
    assert [len(r["samples"]) for r in _decode_rows(cfgname, "clamped", "argmax")] == [439, 329]
    lg = np.concatenate([r["logits"] for r in _decode_rows(cfgname, "clamped", "argmax")]).astype(np.float64)
    clamped = float(((lg.max(1) - lg.min(1)) > 87).mean())
    rows = _decode_rows(cfgname, "stochastic", "sampling")
    lg = np.concatenate([r["logits"] for r in rows]).astype(np.float64)
    s = np.concatenate([r["samples"] for r in rows])
    p = np.exp(lg - lg.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    off, peaked = float((s != lg.argmax(1)).mean()), float((p.max(1) >= 0.5).mean())
    print("SAT decode %-5s spread > 87 at %.2f of the steps; draw != argmax at %.2f, largest probability >= 0.5 at %.2f" % (cfgname, clamped, off, peaked))
    assert np.isfinite(lg).all() and clamped >= 0.5 and off >= 0.25 and peaked >= 0.25
    for kind in ("clamped", "stochastic"):
        for r in _decode_rows(cfgname, kind, "argmax"):
            assert len(np.unique(r["samples"])) >= 5                    # no constant stream
            assert np.array_equal(r["samples"], r["logits"].argmax(1))
