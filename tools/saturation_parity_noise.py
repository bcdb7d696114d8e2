"""The numpy oracle's own float32 noise on every training input of tests/test_saturation_gpu.py (CPU only), the sibling of tools/edge_parity_noise.py for the
saturated regime: per input, what regime it is in (loss, logit spread, the share of saturated gates, how many sigma are exactly 0 / a float32 denormal) and
the distance between the float32 oracle and the same oracle under train_oracle.precision(np.float64) on the float32 run's ReLU sides, as a fraction of the
tests' bounds -- logits 2e-5 * max(1, max|logits|), loss 1e-4 * max(1, |loss|), per gradient tensor its bound in util.assert_grads_match_oracle (a_scale
2e-5, a_rel 1e-4) -- and the number of post-net units within kink_eps = 4e-6 of a ReLU kink.  The bounds must be at least 4 x the noise: exits non-zero
where a fraction is above 0.25 or more than 6 units sit on a kink.
    python tools/saturation_parity_noise.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    import saturation_common as S
    worst = [0.0, 0.0, 0.0, 0]
    for cfgname, scenario in S.TRAIN_CASES:
        o = S.train_input(cfgname, scenario)
        g, s, f, units = S.gate_stats(o), S.softmax_stats(o), S.f64_distance(o), S.near_kink_units(o)
        print("%-5s %-6s T %4d BL %2d  loss %7.2f  spread %5.1f  p_max %.3f  saturated sigma %.3f |tanh| > .999 %.3f  sigma == 0 %5d denormal %5d  |  logits %.3f of the bound  "
              "loss %.4f  worst gradient tensor %.3f (%s)  near-kink units %d" %
              (cfgname, scenario, o.x.shape[1], o.BL, o.loss, s["spread"], s["p_max"], g["sat_sigma"], g["sat_tanh"], g["zero"], g["denormal"],
               f["logits"], f["loss"], f["grad"], f["tensor"], units))
        assert f["finite"]
        worst = [max(worst[0], f["logits"]), max(worst[1], f["loss"]), max(worst[2], f["grad"]), max(worst[3], units)]
    print("worst: logits %.3f of the bound, loss %.4f, gradient %.3f, near-kink units %d" % tuple(worst))
    return 0 if max(worst[:3]) <= 0.25 and worst[3] <= 6 else 1


if __name__ == "__main__":
    sys.exit(main())
