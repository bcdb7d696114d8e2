"""The numpy oracle's own float32 noise on every input of tests/test_train_edges_gpu.py, of tests/test_aux_geometry_gpu.py and of tests/test_width_classes_gpu.py (CPU only; --only edges|aux|widths): per input, the distance between the float32 oracle and
the same oracle under train_oracle.precision(np.float64) evaluated on the float32 run's ReLU sides (the technique of tests/f64_child.py) -- logits, loss,
and per gradient tensor as a fraction of that tensor's bound in util.assert_grads_match_oracle (a_scale 2e-5, a_rel 1e-4) -- and the number of post-net
units within kink_eps = 4e-6 of a ReLU kink (at most max_units = 6 can be enumerated).  The tests' bounds must be at least 4 x these figures.
    python tools/edge_parity_noise.py [--only edges|aux|widths]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    from oracle import train_oracle as TO
    import itertools
    import test_train_edges_gpu as E
    import test_aux_geometry_gpu as X
    import test_width_classes_gpu as W
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    worst = [0.0, 0.0, 0.0, 0]
    for label, o in itertools.chain(E.all_cases() if only in (None, "edges") else (), X.all_cases() if only in (None, "aux") else (), W.all_cases() if only in (None, "widths") else ()):
        with TO.precision(np.float64):
            f64 = o.flat.astype(np.float64)
            lg64, c64 = TO.forward(o.cfg, f64, o.x, o.h.astype(np.float64), o.d, o.b)
            loss64, dl64 = TO.ce_loss(lg64, o.t[:, -o.BL:])
            for c, c32 in zip(c64, o.caches):               # the float32 run's sides
                for key in ("s0", "y0"):
                    v = c[key].copy()
                    flip = (v > 0) != (c32[key] > 0)
                    v[flip] = np.where(c32[key][flip] > 0, 1e-300, -1e-300)
                    c[key] = v
            g64 = TO.backward(o.cfg, f64, c64, dl64)
        offs, _ = o.cfg.param_offsets()
        scale = np.abs(g64).max()
        frac, name = max((np.abs(o.og[a:a + int(np.prod(s))] - g64[a:a + int(np.prod(s))]).max() / (2e-5 * scale + 1e-4 * np.abs(g64[a:a + int(np.prod(s))]).max()), k)
                         for k, (a, s) in offs.items())
        units = int(sum((np.abs(c[key]) < 4e-6).sum() for c in o.caches for key in ("s0", "y0")))
        e_lg, e_loss = float(np.abs(o.lg - lg64).max()), abs(o.loss - loss64)
        print("%-40s T %4d BL %3d maxd %2d  |logits32 - logits64| %.2e (%.2f of 2e-5)  loss %.1e  worst gradient tensor %.3f of its bound (%s)  near-kink units %d"
              % (label, o.x.shape[1], o.BL, o.maxd, e_lg, e_lg / 2e-5, e_loss, frac, name, units))
        worst = [max(worst[0], e_lg / 2e-5), max(worst[1], e_loss / 1e-4), max(worst[2], frac), max(worst[3], units)]
    print("worst: logits %.2f of the bound, loss %.3f, gradient %.3f, near-kink units %d" % tuple(worst))
    return 0 if max(worst[:3]) <= 0.25 and worst[3] <= 6 else 1


if __name__ == "__main__":
    sys.exit(main())
