"""Helpers shared by the parity tests (inputs regenerated from seeds via qpnet_amd.synth)."""
import numpy as np
from qpnet_amd import synth, harness


decode_batch = synth.decode_batch


def build_model(cfg, flat, device):
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**cfg.kwargs())
    sd = {k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(cfg, flat).items()}
    m.load_state_dict(sd)
    return m.to(device).eval()


def plan_query(m, B, attempt=0, n_cus=0):
    """qpn_decode_plan_query on the model's handle: the plan text of a call of B utterances (attempt 1: of its re-run after a give-up)."""
    import ctypes as C
    from qpnet_amd import _lib
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().qpn_decode_plan_query(m._handle, n_cus, B, attempt, buf, len(buf)))
    return buf.value.decode()


def run_giveup_child(which, env_name):
    """The fault-injection hooks exist only in the -DQPN_TESTING build of the library (qpnet_amd/libqpnet_hip_testing.so, built by
    __graft_entry__.build()): the scenario runs in a child process bound to that build (tests/giveup_child.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env[env_name] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "giveup_child.py"), which], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "GIVEUP_CHILD_OK " + which in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def distinct_rows_batch(cfg, batch_length, seed, max_length, batch_size, f0_lo=60.0):
    """A training batch whose rows DIFFER in everything a row owns, the way consecutive chunks of loaders.train_generator(batch_size=B) do: synth.train_inputs
    draws every row's features (another pitch contour, so another d, and another h) and waveform from streams of that row's own.  With the pitch floor
    pinned in every row's buffer the rows share the chunk geometry (receptive field, batch_length) without sharing ceil(max d) of the chunk itself.
    Returns x, h, t, d, blength like synth.train_inputs, checked to differ row by row."""
    x, h, t, d, b = synth.train_inputs(cfg, batch_length, seed, max_length, f0_lo=f0_lo, batch_size=batch_size, pin_f0_floor=True)
    for r in range(batch_size):
        for s in range(r):
            assert not np.array_equal(x[r], x[s]) and not np.array_equal(h[r], h[s]) and not np.array_equal(d[r], d[s])
    return x, h, t, d, b


def snap_to_grid(d, step=1.0 / 16, walk=0):
    """Pitch factors snapped to a multiple of `step` (a power of two: exact in float32 and float64).  On the 1/16 grid d * dilation is a multiple of 1/16,
    1/8, 1/4, 1/2 at the adaptive dilations 1, 2, 4, 8: exact .5 products -- where round-half-to-even (torch.round / np.round, the reference's rule) and
    round-half-away-from-zero (roundf) part -- and exact integers occur at every one of them.
    walk = +1 / -1: the factors are constant over a frame (110 samples), so a snapped frame meets a tie at dilation 1 only if its one value happens to end
    in .5; (n mod 16) * step is added to (subtracted from) sample n, which walks every frame through all sixteen residues.  Zeros (padding) stay zero."""
    d = np.asarray(d)
    g = np.round(d.astype(np.float64) / step) * step
    if walk:
        g = g + walk * step * (np.arange(d.shape[-1]) % 16)
    return np.where(d > 0, g, 0.0).astype(d.dtype)


def assert_grads_match_oracle(TO, cfg, flat, caches, dl, grad, a_scale=2e-5, a_rel=1e-4, kink_eps=4e-6, max_units=6, og=None):
    """Per-tensor comparison of a flat gradient with the numpy oracle's hand-derived backward: |g - ref| <= a_scale * max|ref (all tensors)| +
    a_rel * max|ref (this tensor)|.

    ReLU kinks: where a post-net pre-activation of the oracle's forward lies within fp32 reassociation error of zero (|s0| or |y0| < kink_eps;
    the logits of two correct fp32 implementations differ by ~1e-6), which side of the kink a unit falls on is decided by summation order, not
    by the algorithm -- and the side changes that row's gradient by a whole, small, term.  For those units (at most `max_units`) either side is
    accepted: the gradient must match the oracle's backward for ONE assignment of sides.  Returns the oracle gradient that matched.
    og: the oracle's backward for these caches and dl if the caller has it already (it is computed once per input and shared)."""
    import itertools
    import numpy as np
    offs, _ = cfg.param_offsets()

    def worst(og):
        scale = np.abs(og).max()
        bad = None
        for k, (o, shp) in offs.items():
            n = int(np.prod(shp))
            a, r = grad[o:o + n], og[o:o + n]
            e, bound = np.abs(a - r).max(), a_scale * scale + a_rel * np.abs(r).max()
            if not e <= bound and (bad is None or not e / bound <= bad[1]):          # (not <=: a NaN in the gradient is a mismatch, not a pass)
                bad = ("%s: err %.3e > bound %.3e" % (k, e, bound), e / bound)
        return bad

    if og is None:
        og = TO.backward(cfg, flat, caches, dl)
    bad = worst(og)
    if bad is None:
        return og
    units = [(b, key, idx) for b, c in enumerate(caches) for key in ("s0", "y0") for idx in zip(*np.nonzero(np.abs(c[key]) < kink_eps))]
    assert units, "grad mismatch in %s (no pre-activation within %.0e of a ReLU kink)" % (bad[0], kink_eps)
    saved = [caches[b][key][idx] for b, key, idx in units]
    if len(units) > max_units:
        # too many near-kink units to enumerate their sides (a full-size chunk has ~10 M post-net pre-activations, dozens of them within 4e-6 of
        # zero): ONE more oracle backward with every such unit on the other side measures what the ambiguity is worth per tensor, and twice that
        # (the units' contributions may partly cancel in the all-flipped sum) is added to the tensor's bound
        try:
            for (b, key, idx), v in zip(units, saved):
                caches[b][key][idx] = -np.sign(v) * kink_eps if v != 0 else kink_eps
            ogf = TO.backward(cfg, flat, caches, dl)
        finally:
            for (b, key, idx), v in zip(units, saved):
                caches[b][key][idx] = v
        scale = np.abs(og).max()
        for k, (o, shp) in offs.items():
            n = int(np.prod(shp))
            a, r = grad[o:o + n], og[o:o + n]
            bound = a_scale * scale + a_rel * np.abs(r).max() + 2.0 * np.abs(ogf[o:o + n] - r).max()
            assert np.abs(a - r).max() <= bound, "grad mismatch in %s: err %.3e > bound %.3e (incl. the allowance for %d near-kink units)" % (k, np.abs(a - r).max(), bound, len(units))
        return og
    try:
        for signs in itertools.product((1.0, -1.0), repeat=len(units)):
            for (b, key, idx), sg in zip(units, signs):
                caches[b][key][idx] = sg * kink_eps
            ogv = TO.backward(cfg, flat, caches, dl)
            if worst(ogv) is None:
                return ogv
    finally:
        for (b, key, idx), v in zip(units, saved):
            caches[b][key][idx] = v
    raise AssertionError("grad mismatch in %s, for every side of the %d near-kink units too" % (bad[0], len(units)))


def significant_elements(cfg, grads, thr=1e-2):
    """Boolean mask over the flat parameter vector: elements whose gradient is at least `thr` of their tensor's largest at EVERY step of `grads`
    (a list of flat reference gradients, one per Adam step).  Adam moves such an element by lr * m / sqrt(v) with a relative error of the order of
    the gradient's: two correct float32 runs agree on it tightly, whereas an element whose gradient is at noise level may move by a whole step in
    either direction (m / sqrt(v) = +-1 whatever the size of g)."""
    offs, _ = cfg.param_offsets()
    mask = np.ones(grads[0].size, dtype=bool)
    for g in grads:
        for k, (o, shp) in offs.items():
            n = int(np.prod(shp))
            a = np.abs(g[o:o + n])
            mask[o:o + n] &= a >= thr * max(float(a.max()), 1e-30)
    return mask


def assert_weights_after_adam(w, w_ref, lr, steps, tight=2e-6, frac=0.06, far=0.5, significant=None, sig_max=2e-6, sig_frac=0.0):
    """Final weights after `steps` Adam steps against a reference run.  Adam moves an element by ~lr per step whatever its gradient's size
    (m / sqrt(v)), so where a gradient is at fp32-noise level -- e.g. after a post-net pre-activation fell on the other side of a ReLU kink that lies
    within reassociation error of zero (util.assert_grads_match_oracle) -- two correct runs may disagree on a fraction of a step: all but `frac` of the
    elements agree to `tight`, none differs by more than `far` of the distance travelled.  (The per-step LOSS, north_star's criterion, is checked
    to 1e-4 next to this; gradients are compared with the oracle tensor by tensor in the autograd tests.)
    significant: mask of the elements whose reference gradient is well above noise at every step (significant_elements) -- those keep the
    tight bound of the original fixture check: none further than `sig_max` (all but `sig_frac` of them within `tight` when sig_frac > 0), and they
    must be at least a third of the elements, so that the tight check covers the bulk of the model."""
    import numpy as np
    d = np.abs(np.asarray(w, dtype=np.float64) - np.asarray(w_ref, dtype=np.float64))
    assert d.max() <= far * lr * steps, "max |dw| %.3e > %.3e" % (d.max(), far * lr * steps)
    assert (d > tight).mean() < frac, "%.2f %% of the elements differ by more than %.0e" % (100 * (d > tight).mean(), tight)
    if significant is not None:
        assert significant.shape == d.shape and significant.mean() >= 1.0 / 3, "only %.1f %% of the elements count as significant" % (100 * significant.mean())
        ds = d[significant]
        assert ds.max() <= sig_max, "an element with a significant gradient at every step differs by %.3e > %.1e" % (ds.max(), sig_max)
        if sig_frac > 0:
            assert (ds > tight).mean() <= sig_frac, "%.3f %% of the significant elements differ by more than %.0e" % (100 * (ds > tight).mean(), tight)


FORCED_SIGMOID_BIAS = (-120.0, -104.0, -100.0, -95.0, -90.0, -88.0, -60.0, -17.0, 17.0, 90.0)
FORCED_TANH_BIAS = (-90.0, -50.0, -44.0, -10.0, 10.0, 44.0, 50.0, 90.0)
LOGIT_BIAS = ((0, 150.0), (37, -150.0), (-1, 149.0))          # class, bias: the dominant class, the suppressed one, the runner-up (Q - 1) one logit below


def trained_like_weights(cfg, seed, gate_gain=1.0, post_gain=1.0, forced=False, logit_bias=False):
    """synth.make_weights(cfg, seed) moved from a freshly initialised network's regime (every gate in its linear region, a uniform softmax) to a trained one's:
    gate_gain multiplies every gate WEIGHT (the dilated convolutions and the auxiliary 1x1s of the sigmoid and tanh halves; the residual and skip 1x1s stay, so
    the residual stream stays O(1) and float32 reassociation noise stays at its gain-1 level -- a uniform gain does not do that), post_gain multiplies
    conv_post_2.weight (the logit spread), forced plants the landmark pre-activations as biases in the first and last fixed and the first and last adaptive
    layer (sigma exactly 0, a float32 denormal, exp just below and above float32 overflow, sigma exactly 1, tanh exactly +-1), on channels spread over the
    16-column tiles, and logit_bias makes class 0 dominant, class Q - 1 its runner-up one logit below and class 37 suppressed."""
    flat = synth.make_weights(cfg, seed).copy()
    offs, _ = cfg.param_offsets()
    W = {k: flat[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in offs.items()}
    for k, w in W.items():
        if k.endswith("weight") and ("sigmoid" in k or "tanh" in k):
            w *= np.float32(gate_gain)
    W["conv_post_2.weight"] *= np.float32(post_gain)
    if forced:
        C = cfg.n_resch
        LF, LA = len(cfg.dilationsF), len(cfg.dilationsA)
        layers = [("dilF_%s.%d.conv.bias", 0), ("dilF_%s.%d.conv.bias", LF - 1), ("dilA_%s.%d.conv%s.bias", 0), ("dilA_%s.%d.conv%s.bias", LA - 1)]
        for j, (fmt, i) in enumerate(layers):
            fixed = fmt.startswith("dilF")
            bs = W[fmt % (("sigmoid", i) if fixed else ("sigmoid", i, "C"))]
            bt = W[fmt % (("tanh", i) if fixed else ("tanh", i, "P"))]
            for n, v in enumerate(FORCED_SIGMOID_BIAS):
                bs[(7 * j + 3 * n) % C] = v
            for n, v in enumerate(FORCED_TANH_BIAS):
                bt[(5 * j + 1 + n) % C] = v
    if logit_bias:
        for q, v in LOGIT_BIAS:
            W["conv_post_2.bias"][q] = v
    return flat
