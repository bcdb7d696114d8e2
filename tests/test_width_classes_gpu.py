"""GPU parity at channel widths that are multiples of 16 but not of 32, and at the widths decode takes and training does not -- every width any other test or planner
sweep runs is a multiple of 32 (n_resch in {32, 64, 96, 128, 160, 256, 512}, n_skipch in {32, ..., 512}, n_quantize in {64, ..., 1024}), while train_plan accepts every
multiple of 16 and decode_program every multiple of the tile height 64 / (pad(K) / 16) ("width classes").  A kernel that dropped or double-counted
the tail 16-column block of a tile, the last column group of a weight gradient or the 16-row remainder of a 256-row block would pass everything else.

Training: oracle/train_oracle.py through the helpers of tests/test_train_edges_gpu.py at the project's small-chunk bounds, unchanged: logits 2e-5, loss 1e-4, gradients
a_scale 2e-5 / a_rel 1e-4.  Shallow 2 + 2-layer geometries, weights synth.make_weights(cfg, 7), input util.distinct_rows_batch(cfg, 300, 61, 2500, B) for B = 1 and 2
(T = 440, BL = 298, ceil(max d) 38 / 46).  One cached oracle per input, shared by every launch arrangement run on it; every case runs the autograd path (logits, loss, every
gradient tensor, check_status) and FusedTrainer.step (loss, gradient; the weights after the step too where the knobs are the default ones).  Every check prints its figures
before it asserts (lines starting with WIDTH; pytest -s / -rA shows them).  The numpy oracle's own float32 noise on these inputs: tools/edge_parity_noise.py --only widths
(MEASUREMENTS.md, "Width classes").

  (n_resch, n_skipch, n_quantize)   what it reaches
  (16, 16, 16)      the smallest accepted width of everything: one 16-block per operand, three of the four waves of a layer tile idle
  (48, 80, 48)      generic per-layer kernels with an odd number of 16-column tiles; post-net weight gradient in column groups of 40 padded to 48
  (80, 48, 96)      n_resch in (64, 128] and no power of two; the skip weight gradient (48 x 80) in column groups of 40; n_quantize a multiple of 32 but not of 64
  (112, 144, 80)    every width congruent to 16 mod 32; a 144 x 144 post-net gradient that no single column group fits
  (32, 16, 64)      TINY's stack with the smallest skip width
  (128, 112, 192)   the n_resch = 128 generic path with n_skipch and n_quantize off the 64 grid
  (64, 48, 32)      the paper-width stack (frame-rate aux path, persistent layer kernels, stack queue) with a narrow post-net; n_quantize < 64
  (64, 16, 256)     paper width and class count (the causal-table gradient as a contraction), smallest n_skipch
  (64, 272, 144)    n_skipch > 256 with a 16-row remainder block; n_quantize > 128 and no multiple of 128 (the causal-table gradient as an LDS histogram)

Decode: every case bit for bit against oracle/cpu_oracle.py, on the plan the library picks by itself and on the per-utterance cooperative kernel (QPN_DECODE_COOP=8):
teacher-forced per-step logits (the strong check: a greedy stream of random weights visits a dozen classes), a greedy batch of two ragged rows, and sampling where
n_quantize is 64, 128, 192 or 256.  last_decode_plan must be what qpn_decode_plan_query says and name the kind and group size stated here.

Refusals: a width outside the accepted set raises QpnError with a message that names the quantity, and computes nothing."""
import functools

import numpy as np
import pytest

from qpnet_amd import synth
from qpnet_amd.config import QPNetConfig
import util
import test_train_edges_gpu as E

gpu = pytest.mark.gpu

_SHALLOW = dict(dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1)
WSEED, DSEED = 7, 61
TRAIN_CSQ = ((16, 16, 16), (48, 80, 48), (80, 48, 96), (112, 144, 80), (32, 16, 64), (128, 112, 192), (64, 48, 32), (64, 16, 256), (64, 272, 144))
TRAIN_ONLY_CSQ = ((16, 16, 16), (32, 16, 64), (64, 16, 256))      # decode refuses them: n_resch 16 is no multiple of its tile height 64; n_skipch 16 is a multiple of neither 32 nor 64
_SQ0, _H0, _WG = {"QPN_STACK_QUEUE": "0"}, {"QPN_AUX_HOIST": "0"}, {"QPN_WGRAD_GENERIC": "1"}


def _cfg(csq):
    C, S, Q = csq
    return QPNetConfig(n_quantize=Q, n_resch=C, n_skipch=S, **_SHALLOW)


@functools.lru_cache(maxsize=None)
def _flat(csq):
    return synth.make_weights(_cfg(csq), WSEED)


@functools.lru_cache(maxsize=None)
def _input(csq, B):
    """the chunk of one geometry with the numpy oracle's forward, loss and gradient (E._with_oracle): computed once, shared by every arrangement, never written"""
    cfg = _cfg(csq)
    x, h, t, d, b = util.distinct_rows_batch(cfg, 300, DSEED, 2500, B)
    return E._with_oracle("w%d_%d_%d" % csq, x, h, t, d, b, cfg=cfg, flat=_flat(csq))


def _train_case(csq, B, env=None, tag=None):
    return dict(id="C%d-S%d-Q%d-B%d" % (csq + (B,)) + ("-" + tag if tag else ""), csq=csq, B=B, env=dict(env or {}))


TRAIN_CASES = (
    [_train_case(csq, B) for csq in TRAIN_CSQ for B in (1, 2)]
    + [_train_case(csq, B, env, tag) for csq in TRAIN_CSQ if csq[0] == 64 for env, tag in ((_SQ0, "queue0"), (_H0, "hoist0"), (_WG, "wgrad-generic")) for B in (1, 2)]
    + [_train_case(csq, B, _WG, "wgrad-generic") for csq in ((48, 80, 48), (112, 144, 80)) for B in (1, 2)]
)
assert len({c["id"] for c in TRAIN_CASES}) == len(TRAIN_CASES) == 18 + 18 + 4


def all_cases():
    """(label, input with its oracle) of every training input of this module: what tools/edge_parity_noise.py measures the oracle's own noise on"""
    for csq in TRAIN_CSQ:
        for B in (1, 2):
            yield "width C=%d S=%d Q=%d B=%d" % (csq + (B,)), _input(csq, B)


def _compare(label, o, logits, loss, grad):
    """E._compare under this module's tag: the figures (each also as a fraction of its bound), then the project's small-chunk bounds"""
    from oracle import train_oracle as TO
    e_lg = float(np.abs(logits - o.lg).max()) if logits is not None else float("nan")
    offs, _ = o.cfg.param_offsets()
    scale = np.abs(o.og).max()
    frac = max(np.abs(grad[a:a + int(np.prod(s))] - o.og[a:a + int(np.prod(s))]).max() / (2e-5 * scale + 1e-4 * np.abs(o.og[a:a + int(np.prod(s))]).max()) for a, s in offs.values())
    print("WIDTH %-44s logits %s  loss %.2e (%.3f of 1e-4)  grad %.2e of the largest, worst tensor %.3f of its bound"
          % (label, "%.2e (%.2f of 2e-5)" % (e_lg, e_lg / 2e-5) if logits is not None else "-" * 21, abs(loss - o.loss), abs(loss - o.loss) / 1e-4, np.abs(grad - o.og).max() / scale, frac))
    if logits is not None:
        assert logits.shape == o.lg.shape
        np.testing.assert_allclose(logits, o.lg, atol=2e-5, rtol=0)
    assert abs(loss - o.loss) < 1e-4
    return util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, grad, a_scale=2e-5, a_rel=1e-4, og=o.og)


# ---------------------------------------------------------------- the inputs and the oracle alone (no GPU)
def test_inputs_meet_the_conditions():
    """every training input: the stated chunk (T = 440, BL = 298, ceil(max d) 38 for one row and 46 for two), no more near-kink post-net units than
    util.assert_grads_match_oracle enumerates the sides of, and two rows whose own ceil(max d) differ"""
    for label, o in all_cases():
        B = o.x.shape[0]
        assert o.x.shape == (B, 440) and o.BL == 298 and o.maxd == (38 if B == 1 else 46), (label, o.x.shape, o.BL, o.maxd)
        assert o.lg.shape == (B, 298, o.cfg.n_quantize)
        units = int(sum((np.abs(c[key]) < 4e-6).sum() for c in o.caches for key in ("s0", "y0")))
        print("WIDTH %-32s near-kink post-net units %d" % (label, units))
        assert units <= 6, (label, units)
        own = [int(np.ceil(o.d[r]).max()) for r in range(B)]
        assert max(own) == o.maxd and (B == 1 or own[0] != own[1]), (label, own)


def test_the_oracle_tells_the_last_channel_apart():
    """What makes the cases discriminating, on the oracle alone: zeroing the LAST output channel of the last post-net 1x1, of an adaptive layer's skip 1x1, of a fixed
    layer's residual 1x1 and of the causal table -- the channels of the tail 16-block of every operand width -- each moves the logits by more than 2e-3, a hundred times
    the logits tolerance: a kernel that drops the tail block cannot pass."""
    from oracle import train_oracle as TO
    least = (np.inf, None)
    for csq in TRAIN_CSQ:
        o = _input(csq, 1)
        offs, _ = o.cfg.param_offsets()
        for key in ("conv_post_2.weight", "skipA_1x1.1.weight", "resF_1x1.0.weight", "causal.conv.weight"):
            a, shp = offs[key]
            f2 = o.flat.copy()
            w = f2[a:a + int(np.prod(shp))].reshape(shp)
            assert w[-1].any()
            w[-1] = 0
            moved = float(np.abs(TO.forward(o.cfg, f2, o.x, o.h, o.d, o.b)[0] - o.lg).max())
            print("WIDTH C=%d S=%d Q=%d: last output channel of %s (%d of them) zeroed: logits move by %.3f" % (csq + (key, shp[0], moved)))
            assert moved > 2e-3, (csq, key, moved)
            least = min(least, (moved, (csq, key)))
    print("WIDTH the least movement: %.3f at %s" % least)


# ---------------------------------------------------------------- training
@gpu
@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c["id"] for c in TRAIN_CASES])
def test_training_vs_oracle(case, cuda, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    o = _input(case["csq"], case["B"])
    E._autograd(case["id"] + " autograd", o, cuda, compare=_compare)
    E._fused(case["id"] + " fused step", o, cuda, weights_too=not case["env"], compare=_compare)


# ---------------------------------------------------------------- decode
SINGLE_CU_PAIR = (288, 304)        # n_resch (n_skipch = n_quantize = 64, 2 + 2 layers) either side of DecodeProgram::single_cu_ok: printed by tests/decode_program_sweep.cpp, held to it by tests/test_decode_program_cpu.py
DECODE_CSQ = (
    (72, 72, 64),        # decodes but does not train (n_resch no multiple of 16); Cp = 128
    (48, 80, 48),        # Cp = 64 != C, Sp = 128 != S
    (80, 64, 96),        # cooperative group size 2
    (80, 48, 96),        # the training case itself: n_skipch 48 is a multiple of both tile heights it meets (8 rows of K = n_resch, 16 rows of K = n_skipch)
    (112, 144, 80),      # group size 2
    (264, 136, 64),      # Cp = 512, tile height 2; group size 2
    (128, 112, 192),     # sampling at n_quantize 192
    (64, 48, 32),        # paper-width stack, not the specialised kernel (n_skipch, n_quantize differ)
    (64, 272, 144),      # the training case with n_skipch > 256: Sp = 512, two rows of the post-net matrices a tile
)
COOP_KNOB = 8
# group size of the per-utterance cooperative kernel under QPN_DECODE_COOP=8, by hand from qpn_coop_group_size (decode_plan.h): G doubles while every slice stays whole tiles
# -- n_resch / G a multiple of the tile height 64 / (Cp / 16) -- or a whole fraction of one tile (n_skipch, n_quantize).  The test asks qpn_decode_plan_query and holds it to this.
COOP_G = {(72, 72, 64): 1, (48, 80, 48): 1, (80, 64, 96): 2, (80, 48, 96): 1, (112, 144, 80): 2, (264, 136, 64): 2, (128, 112, 192): 2, (64, 48, 32): 1, (64, 272, 144): 1,
          (288, 64, 64): 8, (304, 64, 64): 8}
DECODE_ALL = DECODE_CSQ + tuple((C, 64, 64) for C in SINGLE_CU_PAIR)
_ONE_CU = "pipe rows=0 waves=0 x 0 (1 per group); one-cu rows=%d"
_UTTS = [(61, 5, 1.0), (62, 3, 1.0)]      # two ragged rows: 549 and 329 samples (test_aux_geometry_gpu._utts at U = 110)


@functools.lru_cache(maxsize=None)
def _decode_flat(csq):
    return synth.make_weights(_cfg(csq), WSEED)


@functools.lru_cache(maxsize=None)
def _decode_reference(csq):
    """the C oracle's results for one geometry, computed once and shared by both plans: teacher-forced logits and samples of one row, the greedy (and, where the class
    count allows it, the sampled) streams of the two ragged rows in input order"""
    from oracle import cpu_oracle
    cfg, flat = _cfg(csq), _decode_flat(csq)
    x, h, d, n = synth.decode_inputs(cfg, 4, 5, 1.0)
    teacher = np.random.RandomState(9).randint(0, cfg.n_quantize, size=n).astype(np.int64)
    ref = dict(forced=cpu_oracle.decode(cfg, flat, h, d, x, n, teacher=teacher, want_logits=True), teacher=teacher)
    bx, bh, bd, ns = util.decode_batch(cfg, _UTTS)
    maxd = int(np.nanmax(np.ceil(bd)))
    for mode in ("argmax", "sampling") if cfg.n_quantize in (64, 128, 192, 256) else ("argmax",):
        ref[mode] = tuple(cpu_oracle.decode(cfg, flat, bh[b], bd[b], bx[b], ns[b], maxd=maxd, mode=mode, seed=5, row=b)["samples"] for b in range(len(ns)))
    return ref


def test_the_sampled_reference_at_192_classes_reaches_the_last_class():
    """on the oracle alone: the sampled streams at n_quantize = 192 visit most classes, the last one (191, in the third 64-class group of a lane) among them"""
    ref = _decode_reference((128, 112, 192))
    seen = np.unique(np.concatenate(ref["sampling"]))
    print("WIDTH sampling at Q=192: %d classes visited, the largest %d" % (seen.size, seen.max()))
    assert seen.size >= 150 and seen.max() == 191 and seen.min() == 0


def _expected_plan(csq, plan, B):
    """what last_decode_plan must start with: the kind, and the group size of the cooperative kernel"""
    if plan == "coop":
        return "coop G=%d rows=%d" % (COOP_G[csq], B)
    if csq[0] == SINGLE_CU_PAIR[1]:
        return "coop G=8 rows=%d" % B           # one CU cannot hold the step state: the library takes the cooperative kernel by itself (n_resch / 16 = 19 is odd: G stops at 8)
    return _ONE_CU % B


@gpu
@pytest.mark.parametrize("plan", ["own", "coop"])
@pytest.mark.parametrize("csq", DECODE_ALL, ids=["C%d-S%d-Q%d" % c for c in DECODE_ALL])
def test_decode_vs_oracle(csq, plan, cuda, monkeypatch):
    import torch
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    monkeypatch.delenv("QPN_DECODE_COOP", raising=False)
    if plan == "coop":
        monkeypatch.setenv("QPN_DECODE_COOP", str(COOP_KNOB))
    cfg, flat, ref = _cfg(csq), _decode_flat(csq), _decode_reference(csq)
    m = util.build_model(cfg, flat, cuda)
    # teacher-forced per-step logits of one row, bitwise
    x, h, d, n = synth.decode_inputs(cfg, 4, 5, 1.0)
    out, logits = m._stream_logits(torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), d[None], torch.from_numpy(ref["teacher"][None]), n)
    lg = logits[0].cpu().numpy()
    assert lg.shape == (n, cfg.n_quantize)
    assert np.array_equal(lg.view(np.uint32), ref["forced"]["logits"].view(np.uint32)), "max abs diff %g" % np.abs(lg - ref["forced"]["logits"]).max()
    np.testing.assert_array_equal(out[0].cpu().numpy(), ref["forced"]["samples"])
    assert util.plan_query(m, 1).startswith(_expected_plan(csq, plan, 1)), util.plan_query(m, 1)
    # two ragged rows, greedy and (n_quantize in {64, 128, 192, 256}) sampled
    bx, bh, bd, ns = util.decode_batch(cfg, _UTTS)
    assert ns[0] > ns[1] and not bh[1, :, -1].any()
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    order = sorted(range(2), key=lambda i: ns[i])
    for mode in ("argmax", "sampling") if "sampling" in ref else ("argmax",):
        m.sampling_seed = 5
        outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode=mode)
        assert m.last_decode_plan == util.plan_query(m, 2) and m.last_decode_plan.startswith(_expected_plan(csq, plan, 2)), (m.last_decode_plan, util.plan_query(m, 2))
        for pos, i in enumerate(order):
            np.testing.assert_array_equal(outs[pos], ref[mode][i], err_msg="C=%d S=%d Q=%d %s %s: row %d" % (csq + (plan, mode, i)))


COOPB_CSQ = ((256, 256, 64), (256, 256, 128))      # 8 skip rows and 2 / 4 of 16 logit rows per workgroup of the batched cooperative kernel


@gpu
@pytest.mark.parametrize("csq", COOPB_CSQ, ids=["C%d-S%d-Q%d" % c for c in COOPB_CSQ])
def test_batched_cooperative_decode_with_few_logit_rows_vs_oracle(csq, cuda, oracle, monkeypatch):
    """decode_program plans "2 of 16 logit rows per workgroup" at n_quantize 64 (tests/decode_program_sweep.cpp, c256_q64): padding rows in the A operand of the
    last post-net contraction.  Three ragged utterances, greedy and sampled, against the oracle -- as test_batched_cooperative_decode_other_widths_vs_oracle."""
    import torch
    monkeypatch.setenv("QPN_DECODE_COOP", "32")
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    cfg, flat = _cfg(csq), _decode_flat(csq)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = util.decode_batch(cfg, [(61, 2, 1.0), (62, 3, 0.5), (63, 1, 1.5)])
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    for mode in ("argmax", "sampling"):
        m.sampling_seed = 5
        outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode=mode)
        assert m.last_decode_plan.startswith("coopb G=32 "), m.last_decode_plan
        o_outs = oracle.batch_fast_generate(cfg, flat, bx, bh, list(ns), bd, mode=mode, seed=5)
        assert [len(a) for a in outs] == sorted(ns)
        for i, (a, b) in enumerate(zip(outs, o_outs)):
            np.testing.assert_array_equal(a, b, err_msg="C=%d S=%d Q=%d %s: stream %d" % (csq + (mode, i)))


# ---------------------------------------------------------------- refusals
def _decode_once(m, cfg, cuda, mode="argmax"):
    import torch
    x, h, d, n = synth.decode_inputs(cfg, 2, 5, 1.0)
    m.sampling_seed = 5
    return m.batch_fast_generate(torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), [n], d[None], mode=mode)[0], (x, h, d, n)


def _train_once(m, cfg, cuda):
    x, h, t, d, b = util.distinct_rows_batch(cfg, 300, DSEED, 2500, 1)
    xt, ht, dt, bt = E._to(cuda, x, h, d, b)
    return m.train()(xt, ht, dt, bt)


@gpu
@pytest.mark.parametrize("C", [8, 24, 40])
def test_decode_refuses_a_stack_width_off_its_tile_height(C, cuda):
    """n_resch 8 and 24 (tile heights 64 and 32) and 40 (16): no whole number of tiles"""
    from qpnet_amd._lib import QpnError
    cfg = _cfg((C, 64, 64))
    m = util.build_model(cfg, synth.make_weights(cfg, WSEED), cuda)
    with pytest.raises(QpnError, match="n_resch %"):
        _decode_once(m, cfg, cuda)


@gpu
@pytest.mark.parametrize("csq", TRAIN_ONLY_CSQ, ids=["C%d-S%d-Q%d" % c for c in TRAIN_ONLY_CSQ])
def test_decode_refuses_the_widths_that_only_train(csq, cuda):
    """(16, 16, 16): n_resch; (32, 16, 64) and (64, 16, 256): n_skipch 16 is a multiple of neither the stack's tile height (32, 16: it is at 64 channels) nor its own (64)"""
    from qpnet_amd._lib import QpnError
    cfg = _cfg(csq)
    m = util.build_model(cfg, _flat(csq), cuda)
    with pytest.raises(QpnError, match="n_skipch %"):
        _decode_once(m, cfg, cuda)


@gpu
def test_training_refuses_72_channels_and_the_module_still_decodes(cuda, oracle):
    from qpnet_amd._lib import QpnError
    csq = (72, 72, 64)
    cfg, flat = _cfg(csq), _decode_flat(csq)
    m = util.build_model(cfg, flat, cuda)
    with pytest.raises(QpnError, match="n_resch, n_skipch, n_quantize multiples of 16"):
        _train_once(m, cfg, cuda)
    y, (x, h, d, n) = _decode_once(m.eval(), cfg, cuda)
    np.testing.assert_array_equal(y, oracle.decode(cfg, flat, h, d, x, n)["samples"])


@gpu
def test_training_refuses_144_channels(cuda):
    """n_resch > 128 selects the GEMM step, which needs multiples of 32"""
    from qpnet_amd._lib import QpnError
    cfg = _cfg((144, 144, 64))
    m = util.build_model(cfg, synth.make_weights(cfg, WSEED), cuda)
    with pytest.raises(QpnError, match="GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32"):
        _train_once(m, cfg, cuda)


@gpu
def test_the_gemm_step_refuses_a_width_of_the_tile_path(cuda, monkeypatch):
    from qpnet_amd._lib import QpnError
    monkeypatch.setenv("QPN_TRAIN_GEMM", "1")
    csq = (80, 48, 96)
    cfg = _cfg(csq)
    m = util.build_model(cfg, _flat(csq), cuda)
    with pytest.raises(QpnError, match="GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32"):
        _train_once(m, cfg, cuda)


@gpu
@pytest.mark.parametrize("csq", [(48, 80, 48), (112, 144, 80)], ids=["Q48", "Q80"])
def test_sampling_refuses_a_class_count_off_the_64_grid(csq, cuda):
    from qpnet_amd._lib import QpnError
    cfg = _cfg(csq)
    m = util.build_model(cfg, _decode_flat(csq), cuda)
    with pytest.raises(QpnError, match="n_quantize in"):
        _decode_once(m, cfg, cuda, mode="sampling")
