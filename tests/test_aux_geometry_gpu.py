"""GPU parity at n_aux and upsampling_factor other than 39 and 110 -- the two constructor arguments that decide which training and decode kernels run and
how they pad and index ("Which kernels a geometry selects").

Training: oracle/train_oracle.py through the helpers of tests/test_train_edges_gpu.py at the project's small-chunk bounds (logits 2e-5, loss 1e-4, gradients
a_scale 2e-5 / a_rel 1e-4; a_rel 2e-4 on the wide stacks, as test_default_geometry_vs_reference has it).  One cached oracle per input, shared by every launch
arrangement run on it; every case runs the autograd path (logits, loss, every gradient tensor, check_status) and FusedTrainer.step (loss, gradient; the
weights after the step too where the knobs are the default ones).  Decode: every kernel family bit for bit against oracle/cpu_oracle.py, two rows of unequal
length so that h arrives zero padded.  The numpy oracle's own float32 noise on the training inputs: tools/edge_parity_noise.py (MEASUREMENTS.md).

Which case lands on which side of each selection condition (A = n_aux, U = upsampling_factor, C = n_resch; Ap = pad4(A), Ktp = pad16(2C + Ap)):
  frame-rate aux path ("hoist": C == 64, U >= 16, A <= 64)     taken: a-A* default knobs, c-U16 / U17 / U80 / U240, d-A28-U80, d-A64-U16
                                                                 refused by A: b-A65, b-A80, d-A65-U16; by U: c-U1, c-U5, c-U15; by the knob: *-hoist0; by C: e-*, f-*
  persistent layer kernels, stack queue (Ktp == 176 or hoist)   Ktp == 176 without the hoist: a-A33-hoist0 (12 padding columns), a-A48-hoist0 (none), c-U1 / U5 / U15,
                                                                 c-U*-hoist0; generic per-layer kernels: a-A2 / A4 / A28 / A49 / A64-hoist0 (Ktp 144 ... 192), b-A65, b-A80;
                                                                 a launch per layer and the generic weight-gradient kernel on both: a-A33 / a-A28 with QPN_STACK_QUEUE=0, QPN_WGRAD_GENERIC=1
  aux_proj_block's LDS and copy loop, k_aux_tail's L*A + U grid  A = 2 (the least synth makes: uv, f0), 4 (Ap == A), 28, 33, 48, 49, 64 (the limit); U = 16 (the lower
                                                                 edge; q0 % U != 0 asserted in test_inputs_meet_the_conditions), 17, 80, 240 (more than k_aux_tail's 128 threads)
  up_bwd_body (not hoisted): float4 loop / scalar tail / pass 2  nq 0 tail 2 (A2), nq 1 (A4), nq 7 (A28), nq 8 tail 1 (A33), nq 12 (A48), nq 12 tail 1 (A49), nq 16 (A64),
                                                                 second pass with na = 1 (A65) and na = 16 (A80); k_up_bwd's j < U stride: U = 240 > 128 (c-U240-hoist0), U = 1
  per-row offsets (b*A + a)*F, DPA / PA at l*B + b               d-* with two and three distinct rows, e-* and f-* with two
  generic geometry (C = 128)                                     e-A28-U80, e-A65-U110
  wide stacks (train_gemm.hip; K1 = 2C + pad32(Ap))              f-C160-S96 (a partial gate tile, the 2C boundary inside a 128-column tile, a partial Sg tile), f-C256-S320 (Sg = 384);
                                                                 Ap 20 inside 32 (A17), Ap == pad32 (A32), Ap 40 inside 64 (A39), Ap 68 inside 96 (A65); f-bl-*: BL and N1 - s_out of
                                                                 the first layer at residues 0, 1, 127 of the 128-row tile, B * BL < 64 (empty time splits of k_gemm_tn) at BL = 1
  decode: R = Ap/16 lanes per row in k_fold_bias / k_aux_project  R 1 (A2, A16), 2 (A17, A28), 4 (A39, A64), 8 (A65), exact and padded ends; fr = ut / U, j = ut - fr*U in each of the
                                                                 one-CU, interpreter, pipe, coop and coopb kernels at U = 1, 5, 16, 80, 240; the h stride (b*A + i)*F + f with B = 2 ragged rows"""
import dataclasses
import functools

import numpy as np
import pytest

from cases import AUX_CASES
from qpnet_amd import synth
from qpnet_amd.config import PAPER, QPNetConfig
import util
import test_train_edges_gpu as E
import test_decode_gpu as D

gpu = pytest.mark.gpu

_SHALLOW = dict(dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1)
GEOS = {   # geometry (n_aux and upsampling_factor are the case's), weight seed
    "paper": (PAPER, 21),
    "c128": (E.C128, 7),
    "w160": (QPNetConfig(n_resch=160, n_skipch=96, **_SHALLOW), 7),
    "w256": (QPNetConfig(n_resch=256, n_skipch=320, **_SHALLOW), 7),
}
# data seed of util.distinct_rows_batch(cfg, 300, seed, 2500, B, f0_lo) per input: 61 (62 for three rows, as in test_train_edges_gpu) unless the oracle's forward has
# more than the 6 post-net units within kink_eps = 4e-6 of a ReLU kink that util.assert_grads_match_oracle enumerates the sides of (test_inputs_meet_the_conditions)
SEEDS = {("paper", 65, 16, 2, None, 60.0): 63, ("paper", 64, 16, 2, None, 60.0): 63,       # seed 61: both rows' own ceil(max d) are the batch's
         ("w160", 39, 110, 1, 1, 66.0): 64, ("w160", 39, 110, 1, 127, 66.0): 64, ("w160", 39, 110, 1, 128, 66.0): 64}      # the first seed whose chunk holds the pinned pitch floor (ceil(max d) = 42)


def _case(group, geo, A, U, B=1, BL=None, env=None, f0_lo=60.0, tag=None):
    env = dict(env or {})
    name = "%s-%sA%d-U%d" % (group, "" if geo == "paper" else {"c128": "", "w160": "C160-S96-", "w256": "C256-S320-"}[geo], A, U)
    name += ("-B%d" % B if B > 1 else "") + ("-BL%d" % BL if BL else "") + ("-" + tag if tag else "")
    return dict(id=name, key=(geo, A, U, B, BL, f0_lo), env=env, weights_too=not env and group in "abc", wide=geo.startswith("w"))


_H0, _SQ0, _WG = {"QPN_AUX_HOIST": "0"}, {"QPN_STACK_QUEUE": "0"}, {"QPN_WGRAD_GENERIC": "1"}
A_VALUES = (2, 4, 28, 33, 48, 49, 64)
U_VALUES = (1, 5, 15, 16, 17, 80, 240)
BOTH = ((28, 80), (65, 16), (64, 16))
WIDE_AU = ((17, 120), (32, 110), (39, 110), (65, 80))
WIDE_BL = (1, 127, 128)            # test_wide_stack_lengths_cover_the_tile_residues
WIDE_F0_LO = 66.0                  # ceil(max d) = 42: N1 - s_out of the first layer = 3 * 42 + 3 + BL - 1 = 128 + BL
CASES = (
    [_case("a", "paper", A, 110) for A in A_VALUES]
    + [_case("a", "paper", A, 110, env=_H0, tag="hoist0") for A in A_VALUES]
    + [_case("a", "paper", A, 110, env=env, tag=tag) for A in (33, 28) for env, tag in ((_SQ0, "queue0"), (_WG, "wgrad-generic"))]
    + [_case("b", "paper", A, 110) for A in (65, 80)]
    + [_case("c", "paper", 39, U) for U in U_VALUES]
    + [_case("c", "paper", 39, U, env=_H0, tag="hoist0") for U in (16, 80, 240)]
    + [_case("d", "paper", A, U, B=2) for A, U in BOTH] + [_case("d", "paper", 28, 80, B=3)]
    + [_case("e", "c128", A, U, B=B) for A, U in ((28, 80), (65, 110)) for B in (1, 2)]
    + [_case("f", geo, A, U, B=B) for geo in ("w160", "w256") for A, U in WIDE_AU for B in (1, 2)]
    + [_case("f-bl", "w160", 39, 110, BL=BL, f0_lo=WIDE_F0_LO) for BL in WIDE_BL]
)
assert len({c["id"] for c in CASES}) == len(CASES)


def _cfg(geo, A, U):
    return dataclasses.replace(GEOS[geo][0], n_aux=A, upsampling_factor=U)


@functools.lru_cache(maxsize=None)
def _flat(geo, A, U):
    return synth.make_weights(_cfg(geo, A, U), GEOS[geo][1])


@functools.lru_cache(maxsize=None)
def _input(key):
    """the chunk of one case with the numpy oracle's forward, loss and gradient (E._with_oracle): computed once, shared by every arrangement, never written"""
    geo, A, U, B, BL, f0_lo = key
    cfg = _cfg(geo, A, U)
    x, h, t, d, b = util.distinct_rows_batch(cfg, 300, SEEDS.get(key, 62 if B == 3 else 61), 2500, B, f0_lo=f0_lo)
    if BL is not None:
        assert BL <= int(b[0])
        b = np.full_like(b, BL)
    return E._with_oracle(geo, x, h, t, d, b, cfg=cfg, flat=_flat(geo, A, U))


def all_cases():
    """(label, input with its oracle) of every training input of this module: what tools/edge_parity_noise.py measures the oracle's own noise on"""
    seen = set()
    for c in CASES:
        if c["key"] not in seen:
            seen.add(c["key"])
            yield "aux %s" % c["id"], _input(c["key"])


def _compare_wide(label, o, logits, loss, grad):
    """E._compare with the wide stacks' a_rel 2e-4 (test_default_geometry_vs_reference)"""
    from oracle import train_oracle as TO
    e_lg = float(np.abs(logits - o.lg).max()) if logits is not None else float("nan")
    print("AUX  %-44s logits %.2e  loss %.2e  grad %.2e of the largest" % (label, e_lg, abs(loss - o.loss), np.abs(grad - o.og).max() / np.abs(o.og).max()))
    if logits is not None:
        assert logits.shape == o.lg.shape
        np.testing.assert_allclose(logits, o.lg, atol=2e-5, rtol=0)
    assert abs(loss - o.loss) < 1e-4
    return util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, grad, a_scale=2e-5, a_rel=2e-4, og=o.og)


# ---------------------------------------------------------------- the inputs and the oracle alone (no GPU)
def _pairs():
    return sorted({c["key"][1:3] for c in CASES})


def test_the_oracle_tells_the_last_feature_and_the_last_tap_apart():
    """What makes the cases discriminating: for every (n_aux, upsampling_factor) used, on the paper-size widths, zeroing feature column A - 1 of h and zeroing
    upsampling weight U - 1 each move the oracle's logits by far more than the 2e-5 tolerance -- a kernel that drops the tail of the aux row or the last tap of
    the upsampling kernel cannot pass."""
    from oracle import train_oracle as TO
    for A, U in _pairs():
        cfg, flat = _cfg("paper", A, U), _flat("paper", A, U)
        x, h, t, d, b = util.distinct_rows_batch(cfg, 300, 61, 2500, 1)
        lg, _ = TO.forward(cfg, flat, x, h, d, b)
        h2 = h.copy()
        h2[:, A - 1, :] = 0
        w_off = cfg.param_offsets()[0]["upsampling.conv.weight"][0]
        f2 = flat.copy()
        f2[w_off + U - 1] = 0
        moved_h = np.abs(TO.forward(cfg, flat, x, h2, d, b)[0] - lg).max()
        moved_w = np.abs(TO.forward(cfg, f2, x, h, d, b)[0] - lg).max()
        print("AUX  A=%d U=%d: feature column A-1 zeroed: logits move by %.2f; upsampling weight U-1 zeroed: by %.2f" % (A, U, moved_h, moved_w))
        assert moved_h > 0.1 and moved_w > 0.1, (A, U, moved_h, moved_w)


def test_inputs_meet_the_conditions():
    """every training input: no more near-kink post-net units than util.assert_grads_match_oracle enumerates the sides of, the upsampled features cover the
    N1 rows (F * U >= N1, at U = 240 and 1 too), rows that differ in their own ceil(max d), and at U = 16 a chunk that does not start on a frame boundary"""
    for label, o in all_cases():
        A, U, B = o.cfg.n_aux, o.cfg.upsampling_factor, o.x.shape[0]
        N1 = o.cfg.receptiveA_field * o.maxd + o.cfg.receptiveF_field + o.BL
        units = int(sum((np.abs(c[key]) < 4e-6).sum() for c in o.caches for key in ("s0", "y0")))
        assert units <= 6, (label, units)
        assert o.h.shape[1] == A and o.h.shape[2] * U >= N1, (label, o.h.shape, N1)
        own = [int(np.ceil(o.d[r]).max()) for r in range(B)]
        assert max(own) == o.maxd and (B == 1 or min(own) < o.maxd), (label, own)
        if U == 16:
            assert (o.h.shape[2] * U - N1) % U != 0, label
    assert _input(_case("c", "paper", 39, 240)["key"]).h.shape[2] <= 6


def test_wide_stack_lengths_cover_the_tile_residues():
    """the condition WIDE_BL and WIDE_F0_LO have to meet (adjust them if the chunk's maxd ever changes): BL itself and N1 - s_out of the first layer (a fixed layer of
    dilation 1: s_out = 1) at residues 0, 1 and 127 of the 128-row GEMM tile, and one length with B * BL < 4 * 16"""
    res_bl, res_n = set(), set()
    for BL in WIDE_BL:
        o = _input(("w160", 39, 110, 1, BL, WIDE_F0_LO))
        assert o.maxd == 42 and o.BL == BL and o.cfg.dilationsF[0] == 1
        N1 = o.cfg.receptiveA_field * o.maxd + o.cfg.receptiveF_field + BL
        res_bl.add(BL % 128)
        res_n.add((N1 - 1) % 128)
    assert {0, 1, 127} <= res_bl and {0, 1, 127} <= res_n
    assert any(1 * BL < 4 * 16 for BL in WIDE_BL)


# ---------------------------------------------------------------- training
@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_training_vs_oracle(case, cuda, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    o = _input(case["key"])
    compare = _compare_wide if case["wide"] else None
    E._autograd(case["id"] + " autograd", o, cuda, compare=compare)
    E._fused(case["id"] + " fused step", o, cuda, weights_too=case["weights_too"], compare=compare)


# ---------------------------------------------------------------- decode
_ONE_CU = "pipe rows=0 waves=0 x 0 (1 per group); one-cu rows=2"
_PLAN = {"pipe": "pipe rows=2", "one-cu": _ONE_CU, "interpreter": _ONE_CU, "coop": "coop G=4", "coopb": "coopb G=32 "}      # what qpn_last_decode_plan starts with
FAMILIES = list(D._TIE_KERNELS)
DECODE_AU = [(A, 110) for A in (2, 16, 17, 28, 64, 65)] + [(39, U) for U in (1, 5, 16, 80, 240)] + [(28, 80), (65, 16)]
DECODE_MORE = (28, 80)             # sampling and teacher-forced logits too
DECODE_WSEED = 29


def _family_cfg(family, A, U):
    geo = D._TIE_KERNELS[family][0]
    return dataclasses.replace(PAPER if geo is None else QPNetConfig(**geo), n_aux=A, upsampling_factor=U)


def _utts(U):
    """two rows: about 400 samples and about 60 % of that"""
    nf = -(-400 // U) + 1
    return [(61, nf, 1.0), (62, max(1, min(nf - 1, int(round(0.6 * nf)))), 1.0)]


@functools.lru_cache(maxsize=None)
def _decode_reference(family, A, U, mode):
    """the C oracle's stream of each row (input order), computed once per geometry and shared by the families that share it"""
    from oracle import cpu_oracle
    cfg = _family_cfg(family, A, U)
    flat = synth.make_weights(cfg, DECODE_WSEED)
    bx, bh, bd, ns = util.decode_batch(cfg, _utts(U))
    maxd = int(np.nanmax(np.ceil(bd)))
    return tuple(cpu_oracle.decode(cfg, flat, bh[b], bd[b], bx[b], ns[b], maxd=maxd, mode=mode, seed=5, row=b)["samples"] for b in range(len(ns)))


def _set_family(family, monkeypatch):
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    for k, v in D._TIE_KERNELS[family][1].items():
        monkeypatch.setenv(k, v)


@gpu
@pytest.mark.parametrize("A,U", DECODE_AU, ids=["A%d-U%d" % au for au in DECODE_AU])
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_vs_oracle(family, A, U, cuda, monkeypatch):
    import torch
    _set_family(family, monkeypatch)
    cfg = _family_cfg(family, A, U)
    flat = synth.make_weights(cfg, DECODE_WSEED)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = util.decode_batch(cfg, _utts(U))
    assert bh.shape[1] == A and ns[0] > ns[1] and not bh[1, :, -1].any()             # the shorter row's features arrive zero padded
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    for mode in ("argmax", "sampling") if (A, U) == DECODE_MORE else ("argmax",):
        m.sampling_seed = 5
        outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode=mode)
        assert m.last_decode_plan.startswith(_PLAN[family]), m.last_decode_plan
        ref = _decode_reference(family, A, U, mode)
        order = sorted(range(2), key=lambda i: ns[i])
        for pos, i in enumerate(order):
            np.testing.assert_array_equal(outs[pos], ref[i], err_msg="%s A=%d U=%d %s: row %d" % (family, A, U, mode, i))


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_step_logits_bitwise_vs_oracle(family, cuda, oracle, monkeypatch):
    """teacher-forced per-step logits at (28, 80), as test_stream_logits_bitwise_vs_oracle checks them at (39, 110)"""
    import torch
    _set_family(family, monkeypatch)
    A, U = DECODE_MORE
    cfg = _family_cfg(family, A, U)
    flat = synth.make_weights(cfg, DECODE_WSEED)
    m = util.build_model(cfg, flat, cuda)
    x, h, d, n = synth.decode_inputs(cfg, 4, 5, 1.0)
    teacher = np.random.RandomState(9).randint(0, 256, size=n).astype(np.int64)
    out, logits = m._stream_logits(torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), d[None], torch.from_numpy(teacher[None]), n)
    r = oracle.decode(cfg, flat, h, d, x, n, teacher=teacher, want_logits=True)
    lg = logits[0].cpu().numpy()
    assert np.array_equal(lg.view(np.uint32), r["logits"].view(np.uint32)), "max abs diff %g" % np.abs(lg - r["logits"]).max()
    np.testing.assert_array_equal(out[0].cpu().numpy(), r["samples"])


@gpu
@pytest.mark.parametrize("family", ["pipe", "one-cu"])
@pytest.mark.parametrize("case", AUX_CASES, ids=[c[0] for c in AUX_CASES])
def test_decode_matches_the_reference_streams(case, family, cuda, golden_dir, monkeypatch):
    """the streams the reference itself produced at these geometries (tests/golden/aux.npz): completion order and list consumption included"""
    import torch
    _set_family(family, monkeypatch)
    name, cfg, wseed, _, _, utts = case
    g = np.load(golden_dir + "/aux.npz")
    m = util.build_model(cfg, synth.make_weights(cfg, wseed), cuda)
    bx, bh, bd, ns = util.decode_batch(cfg, utts)
    nlist = list(ns)
    outs = m.batch_fast_generate(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), nlist, bd, mode="argmax")
    if cfg.n_resch == 64 and len(cfg.dilationsF) == 4:
        assert m.last_decode_plan.startswith(_PLAN[family]), m.last_decode_plan       # the paper-size network keeps its pipelined kernel at another A and U
    assert nlist == list(g[name + "_nleft"])
    for i, s in enumerate(outs):
        np.testing.assert_array_equal(s, g["%s_out%d" % (name, i)].astype(np.int64), err_msg="HIP vs reference stream, row %d" % i)


@gpu
def test_live_output_vs_oracle(cuda):
    """generate_live on the pipelined kernel at (28, 80): the pieces concatenate to the oracle's streams"""
    import torch
    A, U = DECODE_MORE
    cfg = _family_cfg("pipe", A, U)
    m = util.build_model(cfg, synth.make_weights(cfg, DECODE_WSEED), cuda)
    bx, bh, bd, ns = util.decode_batch(cfg, _utts(U))
    rows = [[] for _ in ns]
    for row, start, samples in m.generate_live(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), list(ns), bd, mode="argmax", every=64):
        assert start == sum(len(p) for p in rows[row])
        rows[row].append(samples)
    assert m.last_decode_plan.startswith(_PLAN["pipe"]), m.last_decode_plan
    ref = _decode_reference("pipe", A, U, "argmax")
    for b in range(len(ns)):
        np.testing.assert_array_equal(np.concatenate(rows[b]), ref[b], err_msg="row %d" % b)
