"""GPU parity of the training path where the benchmark-shaped tests never go: batches whose rows differ in everything (pitch factors, features,
waveform), chunk lengths on and next to the kernels' tile edges (16-row stack tiles, 80-row post-net tiles, 32-row weight-gradient stages, BL = 1),
and pitch factors on a grid of ties, integers and the gather's inclusive boundary.

One yardstick throughout: oracle/train_oracle.py (forward, ce_loss, backward through util.assert_grads_match_oracle) at the project's small-chunk
tolerances -- logits 2e-5, loss 1e-4, gradients a_scale 2e-5 / a_rel 1e-4.  The oracle runs once per input (_oracle is cached) and is shared by
every kernel arrangement checked on that input.  Every check prints its figures before it asserts (pytest -s / -rA shows them); the numpy oracle's
own float32 noise on these inputs is measured by tools/edge_parity_noise.py (MEASUREMENTS.md, "Edge-shape parity")."""
import functools
import types

import numpy as np
import pytest

from qpnet_amd import synth
from qpnet_amd.config import PAPER, TINY, QPNetConfig
import util

pytestmark = pytest.mark.gpu

C128 = QPNetConfig(n_resch=128, n_skipch=128, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=2, dilationA_repeat=1)     # the generic (not compile-time-tiled) kernels
CFGS = {"paper": (PAPER, 21), "c128": (C128, 7), "tiny": (TINY, 11)}          # geometry, weight seed
# synth.train_inputs(cfg, 500, seed, 2500, f0_lo=60, pin_f0_floor=True, batch_size=B): on PAPER T = 1100, BL = 394, batch maxd 46.  Seed 61 for one and two
# rows (the rows' own ceil(max d): 43 and 46).  Three rows take seed 62 (46, 40, 42): the three rows of seed 61 have 7 post-net pre-activations within
# kink_eps = 4e-6 of a ReLU kink in the oracle's forward, one more than util.assert_grads_match_oracle enumerates the sides of (seed 62: 2; seed 61 B = 2: 3)
DSEED = {1: 61, 2: 61, 3: 62}
# the launch arrangements whose kernels index rows and batch items by themselves: a launch per layer instead of the work queue, the auxiliary 1x1 at
# sample rate, the generic weight-gradient kernel, the LDS-tiled GEMM path
KNOBS = [{"QPN_STACK_QUEUE": "0"}, {"QPN_AUX_HOIST": "0"}, {"QPN_WGRAD_GENERIC": "1"}, {"QPN_TRAIN_GEMM": "1"}]
KNOB_IDS = [",".join("%s=%s" % kv for kv in k.items()) for k in KNOBS]
EDGE_BL = (1, 14, 15, 16, 17, 31, 32, 33, 79, 80, 81, 160, 161)
EDGE_BL_MORE = (1, 33, 81)
EDGE_BL_C128 = (1, 17, 81)


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrs]          # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _flat(cfgname):
    cfg, wseed = CFGS[cfgname]
    return synth.make_weights(cfg, wseed)


@functools.lru_cache(maxsize=None)
def _chunk(cfgname, B):
    """B = 1: row 1 of the two-row batch, the row whose own ceil(max d) is the batch's"""
    if B == 1:
        return tuple(a[1:2] for a in _chunk(cfgname, 2))
    return util.distinct_rows_batch(CFGS[cfgname][0], 500, DSEED[B], 2500, B)


def _with_oracle(cfgname, x, h, t, d, b, cfg=None, flat=None):
    """the numpy oracle's forward, loss, dL/dlogits and gradient of one input, next to the input (arrays are shared between tests: never written).
    cfg, flat: another geometry / other weights than CFGS[cfgname]'s (tests/saturation_common.py)"""
    from oracle import train_oracle as TO
    cfg, flat = cfg or CFGS[cfgname][0], _flat(cfgname) if flat is None else flat
    BL = int(b[0])
    lg, caches = TO.forward(cfg, flat, x, h, d, b)
    loss, dl = TO.ce_loss(lg, t[:, -BL:])
    og = TO.backward(cfg, flat, caches, dl)
    for a in (x, h, t, d, b, lg, dl, og):
        a.setflags(write=False)
    return types.SimpleNamespace(cfgname=cfgname, cfg=cfg, flat=flat, x=x, h=h, t=t, d=d, b=b, BL=BL, maxd=int(np.ceil(d).max()), lg=lg, caches=caches,
                                 loss=float(loss), dl=dl, og=og)


@functools.lru_cache(maxsize=None)
def _oracle(cfgname, B, BL=None, drop=0):
    """the shared chunk of `cfgname` with B distinct rows, optionally with a shorter batch_length (the same samples: the chunk is then longer than
    RF + BL, as in test_forward_maxd_bound_on_paper_with_a_long_chunk) and with its first `drop` samples cut off x, t and d (T odd, h unchanged: the
    features stay aligned at the chunk's end)"""
    x, h, t, d, b = _chunk(cfgname, B)
    if BL is not None:
        b = np.full_like(b, BL)
    return _with_oracle(cfgname, x[:, drop:].copy(), h.copy(), t[:, drop:].copy(), d[:, drop:].copy(), b.copy())


@functools.lru_cache(maxsize=None)
def _ties(cfgname):
    """two distinct rows with d snapped to the 1/16 grid and walked through its residues (util.snap_to_grid, downwards: ceil(max d), and with it the receptive
    field, stays; exact .5 and integer products d * dilation at every adaptive dilation), a run of the unvoiced value 1.0, and the head rows [0, recA * maxd + recF] of the N1 window -- inclusive: the first output row of the LAST adaptive layer is row recA * maxd + recF --
    at exactly float(maxd), so that the first output row of every adaptive layer gathers row 0 of its input (tap == s_in, the inclusive edge of the
    device-side bound check)"""
    x, h, t, d, b = _chunk(cfgname, 2)
    cfg = CFGS[cfgname][0]
    d = util.snap_to_grid(d, walk=-1)
    maxd = int(np.ceil(d).max())
    T, BL = d.shape[1], int(b[0])
    head = cfg.receptiveA_field * maxd + cfg.receptiveF_field
    w0 = T - (head + BL)
    assert w0 >= 0
    d[0, -200:-140] = 1.0
    d[1, -90:-30] = 1.0
    d[:, w0:w0 + head + 1] = float(maxd)
    return _with_oracle(cfgname, x.copy(), h.copy(), t.copy(), d, b.copy())


def all_cases():
    """(label, input with its oracle) of every input this module runs on the GPU: what tools/edge_parity_noise.py measures the oracle's own noise on"""
    for cfgname, B in (("paper", 2), ("paper", 3), ("c128", 2), ("tiny", 2)):
        yield "distinct rows %s B=%d" % (cfgname, B), _oracle(cfgname, B)
    for BL in EDGE_BL:
        yield "edge paper BL=%d" % BL, _oracle("paper", 1, BL)
    for BL in EDGE_BL_MORE:
        yield "edge paper BL=%d B=2" % BL, _oracle("paper", 2, BL)
    for k in (1, 3):
        yield "odd chunk paper BL=33 drop=%d" % k, _oracle("paper", 1, 33, drop=k)
    for BL in EDGE_BL_C128:
        yield "edge c128 BL=%d" % BL, _oracle("c128", 1, BL)
    for cfgname in ("paper", "c128"):
        yield "ties %s B=2" % cfgname, _ties(cfgname)


def _compare(label, o, logits, loss, grad):
    """figures first, then the project's small-chunk bounds"""
    from oracle import train_oracle as TO
    e_lg = float(np.abs(logits - o.lg).max()) if logits is not None else float("nan")
    print("EDGE %-44s logits %.2e  loss %.2e  grad %.2e of the largest" % (label, e_lg, abs(loss - o.loss), np.abs(grad - o.og).max() / np.abs(o.og).max()))
    if logits is not None:
        assert logits.shape == o.lg.shape
        np.testing.assert_allclose(logits, o.lg, atol=2e-5, rtol=0)
    assert abs(loss - o.loss) < 1e-4
    return util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, grad, a_scale=2e-5, a_rel=1e-4, og=o.og)


def _autograd(label, o, cuda, read_back_maxd=True, compare=None, first=None):
    """logits, loss and loss.backward() of a fresh module (a fresh native handle: the launch knobs are read when it is created) against the oracle.
    read_back_maxd: the exact ceil(max d) (N1 = recA * maxd + recF + BL); False: train.forward_maxd's shape-derived bound (another N1, same logits).
    compare: another set of bounds than _compare's; first(label, o, logits, loss, grad): a check that runs before check_status"""
    import torch
    m = util.build_model(o.cfg, o.flat, cuda).train()
    m.read_back_maxd = read_back_maxd
    xt, ht, tt, dt, bt = _to(cuda, o.x, o.h, o.t, o.d, o.b)
    logits = m(xt, ht, dt, bt)
    loss = torch.nn.CrossEntropyLoss()(logits.reshape(-1, o.cfg.n_quantize), tt[:, -o.BL:].reshape(-1))
    loss.backward()
    grad = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy()
    if first is not None:
        first(label, o, logits.detach().cpu().numpy(), loss.item(), grad)
    m.check_status()                                            # the device-side gather-bound check must not have fired
    (compare or _compare)(label, o, logits.detach().cpu().numpy(), loss.item(), grad)


def _fused(label, o, cuda, weights_too=False, compare=None, first=None):
    """FusedTrainer.step (qpn_train_step: the fused post-net tile, both stack queues, the library's Adam) against the oracle: loss, the step's gradient and --
    weights_too -- the parameters after the step against the oracle's Adam, as test_the_fused_step_bench_times_vs_oracle checks them"""
    from oracle import train_oracle as TO
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(o.cfg, o.flat, cuda).train()
    tr = FusedTrainer(m, lr=1e-4)
    xt, ht, tt, dt = _to(cuda, o.x, o.h, o.t, o.d)
    loss = tr.step(xt, ht, tt, dt, o.b, want_loss=True, maxd=o.maxd)
    if first is not None:
        first(label, o, None, loss, tr.g[:o.flat.size].cpu().numpy())
    tr.check_status()
    og = (compare or _compare)(label, o, None, loss, tr.g[:o.flat.size].cpu().numpy())
    if weights_too:
        wo = o.flat.copy()
        TO.Adam(wo.size).step(wo, og)
        util.assert_weights_after_adam(m.flat_parameters().cpu().numpy(), wo, 1e-4, 1, far=2.0, significant=util.significant_elements(o.cfg, [og]), sig_max=1e-6)


# ---------------------------------------------------------------- A1: batch rows that differ in d, h and waveform
@pytest.mark.parametrize("B", [2, 3])
def test_distinct_rows_are_distinct_and_the_oracle_tells_them_apart(B):
    """What makes the tests below discriminating, asserted on the inputs and the oracle alone: the rows differ in d and h, at least one row's own ceil(max d) is
    below the batch's (its taps reach less far than the shared receptive field), and a row's logits move by far more than the 2e-5 tolerance when the row is
    given another row's pitch factors or features -- a kernel that read row 0's d or h for every row cannot pass."""
    from oracle import train_oracle as TO
    o = _oracle("paper", B)
    assert o.x.shape == (B, 1100) and o.BL == 394 and o.maxd == 46
    own = [int(np.ceil(o.d[r]).max()) for r in range(B)]
    assert max(own) == o.maxd and min(own) < o.maxd, own
    W = TO.unpack(o.cfg, o.flat)
    for r in range(1, B):
        assert not np.array_equal(o.d[r], o.d[0]) and not np.array_equal(o.h[r], o.h[0])
        lg_d, _ = TO.forward_row(o.cfg, W, o.x[r], o.h[r], o.d[0], o.BL, o.maxd)
        lg_h, _ = TO.forward_row(o.cfg, W, o.x[r], o.h[0], o.d[r], o.BL, o.maxd)
        moved_d, moved_h = np.abs(lg_d - o.lg[r]).max(), np.abs(lg_h - o.lg[r]).max()
        print("EDGE row %d of %d given row 0's d: logits move by %.2f; given row 0's h: by %.2f" % (r, B, moved_d, moved_h))
        assert moved_d > 0.1 and moved_h > 0.1


@pytest.mark.parametrize("cfgname,B", [("paper", 2), ("paper", 3), ("c128", 2), ("tiny", 2)], ids=["paper-B2", "paper-B3", "c128-B2", "tiny-B2"])
def test_distinct_rows_autograd_vs_oracle(cfgname, B, cuda):
    """the per-row offsets of the forward and the backward (b * Td in k_train_prep, the per-row tap tables, (b * A + a) * F in the auxiliary kernels, the
    backward's scatter through per-row taps): logits, loss and every gradient tensor, on the paper-size, a generic-kernel and the tiny geometry"""
    o = _oracle(cfgname, B)
    assert min(int(np.ceil(o.d[r]).max()) for r in range(B)) < o.maxd
    _autograd("distinct rows %s B=%d autograd" % (cfgname, B), o, cuda)


@pytest.mark.parametrize("B", [2, 3])
def test_distinct_rows_fused_step_vs_oracle(B, cuda):
    _fused("distinct rows paper B=%d fused step" % B, _oracle("paper", B), cuda, weights_too=True)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_distinct_rows_launch_arrangements_vs_oracle(knobs, B, cuda, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _autograd("distinct rows paper B=%d %s" % (B, KNOB_IDS[KNOBS.index(knobs)]), _oracle("paper", B), cuda)


def test_permuting_the_batch_rows_permutes_the_logits_bit_for_bit(cuda):
    """rows are independent in the forward (no atomics, the same tiles per row wherever the row sits): row r of the permuted batch is bit-identical to the row it came from"""
    import torch
    o = _oracle("paper", 3)
    m = util.build_model(o.cfg, o.flat, cuda)
    perm = [2, 0, 1]
    with torch.no_grad():
        lg = m(*_to(cuda, o.x, o.h, o.d, o.b)).cpu().numpy()
        lgp = m(*_to(cuda, o.x[perm], o.h[perm], o.d[perm], o.b)).cpu().numpy()
    np.testing.assert_allclose(lg, o.lg, atol=2e-5, rtol=0)
    assert np.array_equal(lgp.view(np.uint32), lg[perm].view(np.uint32))


# ---------------------------------------------------------------- A2: chunk lengths on and next to the tile edges
def test_edge_lengths_cover_the_tile_residues():
    """the condition EDGE_BL has to meet (adjust the list if the chunk's maxd ever changes): with the exact maxd, N1 = recA * maxd + recF + BL"""
    o = _oracle("paper", 1, EDGE_BL[0])
    n1 = [o.cfg.receptiveA_field * o.maxd + o.cfg.receptiveF_field + bl for bl in EDGE_BL]
    assert o.maxd == 46 and o.x.shape[1] == 1100
    assert any(bl < 16 for bl in EDGE_BL)
    assert {0, 1, 79} <= {bl % 80 for bl in EDGE_BL}            # the paper-size post-net tiles (k_post_fwd_w / k_post_fb_w<5>)
    assert {0, 1, 31} <= {bl % 32 for bl in EDGE_BL}            # the weight-gradient stages
    assert {0, 1, 15} <= {n % 16 for n in n1}                   # the stack tiles and queue
    assert set(EDGE_BL_MORE) <= set(EDGE_BL)


@pytest.mark.parametrize("BL", EDGE_BL)
def test_tile_edge_lengths_vs_oracle(BL, cuda):
    """one row, the exact maxd: the autograd path and the fused step"""
    o = _oracle("paper", 1, BL)
    _autograd("edge BL=%d autograd" % BL, o, cuda)
    _fused("edge BL=%d fused step" % BL, o, cuda)


@pytest.mark.parametrize("BL", EDGE_BL_MORE)
def test_tile_edge_lengths_with_the_shape_derived_maxd_bound(BL, cuda):
    """train.forward_maxd's bound instead of the exact value: another N1 (more leading context rows, other tile counts) for the same BL"""
    from qpnet_amd.train import forward_maxd
    o = _oracle("paper", 1, BL)
    geo = types.SimpleNamespace(receptiveA_field=o.cfg.receptiveA_field, receptiveF_field=o.cfg.receptiveF_field, upsampling_factor=o.cfg.upsampling_factor)
    assert forward_maxd(geo, o.x.shape[1], o.h.shape[2], o.d.shape[1], BL, None) > o.maxd
    _autograd("edge BL=%d shape-derived maxd" % BL, o, cuda, read_back_maxd=False)


@pytest.mark.parametrize("BL", EDGE_BL_MORE)
def test_tile_edge_lengths_two_distinct_rows(BL, cuda):
    """two batch items: stages and tiles that straddle the item boundary at these lengths"""
    o = _oracle("paper", 2, BL)
    _autograd("edge BL=%d B=2 autograd" % BL, o, cuda)
    _fused("edge BL=%d B=2 fused step" % BL, o, cuda)


@pytest.mark.parametrize("BL", EDGE_BL_MORE)
@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_tile_edge_lengths_launch_arrangements(knobs, BL, cuda, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _autograd("edge BL=%d %s" % (BL, KNOB_IDS[KNOBS.index(knobs)]), _oracle("paper", 1, BL), cuda)


@pytest.mark.parametrize("k", [1, 3])
def test_odd_chunk_longer_than_the_window(k, cuda):
    """the chunk's first k samples dropped from x, t and d: T is odd, no multiple of the frame length and longer than N0 (everything is aligned at the chunk's END)"""
    o = _oracle("paper", 1, 33, drop=k)
    assert o.x.shape[1] == 1100 - k and o.h.shape[2] * o.cfg.upsampling_factor == 1100
    assert o.x.shape[1] > o.cfg.receptive_field(o.maxd) + o.BL
    _autograd("odd chunk T=%d autograd" % o.x.shape[1], o, cuda)
    _autograd("odd chunk T=%d shape-derived maxd" % o.x.shape[1], o, cuda, read_back_maxd=False)
    _fused("odd chunk T=%d fused step" % o.x.shape[1], o, cuda)


@pytest.mark.parametrize("BL", EDGE_BL_C128)
def test_tile_edge_lengths_generic_geometry(BL, cuda):
    o = _oracle("c128", 1, BL)
    _autograd("edge c128 BL=%d autograd" % BL, o, cuda)
    _fused("edge c128 BL=%d fused step" % BL, o, cuda)


# ---------------------------------------------------------------- A3: ties, integers, the gather's inclusive boundary
@pytest.mark.parametrize("cfgname", ["paper", "c128"])
def test_tie_input_has_ties_and_touches_the_gather_boundary(cfgname):
    """on the oracle alone: exact .5 products at every adaptive dilation, the unvoiced value, and every adaptive layer's reach equal to its input length"""
    from oracle import train_oracle as TO
    o = _ties(cfgname)
    for dil in sorted(set(o.cfg.dilationsA)):
        p = o.d.astype(np.float64) * dil
        assert (np.abs(p - np.floor(p) - 0.5) == 0).sum() >= 20 and (p == np.floor(p)).sum() >= 100
    assert (o.d == 1.0).sum() >= 100 and o.maxd == int(o.d.max())
    for c in o.caches:
        adaptive = [lc for lc in c["layers"] if lc["kind"] == "A"]
        assert len(adaptive) == len(o.cfg.dilationsA)
        for lc in adaptive:
            assert -int(lc["idx"].min()) == lc["Lin"]            # the first output row gathers row 0 of the layer's input
    # ... and rounding half away from zero (roundf) instead of half to even would move a good many taps of every adaptive layer
    for (kind, i, dil), lcs in zip(TO._layers(o.cfg), zip(*[c["layers"] for c in o.caches])):
        if kind == "A":
            moved = 0
            for r, lc in enumerate(lcs):
                L = lc["idx"].size
                s_ = (-(o.d[r, -L:]) * np.float32(dil)).astype(np.float32) + np.arange(-L, 0).astype(np.float32)
                assert np.array_equal(np.rint(s_).astype(np.int64), lc["idx"])
                moved += int((-np.floor(-s_.astype(np.float64) + 0.5) != lc["idx"]).sum())
            print("EDGE ties %s: adaptive layer %d (dilation %d): roundf would move %d taps" % (cfgname, i, dil, moved))
            assert moved >= 10


@pytest.mark.parametrize("arrangement", ["paper", "paper,QPN_STACK_QUEUE=0", "c128"])
def test_ties_integers_and_the_gather_boundary_vs_oracle(arrangement, cuda, monkeypatch):
    """round-half-to-even in k_train_prep's tap arithmetic (the reference's torch.round), d == 1.0, and tap == s_in without a status flag (check_status inside
    _autograd / _fused must not raise): the work queue, a launch per layer, the generic geometry"""
    cfgname, _, knob = arrangement.partition(",")
    if knob:
        monkeypatch.setenv(*knob.split("="))
    o = _ties(cfgname)
    _autograd("ties %s autograd" % arrangement, o, cuda)
    _fused("ties %s fused step" % arrangement, o, cuda)
