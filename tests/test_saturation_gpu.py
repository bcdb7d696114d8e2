"""GPU parity in the regime a TRAINED network lives in (every other GPU test builds a freshly initialised one: gates in their linear region, a uniform softmax):
saturated gates -- sigma exactly 0, a float32 denormal, exp() of the hardware past float32 overflow, sigma exactly 1, tanh exactly +-1 -- and a peaked
softmax whose target probability underflows.  Training (every launch arrangement's gate non-linearity and gate backward, the three cross entropies) against
oracle/train_oracle.py, decode (the qgate / qexp clamps, the argmax, the inverse-CDF draw over an exactly-zero tail) bit for bit against oracle/qpnet_oracle.c,
and the cross-entropy kernel alone on hand-made logit rows.  tests/test_saturation_cpu.py holds the conditions on the inputs (tests/saturation_common.py).

Bounds: the project's small-chunk bounds with the float32-relative scaling an absolute bound needs once values stop being O(1) -- logits
2e-5 * max(1, max|ref logits|), loss 1e-4 * max(1, |ref loss|), gradients util.assert_grads_match_oracle(a_scale 2e-5, a_rel 1e-4) as everywhere.  The numpy
oracle's own float32 noise on these inputs is at most 0.10 of them (tools/saturation_parity_noise.py; MEASUREMENTS.md, "Saturated-regime parity")."""
import numpy as np
import pytest

from qpnet_amd.config import PAPER, QPNetConfig
import saturation_common as S
import test_train_edges_gpu as E
import test_decode_gpu as D
import util

pytestmark = pytest.mark.gpu

SCEN = list(S.SCENARIOS)


def _finite(label, o, logits, loss, grad):
    """first of all: nothing the kernels gave is inf or NaN (a failure names the parameter tensor)"""
    if logits is not None:
        assert np.isfinite(logits).all(), "%s: %d non-finite logits" % (label, (~np.isfinite(logits)).sum())
    assert np.isfinite(loss), "%s: loss %r" % (label, loss)
    offs, _ = o.cfg.param_offsets()
    bad = ["%s (%d of %d)" % (k, (~np.isfinite(grad[a:a + int(np.prod(s))])).sum(), int(np.prod(s))) for k, (a, s) in offs.items()
           if not np.isfinite(grad[a:a + int(np.prod(s))]).all()]
    assert not bad, "%s: non-finite gradient in %s" % (label, ", ".join(bad))


def _compare(label, o, logits, loss, grad):
    """figures first, then the bounds of the module docstring"""
    from oracle import train_oracle as TO
    lg_bound, loss_bound = 2e-5 * max(1.0, float(np.abs(o.lg).max())), 1e-4 * max(1.0, abs(o.loss))
    e_lg = float(np.abs(logits - o.lg).max()) if logits is not None else float("nan")
    offs, _ = o.cfg.param_offsets()
    scale = np.abs(o.og).max()
    frac, name = max((np.abs(grad[a:a + int(np.prod(s))] - o.og[a:a + int(np.prod(s))]).max() / (2e-5 * scale + 1e-4 * np.abs(o.og[a:a + int(np.prod(s))]).max()), k)
                     for k, (a, s) in offs.items())
    print("SAT %-44s logits %.2e (%.2f of the bound)  loss %.2e (%.3f)  worst gradient tensor %.3f of its bound (%s)" %
          (label, e_lg, e_lg / lg_bound, abs(loss - o.loss), abs(loss - o.loss) / loss_bound, frac, name))
    if logits is not None:
        assert logits.shape == o.lg.shape
        np.testing.assert_allclose(logits, o.lg, atol=lg_bound, rtol=0)
    assert abs(loss - o.loss) <= loss_bound
    return util.assert_grads_match_oracle(TO, o.cfg, o.flat, o.caches, o.dl, grad, a_scale=2e-5, a_rel=1e-4, og=o.og)


def _autograd(label, o, cuda):
    E._autograd(label, o, cuda, compare=_compare, first=_finite)


# ---------------------------------------------------------------- training
@pytest.mark.parametrize("scenario", SCEN)
@pytest.mark.parametrize("cfgname", ["paper", "c128", "tiny"])
def test_saturated_autograd_vs_oracle(cfgname, scenario, cuda):
    """the default launch arrangement of the paper-size, a generic-kernel and the tiny geometry: logits, loss and every gradient tensor"""
    _autograd("%s %s autograd" % (cfgname, scenario), S.train_input(cfgname, scenario), cuda)


@pytest.mark.parametrize("scenario", SCEN)
def test_saturated_fused_step_vs_oracle(scenario, cuda):
    """qpn_train_step: the cross entropy inside the post-net tile (its loss and dL/dlogits on rows whose target underflows), both stack queues, the library's Adam"""
    E._fused("paper %s fused step" % scenario, S.train_input("paper", scenario), cuda, weights_too=True, compare=_compare, first=_finite)


@pytest.mark.parametrize("scenario", SCEN)
@pytest.mark.parametrize("knobs", E.KNOBS, ids=E.KNOB_IDS)
def test_saturated_launch_arrangements_vs_oracle(knobs, scenario, cuda, monkeypatch):
    """the other copies of the gate arithmetic: a launch per layer, the auxiliary 1x1 at sample rate, the generic weight gradient, the GEMM path (its own
    non-linearity and its own gate backward)"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _autograd("paper %s %s" % (scenario, E.KNOB_IDS[E.KNOBS.index(knobs)]), S.train_input("paper", scenario), cuda)


@pytest.mark.parametrize("scenario", ["peaked", "all"])
def test_saturated_wide_post_net_vs_oracle(scenario, cuda):
    """n_skipch 512: the wide post-net tiles and their fused cross entropy"""
    o = S.train_input("wide", scenario)
    _autograd("wide %s autograd" % scenario, o, cuda)
    E._fused("wide %s fused step" % scenario, o, cuda, compare=_compare, first=_finite)


# ---------------------------------------------------------------- decode
@pytest.mark.parametrize("kind", ["clamped", "stochastic"])
@pytest.mark.parametrize("kernel", list(D._TIE_KERNELS))
def test_saturated_decode_vs_oracle(kernel, kind, cuda, oracle, monkeypatch):
    """every decode kernel on weights whose logit spread is beyond the exp-argument clamp at every step ("clamped") and on weights whose draw differs from the
    argmax at a third of the steps ("stochastic"): greedy and sampling, float64 and float32 pitch factors, two ragged rows -- bit-identical streams"""
    import torch
    geo, env, plan = D._TIE_KERNELS[kernel]
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfgname = {"interpreter": "c128", "coopb": "coopb"}.get(kernel, "paper")
    cfg = S.DECODE_CFGS[cfgname]
    assert cfg == (PAPER if geo is None else QPNetConfig(**geo))
    flat = S.decode_weights(cfgname, kind)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = util.decode_batch(cfg, S.DECODE_UTTS)
    assert sorted(ns) == [329, 439]
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    for extra in (False, True):
        for mode in ("argmax", "sampling"):
            m.sampling_seed = 5
            d_arg = torch.from_numpy(bd).float().to(cuda) if extra else bd
            outs = m.batch_fast_generate(xb, hb, list(ns), d_arg, mode=mode, extra_memory=extra)
            assert plan in m.last_decode_plan, m.last_decode_plan
            o_outs = S.decode_reference(cfgname, kind, mode, extra)
            assert [len(a) for a in outs] == sorted(ns)
            for i, (a, b) in enumerate(zip(outs, o_outs)):
                np.testing.assert_array_equal(a, b, err_msg="%s, %s weights, %s d, %s: stream %d" % (kernel, kind, "float32" if extra else "float64", mode, i))


@pytest.mark.parametrize("kernel", ["pipe", "coopb"])
def test_saturated_stream_logits_bitwise_vs_oracle(kernel, cuda, oracle, monkeypatch):
    """teacher-forced per-step logits with a spread beyond the clamp: bit-identical to the oracle's on the default paper plan and the batched cooperative kernel"""
    import torch
    from qpnet_amd import synth
    geo, env, plan = D._TIE_KERNELS[kernel]
    monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfgname = "coopb" if kernel == "coopb" else "paper"
    cfg, flat = S.DECODE_CFGS[cfgname], S.decode_weights(cfgname, "clamped")
    m = util.build_model(cfg, flat, cuda)
    rows = [synth.decode_inputs(cfg, 3, fs, 1.0) for fs in (61, 62)]               # two utterances of one length: the batched kernel takes two rows and up
    n = rows[0][3]
    x, h, d = (np.stack([r[k] for r in rows]) for k in range(3))
    maxd = int(np.ceil(d).max())
    teacher = np.random.RandomState(9).randint(0, cfg.n_quantize, size=(2, n)).astype(np.int64)
    out, logits = m._stream_logits(torch.from_numpy(x).to(cuda), torch.from_numpy(h).to(cuda), d, torch.from_numpy(teacher), n)
    L, hd = m._native(cuda)
    text = L.qpn_last_decode_plan(hd).decode()
    assert plan in text, text
    for b in range(2):
        r = oracle.decode(cfg, flat, h[b], d[b], x[b], n, maxd=maxd, teacher=teacher[b], want_logits=True)
        lg = logits[b].cpu().numpy()
        assert ((r["logits"].max(1) - r["logits"].min(1)) > 87).mean() >= 0.5
        assert np.array_equal(lg.view(np.uint32), r["logits"].view(np.uint32)), "row %d: max abs diff %g" % (b, np.abs(lg - r["logits"]).max())
        np.testing.assert_array_equal(out[b].cpu().numpy(), r["samples"])


# ---------------------------------------------------------------- the cross-entropy kernel alone
# The class counts the C ABI takes (train_init: multiples of 16): both branches of k_ce's (Q & 255) == 0, a two-pass row (512), a row that is no whole
# number of waves (112) and a row shorter than a wave (16)
CE_Q = (256, 512, 112, 16)
CE_ROWS = ("equal", "spread 1e-3", "spread 50", "spread 200", "one hot 1e4", "max first", "max last", "two maxima", "all -1e4")


def _ce_rows(Q):
    """(B = 2, BL = 9, Q) float32 logits: the nine hand-made rows (both batch items carry them, the second one's classes reversed), and per row the largest,
    the smallest and the last class"""
    rs = np.random.RandomState(Q)
    u = rs.uniform(-0.5, 0.5, Q)
    rows = [np.zeros(Q), 1e-3 * u, 50.0 * u, 200.0 * u, np.full(Q, -1e4), 8.0 * u, 8.0 * u, 8.0 * u, np.full(Q, -1e4)]
    rows[4][Q // 3] = 1e4
    rows[5][0] = 9.0                                    # lane 0's first element
    rows[6][Q - 1] = 9.0                                # the last lane's last element
    rows[7][1] = rows[7][Q - 2] = 9.0                   # two exactly equal maxima
    lg = np.stack([np.stack(rows), np.stack(rows)[:, ::-1]]).astype(np.float32)
    assert lg.shape == (2, len(CE_ROWS), Q)
    return lg


@pytest.mark.parametrize("Q", CE_Q)
def test_ce_loss_on_hand_made_rows(Q, cuda):
    """qpn_ce_loss against train_oracle.ce_loss (float64) with the target on the largest class, on the smallest and on class Q - 1 of every row"""
    import ctypes as C
    import torch
    from oracle import train_oracle as TO
    from qpnet_amd import _lib, synth
    cfg = QPNetConfig(n_quantize=Q, n_resch=64, n_skipch=64, dilationF_depth=1, dilationF_repeat=1, dilationA_depth=1, dilationA_repeat=1)
    m = util.build_model(cfg, synth.make_weights(cfg, 3), cuda)
    L, hd = m._native(cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    lg = _ce_rows(Q)
    B, BL = lg.shape[:2]
    lgt = torch.from_numpy(lg).to(cuda)
    for where, tgt in (("largest", lg.argmax(2)), ("smallest", lg.argmin(2)), ("last", np.full((B, BL), Q - 1))):
        t = np.concatenate([np.zeros((B, 3), np.int64), tgt.astype(np.int64)], axis=1)          # a target row longer than BL: the last BL columns count
        tt = torch.from_numpy(t).to(cuda)
        dl = torch.full((B, BL, Q), float("nan"), device=cuda)
        loss = C.c_double(0)
        _lib.check(L.qpn_ce_loss(hd, lgt.data_ptr(), tt.data_ptr(), t.shape[1], B, BL, dl.data_ptr(), C.byref(loss), stream))
        _lib.check(L.qpn_train_status(hd, stream))
        ref_loss, ref_dl = TO.ce_loss(lg, tgt)
        dl = dl.cpu().numpy()
        err = np.abs(dl.astype(np.float64) - ref_dl).reshape(B * BL, Q).max(1) * (B * BL)
        print("SAT ce Q=%d target on the %-8s loss %.6f (ref %.6f, %.3f of the bound)  dlogits * rows, worst row: %.2e (%s)" %
              (Q, where, loss.value, ref_loss, abs(loss.value - ref_loss) / (1e-4 * max(1.0, abs(ref_loss))), err.max(), CE_ROWS[int(err.argmax()) % BL]))
        assert np.isfinite(loss.value) and np.isfinite(dl).all()
        assert abs(loss.value - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
        np.testing.assert_allclose(dl, ref_dl, atol=2e-5 / (B * BL), rtol=0)


@pytest.mark.parametrize("Q", [100, 3])
def test_ce_loss_refuses_a_class_count_the_kernels_do_not_take(Q, cuda):
    """no multiple of 16: the library says so -- when the handle is made or at the call -- instead of giving a quietly wrong loss"""
    import ctypes as C
    import torch
    from qpnet_amd import _lib, synth
    cfg = QPNetConfig(n_quantize=Q, n_resch=64, n_skipch=64, dilationF_depth=1, dilationF_repeat=1, dilationA_depth=1, dilationA_repeat=1)
    m = util.build_model(cfg, synth.make_weights(cfg, 3), cuda)
    lgt = torch.zeros((2, 9, Q), device=cuda)
    tt = torch.zeros((2, 9), dtype=torch.int64, device=cuda)
    dl = torch.empty_like(lgt)
    loss = C.c_double(0)
    with pytest.raises(_lib.QpnError) as e:
        L, hd = m._native(cuda)
        _lib.check(L.qpn_ce_loss(hd, lgt.data_ptr(), tt.data_ptr(), 9, 2, 9, dl.data_ptr(), C.byref(loss), torch.cuda.current_stream(cuda).cuda_stream))
    assert "multiples of" in str(e.value)
