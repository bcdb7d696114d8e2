"""GPU: teacher-forced scoring through the model -- QPNet.score and FusedTrainer.score on the forward fixtures (tests/golden/forward*.npz, the
reference's logits and loss) against tests/score_spec.py, and against the loss the library already reports for the same batch."""
import functools
import types

import numpy as np
import pytest

from cases import FORWARD_CASES, FORWARD_CASES_D
from qpnet_amd import synth
import score_spec as SP
import util

pytestmark = pytest.mark.gpu

CASES = {c[0]: (c, "forward.npz") for c in FORWARD_CASES}
CASES[FORWARD_CASES_D[0][0]] = (FORWARD_CASES_D[0], "forward_d.npz")
NAMES = list(CASES)


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _host(s):
    return types.SimpleNamespace(nll=s.nll.cpu().numpy(), entropy=s.entropy.cpu().numpy(), argmax=s.argmax.cpu().numpy(), rank=s.rank.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _run(name):
    """one case, computed once and never written: the model's logits, both scores, forward_loss, and the spec on the model's and on the fixture's logits"""
    import os
    import torch
    from qpnet_amd.train import FusedTrainer
    (_, cfg, wseed, dseed, bl, ml), fixture = CASES[name]
    cuda = torch.device("cuda:0")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fixture))
    m = util.build_model(cfg, synth.make_weights(cfg, wseed), cuda)
    x, h, t, d, b = synth.train_inputs(cfg, bl, dseed, ml)
    xt, ht, tt, dt = _to(cuda, x, h, t, d)
    BL = int(b[0])
    with torch.no_grad():
        lg = m(xt, ht, dt, b).cpu().numpy()
    s_model = m.score(xt, ht, dt, b, tt)
    tr = FusedTrainer(m)
    s_trainer = tr.score(xt, ht, tt, dt, b)
    loss = tr.forward_loss(xt, ht, tt, dt, b)
    torch.cuda.synchronize()
    rec = lambda s: torch.stack([s.nll.view(torch.int32), s.entropy.view(torch.int32), s.argmax, s.rank]).cpu().numpy()      # noqa: E731
    return types.SimpleNamespace(name=name, BL=BL, Q=cfg.n_quantize, t=t[:, -BL:], lg=lg, ref_lg=g[name + "_logits"], ref_loss=float(g[name + "_loss"]),
                                 model=_host(s_model), bytes_model=rec(s_model), bytes_trainer=rec(s_trainer), loss=loss, mean_nll=float(s_trainer.nll.double().mean()),
                                 dtypes=[a.dtype for a in s_model], shapes=[tuple(a.shape) for a in s_model], tr=tr, inputs=(xt, ht, tt, dt, b))


@pytest.mark.parametrize("name", NAMES)
def test_model_and_trainer_score_the_same_bytes(name, cuda):
    import torch
    r = _run(name)
    assert r.dtypes == [torch.float32, torch.float32, torch.int32, torch.int32] and r.shapes == [(1, r.BL)] * 4
    np.testing.assert_array_equal(r.bytes_model, r.bytes_trainer)


@pytest.mark.parametrize("name", NAMES)
def test_argmax_and_rank_are_the_specs_on_the_models_own_logits(name, cuda):
    r = _run(name)
    nll, ent, am, rk = SP.score(r.lg, r.t)
    np.testing.assert_array_equal(r.model.argmax, am)
    np.testing.assert_array_equal(r.model.rank, rk)
    err_n, err_e = np.abs(r.model.nll - nll).max(), np.abs(r.model.entropy - ent).max()
    print("SCORE %s: own logits: max |nll - spec| %.3e, max |entropy - spec| %.3e, top1 %.4f, top5 %.4f"
          % (name, err_n, err_e, (am == r.t).mean(), (rk < 5).mean()))
    assert err_n <= 1e-4 and err_e <= 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_nll_against_the_reference_logits_and_loss(name, cuda):
    r = _run(name)
    nll, _, _, _ = SP.score(r.ref_lg, r.t)
    err, dmean = np.abs(r.model.nll - nll).max(), abs(r.model.nll.astype(np.float64).mean() - r.ref_loss)
    print("SCORE %s: reference logits: max |nll - spec| %.3e, |mean nll - reference loss| %.3e" % (name, err, dmean))
    assert err <= 1e-4
    assert dmean <= 1e-4


@pytest.mark.parametrize("name", ["paper", "default"])
def test_mean_nll_is_the_loss_forward_loss_reports(name, cuda):
    """PAPER: the cross entropy fused into the wide post-net tiles; the default widths: a k_ce launch of its own"""
    r = _run(name)
    print("SCORE %s: mean nll %.12f, forward_loss %.12f" % (name, r.mean_nll, r.loss))
    assert abs(r.mean_nll - r.loss) <= 1e-9 * abs(r.loss)


def test_mean_nll_is_the_loss_of_a_two_row_batch(cuda):
    import torch
    from qpnet_amd.config import TINY
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(TINY, synth.make_weights(TINY, 11), cuda)
    x, h, t, d, b = util.distinct_rows_batch(TINY, 300, 71, 30000, 2)
    xt, ht, tt, dt = _to(cuda, x, h, t, d)
    tr = FusedTrainer(m)
    s = tr.score(xt, ht, tt, dt, b)
    loss = tr.forward_loss(xt, ht, tt, dt, b)
    BL = int(b[0])
    assert tuple(s.nll.shape) == (2, BL)
    mean = float(s.nll.double().mean())
    print("SCORE tiny B=2: mean nll %.12f, forward_loss %.12f" % (mean, loss))
    assert abs(mean - loss) <= 1e-9 * abs(loss)
    with torch.no_grad():
        lg = m(xt, ht, dt, b).cpu().numpy()
    nll, ent, am, rk = SP.score(lg, t[:, -BL:])
    np.testing.assert_array_equal(s.argmax.cpu().numpy(), am)
    np.testing.assert_array_equal(s.rank.cpu().numpy(), rk)
    assert not np.array_equal(am[0], am[1])                       # the rows are different utterances: a row mix-up would show


def test_score_of_averaged_weights_needs_averaging(cuda):
    r = _run("tiny")
    xt, ht, tt, dt, b = r.inputs
    with pytest.raises(RuntimeError, match="keeps no averaged weights"):
        r.tr.score(xt, ht, tt, dt, b, weights="ema")
    with pytest.raises(RuntimeError, match="keeps no averaged weights"):
        r.tr.forward_loss(xt, ht, tt, dt, b, weights="ema")
    with pytest.raises(ValueError, match="weights must be"):
        r.tr.score(xt, ht, tt, dt, b, weights="best")
