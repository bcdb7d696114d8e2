"""The start of the training step: the fused first launch (k_step_prep: the per-step refresh and the chunk's preparation as roles of one kernel,
QPN_PREP_FUSE).

It is a launch arrangement of arithmetic that does not change, so it is held against the arrangement it replaces (QPN_PREP_FUSE=0: k_refresh, then
k_train_prep) BITWISE where no float atomic feeds the result -- the forward has none -- and against the numpy oracle in both arms.  The knobs are read once
per native handle: every arm builds a fresh model under its environment."""
import dataclasses

import numpy as np
import pytest

import util
from qpnet_amd import synth
from qpnet_amd.config import PAPER, TINY

pytestmark = pytest.mark.gpu


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a for a in arrs]


_ORACLE = {}


def _oracle(key, cfg, flat, chunk):
    """numpy forward / loss / backward of a chunk, computed once per (case, chunk) and shared by the arms (nothing writes to it)"""
    if key not in _ORACLE:
        from oracle import train_oracle as TO
        x, h, t, d, b = chunk
        lg, caches = TO.forward(cfg, flat, x, h, d, b)
        oloss, dl = TO.ce_loss(lg, t[:, -int(b[0]):])
        _ORACLE[key] = (lg, caches, dl, float(oloss), TO.backward(cfg, flat, caches, dl))
    return _ORACLE[key]


def _autograd_arm(cuda, cfg, flat, chunks):
    """one handle: logits (qpn_train_forward) and the flat gradient (qpn_train_backward) of every chunk in turn, then the fused step's loss of the last one"""
    import torch
    from qpnet_amd.train import FusedTrainer
    m = util.build_model(cfg, flat, cuda).train()
    out = []
    for x, h, t, d, b in chunks:
        xt, ht, tt, dt, bt = _to(cuda, x, h, t, d, b)
        BL = int(b[0])
        m.zero_grad()
        logits = m(xt, ht, dt, bt)
        torch.nn.CrossEntropyLoss()(logits.reshape(-1, cfg.n_quantize), tt[:, -BL:].reshape(-1)).backward()
        out.append((logits.detach().cpu().numpy().copy(), torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu().numpy().copy()))
    tr = FusedTrainer(m, lr=1e-6)
    loss = tr.step(xt, ht, tt, dt, bt, want_loss=True)          # forward + cross entropy inside the post-net kernel where the geometry has it
    tr.check_status()
    return out, loss


# name -> (config, batch size, batch_length(s), knobs of both arms).  Two chunks: two consecutive steps on one handle with different ceil(max d),
# so a table, tap or queue head left over from the first would show in the second.
PREP_CASES = {
    "paper_b2_bl81_two_steps": (PAPER, 2, (81, 81), {}),        # a tile-edge chunk; rows of both batch items in one table workgroup
    "paper_b1_bl1": (PAPER, 1, (1,), {}),
    "tiny": (TINY, 2, (70,), {}),                               # n_resch 32: two table slices, no aux hoist
    "paper_aux_at_sample_rate": (PAPER, 2, (81,), {"QPN_AUX_HOIST": "0"}),
    "paper_upsampling_0": (PAPER, 2, (81,), {}),                # (the model's upsampling_factor is 0: features at sample rate, see _prep_chunks)
    "paper_q1024_table_too_large": (dataclasses.replace(PAPER, n_quantize=1024), 1, (40,), {}),      # a 16-channel slice is 139 KB: k_refresh + k_train_prep
}


def _prep_chunks(case, cfg, B, bls):
    """-> the model's config and its chunks: B distinct rows that share the pinned pitch floor, which sets ceil(max d) (60 Hz, then 120 Hz), with batch_length
    set to the case's (the same samples: the chunk is then longer than RF + BL, as in test_train_edges_gpu)"""
    chunks = []
    for i, bl in enumerate(bls):
        x, h, t, d, b = util.distinct_rows_batch(cfg, 500, 71 + i, 2500, B, f0_lo=(60.0, 120.0)[i])
        assert bl <= int(b[0])
        if case == "paper_upsampling_0":
            h = np.ascontiguousarray(np.repeat(h, cfg.upsampling_factor, axis=2)[:, :, :x.shape[1] + 3])
        chunks.append((x, h, t, d, np.full_like(b, bl)))
    return (dataclasses.replace(cfg, upsampling_factor=0) if case == "paper_upsampling_0" else cfg), chunks


@pytest.mark.parametrize("case", sorted(PREP_CASES))
def test_fused_first_launch_matches_the_two_launches(case, cuda, monkeypatch):
    """QPN_PREP_FUSE=1 against 0, same weights and chunks: logits bitwise (packed weights and biases, X0, tap tables, aux projections all feed them), the
    fused step's loss bitwise (at most two double adds per accumulator slot at these sizes: order-free), gradients against the oracle in both arms."""
    from oracle import train_oracle as TO
    cfg, B, bls, knobs = PREP_CASES[case]
    cfg, chunks = _prep_chunks(case, cfg, B, bls)
    flat = synth.make_weights(cfg, 31)
    if len(chunks) > 1:
        assert len({int(np.ceil(c[3].max())) for c in chunks}) == len(chunks), "the chunks must differ in ceil(max d)"
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    arms = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("QPN_PREP_FUSE", fuse)
        arms[fuse] = _autograd_arm(cuda, cfg, flat, chunks)
    (o1, l1), (o0, l0) = arms["1"], arms["0"]
    assert l1 == l0, "fused step's loss: %r vs %r" % (l1, l0)
    for i, chunk in enumerate(chunks):
        lg, caches, dl, oloss, og = _oracle((case, i), cfg, flat, chunk)
        assert np.array_equal(o1[i][0], o0[i][0]), "chunk %d: logits differ by %.3e" % (i, np.abs(o1[i][0] - o0[i][0]).max())
        np.testing.assert_allclose(o1[i][0], lg, atol=2e-5, rtol=0)          # (the small-chunk bound of test_train_edges_gpu)
        for arm in (o1, o0):
            util.assert_grads_match_oracle(TO, cfg, flat, caches, dl, arm[i][1], og=og)
    assert abs(l1 - _oracle((case, len(chunks) - 1), cfg, flat, chunks[-1])[3]) < 1e-4
