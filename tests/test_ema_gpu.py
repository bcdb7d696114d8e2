"""GPU: averaged weights (an exponential moving average of the parameters) kept inside the fused optimiser step -- qpn_adam_step_avg / qpn_train_step_avg,
FusedTrainer / FlatAdam `ema_decay`, the checkpoints and run_train / run_decode / run_validate.

What the kernel does to element i, in the thread that has just written its new weight w':  e <- e + (w' - e) * omd,  omd = float32(1) - float32(decay), all fp32.
The C-ABI tests restate exactly that in numpy from the DEVICE's own new weights, so their bound is that of one line of arithmetic; the trainer tests run the
recurrence in float64 over the weights after every step."""
import ctypes as C
import os

import numpy as np
import pytest

from qpnet_amd import _lib, synth
from qpnet_amd.config import TINY
import util

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, STEP = 1e-3, 0.9, 0.999, 1e-8, 1e-3, 3
F = np.float32
EINVAL, ERANGE = -1, -4


def _to(dev, *arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


@pytest.fixture(scope="module")
def handle(cuda):
    """one TINY handle for the C-ABI tests on hand-made buffers (no forward is run on it)"""
    L = _lib.lib()
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    yield L, hp
    L.qpn_destroy(hp)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, seed, s=0.01):
    """w, g = N(0,1) * s, non-zero moments (v >= 0) -- the recipe of tests/test_grad_clip_gpu.py -- and e, an independent N(0, 0.1) vector"""
    rs = np.random.RandomState(seed)
    w = (rs.standard_normal(n) * 0.1).astype(F)
    g = (rs.standard_normal(n) * s).astype(F)
    m = (rs.standard_normal(n) * s * 0.3).astype(F)
    v = ((rs.standard_normal(n) * s) ** 2 * 0.5).astype(F)
    e = (np.random.RandomState(seed + 50000).standard_normal(n) * 0.1).astype(F)
    return w, g, m, v, e


def _dev(cuda, arrs, off):
    """device copies; off = 1: every buffer starts one float into its allocation (a base that is not 16-byte aligned)"""
    import torch
    out = []
    for a in arrs:
        t = torch.empty(a.size + off, dtype=torch.float32, device=cuda)
        t[off:].copy_(torch.from_numpy(a))
        out.append(t[off:])
        assert out[-1].data_ptr() % 16 == (4 * off) % 16
    return out


def _avg_rc(L, hp, w, g, m, v, n, max_norm, den, e, decay, step=STEP):
    return L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, B1, B2, EPS, WD,
                               den.data_ptr() if den is not None else None, max_norm, e.data_ptr() if e is not None else None, decay, _stream())


def _avg_call(*a, **kw):
    _lib.check(_avg_rc(*a, **kw))


def _applied(L, hp):
    n = C.c_int64(-1)
    _lib.check(L.qpn_train_applied_updates(hp, C.byref(n), _stream()))
    return int(n.value)


def _omd(decay):
    return F(1.0) - F(decay)


def _ema_ref(w_new, e, decay):
    """-> r, bound: the kernel's line in numpy fp32 and |e_dev - r| <= spacing(|r|) + spacing(|p|).  The contracted (one FMA) and the uncontracted form are each
    within half an ulp of the exact e + (w' - e) * omd given the rounded difference; the uncontracted one adds half an ulp of the product."""
    p = (w_new - e) * _omd(decay)
    r = e + p
    assert p.dtype == F and r.dtype == F
    return r, np.spacing(np.abs(r)) + np.spacing(np.abs(p))


SIZES = [1, 3, 255, 256, 257, 52591, 3 * 2 ** 20 + 1]        # block edges, TINY's parameter count, more than one stride of k_grad_sumsq's grid


@pytest.mark.parametrize("n,off", [(n, 0) for n in SIZES] + [(n, 1) for n in SIZES if n >= 257])
def test_one_call_against_numpy(n, off, cuda, handle):
    """qpn_adam_step_avg on hand-made buffers: unclipped, clipped (max = 0.5 |g|), with a denominator buffer {700, 0, 0, 0} (unclipped and clipped), decay 0.9 and 0.9999.
    w, m, v are torch.equal to the same call with NULL, 0 on copies; e is the numpy restatement from the device's own new weights within the bound of _ema_ref;
    g is unchanged; and e moved by more than 100 x the bound somewhere."""
    import torch
    L, hp = handle
    w0, g0, m0, v0, e0 = _buffers(n, 2000 + n % 977)
    total = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
    assert total > 0
    for den in (None, 700.0):
        gin = g0 if den is None else (g0 * F(den)).astype(F)                # the exchanged buffer holds the SUM: den * g
        dden = torch.tensor([den, 0.0, 0.0, 0.0], dtype=torch.float32, device=cuda) if den else None
        for max_norm in (0.0, 0.5 * total):
            w2, g2, m2, v2 = _dev(cuda, (w0, gin, m0, v0), off)
            _avg_call(L, hp, w2, g2, m2, v2, n, max_norm, dden, None, 0.0)
            assert not torch.equal(w2, torch.from_numpy(w0).to(cuda))       # (the step moves the weights)
            for decay in (0.9, 0.9999):
                w, g, m, v, e = _dev(cuda, (w0, gin, m0, v0, e0), off)
                _avg_call(L, hp, w, g, m, v, n, max_norm, dden, e, decay)
                assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2)
                np.testing.assert_array_equal(g.cpu().numpy(), gin)
                eg = e.cpu().numpy()
                r, bound = _ema_ref(w.cpu().numpy(), e0, decay)
                err = np.abs(eg.astype(np.float64) - r.astype(np.float64))
                moved = np.abs(eg.astype(np.float64) - e0.astype(np.float64))
                print("n %d off %d den %s max_norm %.3g decay %g: max err / bound %.3f, max moved / bound %.3g" % (
                    n, off, den, max_norm, decay, (err / bound).max(), (moved / bound).max()))
                assert (err <= bound).all()
                assert (moved > 100 * bound).any()
    assert L.qpn_train_status(hp, _stream()) == 0


def test_skipped_updates_leave_the_average_alone(cuda, handle):
    """(a) an inf, then a NaN, in g with clipping on; (b) a peer rank's flag in the denominator buffer {700, 1, 0, 0}, clipped and not: e, w, m, v are torch.equal to
    their inputs and the applied-update count stays; once qpn_train_status has been read a clean call applies and moves e.  With clipping off the poisoned buffer is
    stepped as it always was: averaging adds no flag of its own."""
    import torch
    L, hp = handle
    n = 52591
    arrs = _buffers(n, 31)
    total = float(np.sqrt((arrs[1].astype(np.float64) ** 2).sum()))
    ins = [torch.from_numpy(a).to(cuda) for a in arrs]

    def untouched(w, m, v, e):
        return torch.equal(w, ins[0]) and torch.equal(m, ins[2]) and torch.equal(v, ins[3]) and torch.equal(e, ins[4])

    # (the handle's training state -- the status word -- exists from the first clipping call on)
    w, g, m, v, e = _dev(cuda, arrs, 0)
    _avg_call(L, hp, w, g, m, v, n, 0.5 * total, None, e, 0.9)
    assert L.qpn_train_status(hp, _stream()) == 0 and not torch.equal(e, ins[4])
    for poison in (np.inf, np.nan):
        w, g, m, v, e = _dev(cuda, arrs, 0)
        g[n // 3] = poison
        before = _applied(L, hp)
        _avg_call(L, hp, w, g, m, v, n, 0.5 * total, None, e, 0.9)
        assert untouched(w, m, v, e) and _applied(L, hp) == before
        assert L.qpn_train_status(hp, _stream()) == ERANGE and b"non-finite" in L.qpn_last_error()
        g[n // 3] = 0.0
        _avg_call(L, hp, w, g, m, v, n, 0.5 * total, None, e, 0.9)
        assert _applied(L, hp) == before + 1 and not torch.equal(e, ins[4]) and not torch.equal(w, ins[0])
        assert L.qpn_train_status(hp, _stream()) == 0
        # clipping off: stepped as ever, nothing flagged, and the average follows the (poisoned) step
        g[n // 3] = poison
        e1 = e.clone()
        _avg_call(L, hp, w, g, m, v, n, 0.0, None, e, 0.9)
        assert L.qpn_train_status(hp, _stream()) == 0 and _applied(L, hp) == before + 2
        assert not torch.equal(e[:n // 3], e1[:n // 3])
    for max_norm in (0.0, 0.5 * total):
        w, g, m, v, e = _dev(cuda, arrs, 0)
        den = torch.tensor([700.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=cuda)
        before = _applied(L, hp)
        _avg_call(L, hp, w, g, m, v, n, max_norm, den, e, 0.9)
        assert untouched(w, m, v, e) and _applied(L, hp) == before
        assert L.qpn_train_status(hp, _stream()) == ERANGE and b"peer rank" in L.qpn_last_error()
        den[1] = 0.0
        _avg_call(L, hp, w, g, m, v, n, max_norm, den, e, 0.9)
        assert _applied(L, hp) == before + 1 and not torch.equal(e, ins[4])
        assert L.qpn_train_status(hp, _stream()) == 0


def test_argument_errors_touch_nothing_and_null_zero_is_the_clip_call(cuda, handle):
    """decay 0 with a buffer, 1.0, -0.1, NaN, a decay with d_ema = NULL: QPN_EINVAL and every buffer as it was.  qpn_adam_step_avg(NULL, 0) gives
    qpn_adam_step_clip's bits, clipped and not."""
    import torch
    L, hp = handle
    n = 52591
    arrs = _buffers(n, 41)
    total = float(np.sqrt((arrs[1].astype(np.float64) ** 2).sum()))
    ins = [torch.from_numpy(a).to(cuda) for a in arrs]
    w, g, m, v, e = _dev(cuda, arrs, 0)
    before = _applied(L, hp)
    for given, decay, word in ((True, 0.0, b"ema_decay"), (True, 1.0, b"ema_decay"), (True, -0.1, b"ema_decay"), (True, float("nan"), b"ema_decay"), (False, 0.9, b"d_ema")):
        for max_norm in (0.0, 0.5 * total):
            assert _avg_rc(L, hp, w, g, m, v, n, max_norm, None, e if given else None, decay) == EINVAL
            assert word in L.qpn_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(t, i) for t, i in zip((w, g, m, v, e), ins)) and _applied(L, hp) == before
    for max_norm in (0.0, 0.5 * total):
        w, g, m, v = _dev(cuda, arrs[:4], 0)
        w2, g2, m2, v2 = _dev(cuda, arrs[:4], 0)
        _avg_call(L, hp, w, g, m, v, n, max_norm, None, None, 0.0)
        _lib.check(L.qpn_adam_step_clip(hp, w2.data_ptr(), g2.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, STEP, LR, B1, B2, EPS, WD, None, max_norm, _stream()))
        assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2) and not torch.equal(w, ins[0])


# ---------------------------------------------------------------- through the trainers
CHUNKS = [(144, 676), (383, 631), (12, 640), (295, 607), (378, 648)]        # the five chunks of tests/test_grad_clip_gpu.py
WSEED = 12
DECAY = 0.9


def _chunk(cuda, k):
    seed, bl = CHUNKS[k]
    x, h, t, d, b = synth.train_inputs(TINY, bl, seed, 30000)
    return _to(cuda, x, h, t, d, b)


def _recurrence(w_init, applied, decay=DECAY):
    """the average in float64: seeded with the initial weights, moved by the weights after every APPLIED step with the kernel's own fp32 factor"""
    omd = float(_omd(decay))
    e = np.asarray(w_init, dtype=np.float64).copy()
    for w in applied:
        e = e + (np.asarray(w, dtype=np.float64) - e) * omd
    return e


def _tol(nsteps, e):
    """nsteps steps, at most two fp32 roundings each at the largest magnitude"""
    return nsteps * 2 * 2.0 ** -23 * float(np.abs(e).max())


def _five_steps(cuda, want_loss, **kw):
    from qpnet_amd.train import FusedTrainer
    w_init = synth.make_weights(TINY, WSEED)
    m = util.build_model(TINY, w_init, cuda).train()
    tr = FusedTrainer(m, lr=1e-3, ema_decay=DECAY, **kw)
    snaps, norms = [], []
    for k in range(5):
        tr.step(*_chunk(cuda, k), want_loss=want_loss)
        snaps.append(m.flat_parameters().cpu().numpy())
        norms.append(tr.last_grad_norm)
    if want_loss == "lagged":
        assert tr.flush_loss() is not None
    tr.check_status()
    assert tr.step_count == 5
    return tr, m, w_init, snaps, norms


def _check_against_recurrence(tr, w_init, snaps):
    ref = _recurrence(w_init, snaps)
    e = tr.ema.cpu().numpy().astype(np.float64)
    tol = _tol(len(snaps), ref)
    err = np.abs(e - ref).max()
    far_w, far_0 = np.abs(e - snaps[-1]).max(), np.abs(e - w_init).max()
    print("max |e - recurrence| %.3e (bound %.3e); max |e - w_final| %.3e, max |e - w_init| %.3e" % (err, tol, far_w, far_0))
    assert err <= tol
    assert far_w > 100 * tol and far_0 > 100 * tol


@pytest.fixture(scope="module")
def five(cuda):
    """the five steps with want_loss=True (shared: the recurrence test, the decode test)"""
    return _five_steps(cuda, True)


def test_fused_trainer_average_is_the_recurrence_over_its_weights(five):
    tr, m, w_init, snaps, _ = five
    assert tr.ema.dtype.is_floating_point and tr.ema.numel() == TINY.n_params and tr.ema.is_cuda
    _check_against_recurrence(tr, w_init, snaps)


@pytest.mark.parametrize("want_loss", ["lagged", False])
def test_every_loss_mode_moves_the_average(want_loss, cuda):
    tr, m, w_init, snaps, _ = _five_steps(cuda, want_loss)
    _check_against_recurrence(tr, w_init, snaps)


def test_world2_identity_exchange_moves_the_average(cuda):
    """world_size=2 without a process group: the step-by-step path (qpn_adam_step_avg) with the denominator buffer in use"""
    tr, m, w_init, snaps, _ = _five_steps(cuda, True, world_size=2)
    _check_against_recurrence(tr, w_init, snaps)


@pytest.mark.parametrize("kw", [{}, {"world_size": 2}])
def test_clipped_steps_move_the_average(kw, cuda):
    """max_grad_norm = the median of the five unclipped norms: the clipping and averaging instance of k_adam runs, with clipped and unclipped steps"""
    norms = _five_steps(cuda, True, max_grad_norm=1e30)[4]
    c = float(np.median(norms))
    assert sum(v > c for v in norms) == 2 and sum(v < c for v in norms) == 2, norms
    tr, m, w_init, snaps, norms = _five_steps(cuda, True, max_grad_norm=c, **kw)
    assert max(norms) > c > min(norms)
    _check_against_recurrence(tr, w_init, snaps)


def test_flat_adam_average_is_the_recurrence_over_its_weights(cuda):
    """FlatAdam(ema_decay=...) in the reference-style loop: three steps, .ema against the recurrence, ema_state_dict() in the model's layout"""
    import torch
    from qpnet_amd.train import FlatAdam
    w_init = synth.make_weights(TINY, WSEED)
    m = util.build_model(TINY, w_init, cuda).train()
    opt = FlatAdam(m, lr=1e-3, ema_decay=DECAY)
    snaps = []
    for k in range(3):
        xt, ht, tt, dt, bt = _chunk(cuda, k)
        out = m(xt, ht, dt, bt)
        loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, TINY.n_quantize), tt[:, -out.shape[1]:].reshape(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        snaps.append(m.flat_parameters().cpu().numpy())
    m.check_status()
    _check_against_recurrence(opt, w_init, snaps)
    sd = opt.ema_state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys()) and all(sd[k].shape == v.shape for k, v in m.state_dict().items())
    assert torch.equal(torch.cat([v.reshape(-1) for v in sd.values()]), opt.ema)


def test_a_flagged_chunk_is_not_averaged(cuda):
    """a target outside [0, n_quantize) in the second of five chunks (a status flag, as tests/test_runners_gpu.py provokes it): that step raises, applies nothing and
    leaves the average where it was; after the sequence the average is the recurrence over the four APPLIED states."""
    import torch
    from qpnet_amd.train import FusedTrainer
    w_init = synth.make_weights(TINY, WSEED)
    m = util.build_model(TINY, w_init, cuda).train()
    tr = FusedTrainer(m, lr=1e-3, ema_decay=DECAY)
    applied = []
    for k in range(5):
        xt, ht, tt, dt, bt = _chunk(cuda, k)
        if k == 1:
            tt = tt.clone(); tt[0, -3] = 999
            w_before, e_before = m.flat_parameters().clone(), tr.ema.clone()
            with pytest.raises(_lib.QpnError) as err:
                tr.step(xt, ht, tt, dt, bt, want_loss=True)
            assert err.value.code == ERANGE
            assert torch.equal(m.flat_parameters(), w_before) and torch.equal(tr.ema, e_before)
            continue
        tr.step(xt, ht, tt, dt, bt, want_loss=True)
        applied.append(m.flat_parameters().cpu().numpy())
    tr.check_status()
    assert tr.step_count == 4
    ref = _recurrence(w_init, applied)
    e = tr.ema.cpu().numpy().astype(np.float64)
    tol = _tol(4, ref)
    print("max |e - recurrence over the applied states| %.3e (bound %.3e)" % (np.abs(e - ref).max(), tol))
    assert np.abs(e - ref).max() <= tol
    # (a recurrence that counted the flagged step's unchanged weights once more is off by 0.9 |w1 - w0| * omd * decay^3 = 6.6e-5 where Adam's first step moved an
    #  element by lr: more than ten times the bound)
    assert np.abs(e - _recurrence(w_init, applied[:1] + applied[:1] + applied[1:])).max() > 10 * tol


def test_decode_and_validation_use_the_average(five, cuda, oracle):
    """ema_state_dict() copied into a fresh model: its greedy decode of a 3-frame utterance is the oracle's with those weights, bit for bit, and not the live weights'
    stream; forward_loss(weights="ema") is the fresh model's forward_loss (1e-6) and not the live model's."""
    import torch
    from qpnet_amd.train import FusedTrainer
    tr, m, w_init, snaps, _ = five
    sd = tr.ema_state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert sd[k].shape == v.shape and sd[k].dtype == torch.float32
    eflat = tr.ema.cpu().numpy()
    fresh = util.build_model(TINY, w_init, cuda)
    fresh.load_state_dict(sd)
    np.testing.assert_array_equal(fresh.flat_parameters().cpu().numpy(), eflat)
    x, h, d, n = synth.decode_inputs(TINY, 3, 21, 1.0)
    args = (torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda))
    got = fresh.batch_fast_generate(*args, [n], d[None], mode="argmax")[0]
    np.testing.assert_array_equal(got, oracle.decode(TINY, eflat, h, d, x, n)["samples"])
    live = util.build_model(TINY, snaps[-1], cuda).batch_fast_generate(*args, [n], d[None], mode="argmax")[0]
    assert not np.array_equal(got, live)
    chunk = _chunk(cuda, 2)
    l_ema = tr.forward_loss(*chunk, weights="ema")
    l_model = tr.forward_loss(*chunk, weights="model")
    l_fresh = FusedTrainer(fresh).forward_loss(*chunk)
    print("loss ema %.7f fresh %.7f model %.7f" % (l_ema, l_fresh, l_model))
    assert abs(l_ema - l_fresh) <= 1e-6
    assert abs(l_ema - l_model) > 1e-4
    assert abs(tr.forward_loss(*chunk) - l_model) <= 1e-6                   # (the default is the live weights, which the call with "ema" did not touch)
    np.testing.assert_array_equal(m.flat_parameters().cpu().numpy(), snaps[-1])
    with pytest.raises(RuntimeError, match="ema_decay is off"):
        FusedTrainer(fresh).forward_loss(*chunk, weights="ema")


# ---------------------------------------------------------------- runners
def _corpus(root):
    """the corpus of tests/test_grad_clip_gpu.py::test_run_train_reports_the_norm_and_clips"""
    from qpnet_amd import loaders
    from scipy.io import wavfile
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    rs = np.random.RandomState(5)
    feats = []
    for i in range(3):
        h = synth.make_features(45 + 3 * i, 700 + i)
        wavfile.write("%s/wav/u%02d.wav" % (root, i), 22050, (rs.uniform(-0.8, 0.8, (45 + 3 * i) * TINY.upsampling_factor + 11) * 32767).astype(np.int16))
        np.save("%s/feat/u%02d.npy" % (root, i), h)
        feats.append(h)
    st = loaders.calc_stats(feats)
    np.savez(root + "/stats.npz", mean=st.mean_, scale=st.scale_)
    return root


GEO = ["--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2", "--dilationF_repeat", "1", "--dilationA_depth", "1",
       "--dilationA_repeat", "1", "--feature_format", "npy", "--batch_length", "1500", "--max_length", "4000", "--verbose", "1"]


def _flat_sd(sd):
    import torch
    return torch.cat([v.reshape(-1).float() for v in sd.values()])


def test_runners_write_resume_decode_and_validate_the_average(cuda, tmp_path, monkeypatch):
    """run_train --iters 4 --ema_decay 0.9: the final file and the checkpoints carry "ema" in the model's layout, away from "model"; --resume from the run's
    2-iteration checkpoint reproduces the 4-iteration average (atol 2e-6: two runs of one backward, the weight bound of tests/test_grad_clip_gpu.py);
    run_decode --ema / run_validate --ema write what a model loaded from ck["ema"] gives and not what ck["model"] gives; without --ema_decay the files hold
    exactly the old keys and --ema on them fails with the clear error.

    A resumed run restarts the shuffled chunk stream from its beginning (as the reference does), so iterations 3-4 of a resumed run see the chunks iterations 1-2
    saw.  For the resumed and the uninterrupted run to be the same computation both training runs here are fed a stream of period two: the generator's first
    two chunks, repeated."""
    import torch
    import yaml
    from qpnet_amd import loaders, runners
    from qpnet_amd.train import FusedTrainer
    from scipy.io import wavfile
    root = _corpus(str(tmp_path / "corpus"))
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz"]
    batches = runners._batches

    def period_two(*a, **kw):
        gen = batches(*a, **kw)
        first = [next(gen), next(gen)]
        torch.cuda.synchronize()                                            # (the staged copies have landed)
        first = [tuple(t.clone() if torch.is_tensor(t) else t for t in b) for b in first]
        while True:
            yield from first

    def train(exp, extra, two=True):
        os.makedirs(exp)
        with monkeypatch.context() as mp:
            if two:
                mp.setattr(runners, "_batches", period_two)
            assert runners.run_train(common + GEO + ["--expdir", exp, "--config", exp + "/model.conf", "--iters", "4", "--checkpoint_interval", "2",
                                                     "--intervals", "2"] + extra) == 0
        return torch.load(exp + "/checkpoint-final.pkl", map_location="cpu", weights_only=False)

    exp = str(tmp_path / "ema")
    fin = train(exp, ["--ema_decay", "0.9", "--resume", exp + "/none.pkl"])
    assert list(fin.keys()) == ["model", "ema", "ema_decay"] and fin["ema_decay"] == 0.9
    assert list(fin["ema"].keys()) == list(fin["model"].keys())
    assert all(fin["ema"][k].shape == v.shape for k, v in fin["model"].items())
    assert float((_flat_sd(fin["ema"]) - _flat_sd(fin["model"])).abs().max()) > 1e-5
    ck2 = torch.load(exp + "/checkpoint-2.pkl", map_location="cpu", weights_only=False)
    assert list(ck2.keys()) == ["model", "optimizer", "iterations", "ema", "ema_decay"] and ck2["iterations"] == 2
    assert float((_flat_sd(ck2["ema"]) - _flat_sd(fin["ema"])).abs().max()) > 1e-5
    # resume
    exp2 = str(tmp_path / "resumed")
    fin2 = train(exp2, ["--ema_decay", "0.9", "--resume", exp + "/checkpoint-2.pkl"])
    d_e = float((_flat_sd(fin2["ema"]) - _flat_sd(fin["ema"])).abs().max())
    d_w = float((_flat_sd(fin2["model"]) - _flat_sd(fin["model"])).abs().max())
    print("resumed vs uninterrupted: max |de| %.3e, max |dw| %.3e" % (d_e, d_w))
    assert d_e <= 2e-6 and d_w <= 2e-6
    # decode with the average
    conf = exp + "/model.conf"
    dec = ["--feats", root + "/feat", "--stats", root + "/stats.npz", "--config", conf, "--checkpoint", exp + "/checkpoint-final.pkl",
           "--batch_size", "3", "--mode", "argmax", "--intervals", "2000", "--verbose", "0"]
    assert runners.run_decode(dec + ["--outdir", str(tmp_path / "wav_ema") + "/feat_id.wav", "--ema"]) == 0
    assert runners.run_decode(dec + ["--outdir", str(tmp_path / "wav_model") + "/feat_id.wav"]) == 0
    for name, key in (("ema_only.pkl", "ema"), ("model_only.pkl", "model")):
        torch.save({"model": fin[key]}, str(tmp_path / name))
        assert runners.run_decode(dec[:6] + ["--checkpoint", str(tmp_path / name)] + dec[8:] + ["--outdir", str(tmp_path / ("ref_" + key)) + "/feat_id.wav"]) == 0
    differ = 0
    for i in range(3):
        got = wavfile.read("%s/u%02d.wav" % (tmp_path / "wav_ema", i))[1]
        np.testing.assert_array_equal(got, wavfile.read("%s/u%02d.wav" % (tmp_path / "ref_ema", i))[1])
        np.testing.assert_array_equal(wavfile.read("%s/u%02d.wav" % (tmp_path / "wav_model", i))[1], wavfile.read("%s/u%02d.wav" % (tmp_path / "ref_model", i))[1])
        differ += not np.array_equal(got, wavfile.read("%s/u%02d.wav" % (tmp_path / "ref_model", i))[1])
    assert differ > 0
    # validate with the average
    val = common + ["--config", conf, "--batch_length", "1500", "--max_length", "4000", "--verbose", "0"]
    losses = {}
    for tag, ck, extra in (("ema", exp + "/checkpoint-final.pkl", ["--ema"]), ("model", exp + "/checkpoint-final.pkl", []),
                           ("ref_ema", str(tmp_path / "ema_only.pkl"), []), ("ref_model", str(tmp_path / "model_only.pkl"), [])):
        res = str(tmp_path / ("val_" + tag))
        assert runners.run_validate(val + ["--resultdir", res, "--checkpoint", ck] + extra) == 0
        losses[tag] = list(yaml.safe_load(open(res + "/validation_result.yml")).values())[0]
    print("validation losses", losses)
    assert abs(losses["ema"] - losses["ref_ema"]) <= 1e-6 and abs(losses["model"] - losses["ref_model"]) <= 1e-6
    assert abs(losses["ema"] - losses["model"]) > 1e-5
    # without --ema_decay: today's keys, and --ema fails clearly
    exp3 = str(tmp_path / "plain")
    fin3 = train(exp3, ["--resume", exp3 + "/none.pkl"], two=False)
    assert list(fin3.keys()) == ["model"]
    assert list(torch.load(exp3 + "/checkpoint-2.pkl", map_location="cpu", weights_only=False).keys()) == ["model", "optimizer", "iterations"]
    with pytest.raises(KeyError, match="no averaged weights"):
        runners.run_decode(dec[:6] + ["--checkpoint", exp3 + "/checkpoint-final.pkl"] + dec[8:] + ["--outdir", str(tmp_path / "nope") + "/feat_id.wav", "--ema"])
    with pytest.raises(KeyError, match="no averaged weights"):
        runners.run_validate(val + ["--resultdir", str(tmp_path / "val_nope"), "--checkpoint", exp3 + "/checkpoint-final.pkl", "--ema"])
