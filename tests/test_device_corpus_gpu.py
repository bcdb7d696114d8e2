"""GPU: the device-resident corpus -- qpn_cut_chunks against train_generator bit for bit over the cases of tests/device_corpus_spec.py and at tile edges,
the hand-over of its batches from the prefetch thread to a trainer on a non-blocking stream through train.join_staged, the entry point's refusal of a bad
table with real buffers, and run_train --device_corpus against the plain run."""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

from qpnet_amd import _lib, loaders, synth
from qpnet_amd.config import TINY

import device_corpus_spec as S

pytestmark = pytest.mark.gpu

UW = 0.25


def device_batches(utts, U, n_aux, kw, cuda, seed=7, uw=UW, **geom):
    import torch
    c = S.corpus(utts, U, n_aux, cuda)
    np.random.seed(seed)
    p = S.plan_kwargs(U, n_aux, kw, **geom)
    out = list(loaders.device_train_generator(c, *S.FIELDS, p["batch_length"], p["batch_size"], p["max_length"], p["shuffle"], p["epochs"], p["shard"], uw))
    torch.cuda.synchronize()
    return out


def same(got_batches, want_batches, cuda):
    """every batch of the device generator is train_generator's batch moved to the device: values, dtypes, shapes, contiguity"""
    import torch
    assert len(got_batches) == len(want_batches) and len(want_batches) > 0
    for got, want in zip(got_batches, want_batches):
        gx, gh, gt, gd, gb, gmaxd, gw = got
        wx, wh, wt, wd, wb, wmaxd, ww = want
        for name, g, w in (("x", gx, wx), ("h", gh, wh), ("t", gt, wt), ("d", gd, wd), ("w", gw, ww)):
            w = w.to(cuda)
            assert g.device == w.device and g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous(), name
            assert torch.equal(g, w), "%s differs in %d of %d elements" % (name, int((g != w).sum()), g.numel())
        assert gb.device.type == "cpu" and gb.dtype == torch.int64 and gb.tolist() == wb
        assert type(gmaxd) is int and gmaxd == wmaxd


@pytest.mark.parametrize("U,n_aux", sorted(S.GEOMETRIES))
@pytest.mark.parametrize("case", sorted(S.cases(5, 3)))
def test_device_batches_equal_the_host_generators(case, U, n_aux, cuda):
    utts, kw = S.cases(U, n_aux)[case]
    same(device_batches(utts, U, n_aux, kw, cuda), S.host_batches(utts, U, n_aux, kw, UW), cuda)


# (U, n_aux, frames, batch_size): T = 85 and 65 are no multiples of 64 (nor of 4: rows start at every alignment, four-element groups straddle rows, the batch ends
# in a partial group); frames = 17 and 33 are one more than a multiple of the 16- and 32-frame tiles; n_aux = 39 is one full feature tile and a partial one
@pytest.mark.parametrize("U,n_aux,frames,batch_size", [(5, 3, 17, 2), (5, 3, 13, 3), (110, 39, 33, 1), (5, 39, 33, 3)])
def test_tile_edges(U, n_aux, frames, batch_size, cuda):
    rf = S.FIELDS[0] + S.FIELDS[1] + S.FIELDS[2] * 19      # a constant 150 Hz pitch: d = 22050 / 150 / 8 = 18.375
    utts = [S.utterance(frames * (batch_size + 1) + 2 + k, U, n_aux, 60 + k, f0=150.0) for k in range(3)]
    kw = dict(batch_size=batch_size, shuffle=False, epochs=1, shard=None)
    geom = dict(batch_length=frames * U - rf, max_length=10 ** 6)
    want = S.host_batches(utts, U, n_aux, kw, UW, **geom)
    assert all(b[0].shape == (batch_size, frames * U) and b[1].shape[2] == frames for b in want)
    same(device_batches(utts, U, n_aux, kw, cuda, **geom), want, cuda)


def test_without_weights_the_batch_has_six_elements(cuda):
    utts, kw = S.cases(5, 3)["a_one_long_utterance"]
    got = device_batches(utts, 5, 3, kw, cuda, uw=None)
    want = S.host_batches(utts, 5, 3, kw, UW)
    assert all(len(b) == 6 for b in got)
    same([b + (w[6].to(cuda),) for b, w in zip(got, want)], want, cuda)


def _tiny_model(cuda):
    import torch
    from qpnet_amd.qpnet import QPNet
    flat = synth.make_weights(TINY, 11)
    m = QPNet(**TINY.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(TINY, flat).items()})
    return m.to(cuda).train()


def test_hand_over_from_the_prefetch_thread_to_a_trainer_on_its_own_stream(cuda):
    """The generator enqueues on its own stream from a Prefetcher thread; three FusedTrainer.step calls on a non-blocking stream consume its batches through the
    join every staged batch goes through.  The inputs are bit for bit the host generator's, so the first loss may differ by the project's loss-parity bound at most."""
    import torch
    from qpnet_amd.runners import Prefetcher
    from qpnet_amd.train import FusedTrainer
    U, n_aux = TINY.upsampling_factor, TINY.n_aux
    utts, kw = S.cases(U, n_aux)["e_shuffle_two_epochs"]
    want = S.host_batches(utts, U, n_aux, kw, UW)[:3]

    def run(batches, on_stream):
        tr = FusedTrainer(_tiny_model(cuda), lr=1e-4)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(cuda)
        s.wait_stream(torch.cuda.current_stream(cuda))
        losses = []
        with torch.cuda.stream(s):
            for k in range(3):
                bx, bh, bt, bd, bb, maxd, bw = next(batches)
                if on_stream:
                    assert "_qpn_staged" in bx.__dict__
                losses.append(tr.step(bx, bh, bt, bd, bb, want_loss=True, maxd=maxd, sample_weights=bw))
                assert "_qpn_staged" not in bx.__dict__
            tr.check_status()
        s.synchronize()
        return losses
    host = run(iter([tuple(t.to(cuda) if hasattr(t, "to") else t for t in b[:4]) + (torch.tensor(b[4]), b[5], b[6].to(cuda)) for b in want]), False)
    c = S.corpus(utts, U, n_aux, cuda)
    np.random.seed(7)
    p = S.plan_kwargs(U, n_aux, kw)
    dev = run(Prefetcher(loaders.device_train_generator(c, *S.FIELDS, p["batch_length"], p["batch_size"], p["max_length"], p["shuffle"], p["epochs"], p["shard"], UW)), True)
    print("DEVICE_CORPUS hand-over losses: host %r device %r" % (host, dev))
    assert all(np.isfinite(host)) and all(np.isfinite(dev))
    assert abs(dev[0] - host[0]) < 1e-4


def test_a_bad_host_table_is_refused_and_nothing_is_written(cuda):
    """The device copy of the table is fine; the host copy has one segment past the arena end: QPN_ERANGE names it, and nothing was launched (an argument check:
    no bad index ever reaches the kernel)."""
    import torch
    U, n_aux = 5, 3
    utts, kw = S.cases(U, n_aux)["b_short_utterances"]
    c = S.corpus(utts, U, n_aux, cuda)
    rows, frames, bl, mine, maxd = next(loaders.plan_device_batches(c, *S.FIELDS, **S.plan_kwargs(U, n_aux, kw)))
    recs, first = loaders.corpus_segment_table(rows, frames, U)
    blob = np.concatenate([recs.view(np.uint8), first.view(np.uint8)])
    table = torch.from_numpy(blob).to(cuda)
    bad = recs.copy()
    k = len(bad) - 1
    bad["sample0"][k] = c.n_samples - bad["n_samples"][k] + 1
    T = frames * U
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device=cuda) for n in (8 * T, 8 * T, 4 * n_aux * frames, 4 * T, 4 * bl)]
    torch.cuda.synchronize()
    L = _lib.lib()

    def call(h_recs):
        return L.qpn_cut_chunks(c.samples.data_ptr(), c.n_samples, c.feats.data_ptr(), c.factors.data_ptr(), c.n_frames, n_aux, h_recs.ctypes.data, first.ctypes.data,
                                table.data_ptr(), table.data_ptr() + recs.nbytes, len(recs), 1, frames, U, bl, C.c_float(UW),
                                *[o.data_ptr() for o in outs], torch.cuda.current_stream(cuda).cuda_stream)
    rc = call(bad)
    msg = L.qpn_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -4 and "row 0 segment %d" % k in msg, (rc, msg)
    assert all(bool((o == 0x5A).all()) for o in outs)
    assert call(recs) == 0                                  # ... and the same call with the good host copy cuts the batch
    torch.cuda.synchronize()
    want = S.host_batches(utts, U, n_aux, kw, UW)[0]
    assert torch.equal(outs[0].view(torch.int64).view(1, T), want[0].to(cuda)) and torch.equal(outs[4].view(torch.float32).view(1, bl), want[6].to(cuda))


def _file_corpus(root, n=3, frames=45):
    """the corpus of tests/test_runners_gpu.py, built again: .wav + .npy features + stats"""
    from scipy.io import wavfile
    U = TINY.upsampling_factor
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    rs = np.random.RandomState(5)
    feats = []
    for i in range(n):
        h = synth.make_features(frames + 3 * i, 700 + i)
        x = (rs.uniform(-0.8, 0.8, (frames + 3 * i) * U + 11) * 32767).astype(np.int16)
        wavfile.write("%s/wav/u%02d.wav" % (root, i), 22050, x)
        np.save("%s/feat/u%02d.npy" % (root, i), h)
        feats.append(h)
    st = loaders.calc_stats(feats)
    np.savez(root + "/stats.npz", mean=st.mean_, scale=st.scale_)
    return root


def test_run_train_with_the_device_corpus(cuda, tmp_path):
    from qpnet_amd import runners
    root = _file_corpus(str(tmp_path / "corpus"))
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz", "--n_resch", "32", "--n_skipch", "32", "--dilationF_depth", "2",
              "--dilationF_repeat", "1", "--dilationA_depth", "1", "--dilationA_repeat", "1", "--feature_format", "npy", "--batch_length", "1500", "--max_length", "4000",
              "--verbose", "0", "--iters", "4", "--intervals", "1", "--unvoiced_weight", "0.5"]
    recs = {}
    for name, extra in (("plain", []), ("device", ["--device_corpus"])):
        exp = str(tmp_path / name)
        assert runners.run_train(common + extra + ["--expdir", exp, "--config", exp + "/model.conf", "--resume", exp + "/none.pkl"]) == 0
        recs[name] = yaml.safe_load(open(exp + "/loss-final.yml"))
    assert sorted(os.listdir(str(tmp_path / "plain"))) == sorted(os.listdir(str(tmp_path / "device")))
    print("DEVICE_CORPUS run_train losses: plain %r device %r" % (recs["plain"], recs["device"]))
    assert len(recs["device"]) == 4 and all(np.isfinite(recs["device"]))
    assert abs(recs["device"][0] - recs["plain"][0]) < 1e-4
    conf = loaders.load_model_conf(str(tmp_path / "device") + "/model.conf")
    assert not any("device_corpus" in k for k in vars(conf))
    assert vars(conf).keys() == vars(loaders.load_model_conf(str(tmp_path / "plain") + "/model.conf")).keys()
