"""GPU: python -m qpnet_amd.run_validate --per_utterance on a synthetic corpus (cases.generator_corpus: three short files of the TINY geometry and one
too short to score): the per-file yml against QPNet.score on each whole file as ONE chunk, with one chunk per file and with many, and the runner
without the flag against what it has always written."""
import argparse
import os
import shutil
import types

import numpy as np
import pytest
import yaml

from cases import generator_corpus
from qpnet_amd import harness, loaders, synth
from qpnet_amd.config import TINY
import util

pytestmark = pytest.mark.gpu

FRAMES, SLACK = [14, 9, 1, 11], [7, -30, 0, 0]            # (a wav longer and one shorter than its frames: validate_length; u02 has no scored sample)
FS, DENSE = 22050, 8
FIELDS = ("samples", "nll", "bits", "top1", "top5", "entropy")


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    import torch
    from scipy.io import wavfile
    from qpnet_amd import runners
    from qpnet_amd.train import FusedTrainer
    root = str(tmp_path_factory.mktemp("score_runner"))
    U = TINY.upsampling_factor
    pcm, feats, mean, scale = generator_corpus(91, FRAMES, SLACK, U=U)
    os.makedirs(root + "/wav"); os.makedirs(root + "/feat")
    for i, (x, h) in enumerate(zip(pcm, feats)):
        wavfile.write("%s/wav/u%02d.wav" % (root, i), FS, x)
        np.save("%s/feat/u%02d.npy" % (root, i), h)
    np.savez(root + "/stats.npz", mean=mean, scale=scale)
    conf = argparse.Namespace(feature_type="world", feature_format="npy", dense_factor=DENSE, **TINY.kwargs())
    loaders.save_model_conf(root + "/model.conf", conf)
    model = util.build_model(TINY, synth.make_weights(TINY, 11), cuda)
    ck = loaders.save_final(root + "/exp", model)
    ck_b = root + "/exp/checkpoint-b.pkl"
    shutil.copy(ck, ck_b)
    common = ["--waveforms", root + "/wav", "--feats", root + "/feat", "--stats", root + "/stats.npz", "--config", root + "/model.conf", "--verbose", "0"]
    plain, scored = root + "/val_plain", root + "/val_scored"
    assert runners.run_validate(common + ["--resultdir", plain, "--checkpoint", ck, "--batch_length", "500", "--max_length", "1000"]) == 0
    files_plain = sorted(os.listdir(plain))
    assert runners.run_validate(common + ["--resultdir", scored, "--checkpoint", ck, "--per_utterance"]) == 0                     # one chunk per file
    assert runners.run_validate(common + ["--resultdir", scored, "--checkpoint", ck_b, "--per_utterance", "--batch_length", "500", "--max_length", "1000"]) == 0
    # what the runner has always computed: the mean over the un-shuffled generator's chunks of forward_loss
    args = runners._validate_args().parse_args(common + ["--resultdir", plain, "--checkpoint", ck, "--batch_length", "500", "--max_length", "1000"])
    tr = FusedTrainer(model)
    losses = [tr.forward_loss(bx, bh, bt, bd, bb, maxd=maxd) for bx, bh, bt, bd, bb, maxd in runners._batches(args, conf, model, False, 1, cuda)]
    # every file as ONE chunk through QPNet.score
    scaler = loaders.FeatureScaler(mean, scale)
    whole = {}
    for i in range(len(FRAMES)):
        x, h = harness.validate_length(pcm[i].astype(np.float32) / 32768, feats[i], U)
        d = harness.dilated_factor(harness.batch_f0(h, 0), FS, DENSE)
        rf = harness.receptive_field(TINY.receptiveCausal_field, TINY.receptiveF_field, TINY.receptiveA_field, d)
        E = (h.shape[0] - 1) * U
        if E <= rf:
            whole["u%02d" % i] = None
            continue
        xq = torch.from_numpy(loaders.mu_law_transform(TINY.n_quantize)(x)).long()
        s = model.score(xq[None, :E].to(cuda), torch.from_numpy(scaler(h[:h.shape[0] - 1])).float().t()[None].to(cuda),
                        torch.from_numpy(np.repeat(d[:h.shape[0] - 1], U)).float()[None].to(cuda), [E - rf], xq[None, 1:E + 1].to(cuda))
        tg = xq[rf + 1:E + 1].numpy()
        nll = s.nll[0].double().cpu().numpy()
        assert nll.shape == (E - rf,)
        whole["u%02d" % i] = dict(samples=E - rf, nll=nll.mean(), bits=nll.mean() / np.log(2.0), top1=(s.argmax[0].cpu().numpy() == tg).mean(),
                                  top5=(s.rank[0].cpu().numpy() < 5).mean(), entropy=s.entropy[0].double().cpu().numpy().mean(), n_frames=h.shape[0], rf=rf)
    return types.SimpleNamespace(plain=yaml.safe_load(open(plain + "/validation_result.yml")), files_plain=files_plain, losses=losses,
                                 plain_again=yaml.safe_load(open(scored + "/validation_result.yml")), files_scored=sorted(os.listdir(scored)),
                                 utt=yaml.safe_load(open(scored + "/validation_utterances.yml")), whole=whole, U=U)


def test_without_the_flag_the_runner_writes_what_it_always_did(runs):
    assert runs.files_plain == ["validation_result.yml"]
    assert len(runs.losses) >= 2
    assert runs.plain == {"checkpoint-final.pkl": float(sum(runs.losses) / len(runs.losses))}


def test_with_the_flag_the_old_file_is_unchanged_and_the_new_one_merges_by_checkpoint(runs):
    assert runs.files_scored == ["validation_result.yml", "validation_utterances.yml"]
    assert list(runs.plain_again) == ["checkpoint-b.pkl", "checkpoint-final.pkl"] and runs.plain_again["checkpoint-b.pkl"] == runs.plain["checkpoint-final.pkl"]
    assert sorted(runs.utt) == ["checkpoint-b.pkl", "checkpoint-final.pkl"]
    for rec in runs.utt.values():
        assert sorted(rec) == ["skipped", "total", "utterances"] and rec["skipped"] == ["u02"] and sorted(rec["utterances"]) == ["u00", "u01", "u03"]
        assert all(sorted(e) == sorted(FIELDS) for e in list(rec["utterances"].values()) + [rec["total"]])


@pytest.mark.parametrize("ckpt", ["checkpoint-final.pkl", "checkpoint-b.pkl"], ids=["one_chunk_per_file", "many_chunks"])
def test_per_file_numbers_are_those_of_the_whole_file_as_one_chunk(ckpt, runs):
    rec = runs.utt[ckpt]
    assert runs.whole["u02"] is None
    for fid, e in rec["utterances"].items():
        w = runs.whole[fid]
        assert e["samples"] == w["samples"] == (w["n_frames"] - 1) * runs.U - w["rf"]
        print("SCORE_RUNNER %s %s: nll %.6f (whole file %.6f), entropy %.6f (%.6f), top1 %.4f, top5 %.4f"
              % (ckpt, fid, e["nll"], w["nll"], e["entropy"], w["entropy"], e["top1"], e["top5"]))
        assert abs(e["nll"] - w["nll"]) <= 1e-4 and abs(e["entropy"] - w["entropy"]) <= 1e-4
        assert abs(e["bits"] - e["nll"] / np.log(2.0)) <= 1e-12
        # a chunk boundary moves a logit by float32 reassociation at most: an argmax or a rank flips only at a near-tie, one sample in thousands
        assert abs(e["top1"] - w["top1"]) <= 2.0 / w["samples"] and abs(e["top5"] - w["top5"]) <= 2.0 / w["samples"]


@pytest.mark.parametrize("ckpt", ["checkpoint-final.pkl", "checkpoint-b.pkl"])
def test_total_is_the_sample_weighted_combination(ckpt, runs):
    rec = runs.utt[ckpt]
    es = list(rec["utterances"].values())
    n = sum(e["samples"] for e in es)
    assert rec["total"]["samples"] == n
    for k in ("nll", "top1", "top5", "entropy"):
        assert abs(rec["total"][k] - sum(e[k] * e["samples"] for e in es) / n) <= 1e-12
    assert abs(rec["total"]["bits"] - rec["total"]["nll"] / np.log(2.0)) <= 1e-12
