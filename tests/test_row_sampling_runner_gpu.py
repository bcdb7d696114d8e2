"""GPU: python -m qpnet_amd.run_decode --per_file_seed on the small synthetic corpus of test_runners_gpu: with the flag a file's wav depends on the seed and the
file alone -- not on --batch_size or the order of the list; without it (the default, the reference-like per-call stream) it does."""
import argparse
import os

import numpy as np
import pytest

from qpnet_amd import loaders, synth
from qpnet_amd.config import TINY
from test_runners_gpu import _corpus

pytestmark = pytest.mark.gpu


def _experiment(root):
    """model.conf and a final checkpoint with synthetic weights, as a training run leaves them"""
    import torch
    from qpnet_amd.qpnet import QPNet
    conf = argparse.Namespace(feature_format="npy", feature_type="world", dense_factor=8, **TINY.kwargs())
    loaders.save_model_conf(root + "/model.conf", conf)
    m = QPNet(**TINY.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(TINY, synth.make_weights(TINY, 41)).items()})
    return root + "/model.conf", loaders.save_final(root, m)


def _decode(root, conf, ckpt, out, feats, *more):
    from qpnet_amd import runners
    assert runners.run_decode(["--feats", feats, "--stats", root + "/stats.npz", "--config", conf, "--checkpoint", ckpt, "--outdir", out + "/feat_id.wav",
                               "--intervals", "100000", "--verbose", "0", "--seed", "100"] + list(more)) == 0
    wavs = {}
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), "rb") as f:
            wavs[name] = f.read()
    assert sorted(wavs) == ["u00.wav", "u01.wav", "u02.wav"]
    return wavs


def test_per_file_seed_makes_a_wav_independent_of_batch_size_and_list_order(cuda, tmp_path):
    root = _corpus(str(tmp_path / "corpus"))
    conf, ckpt = _experiment(str(tmp_path / "exp"))
    files = sorted(os.path.join(root, "feat", n) for n in os.listdir(root + "/feat"))
    fwd, rev = str(tmp_path / "fwd.txt"), str(tmp_path / "rev.txt")
    open(fwd, "w").write("\n".join(files) + "\n")
    open(rev, "w").write("\n".join(files[::-1]) + "\n")

    def run(name, feats, *more):
        return _decode(root, conf, ckpt, str(tmp_path / name), feats, *more)

    one = run("pf_b1", fwd, "--per_file_seed", "--batch_size", "1")
    three = run("pf_b3", fwd, "--per_file_seed", "--batch_size", "3")
    reverse = run("pf_rev", rev, "--per_file_seed", "--batch_size", "2")
    for name in one:
        assert len(one[name]) > 44 + 2 * 1000
        assert three[name] == one[name], "%s differs between --batch_size 1 and 3 with --per_file_seed" % name
        assert reverse[name] == one[name], "%s differs with the file list reversed (--batch_size 2) with --per_file_seed" % name
    assert len({one[n][44:44 + 2000] for n in one}) == 3                 # three files, three streams
    # without the flag the stream belongs to the call: the batch size changes the wavs (if it did not, the check above would show nothing)
    d1 = run("def_b1", fwd, "--batch_size", "1")
    d3 = run("def_b3", fwd, "--batch_size", "3")
    assert any(d1[n] != d3[n] for n in d1), "the default stream does not depend on the batch size: the comparison above is vacuous"
    assert any(d1[n] != one[n] for n in d1)                               # ... and the flag is not a no-op
