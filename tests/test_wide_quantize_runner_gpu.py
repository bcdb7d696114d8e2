"""GPU: python -m qpnet_amd.run_decode with a 512-class model, in its default (sampling) mode with --per_file_seed, on a synthetic two-file corpus: the wavs are
loaders.samples_to_int16 of what the module call draws for those files with their keys."""
import argparse
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from qpnet_amd import loaders, synth
from qpnet_amd.config import TINY
from test_runners_gpu import _corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dataclasses.replace(TINY, n_resch=64, n_skipch=64, n_quantize=512)
SEED = 100


def _experiment(root):
    """model.conf and a final checkpoint with synthetic weights, as a training run leaves them"""
    import torch
    from qpnet_amd.qpnet import QPNet
    os.makedirs(root)
    conf = argparse.Namespace(feature_format="npy", feature_type="world", dense_factor=8, **CFG.kwargs())
    loaders.save_model_conf(root + "/model.conf", conf)
    m = QPNet(**CFG.kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.weights_to_state_dict(CFG, synth.make_weights(CFG, 41)).items()})
    return root + "/model.conf", loaders.save_final(root, m)


def test_run_decode_writes_the_module_calls_samples_at_512_classes(cuda, tmp_path):
    import torch
    from scipy.io import wavfile
    from qpnet_amd import runners
    from qpnet_amd.qpnet import encode_mu_law
    root = _corpus(str(tmp_path / "corpus"), n=2, frames=3)            # 3 and 6 feature frames: 330 and 660 samples
    conf_path, ckpt = _experiment(str(tmp_path / "exp"))
    files = sorted(os.path.join(root, "feat", n) for n in os.listdir(root + "/feat"))
    lst = str(tmp_path / "feats.txt")
    open(lst, "w").write("\n".join(files) + "\n")
    out = str(tmp_path / "wav")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "qpnet_amd.run_decode", "--feats", lst, "--stats", root + "/stats.npz", "--config", conf_path, "--checkpoint", ckpt,
                        "--outdir", out + "/feat_id.wav", "--intervals", "100000", "--verbose", "0", "--seed", str(SEED), "--per_file_seed", "--batch_size", "2"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == ["u00.wav", "u01.wav"]
    # the module call on the same two files, with the keys run_decode derives for them
    conf = loaders.load_model_conf(conf_path)
    assert conf.n_quantize == 512
    with torch.no_grad():
        model = runners._build_model(conf, cuda).eval()
        loaders.load_checkpoint(ckpt, model, None)
        feats = [loaders.read_features(f, conf.feature_type) for f in files]
        gen = loaders.decode_generator(feats, 22050, ["u00", "u01"], wav_transform=lambda x: encode_mu_law(x, conf.n_quantize),
                                       feat_transform=loaders.read_scaler_stats(root + "/stats.npz", conf.feature_type), dense_factor=conf.dense_factor, batch_size=2,
                                       upsampling_factor=conf.upsampling_factor, f0_factor=1.0, f0_dim_index=1, extra_memory=False, device=cuda)
        seen = 0
        for feat_ids, bx, bh, ns, bd in gen:
            outs = model.batch_fast_generate(bx, bh, ns, bd, mode="sampling", row_seeds=[loaders.row_seed(SEED, i) for i in feat_ids])
            for feat_id, samples in zip(feat_ids, outs):
                fs, pcm = wavfile.read("%s/%s.wav" % (out, feat_id))
                assert fs == 22050 and pcm.dtype == np.int16 and len(samples) >= 300
                np.testing.assert_array_equal(pcm, loaders.samples_to_int16(samples, 512), err_msg=feat_id)
                assert len(np.unique(samples)) >= 64 and (samples >= 256).sum() >= 16 and samples.max() < 512      # a draw over the 512 classes
                seen += 1
        assert seen == 2
