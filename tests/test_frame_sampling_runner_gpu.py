"""GPU: python -m qpnet_amd.run_decode with --<control>_voiced / _unvoiced on the small synthetic corpus of test_runners_gpu: equal values are the plain flags'
wavs byte for byte; different values leave a file's wav alone up to the first sample of the first frame whose uv flag selects the other value, change it
after that, and (with --per_file_seed) do not make it depend on --batch_size."""
import os

import numpy as np
import pytest

from qpnet_amd import loaders
from qpnet_amd.config import TINY
from test_runners_gpu import _corpus
from test_row_sampling_runner_gpu import _experiment, _decode

pytestmark = pytest.mark.gpu


def _pcm(wav):
    return np.frombuffer(wav[44:], dtype="<i2")


def test_voiced_unvoiced_flags_follow_the_uv_flag_of_every_file(cuda, tmp_path):
    root = _corpus(str(tmp_path / "corpus"))
    conf, ckpt = _experiment(str(tmp_path / "exp"))
    files = sorted(os.path.join(root, "feat", n) for n in os.listdir(root + "/feat"))
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(files) + "\n")

    def run(name, *more):
        return _decode(root, conf, ckpt, str(tmp_path / name), lst, "--per_file_seed", *more)

    base = ("--temperature", "0.8", "--top_k", "60", "--top_p", "0.95", "--min_p", "0.01")
    plain = run("plain", "--batch_size", "2", *base)
    # equal voiced and unvoiced values, given as tracks: the plain flags' wavs
    equal = run("equal", "--batch_size", "2", "--temperature_voiced", "0.8", "--temperature_unvoiced", "0.8", "--top_k_voiced", "60", "--top_k_unvoiced", "60",
                "--top_p_voiced", "0.95", "--top_p_unvoiced", "0.95", "--min_p_voiced", "0.01", "--min_p_unvoiced", "0.01")
    one_side = run("one_side", "--batch_size", "3", "--temperature_voiced", "0.8", "--top_k_unvoiced", "60", *base)      # (the unset side takes the plain flag's value)
    for name in plain:
        assert equal[name] == plain[name], "%s: equal voiced / unvoiced values differ from the plain flags" % name
        assert one_side[name] == plain[name], name
    # the unvoiced frames draw with other values: the voiced ones keep the plain flags'
    other = ("--temperature_unvoiced", "1.0", "--top_k_unvoiced", "0", "--top_p_unvoiced", "1.0", "--min_p_unvoiced", "0.0")
    uv2 = run("uv_b2", "--batch_size", "2", *base, *other)
    uv1 = run("uv_b1", "--batch_size", "1", *base, *other)
    U, flipped = TINY.upsampling_factor, 0
    for name in plain:
        assert uv1[name] == uv2[name], "%s depends on --batch_size" % name
        uv = loaders.read_features(os.path.join(root, "feat", name.replace(".wav", ".npy")), "world")[:, 0] > 0.5
        a, b = _pcm(plain[name]), _pcm(uv2[name])
        assert len(a) == len(b) == len(uv) * U - 1
        if uv.all():
            assert plain[name] == uv2[name], "%s is voiced throughout" % name
            continue
        flipped += 1
        i_star = int(np.argmin(uv)) * U                                      # seeds of one sample: frame f starts at sample f U
        np.testing.assert_array_equal(b[:i_star], a[:i_star], err_msg="%s before its first unvoiced frame" % name)
        assert not np.array_equal(b[i_star:], a[i_star:]), "%s does not change in its unvoiced frames" % name
    assert flipped >= 2, "the corpus has too few files with an unvoiced frame"
