"""The corpora and generator settings the device-corpus tests share (tests/test_device_corpus_cpu.py, tests/test_device_corpus_gpu.py): small enough that a
case takes well under a second, shaped so that every path of the chunk walk is taken.  Receptive fields are the TINY configuration's."""
import numpy as np

from qpnet_amd import loaders, synth
from qpnet_amd.config import TINY

FS, DENSE = 22050, 8
FIELDS = (TINY.receptiveCausal_field, TINY.receptiveF_field, TINY.receptiveA_field)
# (U, n_aux) -> (batch_length, max_length): a chunk of a few frames at U = 110, of about twenty at U = 5 (rf = 4 + ceil(max d) is 14 .. 39 samples here)
GEOMETRIES = {(5, 3): (60, 400), (110, 39): (600, 3000)}


def utterance(frames, U, n_aux, seed, f0=None):
    """(x, h): a random waveform in [-1, 1) of frames * U samples (+ a few the length validation trims) and WORLD-like features; f0: a constant pitch"""
    rs = np.random.RandomState(1000 + seed)
    lo, hi = (80.0, 300.0) if f0 is None else (float(f0), float(f0))
    return rs.uniform(-1, 1, frames * U + seed % 3).astype(np.float32) * np.float32(0.999), synth.make_features(frames, seed, lo, hi, n_aux=n_aux)


def scaler(n_aux, seed=5):
    """a feature scaler as calc_stats makes it: the uv column keeps mean 0 / scale 1"""
    rs = np.random.RandomState(seed)
    mean, scale = rs.standard_normal(n_aux), 0.5 + rs.rand(n_aux)
    mean[0], scale[0] = 0.0, 1.0
    return loaders.FeatureScaler(mean, scale)


def cases(U, n_aux):
    """name -> (utterances, generator keywords); every case runs to the end of its epochs"""
    frames_per_chunk = (39 + GEOMETRIES[(U, n_aux)][0]) // U + 1          # an upper bound
    long_one = [utterance(4 * frames_per_chunk + 3, U, n_aux, 1)]
    short = [utterance(1 + k % 3, U, n_aux, 10 + k) for k in range(12)] * 3   # 1..3 frames each; three passes so that several chunks are cut
    steady = [utterance(frames_per_chunk + 2 + k, U, n_aux, 30 + k, f0=150.0) for k in range(5)]
    mixed = [utterance(frames_per_chunk // 2 + 3 * k, U, n_aux, 40 + k) for k in range(7)]
    jump = [utterance(3 * frames_per_chunk, U, n_aux, 50, f0=300.0), utterance(3 * frames_per_chunk, U, n_aux, 51, f0=80.0),
            utterance(2 * frames_per_chunk, U, n_aux, 52, f0=300.0)]
    one = dict(batch_size=1, shuffle=False, epochs=1, shard=None)
    return {
        "a_one_long_utterance": (long_one, one),
        "b_short_utterances": (short, one),
        "c_batch_of_two": (steady, dict(one, batch_size=2)),
        "d_shard_0_of_2": (mixed, dict(one, shard=(0, 2))),
        "d_shard_1_of_2": (mixed, dict(one, shard=(1, 2))),
        "d_unsharded": (mixed, one),
        "e_shuffle_two_epochs": (mixed, dict(one, shuffle=True, epochs=2)),
        "f_pitch_jump": (jump, one),
    }


def host_batches(utts, U, n_aux, kw, unvoiced_weight=0.25, batch_length=None, max_length=None, seed=7):
    """train_generator's batches as runners._batches completes them: [(x, h, t, d, bb, maxd, w)] (CPU tensors, bb a list, w from unvoiced_row_weights)"""
    import torch
    bl, ml = GEOMETRIES.get((U, n_aux), (None, None))                 # (a geometry outside the table is given in full by batch_length / max_length)
    np.random.seed(seed)
    out = []
    for bx, bh, bt, bd, bb in loaders.train_generator(utts, *FIELDS, FS, wav_transform=loaders.mu_law_transform(256), feat_transform=scaler(n_aux), dense_factor=DENSE,
                                                      batch_length=batch_length or bl, max_length=max_length or ml, f0_threshold=0, upsampling_factor=U, **kw):
        w = torch.from_numpy(loaders.unvoiced_row_weights(bh.numpy(), int(bb[0]), U, unvoiced_weight))
        out.append((bx, bh, bt, bd, bb.tolist(), int(np.ceil(float(bd.max()))), w))
    return out


def corpus(utts, U, n_aux, device=None, max_bytes=None):
    return loaders.DeviceCorpus(utts, U, FS, DENSE, 0, loaders.mu_law_transform(256), scaler(n_aux), device, max_bytes)


def plan_kwargs(U, n_aux, kw, batch_length=None, max_length=None):
    bl, ml = GEOMETRIES.get((U, n_aux), (None, None))
    return dict(batch_length=batch_length or bl, max_length=max_length or ml, **kw)
