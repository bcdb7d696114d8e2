"""CPU: the device-resident corpus without a device -- loaders.plan_device_batches walks train_generator's stream, and its segments, applied with numpy to
host copies of the arenas, give train_generator's batches bit for bit; whole-utterance transforms equal per-slice transforms; the refusals."""
import numpy as np
import pytest

from qpnet_amd import loaders

import device_corpus_spec as S

UW = 0.25


def cut_host(c, rows, frames, bl, uw):
    """what qpn_cut_chunks computes, in numpy, from host copies of the arenas"""
    smp, fts, fac, U = c.samples.numpy(), c.feats.numpy(), c.factors.numpy(), c.U
    x, h, d = [], [], []
    for r in rows:
        x.append(np.concatenate([smp[s0:s0 + ns] for s0, ns, f0, nf, fd0 in r]).astype(np.int64))
        h.append(np.concatenate([fts[f0:f0 + nf] for s0, ns, f0, nf, fd0 in r]).T)
        d.append(np.concatenate([np.repeat(fac[fd0:fd0 + -(-ns // U)], U)[:ns] for s0, ns, f0, nf, fd0 in r])[:-1])
    x, h, d = np.stack(x), np.stack(h), np.stack(d)
    pos = np.arange(frames * U - bl, frames * U) // U
    return x[:, :-1], h, x[:, 1:], d, np.where(h[:, 0, :][:, pos] > 0.5, np.float32(1), np.float32(uw)).astype(np.float32)


def planned(utts, U, n_aux, kw, seed=7, **geom):
    c = S.corpus(utts, U, n_aux)
    np.random.seed(seed)
    out = []
    for rows, frames, bl, mine, maxd in loaders.plan_device_batches(c, *S.FIELDS, **S.plan_kwargs(U, n_aux, kw, **geom)):
        if mine:
            recs, first = loaders.corpus_segment_table(rows, frames, U)
            assert first[0] == 0 and first[-1] == len(recs) and len(first) == len(rows) + 1
            out.append(cut_host(c, rows, frames, bl, UW)[:4] + ([bl] * len(rows), maxd) + cut_host(c, rows, frames, bl, UW)[4:])
    return out


def same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for got, want in zip(a, b):
        for k in (0, 1, 2, 3, 6):
            w = want[k].numpy()
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), "element %d differs" % k
        assert got[4] == want[4] and got[5] == want[5]


@pytest.mark.parametrize("U,n_aux", sorted(S.GEOMETRIES))
@pytest.mark.parametrize("case", sorted(S.cases(5, 3)))
def test_planner_walks_the_generators_stream(case, U, n_aux):
    utts, kw = S.cases(U, n_aux)[case]
    want = S.host_batches(utts, U, n_aux, kw, UW)
    assert len(want) >= (2 if case.startswith("d_shard") else 3)
    same(planned(utts, U, n_aux, kw), want)


@pytest.mark.parametrize("U,n_aux", sorted(S.GEOMETRIES))
def test_cases_take_the_paths_they_are_named_for(U, n_aux):
    cs = S.cases(U, n_aux)
    c = S.corpus(cs["b_short_utterances"][0], U, n_aux)
    np.random.seed(7)
    plans = list(loaders.plan_device_batches(c, *S.FIELDS, **S.plan_kwargs(U, n_aux, cs["b_short_utterances"][1])))
    assert max(len(r) for p in plans for r in p[0]) >= 3                       # a chunk spans several utterances
    assert any(r[-1][1] == 1 and r[-1][3] == 0 for p in plans for r in p[0])   # the +1 sample falls into the next utterance: samples, no feature row
    c = S.corpus(cs["f_pitch_jump"][0], U, n_aux)
    plans = list(loaders.plan_device_batches(c, *S.FIELDS, **S.plan_kwargs(U, n_aux, cs["f_pitch_jump"][1])))
    assert len({(p[1], p[2]) for p in plans}) >= 2                             # the receptive field changed between two chunks
    assert len({p[4] for p in plans}) >= 2
    whole = S.host_batches(cs["d_unsharded"][0], U, n_aux, cs["d_unsharded"][1], UW)
    parts = [planned(cs[k][0], U, n_aux, cs[k][1]) for k in ("d_shard_0_of_2", "d_shard_1_of_2")]
    union = [parts[i % 2][i // 2] for i in range(len(parts[0]) + len(parts[1]))]
    same(union, whole)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_whole_utterance_transform_then_slice_is_slice_then_transform(dtype):
    U, n_aux = 110, 39
    x, h = S.utterance(40, U, n_aux, 3)
    h = h.astype(dtype)
    wav_t, feat_t = loaders.mu_law_transform(256), S.scaler(n_aux)
    c = loaders.DeviceCorpus([(x, h)], U, S.FS, S.DENSE, 0, wav_t, feat_t, None)
    import torch
    rs = np.random.RandomState(0)
    for _ in range(20):
        f0 = int(rs.randint(0, 39)); f1 = int(rs.randint(f0 + 1, 41))
        xs = torch.from_numpy(np.asarray(wav_t(np.asarray(x[f0 * U:f1 * U], dtype=np.float32)))).long().numpy()
        hs = torch.from_numpy(np.asarray(feat_t(h[f0:f1].astype(np.result_type(np.float32, dtype), copy=False)))).float().numpy()
        assert np.array_equal(c.samples.numpy()[f0 * U:f1 * U].astype(np.int64), xs)
        assert np.array_equal(c.feats.numpy()[f0:f1], hs)
    assert c.samples.dtype == torch.int16 and c.feats.dtype == torch.float32 and c.factors.dtype == torch.float32
    assert (c.n_utterances, c.n_frames, c.nbytes) == (1, 40, 2 * 40 * U + 4 * 40 * (n_aux + 1))


def test_refusals():
    U, n_aux = 5, 3
    x, h = S.utterance(30, U, n_aux, 1)
    with pytest.raises(ValueError, match="upsampling_factor"):
        loaders.DeviceCorpus([(x, h)], 0, S.FS, S.DENSE, 0, None, None, None)
    with pytest.raises(ValueError, match="40000"):
        loaders.DeviceCorpus([(x, h)], U, S.FS, S.DENSE, 0, lambda v: np.full(len(v), 40000, dtype=np.int64), None, None)
    with pytest.raises(ValueError, match="-1"):
        loaders.DeviceCorpus([(x, h)], U, S.FS, S.DENSE, 0, lambda v: np.full(len(v), -1, dtype=np.int64), None, None)
    calls = []

    def lazy(k):
        def load():
            calls.append(k)
            return S.utterance(30, U, n_aux, k)
        return load
    with pytest.raises(ValueError, match=r"max_bytes = 100\b") as e:
        S.corpus([lazy(0), lazy(1), lazy(2)], U, n_aux, max_bytes=100)
    assert calls == [0] and str(2 * 30 * U + 4 * 30 * (n_aux + 1)) in str(e.value)      # both numbers; no second utterance was loaded
    # rows of unequal length, batch_size = 2: refused when the table is made, before anything could be launched
    c = S.corpus([(x, h)], U, n_aux)
    np.random.seed(7)
    rows, frames, bl, mine, maxd = next(loaders.plan_device_batches(c, *S.FIELDS, batch_length=20, max_length=400, batch_size=2, shuffle=False, epochs=1))
    loaders.corpus_segment_table(rows, frames, U)
    s0, ns, f0, nf, fd0 = rows[1][-1]
    with pytest.raises(ValueError, match="equal length: row 1"):
        loaders.corpus_segment_table([rows[0], rows[1][:-1] + [(s0, ns + U, f0, nf + 1, fd0)]], frames, U)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(loaders.device_train_generator(c, *S.FIELDS, 20, 2, 400, False, 1, None))


def test_corpus_keeps_no_handle_on_its_sources():
    """an utterance is loaded exactly once, in list order, and the corpus keeps what the plan needs only"""
    U, n_aux = 5, 3
    calls = []

    def lazy(k):
        def load():
            calls.append(k)
            return S.utterance(8 + k, U, n_aux, k)
        return load
    c = S.corpus([lazy(k) for k in range(4)], U, n_aux)
    np.random.seed(1)
    list(loaders.plan_device_batches(c, *S.FIELDS, batch_length=20, max_length=400, shuffle=True, epochs=3))
    assert calls == [0, 1, 2, 3]
    assert [m[0] for m in c.meta] == [8, 9, 10, 11] and [m[1] for m in c.meta] == [0, 40, 85, 135] and [m[2] for m in c.meta] == [0, 8, 17, 27]
    assert all(m[3].dtype == np.float64 and m[4].dtype == np.float64 for m in c.meta)
