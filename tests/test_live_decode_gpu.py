"""GPU: live decode output -- finished samples read by the host while the decode kernel runs (qpn_decode_live / qpn_decode_poll,
QPNet.generate_live).  Every kernel mirrors and publishes at its one pick site; the pieces a caller receives concatenate to
exactly what the blocking call returns."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from qpnet_amd import synth
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _collect(gen, B, m=None, ns=None, every=None):
    """Drain a generate_live generator -> per-row streams; checks what every piece must satisfy on the way.
    With the model and the call's lengths: also that EVERY piece was read from the mirror while the call was in flight (generate_live hands the
    rest of a row over from the call's output after finish when a launch ended short -- the give-up path -- and a kernel that never published
    would otherwise pass unnoticed), and, given `every` (few rows, many publishes per row: a stalled host cannot merge them all), that a row longer than it came in more than one piece."""
    rows = [[] for _ in range(B)]
    have = [0] * B
    n_pieces = 0
    for row, start, samples in gen:
        assert 0 <= row < B
        assert isinstance(samples, np.ndarray) and samples.dtype == np.int64 and samples.ndim == 1
        assert len(samples) > 0, "empty piece for row %d" % row
        assert start == have[row], "row %d: piece starts at %d, %d delivered so far" % (row, start, have[row])
        rows[row].append(samples)
        have[row] += len(samples)
        n_pieces += 1
    if m is not None:
        assert m._live_mirror_pieces == n_pieces, "%d of %d pieces came from the mirror, the others from the output after finish" % (m._live_mirror_pieces, n_pieces)
        for b in range(B):
            assert have[b] == ns[b], "row %d: %d samples delivered, %d asked for" % (b, have[b], ns[b])
            if every is not None and ns[b] > every:
                assert len(rows[b]) > 1, "row %d: %d samples in one piece with a publish every %d" % (b, ns[b], every)
    return [np.concatenate(r) if r else np.zeros(0, dtype=np.int64) for r in rows], n_pieces


def _blocking(m, xb, hb, ns, bd, mode):
    """batch_fast_generate's streams, back in input order."""
    outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode=mode)
    order = sorted(range(len(ns)), key=lambda i: ns[i])
    rows = [None] * len(ns)
    for k, b in enumerate(order):
        rows[b] = outs[k]
    return rows


def _ragged(cfg, frames, seed0):
    """Three ragged rows + a one-sample row + a zero-sample row."""
    specs = [(seed0 + b, f, [1.0, 0.5, 1.5][b % 3]) for b, f in enumerate(frames)] + [(seed0 + 7, frames[0], 1.0), (seed0 + 8, frames[0], 1.0)]
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    ns = list(ns)
    ns[3], ns[4] = 1, 0
    return bx, bh, bd, ns


KERNELS = ["pipelined", "one_cu", "interpreter", "cooperative", "batched_cooperative"]


@pytest.mark.parametrize("mode", ["argmax", "sampling"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_pieces_equal_the_blocking_call_on_every_kernel(kernel, mode, cuda, monkeypatch):
    import torch
    from qpnet_amd.config import PAPER, DEFAULT, QPNetConfig
    cfg, frames, plan = PAPER, (6, 9, 7), "pipe rows=5 "
    if kernel == "one_cu":
        monkeypatch.setenv("QPN_DECODE_PIPE", "0")
        plan = "pipe rows=0 "
    elif kernel == "interpreter":
        cfg = QPNetConfig(n_resch=96, n_skipch=256, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=1, dilationA_repeat=1)
        plan = "pipe rows=0 "
    elif kernel == "cooperative":
        monkeypatch.setenv("QPN_DECODE_COOP", "4")
        plan = "coop G="
    elif kernel == "batched_cooperative":
        monkeypatch.delenv("QPN_DECODE_COOPB", raising=False)
        cfg, frames, plan = DEFAULT, (2, 1, 3), "coopb "
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    m.sampling_seed = 77
    bx, bh, bd, ns = _ragged(cfg, frames, 40)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    ref = _blocking(m, xb, hb, ns, bd, mode)
    assert m.last_decode_plan.startswith(plan), m.last_decode_plan
    ref_plan = m.last_decode_plan
    nlist = list(ns)
    got, n_pieces = _collect(m.generate_live(xb, hb, nlist, bd, mode=mode, every=64), len(ns), m, ns, 64)
    assert nlist == list(ns), "generate_live consumed n_samples_list"
    assert m.last_decode_plan == ref_plan, (m.last_decode_plan, ref_plan)
    print("%s %s: %d pieces for rows of %s samples" % (kernel, mode, n_pieces, ns))
    for b in range(len(ns)):
        assert len(got[b]) == ns[b], "row %d: %d samples delivered, %d asked for" % (b, len(got[b]), ns[b])
        np.testing.assert_array_equal(got[b], ref[b], err_msg="row %d" % b)


@pytest.mark.parametrize("mode", ["argmax", "sampling"])
def test_pieces_equal_the_oracle(mode, cuda, oracle):
    import torch
    from qpnet_amd.config import PAPER
    cfg = PAPER
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    m.sampling_seed = 4242
    specs = [(61, 8, 1.0), (62, 5, 1.5)]
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    got, _ = _collect(m.generate_live(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), list(ns), bd, mode=mode), 2, m, ns)
    maxd = int(np.ceil(np.nanmax(bd)))
    for b in range(2):
        x, h, d, n = synth.decode_inputs(cfg, specs[b][1], specs[b][0], specs[b][2])
        r = oracle.decode(cfg, flat, h, d, x, n, maxd=maxd, mode=mode, seed=4242, row=b)
        np.testing.assert_array_equal(got[b], r["samples"], err_msg="row %d" % b)


def _abi_call(m, cuda, cfg, frames, seed):
    """One B = 1 call prepared for the C ABI -> (L, handle, enqueue arguments, out tensor, n, what must stay alive)."""
    import torch
    L, hd = m._native(cuda)
    x, h, d, n = synth.decode_inputs(cfg, frames, seed, 1.0)
    xt = torch.from_numpy(x[None]).to(cuda); ht = torch.from_numpy(h[None]).to(cuda); dt = torch.from_numpy(d[None]).to(cuda)
    out = torch.empty((1, n), dtype=torch.int64, device=cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    m._bind_decode_weights(L, hd, cuda, stream)
    arr = (C.c_int64 * 1)(n)
    maxd = int(np.ceil(d.max()))
    torch.cuda.synchronize()
    args = [hd, 1, 1, h.shape[1], d.shape[0], xt.data_ptr(), ht.data_ptr(), dt.data_ptr(), 0, arr, maxd, 0, 0, None, out.data_ptr(), None, stream]
    return L, hd, args, out, n, (xt, ht, dt, arr)


def test_first_piece_arrives_while_the_kernel_runs(cuda):
    """Through the C ABI: paper-size model, one 200-frame utterance (21 999 samples, ~0.18 s of kernel), a publish every 256 samples."""
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    L, hd, args, out, n, keep = _abi_call(m, cuda, cfg, 200, 5)
    assert n == 21999
    stream = args[-1]
    done = (C.c_int64 * 1)()
    mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()

    def poll():
        _lib.check(L.qpn_decode_poll(hd, done, C.byref(mirror), C.byref(stride), C.byref(running)))
        return int(done[0]), int(running.value)

    _lib.check(L.qpn_decode_live(hd, 256))
    t0 = time.time()
    _lib.check(L.qpn_decode_enqueue(*args))
    t_enq = time.time()
    seen = []
    deadline = t_enq + 30.0
    while True:
        d, r = poll()
        seen.append(d)
        if d > 0:
            break
        assert time.time() < deadline, "nothing published within 30 s"
        time.sleep(0.0005)
    t_first = time.time()
    first, first_running = d, r
    prefix = np.ctypeslib.as_array(mirror, shape=(1, int(stride.value)))[0, :first].copy()
    while r:
        assert time.time() < deadline, "the decode did not end within 30 s"
        time.sleep(0.0005)
        d, r = poll()
        seen.append(d)
    d, r = poll()                       # the last poll before finish
    seen.append(d)
    last = d
    _lib.check(L.qpn_decode_finish(hd, stream))
    t_end = time.time()
    _lib.check(L.qpn_decode_live(hd, 0))
    print("enqueue %.3f ms; first piece (%d samples) %.3f ms after enqueue returned; call %.1f ms; %d polls, %d distinct counts"
          % (1e3 * (t_enq - t0), first, 1e3 * (t_first - t_enq), 1e3 * (t_end - t0), len(seen), len(set(seen))))
    assert first_running == 1, "the first samples arrived only after the kernel had ended"
    assert 0 < first < n and first % 256 == 0, first
    assert all(b >= a for a, b in zip(seen, seen[1:])), "reported progress went backwards"
    assert last == n, (last, n)
    assert int(stride.value) == n
    ref = out[0].cpu().numpy()
    np.testing.assert_array_equal(np.ctypeslib.as_array(mirror, shape=(1, n))[0], ref)
    np.testing.assert_array_equal(prefix, ref[:first])


def test_rows_of_a_multi_launch_plan_publish_under_their_own_index(cuda):
    """49 rows: more than the groups of one pipelined launch hold one each, so rows share groups (stepped alternately)."""
    import torch
    from qpnet_amd.config import PAPER
    cfg = PAPER
    B = 49
    specs = [(300 + b, 6 + (b * 5) % 9, [1.0, 0.5, 1.5][b % 3]) for b in range(B)]      # (= test_decode_gpu._paper_batch(49))
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    ref = _blocking(m, xb, hb, ns, bd, "argmax")
    ref_plan = m.last_decode_plan
    got, n_pieces = _collect(m.generate_live(xb, hb, list(ns), bd, mode="argmax", every=128), B, m, ns)
    assert m.last_decode_plan == ref_plan, (m.last_decode_plan, ref_plan)
    if torch.cuda.get_device_properties(cuda).multi_processor_count == 256:
        assert "(2 per group)" in ref_plan, ref_plan
    print("%d pieces, plan %s" % (n_pieces, ref_plan))
    for b in range(B):
        assert len(got[b]) == ns[b], "row %d stopped at %d of %d" % (b, len(got[b]), ns[b])
        np.testing.assert_array_equal(got[b], ref[b], err_msg="row %d" % b)


def test_two_launches_publish_under_their_own_index(cuda, monkeypatch):
    """... and a plan of TWO pipelined launches (100 rows with at most two per group): the rows of the second launch start late and still arrive whole."""
    import torch
    from qpnet_amd.config import PAPER
    monkeypatch.setenv("QPN_PIPE_NU", "2")
    cfg = PAPER
    B = 100
    specs = [(900 + b, 5 + (b * 5) % 5, [1.0, 0.5, 1.5][b % 3]) for b in range(B)]
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    ref = _blocking(m, xb, hb, ns, bd, "argmax")
    ref_plan = m.last_decode_plan
    if torch.cuda.get_device_properties(cuda).multi_processor_count == 256:
        assert "waves=2 " in ref_plan, ref_plan
    got, _ = _collect(m.generate_live(xb, hb, list(ns), bd, mode="argmax"), B, m, ns)
    assert m.last_decode_plan == ref_plan
    for b in range(B):
        np.testing.assert_array_equal(got[b], ref[b], err_msg="row %d" % b)


def test_state_rules(cuda):
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    L, hd, args, out, n, keep = _abi_call(m, cuda, cfg, 6, 5)
    stream = args[-1]
    done = (C.c_int64 * 1)()
    mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
    pargs = (hd, done, C.byref(mirror), C.byref(stride), C.byref(running))
    # nothing in flight, not armed
    assert L.qpn_decode_poll(*pargs) == -5 and b"in flight" in L.qpn_last_error()
    # in flight, but enqueued unarmed
    _lib.check(L.qpn_decode_enqueue(*args))
    assert L.qpn_decode_poll(*pargs) == -5 and b"without live output" in L.qpn_last_error()
    assert L.qpn_decode_live(hd, 64) == -5                       # (not while a decode is in flight)
    _lib.check(L.qpn_decode_finish(hd, stream))
    plain = out[0].cpu().numpy().copy()
    plain_plan = L.qpn_last_decode_plan(hd)
    # armed, nothing in flight
    assert L.qpn_decode_live(hd, -1) == -1
    _lib.check(L.qpn_decode_live(hd, 64))
    assert L.qpn_decode_poll(*pargs) == -5 and b"in flight" in L.qpn_last_error()
    # null arguments
    assert L.qpn_decode_poll(hd, None, C.byref(mirror), C.byref(stride), C.byref(running)) == -1
    assert L.qpn_decode_poll(hd, done, None, C.byref(stride), C.byref(running)) == -1
    assert L.qpn_decode_poll(hd, done, C.byref(mirror), None, C.byref(running)) == -1
    assert L.qpn_decode_poll(hd, done, C.byref(mirror), C.byref(stride), None) == -1
    # armed + teacher forcing or the logits output
    teacher = torch.zeros((1, n), dtype=torch.int64, device=cuda)
    logits = torch.empty((1, n, cfg.n_quantize), dtype=torch.float32, device=cuda)
    a = list(args); a[13] = teacher.data_ptr()
    assert L.qpn_decode_enqueue(*a) == -1 and b"live output" in L.qpn_last_error()
    a = list(args); a[15] = logits.data_ptr()
    assert L.qpn_decode_enqueue(*a) == -1 and b"live output" in L.qpn_last_error()
    # an armed call, polled to its end
    out.zero_()
    _lib.check(L.qpn_decode_enqueue(*args))
    deadline = time.time() + 30.0
    while True:
        _lib.check(L.qpn_decode_poll(*pargs))
        if not running.value:
            break
        assert time.time() < deadline
        time.sleep(0.0005)
    _lib.check(L.qpn_decode_poll(*pargs))
    assert int(done[0]) == n
    _lib.check(L.qpn_decode_finish(hd, stream))
    assert L.qpn_decode_poll(*pargs) == -5                       # finished: nothing in flight
    np.testing.assert_array_equal(out[0].cpu().numpy(), plain)
    np.testing.assert_array_equal(np.ctypeslib.as_array(mirror, shape=(1, n))[0], plain)
    assert L.qpn_last_decode_plan(hd) == plain_plan
    # disarmed: teacher forcing is accepted again, the blocking call gives the blocking result under the same plan
    _lib.check(L.qpn_decode_live(hd, 0))
    out.zero_()
    _lib.check(L.qpn_decode_enqueue(*args))
    assert L.qpn_decode_poll(*pargs) == -5
    _lib.check(L.qpn_decode_finish(hd, stream))
    np.testing.assert_array_equal(out[0].cpu().numpy(), plain)
    assert L.qpn_last_decode_plan(hd) == plain_plan
    a = list(args); a[13] = teacher.data_ptr()
    _lib.check(L.qpn_decode(*a))


def test_blocking_call_after_a_live_one(cuda):
    import torch
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, [(71, 7, 1.0), (72, 5, 0.5)])
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    before = _blocking(m, xb, hb, ns, bd, "argmax")
    plan = m.last_decode_plan
    got, _ = _collect(m.generate_live(xb, hb, list(ns), bd, mode="argmax"), 2, m, ns)
    after = _blocking(m, xb, hb, ns, bd, "argmax")
    assert m.last_decode_plan == plan
    for b in range(2):
        np.testing.assert_array_equal(before[b], after[b])
        np.testing.assert_array_equal(before[b], got[b])
    # teacher forcing on the same module: live output was disarmed when the generator ended
    x, h, d, n = synth.decode_inputs(cfg, 3, 5, 1.0)
    teacher = np.random.RandomState(9).randint(0, 256, size=n).astype(np.int64)
    m._stream_logits(torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), d[None], torch.from_numpy(teacher[None]), n)


def test_abandoned_generator_leaves_the_model_usable(cuda):
    import torch
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, [(81, 40, 1.0), (82, 30, 1.5)])
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    ref = _blocking(m, xb, hb, ns, bd, "argmax")
    gen = m.generate_live(xb, hb, list(ns), bd, mode="argmax", every=64)
    row, start, samples = next(gen)
    assert start == 0 and 0 < len(samples) < ns[row]
    np.testing.assert_array_equal(samples, ref[row][:len(samples)])
    gen.close()
    again = _blocking(m, xb, hb, ns, bd, "argmax")
    for b in range(2):
        np.testing.assert_array_equal(again[b], ref[b])
    # ... and one that is dropped without close()
    gen = m.generate_live(xb, hb, list(ns), bd, mode="argmax", every=64)
    next(gen)
    del gen
    again = _blocking(m, xb, hb, ns, bd, "argmax")
    for b in range(2):
        np.testing.assert_array_equal(again[b], ref[b])


def test_range_error_is_raised_like_the_blocking_call(cuda):
    """A dilated factor that leaves the rings: batch_fast_generate raises QPN_ERANGE from finish; generate_live does so after its last piece."""
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    x, h, d, n = synth.decode_inputs(cfg, 6, 5, 1.0)
    d = d.copy(); d[n // 2:] = 0.2        # rounds to a tap distance of 0 -> out of contract
    xt, ht = torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda)
    with pytest.raises(_lib.QpnError) as e1:
        m.batch_fast_generate(xt, ht, [n], d[None], mode="argmax")
    assert e1.value.code == -4
    with pytest.raises(_lib.QpnError) as e2:
        for _ in m.generate_live(xt, ht, [n], d[None], mode="argmax"):
            pass
    assert e2.value.code == -4
    y = m.batch_fast_generate(xt, ht, [n], np.ones_like(d)[None], mode="argmax")      # the handle is usable again
    assert len(y[0]) == n


def test_progress_lines_are_written_while_the_kernel_runs(cuda, caplog):
    import logging
    import torch
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    x, h, d, n = synth.decode_inputs(cfg, 30, 5, 1.0)
    with caplog.at_level(logging.INFO):
        pieces = list(m.generate_live(torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), [n], d[None], intervals=1000, mode="argmax", every=64))
    lines = [r.getMessage() for r in caplog.records if "estimated time" in r.getMessage()]
    assert [int(s.split("/")[0]) for s in lines] == list(range(1000, n + 1, 1000)), lines
    assert all(s.split("/")[1].startswith("%d " % n) for s in lines)
    assert len(pieces) > 1


def test_launch_that_gives_up_still_delivers_every_sample(cuda):
    """The pipelined launch gives up at once (the hook of the -DQPN_TESTING build); qpn_decode_finish re-runs the call on the one-CU kernels.
    tests/live_giveup_child.py, in a child process bound to that build."""
    lib = os.path.join(ROOT, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0", QPN_TEST_PIPE_GIVES_UP="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "live_giveup_child.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "LIVE_GIVEUP_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
