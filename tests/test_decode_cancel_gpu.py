"""GPU: cancel a running decode (qpn_decode_cancel / qpn_decode_final_counts, QPNet.generate_live(on_close="cancel")).  A live call stops at
one of its next publish points: every row's published count is final, the samples below it are bit for bit those of the uncancelled call, finish
returns without re-running anything, and nothing of the request carries into the next call.  No test asserts a time: the counts are bounded."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from qpnet_amd import synth
import util
from cancel_common import LiveCall, stop_after_first_count

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocking(m, xb, hb, ns, bd, mode):
    """batch_fast_generate's streams, back in input order."""
    outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode=mode)
    order = sorted(range(len(ns)), key=lambda i: ns[i])
    rows = [None] * len(ns)
    for k, b in enumerate(order):
        rows[b] = outs[k]
    return rows


@pytest.mark.parametrize("mode", ["argmax", "sampling"])
def test_cancel_through_the_c_abi(mode, cuda):
    """Paper-size model, one 400-frame utterance (43 999 samples, ~0.37 s uncancelled), a publish every 256 samples.
    The bound on the final count: at most one check is deferred, so the row stops within two intervals of c1 (the count polled right after
    the request); two more allow for a host view that lags by microseconds against a 2 ms interval.  A call that ran on is 170 intervals away."""
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    m.sampling_seed = 4242
    x, h, d, n = synth.decode_inputs(cfg, 400, 5, 1.0)
    assert n == 43999
    xb, hb = torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda)
    call = LiveCall(m, xb, hb, [n], d[None], mode)
    L, hd = call.L, call.hd
    _lib.check(L.qpn_decode_live(hd, 256))
    call.enqueue()
    c0, c1, last = stop_after_first_count(call)
    t0 = time.time()
    rc = call.finish()
    assert rc == 0, (rc, L.qpn_last_error())
    assert "retried" not in call.plan(), call.plan()
    rc, counts, cancelled = call.final_counts()
    assert rc == 0, (rc, L.qpn_last_error())
    final, c1 = counts[0], c1[0]
    print("%s: count at the request %d, right after it %d, final %d of %d; finish took %.3f ms; plan %s" % (mode, c0[0], c1, final, n, 1e3 * (time.time() - t0), call.plan()))
    assert cancelled == 1
    assert c1 <= final < n, (c1, final, n)
    assert final == last[0], (final, last)
    assert final % 256 == 0, final
    assert final <= c1 + 4 * 256, (c1, final)
    got_out = call.out[0, :final].cpu().numpy()
    got_mirror = call.mirror_rows()[0, :final]
    # the prefix: a blocking call of the same inputs for `final` samples (greedy decode and the counter-based sampler are prefix-stable)
    _lib.check(L.qpn_decode_live(hd, 0))
    ref_call = LiveCall(m, xb, hb, [final], d[None], mode)
    _lib.check(L.qpn_decode(*ref_call.a["call"]))
    ref = ref_call.out[0, :final].cpu().numpy()
    np.testing.assert_array_equal(got_out, ref)
    np.testing.assert_array_equal(got_mirror, ref)


KERNELS = ["pipelined", "one_cu", "interpreter", "cooperative", "batched_cooperative"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_cancel_on_every_kernel(kernel, cuda, monkeypatch):
    """generate_live(on_close="cancel") closed after every long row's first piece; then a blocking call and an armed call that runs to its end."""
    import torch
    from qpnet_amd.config import PAPER, DEFAULT, QPNetConfig
    cfg, frames, plan = PAPER, (400, 300), "pipe rows=4 "
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
        cfg, frames, plan = DEFAULT, (40, 30), "coopb "      # (a step is ten times longer there)
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    # the later blocking call and its reference, from before the cancelled call
    sx, sh, sd, sns = synth.decode_batch(cfg, [(71, 6, 1.0), (72, 6, 0.5)])
    sxb, shb = torch.from_numpy(sx).to(cuda), torch.from_numpy(sh).to(cuda)
    small_ref = _blocking(m, sxb, shb, sns, sd, "argmax")
    # two ragged long rows + a one-sample row + a zero-sample row
    bx, bh, bd, ns = synth.decode_batch(cfg, [(40, frames[0], 1.0), (41, frames[1], 0.5), (47, 3, 1.0), (48, 3, 1.0)])
    ns = list(ns)
    ns[2], ns[3] = 1, 0
    long_rows = (0, 1)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    gen = m.generate_live(xb, hb, list(ns), bd, mode="argmax", every=64, on_close="cancel")
    got = [[] for _ in ns]
    have = [0] * len(ns)
    for row, start, samples in gen:
        assert start == have[row] and len(samples) > 0
        got[row].append(samples)
        have[row] += len(samples)
        if all(have[b] > 0 for b in long_rows):
            break
    assert m.last_decode_plan.startswith(plan), m.last_decode_plan
    # (a precondition of the test, not a property of the product: the request needs rows that are still running to land in)
    assert all(have[b] < ns[b] // 2 for b in long_rows), "row too short for this machine: %s of %s delivered before the request" % (have, ns)
    gen.close()
    counts = m.last_decode_counts
    print("%s: delivered %s, final counts %s of %s, plan %s" % (kernel, have, counts, ns, m.last_decode_plan))
    assert m.last_decode_cancelled is True
    assert "retried" not in m.last_decode_plan, m.last_decode_plan
    for b in long_rows:
        assert counts[b] % 64 == 0 and have[b] <= counts[b] < ns[b], (b, have, counts, ns)
    assert counts[2:] == [1, 0], counts
    # the delivered pieces = the prefix of a blocking call cut to the counts (greedy decode is prefix-stable)
    ref = _blocking(m, xb, hb, counts, bd, "argmax")
    for b in range(len(ns)):
        assert len(ref[b]) == counts[b]
        if have[b]:
            np.testing.assert_array_equal(np.concatenate(got[b]), ref[b][:have[b]], err_msg="row %d" % b)
    # nothing of the request, the abort word or the rings leaks into the next call
    after = _blocking(m, sxb, shb, sns, sd, "argmax")
    for b in range(2):
        np.testing.assert_array_equal(after[b], small_ref[b], err_msg="row %d of the call after the cancelled one" % b)
    # ... and an armed call that is iterated to its end never cancels
    rows = [[] for _ in sns]
    for row, start, samples in m.generate_live(sxb, shb, list(sns), sd, mode="argmax", every=64, on_close="cancel"):
        rows[row].append(samples)
    assert m.last_decode_counts == list(sns) and m.last_decode_cancelled is False, (m.last_decode_counts, m.last_decode_cancelled)
    for b in range(2):
        np.testing.assert_array_equal(np.concatenate(rows[b]), small_ref[b], err_msg="row %d of the armed call after the cancelled one" % b)


def test_cancel_reaches_the_second_launch(cuda, monkeypatch):
    """A plan of TWO pipelined launches (100 rows with at most two per group, longest first): the 300-frame rows are in the first launch, the
    200-frame rows in the second, which starts after the request and publishes nothing."""
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    monkeypatch.setenv("QPN_PIPE_NU", "2")
    cfg = PAPER
    B = 100
    specs = [(900 + b, 300 if b < 50 else 200, [1.0, 0.5, 1.5][b % 3]) for b in range(B)]
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    call = LiveCall(m, xb, hb, ns, bd, "argmax")
    L, hd = call.L, call.hd
    _lib.check(L.qpn_decode_live(hd, 64))
    call.enqueue()
    first_plan = call.plan()
    two_launches = torch.cuda.get_device_properties(cuda).multi_processor_count == 256 and "waves=2 " in first_plan
    if not two_launches:                        # (this case is about the second launch: nothing to request)
        call.finish()
        L.qpn_decode_live(hd, 0)
        pytest.skip("the plan is not two launches on this device: %s" % first_plan)
    c0, c1, last = stop_after_first_count(call)
    rc = call.finish()                          # returns: the test would hang here otherwise
    assert rc == 0, (rc, L.qpn_last_error())
    assert call.plan() == first_plan and "retried" not in call.plan(), call.plan()
    rc, counts, cancelled = call.final_counts()
    assert rc == 0 and cancelled == 1
    print("plan %s; final counts of the first launch %d .. %d, of the second %d .. %d" % (first_plan, min(counts[:50]), max(counts[:50]), min(counts[50:]), max(counts[50:])))
    assert counts[50:] == [0] * 50, counts[50:]
    assert all(c % 64 == 0 and l <= c < n for c, l, n in zip(counts[:50], last[:50], ns[:50])), (counts[:50], last[:50])
    assert max(counts[:50]) > 0
    got_out, got_mirror = call.out.cpu().numpy(), call.mirror_rows()
    _lib.check(L.qpn_decode_live(hd, 0))
    ref = _blocking(m, xb, hb, counts, bd, "argmax")
    for b in range(50):
        np.testing.assert_array_equal(got_out[b, :counts[b]], ref[b], err_msg="row %d" % b)
        np.testing.assert_array_equal(got_mirror[b, :counts[b]], ref[b], err_msg="row %d (mirror)" % b)


def test_state_rules(cuda):
    import torch
    from qpnet_amd import _lib
    from qpnet_amd.config import PAPER
    cfg = PAPER
    m = util.build_model(cfg, synth.make_weights(cfg, 13), cuda)
    x, h, d, n = synth.decode_inputs(cfg, 6, 5, 1.0)
    call = LiveCall(m, torch.from_numpy(x[None]).to(cuda), torch.from_numpy(h[None]).to(cuda), [n], d[None], "argmax")
    L, hd = call.L, call.hd
    cancelled = C.c_int()
    # nothing in flight
    assert call.cancel() == -5 and b"in flight" in L.qpn_last_error()
    # an unarmed call in flight: no publish points to stop at; the call finishes with the blocking result
    call.enqueue()
    assert call.cancel() == -5 and b"without live output" in L.qpn_last_error()
    assert call.final_counts()[0] == -5 and b"in flight" in L.qpn_last_error()
    assert call.finish() == 0
    plain = call.out[0].cpu().numpy().copy()
    assert call.final_counts()[0] == -5 and b"live output" in L.qpn_last_error()          # the last call was not armed
    call.out.zero_()
    _lib.check(L.qpn_decode(*call.a["call"]))
    np.testing.assert_array_equal(plain, call.out[0].cpu().numpy())
    # null arguments
    assert L.qpn_decode_final_counts(hd, None, C.byref(cancelled)) == -1
    assert L.qpn_decode_final_counts(hd, call.done, None) == -1
    assert L.qpn_decode_cancel(None) == -1 and L.qpn_decode_final_counts(None, call.done, C.byref(cancelled)) == -1
    # an armed call: final_counts refuses while it is in flight; a request after the kernels have ended changes nothing
    _lib.check(L.qpn_decode_live(hd, 64))
    call.enqueue()
    assert call.final_counts()[0] == -5 and b"in flight" in L.qpn_last_error()
    deadline = time.time() + 30.0
    while call.poll()[1]:
        assert time.time() < deadline
        time.sleep(0.0005)
    assert call.cancel() == 0
    assert call.finish() == 0
    assert call.final_counts() == (0, [n], 0)
    np.testing.assert_array_equal(call.out[0].cpu().numpy(), plain)
    assert call.cancel() == -5                                                          # finished: nothing in flight
    # two requests in a row (a longer call, so that they land in it)
    _lib.check(L.qpn_decode_live(hd, 0))
    x2, h2, d2, n2 = synth.decode_inputs(cfg, 200, 5, 1.0)
    long_call = LiveCall(m, torch.from_numpy(x2[None]).to(cuda), torch.from_numpy(h2[None]).to(cuda), [n2], d2[None], "argmax")
    _lib.check(L.qpn_decode_live(hd, 64))
    long_call.enqueue()
    assert long_call.cancel() == 0 and long_call.cancel() == 0
    assert long_call.finish() == 0, L.qpn_last_error()
    rc, counts, was_cancelled = long_call.final_counts()
    assert rc == 0 and was_cancelled == 1 and counts[0] % 64 == 0 and counts[0] < n2, (rc, counts, was_cancelled)
    assert "retried" not in long_call.plan()
    # the next armed call starts from a cleared request
    call.enqueue()
    assert call.finish() == 0
    assert call.final_counts() == (0, [n], 0)
    np.testing.assert_array_equal(call.out[0].cpu().numpy(), plain)
    _lib.check(L.qpn_decode_live(hd, 0))


def test_give_up_then_cancel(cuda):
    """The pipelined launch gives up at once (the hook of the -DQPN_TESTING build) and the host cancels before finish: no re-run, no QPN_ENODEV.
    tests/cancel_giveup_child.py, in a child process bound to that build."""
    lib = os.path.join(ROOT, "qpnet_amd", "libqpnet_hip_testing.so")
    assert os.path.exists(lib), "build the testing library first: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, QPN_LIB=lib, HSA_ENABLE_IPC_MODE_LEGACY="0", QPN_TEST_PIPE_GIVES_UP="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cancel_giveup_child.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "CANCEL_GIVEUP_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
