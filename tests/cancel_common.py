"""Shared by tests/test_decode_cancel_gpu.py and tests/cancel_giveup_child.py: one decode call prepared for the C ABI, and the sequence every
cancelling case goes through (wait for the first count, check that the request has time to land, request the stop, drain the polls)."""
import ctypes as C
import time

import numpy as np

from qpnet_amd import _lib


class LiveCall:
    """One decode call through the C ABI (enqueue / poll / cancel / finish / final_counts on the model's handle), with its poll buffers.
    The arguments are what QPNet.batch_fast_generate would pass for the same inputs (QPNet._decode_args: weights bound, seed = m.sampling_seed)."""

    def __init__(self, m, xb, hb, ns, bd, mode="argmax"):
        import torch
        self.a = m._decode_args(xb, hb, list(ns), bd, mode, False)
        self.L, self.hd, self.B, self.ns, self.out, self.stream = (self.a[k] for k in ("L", "hd", "B", "ns", "out", "stream"))
        self.done = (C.c_int64 * self.B)()
        self.mirror, self.stride, self.running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
        torch.cuda.synchronize()

    def enqueue(self):
        self.out.zero_()
        _lib.check(self.L.qpn_decode_enqueue(*self.a["call"]))

    def poll(self):
        _lib.check(self.L.qpn_decode_poll(self.hd, self.done, C.byref(self.mirror), C.byref(self.stride), C.byref(self.running)))
        return [int(v) for v in self.done], int(self.running.value)

    def cancel(self):
        return self.L.qpn_decode_cancel(self.hd)

    def finish(self):
        return self.L.qpn_decode_finish(self.hd, self.stream)

    def final_counts(self):
        cancelled = C.c_int(-1)
        rc = self.L.qpn_decode_final_counts(self.hd, self.done, C.byref(cancelled))
        return rc, [int(v) for v in self.done], int(cancelled.value)

    def mirror_rows(self):
        """The mirror as the last poll returned it (host memory of the handle, valid until the next enqueue): a copy, (B, stride) int64."""
        return np.ctypeslib.as_array(self.mirror, shape=(self.B, max(int(self.stride.value), 1))).astype(np.int64)

    def plan(self):
        return self.L.qpn_last_decode_plan(self.hd).decode("utf-8", "replace")


def stop_after_first_count(call):
    """Poll until the first count appears, request the stop, poll once more, drain the polls.  -> (counts at the request, c1 = the counts of the
    poll right after the request, the last counts polled).  The caller calls finish."""
    longest = max(range(call.B), key=lambda b: call.ns[b])
    deadline = time.time() + 30.0
    while True:
        c0, running = call.poll()
        if max(c0) > 0:
            break
        assert time.time() < deadline, "nothing published within 30 s"
        time.sleep(0.0002)
    # (a precondition of the test, not a property of the product: the request needs a call that is still running to land in)
    assert running == 1 and c0[longest] < call.ns[longest] // 2, "row too short for this machine: %d of %d samples at the first count, running = %d" % (c0[longest], call.ns[longest], running)
    assert call.cancel() == 0, call.L.qpn_last_error()
    c1, running = call.poll()
    last = c1
    while running:
        assert time.time() < deadline, "the decode did not stop within 30 s"
        time.sleep(0.0002)
        d, running = call.poll()
        assert all(a >= b for a, b in zip(d, last)), "reported progress went backwards"
        last = d
    d, _ = call.poll()
    assert all(a >= b for a, b in zip(d, last)), "reported progress went backwards"
    return c0, c1, d
