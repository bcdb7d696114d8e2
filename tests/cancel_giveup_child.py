"""Child process of test_decode_cancel_gpu.test_give_up_then_cancel: runs with QPN_LIB = the -DQPN_TESTING build (qpnet_amd/libqpnet_hip_testing.so)
and QPN_TEST_PIPE_GIVES_UP=1, the hook of tests/giveup_child.py `pipe`: the pipelined launch behaves as if a wait had timed out at once and drains.
The host then requests a stop before it calls finish.  A call with a request is over: qpn_decode_finish neither re-runs it on the one-CU kernels nor
reports QPN_ENODEV, every count is 0, and the next blocking call (which gives up and is re-run, as always under this hook) is correct.
    python tests/cancel_giveup_child.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(cuda):
    import torch
    import util
    from cancel_common import LiveCall
    from oracle import cpu_oracle as oracle
    from qpnet_amd import _lib, synth
    from qpnet_amd.config import PAPER
    cfg = PAPER
    B = 3
    specs = [(300 + b, 6 + (b * 5) % 9, [1.0, 0.5, 1.5][b % 3]) for b in range(B)]
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    maxd = int(np.ceil(np.nanmax(bd)))
    call = LiveCall(m, xb, hb, ns, bd, "argmax")
    L, hd = call.L, call.hd
    _lib.check(L.qpn_decode_live(hd, 64))
    call.enqueue()
    assert call.plan().startswith("pipe rows=%d " % B), call.plan()
    deadline = time.time() + 30.0
    while call.poll()[1]:                       # the launch gives up at once
        assert time.time() < deadline, "the launch that gives up did not end within 30 s"
        time.sleep(0.0005)
    assert call.poll()[0] == [0] * B
    assert call.cancel() == 0, L.qpn_last_error()
    rc = call.finish()
    assert rc == 0, (rc, L.qpn_last_error())
    assert "retried" not in call.plan(), call.plan()
    rc, counts, cancelled = call.final_counts()
    assert (rc, counts, cancelled) == (0, [0] * B, 1), (rc, counts, cancelled)
    _lib.check(L.qpn_decode_live(hd, 0))
    # the handle is as usable as after any other call
    outs = m.batch_fast_generate(xb, hb, list(ns), bd, mode="argmax")
    assert "timed out, retried" in m.last_decode_plan, m.last_decode_plan
    order = sorted(range(B), key=lambda i: ns[i])
    for k, b in enumerate(order):
        x, h, d, n = synth.decode_inputs(cfg, specs[b][1], specs[b][0], specs[b][2])
        r = oracle.decode(cfg, flat, h, d, x, n, maxd=maxd, mode="argmax", seed=0, row=b)
        np.testing.assert_array_equal(outs[k], r["samples"], err_msg="row %d" % b)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    from qpnet_amd import _lib
    assert _lib.LIB_PATH.endswith("libqpnet_hip_testing.so"), _lib.LIB_PATH
    assert os.environ.get("QPN_TEST_PIPE_GIVES_UP")
    main(torch.device("cuda:0"))
    print("CANCEL_GIVEUP_CHILD_OK")
