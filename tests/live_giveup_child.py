"""Child process of test_live_decode_gpu.test_launch_that_gives_up_still_delivers_every_sample: runs with QPN_LIB = the -DQPN_TESTING build
(qpnet_amd/libqpnet_hip_testing.so) and QPN_TEST_PIPE_GIVES_UP=1, the hook of tests/giveup_child.py `pipe`: the pipelined launch behaves as if a
wait had timed out at once, drains, and qpn_decode_finish re-runs the call on the one-CU kernels.  A live call must not notice more than that:
the pieces are contiguous (progress never goes backwards) and concatenate to the oracle's streams.
    python tests/live_giveup_child.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(cuda):
    import torch
    import util
    from oracle import cpu_oracle as oracle
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER
    cfg = PAPER
    B = 5
    specs = [(300 + b, 6 + (b * 5) % 9, [1.0, 0.5, 1.5][b % 3]) for b in range(B)]      # (= test_decode_gpu._paper_batch(5))
    flat = synth.make_weights(cfg, 13)
    m = util.build_model(cfg, flat, cuda)
    bx, bh, bd, ns = synth.decode_batch(cfg, specs)
    maxd = int(np.ceil(np.nanmax(bd)))
    for mode in ("argmax", "sampling"):
        m.sampling_seed = 4242
        have = [0] * B
        rows = [[] for _ in range(B)]
        for row, start, samples in m.generate_live(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), list(ns), bd, mode=mode, every=64):
            assert len(samples) > 0 and start == have[row], (row, start, have[row])
            have[row] += len(samples)
            rows[row].append(samples)
        assert "timed out, retried" in m.last_decode_plan and "pipe rows=0" in m.last_decode_plan.split("retried:")[1], m.last_decode_plan
        assert have == list(ns), (have, ns)
        for b in range(B):
            x, h, d, n = synth.decode_inputs(cfg, specs[b][1], specs[b][0], specs[b][2])
            r = oracle.decode(cfg, flat, h, d, x, n, maxd=maxd, mode=mode, seed=4242, row=b)
            np.testing.assert_array_equal(np.concatenate(rows[b]), r["samples"], err_msg="row %d (%s)" % (b, mode))
    # the handle is as usable as after any other call
    outs = m.batch_fast_generate(torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda), list(ns), bd, mode="argmax")
    assert [len(o) for o in outs] == sorted(ns)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    from qpnet_amd import _lib
    assert _lib.LIB_PATH.endswith("libqpnet_hip_testing.so"), _lib.LIB_PATH
    assert os.environ.get("QPN_TEST_PIPE_GIVES_UP")
    main(torch.device("cuda:0"))
    print("LIVE_GIVEUP_CHILD_OK")
