"""Child process of test_frame_sampling_gpu.test_rerun_after_a_give_up_draws_with_the_same_track: runs with QPN_LIB = the -DQPN_TESTING build
(qpnet_amd/libqpnet_hip_testing.so) and QPN_TEST_PIPE_GIVES_UP=1, the hook of tests/giveup_child.py `pipe`: the pipelined launch behaves as if a
wait had timed out at once, drains, and the call is re-run on the one-CU kernel -- with the draw track the call was enqueued with.
    python tests/frame_sampling_giveup_child.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(cuda):
    import torch
    import frame_spec as FS
    import util
    from qpnet_amd import synth
    from qpnet_amd.config import PAPER
    cfg = PAPER
    flat = synth.make_weights(cfg, 29)
    bx, bh, bd, ns = synth.decode_batch(cfg, [(61, 4, 1.0), (62, 3, 0.5)])
    xb, hb = torch.from_numpy(bx).to(cuda), torch.from_numpy(bh).to(cuda)
    recs = [(1.0, 0, 1.0, 0.0), (0.7, 40, 0.95, 0.01), (1.3, 100, 0.9, 0.05), (0.5, 20, 0.8, 0.02)]
    track = FS.track_of([[recs[(f + b) % 4] for f in range(bh.shape[2])] for b in range(2)])
    kw = dict(mode="sampling", draw_track=track, row_seeds=[0xFEEDFACE12345678, 0x8000000000000001])
    assert os.environ.pop("QPN_TEST_PIPE_GIVES_UP")               # (read when a handle is created)
    ref = util.build_model(cfg, flat, cuda)
    ref.sampling_seed = 77
    good = ref.batch_fast_generate(xb, hb, list(ns), bd, **kw)
    assert "pipe rows=2" in ref.last_decode_plan and "retried" not in ref.last_decode_plan, ref.last_decode_plan
    no_track = ref.batch_fast_generate(xb, hb, list(ns), bd, mode="sampling", row_seeds=kw["row_seeds"])
    os.environ["QPN_TEST_PIPE_GIVES_UP"] = "1"
    m = util.build_model(cfg, flat, cuda)
    m.sampling_seed = 77
    outs = m.batch_fast_generate(xb, hb, list(ns), bd, **kw)
    assert "timed out, retried" in m.last_decode_plan and "pipe rows=0" in m.last_decode_plan.split("retried:")[1], m.last_decode_plan
    for a, b, c in zip(outs, good, no_track):
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(b, c)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    from qpnet_amd import _lib
    assert _lib.LIB_PATH.endswith("libqpnet_hip_testing.so"), _lib.LIB_PATH
    main(torch.device("cuda:0"))
    print("FRAME_SAMPLING_GIVEUP_CHILD_OK")
