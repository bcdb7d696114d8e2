"""CPU: the host-side pieces of live decode output -- the step that turns successive progress reports into pieces, the two exports'
argument checks, and the refusal of CPU tensors."""
import ctypes as C

import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY
from qpnet_amd.qpnet import live_pieces


def _run(n_rows, reports):
    delivered = [0] * n_rows
    return [live_pieces(delivered, r) for r in reports], delivered


def test_pieces_steady_progress():
    out, delivered = _run(1, [[256], [512], [700]])
    assert out == [[(0, 0, 256)], [(0, 256, 512)], [(0, 512, 700)]]
    assert delivered == [700]


def test_pieces_no_progress_brings_nothing():
    out, delivered = _run(2, [[0, 0], [64, 0], [64, 0], [64, 0], [64, 64]])
    assert out == [[], [(0, 0, 64)], [], [], [(1, 0, 64)]]
    assert delivered == [64, 64]


def test_pieces_several_rows_finish_in_one_poll():
    out, delivered = _run(4, [[64, 64, 0, 0], [100, 90, 1, 0]])
    assert out == [[(0, 0, 64), (1, 0, 64)], [(0, 64, 100), (1, 64, 90), (2, 0, 1)]]
    assert delivered == [100, 90, 1, 0]          # (the zero-sample row never has a piece)


def test_pieces_drop_to_zero_then_catch_up():
    """A re-run starts its counts at zero: nothing is taken back, nothing is handed on twice, and the row goes on where it stopped."""
    out, delivered = _run(2, [[128, 64], [0, 0], [64, 0], [128, 64], [192, 64], [300, 200]])
    assert out == [[(0, 0, 128), (1, 0, 64)], [], [], [], [(0, 128, 192)], [(0, 192, 300), (1, 64, 200)]]
    assert delivered == [300, 200]
    covered = sorted((s, e) for step in out for b, s, e in step if b == 0)
    assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_pieces_accept_ctypes_and_numpy_reports():
    import numpy as np
    delivered = [0, 0]
    assert live_pieces(delivered, (C.c_int64 * 2)(3, 0)) == [(0, 0, 3)]
    assert live_pieces(delivered, np.array([3, 5], dtype=np.int64)) == [(1, 0, 5)]
    assert all(type(v) is int for piece in live_pieces([0], np.array([2])) for v in piece)


def test_exports_refuse_a_null_handle():
    L = _lib.lib()
    assert L.qpn_decode_live(None, 256) == -1 and b"null handle" in L.qpn_last_error()
    done = (C.c_int64 * 1)()
    mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
    assert L.qpn_decode_poll(None, done, C.byref(mirror), C.byref(stride), C.byref(running)) == -1 and b"null handle" in L.qpn_last_error()
    assert L.qpn_decode_poll(None, None, None, None, None) == -1


def test_exports_refuse_to_work_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0   # geometry-only handle
    assert L.qpn_decode_live(hp, 256) == -2 and b"no CPU fallback" in L.qpn_last_error()
    done = (C.c_int64 * 1)()
    mirror, stride, running = C.POINTER(C.c_int32)(), C.c_int64(), C.c_int()
    assert L.qpn_decode_poll(hp, done, C.byref(mirror), C.byref(stride), C.byref(running)) == -2
    L.qpn_destroy(hp)


def test_generate_live_refuses_cpu_tensors():
    import numpy as np
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.generate_live(torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440)), mode="argmax")
    with pytest.raises(ValueError):
        m.generate_live(torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440)), every=0)
