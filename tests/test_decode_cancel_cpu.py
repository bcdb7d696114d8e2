"""CPU: the host-side pieces of decode cancel -- generate_live's on_close argument, the two exports' declarations and argument checks."""
import ctypes as C
import os
import re

import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _live_args():
    import numpy as np
    import torch
    return torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440))


def test_on_close_is_checked_before_the_device_is_touched():
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    with pytest.raises(ValueError, match="on_close"):          # (CPU tensors: the "no CPU fallback" refusal would come next)
        m.generate_live(*_live_args(), mode="argmax", on_close="bogus")
    with pytest.raises(ValueError, match="on_close"):
        m.generate_live(*_live_args(), mode="argmax", on_close=None)
    for ok in ("finish", "cancel"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate_live(*_live_args(), mode="argmax", on_close=ok)
    assert m.last_decode_counts is None and m.last_decode_cancelled is False


def test_header_declares_both_exports():
    hdr = open(os.path.join(ROOT, "include", "qpnet_hip.h")).read()
    sigs = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+qpn_decode_cancel\s*\(\s*qpn_handle\s*\*\s*h\s*\)\s*;", sigs)
    assert re.search(r"\bint\s+qpn_decode_final_counts\s*\(\s*qpn_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*h_done\s*,\s*int\s*\*\s*cancelled\s*\)\s*;", sigs)
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert table["qpn_decode_cancel"] == (C.c_int, [C.c_void_p])
    assert table["qpn_decode_final_counts"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)])
    assert "no cancel" not in hdr


def test_exports_refuse_a_null_handle():
    L = _lib.lib()
    done, cancelled = (C.c_int64 * 1)(), C.c_int()
    assert L.qpn_decode_cancel(None) == -1 and b"null handle" in L.qpn_last_error()
    assert L.qpn_decode_final_counts(None, done, C.byref(cancelled)) == -1 and b"null handle" in L.qpn_last_error()
    assert L.qpn_decode_final_counts(None, None, None) == -1


def test_exports_refuse_to_work_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0   # geometry-only handle
    done, cancelled = (C.c_int64 * 1)(), C.c_int()
    assert L.qpn_decode_cancel(hp) == -2 and b"no CPU fallback" in L.qpn_last_error()
    assert L.qpn_decode_final_counts(hp, done, C.byref(cancelled)) == -2
    L.qpn_destroy(hp)
