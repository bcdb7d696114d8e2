"""CPU: the segment-table check of qpn_cut_chunks (qpnet_amd/csrc/corpus_segs.h) -- a sweep of valid tables against every single-field corruption, by a
stand-alone program built with the host sanitizers -- and the entry point's own argument checks, which come before a device is looked for."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from qpnet_amd import _lib, loaders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_check_sweep(tmp_path):
    """tests/corpus_segs_sweep.cpp includes only corpus_segs.h: built with AddressSanitizer and UBSan as a program of its own and run as a child process."""
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path / "corpus_segs_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "corpus_segs_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CORPUS_SEGS_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 50000


def test_numpy_record_is_the_c_record():
    assert loaders.CORPUS_SEG_DTYPE.itemsize == C.sizeof(_lib.QpnCorpusSeg) == 32
    for name, _ in _lib.QpnCorpusSeg._fields_:
        assert loaders.CORPUS_SEG_DTYPE.fields[name][1] == getattr(_lib.QpnCorpusSeg, name).offset


def _call(segs, row_first, B=1, frames=2, U=5, bl=4, n_samples=100, n_frames=20, n_aux=3, align=0, w=True, uw=0.5):
    """qpn_cut_chunks with made-up non-null device pointers: every refusal below is decided on the host, before a device is looked for or touched"""
    L = _lib.lib()
    segs = np.array(segs, dtype=loaders.CORPUS_SEG_DTYPE)
    rf = np.array(row_first, dtype=np.int32)
    fake = 0x10000
    rc = L.qpn_cut_chunks(fake, n_samples, fake, fake, n_frames, n_aux, segs.ctypes.data, rf.ctypes.data, fake, fake, len(segs), B, frames, U, bl, C.c_float(uw),
                          fake + align, fake, fake, fake, fake if w else None, None)
    return rc, L.qpn_last_error().decode()


def test_entry_refuses_a_bad_table_before_any_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up device pointers stay on machines without a GPU (tests/test_device_corpus_gpu.py makes the refusal with real buffers)")
    good =[(10, 2, 2, 11, 2)]                                        # (sample0, frame0, factor0, n_samples, n_frames): T + 1 = 11 samples, 2 feature rows
    rc, msg = _call([(95, 2, 2, 11, 2)], [0, 1])
    assert rc == -4 and "row 0 segment 0" in msg and "samples" in msg
    rc, msg = _call([(10, 19, 2, 11, 2)], [0, 1])
    assert rc == -4 and "row 0 segment 0" in msg and "feature rows" in msg
    rc, msg = _call([(10, 2, 18, 11, 2)], [0, 1])
    assert rc == -4 and "row 0 segment 0" in msg and "factors" in msg
    rc, msg = _call([(10, 2, 2, 10, 2)], [0, 1])
    assert rc == -1 and "row 0:" in msg
    rc, msg = _call(good + [(30, 6, 6, 5, 1), (50, 0, 10, 6, 0)], [0, 1, 3], B=2)
    assert rc == -1 and "row 1:" in msg and "feature rows" in msg
    assert _call(good, [0, 1], U=0)[0] == -1 and _call(good, [0, 1], bl=0)[0] == -1 and _call(good, [0, 1], bl=11)[0] == -1
    assert _call(good, [0, 1], n_aux=0)[0] == -1
    rc, msg = _call(good, [0, 1], align=8)
    assert rc == -1 and "16-byte" in msg
    rc, msg = _call(good, [0, 1], uw=float("nan"))
    assert rc == -1 and "unvoiced_weight" in msg
    rc, msg = _call(good, [0, 1])                                     # a valid call without a GPU
    assert rc == -2 and "no CPU fallback" in msg
