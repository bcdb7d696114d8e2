"""CPU: the decode launch plan (qpnet_amd/csrc/decode_plan.h) through qpn_decode_plan_query on handles created without using a GPU -- the plan strings of
every branch of the policy for the three named geometries on 256 and 64 compute units -- and the planner's invariants over a grid, checked by a
stand-alone program built with the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY, PAPER, DEFAULT, QPNetConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("QPN_DECODE_COOP", "QPN_DECODE_COOPB", "QPN_DECODE_PIPE", "QPN_PIPE_NU", "QPN_DECODE_GENERIC")
PIPE_ONE_CU = "pipe rows=0 waves=0 x 0 (1 per group); one-cu rows=%d"


def pipe(B, waves, rows, per):
    return "pipe rows=%d waves=%d x %d (%d per group); one-cu rows=0" % (B, waves, rows, per)


def query(monkeypatch, cfg, n_cus, B, attempt=0, **knobs):
    """-> (rc, plan text) of a fresh handle created under the knob setting (the environment is read at qpn_create)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(cfg)), C.byref(hp)) == 0
    try:
        buf = C.create_string_buffer(256)
        rc = L.qpn_decode_plan_query(hp, n_cus, B, attempt, buf, len(buf))
        return rc, buf.value.decode()
    finally:
        L.qpn_destroy(hp)


# (geometry, compute units, B, attempt, knobs, plan)
TABLE = [
    (PAPER, 256, 1, 0, {}, pipe(1, 1, 1, 1)),
    (PAPER, 256, 49, 0, {}, pipe(49, 1, 49, 2)),
    (PAPER, 256, 80, 0, {}, pipe(80, 1, 80, 2)),
    (PAPER, 256, 100, 0, {}, pipe(100, 1, 100, 3)),
    (PAPER, 256, 145, 0, {}, pipe(145, 2, 73, 2)),
    (PAPER, 256, 300, 0, {}, pipe(300, 4, 75, 2)),
    (PAPER, 256, 100, 0, {"QPN_PIPE_NU": 2}, pipe(100, 2, 50, 2)),
    (PAPER, 256, 20, 0, {"QPN_DECODE_PIPE": 0}, PIPE_ONE_CU % 20),
    (PAPER, 256, 20, 0, {"QPN_DECODE_COOP": 4}, "coop G=4 rows=20"),
    (PAPER, 256, 80, 0, {"QPN_DECODE_COOP": 4}, "coop G=2 rows=80"),
    (PAPER, 256, 20, 1, {}, PIPE_ONE_CU % 20),
    (DEFAULT, 256, 1, 0, {}, "coopb G=64 groups=1 x 1 rows=1"),
    (DEFAULT, 256, 20, 0, {}, "coopb G=64 groups=4 x 5 rows=20"),
    (DEFAULT, 256, 49, 0, {}, "coopb G=64 groups=4 x 13 rows=49"),
    (DEFAULT, 256, 80, 0, {}, "coopb G=64 launches=2 x 40 rows=80"),
    (DEFAULT, 256, 145, 0, {}, "coopb G=64 launches=3 x 49 rows=145"),
    (DEFAULT, 256, 300, 0, {}, "coopb G=64 launches=5 x 60 rows=300"),
    (DEFAULT, 256, 1, 0, {"QPN_DECODE_COOPB": 0}, "coop G=128 rows=1"),
    (DEFAULT, 256, 20, 0, {"QPN_DECODE_COOPB": 0}, "coop G=8 rows=20"),
    (DEFAULT, 256, 145, 0, {"QPN_DECODE_COOPB": 0}, "coop G=1 rows=145"),
    (DEFAULT, 256, 300, 0, {"QPN_DECODE_COOPB": 0}, "coop G=128 rows=300"),      # known quirk: the per-batch cap applies only while B < n_cus
    (DEFAULT, 256, 1, 0, {"QPN_DECODE_COOPB": 8}, "coop G=128 rows=1"),
    (DEFAULT, 256, 1, 1, {}, "coop G=64 rows=1"),
    (DEFAULT, 256, 20, 1, {}, "coop G=4 rows=20"),
    (DEFAULT, 256, 145, 1, {}, "coop G=1 rows=145"),
    (TINY, 256, 3, 0, {}, PIPE_ONE_CU % 3),
    (PAPER, 64, 3, 0, {}, pipe(3, 1, 3, 1)),
    (PAPER, 64, 20, 0, {}, pipe(20, 1, 20, 3)),
    (PAPER, 64, 20, 0, {"QPN_PIPE_NU": 2}, pipe(20, 2, 10, 2)),
    (DEFAULT, 64, 20, 0, {}, "coopb G=64 launches=2 x 10 rows=20"),
    (DEFAULT, 64, 300, 0, {}, "coopb G=64 launches=19 x 16 rows=300"),
]


@pytest.mark.parametrize("cfg,n_cus,B,attempt,knobs,want", TABLE,
                         ids=["%s-%dcu-B%d-a%d%s" % ({id(PAPER): "paper", id(DEFAULT): "default", id(TINY): "tiny"}[id(t[0])], t[1], t[2], t[3],
                                                    "".join("-%s=%s" % (k[4:].lower(), v) for k, v in t[4].items())) for t in TABLE])
def test_plan_table(monkeypatch, cfg, n_cus, B, attempt, knobs, want):
    assert query(monkeypatch, cfg, n_cus, B, attempt, **knobs) == (0, want)


def test_no_retry_from_one_workgroup_per_utterance(monkeypatch):
    L = _lib.lib()
    assert query(monkeypatch, TINY, 256, 3, 1)[0] == -5 and b"no retry" in L.qpn_last_error()
    assert query(monkeypatch, DEFAULT, 256, 145, 1, QPN_DECODE_COOPB=0)[0] == -5
    assert query(monkeypatch, PAPER, 256, 20, 1, QPN_DECODE_PIPE=0)[0] == -5


def test_query_argument_checks(monkeypatch):
    L = _lib.lib()
    assert L.qpn_decode_plan_query(None, 256, 1, 0, C.create_string_buffer(8), 8) == -1
    assert query(monkeypatch, PAPER, 256, 0)[0] == -1 and query(monkeypatch, PAPER, 256, 1, 2)[0] == -1
    import torch
    if not torch.cuda.is_available():
        assert query(monkeypatch, PAPER, 0, 1)[0] == -2      # a geometry-only handle has no device of its own to plan for


def test_narrow_residual_width_is_refused_not_divided_by(monkeypatch):
    """n_resch in 1..7 makes the batched cooperative kernel's group size n_resch / 8 zero.  The decode program does not cover such a geometry (its channel
    counts are no multiples of the tile height), so every decode entry point refuses it before any plan is made, and so does the query; the planner itself
    evaluates the batched kernel's arithmetic only where that kernel can apply (the sweep below plans for n_resch = 4)."""
    cfg = QPNetConfig(n_resch=4, n_skipch=32, dilationF_depth=2, dilationF_repeat=1, dilationA_depth=1, dilationA_repeat=1)
    for n_cus in (256, 7):
        assert query(monkeypatch, cfg, n_cus, 2) == (-1, "") and b"tile height" in _lib.lib().qpn_last_error()


def test_planner_invariants_sweep(tmp_path):
    """tests/decode_plan_sweep.cpp includes only decode_plan.h: built with AddressSanitizer and UBSan as a program of its own and run as a child process."""
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path / "decode_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "decode_plan_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DECODE_PLAN_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 300000
