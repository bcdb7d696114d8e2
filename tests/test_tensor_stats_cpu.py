"""CPU: per-tensor training statistics (qpn_tensor_stats) without a GPU -- the planner of qpnet_amd/csrc/train_stats_plan.h, the argument checks of the C ABI and the
resource report of the two kernels of train_stats.hip.

tests/train_stats_sweep.cpp includes only the plan header: built with AddressSanitizer and UBSan as a program of its own and run as a child process, over the tensor
tables of the tiny, paper and default geometries (written here from the configurations' parameter layout) and over adversarial tables of its own."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from qpnet_amd import _lib
from qpnet_amd.config import TINY, PAPER, DEFAULT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEM = 2048                                   # QPN_STATS_ITEM (train_stats_plan.h); the sweep prints the header's value
GEOMETRIES = (("tiny", TINY), ("paper", PAPER), ("default", DEFAULT))


def _ends(cfg):
    ends, o = [], 0
    for _, shp in cfg.param_layout():
        n = 1
        for s in shp:
            n *= s
        o += n
        ends.append(o)
    return ends


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    d = tmp_path_factory.mktemp("train_stats")
    tables = str(d / "tables.txt")
    with open(tables, "w") as f:
        for name, cfg in GEOMETRIES:
            ends = _ends(cfg)
            f.write("%s %d %s\n" % (name, len(ends), " ".join(str(e) for e in ends)))
    exe = str(d / "train_stats_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "train_stats_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, tables], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TRAIN_STATS_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_planner_sweep(sweep):
    """every table passed the tiling checks, every malformed one was refused; the real tables are the three geometries'"""
    got = [line.split() for line in sweep.splitlines() if line.startswith("TABLE ")]
    assert [(w[1], int(w[2]), int(w[4])) for w in got] == [(name, len(cfg.param_layout()), cfg.n_params) for name, cfg in GEOMETRIES]
    words = sweep.split("TRAIN_STATS_SWEEP_OK")[1].split()
    assert int(words[0]) >= 3 + 15 and int(words[2]) == 3 and int(words[6]) >= 11
    assert int(words[9]) == ITEM


def test_the_real_tables_have_the_starts_the_kernel_must_cope_with():
    """behind the upsampling pair (110 + 1 elements) every tensor of the three geometries starts 3 floats past a 16-byte boundary"""
    for _, cfg in GEOMETRIES:
        ends = _ends(cfg)
        keys = [k for k, _ in cfg.param_layout()]
        i = keys.index("upsampling.conv.bias")
        assert ends[i] - ends[i - 1] == 1 and ends[i - 1] - ends[i - 2] == 110
        assert {e % 4 for e in ends[i:-1]} == {3}


# ---------------------------------------------------------------- argument checks (no device is looked at before them)
P = C.c_void_p(4096)                          # a non-NULL "device pointer": never dereferenced, every call here returns before the device
ENDS = [4, 9, 20]


@pytest.fixture(scope="module")
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0
    yield L, hp
    L.qpn_destroy(hp)


def _call(L, hp, flat=P, grad=P, m=P, v=P, n=20, step=3, b1=0.9, b2=0.999, eps=1e-8, den=None, nt=None, ends=ENDS, out=True, no_table=False):
    nt = len(ends) if nt is None else nt
    table = None if no_table else (C.c_int64 * max(len(ends), 1))(*ends)
    rec = (_lib.QpnTensorStat * max(nt, 1))() if out else None
    rc = L.qpn_tensor_stats(hp, flat, grad, m, v, n, step, b1, b2, eps, den, nt, table, rec, None)
    return rc, L.qpn_last_error().decode()


BAD = [
    ("d_flat", dict(flat=None)),
    ("h_tensor_end is NULL", dict(no_table=True)),
    ("h_out", dict(out=False)),
    ("n_tensors", dict(nt=0)),
    ("n_tensors", dict(nt=-2)),
    ("n_tensors", dict(nt=(1 << 20) + 1)),
    ("strictly ascending", dict(ends=[4, 4, 20])),
    ("strictly ascending", dict(ends=[4, 3, 20])),
    ("h_tensor_end[0]", dict(ends=[0, 9, 20])),
    ("is not n", dict(n=21)),
    ("is not n", dict(ends=[4, 9, 19])),
    ("d_v is NULL", dict(v=None)),
    ("d_m is NULL", dict(m=None)),
    ("step", dict(step=0)),
    ("beta1", dict(b1=1.0)),
    ("beta1", dict(b1=-0.1)),
    ("beta1", dict(b1=float("nan"))),
    ("beta2", dict(b2=1.0)),
    ("beta2", dict(b2=-0.5)),
    ("beta2", dict(b2=float("nan"))),
    ("eps", dict(eps=float("nan"))),
    ("eps", dict(eps=float("inf"))),
    ("eps", dict(eps=-1e-8)),
]


@pytest.mark.parametrize("word,kw", BAD, ids=["%s-%d" % (b[0].split()[0], i) for i, b in enumerate(BAD)])
def test_argument_errors_name_the_argument(word, kw, handle):
    L, hp = handle
    rc, msg = _call(L, hp, **kw)
    assert rc == -1 and "tensor_stats" in msg and word in msg, (rc, msg)


def test_null_handle():
    L = _lib.lib()
    rc, msg = _call(L, None)
    assert rc == -1 and "null handle" in msg


def test_valid_calls_need_a_device(handle):
    """a handle created without a GPU: every valid form of the call -- all buffers, no gradient, no moments (step and the betas are then not looked at) -- is QPN_ENODEV"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L, hp = handle
    for kw in (dict(), dict(grad=None), dict(m=None, v=None, step=0, b1=7.0, b2=float("nan"), eps=-1.0), dict(den=P), dict(eps=0.0, b1=0.0, b2=0.0)):
        rc, msg = _call(L, hp, **kw)
        assert rc == -2 and "no CPU fallback" in msg, (kw, rc, msg)


# ---------------------------------------------------------------- the compiler's resource report
def test_the_two_kernels_keep_nothing_in_scratch():
    """memory-bound, full occupancy and nothing in scratch memory, like the kernels of train_adam.hip (tests/test_kernel_resources.py reads the same report)"""
    import test_kernel_resources as KR
    if not os.path.exists(KR.HIPCC):
        pytest.skip("hipcc not installed")
    rep = KR._report("train_stats.hip")
    for frag in ("k_tensor_stats_items", "k_tensor_stats_fold"):
        hits = {k: v for k, v in rep.items() if frag in k}
        assert len(hits) == 1, sorted(rep)
        for name, r in hits.items():
            assert r.get("ScratchSize [bytes/lane]", -1) == 0, (name, r)
            assert r.get("Occupancy [waves/SIMD]", -1) >= 8, (name, r)
