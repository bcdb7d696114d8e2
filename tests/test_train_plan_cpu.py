"""CPU: the training layout planner (qpnet_amd/csrc/train_plan.h) -- the gather maps of the packed weights and biases, the gradient slabs and their map,
the per-call arena.  tests/train_plan_sweep.cpp includes only train_plan.h and the HIP-free geometry header: built with AddressSanitizer and UBSan as a
program of its own and run as a child process.  It checks the planner's invariants, and prints a hash of every map, which must be the hash the code in
front of the planner produced for the same geometry (tests/golden/train_plan.json, made from that code: MEASUREMENTS.md)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ("tiny", "paper", "default", "deep64", "paper_aux7", "paper_aux80", "paper_up0", "paper_up8", "paper_q128", "paper_q64",
              "all_adaptive", "all_fixed", "c160")
KEYS = ("wmap", "gmap", "bstart", "blist", "gsrc", "gdst_start", "gdst_list", "gzero", "ctmap", "slabs", "gemm", "params", "arena")


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path_factory.mktemp("train_plan") / "train_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "train_plan_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TRAIN_PLAN_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_planner_invariants_sweep(sweep):
    """every plan and arena passed its checks; 13 geometries x 2 paths x 4 knob settings, five arenas each"""
    words = sweep.split("TRAIN_PLAN_SWEEP_OK")[1].split()
    assert int(words[0]) == len(GEOMETRIES) * 2 * 4 and int(words[2]) == len(GEOMETRIES) * 2 * 4 * 5


def test_width_classes_pass_the_same_invariants(sweep):
    """the nine (n_resch, n_skipch, n_quantize) of tests/test_width_classes_gpu.py -- multiples of 16, not all of 32 -- on the tile path at the four knob settings (the GEMM
    path refuses each): the invariant checks of the named geometries, and no hash (train_plan.json comes from the code in front of the planner)"""
    import test_width_classes_gpu as W
    checked = [line.split()[1] for line in sweep.splitlines() if line.startswith("CHECKED ")]
    assert checked == ["w%d_%d_%d/tile" % csq for csq in W.TRAIN_CSQ]
    words = sweep.split("TRAIN_PLAN_SWEEP_OK")[1].split()
    assert words[3] == "arenas" and int(words[4]) == 4 * len(W.TRAIN_CSQ) and words[5] == "checked"
    assert {line.split()[1].split("/")[0] for line in sweep.splitlines() if line.startswith("GOLDEN ")} == set(GEOMETRIES)


def test_maps_are_those_of_the_code_before_the_planner(sweep):
    with open(os.path.join(ROOT, "tests", "golden", "train_plan.json")) as f:
        want = json.load(f)
    got = {}
    for line in sweep.splitlines():
        if line.startswith("GOLDEN "):
            _, name, key, n, h = line.split()
            got.setdefault(name, {})[key] = [int(n), h]
    assert sorted(want) == sorted("%s/%s" % (g, p) for g in GEOMETRIES for p in ("tile", "gemm"))
    for name in want:
        assert sorted(want[name]) == sorted(KEYS)
        for key in KEYS:
            assert got[name][key] == want[name][key], (name, key)
