"""CPU: the weight-gradient planner (qpnet_amd/csrc/train_wgrad_plan.h) -- the five contraction records of a step, the kernel instance each gets, the
row-block split, the GEMM path's form of a record.  tests/wgrad_plan_sweep.cpp includes only that header and the HIP-free geometry header: built with
AddressSanitizer and UBSan as a program of its own and run as a child process.  It checks the planner's invariants, the boundary cases no GPU test can
hold and the kernel instances bench.py names, and prints one line per launch, which must be the line the code in front of the planner produced for the
same step (tests/golden/wgrad_plan.json, made from that code: MEASUREMENTS.md)."""
import json
import os
import shutil
import subprocess

import pytest

from test_train_plan_cpu import GEOMETRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("default", "generic", "no_stack_queue", "no_hoist", "no_post_pair", "gemm")


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "wgrad_plan_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "WGRAD_PLAN_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_planner_invariants_sweep(sweep):
    """every step passed its checks (the pins and the boundary cases are CHECKs of the same program): 13 named geometries and the nine width classes, B = 1 and 2,
    six knob settings -- the GEMM setting only where train_plan takes the widths -- and no record refused"""
    import test_width_classes_gpu as W
    lines = sweep.splitlines()
    assert [ln.split()[1] for ln in lines if ln.startswith("NAMED ")] == list(GEOMETRIES)
    assert [ln.split()[1] for ln in lines if ln.startswith("CHECKED ")] == ["w%d_%d_%d" % csq for csq in W.TRAIN_CSQ]
    words = sweep.split("WGRAD_PLAN_SWEEP_OK")[1].split()
    n_geom = len(GEOMETRIES) + len(W.TRAIN_CSQ)
    gemm_steps = 2 * len(GEOMETRIES)      # every named geometry is a multiple of 32 in all three widths; none of the width classes is
    assert int(words[6]) == gemm_steps and words[7] == "gemm_steps"
    assert int(words[0]) == n_geom * 2 * (len(KNOBS) - 1) + gemm_steps and words[1] == "steps"
    assert int(words[2]) > int(words[0]) and int(words[4]) == 0 and words[5] == "refused"


def test_records_and_picks_are_those_of_the_code_before_the_planner(sweep):
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plan.json")) as f:
        want = json.load(f)
    got = {}
    for line in sweep.splitlines():
        if line.startswith("GOLDEN "):
            _, step, launch, rest = line.split(" ", 3)
            assert launch not in got.setdefault(step, {}), (step, launch)
            got[step][launch] = rest
    assert sorted(want) == sorted("%s/B%d/%s" % (g, b, k) for g in GEOMETRIES for b in (1, 2) for k in KNOBS)
    for step in want:
        assert got[step] == want[step], step
