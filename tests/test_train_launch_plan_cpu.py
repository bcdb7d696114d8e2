"""CPU: the training step's launch planner (qpnet_amd/csrc/train_launch_plan.h) -- the shape of a call, what the forward and the backward launch, on which stream and
behind which event.  tests/train_launch_plan_sweep.cpp includes only HIP-free headers: built with AddressSanitizer and UBSan as a program of its own and run as a child
process.  It checks the planner's invariants over geometries x knob settings x batch sizes x chunk lengths x CU counts x run-time facts, and prints the plan text of a
fixed subset, which must be the text recorded from the launchers in front of the planner (tests/golden/train_launch_plan.json: MEASUREMENTS.md)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_GEOMETRIES = ("tiny", "paper", "default", "deep64", "paper_up0", "paper_aux80", "c160")
N_GEOMETRIES, N_KNOBS = 13 + 9, 21          # the named ones of test_train_plan_cpu.py and the width classes; the arrangement test's 16 settings, the default and four more


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path_factory.mktemp("train_launch_plan") / "train_launch_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "train_launch_plan_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TRAIN_LAUNCH_PLAN_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_planner_invariants_sweep(sweep):
    """every forward and backward plan passed its checks: geometries x knob settings x B in {1, 3} x 7 chunk lengths x 3 CU counts x (the plain step and each fact of the
    forward flipped) x (the same for the backward), a forward and a backward plan each"""
    words = sweep.split("TRAIN_LAUNCH_PLAN_SWEEP_OK")[1].split()
    assert int(words[0]) == N_GEOMETRIES * N_KNOBS * 2 * 7 * 3 * 9 * 9 * 2


def test_width_classes_and_knob_settings_are_the_gpu_tests(sweep):
    """the sweep's width classes are test_width_classes_gpu.TRAIN_CSQ, its knob settings hold every one of test_backward_launch_arrangements_agree"""
    import test_width_classes_gpu as W
    import test_train_gpu as T
    checked = [line.split()[1] for line in sweep.splitlines() if line.startswith("CHECKED ")]
    assert checked == ["w%d_%d_%d" % csq for csq in W.TRAIN_CSQ]
    settings = {line[7:].split("\t")[0].split("/")[1] for line in sweep.splitlines() if line.startswith("GOLDEN ")}
    mark = [m for m in T.test_backward_launch_arrangements_agree.pytestmark if m.name == "parametrize"][0]
    for knobs in mark.args[1]:
        assert ",".join("%s=%s" % kv for kv in knobs.items()) in settings, knobs
    assert {"default", "QPN_POST_WIDE=0", "QPN_POST_FUSE=0", "QPN_PREP_FUSE=0", "QPN_CE_SEPARATE=1"} <= settings and len(settings) == N_KNOBS


def test_plans_are_the_launches_of_the_code_before_the_planner(sweep):
    """the golden file stores the recorded lines without repetition (every distinct word once, a text as word indices, a case as its forward and backward text)"""
    with open(os.path.join(ROOT, "tests", "golden", "train_launch_plan.json")) as f:
        gold = json.load(f)
    texts = [" ".join(gold["words"][i] for i in t) for t in gold["texts"]]
    want = {"%s/%s/%s" % (geom, knobs, case): texts[fb[0]] + " | " + texts[fb[1]]
            for geom, per_knob in gold["plans"].items() for knobs, cases in per_knob.items() for case, fb in zip(gold["cases"], cases)}
    got = {}
    for line in sweep.splitlines():
        if line.startswith("GOLDEN "):
            key, text = line[7:].split("\t")
            got[key] = text
    assert len(want) == len(GOLDEN_GEOMETRIES) * N_KNOBS * 2 * 2 and {k.split("/")[0] for k in want} == set(GOLDEN_GEOMETRIES)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
