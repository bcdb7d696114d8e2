"""CPU: the decode program planner (qpnet_amd/csrc/decode_program.h) -- the LDS layout of the one-CU kernels, the gather map of the packed weights for every
kernel family, the interpreter's task table, the bias list and every offset the launchers hand on.  tests/decode_program_sweep.cpp includes only that header
and the HIP-free geometry header: built with AddressSanitizer and UBSan as a program of its own and run as a child process.  It decodes the map back through
the kernels' position formulas, and prints a hash of every list, which must be the hash the code in front of the planner produced for the same geometry
(tests/golden/decode_program.json, made from that code: MEASUREMENTS.md)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ("tiny", "paper", "default", "deep64", "paper_aux7", "paper_aux80", "paper_up0", "paper_up8", "paper_q128", "paper_q64",
              "all_adaptive", "all_fixed", "c160", "c160_s96_a17", "c256_q64")
REFUSED = ("refused_c24", "refused_c1024")
BATCHED = ("default", "c256_q64")          # the geometries the batched cooperative kernel takes: the code before the planner opened their maps with its blocks
KEYS = ("map", "tasks", "bias_src", "lds", "fast", "w_past_il", "aux", "cb", "single_cu_ok", "biases")


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path_factory.mktemp("decode_program") / "decode_program_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "decode_program_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DECODE_PROGRAM_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_program_invariants_sweep(sweep):
    """every program passed its checks: 15 geometries, the four with n_resch a multiple of 8 and >= 128 both with and without the batched kernel's blocks"""
    words = sweep.split("DECODE_PROGRAM_SWEEP_OK")[1].split()
    assert int(words[0]) == len(GEOMETRIES) + 4


def test_program_is_that_of_the_code_before_the_planner(sweep):
    with open(os.path.join(ROOT, "tests", "golden", "decode_program.json")) as f:
        want = json.load(f)
    got = {}
    for line in sweep.splitlines():
        if line.startswith("GOLDEN "):
            _, name, key, n, h = line.split()
            got.setdefault(name, {})[key] = [int(n), h]
        elif line.startswith("REFUSED "):
            _, name, rc, message = line.split(None, 3)
            got[name] = {"rc": int(rc), "message": message}
    assert sorted(want) == sorted(["%s/cb%d" % (g, g in BATCHED) for g in GEOMETRIES] + ["%s/cb0" % g for g in REFUSED])
    for name in want:
        if name.split("/")[0] in REFUSED:
            assert got[name] == want[name] and want[name]["rc"] == -1, name          # QPN_EINVAL, and the text
            continue
        assert sorted(want[name]) == sorted(KEYS)
        for key in KEYS:
            assert got[name][key] == want[name][key], (name, key)
