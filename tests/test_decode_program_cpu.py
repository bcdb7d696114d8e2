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
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-pthread",
                    os.path.join(ROOT, "tests", "decode_program_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DECODE_PROGRAM_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_program_invariants_sweep(sweep):
    """every program passed its checks: 15 geometries, the four with n_resch a multiple of 8 and >= 128 both with and without the batched kernel's blocks"""
    words = sweep.split("DECODE_PROGRAM_SWEEP_OK")[1].split()
    assert int(words[0]) == len(GEOMETRIES) + 4 and words[1] == "programs"


def _checked(sweep):
    """name -> refused, of the "CHECKED name[ refused]" lines"""
    return {line.split()[1]: line.endswith(" refused") for line in sweep.splitlines() if line.startswith("CHECKED ")}


def test_width_classes_pass_the_same_invariants(sweep):
    """the (n_resch, n_skipch, n_quantize) of tests/test_width_classes_gpu.py -- multiples of 16 that are not multiples of 32, and the widths that decode without
    training: the invariant checks of the named geometries (with the batched kernel's blocks too where n_resch is a multiple of 8 and >= 128), and no hash
    (decode_program.json comes from the code in front of the planner).  The training widths one tile height or another rules out are refused by the planner."""
    import test_width_classes_gpu as W
    got = _checked(sweep)
    want = {}
    for C, S, Q in list(W.DECODE_CSQ) + [W.COOPB_CSQ[1]] + [csq for csq in W.TRAIN_CSQ if csq not in W.DECODE_CSQ]:
        for cb in (0, 1) if C % 8 == 0 and C >= 128 else (0,):
            want["w%d_%d_%d/cb%d" % (C, S, Q, cb)] = (C, S, Q) in W.TRAIN_ONLY_CSQ
    assert got == want
    words = sweep.split("DECODE_PROGRAM_SWEEP_OK")[1].split()
    assert words[3] == "checked" and int(words[2]) == sum(not refused for refused in want.values())
    assert {line.split()[1].split("/")[0] for line in sweep.splitlines() if line.startswith("GOLDEN ")} == set(GEOMETRIES)


def test_acceptance_is_the_tile_height_rule(sweep):
    """n_resch = 4, 8, ..., 272 x n_skipch in {16, 48, 72, 80, 136, 144} x n_quantize in {16, 32, 48, 64, 80, 96, 192} on a 2 + 2-layer geometry with n_aux 39: the
    planner accepts exactly what the rule restated in the sweep program accepts (it exits at the first difference), every accepted program passed the invariant checks,
    and one CU stops holding the step state between the two widths tests/test_width_classes_gpu.py decodes on either side"""
    import test_width_classes_gpu as W

    def rows(K):          # rows of a 4 KiB tile whose matrix has K input columns: 64 lanes of 16 floats, K padded to 16, 32, 64, ...
        return 1024 // max(16, 1 << (K - 1).bit_length())

    def accepts(C, S, Q, A=39):
        return C % rows(C) == 0 and S % rows(C) == 0 and S % rows(S) == 0 and Q % rows(S) == 0 and (2 * C) % rows(A) == 0
    n = sum(accepts(C, S, Q) for C in range(4, 273, 4) for S in (16, 48, 72, 80, 136, 144) for Q in (16, 32, 48, 64, 80, 96, 192))
    words = sweep.split("DECODE_PROGRAM_SWEEP_OK")[1].split()
    assert words[5] == "swept" and int(words[4]) == 68 * 6 * 7 and words[7] == "accepted" and int(words[6]) == n and 300 < n < 68 * 6 * 7 - 300
    assert all(accepts(*csq) for csq in W.DECODE_ALL) and not any(accepts(*csq) for csq in W.TRAIN_ONLY_CSQ) and not any(accepts(C, 64, 64) for C in (8, 24, 40))
    line = [l for l in sweep.splitlines() if l.startswith("SINGLE_CU ")]
    assert len(line) == 1 and line[0].split() == ["SINGLE_CU", "last", str(W.SINGLE_CU_PAIR[0]), "first_not", str(W.SINGLE_CU_PAIR[1])]


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
