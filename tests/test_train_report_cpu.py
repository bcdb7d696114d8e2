"""CPU: the training reports' ledger (qpnet_amd/csrc/train_report.h) -- how a step's status word, its loss one step late and the clipping norm that travels with that
loss come back without draining the stream.  tests/train_report_sweep.cpp includes only that HIP-free header: built with AddressSanitizer and UBSan as a program of its
own and run as a child process.  It drives seeded random call sequences through the ledger and through a transcription of the bookkeeping the ledger replaced, on a fake
device, compares the two after every call and asserts the ledger's invariants (MEASUREMENTS.md)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QPN_OK, QPN_ENODEV, QPN_ERANGE = 0, -2, -4                              # include/qpnet_hip.h
N_SEQUENCES, TAIL = 1500, 8                                             # of each kind; the calls that fetch every outstanding report at a sequence's end
# every bit the kernels set in the status word: the code it is reported as, and words only its message has
STATUS_BITS = {
    1: (QPN_ERANGE, "pitch-dependent tap outside the layer input"),
    2: (QPN_ERANGE, "target class outside [0, n_quantize)"),
    4: (QPN_ENODEV, "one-launch residual stack gave up"),
    8: (QPN_ERANGE, "a peer rank flagged its chunk"),
    32: (QPN_ERANGE, "teacher logits of a distillation loss"),
    64: (QPN_ERANGE, "among the sample weights"),
    1 << 16: (QPN_ERANGE, "non-finite gradient norm"),
}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = shutil.which("amdclang++")
    if not cxx:
        pytest.skip("no ROCm clang")
    exe = str(tmp_path_factory.mktemp("train_report") / "train_report_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "train_report_sweep.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TRAIN_REPORT_SWEEP_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout


def test_ledger_and_transcription_agree_and_the_invariants_hold(sweep):
    """every operation of every sequence passed: 1500 sequences of 200 over all operations, 1500 of 100 steps-only ones (invariant (b)), each with its tail"""
    words = sweep.split("TRAIN_REPORT_SWEEP_OK")[1].split()
    assert int(words[0]) == N_SEQUENCES * (200 + TAIL) + N_SEQUENCES * (100 + TAIL)
    line = [ln for ln in sweep.splitlines() if ln.startswith("REPORTS ")][0].split()
    counts = dict(zip(line[0::2], map(int, line[1::2])))
    assert counts["REPORTS"] > 10000 and counts["NORMS"] > 10000          # the sequences do raise flags and return norms


def test_status_table_covers_every_bit_the_kernels_set(sweep):
    got = {}
    for ln in sweep.splitlines():
        if ln.startswith("STATUS "):
            _, bit, rc, msg = ln.split(" ", 3)
            got[int(bit)] = (int(rc), msg)
    assert sorted(got) == sorted(STATUS_BITS)
    for bit, (rc, words) in STATUS_BITS.items():
        assert got[bit][0] == rc and words in got[bit][1], bit
        assert sum(words in m for _, m in got.values()) == 1, words    # ... which tell it from every other message


def test_slot_geometry(sweep):
    line = [ln for ln in sweep.splitlines() if ln.startswith("GEOMETRY ")][0].split()
    assert [int(v) for v in line[1:]] == [72, 64, 64]                   # a slot, the partial sums at 0..63, the norm behind them: what train_adam.hip's kernels write
