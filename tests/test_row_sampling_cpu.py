"""CPU: per-row sampling records (qpn_decode_row_sampling; row_seeds= and per-row temperature / top_k / top_p / min_p; loaders.row_seed) -- what is
checked before a device is looked at: the ABI's argument rules on a handle created without a GPU, the Python surface's ValueErrors in front of the
device layer, and the per-file seed of run_decode --per_file_seed."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from qpnet_amd import _lib, loaders
from qpnet_amd.config import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, OK = -1, 0


@pytest.fixture()
def handle():
    L = _lib.lib()
    hp = C.c_void_p()
    assert L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)) == 0      # (without a GPU: a geometry-only handle)
    yield L, hp
    L.qpn_destroy(hp)


def _recs(*rows):
    return (_lib.QpnRowDraw * len(rows))(*[_lib.QpnRowDraw(*r) for r in rows])


GOOD = (0xF00DF00DF00DF00D, 7, 0.7, 40, 0.9, 0.05)


def test_abi_refuses_bad_records_naming_field_and_row(handle):
    L, hp = handle
    Q = TINY.n_quantize
    bad = {"temperature": [(1, 0, 0.0, 0, 1.0, 0.0), (1, 0, -1.0, 0, 1.0, 0.0), (1, 0, float("nan"), 0, 1.0, 0.0), (1, 0, float("inf"), 0, 1.0, 0.0), (1, 0, 1e-45, 0, 1.0, 0.0)],
           "top_k": [(1, 0, 1.0, -1, 1.0, 0.0), (1, 0, 1.0, Q + 1, 1.0, 0.0)],
           "top_p": [(1, 0, 1.0, 0, 0.0, 0.0), (1, 0, 1.0, 0, 1.5, 0.0), (1, 0, 1.0, 0, float("nan"), 0.0)],
           "min_p": [(1, 0, 1.0, 0, 1.0, -0.1), (1, 0, 1.0, 0, 1.0, 1.5), (1, 0, 1.0, 0, 1.0, float("nan"))]}
    for field, recs in bad.items():
        for rec in recs:
            for row in (0, 2):
                rows = [GOOD] * 3
                rows[row] = rec
                assert L.qpn_decode_row_sampling(hp, 3, _recs(*rows)) == EINVAL, (field, rec)
                msg = L.qpn_last_error().decode()
                assert field in msg and ("row %d" % row) in msg, msg
                # the per-value message is qpn_decode_sampling_ex's, with the row in front
                assert L.qpn_decode_sampling_ex(hp, *rec[2:]) == EINVAL
                assert msg == "row %d: %s" % (row, L.qpn_last_error().decode())
    assert L.qpn_decode_row_sampling(hp, -1, _recs(GOOD)) == EINVAL and "n_rows" in L.qpn_last_error().decode()
    assert L.qpn_decode_row_sampling(hp, 2, None) == EINVAL and "NULL" in L.qpn_last_error().decode()
    assert L.qpn_decode_row_sampling(None, 0, None) == EINVAL


def test_abi_accepts_good_records_and_switches_off(handle):
    L, hp = handle
    Q = TINY.n_quantize
    assert L.qpn_decode_row_sampling(hp, 0, None) == OK                          # off on a handle that never had any
    assert L.qpn_decode_row_sampling(hp, 3, _recs(GOOD, (0, 0, 1.0, 0, 1.0, 0.0), ((1 << 64) - 1, (1 << 32) - 1, 100.0, Q, 1.0, 1.0))) == OK
    assert L.qpn_decode_row_sampling(hp, 1, _recs(GOOD)) == OK                   # replaces the table
    assert L.qpn_decode_row_sampling(hp, 0, _recs(GOOD)) == OK                   # 0 rows: off, whatever the pointer
    assert L.qpn_decode_row_sampling(hp, 0, None) == OK


def test_record_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "qpnet_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} qpn_row_draw;", hdr)
    assert m, "qpn_row_draw is not declared"
    decl = re.sub(r"\s+", " ", m.group(1)).strip()
    assert decl == "uint64_t seed; uint32_t stream; float temperature; int32_t top_k; float top_p, min_p;"
    assert [n for n, _ in _lib.QpnRowDraw._fields_] == ["seed", "stream", "temperature", "top_k", "top_p", "min_p"]
    assert C.sizeof(_lib.QpnRowDraw) == 32 and _lib.QpnRowDraw.stream.offset == 8 and _lib.QpnRowDraw.min_p.offset == 24
    assert "qpn_decode_row_sampling" in {n for n, _, _ in _lib.SYMBOLS}


def test_python_surface_refuses_bad_per_row_values_before_any_device_work():
    """CPU tensors: a call that reached the device layer would raise RuntimeError (no CPU fallback); bad per-row values raise ValueError first."""
    import torch
    from qpnet_amd.qpnet import QPNet
    m = QPNet(**TINY.kwargs())
    args = (torch.zeros(2, 1, dtype=torch.long), torch.zeros(2, 39, 4), [10, 10], np.ones((2, 440)))
    bad = (dict(temperature=[0.7]), dict(top_k=[1, 2, 3]), dict(top_p=[0.9]), dict(min_p=(0.1, 0.1, 0.1)), dict(row_seeds=[1]), dict(row_seeds=[1, 2, 3]),      # wrong lengths
           dict(temperature=[1.0, 0.0]), dict(temperature=[1.0, float("nan")]), dict(top_k=[0, -1]), dict(top_k=[0, TINY.n_quantize + 1]), dict(top_k=[0, 1.5]),
           dict(top_p=[1.0, 0.0]), dict(top_p=[0.5, 1.5]), dict(min_p=[0.0, -0.1]), dict(min_p=[0.0, float("nan")]),                                         # a bad value in row 1 of 2
           dict(mode="argmax", temperature=[1.0, 1.0]), dict(mode="argmax", top_k=[0, 0]), dict(mode="argmax", row_seeds=[1, 2]),                            # argmax draws nothing
           dict(row_seeds=[0, 2 ** 64]), dict(row_seeds=[0, -1]), dict(row_seeds=[0, 1.0]), dict(row_seeds=[0, True]))                                       # a seed outside 64 bits
    for kw in bad:
        with pytest.raises(ValueError):
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(ValueError):
            m.generate_live(*args, **kw)
    with pytest.raises(ValueError, match="3 values for a batch of 2"):          # (a tensor of the wrong length is a wrong length, not "not a number")
        m.batch_fast_generate(*args, top_p=torch.tensor([0.9, 0.9, 0.9]))
    for kw, field in ((dict(temperature=[1.0, 0.0]), "temperature"), (dict(top_k=[0, -1]), "top_k"), (dict(top_p=[0.5, 1.5]), "top_p"), (dict(min_p=[0.0, -0.1]), "min_p"),
                      (dict(row_seeds=[0, 2 ** 64]), "row_seeds")):
        with pytest.raises(ValueError, match=r"row 1: .*%s" % field):             # ... naming the row
            m.batch_fast_generate(*args, **kw)
    good = (dict(temperature=[0.7, 1.0], top_k=(0, 40), top_p=np.array([0.9, 1.0]), min_p=[0.0, 0.05]), dict(row_seeds=[0, 2 ** 64 - 1]),
            dict(temperature=0.7, row_seeds=np.array([3, 4], dtype=np.uint64)), dict(top_k=[5, 6]),
            dict(temperature=torch.tensor([0.7, 1.0]), top_k=torch.tensor([0, 40]), row_seeds=torch.tensor([3, 4])))
    for kw in good:
        with pytest.raises(RuntimeError, match="no CPU fallback"):               # good values go on to the device layer
            m.batch_fast_generate(*args, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate_live(*args, **kw)
    # a batch of one row: its controls stay scalars (a list there is the ValueError it was before rows could differ), row_seeds of one value is fine
    one = (torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 39, 4), [10], np.ones((1, 440)))
    for kw in (dict(temperature=[0.7]), dict(top_k=[5]), dict(top_p=(0.9,)), dict(min_p=[0.1]), dict(min_p=np.array([0.1])), dict(top_k=[5], row_seeds=[3])):
        with pytest.raises(ValueError):
            m.batch_fast_generate(*one, **kw)
        with pytest.raises(ValueError):
            m.generate_live(*one, **kw)
    for kw in (dict(row_seeds=[3]), dict(temperature=0.7, top_k=5, row_seeds=[2 ** 64 - 1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.batch_fast_generate(*one, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.generate_live(*one, **kw)
    with pytest.raises(TypeError):                                               # keyword-only, behind min_p
        m.batch_fast_generate(*args, None, "sampling", False, 1.0, 0, 1.0, 0.0, [1, 2])


def test_row_seed_is_the_sha256_rule():
    ids = ["u00", "SF1_100001", "ファイル_07", "a b/c.d", ""]
    for seed in (0, 1, 100, 2 ** 31):
        for i in ids:
            want = int.from_bytes(hashlib.sha256(("%d:%s" % (seed, i)).encode("utf-8")).digest()[:8], "little")
            got = loaders.row_seed(seed, i)
            assert got == want and isinstance(got, int) and 0 <= got < 2 ** 64
    assert loaders.row_seed(100, "u00") != loaders.row_seed(101, "u00")
    assert len({loaders.row_seed(100, i) for i in ids}) == len(ids)


def test_run_decode_has_the_flag_off_by_default():
    from qpnet_amd import runners
    need = ["--feats", "f", "--stats", "s", "--config", "c", "--outdir", "o", "--checkpoint", "k"]
    assert runners._decode_args().parse_args(need).per_file_seed is False
    assert runners._decode_args().parse_args(need + ["--per_file_seed"]).per_file_seed is True
