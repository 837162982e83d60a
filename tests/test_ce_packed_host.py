"""Host side of mmt_ce_rows_gather_cast, the packed typed row gather of the template-cached candidate
elimination (no GPU): the export and header declaration, and the argument checks, which return
MMT_EBADARG before anything is launched (the pointers here are never dereferenced)."""
import ctypes
import os

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mmt_hip.h")
EBADARG = -10000
F32, BF16, F64, F16 = 0, 1, 2, 3


def test_rows_gather_cast_exported_and_declared():
    from mmt_amd import _lib
    assert "mmt_ce_rows_gather_cast" in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mmt_ce_rows_gather_cast")
    assert "int mmt_ce_rows_gather_cast(" in open(HEADER).read()


def _call(**kw):
    from mmt_amd._lib import LIB
    fake = 1 << 20
    a = dict(src=fake, src_rows=9, dst=2 * fake, dst_t=3 * fake, dst_rows=7, idx=4 * fake, idx_pitch=0, S=4, C=768,
             dtype=BF16)
    a.update(kw)
    return LIB.mmt_ce_rows_gather_cast(a["src"], a["src_rows"], a["dst"], a["dst_t"], a["dst_rows"], a["idx"],
                                       a["idx_pitch"], a["S"], a["C"], a["dtype"], None)


@pytest.mark.parametrize("bad", [
    dict(src=None), dict(idx=None),
    dict(dst=None, dst_t=None),                       # no output
    dict(dst=1 << 20), dict(dst_t=1 << 20),           # source equal to an output
    dict(dst=3 << 20),                                # the two outputs equal
    dict(C=770), dict(C=1028), dict(C=0), dict(C=-4),  # C % 4, C > 1024, non-positive
    dict(dtype=F64), dict(dtype=7), dict(dtype=-1),   # unknown dtype of the typed output
    dict(src_rows=0), dict(src_rows=-3), dict(dst_rows=0), dict(dst_rows=-1), dict(S=0), dict(S=-2), dict(S=65536),
    dict(idx_pitch=6), dict(idx_pitch=-1),            # index rows shorter than a destination row
])
def test_rows_gather_cast_rejects_bad_arguments_before_any_launch(bad):
    assert _call(**bad) == EBADARG
