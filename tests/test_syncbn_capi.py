"""The cross-rank batch norm's C ABI (mmt_batchnorm_sync_*): declared in include/mmt_hip.h, bound in _lib.EXPORTED,
and every bad argument rejected on the host before any launch (no GPU needed)."""
import os
import re

import pytest

from conftest import ROOT

NAMES = ("mmt_batchnorm_sync_stats", "mmt_batchnorm_sync_apply", "mmt_batchnorm_sync_bwd_sums",
         "mmt_batchnorm_sync_bwd_dx")
EBADARG = -10000
F = 1 << 20  # 16-B aligned, never dereferenced
M, C, P = 800, 96, 96


def test_entry_points_declared_and_exported():
    from mmt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmt_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"^\s*int\s+%s\s*\(" % n, src, flags=re.M), n
        assert n in _lib.EXPORTED and hasattr(_lib.LIB, n), n


def _calls():
    from mmt_amd._lib import LIB
    nws = int(LIB.mmt_batchnorm_ws_floats(M, C))
    assert nws >= 2 * C
    base = {
        "stats": dict(x=F, M=M, C=C, pitch=P, stats=F, ws=F, ws_floats=nws),
        "apply": dict(x=F, y=F, M=M, C=C, pitch=P, gathered=F, W=2, gamma=F, beta=F, rm=F, rv=F, save=F, n_total=F),
        "bwd_sums": dict(x=F, dy=F, M=M, C=C, pitch=P, save=F, dgb=F, sums=F, ws=F, ws_floats=nws),
        "bwd_dx": dict(x=F, dy=F, dx=F, M=M, C=C, pitch=P, gamma=F, save=F, sums=F, n_total=F, ws=F, ws_floats=3 * C),
    }
    fn = {
        "stats": lambda a: LIB.mmt_batchnorm_sync_stats(a["x"], a["M"], a["C"], a["pitch"], a["stats"], a["ws"],
                                                        a["ws_floats"], None),
        "apply": lambda a: LIB.mmt_batchnorm_sync_apply(a["x"], a["y"], a["M"], a["C"], a["pitch"], a["gathered"], a["W"],
                                                        a["gamma"], a["beta"], a["rm"], a["rv"], 0.1, 1e-5, 1, a["save"],
                                                        a["n_total"], None),
        "bwd_sums": lambda a: LIB.mmt_batchnorm_sync_bwd_sums(a["x"], a["dy"], a["M"], a["C"], a["pitch"], a["save"], 1,
                                                              a["dgb"], a["sums"], a["ws"], a["ws_floats"], None),
        "bwd_dx": lambda a: LIB.mmt_batchnorm_sync_bwd_dx(a["x"], a["dy"], a["dx"], a["M"], a["C"], a["pitch"], a["gamma"],
                                                          a["save"], a["sums"], a["n_total"], 1, a["ws"], a["ws_floats"],
                                                          None),
    }
    return base, fn


# (phase, the one argument made bad): every case must be rejected on the host
BAD = [(ph, k, v) for ph in ("stats", "apply", "bwd_sums", "bwd_dx")
       for k, v in (("x", None), ("x", F + 8), ("pitch", 100), ("M", 0), ("C", 0))]
BAD += [("stats", "stats", None), ("stats", "stats", F + 4), ("stats", "ws", None), ("stats", "ws_floats", 2 * C - 1),
        ("apply", "W", 0), ("apply", "W", -1), ("apply", "gathered", None), ("apply", "gathered", F + 4),
        ("apply", "n_total", None), ("apply", "n_total", F + 4), ("apply", "y", None), ("apply", "save", None),
        ("apply", "rv", None),
        ("bwd_sums", "sums", None), ("bwd_sums", "sums", F + 4), ("bwd_sums", "dy", None), ("bwd_sums", "dgb", None),
        ("bwd_sums", "save", None), ("bwd_sums", "ws", None), ("bwd_sums", "ws_floats", 2 * C - 1),
        ("bwd_dx", "sums", None), ("bwd_dx", "sums", F + 4), ("bwd_dx", "n_total", None), ("bwd_dx", "n_total", F + 4),
        ("bwd_dx", "dx", None), ("bwd_dx", "ws", None), ("bwd_dx", "ws_floats", 3 * C - 1)]


@pytest.mark.parametrize("phase,key,value", BAD)
def test_bad_arguments_rejected_without_gpu_work(phase, key, value):
    base, fn = _calls()
    args = dict(base[phase])
    args[key] = value
    assert fn[phase](args) == EBADARG, (phase, key, value)
