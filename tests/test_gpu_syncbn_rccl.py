"""The cross-rank batch norm of the corner head over a real RCCL process group on the GPU: a fresh child process with
a one-rank "nccl" group runs the SyncBatchNorm head with the collectives forced on, eagerly and captured as one
hipGraph, against the local HIP batch norm (tests/syncbn_nccl_child.py holds the checks)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_sync_batchnorm_head_over_rccl_eager_and_captured(tmp_path):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = tmp_path / "syncbn.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    child = os.path.join(os.path.dirname(__file__), "syncbn_nccl_child.py")
    r = subprocess.run([sys.executable, "-u", child, str(out)], env=env, capture_output=True, text=True, timeout=60)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(out.read_text())
    print(json.dumps(rec))
    assert rec["ok"] and rec["backend"] == "nccl" and rec["sync_bn_modules"] == 22
    assert rec["captured_collectives"] == {"gather": 22, "reduce": 22}
