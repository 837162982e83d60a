"""torch.library registration of the cross-modal MAM attention ops (mmt_amd/ops.py): both exist under torch.ops.mmt
with fake kernels that give the right shapes and dtypes on meta tensors, and the forward carries the registered
autograd formula.  CPU-only: no kernel runs here (GPU: tests/test_gpu_attention_asym_bwd.py)."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import mmt_amd.ops  # noqa: F401  (registers the ops)


@pytest.mark.parametrize("name", ["mam_attention_asym_forward", "mam_attention_asym_backward"])
def test_op_registered(name):
    assert hasattr(torch.ops.mmt, name)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mmt::" + name, "Meta")  # the fake kernel


def test_forward_has_autograd():
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mmt::mam_attention_asym_forward", "Autograd")


def test_fake_shapes_on_meta_tensors():
    q = torch.empty(4, 528, 2304, dtype=torch.bfloat16, device="meta")
    a, lse = torch.ops.mmt.mam_attention_asym_forward(q, 2, 128, 12)
    assert a.shape == (4, 528, 768) and a.dtype == torch.bfloat16 and a.device.type == "meta"
    assert lse.shape == (4, 12, 528) and lse.dtype == torch.float32
    d = torch.ops.mmt.mam_attention_asym_backward(q, a, a, lse, 2, 128, 12)
    assert d.shape == q.shape and d.dtype == torch.bfloat16


def test_fake_shapes_under_fake_tensor_mode():
    with FakeTensorMode():
        q = torch.empty(32, 528, 2304, dtype=torch.bfloat16)
        a, lse = torch.ops.mmt.mam_attention_asym_forward(q, 16, 128, 12)
        assert a.shape == (32, 528, 768) and lse.shape == (32, 12, 528)
        assert torch.ops.mmt.mam_attention_asym_backward(q, a, a, lse, 16, 128, 12).shape == q.shape


def test_wrapper_is_exported():
    from mmt_amd.ops import mam_attention, mam_attention_asym  # noqa: F401
