"""RGBT_Fusion_Cat (fusion_utils.py:86-110), the concat-conv fusion front-end of the shared-backbone models, on
the CPU: builders and state_dict contract, the BatchNorm fold, and the C ABI's answers for the split-input conv mode
(mmt_gemm_params.a1 / k_split with conv_h > 0) as far as they need no device.  Goldens:
tests/golden/make_golden_cat.py (the reference's own forward)."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

import fusion_cat_probes as P

CAT = "RGBT_Fusion_Cat"
STACKED = ["shared", "uni", "asym", "asym_online", "asym_ce"]


def _synth(keys):
    from mmt_amd import synthetic
    return {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}


# ----------------------------------------------------------------------------- builders, state dict
@pytest.mark.parametrize("variant", STACKED)
def test_stacked_builders_take_cat(variant):
    from mmt_amd import model as M
    with torch.device("meta"):
        m = M.BUILDERS[variant](M.hot_path_cfg(fusion_class=CAT, fusion_layers=3), train=False)
    assert type(m.fusion_vi).__name__ == CAT and m.variant == variant
    assert M.BUILDERS[variant].__name__ in M.CAT_BUILDERS


def test_state_dict_contract_and_strict_load():
    from mmt_amd.model import build_asymmetric_shared, hot_path_cfg, reference_state_dict_shapes
    ref = [(k, list(s)) for k, s in json.load(open(GOLDEN + "/state_dict_asym_fusion_cat.json"))]
    assert reference_state_dict_shapes("asym", fusion_class=CAT) == ref
    fus = dict((k, s) for k, s in ref if k.startswith("fusion_vi."))
    assert fus["fusion_vi.fusion1.weight"] == [1536, 1536, 3, 3]
    assert fus["fusion_vi.fusion2.weight"] == [768, 1536, 3, 3] and fus["fusion_vi.fusion3.weight"] == [768, 768, 3, 3]
    assert fus["fusion_vi.fusion1_bn.num_batches_tracked"] == [] and fus["fusion_vi.fusion1_bn.running_var"] == [1536]
    assert len(fus) == 3 * 6
    model = build_asymmetric_shared(hot_path_cfg(fusion_class=CAT), train=False)
    res = model.load_state_dict(_synth(ref), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_vit_large_shapes_follow_hidden_dim():
    """Reference defect D1 (the builders pass a hard-coded 768) parametrised: ViT-L builds at 2048 / 1024."""
    from mmt_amd.model import reference_state_dict_shapes
    ks = dict(reference_state_dict_shapes("asym", hidden=1024, search=384, template=192, fusion_class=CAT))
    assert ks["fusion_vi.fusion1.weight"] == [2048, 2048, 3, 3]
    assert ks["fusion_vi.fusion2.weight"] == [1024, 2048, 3, 3]
    assert ks["fusion_vi.fusion3.weight"] == [1024, 1024, 3, 3]
    assert ks["fusion_vi.fusion1_bn.weight"] == [2048] and ks["fusion_vi.fusion3_bn.running_mean"] == [1024]


def test_two_stream_builder_still_refuses_and_names_a_builder():
    from mmt_amd.model import build_mixformer_vit_rgbt, hot_path_cfg
    with pytest.raises(NotImplementedError, match="build_asymmetric_shared"):
        build_mixformer_vit_rgbt(hot_path_cfg(fusion_class=CAT), train=False)


def test_refused_classes_message_still_lists_the_accepted_names():
    from mmt_amd.model import build_asymmetric_shared, hot_path_cfg
    with pytest.raises(NotImplementedError, match="Attention_Fusion_Bimodal_LNSpecific_Sum.*RGBT_Fusion_Cat"):
        build_asymmetric_shared(hot_path_cfg(fusion_class="RGBT_Fusion_1"), train=False)


@pytest.mark.parametrize("module,builder", [("mixformer_vit_rgbt_shared", "build_mixformer_vit_rgbt_shared"),
                                            ("mixformer_vit_rgbt_unibackbone", "build_mixformer_vit_rgbt_uni"),
                                            ("asymmetric_shared", "build_asymmetric_shared"),
                                            ("asymmetric_shared_online", "build_asymmetric_shared_online_score"),
                                            ("asymmetric_shared_ce", "build_asymmetric_shared_ce")])
def test_tracker_modules_build_cat_through_their_builder(module, builder):
    """The lib/ overlay's tracker modules import the builders that take the cfg: nothing in them names a fusion."""
    import importlib

    from mmt_amd import model as M
    mod = importlib.import_module("lib.test.tracker.%s" % module)
    assert getattr(mod, builder) is getattr(M, builder)
    with torch.device("meta"):
        net = getattr(mod, builder)(M.hot_path_cfg(fusion_class=CAT), train=False)
    assert type(net.fusion_vi).__name__ == CAT
    assert mod.get_tracker_class().__name__ == "MixFormer"


def test_param_groups_cat_at_fusion_lr():
    from mmt_amd import model as M
    from mmt_amd.train import param_groups
    with torch.device("meta"):
        net = M.build_asymmetric_shared(M.hot_path_cfg(fusion_class=CAT), train=False)
    groups = param_groups(net, 1e-4)
    fus = {id(p) for n, p in net.named_parameters() if n.startswith("fusion_vi.")}
    assert len(fus) == 9  # three conv weights, three (gamma, beta)
    at_one = [g for g in groups if "lr" not in g]
    assert len(at_one) == 1 and {id(p) for p in at_one[0]["params"]} == fus
    assert not any(id(p) in fus for g in groups if "lr" in g for p in g["params"])


def test_sync_batchnorm_conversion_keeps_the_hip_route():
    """Under ddp=True the net goes through convert_sync_batchnorm: the three Cat norms become SyncBatchNorm and pass
    the test the head's 22 pass (train._hip_bn_ok), so they take ops.bn_relu / sync_batchnorm_relu as those do."""
    from mmt_amd import model as M
    from mmt_amd.train import _hip_bn_ok
    with torch.device("meta"):
        net = M.build_asymmetric_shared(M.hot_path_cfg(fusion_class=CAT), train=False)
    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net).train()
    cat = [getattr(net.fusion_vi, "fusion%d_bn" % i) for i in (1, 2, 3)]
    head = [m for m in net.box_head.modules() if isinstance(m, torch.nn.SyncBatchNorm)]
    assert all(type(m) is torch.nn.SyncBatchNorm for m in cat) and len(head) == 22
    assert all(_hip_bn_ok(m) for m in cat + head)
    assert [m.num_features for m in cat] == [1536, 768, 768]


# ----------------------------------------------------------------------------- BatchNorm fold
def test_bn_fold_equals_batchnorm_of_conv_fp64():
    """runtime._fold on the Cat key names (conv without bias): conv(x, W') + b' == batch_norm(conv(x, W)) in eval,
    fp64, 2 images of 4 x 4; W' comes back in the head convs' operand layout [cout][(ky, kx, cin)]."""
    from mmt_amd.runtime import MixFormerRGBTRuntime
    g = torch.Generator().manual_seed(3)
    cin, cout = 16, 8
    sd = {"fusion_vi.fusion2.weight": torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64),
          "fusion_vi.fusion2_bn.weight": 1 + 0.3 * torch.randn(cout, generator=g, dtype=torch.float64),
          "fusion_vi.fusion2_bn.bias": torch.randn(cout, generator=g, dtype=torch.float64),
          "fusion_vi.fusion2_bn.running_mean": torch.randn(cout, generator=g, dtype=torch.float64),
          "fusion_vi.fusion2_bn.running_var": 0.5 + torch.rand(cout, generator=g, dtype=torch.float64),
          "fusion_vi.fusion2_bn.num_batches_tracked": torch.tensor(7)}
    w, b = MixFormerRGBTRuntime._fold(None, sd, "fusion_vi.fusion2", conv="", bn="_bn")
    assert tuple(w.shape) == (cout, 9 * cin) and tuple(b.shape) == (cout,)
    x = torch.randn(2, cin, 4, 4, generator=g, dtype=torch.float64)
    ref = F.batch_norm(F.conv2d(x, sd["fusion_vi.fusion2.weight"], padding=1), sd["fusion_vi.fusion2_bn.running_mean"],
                       sd["fusion_vi.fusion2_bn.running_var"], sd["fusion_vi.fusion2_bn.weight"],
                       sd["fusion_vi.fusion2_bn.bias"], False, 0.0, 1e-5)
    got = F.conv2d(x, w.view(cout, 3, 3, cin).permute(0, 3, 1, 2), b, padding=1)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_training_forward_aten_route_equals_the_module_chain():
    """fusion_forward without HIP ops (the CPU stand-ins' route) is the reference's own module chain."""
    from mmt_amd.model import RGBT_Fusion_Cat
    from mmt_amd.train import fusion_forward
    torch.manual_seed(0)
    fu = RGBT_Fusion_Cat(8).train()
    sv, si = torch.randn(2, 8, 4, 4), torch.randn(2, 8, 4, 4)
    ref_mod = RGBT_Fusion_Cat(8).train()
    ref_mod.load_state_dict(fu.state_dict())
    x = torch.cat([sv, si], 1)
    for i in (1, 2, 3):
        x = F.relu(getattr(ref_mod, "fusion%d_bn" % i)(getattr(ref_mod, "fusion%d" % i)(x)))
    got = fusion_forward(fu, sv, si, None)
    assert torch.equal(got, x) and tuple(got.shape) == (2, 8, 4, 4)
    assert int(fu.fusion3_bn.num_batches_tracked) == 1


# ----------------------------------------------------------------------------- C ABI, no device
def test_select_answers_a_kernel_the_c_abi_accepts():
    """Every probe shape: mmt_gemm_select names a kernel; a split on the LDS-DMA K step (64) goes to the LDS-DMA
    kernel for 16-bit operands, a split off it and every fp32 launch to the register-staged one; forcing that
    answer through `impl` is accepted and answers the same kernel."""
    L = P._lib()
    for dname in P.DT:
        for h, pitched, ks, c1, N in P.shapes():
            s = P.Spec(h, ks, c1, N, dtype=dname, pitched=pitched)
            k = P.kernel_of(s)
            assert k is not None, s
            if dname == "f32" or ks % 64:
                assert k == ("reg",), (s, k)
            else:
                assert k[0] == "glds", (s, k)
            forced = s.but(impl=-1 if k == ("reg",) else k[1])
            assert P.kernel_of(forced) == k, (forced, P.kernel_of(forced))
            c = P.select(s)
            assert c.conv == 1 and c.family in (L.GEMM_REG_TILE, L.GEMM_LDS_DMA)


def test_lds_dma_declines_a_split_off_its_k_step():
    s = P.Spec(5, 72, 56, 72)
    assert P.kernel_of(s) == ("reg",)
    for impl in (1, 2, 3, 4):
        assert P.kernel_of(s.but(impl=impl)) == ("reg",)  # the launch follows the answer: never the LDS-DMA kernel
    assert P.kernel_of(s.but(split=False))[0] == "glds"  # the same conv on one map is its shape


def test_k_split_zero_is_todays_answer():
    """k_split == 0 with a1 set or not: the same choice, field by field, as before the split existed."""
    for dname in P.DT:
        s = P.Spec(5, 64, 64, 72, dtype=dname, split=False)
        a, b = P.select(s), P.select(s, a1=P._FAKE)
        assert a is not None and bytes(a) == bytes(b)


@pytest.mark.parametrize("name", list(P.bad_specs()))
@pytest.mark.parametrize("dname", list(P.DT))
def test_unbuilt_split_combinations_are_ebadarg(name, dname):
    """mmt_gemm_select and mmt_gemm itself (the checks run before anything is launched, so no device is touched)
    answer MMT_EBADARG; the same launch without the split is accepted, so the split is what is refused."""
    L = P._lib()
    s, over = P.bad_specs()[name]
    s = s.but(dtype=dname)
    assert P.select(s, **over) is None
    p = P.params_of(s, **over)
    assert L.LIB.mmt_gemm(ctypes.byref(p), P.dtype_code(dname), None) == P.EBADARG
    assert P.select(s.but(split=False)) is not None
