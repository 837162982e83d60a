"""Drop-in boundary (CPU): builders, state_dict key names/shapes identical to the reference's
(recorded from the reference itself in tests/golden/state_dict_*.json), config handling, and the
loud failure when no HIP device is present."""
import json

import pytest
import torch

from conftest import GOLDEN


@pytest.mark.parametrize("variant", ["rgbt", "shared", "asym", "asym_online", "asym_ce", "rgb"])
def test_state_dict_keys_match_reference(variant):
    """rgb: the RGB-only MixFormer of BASELINE config 1 (lib/models/mixformer_vit, 128/288)."""
    from mmt_amd.model import reference_state_dict_shapes
    ref = json.load(open(GOLDEN + "/state_dict_%s.json" % variant))
    ours = reference_state_dict_shapes(variant, search=288 if variant == "rgb" else 320)
    assert [k for k, _ in ours] == [k for k, _ in ref]
    assert dict(ours) == {k: s for k, s in ref}


def test_strict_load_of_reference_shaped_state_dict():
    from mmt_amd import synthetic
    from mmt_amd.model import build_mixformer_vit_rgbt, hot_path_cfg
    keys = json.load(open(GOLDEN + "/state_dict_rgbt.json"))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    m = build_mixformer_vit_rgbt(hot_path_cfg(), train=False)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert m.compute_dtype in (torch.bfloat16, torch.float32)


def test_lib_package_shim_exports_builders():
    from lib.models.mixformer_vit_rgbt import build_mixformer_vit_rgbt, build_mixformer_vit_rgbt_shared  # noqa: F401
    from lib.models.mixformer_vit_rgbt.asymmetric_shared import build_asymmetric_shared  # noqa: F401
    from lib.models.mixformer_vit_rgbt.asymmetric_shared_online import build_asymmetric_shared_online_score  # noqa: F401
    from lib.models.mixformer_vit_rgbt.asymmetric_shared_ce import build_asymmetric_shared_ce
    from lib.models.mixformer_vit import build_mixformer_vit  # noqa: F401
    from lib.models.mixformer_vit.mixformer import MixFormer  # noqa: F401


def test_ce_builder_reads_reference_config():
    """MODEL.BACKBONE.CE_LOC / CE_KEEP_RATIO (lib/config/asymmetric_shared_ce/config.py:23-24)."""
    from mmt_amd.model import build_asymmetric_shared_ce, hot_path_cfg
    cfg = hot_path_cfg()
    m = build_asymmetric_shared_ce(cfg, train=False)
    assert m.ce_loc == (3, 6, 9) and m.ce_keep_ratio == (0.7, 0.7, 0.7)
    cfg.MODEL.BACKBONE.CE_LOC = [2, 5]
    cfg.MODEL.BACKBONE.CE_KEEP_RATIO = [0.5, 0.8]
    m = build_asymmetric_shared_ce(cfg, train=False)
    assert m.ce_loc == (2, 5) and m.ce_keep_ratio == (0.5, 0.8)


def test_forward_refuses_cpu_inputs():
    from mmt_amd.model import build_asymmetric_shared, hot_path_cfg
    m = build_asymmetric_shared(hot_path_cfg(), train=False).eval()
    t = [torch.zeros(1, 3, 128, 128)] * 2
    s = [torch.zeros(1, 3, 320, 320)] * 2
    with pytest.raises(RuntimeError, match="HIP device"):
        m(t, t, s)


def test_unsupported_fusion_class_raises():
    from mmt_amd.model import build_mixformer_vit_rgbt, hot_path_cfg
    cfg = hot_path_cfg()
    cfg.MODEL.FUSION_CLASS = "RGBT_Fusion_Cat"
    with pytest.raises(NotImplementedError):
        build_mixformer_vit_rgbt(cfg, train=False)
    cfg = hot_path_cfg()
    cfg.MODEL.VIT_TYPE = "tiny"
    with pytest.raises(KeyError):
        build_mixformer_vit_rgbt(cfg, train=False)


def test_vit_large_builds_with_hidden_width():
    """Reference defect D1 (fusion width hard-coded 768) is parametrised: ViT-L 192/384 builds."""
    from mmt_amd.model import reference_state_dict_shapes
    ks = dict(reference_state_dict_shapes("asym_online", hidden=1024, search=384, template=192))
    assert ks["fusion_vi.adjust_v.0.weight"] == [512, 1024, 1, 1]
    assert ks["backbone.pos_embed_s"] == [1, 576, 1024]
    assert ks["score_branch.score_token"] == [1, 1, 1024]


def test_config_yaml_overlay(tmp_path):
    from mmt_amd.config import default_cfg, update_config_from_file
    y = tmp_path / "exp.yaml"
    y.write_text("MODEL:\n  HEAD_TYPE: CORNER_UP\n  FUSION_LAYERS: 2\nTEST:\n  SEARCH_SIZE: 320\n  UPDATE_INTERVALS:\n    LASOT: [100]\n")
    cfg = update_config_from_file(default_cfg(), str(y))
    assert cfg.MODEL.HEAD_TYPE == "CORNER_UP" and cfg.MODEL.FUSION_LAYERS == 2
    assert cfg.TEST.SEARCH_SIZE == 320 and cfg.TEST.UPDATE_INTERVALS.LASOT == [100]
    assert cfg.MODEL.VIT_TYPE == "base_patch16"
    assert not hasattr(cfg.TEST.UPDATE_INTERVALS, "RGBT234")


def test_synthetic_weights_are_deterministic():
    from mmt_amd import synthetic
    a = synthetic.uniform("x.weight", (4, 3))
    b = synthetic.uniform("x.weight", (4, 3))
    assert (a == b).all() and a.min() >= -1 and a.max() < 1
    assert not (synthetic.uniform("y.weight", (4, 3)) == a).all()
    # pinned values: the generator must not drift between rounds / machines
    assert abs(float(synthetic.uniform("backbone.blocks.0.attn.qkv.weight", (3,))[0]) - float(
        synthetic.uniform("backbone.blocks.0.attn.qkv.weight", (5,))[0])) == 0.0


def test_ce_template_mask_validation():
    """ce_template_mask (generate_mask_cond, lib/utils/ce_utils.py:14-38) is validated on the host before
    any device work: wrong shape or unequal per-frame counts raise ValueError (the reference views
    attn[mask] as (bs, heads, -1, L)); a valid CTR_POINT mask reaches the device check (no CPU path)."""
    import pytest
    import torch
    from mmt_amd import model as M
    net = M.build_asymmetric_shared_ce(M.hot_path_cfg(), train=False).eval()
    x = [torch.zeros(2, 3, 128, 128)] * 2
    s = [torch.zeros(2, 3, 320, 320)] * 2
    mask = torch.zeros(2, 256, dtype=torch.bool)
    mask[:, [27, 91, 155, 219]] = True  # CTR_POINT: centre token of each 8x8 template
    with pytest.raises(ValueError):
        net(x, x, s, ce_template_mask=mask[:, :128])
    bad = mask.clone()
    bad[1, 0] = True
    with pytest.raises(ValueError):
        net(x, x, s, ce_template_mask=bad)
    with pytest.raises(RuntimeError):
        net(x, x, s, ce_template_mask=mask, ce_keep_rate=0.7)


def test_rgb_only_refuses_bf16():
    """The RGB-only MixFormer (config 1) has no fusion between backbone and corner head, so the bf16
    backbone's token error moves its boxes past the north star's 1e-2 (1.8e-2 with the head in fp32,
    profiles/r03_rgb_dtype.jsonl): bf16 is refused on the host with an explicit error; the module's
    16-bit default is fp16."""
    from mmt_amd import model as M
    from mmt_amd import synthetic
    from mmt_amd.runtime import MixFormerRGBTRuntime
    keys = json.load(open(GOLDEN + "/state_dict_rgb.json"))
    sd = {k: torch.from_numpy(v) for k, v in synthetic.synth_state_dict(keys).items()}
    with pytest.raises(ValueError, match="bf16"):
        MixFormerRGBTRuntime(sd, "rgb", dtype=torch.bfloat16, device="cpu")
    net = M.build_mixformer_vit(M.hot_path_cfg(search=288), train=False)
    assert net.compute_dtype == torch.float16


_OVERLAY_PROBE = r'''
import importlib, importlib.machinery, json, sys
ours, ref = sys.argv[1], sys.argv[2]
sys.path[:] = [ours] + [p for p in sys.path if p not in ("", ours, ref)] + [ref]

OURS_PKGS = ("lib", "lib.test", "lib.test.tracker", "lib.models", "lib.models.mixformer_vit_rgbt",
             "lib.models.mixformer_vit")


def origin(name):
    """Where `name` resolves, without executing any module outside this repo: our overlay packages
    are imported (their __init__ merges __path__); below a reference-only package the child spec is
    looked up on the parent's search locations (importlib.machinery.PathFinder), not imported."""
    parent, _, leaf = name.rpartition(".")
    if not parent:
        return importlib.util.find_spec(name).origin
    if parent in OURS_PKGS:
        importlib.import_module(parent)
        return importlib.util.find_spec(name).origin
    locs = [locate(parent)]
    spec = importlib.machinery.PathFinder.find_spec(leaf, locs[0])
    return None if spec is None else spec.origin


def locate(pkg):
    parent, _, leaf = pkg.rpartition(".")
    if parent in OURS_PKGS or not parent:
        mod = importlib.import_module(parent) if parent else None
        spec = importlib.util.find_spec(pkg)
    else:
        spec = importlib.machinery.PathFinder.find_spec(leaf, locate(parent))
    return list(spec.submodule_search_locations)


names = sys.argv[3:]
print(json.dumps({n: origin(n) for n in names}))
'''


# Files of the reference checkout's lib/ that the overlay test resolves (names only; packages by their
# __init__.py -- lib/config/mixformer_vit_rgbt has none in the reference and is a namespace package).
_REFERENCE_LAYOUT = [
    "lib/__init__.py",
    "lib/config/__init__.py", "lib/config/mixformer_vit_rgbt/config.py",
    "lib/models/__init__.py",
    "lib/models/mixformer_cvt/__init__.py", "lib/models/mixformer_cvt/head.py",
    "lib/models/mixformer_vit/__init__.py", "lib/models/mixformer_vit/mixformer.py",
    "lib/models/mixformer_vit/mixformer_online.py",
    "lib/models/mixformer_vit_rgbt/__init__.py", "lib/models/mixformer_vit_rgbt/mixformer.py",
    "lib/models/mixformer_vit_rgbt/mixformer_shared.py", "lib/models/mixformer_vit_rgbt/asymmetric_shared.py",
    "lib/models/mixformer_vit_rgbt/asymmetric_shared_online.py",
    "lib/models/mixformer_vit_rgbt/asymmetric_shared_ce.py", "lib/models/mixformer_vit_rgbt/fusion_utils.py",
    "lib/test/__init__.py",
    "lib/test/evaluation/__init__.py", "lib/test/evaluation/tracker_rgbt.py", "lib/test/evaluation/running.py",
    "lib/test/parameter/__init__.py", "lib/test/parameter/mixformer_vit_rgbt.py",
    "lib/test/tracker/__init__.py", "lib/test/tracker/basetracker.py", "lib/test/tracker/tracker_utils.py",
    "lib/test/tracker/mixformer_vit.py", "lib/test/tracker/mixformer_vit_rgbt.py",
    "lib/test/tracker/mixformer_vit_rgbt_shared.py", "lib/test/tracker/asymmetric_shared.py",
    "lib/test/tracker/asymmetric_shared_online.py", "lib/test/tracker/asymmetric_shared_ce.py",
    "lib/test/utils/__init__.py",
    "lib/train/__init__.py", "lib/train/data/__init__.py", "lib/train/data/processing_utils.py",
    "lib/utils/__init__.py", "lib/utils/box_ops.py", "lib/utils/ce_utils.py",
]


def test_lib_overlays_reference_package(tmp_path):
    """with this tree first on sys.path and the reference checkout after it (what
    `PYTHONPATH=<this>/multi-modal-tracking_amd python tracking/test.py ...` gives, test.py:10-12
    appending the project root), the reference harness's own modules resolve to the reference
    (tracking/test.py:14-16, tracker_rgbt.py:92-97 / 189-196, parameter/mixformer_vit_rgbt.py:1-4,
    tracker/mixformer_vit_rgbt.py:3,9,10) and the hot-path model and tracker modules to this repo.
    Only spec lookups: no reference module is executed, so the reference checkout is stood in for by
    a tree of empty files with the reference's layout (_REFERENCE_LAYOUT), which holds every module
    looked up here, the ones this repo overlays included."""
    import os
    import subprocess
    import sys
    ref = str(tmp_path / "reference")
    for rel in _REFERENCE_LAYOUT:
        path = os.path.join(ref, *rel.split("/"))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "w").close()
    ours = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modal-tracking_amd")
    from_ref = ["lib.test.evaluation", "lib.test.evaluation.tracker_rgbt", "lib.test.evaluation.running",
                "lib.test.parameter.mixformer_vit_rgbt", "lib.test.utils", "lib.config.mixformer_vit_rgbt.config",
                "lib.train.data.processing_utils", "lib.utils.box_ops", "lib.utils.ce_utils",
                "lib.test.tracker.tracker_utils", "lib.test.tracker.basetracker", "lib.test.tracker.mixformer_vit",
                "lib.models.mixformer_cvt.head", "lib.models.mixformer_vit_rgbt.fusion_utils",
                "lib.models.mixformer_vit.mixformer_online"]
    from_ours = ["lib.models.mixformer_vit_rgbt", "lib.models.mixformer_vit_rgbt.mixformer",
                 "lib.models.mixformer_vit_rgbt.asymmetric_shared_online", "lib.models.mixformer_vit",
                 "lib.test.tracker.mixformer_vit_rgbt", "lib.test.tracker.mixformer_vit_rgbt_shared",
                 "lib.test.tracker.asymmetric_shared", "lib.test.tracker.asymmetric_shared_online",
                 "lib.test.tracker.asymmetric_shared_ce"]
    probe = tmp_path / "probe.py"
    probe.write_text(_OVERLAY_PROBE)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH="")
    out = subprocess.run([sys.executable, str(probe), ours, ref] + from_ref + from_ours, env=env,
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for n in from_ref:
        assert got[n] and got[n].startswith(ref + "/"), (n, got[n])
    for n in from_ours:
        assert got[n] and got[n].startswith(ours + "/"), (n, got[n])


def test_lib_overlay_standalone_without_reference(tmp_path):
    """Without the reference on sys.path (the GPU box), the overlay packages still import and the
    tracker modules take the local BaseTracker."""
    import os
    import subprocess
    import sys
    ours = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modal-tracking_amd")
    code = ("import sys; sys.path[:] = [sys.argv[1]] + [p for p in sys.path if p and 'reference' not in p]\n"
            "import importlib.util as u, lib.test.tracker as t\n"
            "assert u.find_spec('lib.test.evaluation') is None and u.find_spec('lib.config') is None\n"
            "assert len(t.__path__) == 1\n"
            "from lib.test.tracker._basetracker import BaseTracker\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH="")
    out = subprocess.run([sys.executable, "-c", code, ours], env=env, capture_output=True, text=True,
                         timeout=120, cwd=str(tmp_path))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr
