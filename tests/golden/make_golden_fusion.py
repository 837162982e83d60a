"""Golden vectors of the other deformable fusion front-ends and of the uni-backbone model, from the
REFERENCE's own Python (CPU), with the stubs, weights and inputs of make_golden.py (imported, not edited).

Run where the reference checkout is (not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fusion.py

Cases (fusion_utils.py:165-353, mixformer_unibackbone.py:434-446):
  asym   + Attention_Fusion_Bimodal / _LNSpecific_Sum / _LNSpecific_2, 2 encoder layers, B = 1
           -> model_asym_fusion_{bimodal,sum,add2}_b1.npz, state_dict_asym_fusion_{...}.json
  rgbt   + Attention_Fusion_Bimodal, 6 layers (the reference config's untouched default), B = 1
           -> model_rgbt_fusion_bimodal6_b1.npz
  uni    (build_mixformer_vit_rgbt_uni, Attention_Fusion_Bimodal_LNSpecific, 2 layers), B = 1, 2
           -> model_uni_b{1,2}.npz, state_dict_uni.json
"""
import json
import os
import sys
import time
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (install_stubs, run_model, sub, synthetic: used as they are)
from make_golden import install_stubs, run_model, sub, synthetic  # noqa: E402,F401

CLASSES = {"bimodal": "Attention_Fusion_Bimodal", "sum": "Attention_Fusion_Bimodal_LNSpecific_Sum",
           "add2": "Attention_Fusion_Bimodal_LNSpecific_2", "lnspecific": "Attention_Fusion_Bimodal_LNSpecific"}
_CASE = {"fusion_class": CLASSES["lnspecific"], "fusion_layers": 2}


def make_cfg(search=320, template=128, fusion_layers=None, vit="base_patch16", hidden=768):
    cfg = _MAKE_CFG(search, template, _CASE["fusion_layers"] if fusion_layers is None else fusion_layers, vit, hidden)
    cfg.MODEL.FUSION_CLASS = _CASE["fusion_class"]
    return cfg


def build(variant, cfg):
    if variant == "uni":
        from lib.models.mixformer_vit_rgbt.mixformer_unibackbone import build_mixformer_vit_rgbt_uni
        return build_mixformer_vit_rgbt_uni(cfg, train=False)
    return _BUILD(variant, cfg)


_MAKE_CFG, _BUILD = mg.make_cfg, mg.build
mg.make_cfg, mg.build = make_cfg, build  # run_model looks both up in its module at call time


def main():
    install_stubs()
    try:
        import einops  # noqa: F401  (mixformer_unibackbone.py:7; only its forward_test uses it)
    except ImportError:
        sys.modules["einops"] = types.ModuleType("einops")
        sys.modules["einops"].rearrange = None
    cases = [("asym", k, 2, 1, "model_asym_fusion_%s_b1.npz" % k, "state_dict_asym_fusion_%s.json" % k)
             for k in ("bimodal", "sum", "add2")]
    cases += [("rgbt", "bimodal", 6, 1, "model_rgbt_fusion_bimodal6_b1.npz", None),
              ("uni", "lnspecific", 2, 1, "model_uni_b1.npz", "state_dict_uni.json"),
              ("uni", "lnspecific", 2, 2, "model_uni_b2.npz", None)]
    for variant, cls, layers, B, npz, js in cases:
        _CASE.update(fusion_class=CLASSES[cls], fusion_layers=layers)
        t0 = time.time()
        res, keys, _ = run_model(variant, B, timing=False)
        np.savez_compressed(os.path.join(HERE, npz), **res)
        if js:
            with open(os.path.join(HERE, js), "w") as f:
                json.dump(keys, f)
        print(variant, cls, layers, B, "boxes", res["pred_boxes"].reshape(-1, 4).tolist(), "%.1fs" % (time.time() - t0),
              flush=True)


if __name__ == "__main__":
    main()
