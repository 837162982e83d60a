"""Golden vectors of the concat-conv fusion front-end RGBT_Fusion_Cat (fusion_utils.py:86-110;
experiments/asymmetric_shared/attention_lasher_cat_3layer.yaml), from the REFERENCE's own Python (CPU), with the
stubs, weights and inputs of make_golden.py (imported, not edited).

Run where the reference checkout is (not on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cat.py

Cases:
  asym   + RGBT_Fusion_Cat, B = 1 -> model_asym_fusion_cat_b1.npz, state_dict_asym_fusion_cat.json
  shared + RGBT_Fusion_Cat, B = 2 -> model_shared_fusion_cat_b2.npz
"""
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (install_stubs, run_model: used as they are)
from make_golden import install_stubs, run_model  # noqa: E402


def make_cfg(search=320, template=128, fusion_layers=3, vit="base_patch16", hidden=768):
    cfg = _MAKE_CFG(search, template, fusion_layers, vit, hidden)
    cfg.MODEL.FUSION_CLASS = "RGBT_Fusion_Cat"
    return cfg


_MAKE_CFG = mg.make_cfg
mg.make_cfg = make_cfg  # run_model looks it up in its module at call time


def main():
    install_stubs()
    cases = [("asym", 1, "model_asym_fusion_cat_b1.npz", "state_dict_asym_fusion_cat.json"),
             ("shared", 2, "model_shared_fusion_cat_b2.npz", None)]
    for variant, B, npz, js in cases:
        t0 = time.time()
        res, keys, _ = run_model(variant, B, timing=False)
        np.savez_compressed(os.path.join(HERE, npz), **res)
        if js:
            with open(os.path.join(HERE, js), "w") as f:
                json.dump(keys, f)
        print(variant, B, "boxes", res["pred_boxes"].reshape(-1, 4).tolist(), "%.1fs" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
