"""Drop-in for lib/test/tracker/asymmetric_shared_ce.py: MixFormer RGB-T tracker with candidate elimination
(build_asymmetric_shared_ce, Preprocessor_Multimodal) on the MI355X.  By default every frame runs the full
forward; params.kv_cache = True runs the template pass once per template update and a pruning search pass per
frame (the elimination needs the template rows' Q, which the whole-batch cache keeps).  The batched tracker's
params.slot_cache stays refused for this model."""
from lib.models.mixformer_vit_rgbt.asymmetric_shared_ce import build_asymmetric_shared_ce

from ._rgbt import make_batch_tracker_class, make_tracker_class

MixFormer = make_tracker_class(build_asymmetric_shared_ce, multimodal=True, online_score=False, kv_cache=False)
BatchMixFormer = make_batch_tracker_class(build_asymmetric_shared_ce, multimodal=True, online_score=False)


def get_tracker_class():
    return MixFormer


def get_batch_tracker_class():
    """The same tracker for `slots` sequences per step: BatchMixFormer(params, dataset_name, slots)."""
    return BatchMixFormer
