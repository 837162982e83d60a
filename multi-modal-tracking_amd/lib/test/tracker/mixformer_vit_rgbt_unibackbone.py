"""Drop-in for lib/test/tracker/mixformer_vit_rgbt_unibackbone.py: MixFormer RGB-T tracker (build_mixformer_vit_rgbt_uni, Preprocessor_Multimodal) on the MI355X."""
from lib.models.mixformer_vit_rgbt.mixformer_unibackbone import build_mixformer_vit_rgbt_uni

from ._rgbt import make_batch_tracker_class, make_tracker_class

MixFormer = make_tracker_class(build_mixformer_vit_rgbt_uni, multimodal=True, online_score=False)
BatchMixFormer = make_batch_tracker_class(build_mixformer_vit_rgbt_uni, multimodal=True, online_score=False)


def get_tracker_class():
    return MixFormer


def get_batch_tracker_class():
    """The same tracker for `slots` sequences per step: BatchMixFormer(params, dataset_name, slots)."""
    return BatchMixFormer
