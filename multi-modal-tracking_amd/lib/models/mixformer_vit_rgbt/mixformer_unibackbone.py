"""Drop-in for lib/models/mixformer_vit_rgbt/mixformer_unibackbone.py (one plain ViT over both modalities)."""
from mmt_amd.model import MixFormer_RGBT_Uni as MixFormer_RGBT, build_mixformer_vit_rgbt_uni  # noqa: F401
