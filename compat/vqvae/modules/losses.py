"""vqvae.modules.losses (reference: vqvae/modules/losses.py) -> detail_tts_amd.vqvae.modules.losses"""
from detail_tts_amd.vqvae.modules.losses import discriminator_loss, feature_loss, generator_loss, kl_loss  # noqa: F401
