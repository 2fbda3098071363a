"""The DVAE's encoder half: audio features to mel codes (indextts/vqvae/dvae.py)."""
from indextts.vqvae.dvae import CodecEngine, code_count, encoder_forward, nearest_code  # noqa: F401
