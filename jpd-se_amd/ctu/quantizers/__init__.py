"""Quantizers of the reference's `ctu.quantizers` that run on the HIP kernels: the soft-to-hard vector quantizer and its
residual (multi-stage) form.  (The binarizer lives inside the encoder, jpdse_hip.layers.HipBinarizer.)"""
from .s2h_vq import *  # noqa: F401,F403
from .residual_s2h_vq import *  # noqa: F401,F403
