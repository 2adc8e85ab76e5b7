"""A small stand-in for the reference's ``SpatialEncoder`` with a trunk of plain ``torch.nn`` modules (torchvision is not needed), on top
of :mod:`synthetic.model_stub`'s ``PixelNeRFState``: the attribute surface ``diner_amd.glue.encode`` reads -- ``image_padding``,
``padding_pe``, ``feature_padding``, ``num_layers``, ``use_first_pool``, ``upsample_interp``, ``index_interp`` / ``index_padding`` and
``model`` with ``conv1``, ``bn1``, ``relu``, ``maxpool``, ``layer1..layer4`` (reference src/models/image_encoder.py:19-95).  The trunk has
the ResNet's strides (conv1 2, maxpool 2, layers 1 / 2 / 2 / 2) and few channels: 16 | 16 / 24 / 32 / 40.
"""
from __future__ import annotations

import torch
from torch import nn

from .model_stub import PixelNeRFState

CHANNELS = (16, 16, 24, 32, 40)     # conv1, layer1..layer4


def _layer(c_in, c_out, stride):
    return nn.Sequential(nn.Conv2d(c_in, c_out, 3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(c_out), nn.ReLU())


class TrunkStub(nn.Module):
    def __init__(self, c_in):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, CHANNELS[0], 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(CHANNELS[0])
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = _layer(CHANNELS[0], CHANNELS[1], 1)
        self.layer2 = _layer(CHANNELS[1], CHANNELS[2], 2)
        self.layer3 = _layer(CHANNELS[2], CHANNELS[3], 2)
        self.layer4 = _layer(CHANNELS[3], CHANNELS[4], 2)


class SpatialEncoderStub(nn.Module):
    def __init__(self, num_layers=4, image_padding=8, padding_pe=4, use_first_pool=True, upsample_interp="bilinear",
                 index_interp="bilinear", index_padding="border"):
        super().__init__()
        self.num_layers, self.image_padding, self.padding_pe = num_layers, image_padding, padding_pe
        self.use_first_pool, self.upsample_interp = use_first_pool, upsample_interp
        self.index_interp, self.index_padding = index_interp, index_padding
        self.feature_padding = image_padding / 2          # image_padding / conv1.stride (image_encoder.py:58)
        assert self.feature_padding % 1 == 0
        pe_on = padding_pe >= 0 and self.feature_padding > 0
        self.model = TrunkStub(3 + (2 * (1 + 2 * padding_pe) if pe_on else 0))
        self.latent_size = sum(CHANNELS[:num_layers])
        self.latent = self.depths = self.depths_std = self.normals = None
        self.nviews = self.nobjects = None


def encoder_model(weights=None, device="cuda", seed=0, num_freqs=6, d_hidden=64, n_blocks=3, combine_layer=2, **encoder_kw):
    """``PixelNeRFState`` whose encoder is a :class:`SpatialEncoderStub` (``encoder_kw``) and whose fusion MLP takes that encoder's latent
    size; ``weights``: a ``synth.make_mlp_weights`` dict for the MLP (default: drawn here with ``seed``).  Nothing is encoded yet."""
    from . import synth
    torch.manual_seed(seed)
    enc = SpatialEncoderStub(**encoder_kw)
    dims = dict(d_latent=enc.latent_size, d_hidden=d_hidden, n_blocks=n_blocks, combine_layer=combine_layer)
    m = PixelNeRFState(feature_padding=enc.feature_padding, num_freqs=num_freqs, **dims)
    m.encoder = enc
    if weights is None:
        weights = synth.make_mlp_weights(seed + 1, bias_scale=0.1, **dims)
    m.mlp_fine.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()}, strict=True)
    return m.to(device)
