"""What the geometry GPU tests share: decoders (the fresh "fog" decoder, the planted box), shape codes, points, the planted box's level
and bound, and mesh equality.  ``amd`` and ``dev`` are the fixtures of ``oracle_bands``."""
import numpy as np
import torch

from oracle import supnerf_oracle as O
from planted_decoder import planted_params

LEVEL_BOX = float(np.log1p(np.exp(np.float32(0.0))))        # softplus(0): the planted box's surface d1 = H
BOUND_BOX = (-0.7, 0.7)


def model(amd, dev, sb, tb, params=None, seed=0):
    m = amd.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
    m.load_state_dict(params if params is not None else O.init_decoder_params(sb, tb, seed=seed, sigma_bias=-2.0), strict=True)
    return m.to(dev)


def box(amd, dev, sb=3, tb=1, seed=1, **planted):
    """The planted box decoder (``planted``: ``far_pre``, ``wobble``)."""
    return model(amd, dev, sb, tb, params=planted_params(sb, tb, seed=seed, **planted))


def codes(B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 256, generator=g) * 0.5).to(dev)


def points(P, seed, dev):
    """(xyz (P, 3) in the unit cube, unit view directions (P, 3), the generator for more)."""
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(P, 3, generator=g) - 0.5).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1).to(dev)
    return xyz, vd, g


def latent(model, sc):
    """The latent terms the density reads: a zero texture code."""
    return model.latent_terms(sc, torch.zeros_like(sc)).detach()


def same_meshes(a, b):
    return len(a) == len(b) and all(torch.equal(va, vb) and torch.equal(fa, fb) for (va, fa), (vb, fb) in zip(a, b))
