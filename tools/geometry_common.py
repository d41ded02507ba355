"""What the geometry timing tools (geometry_time, density_grad_time, narrow_band_time, mesh_grad_time) share: the import path, device-event
timing, the decoders they time (the fresh "fog" decoder, the planted box with ``wobble``), shape codes and the common arguments."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import supnerf_amd as A  # noqa: E402
from oracle import supnerf_oracle as O  # noqa: E402
from planted_decoder import WOBBLE, planted_params  # noqa: E402

LEVEL_BOX = float(np.log1p(np.exp(np.float32(0.0))))        # softplus(0): the planted box's surface
BOUND_BOX = (-0.7, 0.7)


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:
        return None


def timed(fn):
    """Milliseconds of one call between two device events (host reads inside the call included)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    return float(np.median([timed(fn) for _ in range(reps)]))


def alternate(f_a, f_b, reps):
    """Median milliseconds of ``f_a`` and of ``f_b``, called in turn ``reps`` times."""
    t_a, t_b = [], []
    for _ in range(reps):
        t_a.append(timed(f_a))
        t_b.append(timed(f_b))
    return float(np.median(t_a)), float(np.median(t_b))


def _decoder(params, sb, tb, dev):
    m = A.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
    m.load_state_dict(params)
    return m.to(dev)


def fog_decoder(sb, tb, dev):
    return _decoder(O.init_decoder_params(sb, tb, seed=0, sigma_bias=-2.0), sb, tb, dev)


def box_decoder(sb, tb, dev):
    return _decoder(planted_params(sb, tb, seed=1, wobble=WOBBLE), sb, tb, dev)


def codes(B, seed, dev):
    return (torch.randn(B, 256, generator=torch.Generator().manual_seed(seed)) * 0.5).to(dev)


def latent(model, sc):
    """The latent terms the density reads: a zero texture code."""
    return model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous()


def arguments(*extra):
    """The parser of ``--reps`` and ``--commit`` plus ``extra``: (flag, keyword arguments) pairs."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    ap.add_argument("--commit", default=None, help="commit to report when the tree has no .git")
    return ap.parse_args()


BLOCKS = ("--blocks", dict(type=int, nargs=2, default=(3, 1)))
RES = ("--res", dict(type=int, nargs="+", default=[128, 256, 512]))
BATCH = ("--batch", dict(type=int, nargs="+", default=[1, 8]))


def report(tool, a, blocks, **fields):
    print(json.dumps({"tool": tool, "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0), "blocks": list(blocks), **fields}))
