"""Test helper: exact comparisons against the golden vectors on any CPU.

The fixtures under tests/golden/ hold the reference's float32 outputs, recorded on one x86-64 CPU, and the oracle reproduces them bit for
bit wherever the CPU arithmetic is the recording's.  The BLAS and vector-math libraries choose their kernels by CPU model, so on another
CPU the same operations round differently in the last bits.  ``recording_arithmetic()`` tells the two cases apart with a canary recorded
next to the fixtures (golden/cpu_arith.json, golden/gen_cpu_arith.py): where it matches bit for bit, every check stays exactly as tight as
written; elsewhere a check also admits GOLDEN_ULPS float32 ulps of the expected values' largest magnitude."""
import functools
import importlib.util
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_ULPS = 64
_EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def recording_arithmetic():
    """True when this host's float32 CPU arithmetic reproduces the fixtures' recording bit for bit."""
    spec = importlib.util.spec_from_file_location("gen_cpu_arith", os.path.join(GOLDEN, "gen_cpu_arith.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "cpu_arith.json")) as f:
        return gen.canary_digests() == json.load(f)


def golden_tol(expected, tol=0.0):
    """``tol`` on the recording's arithmetic; elsewhere at least GOLDEN_ULPS float32 ulps of max |expected|."""
    if recording_arithmetic():
        return tol
    e = torch.as_tensor(expected).detach()
    if not e.is_floating_point() or e.numel() == 0:
        return tol
    return max(tol, GOLDEN_ULPS * _EPS32 * float(e.double().abs().max()))


def golden_equal(actual, expected):
    """``torch.equal`` on the recording's arithmetic; elsewhere equal shapes and dtypes and at most golden_tol(expected) apart."""
    a, e = torch.as_tensor(actual).detach(), torch.as_tensor(expected).detach()
    if recording_arithmetic() or not e.is_floating_point():
        return torch.equal(a, e)
    if a.shape != e.shape or a.dtype != e.dtype:
        return False
    return a.numel() == 0 or float((a.double() - e.double()).abs().max()) <= golden_tol(e)
