#!/usr/bin/env python3
"""Fixture ``cpu_arith.json`` for tests/cpu_arith.py: the CPU float32 arithmetic the golden vectors were recorded with.

    python tests/golden/gen_cpu_arith.py

Run on the host (and with the torch build) that produced the other fixtures.  Seeded inputs and the outputs of the operations whose
last bits depend on the CPU's BLAS / vector-math code path (matrix products at the decoder's shapes, exp / softplus, cumprod, sums),
stored as the SHA-256 of every output's float32 bytes."""
import hashlib
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def canary_inputs():
    g = torch.Generator().manual_seed(1234)
    return {"x63": torch.randn(4096, 63, generator=g), "w63": torch.randn(256, 63, generator=g) * 0.1,
            "x256": torch.randn(4096, 256, generator=g), "w256": torch.randn(256, 256, generator=g) * 0.06,
            "b256": torch.randn(256, generator=g) * 0.01, "r3": torch.randn(512, 3, 3, generator=g), "v3": torch.randn(512, 3, 1, generator=g),
            "s": torch.randn(1024, 64, generator=g)}


def canary_outputs(i):
    F = torch.nn.functional
    return {"lin63": F.linear(i["x63"], i["w63"], i["b256"]), "lin256": F.linear(i["x256"], i["w256"], i["b256"]),
            "bmm3": torch.matmul(i["r3"], i["v3"]), "exp": torch.exp(-i["s"].abs()), "softplus": F.softplus(i["s"]),
            "cumprod": torch.cumprod(1.0 - torch.sigmoid(i["s"]), -1), "rowsum": (i["s"] * torch.sigmoid(i["s"])).sum(-1)}


def canary_digests():
    with torch.no_grad():
        out = canary_outputs(canary_inputs())
    return {k: hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() for k, v in out.items()}


if __name__ == "__main__":
    d = canary_digests()
    with open(os.path.join(HERE, "cpu_arith.json"), "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print("cpu_arith.json:", d)
