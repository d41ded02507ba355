"""GPU tests of the scene composite FORWARD (snr_scene_composite_fwd: scene_fast_kernel<RUN> + scene_general_kernel) at its tie, list and
grid-stride seams, on inputs that turn a sorted slot into a colour (tests/scene_cases.py; their teeth: tests/test_scene_cases_cpu.py).

The reference for every value is ``oracle.scene_composite`` in fp32 (o32) and, as o64, the dense restatement
(tests/scene_grad_restatement.py) in float64 up to 512 samples per pixel and the oracle in float64 above; judged by the project's fp32 band
(tests/oracle_bands.py).  Every case also holds the project's bit rule: the hint only changes how the ranks are found, so ``run_length`` = S
and ``run_length`` = 0 give equal bits.  A case that names a kernel path asserts it by the launcher's own preconditions (``launch_path``).

Which member of a tie group survives is not observable in forward values (its data lands on the group's first slot, whose interval has width
zero); these tests see that a tie group vanishes and where every other sample lands.  The survivor rule belongs to test_scene_grad_gpu.py."""
import pytest
import torch

import scene_cases as SC
import scene_grad_restatement as R
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, check_all  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

NAMES = ("rgb", "depth", "acc")
MAX_WAVES = 8192 * 4            # the launch's cap: 8192 workgroups of 4 waves, one pixel per wave and trip
MARK_BITS = 0x7fc5ce4e          # what the fast pass leaves in rgb[3 pix] for the marked-only general pass


def launch_path(n, run):
    """The kernels a launch takes, by what the launcher and scene_general_kernel read: "fast" = scene_fast_kernel<run> then the marked-only
    general kernel, "merge" = the general kernel's list merge, "rank" = its rank sort."""
    if n <= 256 and run in (32, 64, 128):
        return "fast"
    return "merge" if run > 1 and n % run == 0 else "rank"


def run_kernel(amd, dev, sig, rgb, z, white, run):
    return amd.ops.scene_composite(sig.to(dev), rgb.to(dev), z.to(dev), white, run)


def oracle_refs(sig, rgb, z, white):
    return O.scene_composite(sig, rgb, z, white), O.scene_composite(sig.double(), rgb.double(), z.double(), white)


def dense_o64(dev, sig, rgb, z, whites=(True, False)):
    """The dense restatement in float64 for both backgrounds: the merge (P n^2 booleans, in chunks of pixels, evaluated by torch on the
    device) is made once and composited twice.  -> {white: (rgb, depth, acc)} on the CPU."""
    assert z.shape[1] <= 512
    outs = {w: [] for w in whites}
    for a in range(0, max(z.shape[0], 1), 256):
        merged = R.merged_rows(*[t[a:a + 256].to(dev).double() for t in (sig, rgb, z)])
        for w in whites:
            outs[w].append([o.cpu() for o in O.composite(*merged, w)])
    return {w: tuple(torch.cat([c[k] for c in outs[w]]) for k in range(3)) for w in whites}


def in_band_and_same_bits(amd, dev, sig, rgb, z, white, S, o32, o64, name):
    """Hint S and hint 0: equal bits, and inside the band."""
    got = run_kernel(amd, dev, sig, rgb, z, white, S)
    rank = run_kernel(amd, dev, sig, rgb, z, white, 0)
    for k, a, b in zip(NAMES, got, rank):
        assert torch.equal(a, b), (name, k, int((a != b).sum()))
    check_all([(f"{name} hint {S} {k}", g, a, b) for k, g, a, b in zip(NAMES, got, o32, o64)]
              + [(f"{name} hint 0 {k}", g, a, b) for k, g, a, b in zip(NAMES, rank, o32, o64)], "fp32")
    return got


# ------------------------------------------------------------------------------------------------ probe batches
PROBES = [("fast", 1, 32), ("fast", 3, 32), ("fast", 5, 32), ("fast", 7, 32), ("fast", 8, 32),      # RUN 32: n = 32, 96, 160, 224: a partial last pass
          ("fast", 1, 64), ("fast", 2, 64), ("fast", 3, 64), ("fast", 4, 64),                       # RUN 64
          ("fast", 1, 128), ("fast", 2, 128),                                                       # RUN 128
          ("merge", 3, 16), ("merge", 2, 5), ("merge", 3, 85), ("merge", 5, 64), ("merge", 2, 256)]
_batch = {}


def probe_batch(dev, Nb, S):
    """The batch of one shape with its references, made once and left unchanged (the latest shape only: the cases of a shape are neighbours)."""
    if (Nb, S) not in _batch:
        _batch.clear()
        sig, rgb, z, meta = SC.batch(Nb, S, torch.Generator().manual_seed(100 * Nb + S))
        o64 = dense_o64(dev, sig, rgb, z)
        o32 = {w: O.scene_composite(sig, rgb, z, w) for w in (True, False)}
        _batch[(Nb, S)] = (sig, rgb, z, meta, o32, o64)
    return _batch[(Nb, S)]


@pytest.mark.parametrize("path,Nb,S,white", [(*p, w) for p in PROBES for w in (True, False)])
def test_probe_batches(amd, dev, path, Nb, S, white):
    """One launch of every tie class of one shape, slot by slot, among as many random pixels; then the same with hint 0 (rank sort only)."""
    n = Nb * S
    assert launch_path(n, S) == path and launch_path(n, 0) == "rank"
    sig, rgb, z, meta, o32, o64 = probe_batch(dev, Nb, S)
    # pixels that the merge finishes and pixels that it must hand on (ties across lists, a descending list) are both in the launch
    tied = torch.tensor([SC.has_tie(z[i]) for i in torch.nonzero(meta["row"] >= 0).flatten()[::max(n // 4, 1)]])
    assert bool(tied.any()) and not bool(tied.all()) and "descending" in meta["names"]
    got = in_band_and_same_bits(amd, dev, sig, rgb, z, white, S, o32[white], o64[white], f"({Nb},{S}) {path}")
    # said directly: a tie-free slot shows its own sample, a slot of a tie group shows nothing
    free, lit = meta["free"], meta["lit"]
    want = SC.colours(n)[lit[free]]
    assert float((got[0].cpu()[free] - want).abs().max()) < 1e-4
    hidden = (meta["row"] >= 0) & ~free
    assert float((got[0].cpu()[hidden] - (1.0 if white else 0.0)).abs().max()) == 0 and float(got[1].cpu()[hidden].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ grid-stride loop and prefetch
@pytest.mark.parametrize("Nb,S", [(3, 32), (1, 64), (2, 128)])
def test_grid_stride(amd, dev, Nb, S):
    """More pixels than two trips of every wave: three trips for five waves, two for the rest, the fast kernel's prefetch taken twice, with
    pixels that the fast pass marks (a tie at a list's end, a descending list) inside the strides."""
    P = 2 * MAX_WAVES + 5
    n = Nb * S
    assert launch_path(n, S) == "fast" and P > 2 * MAX_WAVES
    sig, rgb, z = R.shape_case(Nb, S, P)
    gen = torch.Generator().manual_seed(P + n)
    rows = SC.tie_rows(Nb, S, gen)
    for name, step in (("tie_at_end", 97), ("descending", 101)):
        if name in rows:
            at = torch.arange(0, P, step)
            z[at] = rows[name].reshape(-1)
            sig[at] = torch.rand(at.numel(), n, generator=gen) * 2 - 0.3
            rgb[at] = torch.rand(at.numel(), n, 3, generator=gen)
    o32, o64 = oracle_refs(sig, rgb, z, True)
    in_band_and_same_bits(amd, dev, sig, rgb, z, True, S, o32, o64, f"grid stride ({Nb},{S})")


# ------------------------------------------------------------------------------------------------ C ABI seams
def abi_call(amd, dev, ins, P, n, run, white, rgb, depth, acc):
    ops = amd.ops
    rc = amd._lib.lib().snr_scene_composite_fwd(ops._p(ins[0]), ops._p(ins[1]), ops._p(ins[2]), P, n, run, ops.WHITE_BKGD if white else 0,
                                                ops._p(rgb), ops._p(depth), ops._p(acc), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("path,Nb,S,run", [("fast", 3, 32, 32), ("fast", 2, 64, 64), ("rank", 3, 32, 0), ("merge", 2, 5, 5), ("rank", 1, 257, 0)])
def test_abi_outputs_nulls_and_mark(amd, dev, path, Nb, S, run, white):
    """Caller-owned outputs with canaries behind them: every element written, nothing behind; ``depth`` / ``acc`` NULL, one at a time and
    both; an ``rgb`` buffer that already holds the fast pass's mark in every word."""
    n = Nb * S
    assert launch_path(n, run) == path
    sig, rgb, z, meta = SC.batch(Nb, S, torch.Generator().manual_seed(n + run))
    P = min(z.shape[0], 301)
    ins = [t[:P].to(dev).contiguous() for t in (sig, rgb, z)]
    assert bool((meta["row"][:P] >= 0).any()) and bool((meta["row"][:P] < 0).any())
    want = amd.ops.scene_composite(*ins, white, run)
    CAN, PAD = 12345.5, 256
    sizes = {"rgb": 3 * P, "depth": P, "acc": P}

    def fresh(fill_bits=None):
        bufs = {k: torch.full((m + PAD,), CAN, device=dev) for k, m in sizes.items()}
        for k, m in sizes.items():
            bufs[k][:m] = float("nan")
        if fill_bits is not None:
            bufs["rgb"][:sizes["rgb"]] = torch.full((sizes["rgb"],), fill_bits, dtype=torch.int32, device=dev).view(torch.float32)
        return bufs

    def check(bufs, used):
        for k, ref in zip(NAMES, want):
            body, tail = bufs[k][:sizes[k]], bufs[k][sizes[k]:]
            assert bool((tail == CAN).all()), k
            if k in used:
                assert torch.equal(body, ref.reshape(-1)), k
            else:
                assert bool(torch.isnan(body).all()), k               # not handed to the call: untouched

    for used in (NAMES, ("rgb", "acc"), ("rgb", "depth"), ("rgb",)):
        bufs = fresh()
        abi_call(amd, dev, ins, P, n, run, white, bufs["rgb"], bufs["depth"] if "depth" in used else None, bufs["acc"] if "acc" in used else None)
        check(bufs, used)
    bufs = fresh(MARK_BITS)
    assert int(bufs["rgb"][:3 * P].view(torch.int32)[0]) == MARK_BITS
    abi_call(amd, dev, ins, P, n, run, white, bufs["rgb"], bufs["depth"], bufs["acc"])
    check(bufs, NAMES)


# ------------------------------------------------------------------------------------------------ limits
@pytest.mark.parametrize("run", [0, 853])
def test_most_samples_per_pixel(amd, dev, run):
    """1706 samples per pixel: all the LDS a workgroup can be granted (4 waves x 6 rows x 1706 floats = 163 776 bytes)."""
    n = 1706
    assert 4 * 6 * n * 4 <= 160 * 1024 < 4 * 6 * (n + 1) * 4 and launch_path(n, run) == ("merge" if run else "rank")
    sig, rgb, z = R.shape_case(2, 853, 5)
    o32, o64 = oracle_refs(sig, rgb, z, True)
    got = run_kernel(amd, dev, sig, rgb, z, True, run)
    check_all([(f"n 1706 run {run} {k}", g, a, b) for k, g, a, b in zip(NAMES, got, o32, o64)], "fp32")


def test_limits(amd, dev):
    with pytest.raises(amd.SnrError):
        amd.ops.scene_composite(torch.zeros(2, 1707, device=dev), torch.zeros(2, 1707, 3, device=dev), torch.zeros(2, 1707, device=dev))
    for run in (0, 64):
        e = amd.ops.scene_composite(torch.zeros(0, 128, device=dev), torch.zeros(0, 128, 3, device=dev), torch.zeros(0, 128, device=dev), True, run)
        assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2].shape == (0,)


@pytest.mark.parametrize("white", [True, False])
def test_sixteen_lists_of_64(amd, dev, white):
    """n = 1024 in lists of 64: above the fast kernel's 256, the general kernel's merge over 16 lists, every tie class slot by slot."""
    Nb, S = 16, 64
    assert launch_path(Nb * S, S) == "merge"
    rows = SC.tie_rows(Nb, S, torch.Generator().manual_seed(1024))
    parts = [SC.probe(r) for r in rows.values()]
    sig, rgb, z = [torch.cat([p[k] for p in parts]) for k in range(3)]
    o32, o64 = oracle_refs(sig, rgb, z, white)
    in_band_and_same_bits(amd, dev, sig, rgb, z, white, S, o32, o64, "(16,64)")


# ------------------------------------------------------------------------------------------------ permutation of lists
@pytest.mark.parametrize("Nb,S", [(3, 32), (7, 32), (4, 64), (2, 128), (3, 16), (3, 85), (5, 64)])
def test_swapping_lists(amd, dev, Nb, S):
    """Tie-free pixels: which object comes first in memory changes nothing, bit for bit, under the same hint."""
    gen = torch.Generator().manual_seed(Nb + S)
    n = Nb * S
    z = torch.cat([SC.base_lists(Nb, S, gen).reshape(1, n) for _ in range(40)])
    sig, rgb = torch.rand(40, n, generator=gen) * 2 - 0.3, torch.rand(40, n, 3, generator=gen)
    p_sig, p_rgb, p_z, _, free = SC.probe(SC.tie_rows(Nb, S, gen)["descending"])
    assert bool(free.all())
    sig, rgb, z = torch.cat([sig, p_sig]), torch.cat([rgb, p_rgb]), torch.cat([z, p_z])
    assert bool(R.tie_free(z).all())
    order = torch.arange(Nb).roll(1)
    swap = lambda t: t.view(t.shape[0], Nb, S, *t.shape[2:])[:, order].reshape(t.shape).contiguous()   # noqa: E731
    for run in (S, 0):
        base = run_kernel(amd, dev, sig, rgb, z, True, run)
        got = run_kernel(amd, dev, swap(sig), swap(rgb), swap(z), True, run)
        for a, b in zip(got, base):
            assert torch.equal(a, b)
