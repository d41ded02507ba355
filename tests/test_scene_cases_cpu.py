"""CPU tests of the scene-composite forward inputs (tests/scene_cases.py): that they have teeth.  On every named row the reference
(``oracle.scene_composite``) and the dense restatement agree; a plain stable sort that does not collapse equal depths, and a merge that
counts one list one slot off, leave the fp32 band of tests/oracle_bands.py that the GPU tests judge the kernels with; a tie-free probe
pixel renders its lit sample's colour and depth, so that a slot number IS a colour."""
import pytest
import torch

import scene_cases as SC
import scene_grad_restatement as R
from oracle import supnerf_oracle as O
from oracle_bands import in_band

# every (Nb, S) of the probe batches of tests/test_scene_forward_gpu.py
SHAPES = [(1, 32), (3, 32), (5, 32), (7, 32), (8, 32), (1, 64), (2, 64), (3, 64), (4, 64), (1, 128), (2, 128),
          (3, 16), (2, 5), (3, 85), (5, 64), (2, 256)]
NAMES = ("rgb", "depth", "acc")


def stable_sort_variant(sig, rgb, z, white):
    """A merge that is NOT the rule: a plain stable sort, equal depths keep their own slots and their own data."""
    order = torch.sort(z, dim=1, stable=True).indices
    return O.composite(sig.gather(1, order), rgb.gather(1, order[:, :, None].expand(-1, -1, 3)), z.gather(1, order), white)


def shifted_list_variant(sig, rgb, z, white, S, q):
    """A merge that counts every sample of list q one slot too far (the last slot stays in range)."""
    lt, eb, _ = R.ranks(z)
    n = z.shape[1]
    pos = (lt + eb + (torch.arange(n) // S == q).long()[None]).clamp(max=n - 1)
    z_s = torch.zeros_like(z).scatter(1, pos, z)
    s_s = torch.zeros_like(sig).scatter(1, pos, sig)
    c_s = torch.zeros_like(rgb).scatter(1, pos[:, :, None].expand(-1, -1, 3), rgb)
    return O.composite(s_s, c_s, z_s, white)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"{p[0]}x{p[1]}")
def probes(request):
    """name -> (row, sig, rgb, z, lit, free, merged float64 rows) of one shape; the dense merge is made once and composited per background."""
    Nb, S = request.param
    rows = SC.tie_rows(Nb, S, torch.Generator().manual_seed(100 * Nb + S))
    out = {}
    for name, row in rows.items():
        sig, rgb, z, lit, free = SC.probe(row)
        merged = [torch.cat(p) for p in zip(*[R.merged_rows(sig[a:a + 128].double(), rgb[a:a + 128].double(), z[a:a + 128].double())
                                              for a in range(0, z.shape[0], 128)])]
        out[name] = (row, sig, rgb, z, lit, free, merged)
    return Nb, S, out


def test_rows_are_what_they_are_named(probes):
    Nb, S, out = probes
    want = {"plain", "all_empty", "partial_minus1", "equal_neighbours", "descending"}
    if Nb > 1:
        want |= {"last_eq_first", "tie_at_start", "tie_at_end", "const_real_eq", "two_equal_lists", "empties"}
    assert want <= set(out) and set(out) - want <= {"empty_last"}
    z = {k: v[0] for k, v in out.items()}
    asc = lambda r: bool((r[:, 1:] >= r[:, :-1]).all())                       # noqa: E731  what the kernels' order check accepts
    for k, r in z.items():
        assert r.shape == (Nb, S) and r.dtype == torch.float32
        assert asc(r) == (k != "descending"), k
        assert SC.has_tie(r) == (k not in ("plain", "descending")), k
    assert bool((z["plain"][:, 1:] > z["plain"][:, :-1]).all())
    assert bool((z["all_empty"] == -1).all()) and bool((z["partial_minus1"][0, :3] == -1).all()) and float(z["partial_minus1"][0, 3]) > 0
    a = min(4, S - 2)
    assert float(z["equal_neighbours"][0, a]) == float(z["equal_neighbours"][0, a + 1])
    if Nb > 1:
        assert float(z["last_eq_first"][1, 0]) == float(z["last_eq_first"][0, S - 1])
        assert float(z["tie_at_start"][0, 0]) in z["tie_at_start"][1].tolist() and float(z["tie_at_end"][0, S - 1]) in z["tie_at_end"][1].tolist()
        c = z["const_real_eq"]
        assert bool((c[1] == c[0, S // 2]).all()) and float(c[0, S // 2]) > 0
        assert torch.equal(z["two_equal_lists"][0], z["two_equal_lists"][1])
        e = z["empties"]
        assert bool((e[0] == -1).all()) and bool((e[Nb - 1] == -1).all() if Nb > 2 else (z["empty_last"][1] == -1).all())


@pytest.mark.parametrize("white", [True, False])
def test_oracle_restatement_and_variants(probes, white):
    Nb, S, out = probes
    for name, (row, sig, rgb, z, lit, free, merged) in out.items():
        o64 = O.composite(*merged, white)
        r32 = O.composite(*[m.float() for m in merged], white)                  # (the merge only moves values: exact in either format)
        o32 = O.scene_composite(sig, rgb, z, white)
        for k, a, b, c in zip(NAMES, o32, r32, o64):                             # 1. the reference inside the band around the restatement
            ok, _, msg = in_band(a, b, c, "fp32", f"{name} {k}")
            assert ok, msg
        assert all(torch.equal(a, b) for a, b in zip(O.scene_composite(sig.double(), rgb.double(), z.double(), white), o64))
        var = stable_sort_variant(sig.double(), rgb.double(), z.double(), white)
        if SC.has_tie(row):                                                     # 2. the stable sort is seen wherever there is a tie ...
            for k in (0, 1):
                ok, _, msg = in_band(var[k], o32[k], o64[k], "fp32", f"stable sort, {name} {NAMES[k]}")
                assert not ok, msg
        else:                                                                   #    ... and is the rule where there is none
            assert name in ("plain", "descending")
            assert all(torch.equal(a, b) for a, b in zip(var, o64))
        if name == "plain":                                                     # 3. one list counted one slot off
            for q in range(Nb):
                bad = shifted_list_variant(sig.double(), rgb.double(), z.double(), white, S, q)
                for k in (0, 1):
                    ok, _, msg = in_band(bad[k], o32[k], o64[k], "fp32", f"list {q} shifted, {NAMES[k]}")
                    assert not ok, msg
        # 4. a tie-free slot renders its own sample, every other pixel nothing: a slot number is a colour
        n = Nb * S
        assert int(free.sum()) == n - sum(int(c) for c in torch.unique(row, return_counts=True)[1] if c > 1)
        want_rgb = torch.where(free[:, None], SC.colours(n)[lit].double(), torch.full((n, 3), 1.0 if white else 0.0, dtype=torch.float64))
        want_depth = torch.where(free, row.reshape(-1)[lit].double(), torch.zeros(n, dtype=torch.float64))
        for k, got, want in (("rgb", o64[0], want_rgb), ("depth", o64[1], want_depth)):
            ok, _, msg = in_band(got, want, want, "fp32", f"{name} lit {k}")
            assert ok, msg
        assert torch.unique(o64[0][free].float(), dim=0).shape[0] == int(free.sum())
        if name in ("plain", "descending"):
            assert bool(free.all())


def test_batch_layout():
    """The shuffled launch holds every probe pixel once and as many random pixels, with its bookkeeping."""
    Nb, S = 3, 32
    sig, rgb, z, meta = SC.batch(Nb, S, torch.Generator().manual_seed(5))
    n, rows = Nb * S, len(meta["names"])
    assert z.shape == (2 * n * rows, n) and sig.shape == z.shape and rgb.shape == (*z.shape, 3)
    assert int((meta["row"] >= 0).sum()) == n * rows and int((meta["row"] == -1).sum()) == n * rows
    lit = sig == SC.LIT
    assert bool((lit.sum(1) == (meta["row"] >= 0)).all())
    p = torch.nonzero(meta["row"] >= 0).flatten()
    assert torch.equal(lit[p].long().argmax(1), meta["lit"][p])
    # probe and random pixels alternate often enough for both kinds to meet inside one wave's stride
    kinds = (meta["row"] >= 0).long()
    assert int((kinds[1:] != kinds[:-1]).sum()) > n * rows // 2
