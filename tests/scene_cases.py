"""Test helper: inputs for the scene composite FORWARD (snr_scene_composite_fwd) that turn a sample's sorted slot into a colour, so that a
mis-ranked sample, a list counted one slot off or a tie group that fails to vanish moves a pixel by 1e-3 and more.  CPU only.

``tie_rows``  named depth rows (Nb, S) of one pixel: one row per tie class that the fast merge (scene_merge_fast) has separate code for.
``probe``     one pixel per sorted slot k of a row: sigma 0 everywhere except 1e4 on the sample that the rule of
              ``scene_grad_restatement.ranks`` puts on slot k, colours that are exact small fractions of the sample index.
``batch``     all probes of one shape plus as many ``shape_case`` random pixels, shuffled into one launch.

The depths of a row come from ONE jittered grid of n = Nb*S cells shared by all lists, near + (g + 0.4 u) * 4/n: distinct by construction
inside a list and across lists (n uniform fp32 draws do collide), and never closer than 0.6 * 4/n, so that a lit sample on a tie-free slot is
opaque (1e4 * 2.4/n >= 23 up to n = 1024: alpha = 1 - e^-23 at worst) and the pixel IS that sample's colour and depth.
The lists take their cells through random offsets and strides, so they overlap partly, like objects behind one another."""
import torch

import scene_grad_restatement as R

LIT = 1e4


def base_lists(Nb, S, gen):
    """(Nb, S) fp32 depths, every list strictly ascending, all n depths distinct and at least 0.6 * 4/n apart."""
    n = Nb * S
    start = torch.rand(Nb, 1, generator=gen) * 0.5 * n
    stride = 0.5 + torch.rand(Nb, 1, generator=gen)
    key = start + (torch.arange(S)[None] + torch.rand(Nb, S, generator=gen)) * stride          # ascending inside a list
    cell = torch.argsort(torch.argsort(key.view(-1))).view(Nb, S)                                # its place among all n keys
    near = 2 + 20 * float(torch.rand((), generator=gen))
    z = (near + (cell + 0.4 * torch.rand(Nb, S, generator=gen)) * (4.0 / n)).float()
    assert bool((z[:, 1:] > z[:, :-1]).all()) and bool(R.tie_free(z.view(1, n)).all())
    return z


def tie_rows(Nb, S, gen):
    """dict name -> (Nb, S) fp32 depth row of one pixel.  Rows that need two lists are left out when Nb = 1."""
    z = base_lists(Nb, S, gen)
    rows = {"plain": z}

    def variant(name):
        rows[name] = z.clone()
        return rows[name]
    if Nb > 1:
        r = variant("last_eq_first")                                  # list 1 starts where list 0 ends
        v = torch.sort(r[:2].reshape(-1))[0]                          # (the two lists' own grid depths, dealt out again)
        r[0] = v[:S]; r[1] = v[S - 1:2 * S - 1]
        r = variant("tie_at_start")                                   # list 1 holds list 0's element 0
        r[1, S // 2] = r[0, 0]; r[1] = torch.sort(r[1])[0]
        r = variant("tie_at_end")                                     # ... list 0's element S - 1
        r[1, S // 2] = r[0, S - 1]; r[1] = torch.sort(r[1])[0]
        r = variant("const_real_eq")                                  # a constant list at a REAL depth that a sample elsewhere has
        r[1] = r[0, S // 2]
        r = variant("two_equal_lists")
        r[1] = r[0]
        r = variant("empties")                                        # lists that miss the pixel, the first and the last among them
        r[0] = -1
        if Nb > 2:
            r[Nb - 1] = -1
        if Nb > 4:
            r[2] = -1
        if Nb == 2:
            variant("empty_last")[1] = -1
    variant("all_empty")[:] = -1
    variant("partial_minus1")[0, :3] = -1                             # a list that starts with some -1 and then increases
    r = variant("equal_neighbours")                                   # passes the kernels' <= order check; its own list must refuse it
    a = min(4, S - 2)
    r[0, a + 1] = r[0, a]
    r = variant("descending")                                         # a wrong hint for this pixel only
    r[Nb // 2] = r[Nb // 2].flip(0)
    return rows


def has_tie(row):
    """Any two samples of the row share a depth (-1 included: empty samples are a tie group like any other)."""
    zs = torch.sort(row.reshape(-1))[0]
    return bool((zs[1:] == zs[:-1]).any())


def colours(n):
    """(n, 3) fp32, exact: ((i+1)/1024, ((7i) % 64 + 1)/128, ((13i) % 32 + 1)/64); distinct rows for n <= 1024, none of them white or black."""
    i = torch.arange(n)
    return torch.stack([(i + 1) / 1024, ((7 * i) % 64 + 1) / 128, ((13 * i) % 32 + 1) / 64], 1).float()


def probe(row):
    """sig (n,n), rgb (n,n,3), z (n,n), lit (n,), free (n,): pixel k lights the sample that the rule puts on sorted slot k.  A first slot
    of a tie group is fed by the group's survivor (ea == 0), every other slot holds the sample that sits there (pos == k).  ``free[k]``:
    slot k belongs to no tie group; the pixel then renders colours(n)[lit[k]] at depth row[lit[k]].  Every other pixel must render nothing."""
    z = row.reshape(1, -1).float()
    n = z.shape[1]
    lt, eb, ea = [t[0] for t in R.ranks(z)]
    idx = torch.arange(n)
    sitter = torch.empty(n, dtype=torch.long); sitter[lt + eb] = idx
    feeder = torch.full((n,), -1, dtype=torch.long); feeder[lt[ea == 0]] = idx[ea == 0]
    lit = torch.where(feeder >= 0, feeder, sitter)
    free = (eb + ea)[lit] == 0
    sig = torch.zeros(n, n); sig[idx, lit] = LIT
    return sig, colours(n)[None].expand(n, n, 3).contiguous(), z.expand(n, n).contiguous(), lit, free


def batch(Nb, S, gen):
    """One launch: every row's probe and the same number of ``shape_case`` pixels, shuffled so that pixels the fast pass marks and pixels it
    finishes are neighbours.  -> sig (P,n), rgb (P,n,3), z (P,n), meta = dict(names, row (P,) index into names or -1, lit (P,), free (P,))."""
    rows = tie_rows(Nb, S, gen)
    names = list(rows)
    parts = [probe(rows[k]) for k in names]
    n = Nb * S
    Pp = n * len(names)
    rnd = R.shape_case(Nb, S, Pp)
    sig = torch.cat([p[0] for p in parts] + [rnd[0]])
    rgb = torch.cat([p[1] for p in parts] + [rnd[1]])
    z = torch.cat([p[2] for p in parts] + [rnd[2]])
    row = torch.cat([torch.arange(len(names)).repeat_interleave(n), torch.full((Pp,), -1)])
    lit = torch.cat([p[3] for p in parts] + [torch.full((Pp,), -1)])
    free = torch.cat([p[4] for p in parts] + [torch.zeros(Pp, dtype=torch.bool)])
    perm = torch.randperm(2 * Pp, generator=gen)
    return sig[perm].contiguous(), rgb[perm].contiguous(), z[perm].contiguous(), dict(names=names, row=row[perm], lit=lit[perm], free=free[perm])
