"""Test helper: the rules of the compact scene kernels (include/supnerf_hip.h, "Scene rows, compact") in a few lines of torch, on top of the
dense outputs of tests/scene_rows_restatement.py or of the dense kernels: dtype-generic, bit-preserving (only copies and fills)."""
import torch


def capacity(n):
    """n rounded up to a multiple of 32, at least 32."""
    return max(32, 32 * -(-int(n) // 32))


def slots(hit, C):
    """hit (Nr,Nb) -> scan (Nr,Nb) int32 inclusive prefix sum along the pixels, slot = scan - 1, kept = hit and 0 <= slot < C, count (Nb,)."""
    scan = torch.cumsum(hit.to(torch.int32), 0, dtype=torch.int32)
    slot = scan - 1
    kept = hit.bool() & (slot >= 0) & (slot < C)
    count = scan[-1] if hit.shape[0] else torch.zeros(hit.shape[1], dtype=torch.int32, device=hit.device)
    return scan, slot, kept, count


def pair_of_slot(slot, kept, C):
    """(Nb,C) int32: the pixel index of each slot, -1 on padding."""
    Nr, Nb = kept.shape
    out = torch.full((Nb, C), -1, dtype=torch.int32, device=kept.device)
    r, b = torch.nonzero(kept, as_tuple=True)
    out[b, slot[r, b].long()] = r.to(torch.int32)
    return out


def compact_rows(rows, slot, kept, C, fill):
    """Object-major dense rows (Nb*Nr, ...) -> compact rows (Nb*C, ...): a kept pair's row at b*C + slot, ``fill`` (broadcast) on padding."""
    Nr, Nb = kept.shape
    out = torch.empty((Nb * C,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    out[:] = torch.as_tensor(fill, dtype=rows.dtype, device=rows.device)
    r, b = torch.nonzero(kept, as_tuple=True)
    out[b * C + slot[r, b].long()] = rows[b * Nr + r]
    return out


def scatter_rows(compact, slot, kept, fill):
    """The inverse: compact rows (Nb*C, ...) -> object-major dense rows (Nb*Nr, ...), ``fill`` on every pair that is not kept."""
    Nr, Nb = kept.shape
    C = compact.shape[0] // Nb
    out = torch.empty((Nb * Nr,) + tuple(compact.shape[1:]), dtype=compact.dtype, device=compact.device)
    out[:] = torch.as_tensor(fill, dtype=compact.dtype, device=compact.device)
    r, b = torch.nonzero(kept, as_tuple=True)
    out[b * Nr + r] = compact[b * C + slot[r, b].long()]
    return out


def scene_samples_compact(dense, hit, C, S):
    """The dense outputs (dict or tuple: xyz, viewdir (Nb*Nr,S,3), z_vals (Nr,Nb*S)) and hit (Nr,Nb) -> dict: xyz, viewdir (Nb*C,S,3) with the
    padding constants, z_vals with -1 on every pair that is not kept, kept, pair_of_slot, scan, slot, count."""
    xyz, viewdir, z = (dense["xyz"], dense["viewdir"], dense["z_vals"]) if isinstance(dense, dict) else dense[:3]
    scan, slot, kept, count = slots(hit, C)
    Nr, Nb = kept.shape
    z = torch.where(kept[:, :, None].expand(Nr, Nb, S).reshape(Nr, Nb * S), z, torch.full_like(z, -1.0))
    return dict(xyz=compact_rows(xyz, slot, kept, C, 0.0), viewdir=compact_rows(viewdir, slot, kept, C, [0.0, 0.0, 1.0]), z_vals=z, kept=kept,
                pair_of_slot=pair_of_slot(slot, kept, C), scan=scan, slot=slot, count=count)


def gather_compact(sigmas, rgbs, slot, kept, S):
    """Compact decoder outputs (Nb*C*S), (Nb*C*S,3) -> rows (Nr,Nb*S), (Nr,Nb*S,3): a kept pair's rows from its slot, (0, white) elsewhere."""
    Nr, Nb = kept.shape
    sig = scatter_rows(sigmas.reshape(-1, S), slot, kept, 0.0).reshape(Nb, Nr, S).permute(1, 0, 2).reshape(Nr, Nb * S)
    rgb = scatter_rows(rgbs.reshape(-1, S, 3), slot, kept, 1.0).reshape(Nb, Nr, S, 3).permute(1, 0, 2, 3).reshape(Nr, Nb * S, 3)
    return sig, rgb


def gather_compact_bwd(d_sig_rows, d_rgb_rows, pos, S):
    """Rows' gradients (Nr,Nb*S), (Nr,Nb*S,3) -> the compact ones (Nb*C*S), (Nb*C*S,3) through pair_of_slot ``pos`` (Nb,C): exact zeros on padding."""
    Nb, C = pos.shape
    Nr = d_sig_rows.shape[0]
    live = pos >= 0
    r = pos.clamp_min(0).long()                                                  # (Nb,C)
    b = torch.arange(Nb, device=pos.device)[:, None].expand(Nb, C)
    sig = torch.where(live[..., None], d_sig_rows.reshape(Nr, Nb, S)[r, b], torch.zeros((), dtype=d_sig_rows.dtype, device=pos.device))
    rgb = torch.where(live[..., None, None], d_rgb_rows.reshape(Nr, Nb, S, 3)[r, b], torch.zeros((), dtype=d_rgb_rows.dtype, device=pos.device))
    return sig.reshape(-1), rgb.reshape(-1, 3)
