"""Tensor-level operators over the C ABI: torch allocates, the HIP library computes.

Everything here requires fp32 tensors on an AMD GPU (``tensor.is_cuda`` under PyTorch-ROCm).
There is no CPU/eager fallback -- a CPU tensor raises."""
import ctypes as C
import functools
import math
import operator
import threading
import warnings
import weakref
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import BF16X3, BOX_DETACH, FP32, METRIC_Z, WHITE_BKGD, Z_BOX, Z_PER_OBJECT, Z_PER_RAY, Z_SHARED, RenderArgs, SnrError, check

_AUTO_DOWNGRADES = set()
IDENTITY_FRAME = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
PRECISIONS = {"fp32": FP32, "bf16x3": BF16X3}


def resolve_precision(precision, shape_blocks, texture_blocks, points_per_obj, backward=False) -> int:
    """'fp32' (exact fp32 MFMA), 'bf16x3' (the split kernels: every fp32 operand as two 16-bit pieces, three MFMAs per product, several times
    faster -- fp16 pieces in the forward chain, ~2^-22 per product, bf16 pieces in the backward chain, ~2^-17) or 'auto'
    (bf16x3 where the kernel supports the configuration, else fp32).  Asking for 'bf16x3' where it is unsupported raises.
    A pair (forward, backward) names the two launches apart, e.g. ("fp32", "bf16x3"): the reference's forward values bit for bit in
    its own arithmetic, the gradient on the split-bf16 kernel (it applies the ReLU pattern the forward saved; 2^-17 per product) --
    ``backward`` picks the member.  (A training triple (forward chain, backward chain, products) resolves like its first two.)"""
    if isinstance(precision, tuple):
        if len(precision) not in (2, 3):
            raise SnrError(f"a precision tuple is (forward, backward) or (forward chain, backward chain, products), got {precision!r}")
        precision = precision[1 if backward else 0]
    if isinstance(precision, int) and not isinstance(precision, bool):
        return precision
    if precision is None or precision == "auto":
        ok = _lib.lib().snr_precision_supported(BF16X3, shape_blocks, texture_blocks, int(points_per_obj))
        if not ok:
            key = (shape_blocks, texture_blocks, int(points_per_obj) % WAVE_TILE == 0)
            if key not in _AUTO_DOWNGRADES:          # say it once per configuration: 'auto' is several times slower here
                _AUTO_DOWNGRADES.add(key)
                warnings.warn(f"supnerf_amd: precision 'auto' runs the exact fp32 kernels for shape_blocks={shape_blocks}, texture_blocks={texture_blocks}, "
                              f"{points_per_obj} points per object: the split kernels need shape_blocks + texture_blocks <= 4 and whole 32-point tiles "
                              "per object", RuntimeWarning, stacklevel=3)
        return BF16X3 if ok else FP32
    if precision not in PRECISIONS:
        raise SnrError(f"unknown precision {precision!r}")
    code = PRECISIONS[precision]
    if not _lib.lib().snr_precision_supported(code, shape_blocks, texture_blocks, int(points_per_obj)):
        raise SnrError(f"precision {precision!r} is not available for shape_blocks={shape_blocks}, texture_blocks={texture_blocks}, "
                       f"{points_per_obj} points per object (needs <= 4 blocks in total and whole 32-point tiles per object)")
    return code


PRECISION_NAMES = {FP32: "fp32", BF16X3: "bf16x3"}
FP16_MAX = 65504.0
# what the range guard of precision "auto" accepts between the split forward and the exact-fp32 forward of the same launch: |a - b| <=
# RANGE_TOL * max(1, |b|) per value (measured distance of a healthy decoder: 6e-8 .. 1.6e-6)
RANGE_TOL = 1e-5


def precision_pair(precision, shape_blocks, texture_blocks, points_per_obj):
    """(forward, backward) arithmetic names a launch pair with this request would run in."""
    f = resolve_precision(precision, shape_blocks, texture_blocks, points_per_obj)
    b = resolve_precision(precision, shape_blocks, texture_blocks, points_per_obj, backward=True)
    return PRECISION_NAMES[f], PRECISION_NAMES[b]


def split_supported(shape_blocks, texture_blocks, points_per_obj) -> bool:
    return bool(_lib.lib().snr_precision_supported(BF16X3, shape_blocks, texture_blocks, int(points_per_obj)))


def outputs_disagree(split_outs, exact_outs, tol=RANGE_TOL):
    """0-dim device tensor: how many values of the split-arithmetic outputs are non-finite where the exact ones are finite, or further
    than ``tol * max(1, |exact|)`` from them (one host read decides; the range guard of ``auto``)."""
    bad = None
    for a, b in zip(split_outs, exact_outs):
        a, b = a.detach().reshape(-1), b.detach().reshape(-1)
        fin = torch.isfinite(b)
        n = ((~torch.isfinite(a)) & fin).sum() + (((a - b).abs() > tol * b.abs().clamp_min(1.0)) & fin).sum()
        bad = n if bad is None else bad + n
    return bad


def clamped_weight_count(params) -> torch.Tensor:
    """0-dim device tensor: entries of the per-point weights beyond the fp16 range -- the split forward packs them clamped to +-65504."""
    return sum((p.detach().abs() > FP16_MAX).sum() for p in params)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise SnrError("supnerf_amd operators need tensors on the GPU (no CPU fallback)")


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _p(t: Optional[torch.Tensor]):
    """Device address for the C ABI.  The ABI takes dense buffers and cannot know strides (include/supnerf_hip.h: "contiguous"), so
    EVERY pointer that crosses it goes through here and a tensor that is not a dense GPU buffer raises instead of being read out
    of bounds (round 2's fault: ``get_rays``' origins are a stride-0 view of the pose's three numbers)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise SnrError("supnerf_amd operators need tensors on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise SnrError(f"internal: a non-contiguous tensor (shape {tuple(t.shape)}, strides {t.stride()}) reached the C ABI; "
                       "operands must be made dense with _f32c first")
    return C.c_void_p(t.data_ptr())


def _p_rows(t: torch.Tensor):
    """Address of a 2-D row-major operand that travels WITH its leading dimension (snr_weight_grad's G, X, dW: a column block of a wider
    buffer is fine there); only the rows must be dense."""
    if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
        raise SnrError(f"expected a 2-D fp32 row-major GPU tensor, got shape {tuple(t.shape)} strides {t.stride()} {t.dtype} on {t.device}")
    return C.c_void_p(t.data_ptr())


def _ptr(t: Optional[torch.Tensor], dtype=torch.float32) -> int:
    """Like ``_p`` for struct fields (plain integer address), with the element type checked too."""
    if t is None:
        return 0
    if t.dtype != dtype:
        raise SnrError(f"internal: a {t.dtype} tensor reached the C ABI where {dtype} is expected")
    return _p(t).value or 0


def raw_stream(dev) -> int:
    """The current HIP stream of `dev` as an integer handle.  torch.cuda.current_stream() builds a Python Stream object per call (5 us; the
    public render functions ask ~18 times per optimiser iteration); the raw getter behind it does not."""
    d = dev if isinstance(dev, torch.device) else torch.device(dev)
    idx = d.index if d.index is not None else torch.cuda.current_device()
    try:
        return int(torch._C._cuda_getCurrentRawStream(idx))
    except AttributeError:      # (a torch build without the private getter)
        return int(torch.cuda.current_stream(d).cuda_stream)


def _stream(dev):
    return C.c_void_p(raw_stream(dev))


# ------------------------------------------------------------------------------------ weights
class DecoderLayer(NamedTuple):
    stem: str                # state-dict key without ".weight" / ".bias" (reference naming, src/model_supnerf.py:184-199)
    n_out: int
    n_in: int
    slot: Optional[int]      # place among the MFMA layers in the order the kernels consume them; None: one of the two narrow heads


@functools.lru_cache(maxsize=None)
def decoder_layers(shape_blocks: int, texture_blocks: int) -> Sequence[DecoderLayer]:
    """The per-point layers in the order snr_pack_weights expects their tensors: the Python twin of csrc/snr_layout.h's layer table
    (tests/test_host_logic.py ties the two).  The kernels are built for the decoder of every shipped config: W = latent = 256,
    L_xyz = 10, L_dir = 4."""
    rows = [("encoding_xyz.0", 256, 63, True)] + [(f"shape_layer_{j}.0", 256, 256, True) for j in range(1, shape_blocks + 1)]
    rows += [("encoding_shape", 256, 256, True), ("sigma.0", 1, 256, False), ("encoding_viewdir.0", 256, 256 + 27, True)]
    rows += [(f"texture_layer_{j}.0", 256, 256, True) for j in range(1, texture_blocks + 1)]
    rows += [("rgb.0", 128, 256, True), ("rgb.2", 3, 128, False)]
    slots = iter(range(len(rows)))
    return tuple(DecoderLayer(stem, n_out, n_in, next(slots) if mfma else None) for stem, n_out, n_in, mfma in rows)


def per_point_tensor_names(shape_blocks: int, texture_blocks: int) -> Sequence[str]:
    """State-dict keys of the per-point layers in the order snr_pack_weights expects them."""
    return [l.stem + q for l in decoder_layers(shape_blocks, texture_blocks) for q in (".weight", ".bias")]


def check_decoder_shapes(params: Dict[str, torch.Tensor], shape_blocks: int, texture_blocks: int):
    for l in decoder_layers(shape_blocks, texture_blocks):
        k, shp = l.stem + ".weight", (l.n_out, l.n_in)
        if k not in params or tuple(params[k].shape) != shp:
            got = tuple(params[k].shape) if k in params else None
            raise SnrError(f"unsupported decoder: {k} is {got}, the gfx950 kernels need {shp} "
                           "(W=256, latent_dim=256, num_xyz_freq=10, num_dir_freq=4)")


def pack_weights(params: Dict[str, torch.Tensor], shape_blocks: int, texture_blocks: int) -> torch.Tensor:
    """nn.Linear tensors (reference state-dict names) -> the kernels' packed stream buffer."""
    check_decoder_shapes(params, shape_blocks, texture_blocks)
    names = per_point_tensor_names(shape_blocks, texture_blocks)
    ts = [_f32c(params[n].detach()) for n in names]
    _need_gpu(*ts)
    dev = ts[0].device
    nbytes = _lib.lib().snr_packed_bytes(shape_blocks, texture_blocks)
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    with torch.cuda.device(dev):
        check(_lib.lib().snr_pack_weights(arr, len(ts), shape_blocks, texture_blocks, _p(packed), _stream(dev)), "snr_pack_weights")
    return packed


# ------------------------------------------------------------------------------------ composite
def composite_fwd(sigmas, rgbs, z_vals, z_mode, white_bkgd, rays_per_obj=0):
    sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
    n_rays, S = _composite_shapes("composite_fwd", sigmas, rgbs, z_vals, z_mode, rays_per_obj)
    _need_gpu(sigmas, rgbs, z_vals)
    dev = rgbs.device
    rgb = torch.empty(n_rays, 3, device=dev)
    depth = torch.empty(n_rays, device=dev)
    acc = torch.empty(n_rays, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_composite_fwd(_p(sigmas), _p(rgbs), _p(z_vals), z_mode, WHITE_BKGD if white_bkgd else 0, n_rays,
                                           rays_per_obj, S, _p(rgb), _p(depth), _p(acc), _stream(dev)), "snr_composite_fwd")
    return rgb, depth, acc


def scene_composite(sigmas, rgbs, z_vals, white_bkgd=True, run_length=0):
    """Per-pixel depth merge of n = Nb*S samples + composite (scripts/demo.py:555-565): sigmas, z_vals (P, n); rgbs (P, n, 3)
    -> rgb (P,3), depth (P), acc_trans (P).  Inference only (the reference runs it under no_grad).  ``run_length`` = S tells the kernel that
    every object's S samples are contiguous and ascending, so it merges the lists instead of rank-sorting (verified per pixel, see the header)."""
    sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
    _need_gpu(sigmas, rgbs, z_vals)
    P, n = _scene_shapes("scene_composite", sigmas, rgbs, z_vals)
    dev = sigmas.device
    rgb = torch.empty(P, 3, device=dev); depth = torch.empty(P, device=dev); acc = torch.empty(P, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_scene_composite_fwd(_p(sigmas), _p(rgbs), _p(z_vals), P, n, int(run_length), WHITE_BKGD if white_bkgd else 0,
                                                 _p(rgb), _p(depth), _p(acc), _stream(dev)), "snr_scene_composite_fwd")
    return rgb, depth, acc


SCENE_BWD_MAX_N = 512       # snr_scene_composite_bwd: samples per pixel (8 objects x 64 samples)


def _scene_shapes(name, sigmas, rgbs, z_vals):
    if sigmas.dim() != 2 or rgbs.shape != (*sigmas.shape, 3) or z_vals.shape != sigmas.shape:
        raise SnrError(f"{name}: expected sigmas/z (P,n) and rgbs (P,n,3), got {tuple(sigmas.shape)}, {tuple(z_vals.shape)}, {tuple(rgbs.shape)}")
    return sigmas.shape


def _composite_shapes(name, sigmas, rgbs, z_vals, z_mode, rays_per_obj, grads=None):
    """Sizes the stand-alone composite kernels index with -> (n_rays, S): rgbs (..., S, 3), sigmas n_rays * S values, z_vals S (shared),
    B * S with B * rays_per_obj == n_rays (per object) or n_rays * S (per ray) values; ``grads`` = (d_rgb, d_depth, d_acc), each None or
    3 n_rays / n_rays / n_rays values.  Elements are counted, not dimensions: callers pass (B, n, S) as well as (N, S).  The C ABI sees
    pointers only, so a short operand here is an out-of-bounds read on the device.  An empty packet (n_rays == 0) launches nothing."""
    if rgbs.dim() < 2 or rgbs.shape[-1] != 3:
        raise SnrError(f"{name}: expected rgbs (..., S, 3), got {tuple(rgbs.shape)}")
    S = rgbs.shape[-2]
    n_rays = rgbs.numel() // (3 * S) if rgbs.numel() else 0
    if sigmas.numel() != n_rays * S:
        raise SnrError(f"{name}: sigmas {tuple(sigmas.shape)} do not hold one value per sample of rgbs {tuple(rgbs.shape)} ({n_rays} rays x {S} samples)")
    if n_rays:
        rpo = int(rays_per_obj)
        if z_mode == Z_PER_OBJECT and (rpo < 1 or n_rays % rpo):
            raise SnrError(f"{name}: per-object depths need rays_per_obj >= 1 that divides the ray count, got rays_per_obj {rpo} for {n_rays} rays")
        want = {Z_SHARED: S, Z_PER_OBJECT: n_rays // max(rpo, 1) * S, Z_PER_RAY: n_rays * S}.get(z_mode)
        if want is not None and z_vals.numel() != want:
            raise SnrError(f"{name}: z_vals {tuple(z_vals.shape)} hold {z_vals.numel()} depths, z_mode {z_mode} needs {want} for {n_rays} rays x {S} samples"
                           + (f" in {n_rays // rpo} objects of {rpo} rays" if z_mode == Z_PER_OBJECT else ""))
    for g, per_ray, gname in zip(grads or (), (3, 1, 1), ("d_rgb", "d_depth", "d_acc")):
        if g is not None and g.numel() != per_ray * n_rays:
            raise SnrError(f"{name}: {gname} {tuple(g.shape)} holds {g.numel()} values, {n_rays} rays need {per_ray * n_rays}")
    return n_rays, S


def scene_composite_bwd(sigmas, rgbs, z_vals, white_bkgd, run_length, d_rgb, d_depth=None, d_acc=None, need_dz=True):
    """Backward of ``scene_composite`` in one launch (rules: include/supnerf_hip.h): d_rgb (P,3), d_depth (P) / d_acc (P) or None
    -> d_sigmas (P,n), d_rgbs (P,n,3), d_z (P,n) or None.  n <= 512."""
    sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
    # dense copies are NAMED so that they live until the launch is enqueued (see composite_bwd)
    d_rgb, d_depth, d_acc = _f32c(d_rgb), _f32c(d_depth), _f32c(d_acc)
    _need_gpu(sigmas, rgbs, z_vals, d_rgb, d_depth, d_acc)
    P, n = _scene_shapes("scene_composite_bwd", sigmas, rgbs, z_vals)
    if d_rgb is None or d_rgb.shape != (P, 3) or any(g is not None and g.numel() != P for g in (d_depth, d_acc)):
        raise SnrError(f"scene_composite_bwd: expected d_rgb ({P},3) and d_depth / d_acc ({P},) or None")
    if n > SCENE_BWD_MAX_N:
        raise SnrError(f"scene_composite_bwd: {n} samples per pixel, the backward takes at most {SCENE_BWD_MAX_N}")
    dev = sigmas.device
    d_sig = torch.empty(P, n, device=dev)
    d_rgbs = torch.empty(P, n, 3, device=dev)
    d_z = torch.empty(P, n, device=dev) if need_dz else None
    with torch.cuda.device(dev):
        check(_lib.lib().snr_scene_composite_bwd(_p(sigmas), _p(rgbs), _p(z_vals), P, n, int(run_length), WHITE_BKGD if white_bkgd else 0,
                                                 _p(d_rgb), _p(d_depth), _p(d_acc), _p(d_sig), _p(d_rgbs), _p(d_z), _stream(dev)),
              "snr_scene_composite_bwd")
    return d_sig, d_rgbs, d_z


class SceneComposite(torch.autograd.Function):
    """``scene_composite`` with gradients: to sigmas (P,n) and rgbs (P,n,3) always, to z_vals (P,n) when it needs one.  At most 512
    samples per pixel when any input requires grad."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, z_vals, white_bkgd, run_length):
        sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
        if any(ctx.needs_input_grad[:3]) and sigmas.dim() == 2 and sigmas.shape[1] > SCENE_BWD_MAX_N:
            raise SnrError(f"SceneComposite: {sigmas.shape[1]} samples per pixel, the backward takes at most {SCENE_BWD_MAX_N} "
                           "(ops.scene_composite renders more, without gradients)")
        out = scene_composite(sigmas, rgbs, z_vals, white_bkgd, run_length)
        ctx.save_for_backward(sigmas, rgbs, z_vals)
        ctx.cfg = (bool(white_bkgd), int(run_length))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_acc):
        sigmas, rgbs, z_vals = ctx.saved_tensors
        white, run_length = ctx.cfg
        need_dz = ctx.needs_input_grad[2]
        if d_rgb is None:
            d_rgb = torch.zeros(sigmas.shape[0], 3, device=sigmas.device)
        d_sig, d_rgbs, d_z = scene_composite_bwd(sigmas, rgbs, z_vals, white, run_length, d_rgb, d_depth, d_acc, need_dz)
        return d_sig, d_rgbs, d_z, None, None


def _scene_lists(name, cam2obj, wlh, rois, pixels, jitter, S):
    """Shapes and types of the scene sample kernels' operands -> (Nr, Nb)."""
    Nb = cam2obj.shape[0] if cam2obj.dim() == 3 else -1
    if Nb < 1 or cam2obj.shape != (Nb, 3, 4) or wlh.shape != (Nb, 3) or rois.shape != (Nb, 4) or pixels.dim() != 2 or pixels.shape[1] != 2:
        raise SnrError(f"{name}: expected cam2obj (Nb,3,4), wlh (Nb,3), rois (Nb,4), pixels (Nr,2), got {tuple(cam2obj.shape)}, {tuple(wlh.shape)}, "
                       f"{tuple(rois.shape)}, {tuple(pixels.shape)}")
    if rois.dtype != torch.int32 or pixels.dtype != torch.int32:
        raise SnrError(f"{name}: rois and pixels are int32 tensors, got {rois.dtype} and {pixels.dtype}")
    Nr = pixels.shape[0]
    if int(S) < 1 or (jitter is not None and jitter.shape != (Nr * Nb, int(S))):
        raise SnrError(f"{name}: expected n_samples >= 1 and jitter (Nr*Nb, S) = ({Nr * Nb}, {int(S)}) or None")
    return Nr, Nb


def _scene_samples_fwd(ctx, name, cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale, rend_aabb, shapenet_obj_cood, hit_scan=None, capacity=None):
    """Forward of ``SceneSamples`` and, with ``hit_scan`` and ``capacity``, of ``SceneSamplesCompact``: R = Nr or capacity rows per object
    -> xyz, viewdir (Nb*R,S,3), z_vals (Nr,Nb*S), the pair flags (Nr,Nb) uint8, and valid (Nr) uint8 or pair_of_slot (Nb,capacity) int32."""
    compact = hit_scan is not None
    cam2obj, wlh, jitter = _f32c(cam2obj), _f32c(wlh), _f32c(jitter)
    Nr, Nb = _scene_lists(name, cam2obj, wlh, rois, pixels, jitter, S)
    if len(Kvec) != 4:
        raise SnrError(f"{name}: Kvec is (fx, fy, cx, cy)")
    if compact:
        cap = _scene_capacity_arg(name, capacity)
        hit_scan = _scene_scan(name, hit_scan, Nr, Nb)
    _need_gpu(cam2obj, wlh, rois, pixels, jitter, hit_scan)
    rois, pixels = rois.contiguous(), pixels.contiguous()
    cfg = (*[float(v) for v in Kvec], int(S), float(adjust_scale), int(bool(rend_aabb)), int(bool(shapenet_obj_cood)))
    S = cfg[4]
    dev = cam2obj.device
    ctx.set_materialize_grads(False)        # (the kernel takes null for the gradients of outputs that were not used)
    R = cap if compact else Nr
    xyz, viewdir = torch.empty(Nb * R, S, 3, device=dev), torch.empty(Nb * R, S, 3, device=dev)
    z = torch.empty(Nr, Nb * S, device=dev)
    flag = torch.empty(Nr, Nb, dtype=torch.uint8, device=dev)
    last = torch.empty(Nb, cap, dtype=torch.int32, device=dev) if compact else torch.empty(Nr, dtype=torch.uint8, device=dev)
    lists = (_p(cam2obj), _p(wlh), _p(rois), _p(pixels), *cfg[:4], _p(jitter), Nr, Nb, *cfg[4:])
    outs = (_p(xyz), _p(viewdir), _p(z), _p(flag), _p(last))
    with torch.cuda.device(dev):
        if compact:
            check(_lib.lib().snr_scene_samples_compact_fwd(*lists, _p(hit_scan), cap, *outs, _stream(dev)), "snr_scene_samples_compact_fwd")
        else:
            check(_lib.lib().snr_scene_samples_fwd(*lists, *outs, _stream(dev)), "snr_scene_samples_fwd")
    ctx.save_for_backward(cam2obj, wlh, rois, pixels, jitter, *((hit_scan,) if compact else ()))
    ctx.cfg = cfg + ((cap,) if compact else ())
    ctx.mark_non_differentiable(flag, last)
    return xyz, viewdir, z, flag, last


def _scene_samples_bwd(ctx, name, n_inputs, d_xyz, d_viewdir, d_z):
    """Backward of both sample classes to cam2obj, one gradient slot per forward input; the compact one saved ``hit_scan`` and the capacity."""
    cam2obj, wlh, rois, pixels, jitter, *hit_scan = ctx.saved_tensors
    if ctx.needs_input_grad[1] or ctx.needs_input_grad[5]:
        raise SnrError(f"{name}: the box sizes and the jitter are data, no gradient is provided")
    if not ctx.needs_input_grad[0] or (d_xyz is None and d_viewdir is None and d_z is None):
        return (None,) * n_inputs
    *cfg, cap = ctx.cfg if hit_scan else (*ctx.cfg, None)
    Nr, Nb = pixels.shape[0], cam2obj.shape[0]
    dev = cam2obj.device
    d_xyz, d_viewdir, d_z = _f32c(d_xyz), _f32c(d_viewdir), _f32c(d_z)       # NAMED: they live until the launch is enqueued (see composite_bwd)
    if Nr == 0:
        return (torch.zeros_like(cam2obj),) + (None,) * (n_inputs - 1)
    d_cam2obj = torch.empty_like(cam2obj)
    n_ws = int(_lib.lib().snr_scene_samples_bwd_ws_bytes(Nr, Nb))
    ws = torch.empty(n_ws // 8, dtype=torch.float64, device=dev)
    lists = (_p(cam2obj), _p(wlh), _p(rois), _p(pixels), *cfg[:4], _p(jitter), Nr, Nb, *cfg[4:])
    grads = (_p(d_xyz), _p(d_viewdir), _p(d_z), _p(d_cam2obj), _p(ws), n_ws)
    with torch.cuda.device(dev):
        if hit_scan:
            check(_lib.lib().snr_scene_samples_compact_bwd(*lists, _p(hit_scan[0]), cap, *grads, _stream(dev)), "snr_scene_samples_compact_bwd")
        else:
            check(_lib.lib().snr_scene_samples_bwd(*lists, *grads, _stream(dev)), "snr_scene_samples_bwd")
    return (d_cam2obj,) + (None,) * (n_inputs - 1)


class SceneSamples(torch.autograd.Function):
    """Rays, bounds and samples of every (pixel, object) pair of a scene in one launch (snr_scene_samples_fwd; rules: include/supnerf_hip.h):
    cam2obj (Nb,3,4) [differentiable], wlh (Nb,3), rois (Nb,4) int32, pixels (Nr,2) int32, Kvec = (fx, fy, cx, cy) host numbers, jitter
    (Nr*Nb,S) or None -> xyz, viewdir (Nb*Nr,S,3) object-major, z_vals (Nr,Nb*S) pixel-major, hit (Nr,Nb) uint8, valid (Nr) uint8.
    Backward to cam2obj: two launches, the same bits from run to run."""

    @staticmethod
    def forward(ctx, cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale, rend_aabb, shapenet_obj_cood):
        return _scene_samples_fwd(ctx, "scene_samples", cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale, rend_aabb, shapenet_obj_cood)

    @staticmethod
    def backward(ctx, d_xyz, d_viewdir, d_z, _d_hit, _d_valid):
        return _scene_samples_bwd(ctx, "scene_samples", 10, d_xyz, d_viewdir, d_z)


def _scene_gather_fwd(ctx, sigmas, rgbs, flag, S, hit_scan=None, pair_of_slot=None):
    """Forward of ``SceneGather`` (``flag`` = hit) and, with ``hit_scan`` and ``pair_of_slot``, of ``SceneGatherCompact`` (``flag`` = kept): the
    decoder's Nb*R*S values, R = Nr or C -> rows (Nr,Nb*S) / (Nr,Nb*S,3)."""
    compact = pair_of_slot is not None
    sigmas, rgbs = _f32c(sigmas), _f32c(rgbs)
    S = int(S)
    ok = flag.dim() == 2 and flag.dtype == torch.uint8 and S >= 1 and (not compact or (pair_of_slot.dim() == 2 and pair_of_slot.dtype == torch.int32))
    if ok:
        Nr, Nb = flag.shape
        R = pair_of_slot.shape[1] if compact else Nr
        ok = (not compact or (pair_of_slot.shape[0] == Nb and Nb >= 1)) and sigmas.numel() == Nb * R * S and rgbs.numel() == 3 * sigmas.numel()
    if not ok and compact:
        raise SnrError(f"scene_gather_compact: expected sigmas (Nb*C*S), rgbs (Nb*C*S,3), kept (Nr,Nb) uint8 and pair_of_slot (Nb,C) int32, got "
                       f"{tuple(sigmas.shape)}, {tuple(rgbs.shape)}, {tuple(flag.shape)} {flag.dtype}, {tuple(pair_of_slot.shape)} "
                       f"{pair_of_slot.dtype}, S = {S}")
    if not ok:
        raise SnrError(f"scene_gather: expected sigmas (Nb*Nr*S), rgbs (Nb*Nr*S,3) and hit (Nr,Nb) uint8, got {tuple(sigmas.shape)}, "
                       f"{tuple(rgbs.shape)}, {tuple(flag.shape)} {flag.dtype}, S = {S}")
    if compact:
        cap = _scene_capacity_arg("scene_gather_compact", R)
        hit_scan = _scene_scan("scene_gather_compact", hit_scan, Nr, Nb)
        pair_of_slot = pair_of_slot.contiguous()
    _need_gpu(sigmas, rgbs, hit_scan, flag, pair_of_slot)
    flag = flag.contiguous()
    dev = sigmas.device
    ctx.set_materialize_grads(False)
    sig_rows, rgb_rows = torch.empty(Nr, Nb * S, device=dev), torch.empty(Nr, Nb * S, 3, device=dev)
    with torch.cuda.device(dev):
        if compact:
            check(_lib.lib().snr_scene_gather_compact_fwd(_p(sigmas), _p(rgbs), _p(hit_scan), _p(flag), Nr, Nb, S, cap, _p(sig_rows), _p(rgb_rows),
                                                          _stream(dev)), "snr_scene_gather_compact_fwd")
        else:
            check(_lib.lib().snr_scene_gather_fwd(_p(sigmas), _p(rgbs), _p(flag), Nr, Nb, S, _p(sig_rows), _p(rgb_rows), _stream(dev)),
                  "snr_scene_gather_fwd")
    ctx.save_for_backward(pair_of_slot if compact else flag)
    ctx.cfg = (S, Nr, sigmas.shape, rgbs.shape)
    return sig_rows, rgb_rows


def _scene_gather_bwd(ctx, d_sig_rows, d_rgb_rows, compact):
    """Backward of both gather classes: the inverse scatter through the saved hit (Nr,Nb) or, ``compact``, pair_of_slot (Nb,C)."""
    saved, = ctx.saved_tensors
    S, Nr, sig_shape, rgb_shape = ctx.cfg
    Nb = saved.shape[0 if compact else 1]
    dev = saved.device
    d_sig_rows = _f32c(d_sig_rows) if ctx.needs_input_grad[0] else None          # NAMED, as in composite_bwd
    d_rgb_rows = _f32c(d_rgb_rows) if ctx.needs_input_grad[1] else None
    d_sig = torch.empty(sig_shape, device=dev) if d_sig_rows is not None else None
    d_rgb = torch.empty(rgb_shape, device=dev) if d_rgb_rows is not None else None
    if d_sig is not None or d_rgb is not None:
        with torch.cuda.device(dev):
            if compact:
                check(_lib.lib().snr_scene_gather_compact_bwd(_p(d_sig_rows), _p(d_rgb_rows), _p(saved), Nr, Nb, S, saved.shape[1], _p(d_sig),
                                                              _p(d_rgb), _stream(dev)), "snr_scene_gather_compact_bwd")
            else:
                check(_lib.lib().snr_scene_gather_bwd(_p(d_sig_rows), _p(d_rgb_rows), _p(saved), Nr, Nb, S, _p(d_sig), _p(d_rgb), _stream(dev)),
                      "snr_scene_gather_bwd")
    return d_sig, d_rgb


class SceneGather(torch.autograd.Function):
    """The decoder's object-major sigmas (Nb*Nr*S values) and rgbs (Nb*Nr*S,3) as the composite's pixel-major rows (Nr,Nb*S) / (Nr,Nb*S,3),
    sigma 0 and white where ``hit`` (Nr,Nb) uint8 is 0: the permutes and ``torch.where`` of ``scene.render_scene_batch`` in one launch, bit for
    bit; backward the inverse scatter in one launch."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, hit, S):
        return _scene_gather_fwd(ctx, sigmas, rgbs, hit, S)

    @staticmethod
    def backward(ctx, d_sig_rows, d_rgb_rows):
        return (*_scene_gather_bwd(ctx, d_sig_rows, d_rgb_rows, False), None, None)


def scene_capacity(n) -> int:
    """Slots per object of the compact scene route that hold ``n`` pairs: ``n`` rounded up to a multiple of 32 (whole decoder tiles for every
    sample count), at least 32."""
    return max(WAVE_TILE, _tile_pad(int(n)) or int(n))


def _scene_capacity_arg(name, capacity):
    try:
        cap = None if isinstance(capacity, bool) else operator.index(capacity)
    except TypeError:
        cap = None
    if cap is None or cap < 1 or cap % WAVE_TILE != 0:
        raise SnrError(f"{name}: capacity is a positive multiple of 32 (ops.scene_capacity), got {capacity!r}")
    return cap


def _scene_scan(name, hit_scan, Nr, Nb):
    if hit_scan.shape != (Nr, Nb) or hit_scan.dtype != torch.int32:
        raise SnrError(f"{name}: expected hit_scan (Nr,Nb) = ({Nr},{Nb}) int32, got {tuple(hit_scan.shape)} {hit_scan.dtype}")
    return hit_scan.contiguous()


def scene_pair_hits(cam2obj, wlh, rois, pixels, Kvec, rend_aabb=True):
    """hit (Nr,Nb) uint8 of every (pixel, object) pair, the flags of ``SceneSamples`` without its samples (snr_scene_pair_hits): what the
    compact route scans, ``torch.cumsum(hit.to(torch.int32), 0)``."""
    cam2obj, wlh = _f32c(cam2obj.detach()), _f32c(wlh)
    Nr, Nb = _scene_lists("scene_pair_hits", cam2obj, wlh, rois, pixels, None, 1)
    if len(Kvec) != 4:
        raise SnrError("scene_pair_hits: Kvec is (fx, fy, cx, cy)")
    _need_gpu(cam2obj, wlh, rois, pixels)
    rois, pixels = rois.contiguous(), pixels.contiguous()
    dev = cam2obj.device
    hit = torch.empty(Nr, Nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_scene_pair_hits(_p(cam2obj), _p(wlh), _p(rois), _p(pixels), *[float(v) for v in Kvec], Nr, Nb, int(bool(rend_aabb)),
                                             _p(hit), _stream(dev)), "snr_scene_pair_hits")
    return hit


class SceneSamplesCompact(torch.autograd.Function):
    """``SceneSamples`` with only the pairs that hit handed on (snr_scene_samples_compact_fwd; rules: include/supnerf_hip.h): ``hit_scan``
    (Nr,Nb) int32 = ``torch.cumsum`` of ``scene_pair_hits`` along the pixels, ``capacity`` C slots per object (``scene_capacity``) -> xyz,
    viewdir (Nb*C,S,3), a pair at row b*C + hit_scan - 1; z_vals (Nr,Nb*S) pixel-major and dense, -1 on pairs that are not kept; kept (Nr,Nb)
    uint8; pair_of_slot (Nb,C) int32, -1 on padding.  A hit pair beyond the capacity is dropped.  Backward to cam2obj: two launches, the
    bits of ``SceneSamples``' backward."""

    @staticmethod
    def forward(ctx, cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale, rend_aabb, shapenet_obj_cood, hit_scan, capacity):
        return _scene_samples_fwd(ctx, "scene_samples_compact", cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale, rend_aabb, shapenet_obj_cood,
                                  hit_scan, capacity)

    @staticmethod
    def backward(ctx, d_xyz, d_viewdir, d_z, _d_kept, _d_slots):
        return _scene_samples_bwd(ctx, "scene_samples_compact", 12, d_xyz, d_viewdir, d_z)


class SceneGatherCompact(torch.autograd.Function):
    """``SceneGather`` from the compact layout: sigmas (Nb*C*S values) and rgbs (Nb*C*S,3) of the decoder -> rows (Nr,Nb*S) / (Nr,Nb*S,3), a
    kept pair's rows from its slot (``hit_scan`` - 1), sigma 0 and white on every other pair; backward through ``pair_of_slot`` (Nb,C), exact
    zeros on padding slots.  ``hit_scan``, ``kept`` and ``pair_of_slot`` as ``SceneSamplesCompact`` took and gave them."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, hit_scan, kept, pair_of_slot, S):
        return _scene_gather_fwd(ctx, sigmas, rgbs, kept, S, hit_scan, pair_of_slot)

    @staticmethod
    def backward(ctx, d_sig_rows, d_rgb_rows):
        return (*_scene_gather_bwd(ctx, d_sig_rows, d_rgb_rows, True), None, None, None, None)


def composite_bwd(sigmas, rgbs, z_vals, z_mode, white_bkgd, rays_per_obj, d_rgb, d_depth, d_acc, need_dz):
    sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
    # dense copies are NAMED so that they live until the launch is enqueued: `_p(_f32c(t))` inside the argument list frees the temporary before
    # the next argument is evaluated, and the allocator hands the same block to the next temporary (found by tests/test_strided_operands.py)
    d_rgb, d_depth, d_acc = _f32c(d_rgb), _f32c(d_depth), _f32c(d_acc)
    n_rays, S = _composite_shapes("composite_bwd", sigmas, rgbs, z_vals, z_mode, rays_per_obj, grads=(d_rgb, d_depth, d_acc))
    _need_gpu(sigmas, rgbs, z_vals, d_rgb, d_depth, d_acc)
    dev = rgbs.device
    d_sig = torch.empty(n_rays, S, device=dev)
    d_rgbs = torch.empty(n_rays, S, 3, device=dev)
    d_z = torch.empty(n_rays, S, device=dev) if need_dz else None
    with torch.cuda.device(dev):
        check(_lib.lib().snr_composite_bwd(_p(sigmas), _p(rgbs), _p(z_vals), z_mode, WHITE_BKGD if white_bkgd else 0, n_rays,
                                           rays_per_obj, S, _p(d_rgb), _p(d_depth), _p(d_acc),
                                           _p(d_sig), _p(d_rgbs), _p(d_z), _stream(dev)), "snr_composite_bwd")
    return d_sig, d_rgbs, d_z


class Composite(torch.autograd.Function):
    """Alpha composite of (N,S) densities / (N,S,3) colours; z per z_mode.  Gradients flow to sigmas and
    rgbs always and to z_vals when it is per-ray (family B keeps its box bounds differentiable)."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, z_vals, z_mode, white_bkgd, rays_per_obj):
        sigmas, rgbs, z_vals = _f32c(sigmas), _f32c(rgbs), _f32c(z_vals)
        out = composite_fwd(sigmas, rgbs, z_vals, z_mode, white_bkgd, rays_per_obj)
        ctx.save_for_backward(sigmas, rgbs, z_vals)
        ctx.cfg = (z_mode, white_bkgd, rays_per_obj)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_acc):
        sigmas, rgbs, z_vals = ctx.saved_tensors
        z_mode, white, rpo = ctx.cfg
        need_dz = ctx.needs_input_grad[2]
        if need_dz and z_mode != Z_PER_RAY:
            raise SnrError("gradient wrt shared / per-object z_vals is not provided (the reference detaches them, "
                           "src/utils.py:468-469)")
        d_sig, d_rgbs, d_z = composite_bwd(sigmas, rgbs, z_vals, z_mode, white, rpo, d_rgb, d_depth, d_acc, need_dz)
        return d_sig.view(sigmas.shape), d_rgbs.view(rgbs.shape), (d_z.view(z_vals.shape) if need_dz else None), None, None, None


# ------------------------------------------------------------------------------------ loss / metric tail
def loss_tail_fwd(rgb, acc, rgb_tgt, occ, loss_occ_coef, rays_per_obj):
    """(B,4) = [loss, loss_rgb, loss_occ, mse_fg] per object (src/optimizer_nuscenes.py:729-744), one launch."""
    rgb, acc, rgb_tgt, occ = _f32c(rgb), _f32c(acc), _f32c(rgb_tgt), _f32c(occ)
    _need_gpu(rgb, acc, rgb_tgt, occ)
    n = acc.numel()
    if rgb.numel() != 3 * n or rgb_tgt.numel() != 3 * n or occ.numel() != n or rays_per_obj < 1 or n % rays_per_obj:
        raise SnrError(f"loss_tail: rgb {tuple(rgb.shape)}, acc {tuple(acc.shape)}, rgb_tgt {tuple(rgb_tgt.shape)}, occ {tuple(occ.shape)} "
                       f"do not describe whole objects of {rays_per_obj} rays")
    dev = rgb.device
    out = torch.empty(n // rays_per_obj, 4, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_loss_tail_fwd(_p(rgb), _p(acc), _p(rgb_tgt), _p(occ), n, rays_per_obj, float(loss_occ_coef), _p(out), _stream(dev)),
              "snr_loss_tail_fwd")
    return out


class LossTail(torch.autograd.Function):
    """loss (B,) [differentiable wrt rgb and acc_trans] and metrics (B,3) = [loss_rgb, loss_occ, mse_fg] [not differentiable] of the
    optimise iteration.  Backward is one launch that writes the seeds of the render backward."""

    @staticmethod
    def forward(ctx, rgb, acc, rgb_tgt, occ, loss_occ_coef, rays_per_obj):
        rgb, acc, rgb_tgt, occ = _f32c(rgb), _f32c(acc), _f32c(rgb_tgt), _f32c(occ)
        ctx.set_materialize_grads(False)        # (no zero tensors for outputs nobody differentiated: each would be a fill launch)
        out = loss_tail_fwd(rgb, acc, rgb_tgt, occ, loss_occ_coef, rays_per_obj)
        ctx.save_for_backward(rgb, acc, rgb_tgt, occ)
        ctx.cfg = (float(loss_occ_coef), int(rays_per_obj))
        loss, metrics = out[:, 0].contiguous(), out[:, 1:].contiguous()
        ctx.mark_non_differentiable(metrics)
        return loss, metrics

    @staticmethod
    def backward(ctx, g_loss, _g_metrics):
        rgb, acc, rgb_tgt, occ = ctx.saved_tensors
        coef, rpo = ctx.cfg
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            raise SnrError("loss_tail: the targets and occupancy labels are data, no gradient is provided")
        dev = rgb.device
        if g_loss is None:
            return None, None, None, None, None, None
        d_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        d_acc = torch.empty_like(acc) if ctx.needs_input_grad[1] else None
        if d_rgb is not None or d_acc is not None:
            g_loss = _f32c(g_loss)
            with torch.cuda.device(dev):
                check(_lib.lib().snr_loss_tail_bwd(_p(rgb), _p(acc), _p(rgb_tgt), _p(occ), acc.numel(), rpo, coef, _p(g_loss),
                                                   _p(d_rgb), _p(d_acc), _stream(dev)), "snr_loss_tail_bwd")
        return d_rgb, d_acc, None, None, None, None


# ------------------------------------------------------------------------------------ the rest of an optimise iteration
class PoseRays(torch.autograd.Function):
    """Pose parameters -> camera-in-object pose, rays of the pixel grid, stratified depths, in one launch for B objects
    (src/optimizer_nuscenes.py:685-699 + get_rays + the sphere bounds + sample_from_rays' depth vector); backward in one launch.
    rot_vec, trans_vec (B,3); cam_dirs (B,n,3); half_diag (B,); jitter (B,S) or None
    -> cam2opt (B,3,4), rays_o (B*n,3), viewdir (B*n,3), z_vals (B,S) [detached from the pose like the reference's]."""

    @staticmethod
    def forward(ctx, rot_vec, trans_vec, cam_dirs, half_diag, jitter, n_samples, opt_cam_pose):
        rot_vec, trans_vec, cam_dirs, half_diag, jitter = [_f32c(t) for t in (rot_vec, trans_vec, cam_dirs, half_diag, jitter)]
        _need_gpu(rot_vec, trans_vec, cam_dirs, half_diag, jitter)
        B, n = cam_dirs.shape[0], cam_dirs.shape[1]
        if rot_vec.shape != (B, 3) or trans_vec.shape != (B, 3) or half_diag.numel() != B or (jitter is not None and jitter.shape != (B, n_samples)):
            raise SnrError("pose_rays: expected rot_vec / trans_vec (B,3), cam_dirs (B,n,3), half_diag (B,), jitter (B,S)")
        dev = cam_dirs.device
        ctx.set_materialize_grads(False)        # (the kernel takes null for the gradients of outputs that were not used)
        cam2opt = torch.empty(B, 3, 4, device=dev)
        rays_o, viewdir = torch.empty(B * n, 3, device=dev), torch.empty(B * n, 3, device=dev)
        z = torch.empty(B, n_samples, device=dev)
        with torch.cuda.device(dev):
            check(_lib.lib().snr_pose_rays_fwd(_p(rot_vec), _p(trans_vec), _p(cam_dirs), _p(half_diag), _p(jitter), B, n, int(n_samples),
                                               int(bool(opt_cam_pose)), _p(cam2opt), _p(rays_o), _p(viewdir), _p(z), _stream(dev)), "snr_pose_rays_fwd")
        ctx.save_for_backward(rot_vec, trans_vec, cam_dirs)
        ctx.opt_cam_pose = int(bool(opt_cam_pose))
        ctx.mark_non_differentiable(z)
        return cam2opt, rays_o, viewdir, z

    @staticmethod
    def backward(ctx, d_cam2opt, d_rays_o, d_viewdir, _d_z):
        rot_vec, trans_vec, cam_dirs = ctx.saved_tensors
        if ctx.needs_input_grad[2]:
            raise SnrError("pose_rays: the pixel direction table is data, no gradient is provided")
        B, n = cam_dirs.shape[0], cam_dirs.shape[1]
        dev = cam_dirs.device
        d_rot, d_tr = torch.empty_like(rot_vec), torch.empty_like(trans_vec)
        d_rays_o, d_viewdir, d_cam2opt = _f32c(d_rays_o), _f32c(d_viewdir), _f32c(d_cam2opt)
        with torch.cuda.device(dev):
            check(_lib.lib().snr_pose_rays_bwd(_p(rot_vec), _p(trans_vec), _p(cam_dirs), B, n, ctx.opt_cam_pose, _p(d_rays_o),
                                               _p(d_viewdir), _p(d_cam2opt), _p(d_rot), _p(d_tr), _stream(dev)), "snr_pose_rays_bwd")
        return d_rot, d_tr, None, None, None, None, None


class CamRays(torch.autograd.Function):
    """Camera pose -> rays of a pixel table (+ the stratified depth vector), one launch; backward one launch.  What the public
    ``get_rays`` / ``render_rays_v2`` need per call (src/utils.py:107-135,159-164,468-469) when the pose lives on the GPU.
    c2w (B,3,4); cam_dirs (B,n,3) = [(px-cx)/fx, (py-cy)/fy, 1]; half_diag (B,) or None; jitter (B,S) or None
    -> rays_o (B*n,3), viewdir (B*n,3), z_vals (B,S) [None when half_diag is None; detached from the pose like the reference's]."""

    @staticmethod
    def forward(ctx, c2w, cam_dirs, half_diag, jitter, n_samples):
        c2w, cam_dirs, half_diag, jitter = [_f32c(t) for t in (c2w, cam_dirs, half_diag, jitter)]
        _need_gpu(c2w, cam_dirs, half_diag, jitter)
        B, n = cam_dirs.shape[0], cam_dirs.shape[1]
        if c2w.shape != (B, 3, 4) or cam_dirs.shape[-1] != 3 or (half_diag is not None and half_diag.numel() != B) or \
                (jitter is not None and jitter.shape != (B, n_samples)):
            raise SnrError("cam_rays: expected c2w (B,3,4), cam_dirs (B,n,3), half_diag (B,), jitter (B,S)")
        dev = cam_dirs.device
        ctx.set_materialize_grads(False)
        rays_o, viewdir = torch.empty(B * n, 3, device=dev), torch.empty(B * n, 3, device=dev)
        z = torch.empty(B, n_samples, device=dev) if half_diag is not None else None
        with torch.cuda.device(dev):
            check(_lib.lib().snr_cam_rays_fwd(_p(c2w), _p(cam_dirs), _p(half_diag), _p(jitter), B, n, int(n_samples), _p(rays_o), _p(viewdir), _p(z),
                                              _stream(dev)), "snr_cam_rays_fwd")
        ctx.save_for_backward(c2w, cam_dirs)
        if z is not None:
            ctx.mark_non_differentiable(z)
        return rays_o, viewdir, z

    @staticmethod
    def backward(ctx, d_rays_o, d_viewdir, _d_z):
        c2w, cam_dirs = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise SnrError("cam_rays: the pixel direction table is data, no gradient is provided")
        if d_rays_o is None and d_viewdir is None:
            return None, None, None, None, None
        B, n = cam_dirs.shape[0], cam_dirs.shape[1]
        dev = cam_dirs.device
        d_rays_o, d_viewdir = _f32c(d_rays_o), _f32c(d_viewdir)
        d_c2w = torch.empty_like(c2w)
        with torch.cuda.device(dev):
            check(_lib.lib().snr_cam_rays_bwd(_p(c2w), _p(cam_dirs), B, n, _p(d_rays_o), _p(d_viewdir), _p(d_c2w), _stream(dev)), "snr_cam_rays_bwd")
        return d_c2w, None, None, None, None


def metric_row(loss_out, depth_pred, depth0, first, cam2opt, gt_R, gt_T, opt_cam_pose, row, lidar_count=None):
    """row (B,4) <- [PSNR, depth error over each object's first ``lidar_count`` pixels, rotation error, translation error]
    (src/optimizer_nuscenes.py:739-765); depth0 = the measured depths (first = False) or a buffer that receives the rendered depths of
    the first iteration (first = True)."""
    _need_gpu(loss_out, depth_pred, depth0, cam2opt, gt_R, gt_T, row, lidar_count)
    B = cam2opt.shape[0]
    n_lidar = depth_pred.shape[-1] if depth_pred is not None else 0
    for t in (loss_out, depth_pred, depth0, cam2opt, gt_R, gt_T, row):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise SnrError("metric_row: fp32 contiguous tensors expected")
    if lidar_count is not None and (lidar_count.dtype != torch.int32 or lidar_count.numel() != B or not lidar_count.is_contiguous()):
        raise SnrError("metric_row: lidar_count must be a contiguous int32 (B,) tensor")
    if n_lidar and (depth_pred.numel() != B * n_lidar or depth0 is None or depth0.numel() != B * n_lidar):
        raise SnrError("metric_row: depth_pred / depth0 must both be (B, n_lidar)")
    dev = cam2opt.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_metric_row(_p(loss_out), _p(depth_pred), _p(depth0), int(n_lidar), int(bool(first)), _p(cam2opt), _p(gt_R), _p(gt_T),
                                        B, int(bool(opt_cam_pose)), _p(row), C.c_void_p(0 if lidar_count is None else lidar_count.data_ptr()),
                                        _stream(dev)), "snr_metric_row")
    return row


class DeviceAdamW:
    """torch.optim.AdamW's update (amsgrad off, same defaults) for up to 4 parameter groups as ONE launch per step
    (src/optimizer_nuscenes.py:1762-1769).  ``groups``: [(parameter tensor, lr), ...]; gradients are read from ``.grad``."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not 1 <= len(groups) <= 4:
            raise SnrError("DeviceAdamW: 1 to 4 parameter groups")
        self.params = [p for p, _ in groups]
        self.lr = [float(lr) for _, lr in groups]
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise SnrError("DeviceAdamW: fp32 contiguous parameters on the GPU")
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.steps = 0

    def restart(self, scale: float = 1.0):
        """What re-creating the optimiser does (src/optimizer_nuscenes.py:1771-1775): fresh moments and step count, rates times ``scale``."""
        self.lr = [v * scale for v in self.lr]
        for t in self.exp_avg + self.exp_avg_sq:
            t.zero_()
        self.steps = 0

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        n = len(self.params)
        grads = []
        for p in self.params:
            if p.grad is None:
                raise SnrError("DeviceAdamW.step: a parameter has no gradient")
            grads.append(_f32c(p.grad))
        self.steps += 1
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        numel = (C.c_int64 * n)(*[p.numel() for p in self.params])
        lr = (C.c_float * n)(*self.lr)
        dev = self.params[0].device
        with torch.cuda.device(dev):
            check(_lib.lib().snr_adamw_step(arr([p.data for p in self.params]), arr(grads), arr(self.exp_avg), arr(self.exp_avg_sq), numel, lr, n, self.steps,
                                            self.betas[0], self.betas[1], self.eps, self.weight_decay, _stream(dev)), "snr_adamw_step")


class LatentLayers(torch.autograd.Function):
    """The per-object latent layers of a FROZEN decoder (src/model_supnerf.py:253,261) and the biases their outputs fold into, one launch;
    backward to the two codes one launch.  shapecode, texturecode (B,256); w_lat, b_lat, w_nxt, b_nxt: ``model._stacked()``.
    -> z (B, n_lat, 256), latent_bias (B, n_lat, 256) [no gradient: the render backward returns the gradient of z itself]."""

    @staticmethod
    def forward(ctx, shapecode, texturecode, w_lat, b_lat, w_nxt, b_nxt, shape_blocks, texture_blocks):
        shapecode, texturecode = _f32c(shapecode), _f32c(texturecode)
        _need_gpu(shapecode, texturecode, w_lat, b_lat, w_nxt, b_nxt)
        n_lat, B, dev = shape_blocks + texture_blocks, shapecode.shape[0], shapecode.device
        if shapecode.shape != (B, 256) or texturecode.shape != (B, 256) or w_lat.shape != (512, n_lat * 256) or w_nxt.shape != (n_lat * 256, n_lat * 256) \
                or b_lat.numel() != n_lat * 256 or b_nxt.numel() != n_lat * 256:
            raise SnrError("latent_layers: expected codes (B,256), w_lat (512, n_lat*256), w_nxt (n_lat*256, n_lat*256), biases (n_lat*256)")
        z, lb = torch.empty(B, n_lat, 256, device=dev), torch.empty(B, n_lat, 256, device=dev)
        with torch.cuda.device(dev):
            check(_lib.lib().snr_latent_fwd(_p(shapecode), _p(texturecode), _p(w_lat), _p(b_lat), _p(w_nxt), _p(b_nxt), B, int(shape_blocks),
                                            int(texture_blocks), _p(z), _p(lb), _stream(dev)), "snr_latent_fwd")
        ctx.save_for_backward(z, w_lat)
        ctx.blocks = (int(shape_blocks), int(texture_blocks))
        ctx.mark_non_differentiable(lb)
        ctx.set_materialize_grads(False)
        return z, lb

    @staticmethod
    def backward(ctx, d_z, _d_lb):
        z, w_lat = ctx.saved_tensors
        if d_z is None:
            return (None,) * 8
        if any(ctx.needs_input_grad[2:6]):
            raise SnrError("latent_layers: the stacked weights are constants here (training mode runs the per-layer torch form)")
        sb, tb = ctx.blocks
        B, dev = z.shape[0], z.device
        d_z = _f32c(d_z)
        d_sc = torch.empty(B, 256, device=dev) if ctx.needs_input_grad[0] else None
        d_tc = torch.empty(B, 256, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            check(_lib.lib().snr_latent_bwd(_p(d_z), _p(z), _p(w_lat), B, sb, tb, _p(d_sc), _p(d_tc), _stream(dev)), "snr_latent_bwd")
        return d_sc, d_tc, None, None, None, None, None, None


# ------------------------------------------------------------------------------------ several views of one instance (csrc/snr_views.hip)
def view_pixels(img_cat, occ_cat, crop_offset, roi, Kvec, picks):
    """One iteration's random pixels of V views' native-resolution rois (``render_rays``, src/utils.py:380-432), one launch, no host read.
    img_cat (sum h w, 3), occ_cat (sum h w): the views' crops, row-major, concatenated; crop_offset (V+1,) int64 pixel offsets;
    roi (V,4) int32 x0 y0 x1 y1; Kvec (V,4) fx fy cx cy; picks (V,n) int32 = y w + x into the view's crop, -1 (or anything outside
    [0, h w)) = a padding ray -> cam_dirs (V,n,3) = [(x-cx)/fx, (y-cy)/fy, 1], rgb_tgt (V,n,3), occ (V,n); padding rays get (0,0,1), 0, 0,
    and occ = 0 is a zero weight in every sum of ``LossTail``.  All inputs are data: no gradient."""
    _need_gpu(img_cat, occ_cat, crop_offset, roi, Kvec, picks)
    for t in (img_cat, occ_cat, Kvec):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise SnrError("view_pixels: img_cat, occ_cat and Kvec must be fp32 contiguous tensors")
    if crop_offset.dtype != torch.int64 or not crop_offset.is_contiguous() or crop_offset.dim() != 1 or crop_offset.numel() < 1:
        raise SnrError("view_pixels: crop_offset must be a contiguous int64 (V+1,) tensor")
    V = crop_offset.numel() - 1
    for t, name in ((roi, "roi"), (picks, "picks")):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise SnrError(f"view_pixels: {name} must be a contiguous int32 tensor")
    if tuple(roi.shape) != (V, 4) or tuple(Kvec.shape) != (V, 4) or picks.dim() != 2 or picks.shape[0] != V:
        raise SnrError(f"view_pixels: expected roi (V,4), Kvec (V,4), picks (V,n) for the V = {V} views of crop_offset, got {tuple(roi.shape)}, "
                       f"{tuple(Kvec.shape)}, {tuple(picks.shape)}")
    if occ_cat.dim() != 1 or img_cat.numel() != 3 * occ_cat.numel():
        raise SnrError(f"view_pixels: img_cat {tuple(img_cat.shape)} and occ_cat {tuple(occ_cat.shape)} must be (P,3) and (P,)")
    dev = picks.device
    if any(t.device != dev for t in (img_cat, occ_cat, crop_offset, roi, Kvec)):
        raise SnrError("view_pixels: all tensors on one GPU")
    n = picks.shape[1]
    cam_dirs, rgb_tgt, occ = torch.empty(V, n, 3, device=dev), torch.empty(V, n, 3, device=dev), torch.empty(V, n, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_view_pixels(_p(img_cat), _p(occ_cat), _p(crop_offset), _p(roi), _p(Kvec), _p(picks), V, n, _p(cam_dirs), _p(rgb_tgt),
                                         _p(occ), _stream(dev)), "snr_view_pixels")
    return cam_dirs, rgb_tgt, occ


def view_offset_of(view_counts) -> Tuple[int, ...]:
    """(I+1,) offsets of I instances' contiguous views from their view counts; an instance without a view raises."""
    counts = [int(c) for c in view_counts]
    if not counts or any(c < 1 for c in counts):
        raise SnrError(f"every instance needs at least one view, got view counts {counts}")
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return tuple(off)


@functools.lru_cache(maxsize=32)
def _view_offset_on(offsets: Tuple[int, ...], dev_str: str) -> torch.Tensor:
    return torch.tensor(offsets, dtype=torch.int64).to(torch.device(dev_str))


def _view_offset_args(view_offset, n_instances, dev):
    """The relation is host knowledge: checked here, before any launch; its device copy is made once per (offsets, device)."""
    off = tuple(int(v) for v in (view_offset.tolist() if isinstance(view_offset, torch.Tensor) else view_offset))
    if len(off) != n_instances + 1 or off[0] != 0:
        raise SnrError(f"instance_rows: view_offset must hold I + 1 = {n_instances + 1} offsets starting at 0, got {off}")
    if any(b <= a for a, b in zip(off, off[1:])):
        raise SnrError(f"instance_rows: an instance without a view (view_offset {off})")
    return off, _view_offset_on(off, str(dev)), (C.c_int64 * len(off))(*off)


def instance_rows_fwd(rows, view_offset):
    """rows (I,...) -> (V,...): row v is the row of v's instance (``view_offset`` (I+1,): a host sequence or CPU tensor)."""
    rows = _f32c(rows)
    _need_gpu(rows)
    n_inst = rows.shape[0]
    off, off_d, off_h = _view_offset_args(view_offset, n_inst, rows.device)
    n_cols = rows.numel() // n_inst if n_inst else 0
    if n_cols < 1:
        raise SnrError(f"instance_rows: rows {tuple(rows.shape)} have no column")
    out = torch.empty(off[-1], *rows.shape[1:], device=rows.device)
    with torch.cuda.device(rows.device):
        check(_lib.lib().snr_instance_rows_fwd(_p(rows), _p(off_d), off_h, n_inst, off[-1], n_cols, _p(out),
                                               _stream(rows.device)), "snr_instance_rows_fwd")
    return out


class InstanceRows(torch.autograd.Function):
    """The views of an instance share its row: rows (I,...,256), view_offset (I+1,) [host] -> (V,...,256), row v a copy of its instance's.
    Backward: the gradient of row i is the sum of its views' gradients in ASCENDING view order, plain fp32 adds from the first term, one
    thread per element -- no atomics (torch's ``index_select`` backward is an atomic ``index_add``), the same bits every run."""

    @staticmethod
    def forward(ctx, rows, view_offset):
        ctx.set_materialize_grads(False)
        ctx.view_offset, ctx.shape = view_offset, tuple(rows.shape)
        return instance_rows_fwd(rows, view_offset)

    @staticmethod
    def backward(ctx, d_out):
        if d_out is None:
            return None, None
        d_out = _f32c(d_out)
        n_inst = ctx.shape[0]
        off, off_d, off_h = _view_offset_args(ctx.view_offset, n_inst, d_out.device)
        d_rows = torch.empty(ctx.shape, device=d_out.device)
        with torch.cuda.device(d_out.device):
            check(_lib.lib().snr_instance_rows_bwd(_p(d_out), _p(off_d), off_h, n_inst, off[-1],
                                                   d_rows.numel() // n_inst, _p(d_rows), _stream(d_out.device)), "snr_instance_rows_bwd")
        return d_rows, None


# ------------------------------------------------------------------------------------ cross-view evaluation (csrc/snr_cross.hip)
def cross_pairs(view_offset, n_snapshots):
    """The (code row, target view) pairs of ``eval_cross_view`` (src/optimizer_nuscenes.py:1322-1335), built on the host: for every
    instance, every snapshot c, every view ii whose codes are rendered and every view num that is rendered -- in that order -- the row
    ``[c V + ii, num]``: the code row indexes the flattened (C V) code rows, views instance-major.  Returns pairs (P,2) int32 and the
    (I+1,) int64 offsets of every instance's pairs (instance i owns C V_i^2 of them)."""
    off = [int(v) for v in (view_offset.tolist() if isinstance(view_offset, torch.Tensor) else view_offset)]
    n_snap = int(n_snapshots)
    if len(off) < 2 or off[0] != 0 or any(b <= a for a, b in zip(off, off[1:])) or n_snap < 1:
        raise SnrError(f"cross_pairs: view_offset must hold I + 1 strictly ascending offsets starting at 0 and n_snapshots >= 1, got {off}, {n_snap}")
    V = off[-1]
    rows, pair_off = [], [0]
    for v0, v1 in zip(off, off[1:]):
        views = torch.arange(v0, v1, dtype=torch.int32)
        code = (torch.arange(n_snap, dtype=torch.int32)[:, None, None] * V + views[None, :, None]).expand(n_snap, v1 - v0, v1 - v0)
        rows.append(torch.stack([code, views[None, None, :].expand_as(code)], dim=-1).reshape(-1, 2))
        pair_off.append(pair_off[-1] + rows[-1].shape[0])
    return torch.cat(rows).contiguous(), torch.tensor(pair_off, dtype=torch.int64)


def cross_metrics(rgb, depth_pred, tgt, occ, lid_depth, lid_cnt, pairs, n_codes=None):
    """(P,3) = [mse_fg, depth_err, sum |occ|] of P rendered (code row, target view) pairs, one launch (``snr_cross_metrics``).
    rgb (P,n,3), depth_pred (P,n_l): the pairs' renders; tgt (V,n,3), occ (V,n), lid_depth (V,n_l), lid_cnt (V,) int32: the V views'
    targets, labels, measured depths and lidar counts, read through the pair's target view; pairs (P,2) int32 (a CPU tensor is uploaded;
    a GPU tensor is read back once for the host check); ``n_codes``: the number of code rows the pairs index, checked on the host
    (default: whatever the table spans).  n_l = 0: depth_err = 0."""
    _need_gpu(rgb, depth_pred, tgt, occ, lid_depth, lid_cnt)
    for t in (rgb, depth_pred, tgt, occ, lid_depth):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise SnrError("cross_metrics: rgb, depth_pred, tgt, occ and lid_depth must be fp32 contiguous tensors")
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
        raise SnrError(f"cross_metrics: pairs must be an int32 (P,2) tensor with P >= 1, got {pairs.dtype} {tuple(pairs.shape)}")
    P = pairs.shape[0]
    if rgb.dim() != 3 or rgb.shape[0] != P or rgb.shape[2] != 3 or rgb.shape[1] < 1 or depth_pred.dim() != 2 or depth_pred.shape[0] != P:
        raise SnrError(f"cross_metrics: expected rgb (P,n,3) and depth_pred (P,n_l) for the P = {P} pairs, got {tuple(rgb.shape)}, {tuple(depth_pred.shape)}")
    n, n_l = rgb.shape[1], depth_pred.shape[1]
    V = occ.shape[0] if occ.dim() == 2 else 0
    if V < 1 or tuple(tgt.shape) != (V, n, 3) or tuple(occ.shape) != (V, n) or tuple(lid_depth.shape) != (V, n_l):
        raise SnrError(f"cross_metrics: expected tgt (V,{n},3), occ (V,{n}), lid_depth (V,{n_l}), got {tuple(tgt.shape)}, {tuple(occ.shape)}, "
                       f"{tuple(lid_depth.shape)}")
    if lid_cnt.dtype != torch.int32 or not lid_cnt.is_contiguous() or tuple(lid_cnt.shape) != (V,):
        raise SnrError(f"cross_metrics: lid_cnt must be a contiguous int32 (V,) = ({V},) tensor")
    dev = rgb.device
    if any(t.device != dev for t in (depth_pred, tgt, occ, lid_depth, lid_cnt)):
        raise SnrError("cross_metrics: all tensors on one GPU")
    pairs_h = pairs.cpu().contiguous()
    pairs_d = pairs.contiguous() if pairs.is_cuda else pairs_h.to(dev)
    if pairs_d.device != dev:
        raise SnrError("cross_metrics: all tensors on one GPU")
    if n_codes is None:     # (the code row is the caller's bookkeeping: without a count its range is whatever the table itself spans)
        n_codes = max(int(pairs_h[:, 0].max()) + 1, 1)
    out = torch.empty(P, 3, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_cross_metrics(_p(rgb), _p(depth_pred), _p(tgt), _p(occ), _p(lid_depth), _p(lid_cnt), _p(pairs_d),
                                           C.cast(pairs_h.data_ptr(), C.POINTER(C.c_int32)), P, V, int(n_codes), n, n_l, _p(out), _stream(dev)),
              "snr_cross_metrics")
    return out


class TableAdamW:
    """torch.optim.AdamW's update (amsgrad off, same defaults) for ANY number of tensors as ONE launch per step: the training step's
    optimiser (src/trainer_unified_nuscenes.py:414-422; torch's foreach form is ~18 launches over the 36 tensors, its ``fused=True`` form
    does not reproduce the update on this ROCm build).  ``groups``: [(list of parameters, lr), ...] (up to 4).  Gradients are read from
    the ``.grad`` tensors the parameters hold WHEN THE OPTIMISER IS BUILT (the trainer's bucket views: fixed addresses), which are
    checked again at every step.  After the launch the parameters' version counters are bumped, so caches keyed on them (the packed
    weight stream) see the change."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not 1 <= len(groups) <= 4:
            raise SnrError("TableAdamW: 1 to 4 parameter groups")
        self.lr = [float(lr) for _, lr in groups]
        self.params, self.group_of = [], []
        for gi, (ps, _) in enumerate(groups):
            for p in ps:
                if p.requires_grad:
                    self.params.append(p); self.group_of.append(gi)
        if not self.params:
            raise SnrError("TableAdamW: no trainable parameter")
        dev = self.params[0].device
        for p in self.params:
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise SnrError("TableAdamW: fp32 contiguous parameters on one GPU")
            if p.grad is None or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.shape != p.shape or p.grad.device != dev:
                raise SnrError("TableAdamW: every parameter needs its dense fp32 .grad buffer before the optimiser is built (GradBucket)")
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.steps = 0
        self._key = None
        self._table = None
        self._build_table()

    def _build_table(self):
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for p in self.params)
        if key == self._key:
            return
        rows = [[p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), g]
                for p, m, v, g in zip(self.params, self.exp_avg, self.exp_avg_sq, self.group_of)]
        self._table = torch.tensor(rows, dtype=torch.int64).to(self.params[0].device)
        self._max_numel = max(p.numel() for p in self.params)
        self._key = key

    def zero_grad(self, set_to_none=False):
        if set_to_none:
            raise SnrError("TableAdamW reads the gradients from fixed buffers: clear them in place (GradBucket.zero)")
        for p in self.params:
            p.grad.zero_()

    def step(self):
        for p in self.params:
            if p.grad is None:
                raise SnrError("TableAdamW.step: a parameter lost its .grad buffer (zero_grad(set_to_none=True)?)")
        self._build_table()          # (a moved parameter or a replaced gradient buffer: new table)
        self.steps += 1
        lr = (C.c_float * len(self.lr))(*self.lr)
        dev = self.params[0].device
        with torch.cuda.device(dev):
            check(_lib.lib().snr_adamw_table_step(_p(self._table), len(self.params), int(self._max_numel), lr, len(self.lr), self.steps,
                                                  self.betas[0], self.betas[1], self.eps, self.weight_decay, _stream(dev)), "snr_adamw_table_step")
        torch.autograd.graph.increment_version(self.params)


# ------------------------------------------------------------------------------------ decoder on points
def decoder_fwd(xyz, viewdir, latent, packed, shape_blocks, texture_blocks, save_masks=False, precision="fp32", activations=None):
    """xyz, viewdir (P,3); latent (B,NLAT,256) -> sigmas (P,), rgbs (P,3)[, relu masks]."""
    xyz, viewdir, latent = _f32c(xyz), _f32c(viewdir), _f32c(latent)
    _need_gpu(xyz, viewdir, latent, packed)
    P = xyz.shape[0]
    B = latent.shape[0]
    if P % B:
        raise SnrError("number of points is not divisible by the number of objects")
    dev = xyz.device
    sig = torch.empty(P, device=dev)
    rgb = torch.empty(P, 3, device=dev)
    masks = None
    if save_masks:
        masks = torch.empty(_lib.lib().snr_mask_bytes(P, shape_blocks, texture_blocks), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_decoder_fwd(_p(xyz), _p(viewdir), _p(latent), _p(packed), P, P // B if B else 1, shape_blocks,
                                         texture_blocks, _p(sig), _p(rgb), _p(masks), _p(activations),
                                         resolve_precision(precision, shape_blocks, texture_blocks, P // B if B else 1), _stream(dev)),
              "snr_decoder_fwd")
    return sig, rgb, masks


def decoder_bwd(xyz, viewdir, latent, packed, masks, sigmas, d_sig, d_rgb, shape_blocks, texture_blocks,
                need_latent=True, need_xyz=True, need_dir=True, precision="fp32", layer_grads=None):
    xyz, viewdir, latent, sigmas = _f32c(xyz), _f32c(viewdir), _f32c(latent), _f32c(sigmas)
    _need_gpu(xyz, viewdir, latent, packed, masks, sigmas, d_sig, d_rgb, layer_grads)
    if masks is None or sigmas is None:
        raise SnrError("decoder_bwd needs the ReLU bits and densities saved by decoder_fwd(..., save_masks=True)")
    masks, d_sig, d_rgb = masks.contiguous(), _f32c(d_sig), _f32c(d_rgb)
    P, B = xyz.shape[0], latent.shape[0]
    dev = xyz.device
    if need_latent and shape_blocks + texture_blocks > 0 and _tile_pad(P // B):
        raise SnrError(f"gradient wrt the latent codes needs whole 32-point wave tiles per object, got {P // B} points per object "
                       f"({P} points / {B} codes): pad the ray batch of every object to a multiple of 32 / n_samples rays, or detach the codes")
    d_latent = torch.empty_like(latent) if need_latent else None
    d_xyz = torch.empty_like(xyz) if need_xyz else None
    d_dir = torch.empty_like(viewdir) if need_dir else None
    ws_bytes = _lib.lib().snr_decoder_bwd_ws_bytes(P, P // B, shape_blocks, texture_blocks)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_decoder_bwd(_p(xyz), _p(viewdir), _p(latent), _p(packed), _p(masks), _p(sigmas), _p(d_sig),
                                         _p(d_rgb), P, P // B, shape_blocks, texture_blocks, _p(d_latent), _p(d_xyz),
                                         _p(d_dir), _p(layer_grads), _p(ws), ws_bytes, resolve_precision(precision, shape_blocks, texture_blocks, P // B),
                                         _stream(dev)), "snr_decoder_bwd")
    return d_latent, d_xyz, d_dir


# The latent-gradient partials are reduced per object over whole tiles of points (csrc/snr_host.hpp):
WAVE_TILE = 32          # "partial rows of 32 points": the decoder / render backward, split and exact fp32 with one wave per SIMD
DENSITY_TILE = 64       # "partial rows of 64 points": the density backward (mode 2), always the exact-fp32 backward with two waves per SIMD


def _tile_pad(per_obj: int, unit: int = 1, tile: int = WAVE_TILE) -> int:
    """Items per object after padding so that items x unit is a multiple of ``tile`` points (0 = no padding needed).  THE statement
    of the per-object tile rule: the Functions pad with it, the raw backwards check their operands with it, ``model`` sizes its probe
    launches with it.  Whether a latent gradient is wanted -- the only reason to pad -- is asked in two ways that differ under
    ``torch.no_grad()``: the Functions read ``ctx.needs_input_grad``, which does not see grad mode; ``model`` and ``driver`` read
    ``torch.is_grad_enabled() and lat.requires_grad``."""
    if (per_obj * unit) % tile == 0:
        return 0
    step = tile // math.gcd(tile, unit)
    return -(-per_obj // step) * step


def _pad_rows(t, B, n, n_pad):
    """(B*n, ...) -> (B*n_pad, ...): every object's block padded with zero rows (dummy points / rays: their upstream gradients are zero)."""
    if t is None:
        return None
    v = t.reshape(B, n, *t.shape[1:])
    out = v.new_zeros(B, n_pad, *t.shape[1:])
    out[:, :n] = v
    return out.reshape(B * n_pad, *t.shape[1:])


def _unpad_rows(t, B, n, n_pad):
    if t is None:
        return None
    return t.reshape(B, n_pad, *t.shape[1:])[:, :n].reshape(B * n, *t.shape[1:])


class ObjectPad(NamedTuple):
    """What a Function's ``ctx.pad`` carries from forward to backward: B objects of n rows each, launched as n_pad rows each
    (``_tile_pad``'s count; 0 = launched as they are).  ``pad`` / ``strip`` hand back their argument itself when nothing was padded."""
    B: int
    n: int
    n_pad: int

    def pad(self, t):
        return _pad_rows(t, *self) if self.n_pad and t is not None else t

    def strip(self, t):
        return _unpad_rows(t, *self) if self.n_pad and t is not None else t


class DecoderPoints(torch.autograd.Function):
    """SUPNeRF.forward on explicit points.  Differentiable wrt latent terms, xyz and viewdir (weights are
    treated as constants on this path)."""

    @staticmethod
    def forward(ctx, xyz, viewdir, latent, packed, shape_blocks, texture_blocks, precision="fp32"):
        xyz, viewdir, latent = _f32c(xyz), _f32c(viewdir), _f32c(latent)
        need = any(ctx.needs_input_grad[:3])
        B, P = max(latent.shape[0], 1), xyz.shape[0]
        # the latent-gradient reduction works on whole 32-point wave tiles per object: other point counts (the reference takes any) are padded
        # per object with dummy points whose upstream gradients are zero
        n_pad = _tile_pad(P // B) if (ctx.needs_input_grad[2] and shape_blocks + texture_blocks > 0 and P % B == 0 and P > 0) else 0
        ctx.pad = pad = ObjectPad(B, P // B, n_pad)
        xyz, viewdir = pad.pad(xyz), pad.pad(viewdir)
        prec = resolve_precision(precision, shape_blocks, texture_blocks, xyz.shape[0] // B)
        sig, rgb, masks = decoder_fwd(xyz, viewdir, latent, packed, shape_blocks, texture_blocks, save_masks=need, precision=prec)
        if need:
            ctx.save_for_backward(xyz, viewdir, latent, packed, masks, sig)
            ctx.cfg = (shape_blocks, texture_blocks, resolve_precision(precision, shape_blocks, texture_blocks, xyz.shape[0] // B, backward=True))
        return pad.strip(sig), pad.strip(rgb)

    @staticmethod
    def backward(ctx, d_sig, d_rgb):
        xyz, viewdir, latent, packed, masks, sig = ctx.saved_tensors
        sb, tb, prec = ctx.cfg
        pad = ctx.pad
        d_lat, d_xyz, d_dir = decoder_bwd(xyz, viewdir, latent, packed, masks, sig, pad.pad(_f32c(d_sig)), pad.pad(_f32c(d_rgb)), sb, tb,
                                          ctx.needs_input_grad[2], ctx.needs_input_grad[0], ctx.needs_input_grad[1], precision=prec)
        return pad.strip(d_xyz), pad.strip(d_dir), d_lat, None, None, None, None


# ------------------------------------------------------------------------------------ density-only decoder on points
def _density_shapes(xyz, latent, shape_blocks, texture_blocks):
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise SnrError(f"xyz must be (P, 3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    n_lat = max(shape_blocks + texture_blocks, 1)
    if not torch.is_tensor(latent) or latent.dim() != 3 or latent.shape[0] < 1 or tuple(latent.shape[1:]) != (n_lat, 256):
        raise SnrError(f"latent must be (B, {n_lat}, 256), got {tuple(latent.shape) if torch.is_tensor(latent) else type(latent).__name__}")
    P, B = xyz.shape[0], latent.shape[0]
    if P % B:
        raise SnrError(f"{P} points do not split evenly over {B} objects")
    return P, B


def density_fwd(xyz, latent, packed, shape_blocks, texture_blocks, save_masks=False):
    """Density-only exact-fp32 decoder: xyz (P,3); latent (B,NLAT,256) -> sigmas (P,)[, relu masks].  sigma is bit-identical to
    ``decoder_fwd(..., precision="fp32")``'s; the masks (``save_masks``) hold encoding_xyz's and the shape layers' ReLU bits in
    ``decoder_fwd``'s layout, the texture-branch slots unwritten (``snr_density_fwd_masks``)."""
    P, B = _density_shapes(xyz, latent, shape_blocks, texture_blocks)
    _need_gpu(xyz, latent, packed)
    xyz, latent = _f32c(xyz), _f32c(latent)
    dev = xyz.device
    sig = torch.empty(P, device=dev)
    masks = None
    if save_masks:
        masks = torch.empty(_lib.lib().snr_mask_bytes(P, shape_blocks, texture_blocks), dtype=torch.uint8, device=dev)
    if P == 0:
        return sig, masks
    with torch.cuda.device(dev):
        if save_masks:
            check(_lib.lib().snr_density_fwd_masks(_p(xyz), _p(latent), _p(packed), P, P // B, shape_blocks, texture_blocks, _p(sig), _p(masks),
                                                   _stream(dev)), "snr_density_fwd_masks")
        else:
            check(_lib.lib().snr_density_fwd(_p(xyz), _p(latent), _p(packed), P, P // B, shape_blocks, texture_blocks, _p(sig), _stream(dev)),
                  "snr_density_fwd")
    return sig, masks


def density_bwd(xyz, latent, packed, masks, sigmas, d_sig, shape_blocks, texture_blocks, need_latent=True, need_xyz=True):
    """Backward of ``density_fwd`` (``snr_density_bwd``): (d_latent (B,NLAT,256) or None, d_xyz (P,3) or None) given d_sig (P,).  The
    texture rows of d_latent are zero; the latent gradient needs a multiple of 64 points per object.  Equal, bit for bit, to
    ``decoder_bwd(..., d_rgb=0, precision="fp32")``'s d_xyz and shape rows."""
    P, B = _density_shapes(xyz, latent, shape_blocks, texture_blocks)
    if masks is None or sigmas is None or d_sig is None:
        raise SnrError("density_bwd needs the ReLU bits and densities saved by density_fwd(..., save_masks=True) and d_sig")
    if tuple(sigmas.shape) != (P,) or tuple(d_sig.shape) != (P,):
        raise SnrError(f"sigmas and d_sig must be ({P},), got {tuple(sigmas.shape)} and {tuple(d_sig.shape)}")
    _need_gpu(xyz, latent, packed, masks, sigmas, d_sig)
    xyz, latent, sigmas, d_sig, masks = _f32c(xyz), _f32c(latent), _f32c(sigmas), _f32c(d_sig), masks.contiguous()
    if masks.dtype != torch.uint8 or masks.numel() < _lib.lib().snr_mask_bytes(P, shape_blocks, texture_blocks):
        raise SnrError("density_bwd: masks must be the uint8 buffer density_fwd(..., save_masks=True) returned for these points")
    lat_rows = shape_blocks + texture_blocks > 0
    if need_latent and lat_rows and _tile_pad(P // B, 1, DENSITY_TILE):
        raise SnrError(f"the latent gradient of the density path needs a multiple of 64 points per object, got {P // B} "
                       "(DensityPoints pads them)")
    dev = xyz.device
    d_latent = (torch.empty_like(latent) if lat_rows else torch.zeros_like(latent)) if need_latent else None
    d_xyz = torch.empty_like(xyz) if need_xyz else None
    if P == 0:
        return (torch.zeros_like(latent) if need_latent else None), d_xyz
    ws_bytes = _lib.lib().snr_decoder_bwd_ws_bytes(P, P // B, shape_blocks, texture_blocks) if need_latent and lat_rows else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        check(_lib.lib().snr_density_bwd(_p(xyz), _p(latent), _p(packed), _p(masks), _p(sigmas), _p(d_sig), P, P // B, shape_blocks,
                                         texture_blocks, _p(d_latent), _p(d_xyz), _p(ws), ws_bytes, _stream(dev)), "snr_density_bwd")
    return d_latent, d_xyz


class DensityPoints(torch.autograd.Function):
    """sigma of the decoder on explicit points, density head only.  Differentiable wrt xyz and the latent terms (the decoder weights are
    constants on this path).  With a latent gradient to form, every object's points are padded to a multiple of 64 with dummy points
    whose upstream gradient is zero."""

    @staticmethod
    def forward(ctx, xyz, latent, packed, shape_blocks, texture_blocks):
        P, B = _density_shapes(xyz, latent, shape_blocks, texture_blocks)
        xyz, latent = _f32c(xyz), _f32c(latent)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        n_pad = _tile_pad(P // B, 1, DENSITY_TILE) if (ctx.needs_input_grad[1] and shape_blocks + texture_blocks > 0) else 0
        ctx.pad = pad = ObjectPad(B, P // B, n_pad)
        xyz = pad.pad(xyz)
        sig, masks = density_fwd(xyz, latent, packed, shape_blocks, texture_blocks, save_masks=need)
        if need:
            ctx.save_for_backward(xyz, latent, packed, masks, sig)
            ctx.cfg = (shape_blocks, texture_blocks)
        return pad.strip(sig)

    @staticmethod
    def backward(ctx, d_sig):
        xyz, latent, packed, masks, sig = ctx.saved_tensors
        sb, tb = ctx.cfg
        pad = ctx.pad
        d_lat, d_xyz = density_bwd(xyz, latent, packed, masks, sig, pad.pad(_f32c(d_sig)), sb, tb, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return pad.strip(d_xyz), d_lat, None, None, None


# ------------------------------------------------------------------------------------ density on lattices, and the narrow band's passes
def density_grid(lat, latent, packed, shape_blocks, texture_blocks):
    """sigma (B, n0, n1, n2) of the B objects of ``latent`` on the ``Lattice`` ``lat``, its points made in the kernel (``snr_density_grid``)."""
    B, dev = latent.shape[0], latent.device
    out = torch.empty(B, *lat.n, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_density_grid(lat, B, _p(latent), _p(packed), shape_blocks, texture_blocks, _p(out), _stream(dev)), "snr_density_grid")
    return out


def density_bricks(lat, bricks, n, latent, packed, shape_blocks, texture_blocks, out):
    """sigma at the points of the first ``n`` bricks (object, I, J, K) of the int32 list ``bricks`` on ``lat``, written into the grids
    ``out`` (B, n0, n1, n2) (``snr_density_bricks``); entries out of range are skipped, the other points of ``out`` are left alone."""
    dev = out.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_density_bricks(lat, out.shape[0], _ptr(bricks, torch.int32), n, _p(latent), _p(packed), shape_blocks,
                                            texture_blocks, _p(out), _stream(dev)), "snr_density_bricks")
    return out


def band_classify(coarse, lat, level, band, state, fill):
    """Per brick of ``lat`` from the coarse grids: state 1 / 0 (active or not) and the fill value (``snr_band_classify``)."""
    dev = coarse.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_band_classify(_p(coarse), coarse.shape[0], lat, level, band, _ptr(state, torch.int32), _ptr(fill), _stream(dev)),
              "snr_band_classify")


def band_compact(state, scan, lat, bricks):
    """The bricks of state 1 as a list (object, I, J, K) in ``bricks``, at the slots their inclusive ``scan`` gives (``snr_band_compact``)."""
    dev = state.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_band_compact(_ptr(state, torch.int32), _ptr(scan, torch.int32), state.shape[0], lat, _ptr(bricks, torch.int32),
                                          _stream(dev)), "snr_band_compact")


def band_fill(grid, lat, state, fill):
    """The points of the bricks of state 0 set to their brick's fill value (``snr_band_fill``)."""
    dev = grid.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_band_fill(_p(grid), grid.shape[0], lat, _ptr(state, torch.int32), _ptr(fill), _stream(dev)), "snr_band_fill")


def band_seam(grid, lat, level, stamp, state, bricks, n_new):
    """One growth round (``snr_band_seam``): the unevaluated bricks at the ends of crossing edges get state ``stamp`` and are listed in
    ``bricks``; their number goes to ``n_new`` (1,) int32 on the device."""
    dev = grid.device
    with torch.cuda.device(dev):
        check(_lib.lib().snr_band_seam(_p(grid), grid.shape[0], lat, level, stamp, _ptr(state, torch.int32), _ptr(bricks, torch.int32),
                                       _ptr(n_new, torch.int32), _stream(dev)), "snr_band_seam")


# ------------------------------------------------------------------------------------ iso-surface and its backward
class IsoMesh(NamedTuple):
    verts: torch.Tensor        # (sum V, 3) fp32, object after object
    faces: torch.Tensor        # (sum F, 3) int32, indices local to each object
    n_verts: list              # V per object
    n_faces: list              # F per object
    edge_mask: torch.Tensor    # (B, nv) uint8: the crossing edges of each grid point (the forward's topology)
    edge_scan: torch.Tensor    # (B, nv) int32: inclusive scan of their counts per object
    vert_offset: torch.Tensor  # (B,) int64: where each object's vertices start


def iso_extract(grid, lat, level):
    """Marching tetrahedra of the fp32 grids (B, n0, n1, n2) on ``lat`` (a ``Lattice``): ``snr_iso_count``, two ``torch.cumsum`` per object,
    ``snr_iso_emit``; one host read (the output sizes).  A non-finite grid value raises.  Returns an ``IsoMesh``."""
    B = grid.shape[0]
    nv = lat.n[0] * lat.n[1] * lat.n[2]
    nc = (lat.n[0] - 1) * (lat.n[1] - 1) * (lat.n[2] - 1)
    dev = grid.device
    lib, st = _lib.lib(), _stream(dev)
    tri_count = torch.empty(B, nc, dtype=torch.uint8, device=dev)
    edge_mask = torch.empty(B, nv, dtype=torch.uint8, device=dev)
    edge_count = torch.empty(B, nv, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.snr_iso_count(_p(grid), B, lat, level, _ptr(tri_count, torch.uint8), _ptr(edge_mask, torch.uint8),
                                _ptr(edge_count, torch.uint8), st), "snr_iso_count")
        # per object: <= 7 * 512^3 vertices and <= 12 * 511^3 triangles, both below 2^31
        edge_scan = torch.cumsum(edge_count, dim=1, dtype=torch.int32)
        tri_scan = torch.cumsum(tri_count, dim=1, dtype=torch.int32)
        n_vert, n_tri = edge_scan[:, -1].long(), tri_scan[:, -1].long()
        vert_off, tri_off = torch.cumsum(n_vert, 0) - n_vert, torch.cumsum(n_tri, 0) - n_tri
        bad = (~torch.isfinite(grid)).any().long().view(1)
        host = torch.cat([bad, n_vert, n_tri]).cpu().tolist()
        if host[0]:
            raise SnrError("extract_mesh: the grid holds a non-finite value")
        nvs, nts = host[1:1 + B], host[1 + B:]
        verts = torch.empty(sum(nvs), 3, device=dev)
        faces = torch.empty(sum(nts), 3, dtype=torch.int32, device=dev)
        check(lib.snr_iso_emit(_p(grid), B, lat, level, _ptr(edge_mask, torch.uint8), _ptr(edge_scan, torch.int32),
                               _ptr(tri_scan, torch.int32), _ptr(vert_off, torch.int64), _ptr(tri_off, torch.int64),
                               _ptr(verts), _ptr(faces, torch.int32), st), "snr_iso_emit")
    return IsoMesh(verts, faces, nvs, nts, edge_mask, edge_scan, vert_off)


def iso_grad(grid, lat, level, edge_mask, edge_scan, vert_offset, d_verts, want_surface=False):
    """Backward of ``iso_extract``'s vertices (``snr_iso_grad``): d_grid (B, n0, n1, n2) fp32 from d_verts (sum V, 3), gathered per grid
    point in a fixed order (deterministic); with ``want_surface`` also on_surface (B, nv) uint8, 1 at the ends of crossing edges."""
    B = grid.shape[0]
    dev = grid.device
    d_verts = _f32c(d_verts)
    d_grid = torch.empty(grid.shape, device=dev)
    on = torch.empty(edge_mask.shape, dtype=torch.uint8, device=dev) if want_surface else None
    if B:
        with torch.cuda.device(dev):
            check(_lib.lib().snr_iso_grad(_p(grid), B, lat, level, _ptr(edge_mask, torch.uint8), _ptr(edge_scan, torch.int32),
                                          _ptr(vert_offset, torch.int64), _p(d_verts) if d_verts.numel() else C.c_void_p(0), _p(d_grid),
                                          _p(on), _stream(dev)), "snr_iso_grad")
    return d_grid, on


def iso_surface_points(on_surface, d_grid, lat):
    """The grid points flagged by ``iso_grad`` as a point list for the density backward (``snr_iso_surface_points``): (xyz (B n, 3) lattice
    coordinates, d_sig (B n), n, counts (B,) int64 on the device) with n the largest count rounded up to a multiple of 64 (the padding
    points: xyz = lo, d_sig = 0).  One host read (n)."""
    B = on_surface.shape[0]
    dev = on_surface.device
    scan = torch.cumsum(on_surface, dim=1, dtype=torch.int32)
    counts = scan[:, -1].long() if B else torch.zeros(0, dtype=torch.int64, device=dev)
    n = int(counts.max()) if B else 0
    n = _tile_pad(n, 1, DENSITY_TILE) or n
    xyz = torch.empty(B * n, 3, device=dev)
    d_sig = torch.empty(B * n, device=dev)
    if B:
        with torch.cuda.device(dev):
            check(_lib.lib().snr_iso_surface_points(_ptr(on_surface, torch.uint8), _ptr(scan, torch.int32), _p(d_grid), B, lat, n, _p(xyz),
                                                    _p(d_sig), _stream(dev)), "snr_iso_surface_points")
    return xyz, d_sig, n, counts


def _iso_forward(ctx, grid, lat, level, *saved):
    """The forward of both iso Functions: ``iso_extract``, its topology saved after ``saved`` for the backward."""
    m = iso_extract(grid, lat, level)
    ctx.save_for_backward(*saved, grid, m.edge_mask, m.edge_scan, m.vert_offset)
    sizes = torch.tensor([m.n_verts, m.n_faces], dtype=torch.int64)
    ctx.mark_non_differentiable(m.faces, sizes)
    return m.verts, m.faces, sizes


class IsoVertices(torch.autograd.Function):
    """Iso-surface vertices of grids (B, n0, n1, n2), differentiable wrt the grid values at the forward's topology.  Forward: ``iso_extract``
    (output unchanged).  Saves the grid, edge_mask and edge_scan (4 + 1 + 4 = 9 bytes per grid point) rather than rerun the count pass.
    Backward: ``snr_iso_grad``.  Returns (verts, faces, sizes): sizes (2, B) int64 on the host, V and F per object."""

    @staticmethod
    def forward(ctx, grid, lat, level):
        ctx.cfg = (lat, level)
        return _iso_forward(ctx, grid, lat, level)

    @staticmethod
    def backward(ctx, d_verts, d_faces, d_sizes):
        grid, edge_mask, edge_scan, vert_off = ctx.saved_tensors
        lat, level = ctx.cfg
        d_grid, _ = iso_grad(grid, lat, level, edge_mask, edge_scan, vert_off, d_verts)
        return d_grid, None, None


class IsoVerticesLatent(torch.autograd.Function):
    """Iso-surface vertices of the density grids of B objects, differentiable wrt their latent terms (B, NLAT, 256).  ``grid`` must hold
    the density forward's value at both ends of every crossing edge (a dense grid, or a narrow-band grid at its fixpoint); its other
    values only decide the topology.  Forward: ``iso_extract`` of the grid.  Backward: ``snr_iso_grad`` -> ``snr_iso_surface_points`` ->
    ``density_fwd(save_masks=True)`` and ``density_bwd(need_latent=True)`` on the surface points of all B objects in one launch each: the
    decoder runs at those points only.  Returns (verts, faces, sizes) like ``IsoVertices``."""

    @staticmethod
    def forward(ctx, latent, packed, grid, lat, level, shape_blocks, texture_blocks):
        ctx.cfg = (lat, level, shape_blocks, texture_blocks)
        return _iso_forward(ctx, grid, lat, level, latent, packed)

    @staticmethod
    def backward(ctx, d_verts, d_faces, d_sizes):
        latent, packed, grid, edge_mask, edge_scan, vert_off = ctx.saved_tensors
        lat, level, sb, tb = ctx.cfg
        d_grid, on = iso_grad(grid, lat, level, edge_mask, edge_scan, vert_off, d_verts, want_surface=True)
        xyz, d_sig, n, _ = iso_surface_points(on, d_grid, lat)
        if n == 0:
            return torch.zeros_like(latent), None, None, None, None, None, None
        latent = _f32c(latent)
        sig, masks = density_fwd(xyz, latent, packed, sb, tb, save_masks=True)
        d_lat, _ = density_bwd(xyz, latent, packed, masks, sig, d_sig, sb, tb, need_latent=True, need_xyz=False)
        return d_lat, None, None, None, None, None, None


# ------------------------------------------------------------------------------------ mesh components
MESH_SLAB = 4096         # list entries per slab of the fixed-order float64 sums (include/supnerf_hip.h, "Fixed-order segmented sums")


class MeshComponents(NamedTuple):
    vert_label: torch.Tensor   # (sum V,) int32: component of each vertex, local to its object
    face_label: torch.Tensor   # (sum F,) int32: component of each face (its first vertex's)
    n_comps: list              # C per object
    comp_offset: list          # (B + 1): where each object's components start in the arrays below
    n_verts: torch.Tensor      # (sum C,) int64
    n_faces: torch.Tensor      # (sum C,) int64
    area: torch.Tensor         # (sum C,) float64
    volume: torch.Tensor       # (sum C,) float64, signed, about the component's vertex of smallest index
    bbox_lo: torch.Tensor      # (sum C, 3) fp32
    bbox_hi: torch.Tensor      # (sum C, 3) fp32


def _host_offsets(sizes):
    """[0, s0, s0 + s1, ...]: where each object's items start in a packed array, and the total."""
    off = [0]
    for s in sizes:
        off.append(off[-1] + int(s))
    return off


def _offsets(sizes, dev):
    off = _host_offsets(sizes)
    return off, torch.tensor(off, dtype=torch.int64).to(dev)


def _last_slots(off_h, dev):
    """(the objects that are not empty, the last packed slot of each as an int64 index tensor on ``dev``): what a host read gathers."""
    full = [b for b in range(len(off_h) - 1) if off_h[b + 1] > off_h[b]]
    return full, torch.tensor([off_h[b + 1] - 1 for b in full], dtype=torch.int64).to(dev)


def _segments(sorted_ids, n_segments, dev):
    """(seg_start, slab_offset), both (n_segments + 1) int64, of a list sorted by segment id (include/supnerf_hip.h, "Fixed-order
    segmented sums")."""
    seg_start = torch.searchsorted(sorted_ids, torch.arange(n_segments + 1, dtype=sorted_ids.dtype, device=dev))
    slab_off = torch.zeros(n_segments + 1, dtype=torch.int64, device=dev)
    torch.cumsum((seg_start[1:] - seg_start[:-1] + (MESH_SLAB - 1)) // MESH_SLAB, 0, out=slab_off[1:])
    return seg_start, slab_off


class PackedMesh(NamedTuple):
    """Several objects' meshes in the form the ``snr_mesh_*`` and ``snr_raster_*`` entry points take."""
    verts: torch.Tensor        # (sum V, 3) fp32, object after object
    faces: torch.Tensor        # (sum F, 3) int32, indices local to each object
    vert_offset: torch.Tensor  # (B + 1,) int64 on the device: where each object's vertices start
    face_offset: torch.Tensor  # (B + 1,) int64 on the device
    n_verts: list              # V per object
    n_faces: list              # F per object


def pack_mesh(verts, faces, n_verts, n_faces) -> PackedMesh:
    """Check ``verts`` (sum V, 3) fp32 and ``faces`` (sum F, 3) int32 against the per-object counts ``n_verts`` / ``n_faces`` (host lists)
    and put the offsets on the device."""
    _need_gpu(verts, faces)
    n_verts, n_faces = [int(x) for x in n_verts], [int(x) for x in n_faces]
    B = len(n_verts)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise SnrError(f"a packed mesh is verts (sum V, 3) fp32 and faces (sum F, 3) int32, got {tuple(verts.shape)} {verts.dtype} and "
                       f"{tuple(faces.shape)} {faces.dtype}")
    if len(n_faces) != B or min(n_verts + n_faces + [0]) < 0 or sum(n_verts) != verts.shape[0] or sum(n_faces) != faces.shape[0]:
        raise SnrError(f"n_verts {n_verts} and n_faces {n_faces} do not add up to {verts.shape[0]} vertices and {faces.shape[0]} faces")
    if max(n_verts + [0]) > 2 ** 31 - 1:
        raise SnrError("an object has more than 2^31 - 1 vertices")
    verts, faces = _f32c(verts.detach()), faces.contiguous()
    return PackedMesh(verts, faces, _offsets(n_verts, verts.device)[1], _offsets(n_faces, verts.device)[1], n_verts, n_faces)


def mesh_components(verts, faces, n_verts, n_faces):
    """The connected components of a packed mesh (include/supnerf_hip.h, "Mesh components"): ``verts`` (sum V, 3) fp32 and ``faces``
    (sum F, 3) int32 with indices local to each object, ``n_verts`` / ``n_faces`` the V and F per object (host lists), as ``iso_extract``
    returns them.  ``snr_mesh_hook`` (lock-free union-find over the faces) -> ``snr_mesh_flatten`` -> one ``torch.cumsum`` per object ->
    ``snr_mesh_label``; counts and boxes by ``snr_mesh_boxes``; area and volume by a stable sort of the faces by component,
    ``snr_mesh_face_terms`` and ``snr_mesh_segment_sum`` (fixed order: the same bits from run to run).  One host read: the component
    counts together with the bad-index flag; a face index outside its object raises.  Returns a ``MeshComponents``."""
    mesh = pack_mesh(verts, faces, n_verts, n_faces)
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), verts.device
    nV, nF = verts.shape[0], faces.shape[0]
    lib, st = _lib.lib(), _stream(dev)
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    voff_h = _host_offsets(n_verts)
    with torch.cuda.device(dev):
        parent = torch.empty(nV, dtype=i32, device=dev)
        root = torch.empty(nV, dtype=i32, device=dev)
        is_root = torch.empty(nV, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(lib.snr_mesh_hook(_ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), B, nV, nF, _ptr(parent, i32), _ptr(bad, i32), st),
              "snr_mesh_hook")
        check(lib.snr_mesh_flatten(_ptr(parent, i32), _ptr(voff, i64), B, nV, _ptr(root, i32), _ptr(is_root, torch.uint8), st),
              "snr_mesh_flatten")
        root_scan = torch.empty(nV, dtype=i32, device=dev)
        for b in range(B):
            if n_verts[b]:
                torch.cumsum(is_root[voff_h[b]:voff_h[b + 1]], 0, dtype=i32, out=root_scan[voff_h[b]:voff_h[b + 1]])
        full, last = _last_slots(voff_h, dev)
        host = torch.cat([bad.long(), root_scan[last].long()]).cpu().tolist()          # the one host read
        if host[0]:
            raise SnrError("mesh_components: a face index lies outside its object's vertices")
        n_comps = [0] * B
        for b, c in zip(full, host[1:]):
            n_comps[b] = c
        coff_h, coff = _offsets(n_comps, dev)
        nC = coff_h[-1]
        if nC > 2 ** 31 - 1:
            raise SnrError("more than 2^31 - 1 components in one call")
        vert_label = torch.empty(nV, dtype=i32, device=dev)
        face_label = torch.empty(nF, dtype=i32, device=dev)
        check(lib.snr_mesh_label(_ptr(root, i32), _ptr(root_scan, i32), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), B, nV, nF,
                                 _ptr(vert_label, i32), _ptr(face_label, i32), st), "snr_mesh_label")
        comp_verts = torch.empty(nC, dtype=i64, device=dev)
        bbox_lo, bbox_hi = torch.empty(nC, 3, device=dev), torch.empty(nC, 3, device=dev)
        check(lib.snr_mesh_boxes(_ptr(verts), _ptr(vert_label, i32), _ptr(voff, i64), _ptr(coff, i64), B, nV, nC, _ptr(comp_verts, i64),
                                 _ptr(bbox_lo), _ptr(bbox_hi), st), "snr_mesh_boxes")
        area, volume = torch.zeros(nC, dtype=f64, device=dev), torch.zeros(nC, dtype=f64, device=dev)
        comp_faces = torch.zeros(nC, dtype=i64, device=dev)
        if nF and nC:
            key = face_label
            if B > 1:       # component ids of the whole call: the object's first id added to every face of the object
                key = face_label + torch.repeat_interleave(coff[:-1].to(i32), torch.tensor(n_faces, dtype=i64).to(dev), output_size=nF)
            key, order = torch.sort(key, stable=True)
            seg_start, slab_off = _segments(key, nC, dev)
            comp_faces = seg_start[1:] - seg_start[:-1]
            area_t, vol_t = torch.empty(nF, dtype=f64, device=dev), torch.empty(nF, dtype=f64, device=dev)
            check(lib.snr_mesh_face_terms(_ptr(verts), _ptr(faces, i32), _ptr(root, i32), _ptr(order, i64), _ptr(voff, i64), _ptr(foff, i64),
                                          B, nV, nF, _ptr(area_t, f64), _ptr(vol_t, f64), st), "snr_mesh_face_terms")
            n_slabs = int(lib.snr_segment_slab_bound(nC, nF))
            partial = torch.empty(n_slabs, 2, dtype=f64, device=dev)
            check(lib.snr_mesh_segment_sum(_ptr(area_t, f64), _ptr(vol_t, f64), _ptr(seg_start, i64), _ptr(slab_off, i64), nC, nF,
                                           _ptr(partial, f64), n_slabs, _ptr(area, f64), _ptr(volume, f64), st), "snr_mesh_segment_sum")
    return MeshComponents(vert_label, face_label, n_comps, coff_h, comp_verts, comp_faces, area, volume, bbox_lo, bbox_hi)


# ------------------------------------------------------------------------------------ mesh simplification
SIMPLIFY_PLACEMENTS = ("mean", "quadric")


class SimplifiedMesh(NamedTuple):
    verts: torch.Tensor        # (sum V', 3) fp32: one vertex per cluster, object after object
    faces: torch.Tensor        # (sum F', 3) int32, indices local to each object
    n_verts: list              # V' per object
    n_faces: list              # F' per object
    vert_map: torch.Tensor     # (sum V,) int32: the new local index of every old vertex
    members: torch.Tensor      # (sum V',) int32: how many old vertices each new one stands for
    face_index: torch.Tensor   # (sum F',) int64: the kept faces, as indices into the old packed face array
    attributes: Optional[torch.Tensor]     # (sum V', C) fp32 or None


def _per_object_f32(x, B, width, dev, what):
    t = torch.as_tensor(x, dtype=torch.float32) if not torch.is_tensor(x) else x.detach().float()
    shape = (B,) if width == 1 else (B, width)
    if t.dim() == 0 or (width > 1 and t.dim() == 1 and t.shape[0] == width):
        t = t.expand(shape)
    if tuple(t.shape) != shape:
        raise SnrError(f"mesh_simplify: {what} is one value or one per object {shape}, got {tuple(t.shape)}")
    return t.to(dev).contiguous()


def mesh_simplify(verts, faces, n_verts, n_faces, cell, origin, placement="quadric", attributes=None) -> SimplifiedMesh:
    """Quadric vertex clustering of a packed mesh (include/supnerf_hip.h, "Mesh simplification"): ``verts`` (sum V, 3) fp32 and ``faces``
    (sum F, 3) int32 with indices local to each object, ``n_verts`` / ``n_faces`` the V and F per object (host lists); ``cell`` (B,) > 0
    and ``origin`` (B, 3) the grid of cubic cells each object lays over its vertices (one value serves every object).  All vertices of an
    object that fall into one cell become one new vertex -- whether or not faces connect them: two sheets that pass through one cell merge
    there -- placed at their mean (``placement="mean"``) or where the planes of the original faces around them meet, inside the cell
    (``"quadric"``, which keeps edges and corners).  A face survives iff its corners land in three different cells; survivors keep their
    order and winding, and faces that come out equal are all kept.  ``attributes`` (sum V, C) fp32, C <= 16, are averaged per cluster.

    ``snr_simplify_keys`` -> a stable ``torch.sort`` (a second one by object when B > 1), head flags and ``torch.cumsum`` ->
    ``snr_simplify_faces`` -> ``torch.cumsum`` of the keep flags -> the one host read (both flags, the cluster counts and the kept-face
    counts) -> ``snr_simplify_compact``; a stable sort of the face corners by cluster (quadric only) -> ``snr_simplify_positions`` and
    ``snr_simplify_attributes`` (float64 sums in a fixed order: the same bits from run to run).  A non-finite coordinate, a cell index of
    2^20 or beyond and a face index outside its object raise.  Nothing here is differentiable."""
    if placement not in SIMPLIFY_PLACEMENTS:
        raise SnrError(f"mesh_simplify: placement is 'mean' or 'quadric', got {placement!r}")
    if not torch.is_tensor(cell) or not cell.is_cuda:               # (a cell on the device is checked there: it rides the one host read)
        cell_h = torch.as_tensor(cell, dtype=torch.float32).reshape(-1)
        if not bool(((cell_h > 0) & torch.isfinite(cell_h)).all()):
            raise SnrError(f"mesh_simplify: cell must be positive and finite, got {cell_h.tolist()}")
    if faces.dtype != torch.int32:
        raise SnrError(f"mesh_simplify: faces are int32, got {faces.dtype}")
    mesh = pack_mesh(verts, faces, n_verts, n_faces)
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), verts.device
    nV, nF = verts.shape[0], faces.shape[0]
    cell = _per_object_f32(cell, B, 1, dev, "cell")
    origin = _per_object_f32(origin, B, 3, dev, "origin")
    if attributes is not None:
        _need_gpu(attributes)
        if attributes.dim() != 2 or attributes.shape[0] != nV or not 1 <= attributes.shape[1] <= RASTER_MAX_CHANNELS:
            raise SnrError(f"mesh_simplify: attributes are ({nV}, C) with 1 <= C <= {RASTER_MAX_CHANNELS}, got {tuple(attributes.shape)}")
        attributes = _f32c(attributes.detach())
    lib, st = _lib.lib(), _stream(dev)
    i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    with torch.cuda.device(dev):
        bad = torch.zeros(3, dtype=i32, device=dev)                 # a vertex without a cell, a face index out of range, a bad cell edge
        bad[2:] = (~((cell > 0) & torch.isfinite(cell))).any().to(i32)
        key = torch.empty(nV, dtype=i64, device=dev)
        check(lib.snr_simplify_keys(_ptr(verts), _ptr(voff, i64), _ptr(cell), _ptr(origin), B, nV, _ptr(key, i64), _ptr(bad[0:1], i32), st),
              "snr_simplify_keys")
        # rule 2: the vertices by (object, key, index); a cluster starts where the key or the object changes
        key, vert_order = torch.sort(key, stable=True)
        counts_v = torch.tensor(n_verts, dtype=i64).to(dev)
        obj = torch.repeat_interleave(torch.arange(B, dtype=i32, device=dev), counts_v, output_size=nV)
        if B > 1:
            obj_sorted, by_obj = torch.sort(obj[vert_order], stable=True)
            key, vert_order = key[by_obj], vert_order[by_obj]
        else:
            obj_sorted = obj
        head = torch.ones(nV, dtype=torch.bool, device=dev)
        if nV > 1:
            head[1:] = (key[1:] != key[:-1]) | (obj_sorted[1:] != obj_sorted[:-1])
        cluster_sorted = torch.cumsum(head, 0, dtype=i64) - 1       # the cluster of the whole call, per sorted vertex
        cluster_of = torch.empty(nV, dtype=i64, device=dev)
        cluster_of[vert_order] = cluster_sorted
        voff_h, foff_h = _host_offsets(n_verts), _host_offsets(n_faces)
        (full, last_v), (with_faces, last_f) = _last_slots(voff_h, dev), _last_slots(foff_h, dev)
        first_cluster = torch.zeros(B, dtype=i64, device=dev)       # (object b's vertices hold the sorted slots voff[b] .. voff[b + 1])
        if full:
            first_cluster[torch.tensor(full, dtype=i64).to(dev)] = cluster_sorted[torch.tensor([voff_h[b] for b in full], dtype=i64).to(dev)]
        vert_map = (cluster_of - first_cluster[obj.long()]).to(i32)
        # rule 6
        new_faces = torch.empty(nF, 3, dtype=i32, device=dev)
        keep = torch.empty(nF, dtype=u8, device=dev)
        check(lib.snr_simplify_faces(_ptr(faces, i32), _ptr(vert_map, i32), _ptr(voff, i64), _ptr(foff, i64), B, nV, nF,
                                     _ptr(new_faces, i32), _ptr(keep, u8), _ptr(bad[1:2], i32), st), "snr_simplify_faces")
        keep_scan = torch.cumsum(keep, 0, dtype=i64)
        host = torch.cat([bad.long(), cluster_sorted[last_v] + 1, keep_scan[last_f]]).cpu().tolist()      # the one host read
        if host[2]:
            raise SnrError("mesh_simplify: cell must be positive and finite")
        if host[0]:
            raise SnrError("mesh_simplify: a vertex is not finite or lies 2^20 cells or more from the origin")
        if host[1]:
            raise SnrError("mesh_simplify: a face index lies outside its object's vertices")
        ends_v, ends_f = host[3:3 + len(full)], host[3 + len(full):]
        new_n_verts, new_n_faces, prev = [0] * B, [0] * B, 0
        for b, e in zip(full, ends_v):
            new_n_verts[b], prev = e - prev, e
        prev = 0
        for b, e in zip(with_faces, ends_f):
            new_n_faces[b], prev = e - prev, e
        nC, nK = sum(new_n_verts), sum(new_n_faces)
        out_faces = torch.empty(nK, 3, dtype=i32, device=dev)
        face_index = torch.empty(nK, dtype=i64, device=dev)
        check(lib.snr_simplify_compact(_ptr(new_faces, i32), _ptr(keep, u8), _ptr(keep_scan, i64), nF, nK, _ptr(out_faces, i32),
                                       _ptr(face_index, i64), st), "snr_simplify_compact")
        # rules 3 to 5 and 7: the sorted member and corner lists, cut into slabs
        vseg, vslab = _segments(cluster_sorted, nC, dev)
        members = (vseg[1:] - vseg[:-1]).to(i32)
        out_verts = torch.empty(nC, 3, device=dev)
        quadric = placement == "quadric" and nF > 0
        corder = cseg = cslab = cpartial = None
        n_cslabs = 0
        if quadric and nC:
            counts_f = torch.tensor(n_faces, dtype=i64).to(dev)
            face_v0 = torch.repeat_interleave(voff[:-1], counts_f, output_size=nF)
            corner_cluster, corder = torch.sort(cluster_of[(faces.long() + face_v0[:, None]).view(-1)], stable=True)
            cseg, cslab = _segments(corner_cluster, nC, dev)
            n_cslabs = int(lib.snr_segment_slab_bound(nC, nF * 3))
            cpartial = torch.empty(n_cslabs, 9, dtype=f64, device=dev)
        n_vslabs = int(lib.snr_segment_slab_bound(nC, nV))
        vpartial = torch.empty(n_vslabs, 3, dtype=f64, device=dev)
        check(lib.snr_simplify_positions(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(cell), _ptr(origin), B, nV, nF,
                                         _ptr(vert_order, i64), _ptr(vseg, i64), _ptr(vslab, i64), _ptr(corder, i64), _ptr(cseg, i64),
                                         _ptr(cslab, i64), nC, int(quadric), _ptr(vpartial, f64), n_vslabs, _ptr(cpartial, f64), n_cslabs,
                                         _ptr(out_verts), st), "snr_simplify_positions")
        out_attr = None
        if attributes is not None:
            nCh = attributes.shape[1]
            out_attr = torch.empty(nC, nCh, device=dev)
            apartial = torch.empty(n_vslabs, nCh, dtype=f64, device=dev)
            check(lib.snr_simplify_attributes(_ptr(attributes), nCh, nV, _ptr(vert_order, i64), _ptr(vseg, i64), _ptr(vslab, i64), nC,
                                              _ptr(apartial, f64), n_vslabs, _ptr(out_attr), st), "snr_simplify_attributes")
    return SimplifiedMesh(out_verts, out_faces, new_n_verts, new_n_faces, vert_map, members, face_index, out_attr)


# ------------------------------------------------------------------------------------ mesh distance
NEAREST_MAX_CELLS = 256         # cells per axis of an object's grid (include/supnerf_hip.h, "Mesh distance", D3)
NEAREST_MAX_PAIRS = 1 << 26     # (cell, face) pairs of one index: 12 bytes each, sorted once
NEAREST_CELL_FACTOR = 2.0       # the default cell edge is this times the square root of the object's mean face area


class NearestIndex(NamedTuple):
    """The grid of D3 over a packed mesh: what ``mesh_nearest_query`` walks."""
    cell: torch.Tensor         # (B,) fp32: the cell edge per object
    grid_lo: torch.Tensor      # (B, 3) fp32: the exact minimum of each object's vertices (0 without vertices)
    grid_hi: torch.Tensor      # (B, 3) fp32: their exact maximum
    cell_offset: torch.Tensor  # (B + 1,) int64 on the device: where each object's cells start
    cell_start: torch.Tensor   # (n_cells + 1,) int64: cell c's faces at pair_face[cell_start[c] : cell_start[c + 1]]
    pair_face: torch.Tensor    # (n_pairs,) int32: object-local face indices, ascending within a cell
    n_cells: int
    n_pairs: int


def mesh_face_areas(mesh: PackedMesh) -> torch.Tensor:
    """(sum F,) float64: the area term of every face (include/supnerf_hip.h, "Mesh components", rule 3), by ``snr_mesh_face_terms``; 0 for
    a face with an index outside its object."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    dev, nV, nF = verts.device, verts.shape[0], faces.shape[0]
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    area, vol = torch.zeros(nF, dtype=f64, device=dev), torch.empty(nF, dtype=f64, device=dev)
    if nF:
        with torch.cuda.device(dev):
            root = torch.zeros(nV, dtype=i32, device=dev)           # (the volume term's reference vertex; that term is not used)
            check(_lib.lib().snr_mesh_face_terms(_ptr(verts), _ptr(faces, i32), _ptr(root, i32), None, _ptr(voff, i64), _ptr(foff, i64),
                                                 len(n_verts), nV, nF, _ptr(area, f64), _ptr(vol, f64), _stream(dev)), "snr_mesh_face_terms")
    return area


def mesh_cumulative_area(mesh: PackedMesh, areas=None) -> torch.Tensor:
    """(sum F,) float64: per object the INCLUSIVE scan of its face areas (one ``torch.cumsum`` per object): D5's ``cum``."""
    areas = mesh_face_areas(mesh) if areas is None else areas
    cum = torch.empty_like(areas)
    off = _host_offsets(mesh.n_faces)
    for b in range(len(mesh.n_faces)):
        if mesh.n_faces[b]:
            torch.cumsum(areas[off[b]:off[b + 1]], 0, out=cum[off[b]:off[b + 1]])
    return cum


def _nearest_grid(mesh, cell):
    """(grid_lo, grid_hi (B, 3) fp32, cells per object (B,) int64) of D3 on the device: the same float64 operations as the kernels'."""
    verts, B, dev = mesh.verts, len(mesh.n_verts), mesh.verts.device
    lo, hi = torch.zeros(B, 3, device=dev), torch.zeros(B, 3, device=dev)
    off = _host_offsets(mesh.n_verts)
    for b in range(B):
        if mesh.n_verts[b]:
            lo[b], hi[b] = verts[off[b]:off[b + 1]].amin(0), verts[off[b]:off[b + 1]].amax(0)
    n = torch.ceil((hi.double() - lo.double()) / cell.double()[:, None])
    n = torch.where(n >= 1.0, n.clamp(max=float(NEAREST_MAX_CELLS)), torch.ones_like(n)).long()           # (a NaN gives 1)
    return lo, hi, n.prod(1)


def mesh_default_cell(mesh: PackedMesh, factor=NEAREST_CELL_FACTOR) -> torch.Tensor:
    """(B,) fp32 on the device: the default cell edge of ``geometry.mesh_index`` -- ``factor`` times the square root of the object's mean
    face area, but no less than 1/256 of its largest extent, below which the 256 cells per axis would no longer cover the object and its
    border cells, which reach outwards without end, would hold most of the faces.  An object without area gets one cell."""
    B, dev = len(mesh.n_verts), mesh.verts.device
    areas = mesh_face_areas(mesh)
    off = _host_offsets(mesh.n_faces)
    mean = torch.stack([areas[off[b]:off[b + 1]].mean() if mesh.n_faces[b] else areas.new_zeros(()) for b in range(B)])
    lo, hi, _ = _nearest_grid(mesh, torch.ones(B, device=dev))
    base, extent = (float(factor) * torch.sqrt(mean)).float(), (hi - lo).amax(1)
    whole = torch.where((extent > 0) & torch.isfinite(extent), extent, torch.ones_like(extent))            # one cell
    return torch.where((base > 0) & torch.isfinite(base), torch.maximum(base, whole / NEAREST_MAX_CELLS), whole)


def mesh_nearest_index(mesh: PackedMesh, cell) -> NearestIndex:
    """The grid of D3 (include/supnerf_hip.h, "Mesh distance") over a packed mesh: ``cell`` (B,) fp32 > 0 on the device, the cell edge per
    object.  ``snr_nearest_count`` -> one ``torch.cumsum`` -> the one host read (the flag, the pair count and the cell count) ->
    ``snr_nearest_emit`` -> one stable ``torch.sort`` by cell -> ``torch.searchsorted``.  A face index outside its object, a non-finite
    vertex and a cell that is not positive and finite raise; so do more than ``NEAREST_MAX_PAIRS`` pairs, with the factor by which to
    grow the cells."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), verts.device
    nV, nF = verts.shape[0], faces.shape[0]
    lib, st = _lib.lib(), _stream(dev)
    i32, i64 = torch.int32, torch.int64
    cell = _per_object_f32(cell, B, 1, dev, "cell")
    with torch.cuda.device(dev):
        lo, hi, cells = _nearest_grid(mesh, cell)
        coff = torch.zeros(B + 1, dtype=i64, device=dev)
        torch.cumsum(cells, 0, out=coff[1:])
        bad = torch.zeros(2, dtype=i32, device=dev)
        bad[1:] = (~((cell > 0) & torch.isfinite(cell))).any().to(i32)
        count = torch.zeros(nF, dtype=i32, device=dev)
        n_cells_bound = min(B * NEAREST_MAX_CELLS ** 3, 1 << 38)    # (the count is on the device still; each object's is checked there)
        check(lib.snr_nearest_count(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(cell), _ptr(lo), _ptr(hi),
                                    _ptr(coff, i64), B, nV, nF, n_cells_bound, _ptr(count, i32), _ptr(bad[0:1], i32), st), "snr_nearest_count")
        scan = torch.cumsum(count, 0, dtype=i64)
        total = scan[-1:] if nF else torch.zeros(1, dtype=i64, device=dev)
        host = torch.cat([bad.long(), total, coff[-1:]]).cpu().tolist()                                      # the one host read
        if host[1]:
            raise SnrError("mesh_index: cell must be positive and finite")
        if host[0]:
            raise SnrError("mesh_index: a face index lies outside its object's vertices, or a vertex is not finite")
        n_pairs, n_cells = host[2], host[3]
        if n_pairs > NEAREST_MAX_PAIRS:
            raise SnrError(f"mesh_index: {n_pairs} (cell, face) pairs exceed the limit of {NEAREST_MAX_PAIRS}; cells "
                           f"{_nearest_fit(mesh, cell):.3g} times as large would fit")
        pair_cell = torch.empty(n_pairs, dtype=i64, device=dev)
        pair_face = torch.empty(n_pairs, dtype=i32, device=dev)
        first = scan - count                                        # the exclusive scan
        check(lib.snr_nearest_emit(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(cell), _ptr(lo), _ptr(hi),
                                   _ptr(coff, i64), _ptr(first, i64), B, nV, nF, n_cells, n_pairs, _ptr(pair_cell, i64),
                                   _ptr(pair_face, i32), st), "snr_nearest_emit")
        pair_cell, order = torch.sort(pair_cell, stable=True)
        cell_start = torch.searchsorted(pair_cell, torch.arange(n_cells + 1, dtype=i64, device=dev))
    return NearestIndex(cell, lo, hi, coff, cell_start, pair_face[order].contiguous(), n_cells, n_pairs)


def _nearest_fit(mesh, cell):
    """The factor (a power of 1.25) by which to grow ``cell`` so that the pairs fit ``NEAREST_MAX_PAIRS``: counted, not estimated.  Only
    the error path comes here; each trial is one launch and one host read."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev, i32, i64 = len(n_verts), verts.device, torch.int32, torch.int64
    factor = 1.0
    for _ in range(64):
        factor *= 1.25
        c = (cell * factor).contiguous()
        lo, hi, cells = _nearest_grid(mesh, c)
        coff = torch.zeros(B + 1, dtype=i64, device=dev)
        torch.cumsum(cells, 0, out=coff[1:])
        count = torch.zeros(faces.shape[0], dtype=i32, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(_lib.lib().snr_nearest_count(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(c), _ptr(lo), _ptr(hi),
                                           _ptr(coff, i64), B, verts.shape[0], faces.shape[0], min(B * NEAREST_MAX_CELLS ** 3, 1 << 38), _ptr(count, i32),
                                           _ptr(bad, i32), _stream(dev)), "snr_nearest_count")
        if int(count.sum(dtype=i64)) <= NEAREST_MAX_PAIRS:
            break
    return factor


def _packed_counts(counts, B, total, what):
    counts = [int(c) for c in counts]
    if len(counts) != B or min(counts + [0]) < 0 or sum(counts) != total:
        raise SnrError(f"{what}: per-object counts {counts} do not add up to {total} rows for {B} objects")
    return counts


def mesh_nearest_query(mesh: PackedMesh, index: NearestIndex, points, n_queries):
    """(face (sum Q,) int32, weights (sum Q, 3) fp32, dist2 (sum Q,) float64): per query the closest face of ITS object (object-local
    index, -1 for none), the barycentric weights of the closest point and the squared distance, by ``snr_nearest_query`` (D1 - D4: the
    brute-force answer bit for bit, whatever the grid).  ``points`` (sum Q, 3) fp32 object after object, ``n_queries`` the Q per object
    (a host list).  Nothing is read back: a bad face index that only this launch could notice gives a skipped face."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), verts.device
    _need_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise SnrError(f"mesh_nearest_query: points are (sum Q, 3), got {tuple(points.shape)}")
    points = _f32c(points.detach())
    nQ = points.shape[0]
    n_queries = _packed_counts(n_queries, B, nQ, "mesh_nearest_query")
    if tuple(index.cell.shape) != (B,) or index.cell_offset.shape[0] != B + 1 or index.cell_start.shape[0] != index.n_cells + 1:
        raise SnrError("mesh_nearest_query: this index was not built for this mesh")
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    with torch.cuda.device(dev):
        qoff = _offsets(n_queries, dev)[1]
        face = torch.empty(nQ, dtype=i32, device=dev)
        weights = torch.empty(nQ, 3, device=dev)
        dist2 = torch.empty(nQ, dtype=f64, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(_lib.lib().snr_nearest_query(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(points), _ptr(qoff, i64),
                                           _ptr(index.cell), _ptr(index.grid_lo), _ptr(index.grid_hi), _ptr(index.cell_offset, i64),
                                           _ptr(index.cell_start, i64), _ptr(index.pair_face, i32), B, verts.shape[0], faces.shape[0], nQ,
                                           index.n_cells, index.n_pairs, _ptr(face, i32), _ptr(weights), _ptr(dist2, f64), _ptr(bad, i32),
                                           _stream(dev)), "snr_nearest_query")
    return face, weights, dist2


def mesh_surface_sample(mesh: PackedMesh, cum, uniforms, n_samples):
    """(points (sum S, 3) fp32, face (sum S,) int32, weights (sum S, 3) fp32): stratified area-uniform samples by ``snr_surface_sample``
    (D5) from ``cum`` (sum F,) float64 (``mesh_cumulative_area``) and ``uniforms`` (sum S, 3) float64 in [0, 1); ``n_samples`` the S per
    object (a host list).  An object without area gets face -1.  Nothing is read back."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), verts.device
    _need_gpu(cum, uniforms)
    if uniforms.dim() != 2 or uniforms.shape[1] != 3 or uniforms.dtype != torch.float64 or cum.dtype != torch.float64 or \
            tuple(cum.shape) != (faces.shape[0],):
        raise SnrError(f"mesh_surface_sample: uniforms are (sum S, 3) float64 and cum is (sum F,) float64, got {tuple(uniforms.shape)} "
                       f"{uniforms.dtype} and {tuple(cum.shape)} {cum.dtype}")
    nS = uniforms.shape[0]
    n_samples = _packed_counts(n_samples, B, nS, "mesh_surface_sample")
    uniforms, cum = uniforms.contiguous(), cum.contiguous()
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    with torch.cuda.device(dev):
        soff = _offsets(n_samples, dev)[1]
        points, weights = torch.empty(nS, 3, device=dev), torch.empty(nS, 3, device=dev)
        face = torch.empty(nS, dtype=i32, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(_lib.lib().snr_surface_sample(_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), _ptr(cum, f64), _ptr(uniforms, f64),
                                            _ptr(soff, i64), B, verts.shape[0], faces.shape[0], nS, _ptr(points), _ptr(face, i32), _ptr(weights),
                                            _ptr(bad, i32), _stream(dev)), "snr_surface_sample")
    return points, face, weights


def object_sums(d, d2, n_per_object):
    """(sum d, sum d2) (B,) float64 per object of two (sum Q,) float64 lists packed object after object, by ``snr_mesh_segment_sum`` with
    the objects as segments: the fixed order of include/supnerf_hip.h ("Fixed-order segmented sums"), the same bits from run to run."""
    _need_gpu(d, d2)
    dev, B, n = d.device, len(n_per_object), d.shape[0]
    i64, f64 = torch.int64, torch.float64
    out_a, out_b = torch.zeros(B, dtype=f64, device=dev), torch.zeros(B, dtype=f64, device=dev)
    if B == 0 or n == 0:
        return out_a, out_b
    lib = _lib.lib()
    with torch.cuda.device(dev):
        seg_start = _offsets(n_per_object, dev)[1]
        slab_off = torch.zeros(B + 1, dtype=i64, device=dev)
        torch.cumsum((seg_start[1:] - seg_start[:-1] + (MESH_SLAB - 1)) // MESH_SLAB, 0, out=slab_off[1:])
        n_slabs = int(lib.snr_segment_slab_bound(B, n))
        partial = torch.empty(n_slabs, 2, dtype=f64, device=dev)
        check(lib.snr_mesh_segment_sum(_ptr(d.contiguous(), f64), _ptr(d2.contiguous(), f64), _ptr(seg_start, i64), _ptr(slab_off, i64), B, n,
                                       _ptr(partial, f64), n_slabs, _ptr(out_a, f64), _ptr(out_b, f64), _stream(dev)), "snr_mesh_segment_sum")
    return out_a, out_b


# ------------------------------------------------------------------------------------ mesh containment
def _inside_args(mesh, index, what):
    """The pointers and sizes ``snr_inside_query`` and ``snr_inside_lattice`` take for the mesh and its grid (``index``: a
    ``NearestIndex`` built over this mesh)."""
    verts, faces, voff, foff, n_verts, n_faces = mesh
    B = len(n_verts)
    if not isinstance(index, NearestIndex) or tuple(index.cell.shape) != (B,) or index.cell_offset.shape[0] != B + 1 or \
            index.cell_start.shape[0] != index.n_cells + 1:
        raise SnrError(f"{what}: this index was not built for this mesh")
    i32, i64 = torch.int32, torch.int64
    grid = (_ptr(index.cell), _ptr(index.grid_lo), _ptr(index.grid_hi), _ptr(index.cell_offset, i64), _ptr(index.cell_start, i64),
            _ptr(index.pair_face, i32))
    return (_ptr(verts), _ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64)), grid, (B, verts.shape[0], faces.shape[0])


def mesh_inside_query(mesh: PackedMesh, index: NearestIndex, points, n_queries):
    """winding (sum Q,) int32: per query the integer winding number along +z of ITS object's mesh, by ``snr_inside_query``
    (include/supnerf_hip.h, "Mesh containment", W1 - W5: the brute-force integers, whatever the grid).  ``points`` (sum Q, 3) fp32 object
    after object, ``n_queries`` the Q per object (a host list), ``index`` what ``mesh_nearest_index`` built over ``mesh``.  Nothing is read
    back: a bad face index that only this launch could notice gives a skipped face."""
    dev = mesh.verts.device
    _need_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise SnrError(f"mesh_inside_query: points are (sum Q, 3), got {tuple(points.shape)}")
    m, g, (B, nV, nF) = _inside_args(mesh, index, "mesh_inside_query")
    points = _f32c(points.detach())
    nQ = points.shape[0]
    n_queries = _packed_counts(n_queries, B, nQ, "mesh_inside_query")
    i32, i64 = torch.int32, torch.int64
    with torch.cuda.device(dev):
        qoff = _offsets(n_queries, dev)[1]
        winding = torch.empty(nQ, dtype=i32, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(_lib.lib().snr_inside_query(*m, _ptr(points), _ptr(qoff, i64), *g, B, nV, nF, nQ, index.n_cells, index.n_pairs,
                                          _ptr(winding, i32), _ptr(bad, i32), _stream(dev)), "snr_inside_query")
    return winding


def mesh_inside_lattice(mesh: PackedMesh, index: NearestIndex, lat_lo, lat_h, n):
    """winding (B, nx, ny, nz) int32: the winding numbers of ``mesh_inside_query`` at the points lat_lo + lat_h (i, j, k) of one lattice
    per object (an fp32 multiply, then an fp32 add: the points of ``geometry.lattice_points``), by ``snr_inside_lattice`` (W6: the same
    integers, the work that does not depend on z done once per face and run of 16 z-points).  ``lat_lo`` and ``lat_h`` are (B, 3) fp32
    (or 3 numbers for every object), ``n`` = (nx, ny, nz) shared by the objects.  Nothing is read back."""
    dev = mesh.verts.device
    m, g, (B, nV, nF) = _inside_args(mesh, index, "mesh_inside_lattice")
    n = tuple(int(x) for x in n)
    if len(n) != 3 or min(n) < 1:
        raise SnrError(f"mesh_inside_lattice: n is three positive point counts, got {n}")
    lat_lo, lat_h = _per_object_f32(lat_lo, B, 3, dev, "lat_lo"), _per_object_f32(lat_h, B, 3, dev, "lat_h")
    i32 = torch.int32
    with torch.cuda.device(dev):
        winding = torch.empty((B,) + n, dtype=i32, device=dev)
        bad = torch.zeros(1, dtype=i32, device=dev)
        check(_lib.lib().snr_inside_lattice(*m, *g, _ptr(lat_lo), _ptr(lat_h), B, nV, nF, index.n_cells, index.n_pairs, n[0], n[1], n[2],
                                            _ptr(winding, i32), _ptr(bad, i32), _stream(dev)), "snr_inside_lattice")
    return winding


# ------------------------------------------------------------------------------------ mesh ray casting
def _raycast_rays(mesh, index, rays_o, rays_d, t_min, t_max, n_rays, what):
    """The leading arguments of the C calls of ``mesh_raycast_first`` / ``mesh_raycast_crossings`` from the checked ray arrays, the ray
    count, and the dense arrays those pointers name (the caller holds them until its launch is enqueued)."""
    _need_gpu(rays_o, rays_d, t_min, t_max)
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape:
        raise SnrError(f"{what}: rays_o and rays_d are (sum N, 3), got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
    nR = rays_o.shape[0]
    if tuple(t_min.shape) != (nR,) or tuple(t_max.shape) != (nR,):
        raise SnrError(f"{what}: t_min and t_max are (sum N,), got {tuple(t_min.shape)} and {tuple(t_max.shape)} for {nR} rays")
    m, g, (B, nV, nF) = _inside_args(mesh, index, what)
    n_rays = _packed_counts(n_rays, B, nR, what)
    rays = [_f32c(x.detach()) for x in (rays_o, rays_d, t_min, t_max)]
    roff = _offsets(n_rays, rays_o.device)[1]
    args = (*m, _ptr(rays[0]), _ptr(rays[1]), _ptr(roff, torch.int64), _ptr(rays[2]), _ptr(rays[3]), *g, B, nV, nF, nR, index.n_cells,
            index.n_pairs)
    return args, nR, (rays, roff)


def mesh_raycast_first(mesh: PackedMesh, index: NearestIndex, rays_o, rays_d, t_min, t_max, n_rays, cull=0):
    """(face (sum N,) int32, t (sum N,) float64, weights (sum N, 3) fp32, side (sum N,) int8): per ray o + t d the first face of ITS
    object's mesh that it hits with t_min < t < t_max (object-local index, -1 for none; t = +inf for none), the barycentric weights of
    the hit and the side it was hit from (+1 front, -1 back, 0 none), by ``snr_raycast_first`` (include/supnerf_hip.h, "Mesh ray casting",
    R1 - R6: the brute-force answer bit for bit, whatever the grid).  ``rays_o`` and ``rays_d`` (sum N, 3) fp32 object after object,
    ``t_min`` and ``t_max`` (sum N,) fp32, ``n_rays`` the N per object (a host list), ``index`` what ``mesh_nearest_index`` built over
    ``mesh``; ``cull``: 0 none, 1 drops back-facing faces, 2 front-facing ones.  Nothing is read back."""
    if cull not in (0, 1, 2):
        raise SnrError(f"mesh_raycast_first: cull is 0 (none), 1 (back) or 2 (front), got {cull!r}")
    dev = mesh.verts.device
    with torch.cuda.device(dev):
        args, nR, keep = _raycast_rays(mesh, index, rays_o, rays_d, t_min, t_max, n_rays, "mesh_raycast_first")
        face = torch.empty(nR, dtype=torch.int32, device=dev)
        t = torch.empty(nR, dtype=torch.float64, device=dev)
        weights = torch.empty(nR, 3, device=dev)
        side = torch.empty(nR, dtype=torch.int8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        check(_lib.lib().snr_raycast_first(*args, int(cull), _ptr(face, torch.int32), _ptr(t, torch.float64), _ptr(weights),
                                           _ptr(side, torch.int8), _ptr(bad, torch.int32), _stream(dev)), "snr_raycast_first")
    return face, t, weights, side


def mesh_raycast_crossings(mesh: PackedMesh, index: NearestIndex, rays_o, rays_d, t_min, t_max, n_rays):
    """(signed (sum N,) int32, total (sum N,) int32): per ray the faces of ITS object's mesh that it crosses with t_min < t < t_max --
    +1 where it leaves through the face, -1 where it enters, and their number -- by ``snr_raycast_crossings`` (R1 - R6: the brute-force
    integers, whatever the grid).  The arguments are those of ``mesh_raycast_first``.  Nothing is read back."""
    dev = mesh.verts.device
    with torch.cuda.device(dev):
        args, nR, keep = _raycast_rays(mesh, index, rays_o, rays_d, t_min, t_max, n_rays, "mesh_raycast_crossings")
        signed = torch.empty(nR, dtype=torch.int32, device=dev)
        total = torch.empty(nR, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        check(_lib.lib().snr_raycast_crossings(*args, _ptr(signed, torch.int32), _ptr(total, torch.int32), _ptr(bad, torch.int32),
                                               _stream(dev)), "snr_raycast_crossings")
    return signed, total


# ------------------------------------------------------------------------------------ mesh smoothing
SMOOTH_KEY_BITS = 31            # snr_smooth_edge_keys: (global source index) << 31 | local target index
SMOOTH_NO_KEY = 2 ** 63 - 1     # a discarded pair


class MeshAdjacency(NamedTuple):
    nbr_start: torch.Tensor    # (sum V + 1,) int64: vertex i's neighbours at nbr[nbr_start[i] : nbr_start[i + 1]]
    nbr: torch.Tensor          # (E2,) int32: indices local to the object, ascending within each vertex
    edge_faces: torch.Tensor   # (E2,) int32: how many faces name the undirected edge; the same in both directions
    degree: torch.Tensor       # (sum V,) int32
    boundary: torch.Tensor     # (sum V,) bool: one of the vertex's edges has exactly one face
    nonmanifold: torch.Tensor  # (sum V,) bool: one of the vertex's edges has more than two faces
    boundary_edges: list       # per object: undirected edges with one face
    nonmanifold_edges: list    # per object: undirected edges with more than two faces
    n_verts: list              # V per object
    vert_offset: torch.Tensor  # (B + 1,) int64 on the device
    edge_offset: list          # (B + 1) host: where each object's entries of nbr start, and E2


def mesh_adjacency(verts, faces, n_verts, n_faces) -> MeshAdjacency:
    """Which vertices of a packed mesh are neighbours (include/supnerf_hip.h, "Mesh smoothing", rules 1 to 3): ``verts`` (sum V, 3) fp32
    and ``faces`` (sum F, 3) int32 with indices local to each object, ``n_verts`` / ``n_faces`` the V and F per object (host lists).
    ``snr_smooth_edge_keys`` (six keys per face) -> one ``torch.sort`` -> head flags, ``torch.cumsum`` and integer scatters (a neighbour is
    a run of equal keys, ``edge_faces`` its length) -> ``torch.searchsorted`` of the runs' sources (``nbr_start``) -> the one host read
    (the bad-index flag and per object where its entries end, E2 last, with the running counts of boundary and non-manifold entries
    there) -> slices -> ``snr_smooth_vertex_flags``.  A face index outside its object raises.  Only integers: the result is exact and the
    same from run to run."""
    if faces.dtype != torch.int32:
        raise SnrError(f"mesh_adjacency: faces are int32, got {faces.dtype}")
    mesh = pack_mesh(verts, faces, n_verts, n_faces)
    _, faces, voff, foff, n_verts, n_faces = mesh
    B, dev = len(n_verts), faces.device
    nV, nF = sum(n_verts), sum(n_faces)
    if nV >= 2 ** 32:
        raise SnrError("mesh_adjacency: 2^32 vertices or more in one call")
    lib, st = _lib.lib(), _stream(dev)
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    nK = 6 * nF
    with torch.cuda.device(dev):
        bad = torch.zeros(1, dtype=i32, device=dev)
        key = torch.empty(nK, dtype=i64, device=dev)
        check(lib.snr_smooth_edge_keys(_ptr(faces, i32), _ptr(voff, i64), _ptr(foff, i64), B, nV, nF, _ptr(key, i64), _ptr(bad, i32), st),
              "snr_smooth_edge_keys")
        key, _ = torch.sort(key)
        valid = key != SMOOTH_NO_KEY
        head = valid.clone()
        if nK > 1:
            head[1:] &= key[1:] != key[:-1]
        # every valid key goes to the slot of its run (the members of a run hold one key: they store the same values), a discarded pair to
        # slot nK; the CSR is the first E2 entries of arrays sized by their bound 6 F, so nothing here waits for E2
        slot = torch.where(valid, torch.cumsum(head, 0, dtype=i64) - 1, nK)
        src = torch.full((nK + 1,), nV, dtype=i64, device=dev).scatter_(0, slot, key >> SMOOTH_KEY_BITS)[:nK]       # (nV: no run)
        nbr = torch.zeros(nK + 1, dtype=i32, device=dev).scatter_(0, slot, (key & (2 ** SMOOTH_KEY_BITS - 1)).to(i32))[:nK]
        edge_faces = torch.zeros(nK + 1, dtype=i32, device=dev).scatter_add_(0, slot, torch.ones(nK, dtype=i32, device=dev))[:nK]
        nbr_start = torch.searchsorted(src, torch.arange(nV + 1, dtype=i64, device=dev))      # (the runs ascend by source)
        degree = (nbr_start[1:] - nbr_start[:-1]).to(i32)
        # rule 3 per object: both directions of an edge carry its count, so half the entries of a class are its edges
        ends = nbr_start[voff]
        one, many = torch.zeros(nK + 1, dtype=i64, device=dev), torch.zeros(nK + 1, dtype=i64, device=dev)
        torch.cumsum(edge_faces == 1, 0, dtype=i64, out=one[1:])    # (two scans of one row each: a scan along the rows of a (2, 6 F)
        torch.cumsum(edge_faces > 2, 0, dtype=i64, out=many[1:])    # tensor took 13.6 ms at F = 1.0 M, these 0.1 ms)
        host = torch.cat([bad.long(), ends, one[ends], many[ends]]).cpu().tolist()                               # the one host read
        if host[0]:
            raise SnrError("mesh_adjacency: a face index lies outside its object's vertices")
        edge_offset, c1, c2 = host[1:2 + B], host[2 + B:3 + 2 * B], host[3 + 2 * B:]
        boundary_edges = [(c1[b + 1] - c1[b]) // 2 for b in range(B)]
        nonmanifold_edges = [(c2[b + 1] - c2[b]) // 2 for b in range(B)]
        nE = edge_offset[-1]
        nbr, edge_faces = nbr[:nE].contiguous(), edge_faces[:nE].contiguous()
        flags = torch.empty(2, nV, dtype=u8, device=dev)
        check(lib.snr_smooth_vertex_flags(_ptr(nbr_start, i64), _ptr(edge_faces, i32), nV, nE, _ptr(flags[0], u8), _ptr(flags[1], u8), st),
              "snr_smooth_vertex_flags")
    return MeshAdjacency(nbr_start, nbr, edge_faces, degree, flags[0].bool(), flags[1].bool(), boundary_edges, nonmanifold_edges, n_verts, voff,
                         edge_offset)


def _smooth_values(x, adjacency, what):
    _need_gpu(x)
    nV = sum(adjacency.n_verts)
    if x.dim() != 2 or x.shape[0] != nV or not 1 <= x.shape[1] <= RASTER_MAX_CHANNELS:
        raise SnrError(f"{what}: values are ({nV}, C) with 1 <= C <= {RASTER_MAX_CHANNELS}, got {tuple(x.shape)}")
    return _f32c(x.detach())


def _smooth_csr(a):
    """What every gather over a ``MeshAdjacency`` takes beside its values: the CSR, the offsets and the sizes."""
    i32, i64 = torch.int32, torch.int64
    return (_ptr(a.nbr_start, i64), _ptr(a.nbr, i32), _ptr(a.vert_offset, i64), len(a.n_verts), sum(a.n_verts), a.nbr.shape[0])


def mesh_smooth(x, adjacency, iterations=10, lam=0.5, mu=-0.53, pinned=None):
    """``iterations`` Taubin lambda|mu iterations (include/supnerf_hip.h, "Mesh smoothing", rules 4 to 6) of the values ``x`` (sum V, C)
    fp32, C <= 16 -- positions or any per-vertex data -- over a ``MeshAdjacency``: a step with ``lam``, then, unless ``mu`` is None, a step
    with ``mu`` on its result.  ``pinned`` (sum V,) bool: vertices that keep their bits (they still serve as neighbours).  One
    ``snr_smooth_step`` launch per half-step between two buffers, no host read; ``iterations=0`` returns a copy.  Not differentiable."""
    factors = [float(lam)] + ([] if mu is None else [float(mu)])
    if not all(math.isfinite(f) for f in factors):
        raise SnrError(f"mesh_smooth: lam and mu must be finite, got {lam} and {mu}")
    iterations = int(iterations)
    if iterations < 0:
        raise SnrError(f"mesh_smooth: iterations must not be negative, got {iterations}")
    x = _smooth_values(x, adjacency, "mesh_smooth")
    nV, C_ = x.shape
    dev = x.device
    if pinned is not None:
        _need_gpu(pinned)
        if pinned.dtype != torch.bool or tuple(pinned.shape) != (nV,):
            raise SnrError(f"mesh_smooth: pinned is a bool mask ({nV},), got {pinned.dtype} {tuple(pinned.shape)}")
        pinned = pinned.to(torch.uint8).contiguous()
    cur = x.clone()
    if iterations == 0 or nV == 0:
        return cur
    lib, st, csr = _lib.lib(), _stream(dev), _smooth_csr(adjacency)
    with torch.cuda.device(dev):
        other = torch.empty_like(cur)
        for _ in range(iterations):
            for f in factors:
                check(lib.snr_smooth_step(_ptr(cur), C_, *csr, _ptr(pinned, torch.uint8), f, _ptr(other), st), "snr_smooth_step")
                cur, other = other, cur
    return cur


def mesh_laplacian_values(x, adjacency, transpose=False):
    """The umbrella operator U (rule 7 of "Mesh smoothing") of the values ``x`` (sum V, C), or its transpose applied to them
    (``snr_smooth_laplacian``).  No autograd: ``MeshLaplacian`` is the differentiable form."""
    x = _smooth_values(x, adjacency, "mesh_laplacian")
    out = torch.empty_like(x)
    if x.shape[0]:
        with torch.cuda.device(x.device):
            check(_lib.lib().snr_smooth_laplacian(_ptr(x), x.shape[1], *_smooth_csr(adjacency), int(bool(transpose)), _ptr(out),
                                                  _stream(x.device)), "snr_smooth_laplacian")
    return out


class MeshLaplacian(torch.autograd.Function):
    """U = (mean of the neighbours) - x per vertex and channel, of ``x`` (sum V, C) over a ``MeshAdjacency`` (which is a constant); the
    backward applies the transpose to the incoming gradient.  Both are gathers over the same CSR."""

    @staticmethod
    def forward(ctx, x, adjacency):
        ctx.adjacency = adjacency
        return mesh_laplacian_values(x, adjacency)

    @staticmethod
    def backward(ctx, grad):
        return mesh_laplacian_values(grad, ctx.adjacency, transpose=True), None


# ------------------------------------------------------------------------------------ mesh rasteriser
RASTER_MAX_CHANNELS = 16


def _mesh_args(mesh):
    """What every rasteriser entry point takes of its mesh beside the arrays: both offsets, B, sum V and sum F."""
    i64 = torch.int64
    return (_ptr(mesh.vert_offset, i64), _ptr(mesh.face_offset, i64), len(mesh.n_verts), mesh.verts.shape[0], mesh.faces.shape[0])


def raster_project(mesh, obj_to_cam, camera):
    """screen (sum V, 3) = (u, v, camera z) of every vertex of the ``PackedMesh`` (``snr_raster_project``; header rule 1): ``obj_to_cam``
    (B, 3, 4) fp32 on the device maps each object's stored vertices to the camera frame, ``camera`` = (fx, fy, cx, cy) host floats."""
    dev, B = mesh.verts.device, len(mesh.n_verts)
    if tuple(obj_to_cam.shape) != (B, 3, 4):
        raise SnrError(f"obj_to_cam must be ({B}, 3, 4), one matrix per object, got {tuple(obj_to_cam.shape)}")
    fx, fy, cx, cy = [float(v) for v in camera]
    screen = torch.empty(mesh.verts.shape[0], 3, device=dev)
    voff, _, _, nV, _ = _mesh_args(mesh)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_raster_project(_ptr(mesh.verts), voff, B, nV, _ptr(_f32c(obj_to_cam)), fx, fy, cx, cy, _ptr(screen),
                                            _stream(dev)), "snr_raster_project")
    return screen


def raster_faces(mesh, screen, image_of_object, n_images, H, W, z_near, cull_sign=None):
    """keys (n_images, H, W) int64: per pixel the unsigned minimum of (bits(depth) << 32) | packed face over the faces that cover it, all
    ones where none does (``snr_raster_faces``; header rules 2 - 6).  The buffer is allocated and preset here.  ``image_of_object`` (B,)
    int32 on the device: the image each object is drawn into; ``cull_sign`` (B,) int32 or None: a face with A cull_sign > 0 is dropped."""
    dev, i32 = mesh.verts.device, torch.int32
    n_images, H, W = int(n_images), int(H), int(W)
    if min(n_images, H, W) < 0:
        raise SnrError(f"n_images, H and W must not be negative, got {n_images}, {H}, {W}")
    if n_images * H * W >= 2 ** 31:
        raise SnrError(f"{n_images} images of {H} x {W} pixels: the rasteriser takes fewer than 2^31 pixels per call")
    keys = torch.full((n_images, H, W), -1, dtype=torch.int64, device=dev)
    voff, foff, B, nV, nF = _mesh_args(mesh)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_raster_faces(_ptr(screen), _ptr(mesh.faces, i32), voff, foff, _ptr(image_of_object, i32), _ptr(cull_sign, i32), B,
                                          nV, nF, n_images, H, W, float(z_near), _ptr(keys, torch.int64), _stream(dev)), "snr_raster_faces")
    return keys


def raster_resolve(mesh, screen, keys):
    """(face (n_images, H, W) int32, -1 where empty; depth (n_images, H, W), 0 where empty; weights (n_images, H, W, 3)) of the keys of
    ``raster_faces`` (``snr_raster_resolve``; header rule 7)."""
    dev, i32 = mesh.verts.device, torch.int32
    n_images, H, W = keys.shape
    face = torch.empty(n_images, H, W, dtype=i32, device=dev)
    depth = torch.empty(n_images, H, W, device=dev)
    weights = torch.empty(n_images, H, W, 3, device=dev)
    voff, foff, B, nV, nF = _mesh_args(mesh)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_raster_resolve(_ptr(keys, torch.int64), _ptr(screen), _ptr(mesh.faces, i32), voff, foff, B, nV, nF, n_images, H, W,
                                            _ptr(face, i32), _ptr(depth), _ptr(weights), _stream(dev)), "snr_raster_resolve")
    return face, depth, weights


def raster_interpolate(mesh, face, weights, attributes, background=0.0):
    """out (..., C): per pixel of ``face`` (...) / ``weights`` (..., 3) the winning face's per-vertex ``attributes`` (sum V, C) fp32 weighed
    by the barycentric weights, ``background`` where empty (``snr_raster_interpolate``; header rule 8)."""
    dev, i32 = mesh.verts.device, torch.int32
    nV = mesh.verts.shape[0]
    if attributes.dim() != 2 or attributes.shape[0] != nV or not 1 <= attributes.shape[1] <= RASTER_MAX_CHANNELS:
        raise SnrError(f"attributes must be ({nV}, C) with 1 <= C <= {RASTER_MAX_CHANNELS}, got {tuple(attributes.shape)}")
    if tuple(weights.shape) != tuple(face.shape) + (3,) or face.dtype != i32:
        raise SnrError(f"face (...) int32 and weights (..., 3) do not match: {tuple(face.shape)} {face.dtype}, {tuple(weights.shape)}")
    _need_gpu(attributes)
    C_ = attributes.shape[1]
    out = torch.empty(tuple(face.shape) + (C_,), device=dev)
    voff, foff, B, _, nF = _mesh_args(mesh)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_raster_interpolate(_ptr(face.contiguous(), i32), _ptr(_f32c(weights)), _ptr(mesh.faces, i32), voff, foff, B, nV,
                                                nF, _ptr(_f32c(attributes.detach())), C_, face.numel(), float(background), _ptr(out),
                                                _stream(dev)), "snr_raster_interpolate")
    return out


def rasterize(mesh, obj_to_cam, camera, image_of_object, n_images, H, W, z_near, cull_sign=None):
    """``raster_project`` -> ``raster_faces`` -> ``raster_resolve`` on the current stream: (face, depth, weights, screen).  Nothing is read
    back to the host."""
    screen = raster_project(mesh, obj_to_cam, camera)
    keys = raster_faces(mesh, screen, image_of_object, n_images, H, W, z_near, cull_sign)
    return raster_resolve(mesh, screen, keys) + (screen,)


# ------------------------------------------------------------------------------------ mesh painting
PAINT_BLENDS = ("weighted", "best")
PAINT_GRID_THREADS = 2048 * 256      # the threads of one pass of the paint kernels' grid-stride loops (snr_paint.hip: PAINT_MAX_BLOCKS)


class PaintState(NamedTuple):
    """What ``snr_paint_view`` keeps per vertex between the views (include/supnerf_hip.h, "Mesh painting", rule P4)."""
    sum_rgb: torch.Tensor      # (sum V, 3) fp32: the sum of g c over the views that see the vertex
    sum_w: torch.Tensor        # (sum V,) fp32: the sum of g
    seen: torch.Tensor         # (sum V,) int32: how many views see it
    best_w: torch.Tensor       # (sum V,) fp32: the largest g
    best: torch.Tensor         # (sum V,) int32: the first view that has it; -1 where none
    best_rgb: torch.Tensor     # (sum V, 3) fp32: that view's colour


def paint_state(n_verts, device) -> PaintState:
    """The state of ``paint_view`` before the first view: zeros, and ``best`` = -1."""
    n = int(n_verts)
    if n < 0:
        raise SnrError(f"paint_state: n_verts must not be negative, got {n_verts}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise SnrError("supnerf_amd operators need tensors on the GPU (no CPU fallback)")
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    return PaintState(z(n, 3), z(n), z(n, dtype=torch.int32), z(n), torch.full((n,), -1, dtype=torch.int32, device=dev), z(n, 3))


def _paint_dense(t, what, shape, dtype=torch.float32):
    """A buffer the paint kernels read or update where it lies: on the GPU, of this shape and type, contiguous -- nothing is converted."""
    _need_gpu(t)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
        raise SnrError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype}"
                       f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    return t


def _paint_state(state, nV, what):
    if not isinstance(state, PaintState):
        raise SnrError(f"{what}: state is what paint_state returns")
    i32 = torch.int32
    for name, shape, dtype in (("sum_rgb", (nV, 3), torch.float32), ("sum_w", (nV,), torch.float32), ("seen", (nV,), i32),
                               ("best_w", (nV,), torch.float32), ("best", (nV,), i32), ("best_rgb", (nV, 3), torch.float32)):
        _paint_dense(getattr(state, name), f"{what}: state.{name}", shape, dtype)
    return state


def paint_view(mesh, screen, normals, image, mask, depth, centre, tol, z_near, k, state):
    """One view painted into ``state`` in place (``snr_paint_view``; include/supnerf_hip.h, "Mesh painting", rules P1 - P4).  ``mesh``: the
    ``PackedMesh``; ``screen`` (sum V, 3): ``raster_project``'s for this view; ``normals`` (sum V, 3) or None (every view weighs 1);
    ``image`` (H, W, 3), ``mask`` (H, W) or None, ``depth`` (H, W): the view's photograph, its occupancy and ``raster_resolve``'s depth
    on one pixel grid; ``centre``: the camera centre in the frame of the stored vertices, three host floats; ``tol`` >= 0: how far behind
    the depth buffer a vertex may lie and still count as seen (camera z); ``k`` >= 0: the view's index.  Views go in ascending ``k`` on
    one stream.  Every tensor is read where it lies: fp32, contiguous, on the GPU, else ``SnrError``."""
    nV = mesh.verts.shape[0]
    _paint_dense(screen, "paint_view: screen", (nV, 3))
    if normals is not None:
        _paint_dense(normals, "paint_view: normals", (nV, 3))
    _need_gpu(image)
    if image.dim() != 3 or image.shape[2] != 3:
        raise SnrError(f"paint_view: image must be (H, W, 3), got {tuple(image.shape)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H * W >= 2 ** 31:
        raise SnrError(f"paint_view: an image of {H} x {W} pixels: the paint kernels take fewer than 2^31 pixels per view")
    _paint_dense(image, "paint_view: image", (H, W, 3))
    _paint_dense(depth, f"paint_view: depth (the image is {H} x {W})", (H, W))
    if mask is not None:
        _paint_dense(mask, f"paint_view: mask (the image is {H} x {W})", (H, W))
    centre = [float(c) for c in centre]
    tol, z_near, k = float(tol), float(z_near), int(k)
    if len(centre) != 3:
        raise SnrError(f"paint_view: centre is three numbers, got {len(centre)}")
    if not (tol >= 0 and math.isfinite(tol)):
        raise SnrError(f"paint_view: tol must be finite and not negative, got {tol}")
    if not z_near > 0:
        raise SnrError(f"paint_view: z_near must be positive, got {z_near}")
    if k < 0:
        raise SnrError(f"paint_view: the view index must not be negative, got {k}")
    _paint_state(state, nV, "paint_view")
    dev, i32 = mesh.verts.device, torch.int32
    with torch.cuda.device(dev):
        check(_lib.lib().snr_paint_view(_ptr(screen), _ptr(mesh.verts), _ptr(normals), nV, _ptr(image), _ptr(mask), _ptr(depth), H, W, *centre,
                                        tol, z_near, k, _ptr(state.sum_rgb), _ptr(state.sum_w), _ptr(state.seen, i32), _ptr(state.best_w),
                                        _ptr(state.best, i32), _ptr(state.best_rgb), _stream(dev)), "snr_paint_view")
    return state


def paint_finish(state, blend="weighted", background=0.0):
    """(colors (sum V, 3) fp32, filled (sum V,) int32) of a ``PaintState`` (``snr_paint_finish``; rule P5): per vertex some view saw the
    weighted mean of its views (``blend="weighted"``) or the colour of its best view (``"best"``) and filled = 0; ``background`` and -1
    elsewhere."""
    if blend not in PAINT_BLENDS:
        raise SnrError(f"blend is one of {PAINT_BLENDS}, got {blend!r}")
    if not isinstance(state, PaintState):
        raise SnrError("paint_finish: state is what paint_state returns")
    nV = state.seen.shape[0]
    _paint_state(state, nV, "paint_finish")
    dev, i32 = state.seen.device, torch.int32
    colors = torch.empty(nV, 3, device=dev)
    filled = torch.empty(nV, dtype=i32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_paint_finish(_ptr(state.sum_rgb), _ptr(state.sum_w), _ptr(state.seen, i32), _ptr(state.best_rgb), nV,
                                          PAINT_BLENDS.index(blend), float(background), _ptr(colors), _ptr(filled, i32), _stream(dev)),
              "snr_paint_finish")
    return colors, filled


def paint_fill(colors, filled, adjacency, rounds):
    """``rounds`` Jacobi rounds of rule P6 over a ``MeshAdjacency`` (``snr_paint_fill``): in round r = 1, 2, ... every vertex with
    ``filled`` < 0 that has a filled neighbour takes the mean of its filled neighbours' colours and ``filled`` = r.  One launch per round
    between two buffers, no host read; returns new (colors, filled), ``rounds=0`` copies."""
    rounds = int(rounds)
    if rounds < 0:
        raise SnrError(f"paint_fill: rounds must not be negative, got {rounds}")
    nV = sum(adjacency.n_verts)
    _paint_dense(colors, "paint_fill: colors", (nV, 3))
    _paint_dense(filled, "paint_fill: filled", (nV,), torch.int32)
    dev, i32 = colors.device, torch.int32
    cur, cur_f = colors.clone(), filled.clone()
    if rounds == 0 or nV == 0:
        return cur, cur_f
    lib, st, csr = _lib.lib(), _stream(dev), _smooth_csr(adjacency)
    with torch.cuda.device(dev):
        other, other_f = torch.empty_like(cur), torch.empty_like(cur_f)
        for r in range(1, rounds + 1):
            check(lib.snr_paint_fill(_ptr(cur), _ptr(cur_f, i32), *csr, r, _ptr(other), _ptr(other_f, i32), st), "snr_paint_fill")
            cur, other, cur_f, other_f = other, cur, other_f, cur_f
    return cur, cur_f


# ------------------------------------------------------------------------------------ ray-cast surfaces
def _ray_shapes(rays_o, rays_d, *per_ray):
    """R of rays_o, rays_d (R, 3) and any number of per-ray (R,) tensors: the sizes the ray kernels index by."""
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or tuple(rays_d.shape) != tuple(rays_o.shape):
        raise SnrError(f"rays_o and rays_d must both be (R, 3), got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
    R = rays_o.shape[0]
    for t in per_ray:
        if tuple(t.shape) != (R,):
            raise SnrError(f"a per-ray tensor of {R} rays must be ({R},), got {tuple(t.shape)}")
    return R


def ray_march_points(rays_o, rays_d, ta, tb, n_samples):
    """The (R n_samples, 3) point list of the march of [ta, tb] (R,) along rays_o + t rays_d (R, 3), ray-major: t_k = ta + step k with
    step = (tb - ta) / (n_samples - 1), the last sample tb itself (``snr_ray_march_points``)."""
    R, dev = _ray_shapes(rays_o, rays_d, ta, tb), rays_o.device
    if n_samples < 2:
        raise SnrError(f"a march takes at least 2 samples, got {n_samples}")
    xyz = torch.empty(R * n_samples, 3, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_ray_march_points(_ptr(rays_o), _ptr(rays_d), _ptr(ta), _ptr(tb), R, n_samples, _ptr(xyz), _stream(dev)),
              "snr_ray_march_points")
    return xyz


def ray_first_crossing(sigmas, ta, tb, level, va=None, vb=None, state=None):
    """The first crossing of ``level`` (outside -> inside, inside iff sigma >= level) in sigmas (R, S), the densities of the march of
    [ta, tb]; ``ta`` and ``tb`` (R,) are replaced IN PLACE by the crossing's bracket (``snr_ray_first_crossing``).  Without ``state``
    this is the first march: it decides state (R,) uint8 (2 starts inside, 1 crossing, 0 miss) and rays of state 0 / 2 get the dummy
    interval [ta, ta], va = vb = 0.  With ``state`` (and ``va``, ``vb``) it is a refinement: only state-1 rays change.  Returns
    (ta, tb, va, vb, state)."""
    if sigmas.dim() != 2 or not sigmas.is_contiguous() or tuple(ta.shape) != (sigmas.shape[0],) or tuple(tb.shape) != tuple(ta.shape):
        raise SnrError(f"ray_first_crossing takes dense sigmas (R, S) and ta, tb (R,), got {tuple(sigmas.shape)}, {tuple(ta.shape)}, "
                       f"{tuple(tb.shape)}")
    R, S = sigmas.shape
    dev = sigmas.device
    first = state is None
    if first:
        va, vb = torch.empty(R, device=dev), torch.empty(R, device=dev)
        state = torch.empty(R, dtype=torch.uint8, device=dev)
    elif va is None or vb is None or any(tuple(t.shape) != (R,) for t in (va, vb, state)):
        raise SnrError("a refinement march takes the va, vb and state (R,) of the march before it")
    with torch.cuda.device(dev):
        check(_lib.lib().snr_ray_first_crossing(_ptr(sigmas), R, S, level, int(first), _ptr(ta), _ptr(tb), _ptr(va), _ptr(vb),
                                                _ptr(state, torch.uint8), _stream(dev)), "snr_ray_first_crossing")
    return ta, tb, va, vb, state


def ray_hit_points(rays_o, rays_d, ta, tb, va, vb, state, level):
    """(depth (R,), width (R,), x (R, 3)) of the final brackets (``snr_ray_hit_points``): depth = ta + (level - va) / (vb - va) (tb - ta)
    and width = tb - ta on state 1; depth = ta (the near bound), width 0 on state 2; both 0 on state 0; x = rays_o + depth rays_d."""
    R, dev = _ray_shapes(rays_o, rays_d, ta, tb, va, vb, state), rays_o.device
    depth, width, xyz = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, 3, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_ray_hit_points(_ptr(rays_o), _ptr(rays_d), _ptr(ta), _ptr(tb), _ptr(va), _ptr(vb), _ptr(state, torch.uint8), R,
                                            level, _ptr(depth), _ptr(width), _ptr(xyz), _stream(dev)), "snr_ray_hit_points")
    return depth, width, xyz


def ray_brackets(rays_o, rays_d, near, far, latent, packed, level, n_samples, levels, refine_samples, shape_blocks, texture_blocks):
    """The search of ``RaySurface``: the first march of [near, far] with ``n_samples`` samples, then ``levels`` marches of the brackets
    with ``refine_samples``; each march is ``ray_march_points`` -> ``density_fwd`` -> ``ray_first_crossing``.  Returns
    (ta, tb, va, vb, state); nothing is read back to the host."""
    ta, tb = near.clone(), far.clone()
    va = vb = state = None
    for S in (n_samples,) + (refine_samples,) * levels:
        xyz = ray_march_points(rays_o, rays_d, ta, tb, S)
        sig, _ = density_fwd(xyz, latent, packed, shape_blocks, texture_blocks)
        ta, tb, va, vb, state = ray_first_crossing(sig.view(-1, S), ta, tb, level, va, vb, state)
    return ta, tb, va, vb, state


class RaySurface(torch.autograd.Function):
    """Along each of R = B n rays (object-major over the B objects of ``latent``), the first point where the density rises through
    ``level``: (depth (R,), state (R,) uint8, normal (R, 3), width (R,)).  Forward: ``ray_brackets``, ``ray_hit_points``, then the density
    forward (saving its ReLU bits) and backward (d sigma = 1) at the hit points x: g = grad sigma(x), normal = -g / |g| on state 1.
    Backward of the depth by the implicit function theorem on sigma(o + t d; code) = level at x: with slope = g . d and
    c = -d_depth / slope on state 1, 0 elsewhere: d rays_o = c g, d rays_d = t c g, d latent = ``density_bwd(d_sig = c)`` on the saved bits.
    With a latent gradient to form, the hit points of every object are padded to a multiple of 64 as ``DensityPoints`` pads.  ``near``,
    ``far`` and ``level`` get no gradient, nor does the topology (which crossing is first, hit or miss); nothing is clamped on a grazing ray."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, near, far, latent, packed, level, n_samples, levels, refine_samples, shape_blocks, texture_blocks):
        _need_gpu(rays_o, rays_d, near, far, latent, packed)
        o, d, latent = _f32c(rays_o.detach()), _f32c(rays_d.detach()), _f32c(latent.detach())
        R, B = o.shape[0], latent.shape[0]
        if R % B:
            raise SnrError(f"{R} rays do not split evenly over {B} objects")
        sb, tb = shape_blocks, texture_blocks
        br = ray_brackets(o, d, _f32c(near.detach()), _f32c(far.detach()), latent, packed, level, n_samples, levels, refine_samples, sb, tb)
        state = br[4]
        t, width, x = ray_hit_points(o, d, *br, level)
        ctx.pad = pad = ObjectPad(B, R // B, _tile_pad(R // B, 1, DENSITY_TILE) if (ctx.needs_input_grad[4] and sb + tb > 0) else 0)
        x = pad.pad(x)
        sig, masks = density_fwd(x, latent, packed, sb, tb, save_masks=True)
        g = pad.strip(density_bwd(x, latent, packed, masks, sig, torch.ones_like(sig), sb, tb, need_latent=False)[1])
        hit = state == 1
        norm = g.norm(dim=1, keepdim=True)
        good = hit[:, None] & torch.isfinite(norm) & (norm > 0)
        normal = torch.where(good, -g / torch.where(good, norm, torch.ones_like(norm)), torch.zeros_like(g))
        if any(ctx.needs_input_grad[i] for i in (0, 1, 4)):
            slope = g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1] + g[:, 2] * d[:, 2]
            ctx.save_for_backward(d, t, g, slope, hit, x, latent, packed, masks, sig)
            ctx.cfg = (sb, tb)
        ctx.mark_non_differentiable(state, normal, width)
        return t, state, normal, width

    @staticmethod
    def backward(ctx, d_t, _d_state, _d_normal, _d_width):
        d, t, g, slope, hit, x, latent, packed, masks, sig = ctx.saved_tensors
        sb, tb = ctx.cfg
        c = torch.where(hit, -_f32c(d_t) / slope, torch.zeros_like(t))
        d_o = c[:, None] * g if ctx.needs_input_grad[0] else None
        d_d = (t * c)[:, None] * g if ctx.needs_input_grad[1] else None
        d_lat = None
        if ctx.needs_input_grad[4]:
            d_lat, _ = density_bwd(x, latent, packed, masks, sig, ctx.pad.pad(c), sb, tb, need_latent=True, need_xyz=False)
        return d_o, d_d, None, None, d_lat, None, None, None, None, None, None, None


def weight_grad(G, n_out, X, n_in, want_bias=True, out=None, ws=None, precision="fp32"):
    """dW (n_out, n_in) = G[:, :n_out]^T X[:, :n_in] and db (n_out,) = column sums of G, one split-K MFMA launch + one reduction
    (include/supnerf_hip.h: snr_weight_grad).  G, X: 2-D fp32 row-major views (a column slice of a wider buffer is fine).  ``out``:
    optional (dW_view, db) to write into (dW_view may be a column block of a wider matrix).  ``precision``: "fp32" (exact) or "bf16x3"
    (split-bf16 products, ~2^-17 operand error, several times faster; bias sums and narrow heads stay fp32)."""
    if precision not in PRECISIONS:
        raise SnrError(f"weight_grad: precision must be 'fp32' or 'bf16x3', got {precision!r}")
    _need_gpu(G, X)
    if G.dim() != 2 or X.dim() != 2 or G.shape[0] != X.shape[0] or G.stride(1) != 1 or X.stride(1) != 1 or G.dtype != torch.float32 or X.dtype != torch.float32:
        raise SnrError(f"weight_grad: G {tuple(G.shape)} / X {tuple(X.shape)} must be fp32 (P, n) row-major views of the same points")
    if n_out > G.shape[1] or n_in > X.shape[1]:
        raise SnrError("weight_grad: n_out / n_in exceed the operands' columns")
    P, dev = G.shape[0], G.device
    dW, db = out if out is not None else (torch.empty(n_out, n_in, device=dev), torch.empty(n_out, device=dev) if want_bias else None)
    if dW.stride(1) != 1:
        raise SnrError("weight_grad: dW must be row-major")
    nbytes = _lib.lib().snr_weight_grad_ws_bytes(P, n_out, n_in)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_weight_grad(_p_rows(G), G.stride(0), n_out, _p_rows(X), X.stride(0), n_in, P, _p_rows(dW), dW.stride(0), _p(db), PRECISIONS[precision],
                                         _p(ws), ws.numel(), _stream(dev)), "snr_weight_grad")
    return dW, db


def pe_points(xyz, viewdir):
    """(P,96) = PE(xyz) (63 columns, 1 zero) | PE(viewdir) (27 columns, 5 zeros): include/supnerf_hip.h snr_pe_points."""
    xyz, viewdir = _f32c(xyz), _f32c(viewdir)
    _need_gpu(xyz, viewdir)
    P, dev = xyz.shape[0], xyz.device
    if xyz.shape != (P, 3) or viewdir.shape != (P, 3):
        raise SnrError("pe_points: xyz and viewdir must both be (P,3)")
    out = torch.empty(P, 96, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_pe_points(_p(xyz), _p(viewdir), P, _p(out), _stream(dev)), "snr_pe_points")
    return out


_PACK_CACHE = {}
_PACK_LOCK = threading.Lock()


def _packed_for(names, weights, shape_blocks, texture_blocks):
    """The packed stream of these per-point weights, re-packed only when a tensor changed (every optimiser step bumps the versions; an
    evaluation pass between two steps, or a second forward before the update, re-uses the buffer).  One slot per device (DataParallel enters
    from one thread per GPU).  A hit must PROVE identity: the entry holds weak references to the very tensors it was packed from, and
    ``ref() is w`` is required for every one -- (data_ptr, _version) alone would also match a NEW model whose weights the caching
    allocator placed at a freed model's addresses (same construction, same version counters), and the step would silently run on the
    old model's weights."""
    dev = (weights[0].device, raw_stream(weights[0].device) if weights[0].is_cuda else 0)   # (one slot per device AND stream)
    key = (shape_blocks, texture_blocks) + tuple((w.data_ptr(), w._version) for w in weights)
    with _PACK_LOCK:
        hit = _PACK_CACHE.get(dev)
        if hit is not None and hit[0] == key and len(hit[1]) == len(weights) and all(r() is w for r, w in zip(hit[1], weights)):
            return hit[2]
    packed = pack_weights(dict(zip(names, weights)), shape_blocks, texture_blocks)
    with _PACK_LOCK:
        while len(_PACK_CACHE) >= 16:
            _PACK_CACHE.pop(next(iter(_PACK_CACHE)))
        _PACK_CACHE[dev] = (key, [weakref.ref(w) for w in weights], packed)
    return packed


def sigma_pre_grad(d_sig, sig):
    """Gradient wrt the density head's pre-activation from the upstream ``d_sig`` and the saved density sigma = softplus(pre):
    softplus'(pre) = sigmoid(pre) = 1 - exp(-sigma), formed as -expm1(-sigma).  (1 - exp(-sigma) is exactly 0 in fp32 for sigma below ~6e-8,
    where sigmoid(pre) ~ sigma still carries the gradient of the 1e10-wide last interval; past the softplus threshold it is 1.)"""
    return d_sig * -torch.expm1(-sig)


class DecoderPointsTrain(torch.autograd.Function):
    """Training-mode decoder (SURVEY 8a9 mode B): like DecoderPoints but the per-point decoder WEIGHTS are inputs too and
    receive gradients.  The layer-chain kernels additionally write every layer's input X_l (forward) and pre-activation
    gradient G_l (backward) to HBM, and the weight gradients dW_l = G_l^T X_l, db_l = sum_p G_l come from the split-K MFMA kernels
    behind ``weight_grad`` (no library BLAS).  ``precision``: "fp32" = exact fp32 MFMA throughout; "bf16x3" = split-bf16
    products in all three (the chains and the weight-gradient product; bias sums and the two narrow heads stay fp32); a pair
    (forward chain, backward chain) -- the products follow the backward chain -- or a triple (forward chain, backward chain, products),
    e.g. ("fp32", "bf16x3", "bf16x3"): exact fp32 forward, split-bf16 backward chain (on the ReLU bits the forward saved) and
    weight-gradient products.  ``weights`` = the
    per-point tensors in per_point_tensor_names order."""

    @staticmethod
    def forward(ctx, xyz, viewdir, latent, shape_blocks, texture_blocks, precision, *weights):
        xyz, viewdir, latent = _f32c(xyz), _f32c(viewdir), _f32c(latent)
        # ragged point counts per object: padded to whole wave tiles with dummy points like DecoderPoints (zero upstream gradient, so they add
        # nothing to any weight gradient either)
        B, P0 = max(latent.shape[0], 1), xyz.shape[0]
        n_pad = _tile_pad(P0 // B) if (shape_blocks + texture_blocks > 0 and P0 % B == 0 and P0 > 0) else 0
        ctx.pad = pad = ObjectPad(B, P0 // B, n_pad)
        xyz, viewdir = pad.pad(xyz), pad.pad(viewdir)
        # one arithmetic for the whole step: the forward / backward layer chains and the weight-gradient products
        # ``precision``: one name for the whole step, (forward chain, backward chain) -- the products follow the backward chain -- or (forward
        # chain, backward chain, products); ("fp32", "auto", "bf16x3") is what "auto" trains in (model.forward): the forward chain decides
        # where a training run ends up, what runs behind it does not
        wgrad_override = precision[2] if isinstance(precision, tuple) and len(precision) == 3 else None
        per_obj = xyz.shape[0] // max(latent.shape[0], 1)
        prec = resolve_precision(precision, shape_blocks, texture_blocks, per_obj)
        prec_bwd = resolve_precision(precision, shape_blocks, texture_blocks, per_obj, backward=True)
        wgrad_precision = wgrad_override or ("bf16x3" if prec_bwd == BF16X3 else "fp32")       # (a pair: the products follow the backward chain)
        if wgrad_precision not in ("fp32", "bf16x3"):
            raise SnrError(f"weight-gradient products run in 'fp32' or 'bf16x3', not {wgrad_precision!r}")
        names = per_point_tensor_names(shape_blocks, texture_blocks)
        packed = _packed_for(names, weights, shape_blocks, texture_blocks)
        P, dev = xyz.shape[0], xyz.device
        n_slots = sum(l.slot is not None for l in decoder_layers(shape_blocks, texture_blocks))
        act = torch.empty(n_slots, P, 256, device=dev)
        sig, rgb, masks = decoder_fwd(xyz, viewdir, latent, packed, shape_blocks, texture_blocks, save_masks=True, precision=prec,
                                      activations=act)
        ctx.save_for_backward(xyz, viewdir, latent, packed, masks, sig, act, *weights)
        ctx.cfg = (shape_blocks, texture_blocks, wgrad_precision, prec_bwd)
        return pad.strip(sig), pad.strip(rgb)

    @staticmethod
    def backward(ctx, d_sig, d_rgb):
        xyz, viewdir, latent, packed, masks, sig, act, *weights = ctx.saved_tensors
        sb, tb, wprec, prec = ctx.cfg
        P, dev = xyz.shape[0], xyz.device
        layers = decoder_layers(sb, tb)
        n_slots = sum(l.slot is not None for l in layers)
        G = torch.empty(n_slots, P, 256, device=dev)
        pad = ctx.pad
        d_sig, d_rgb = pad.pad(_f32c(d_sig)), pad.pad(_f32c(d_rgb))
        d_lat, d_xyz, d_dir = decoder_bwd(xyz, viewdir, latent, packed, masks, sig, d_sig, d_rgb, sb, tb,
                                          ctx.needs_input_grad[2], ctx.needs_input_grad[0], ctx.needs_input_grad[1], precision=prec,
                                          layer_grads=G)
        # ---- weight gradients: dW_l = G_l^T X_l, db_l = sum_p G_l on the split-K MFMA kernel (snr_weight_grad), one launch + one
        # reduction per layer; X of layer 0 and the direction features are the positional encodings, one launch of snr_pe_points (``pe``:
        # columns 0..63 PE(xyz), 64..95 PE(dir); round 2 recomputed them with torch.sin / cos / cat: 0.3 ms a step)
        pe = pe_points(xyz, viewdir)
        ws = torch.empty(_lib.lib().snr_weight_grad_ws_bytes(P, 256, 256), dtype=torch.uint8, device=dev)
        grads = {}
        for l in layers:                       # MFMA layers in order; the two small heads follow
            if l.slot is None:
                continue
            li, n_pe = l.slot, l.n_in % 256    # n_in = the 256 columns of the activation before it (not the first layer) + positional-encoding columns
            k_pe = (n_pe + 3) // 4 * 4         # (as pe_points pads them: 63 -> 64, 27 -> 28)
            if l.n_in < 256:                   # encoding_xyz: PE(xyz)
                dW, db = weight_grad(G[li], l.n_out, pe[:, :64], k_pe, ws=ws, precision=wprec)
                grads[l.stem] = (dW[:, :n_pe].contiguous(), db)
            elif n_pe:                         # encoding_viewdir: act || PE(dir)
                dW = torch.empty(l.n_out, 256 + k_pe, device=dev)
                _, db = weight_grad(G[li], l.n_out, act[li - 1], 256, out=(dW[:, :256], torch.empty(l.n_out, device=dev)), ws=ws, precision=wprec)
                weight_grad(G[li], l.n_out, pe[:, 64:], k_pe, out=(dW[:, 256:], None), ws=ws, precision=wprec)
                grads[l.stem] = (dW[:, :l.n_in].contiguous(), db)
            else:
                grads[l.stem] = weight_grad(G[li], l.n_out, act[li - 1], 256, ws=ws, precision=wprec)
        # the heads read the output of the layer before them: sigma.0 (pre = w . y + b) the input of enc_viewdir, rgb.2 that of rgb.0
        upstream = {"sigma.0": sigma_pre_grad(d_sig, sig).reshape(P, 1), "rgb.2": d_rgb.reshape(P, 3)}
        for before, l in zip(layers, layers[1:]):
            if l.slot is None:
                grads[l.stem] = weight_grad(upstream[l.stem], l.n_out, act[before.slot], l.n_in, ws=ws)
        out = [g for l in layers for g in grads[l.stem]]
        return (pad.strip(d_xyz), pad.strip(d_dir), d_lat, None, None, None, *out)


# ------------------------------------------------------------------------------------ fused render
def _render_args(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, frame, xyz_mul, z_mode, flags, rays_per_obj,
                 n_samples, shape_blocks, texture_blocks, precision=FP32, latent_bias=None, box_half=None, rng=None):
    a = RenderArgs()
    a.rays_o, a.rays_d, a.t_vals = _ptr(rays_o), _ptr(rays_d), _ptr(t_vals)
    a.xyz_div, a.z_scale = _ptr(xyz_div), _ptr(z_scale)
    a.latent, a.packed = _ptr(latent), _ptr(packed)
    a.frame = (C.c_float * 9)(*[float(v) for v in frame])
    a.xyz_mul = float(xyz_mul)
    a.z_mode, a.flags = int(z_mode), int(flags)
    a.n_rays, a.rays_per_obj = int(rays_o.shape[0]), int(rays_per_obj)
    a.n_samples, a.shape_blocks, a.texture_blocks = int(n_samples), int(shape_blocks), int(texture_blocks)
    a.precision = int(precision)
    a.latent_bias = _ptr(latent_bias)
    a.box_half = _ptr(box_half)
    a.rng_seed, a.rng_offset, a.rng_threads = [int(v) & 0xFFFFFFFFFFFFFFFF for v in (rng if rng is not None else (0, 0, 0))]
    # sizes the kernels index with: a short buffer here is an out-of-bounds read on the device
    N, S, B = a.n_rays, a.n_samples, max(a.n_rays // max(a.rays_per_obj, 1), 1)
    if rays_o.numel() != 3 * N or rays_d.numel() != 3 * N:
        raise SnrError(f"render: rays_o {tuple(rays_o.shape)} / rays_d {tuple(rays_d.shape)} are not (N,3)")
    want_t = {Z_SHARED: S, Z_PER_OBJECT: B * S, Z_PER_RAY: N * S, Z_BOX: N * S}[a.z_mode]
    if t_vals is not None and t_vals.numel() != want_t:
        raise SnrError(f"render: depths / jitter hold {t_vals.numel()} values, z_mode {a.z_mode} needs {want_t}")
    if a.z_mode == Z_BOX:
        if box_half is None or box_half.numel() != 3 * B or z_scale is None:
            raise SnrError("render: box sampling needs box_half (B,3) and z_scale (B,)")
    elif t_vals is None or xyz_div is None:
        raise SnrError("render: depths and xyz_div are required")
    for t, name in ((xyz_div, "xyz_div"), (z_scale, "z_scale")):
        if t is not None and t.numel() < B:
            raise SnrError(f"render: {name} holds {t.numel()} values for {B} objects")
    return a


def reserve_rand_like(dev, numel):
    """(seed, offset, threads) describing what ``torch.rand_like`` of ``numel`` floats would draw from ``dev``'s default generator
    right now, and advance the generator exactly as that call would (aten/src/ATen/native/cuda/DistributionTemplates.h:
    calc_execution_policy).  The box-sampling kernels regenerate those numbers themselves (family B's jitter, src/renderer.py:40), so a
    seeded run consumes the generator like the reference without an (N,S) tensor or an extra launch."""
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    props = torch.cuda.get_device_properties(idx)
    block = 256
    grid = min(props.multi_processor_count * (props.max_threads_per_multi_processor // block), (numel + block - 1) // block)
    threads = max(grid, 1) * block
    seed, offset = gen.initial_seed(), gen.get_offset()
    gen.set_offset(offset + ((max(numel, 1) - 1) // (threads * 4) + 1) * 4)
    return seed, offset, threads


def render_probe(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg, precision):
    """The fused forward once more, without autograd and WITHOUT consuming the device generator (box sampling with in-kernel jitter draws
    from the state the real launch is about to reserve): (rgb, depth, acc_trans) in ``precision``.  Used by the range guard of ``auto``."""
    c = cfg.replace(precision=precision)
    with torch.no_grad():
        if c.z_mode == Z_BOX and t_vals is None and c.rng is None:
            dev = torch.device(rays_o.device)
            gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
            off = gen.get_offset()
            c.rng = reserve_rand_like(dev, rays_o.shape[0] * c.n_samples)
            gen.set_offset(off)
        return render_fwd(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, c)[:3]


def fused_supported(n_samples: int) -> bool:
    """The single-launch render needs every ray inside one 128-point workgroup tile."""
    return 1 <= n_samples <= 128 and 128 % n_samples == 0


class RenderCfg:
    """Per-launch constants of the render operators (not tensors)."""

    def __init__(self, n_samples, z_mode, rays_per_obj, shape_blocks, texture_blocks, frame=IDENTITY_FRAME, xyz_mul=1.0,
                 white_bkgd=False, metric_z=False, precision=None, box_half=None, box_detach=False):
        self.n_samples, self.z_mode, self.rays_per_obj = n_samples, z_mode, rays_per_obj
        # "fp32" | "bf16x3" | "auto" | None.  None = not chosen here: ``model.fused_render`` substitutes the module's ``precision``; the
        # bare operators (render_fwd, encode) treat it as "auto", the library default.  (It used to default to "fp32", which made
        # every caller that did not pass it run the exact kernels whatever the module said.)
        self.precision = precision
        self.shape_blocks, self.texture_blocks = shape_blocks, texture_blocks
        self.frame, self.xyz_mul = tuple(float(v) for v in frame), float(xyz_mul)
        self.flags = (WHITE_BKGD if white_bkgd else 0) | (METRIC_Z if metric_z else 0) | (BOX_DETACH if box_detach else 0)
        # optional (B, NLAT, 256) fp32 on the device: the latent terms folded into the next layers' biases (model.latent_biases);
        # forward only, no gradient flows through it (the backward kernel returns the gradient of the latent terms themselves)
        self.latent_bias = None
        # z_mode Z_BOX (family B, src/renderer.py:91-115): (B,3) half extents of the objects' boxes on the device; the depths argument of the
        # operators then is the (N,S) jitter or None = drawn in the kernel from ``rng`` = (seed, offset, threads), see reserve_rand_like
        self.box_half = box_half
        self.rng = None

    def replace(self, **changes):
        """A shallow copy with the named attributes set: THE per-launch copy (a launch records its generator state in its own)."""
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__, **changes)
        return c


def _box_rng(cfg, t_vals, dev, n_points):
    """Box sampling without a caller-supplied jitter: fix the generator state the kernels will draw from (once per forward; the
    backward replays it from the same cfg)."""
    if cfg.z_mode == Z_BOX and t_vals is None and cfg.rng is None:
        cfg.rng = reserve_rand_like(dev, n_points)


def render_fwd(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg: RenderCfg, save_for_bwd=False):
    rays_o, rays_d, t_vals, xyz_div, z_scale, latent = [_f32c(t) for t in (rays_o, rays_d, t_vals, xyz_div, z_scale, latent)]
    _need_gpu(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed)
    if not fused_supported(cfg.n_samples):
        raise SnrError(f"fused render needs n_samples dividing 128 (got {cfg.n_samples}); use the unfused operators")
    dev = rays_o.device
    N, S = rays_o.shape[0], cfg.n_samples
    rgb = torch.empty(N, 3, device=dev)
    depth = torch.empty(N, device=dev)
    acc = torch.empty(N, device=dev)
    sig = rgbs = masks = None
    if save_for_bwd:
        sig = torch.empty(N * S, device=dev)
        rgbs = torch.empty(N * S, 3, device=dev)
        masks = torch.empty(_lib.lib().snr_mask_bytes(N * S, cfg.shape_blocks, cfg.texture_blocks), dtype=torch.uint8, device=dev)
    prec = resolve_precision(cfg.precision, cfg.shape_blocks, cfg.texture_blocks, cfg.rays_per_obj * S)
    lb = cfg.latent_bias
    if lb is not None:
        lb = _f32c(lb.detach())
        if lb.shape != latent.shape or lb.device != dev:
            raise SnrError(f"latent_bias must match the latent terms: {tuple(lb.shape)} on {lb.device} vs {tuple(latent.shape)} on {dev}")
    _box_rng(cfg, t_vals, dev, N * S)
    bh = _f32c(cfg.box_half)
    a = _render_args(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg.frame, cfg.xyz_mul, cfg.z_mode, cfg.flags,
                     cfg.rays_per_obj, S, cfg.shape_blocks, cfg.texture_blocks, prec, latent_bias=lb, box_half=bh, rng=cfg.rng)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_render_fwd(C.byref(a), _p(rgb), _p(depth), _p(acc), _p(sig), _p(rgbs), _p(masks), _stream(dev)),
              "snr_render_fwd")
    return rgb, depth, acc, sig, rgbs, masks


def pad_render_inputs(rays_o, rays_d, t_vals, z_scale, cfg, B, n, n_pad):
    """Every object's n rays padded to n_pad with dummy rays (whole 32-point wave tiles per object); returns the padded operands and a
    copy of ``cfg`` for the padded launch; ``z_scale`` (B,), one per object, comes back unchanged (the ABI has no per-ray scale).
    Box sampling with in-kernel jitter (Z_BOX, no jitter tensor): the kernel's Philox stream is indexed by the LAUNCH's point index, which padding shifts -- so the reference's draw, ``torch.rand_like`` of the caller's (N,S) table
    (src/renderer.py:40: the same numbers and the same generator consumption), is materialised BEFORE padding and padded like any other
    jitter table; seeded parity with the reference survives ragged ray counts."""
    cfg = cfg.replace(rays_per_obj=n_pad)       # (z_scale is (B,), one per object like xyz_div: padding rays leaves it as it is)
    if cfg.z_mode == Z_BOX and t_vals is None and cfg.rng is None:
        t_vals = torch.rand(B * n, cfg.n_samples, device=rays_o.device)
    rays_o, rays_d = _pad_rows(rays_o, B, n, n_pad), _pad_rows(rays_d, B, n, n_pad)
    if cfg.z_mode in (Z_PER_RAY, Z_BOX) and t_vals is not None:
        t_vals = _pad_rows(t_vals, B, n, n_pad)
    if cfg.z_mode == Z_BOX:             # (a dummy ray with direction 0 would divide 0 by 0 in the slab test: give it any unit direction)
        rays_d = rays_d.clone()
        rays_d.view(B, n_pad, 3)[:, n:, 2] = 1.0
    return rays_o, rays_d, t_vals, z_scale, cfg


class FusedRender(torch.autograd.Function):
    """rays -> (rgb, depth, acc_trans) in one launch; backward in one launch (+ a small reduction).  ``t_vals``: the depths in
    ``cfg.z_mode``'s layout; for Z_BOX the (N,S) jitter, or None (drawn in the kernel).  Gradients: rays_o, rays_d, latent always; t_vals for
    per-ray depths; for Z_BOX the gradient through the box bounds is part of d_rays_o / d_rays_d."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg):
        rays_o, rays_d, t_vals, xyz_div, z_scale, latent = [_f32c(t) for t in (rays_o, rays_d, t_vals, xyz_div, z_scale, latent)]
        need = any(ctx.needs_input_grad[:6])
        ctx.set_materialize_grads(False)        # (e.g. the depth output of an optimise iteration: the kernel takes null upstream gradients)
        # few samples per ray (S < 32) and a ray count that leaves a partial 32-point wave tile per object: pad every object with dummy rays
        # (see DecoderPoints); the outputs and gradients of the dummies are dropped
        n = cfg.rays_per_obj
        B = rays_o.shape[0] // n if n else 0
        n_pad = _tile_pad(n, cfg.n_samples) if (ctx.needs_input_grad[5] and cfg.shape_blocks + cfg.texture_blocks > 0 and B > 0) else 0
        ctx.pad = pad = ObjectPad(B, n, n_pad)
        if n_pad:
            rays_o, rays_d, t_vals, z_scale, cfg = pad_render_inputs(rays_o, rays_d, t_vals, z_scale, cfg, *pad)
        else:
            cfg = cfg.replace()                 # (the launch's generator state is recorded in it: one copy per call)
        rgb, depth, acc, sig, rgbs, masks = render_fwd(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg, save_for_bwd=need)
        if need:
            ctx.save_for_backward(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, sig, rgbs, masks)
            ctx.cfg = cfg
        return pad.strip(rgb), pad.strip(depth), pad.strip(acc)

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_acc):
        rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, sig, rgbs, masks = ctx.saved_tensors
        cfg = ctx.cfg
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            raise SnrError("xyz_div / z_scale are per-object constants (object size); no gradient is provided")
        need_t = ctx.needs_input_grad[2]
        if need_t and cfg.z_mode != Z_PER_RAY:
            raise SnrError("gradient wrt shared / per-object depths or the box jitter is not provided (the reference detaches them)")
        if d_rgb is None and d_depth is None and d_acc is None:
            return None, None, None, None, None, None, None, None
        pad = ctx.pad
        d_o, d_d, d_t, d_lat = render_bwd(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg, sig, rgbs, masks,
                                          pad.pad(d_rgb), pad.pad(d_depth), pad.pad(d_acc),
                                          need_o=ctx.needs_input_grad[0], need_d=ctx.needs_input_grad[1], need_t=need_t,
                                          need_latent=ctx.needs_input_grad[5])
        return pad.strip(d_o), pad.strip(d_d), pad.strip(d_t), None, None, d_lat, None, None


def render_bwd(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg: RenderCfg, sig, rgbs, masks, d_rgb, d_depth, d_acc,
               need_o=True, need_d=True, need_t=False, need_latent=True):
    """Backward of the fused render on what ``render_fwd(..., save_for_bwd=True)`` saved: one launch + the small reduction of the
    latent-term partials.  Returns (d_rays_o, d_rays_d, d_t, d_latent), None where not asked for.  Any operand may be a strided view
    (get_rays' origins, for one, are a stride-0 view of the pose's 3 numbers): everything is made dense here."""
    rays_o, rays_d, t_vals, xyz_div, z_scale, latent = [_f32c(t) for t in (rays_o, rays_d, t_vals, xyz_div, z_scale, latent)]
    sig, rgbs, d_rgb, d_depth, d_acc = [_f32c(t) for t in (sig, rgbs, d_rgb, d_depth, d_acc)]
    _need_gpu(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, sig, rgbs, masks, d_rgb, d_depth, d_acc)
    if sig is None or rgbs is None or masks is None:
        raise SnrError("render_bwd needs what render_fwd(..., save_for_bwd=True) saved: per-point sigmas, rgbs and the ReLU bits")
    if cfg.z_mode == Z_BOX and t_vals is None and cfg.rng is None:
        raise SnrError("render_bwd: box sampling with in-kernel jitter needs the cfg the forward ran with (it holds the generator state)")
    masks, packed = masks.contiguous(), packed.contiguous()
    dev = rays_o.device
    N, S = rays_o.shape[0], cfg.n_samples
    if sig.numel() != N * S or rgbs.numel() != 3 * N * S or masks.numel() < _lib.lib().snr_mask_bytes(N * S, cfg.shape_blocks, cfg.texture_blocks):
        raise SnrError(f"render_bwd: saved sigmas / rgbs / ReLU bits do not belong to {N} rays x {S} samples")
    for t, k, name in ((d_rgb, 3 * N, "d_rgb"), (d_depth, N, "d_depth"), (d_acc, N, "d_acc")):
        if t is not None and t.numel() != k:
            raise SnrError(f"render_bwd: {name} holds {t.numel()} values, expected {k}")
    if need_latent and cfg.shape_blocks + cfg.texture_blocks > 0 and _tile_pad(cfg.rays_per_obj, cfg.n_samples):
        raise SnrError(f"gradient wrt the latent codes needs whole 32-point wave tiles per object, got {cfg.rays_per_obj} rays x {cfg.n_samples} "
                       "samples per object: pad the ray batch of every object so that rays x samples is a multiple of 32, or detach the codes")
    if need_t and cfg.z_mode != Z_PER_RAY:
        raise SnrError("render_bwd: d_t exists for per-ray depths only")
    d_lat = torch.empty_like(latent) if need_latent else None
    d_o = torch.empty_like(rays_o) if need_o else None      # (the kernel writes every ray's gradient exactly once: no memset)
    d_d = torch.empty_like(rays_d) if need_d else None
    d_t = torch.empty_like(t_vals) if need_t else None
    bh = _f32c(cfg.box_half)
    a = _render_args(rays_o, rays_d, t_vals, xyz_div, z_scale, latent, packed, cfg.frame, cfg.xyz_mul, cfg.z_mode, cfg.flags,
                     cfg.rays_per_obj, cfg.n_samples, cfg.shape_blocks, cfg.texture_blocks,
                     resolve_precision(cfg.precision, cfg.shape_blocks, cfg.texture_blocks, cfg.rays_per_obj * cfg.n_samples, backward=True),
                     box_half=bh, rng=cfg.rng)
    ws_bytes = _lib.lib().snr_render_bwd_ws_bytes(C.byref(a))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_render_bwd(C.byref(a), _p(sig), _p(rgbs), _p(masks), _p(d_rgb), _p(d_depth), _p(d_acc), _p(d_lat), _p(d_o), _p(d_d),
                                        _p(d_t), _p(ws), ws_bytes, _stream(dev)), "snr_render_bwd")
    return d_o, d_d, d_t, d_lat


# ------------------------------------------------------------------------------------ encode
def encode(rays_o, rays_d, t_vals, xyz_div, z_scale, cfg: RenderCfg, want_pe=False, want_hit=False):
    """Sample points of a ray packet: xyz (N,S,3), viewdir (N,S,3), z (N,S) [, PE(xyz) (N,S,63), PE(dir) (N,27)] [, hit (N) bool: the
    rays that meet their box, Z_BOX]."""
    rays_o, rays_d, t_vals, xyz_div, z_scale = [_f32c(t) for t in (rays_o, rays_d, t_vals, xyz_div, z_scale)]
    _need_gpu(rays_o, rays_d, t_vals, xyz_div, z_scale)
    dev = rays_o.device
    N, S = rays_o.shape[0], cfg.n_samples
    xyz = torch.empty(N, S, 3, device=dev)
    vd = torch.empty(N, S, 3, device=dev)
    z = torch.empty(N, S, device=dev)
    pe = torch.empty(N, S, 63, device=dev) if want_pe else None
    ped = torch.empty(N, 27, device=dev) if want_pe else None
    hit = torch.empty(N, dtype=torch.uint8, device=dev) if want_hit else None
    _box_rng(cfg, t_vals, dev, N * S)
    bh = _f32c(cfg.box_half)
    a = _render_args(rays_o, rays_d, t_vals, xyz_div, z_scale, None, None, cfg.frame, cfg.xyz_mul, cfg.z_mode, cfg.flags,
                     cfg.rays_per_obj, S, cfg.shape_blocks, cfg.texture_blocks, box_half=bh, rng=cfg.rng)
    with torch.cuda.device(dev):
        check(_lib.lib().snr_encode_fwd(C.byref(a), _p(xyz), _p(vd), _p(z), _p(pe), _p(ped), _p(hit), _stream(dev)), "snr_encode_fwd")
    out = (xyz, vd, z, pe, ped) if want_pe else (xyz, vd, z)
    return out + (hit.bool(),) if want_hit else out
