"""Family-B renderer API: ``NeRFRenderer``, ``render_rays_v3`` and ``volume_rendering3`` with the
signatures of the reference's src/renderer.py, on the HIP kernels.

Family B samples between per-ray box entry / exit depths (ray-AABB slab test in the frame where the
object diagonal is 2), composites against a white background by default and reports metric depth
``|xyz - o| * diag/2``.  From ``(rays_o, viewdir, obj_sz)`` on, everything is ONE launch (``SNR_Z_BOX``): the slab
test, the hit / miss bounds, the stratified per-ray depths, points, positional encoding, decoder and composite;
the backward launch returns the gradient through the box bounds to origins and directions like the reference's
autograd through ``ray_box_intersection_tensor``.  The jitter is the reference's ``torch.rand_like`` draw from the
device generator, regenerated inside the kernel (``ops.reserve_rand_like``) -- no (N,S) tensor exists.  Sample counts
that are not a power of two dividing 128, foreign decoders and CPU inputs take the torch formulation of the same
arithmetic (slab test and depth table as tensor ops, then the encode / decoder / composite launches).
"""
import numpy as np
import torch

from . import ops
from . import utils as U
from ._lib import SnrError
from .ops import Z_BOX, Z_PER_RAY


def volume_rendering3(sigmas, rgbs, z_vals, white_bkgd=False):
    """src/renderer.py:355-379: per-ray z_vals (N,S)."""
    return U._composite(sigmas, rgbs, z_vals, Z_PER_RAY, white_bkgd)


_unit_depths = U._unit_depths     # the stratified per-ray depth table lives beside its module-level twin, utils.sample_from_rays_v2

# True: family B's jitter is drawn inside the kernels from the device generator's state (same numbers torch.rand_like would give, same
# generator consumption).  False: torch.rand_like makes the (N,S) table and the kernels read it.
KERNEL_JITTER = True
_BOX_CONST = {}


def _box_constants(obj_sz, B, dev):
    """(diag, box_half (B,3), z_scale (B,)) on ``dev`` for B objects of size obj_sz = (w, l, h), cached: the half extents
    (l, w, h) / diag and the frame scale diag / 2 of src/renderer.py:92-103 never change for an object."""
    sz = np.asarray(obj_sz)
    key = (tuple(float(v) for v in sz.reshape(-1)), str(sz.dtype), int(B), U._stream_key(dev))
    hit = _BOX_CONST.get(key)
    if hit is None:
        diag = np.linalg.norm(sz).astype(np.float32)
        w, l, h = sz
        half = np.asarray([l / diag, w / diag, h / diag]).astype(np.float32)
        hit = U._cache_put(_BOX_CONST, key, (diag, torch.from_numpy(half).to(dev)[None, :].repeat(B, 1).contiguous(),
                                             torch.full((B,), float(diag / 2), device=dev)), limit=64)
    return hit


def _pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def _box_bounds(rays_o_n, viewdir, obj_sz, diag):
    """near/far (N,1) of the box with half extents (l,w,h)/diag; rays that miss get -1/-1
    (src/renderer.py:95-107).  The values are the reference's; the gradient follows the one-launch path's rule for a direction component
    that is exactly 0 (``utils._slab_guarded``), so both paths agree on a finite pose gradient for axis-parallel rays."""
    w, l, h = [float(v) for v in obj_sz]
    half = torch.tensor([l / diag, w / diag, h / diag], dtype=torch.float32, device=rays_o_n.device)
    t_near, t_far, hit = U._slab_guarded(rays_o_n, viewdir, -half.expand_as(rays_o_n), half.expand_as(rays_o_n))
    minus1 = torch.full_like(t_near, -1.0)
    return torch.where(hit, t_near, minus1)[:, None], torch.where(hit, t_far, minus1)[:, None], hit


class NeRFRenderer(torch.nn.Module):
    """src/renderer.py:15-352."""

    def __init__(self, n_samples=64, noise_std=0.0, white_bkgd=True):
        super().__init__()
        self.n_samples = n_samples
        self.noise_std = noise_std
        self.white_bkgd = white_bkgd

    def sample_from_ray(self, rays):
        """rays (N,8) = [origin, direction, near, far] -> depths (N,S)."""
        return _unit_depths(rays[:, -2:-1], rays[:, -1:], self.n_samples)

    def volume_render(self, sigmas, rgbs, z_vals):
        """src/renderer.py:43-65: sigmas (N,S), rgbs (N,S,3), z_vals (N,S)."""
        return U._composite(sigmas, rgbs, z_vals, Z_PER_RAY, self.white_bkgd)

    def volume_render_batch(self, sigmas, rgbs, z_vals):
        """src/renderer.py:67-89: leading batch dimension, z_vals (B,n,S)."""
        B, n, S = rgbs.shape[:3]
        sig = sigmas.squeeze(-1) if sigmas.dim() == rgbs.dim() else sigmas
        rgb, depth, acc = ops.Composite.apply(sig.reshape(B * n, S), rgbs.reshape(B * n, S, 3), z_vals.reshape(B * n, S),
                                              Z_PER_RAY, self.white_bkgd, 0)
        return rgb.view(B, n, 3), depth.view(B, n), acc.view(B, n)

    # ---- sample preparation
    def _rays_in_box_frame(self, rays_o, viewdir, obj_sz, jitter=None, detach_bounds=False):
        obj_sz = np.asarray(obj_sz)
        diag = np.linalg.norm(obj_sz).astype(np.float32)
        o_n = rays_o / (diag / 2)
        if detach_bounds:
            with torch.no_grad():
                near, far, hit = _box_bounds(o_n.detach(), viewdir.detach(), obj_sz, diag)
        else:
            near, far, hit = _box_bounds(o_n, viewdir, obj_sz, diag)
        return o_n, _unit_depths(near, far, self.n_samples, jitter), hit, diag

    def prepare_sampled_rays(self, rays_o, viewdir, obj_sz):
        """src/renderer.py:91-115: xyz (N,S,3), viewdir (N,S,3), metric z_vals (N,S), hit (N,)."""
        if rays_o.is_cuda and not (rays_o.requires_grad or viewdir.requires_grad) and _pow2(self.n_samples) and rays_o.shape[0] > 0:
            # one launch: slab test, bounds, depths, points, metric z and the hit map
            dev = rays_o.device
            _, half, zs = _box_constants(obj_sz, 1, dev)
            cfg = ops.RenderCfg(self.n_samples, Z_BOX, rays_o.shape[0], 0, 0, metric_z=True, box_half=half)
            jitter = U._jitter_override()
            if jitter is None and not KERNEL_JITTER:
                jitter = torch.rand(rays_o.shape[0], self.n_samples, device=dev)
            return ops.encode(rays_o, viewdir, None if jitter is None else jitter.to(dev), None, zs, cfg, want_hit=True)
        o_n, t, hit, diag = self._rays_in_box_frame(rays_o, viewdir, obj_sz)
        if not rays_o.is_cuda or rays_o.requires_grad or viewdir.requires_grad or t.requires_grad:
            xyz = o_n[:, None, :] + t[:, :, None] * viewdir[:, None, :]
            z_vals = torch.norm((xyz - o_n[:, None, :]) * (diag / 2), p=2, dim=-1)
            return xyz, viewdir.unsqueeze(-2).repeat(1, self.n_samples, 1), z_vals, hit
        cfg = ops.RenderCfg(self.n_samples, Z_PER_RAY, max(rays_o.shape[0], 1), 0, 0, metric_z=True)
        dev = rays_o.device
        xyz, vd, z_vals = ops.encode(o_n, viewdir, t, torch.ones(1, device=dev), torch.full((1,), float(diag / 2), device=dev), cfg)
        return xyz, vd, z_vals, hit

    # ---- render
    def _render(self, model, device, rays_o, viewdir, obj_sz, shapecode, texturecode, kitti2nusc, white_bkgd, jitter=None,
                detach_bounds=False, adjust_scale=1.0, frame=None):
        dev = torch.device(device)
        rays_o, viewdir = rays_o.to(dev), viewdir.to(dev)
        S = self.n_samples
        B = shapecode.shape[0]
        if frame is None:
            frame = U._frame(False, kitti2nusc, False)
        if U._is_native(model) and ops.fused_supported(S) and _pow2(S) and rays_o.is_cuda and rays_o.shape[0] > 0:
            # ONE launch from (rays_o, viewdir, obj_sz): box bounds and depths are made in the kernel's prologue (SNR_Z_BOX)
            _, half, zs = _box_constants(obj_sz, B, dev)
            cfg = ops.RenderCfg(S, Z_BOX, max(rays_o.shape[0] // B, 1), getattr(model, "shape_blocks", 0), getattr(model, "texture_blocks", 0),
                                frame=frame, xyz_mul=adjust_scale, white_bkgd=white_bkgd, metric_z=True, precision=None, box_half=half,
                                box_detach=detach_bounds)
            if jitter is None:
                jitter = U._jitter_override()
            if jitter is None and not KERNEL_JITTER:
                jitter = torch.rand(rays_o.shape[0], S, device=dev)      # (the reference's rand_like draw, src/renderer.py:40)
            return model.fused_render(rays_o, viewdir, None if jitter is None else jitter.to(dev), None, zs, shapecode, texturecode, cfg)
        o_n, t, hit, diag = self._rays_in_box_frame(rays_o, viewdir, obj_sz, jitter, detach_bounds)
        cfg = ops.RenderCfg(S, Z_PER_RAY, max(rays_o.shape[0] // B, 1), getattr(model, "shape_blocks", 0),
                            getattr(model, "texture_blocks", 0), frame=frame, xyz_mul=adjust_scale, white_bkgd=white_bkgd, metric_z=True,
                            precision=None)
        one = torch.ones(B, device=dev)
        zs = torch.full((B,), float(diag / 2), device=dev)
        if rays_o.shape[0] == 0:
            e = torch.empty(0, device=dev)
            return e.view(0, 3), e, e
        if U._is_native(model) and ops.fused_supported(S):
            return model.fused_render(o_n, viewdir, t, one, zs, shapecode, texturecode, cfg)      # (CPU-resident rays are refused there: no fallback)
        m = torch.tensor(frame, device=dev).view(3, 3)
        p = o_n[:, None, :] + t[:, :, None] * viewdir[:, None, :]
        z_vals = torch.norm((p - o_n[:, None, :]) * (diag / 2), p=2, dim=-1)
        xyz = (p * adjust_scale) @ m.T
        vd = (viewdir @ m.T)[:, None, :].repeat(1, S, 1)
        sigmas, rgbs = model(xyz, vd, shapecode, texturecode)
        return U._composite(sigmas, rgbs, z_vals, Z_PER_RAY, white_bkgd)

    def render_rays(self, model, device, img, mask_occ, cam_pose, obj_sz, K, roi, shapecode, texturecode, kitti2nusc=False, im_sz=64,
                    n_rays=None):
        """src/renderer.py:117-167."""
        rays_o, viewdir = U.get_rays(K, cam_pose, roi, uv_steps=[im_sz, im_sz])
        rgb_tgt, occ_pixels = U._resize_to(img, mask_occ, im_sz, device)      # (cached per crop like family A's: the loops pass the same crop every iteration)
        if n_rays is not None:
            n_rays = int(np.minimum(rays_o.shape[0], n_rays))
            ids = np.random.permutation(rays_o.shape[0])[:n_rays]
            rays_o, viewdir, rgb_tgt, occ_pixels = rays_o[ids], viewdir[ids], rgb_tgt[ids], occ_pixels[ids]
        rgb, depth, acc = self._render(model, device, rays_o, viewdir, obj_sz, shapecode, texturecode, kitti2nusc, self.white_bkgd)
        return rgb, depth, acc, rgb_tgt, occ_pixels

    def render_rays_specified(self, model, device, img, mask_occ, cam_pose, obj_sz, K, roi, x_vec, y_vec, shapecode, texturecode,
                              kitti2nusc=False):
        """src/renderer.py:169-201."""
        rays_o, viewdir = U.get_rays_specified(K, cam_pose, x_vec + int(roi[0]), y_vec + int(roi[1]))
        rgb_tgt = img[y_vec, x_vec, :].to(device)
        occ_pixels = mask_occ[y_vec, x_vec, :].to(device)
        rgb, depth, acc = self._render(model, device, rays_o, viewdir, obj_sz, shapecode, texturecode, kitti2nusc, self.white_bkgd)
        return rgb, depth, acc, rgb_tgt, occ_pixels

    def prepare_pixel_samples(self, img, mask_occ, cam_pose, obj_sz, K, roi, n_rays, im_sz=None):
        """src/renderer.py:203-236."""
        if im_sz is None:
            rays_o, viewdir = U.get_rays(K, cam_pose, roi)
        else:
            rays_o, viewdir = U.get_rays(K, cam_pose, roi, uv_steps=[im_sz, im_sz])
            img, mask_occ = U._resize(img, mask_occ, im_sz)
        n_rays = int(np.minimum(rays_o.shape[0], n_rays))
        ids = np.random.permutation(rays_o.shape[0])[:n_rays]
        rays_o, viewdir = rays_o[ids], viewdir[ids]
        rgb_tgt = img.reshape(-1, 3)[ids]
        occ_pixels = mask_occ.reshape(-1, 1)[ids]
        xyz, vd, z_vals, _ = self.prepare_sampled_rays(rays_o, viewdir, obj_sz)
        return xyz, vd, z_vals, rgb_tgt, occ_pixels

    def render_full_img(self, model, device, cam_pose, obj_sz, K, roi, shapecode, texturecode, out_depth=False, debug_occ=False,
                        kitti2nusc=False):
        """src/renderer.py:238-294 (one launch instead of slabs of max(roi_w, roi_h) rays)."""
        if debug_occ:
            raise SnrError("debug_occ opens a cv2 window in the reference; not available in this package")
        rays_o, viewdir = U.get_rays(K, cam_pose, roi)
        with torch.no_grad():
            rgb, depth, acc = self._render(model, device, rays_o, viewdir, obj_sz, shapecode, texturecode, kitti2nusc, self.white_bkgd)
        h, w = int(roi[3] - roi[1]), int(roi[2] - roi[0])
        if out_depth:
            return rgb.reshape(h, w, 3), depth.reshape(h, w)
        return rgb.reshape(h, w, 3)

    def render_virtual_imgs(self, model, device, obj_sz, K, shapecode, texturecode, radius=40., tilt=np.pi / 6, pan_num=8, img_sz=128,
                            kitti2nusc=False):
        """src/renderer.py:296-352 (axis arrows drawn with cv2 in the reference are omitted)."""
        cx, cy = float(K[0, 2]), float(K[1, 2])
        roi = np.asarray([cx - img_sz / 2, cy - img_sz / 2, cx + img_sz / 2, cy + img_sz / 2]).astype(np.int64)
        cam_init = np.asarray([[0, 0, 1, -radius], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]]).astype(np.float32)
        ct, st = np.cos(tilt), np.sin(tilt)
        cam_tilt = np.asarray([[ct, 0, st, 0], [0, 1, 0, 0], [-st, 0, ct, 0], [0, 0, 0, 1]]).astype(np.float32) @ cam_init
        views = []
        for pan in np.linspace(0, 2 * np.pi, pan_num, endpoint=False):
            cp, sp = np.cos(pan), np.sin(pan)
            pose = np.asarray([[cp, -sp, 0, 0], [sp, cp, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).astype(np.float32) @ cam_tilt
            views.append(self.render_full_img(model, device, torch.from_numpy(pose[:3, :]), obj_sz, K, roi, shapecode, texturecode,
                                              kitti2nusc=kitti2nusc).cpu())
        return views


def render_rays_v3(model, device, img, mask_occ, cam_pose, obj_wlh, K, roi, n_samples, shapecode, texturecode, shapenet_obj_cood,
                   sym_aug, kitti2nusc=False, im_sz=64, n_rays=None, adjust_scale=1.0):
    """src/renderer.py:382-473: box bounds detached (numpy in the reference), ``adjust_scale``, frame edits, black
    background.  The reference samples with a default ``NeRFRenderer()`` (64 depths) whatever ``n_samples`` says and
    fails in the decoder unless n_samples == 64; the same restriction is enforced here."""
    if n_samples != 64:
        raise SnrError("render_rays_v3 only works with n_samples == 64 (reference behaviour, src/renderer.py:393,434-437)")
    renderer = NeRFRenderer()
    rays_o, viewdir = U.get_rays(K, cam_pose, roi, uv_steps=[im_sz, im_sz])
    rgb_tgt, occ_pixels = U._resize_to(img, mask_occ, im_sz, device)
    if n_rays is not None:
        n_rays = int(np.minimum(rays_o.shape[0], n_rays))
        ids = np.random.permutation(rays_o.shape[0])[:n_rays]
        rays_o, viewdir, rgb_tgt, occ_pixels = rays_o[ids], viewdir[ids], rgb_tgt[ids], occ_pixels[ids]
    frame = U._frame(U._sym_coin(sym_aug), kitti2nusc, shapenet_obj_cood)
    rgb, depth, acc = renderer._render(model, device, rays_o, viewdir, obj_wlh, shapecode, texturecode, kitti2nusc, False,
                                       detach_bounds=True, adjust_scale=adjust_scale, frame=frame)
    return rgb, depth, acc, rgb_tgt, occ_pixels
