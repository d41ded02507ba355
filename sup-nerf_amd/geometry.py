"""``supnerf_amd.geometry`` -- the surface a shape code stands for.

After an optimisation or a training run a caller holds one 256-float shape code per object; this module turns codes into geometry:

  * ``query_density(model, xyz, shapecode)``: sigma at arbitrary decoder-frame points, B codes, object-major (``snr_density_fwd``);
  * ``density_grid(model, shapecode, resolution, bound)``: sigma on a lattice generated in the kernel, (B, nx, ny, nz)
    (``snr_density_grid``);
  * ``narrow_band_grid(model, shapecode, resolution, level=...)``: the same grid with the decoder run only in the bricks of 8^3 points
    that the surface crosses (a coarse pass, ``snr_band_*``, ``snr_density_bricks``); exact wherever the mesh reads it;
  * ``extract_mesh(model_or_grid, shapecode, level=...)``: the iso-surface sigma = level by marching tetrahedra on the GPU
    (``snr_iso_count`` -> two ``torch.cumsum`` -> ``snr_iso_emit``), one (verts (V,3) fp32, faces (F,3) int32) pair per object
    (``narrow_band=True``: on the narrow-band grid; ``differentiable=True``: vertices with autograd to the grid or the shape codes);
  * ``density(model, xyz, shapecode)``: sigma (P,) like ``query_density``, differentiable wrt ``xyz`` and ``shapecode``
    (``ops.DensityPoints``: ``snr_density_fwd_masks`` forward, ``snr_density_bwd`` backward), for losses that read the density only;
  * ``density_gradient(model, xyz, shapecode)``: sigma and d sigma / d xyz in two launches, no autograd;
  * ``vertex_normals(model, meshes, shapecode)``: unit outward normals -grad sigma / |grad sigma| at the vertices of ``extract_mesh``;
  * ``vertex_colors(model, meshes, normals, shapecode, texturecode)``: the decoder's raw rgb at every vertex, seen head-on;
  * ``ray_surface(model, rays_o, rays_d, near, far, shapecode, level=...)``: along each ray the first point where sigma rises through
    ``level``: depth, state (miss / hit / starts inside), outward normal and the bracket width that bounds the depth's error, with autograd
    from the depth to the ray origins, directions and shape codes (``ops.RaySurface``: ``snr_ray_*`` around the density launches);
  * ``surface_depth(model, cam_pose, obj_diag, K, roi, shapecode, level=...)``: the same for a camera's pixel grid or listed pixels (lidar
    returns), in metric units;
  * ``mesh_components(meshes)``: the connected pieces of each mesh -- a component label per vertex and face and, per component, vertex and
    face counts, bounding box, area and signed volume (``ops.mesh_components``: a lock-free union-find over the faces, ``snr_mesh_*``);
    ``select_components(mesh, components, keep)``: the sub-mesh of some components, with the index maps back to the full mesh;
    ``largest_component(meshes, by=..., drop_cavities=...)``: the object without its floaters (and, by default, without the closed pockets
    inside it); ``extract_mesh(..., keep="largest")`` does it in one call;
  * ``simplify_mesh(meshes, cell)``: each mesh with a fraction of its faces, by quadric vertex clustering -- one new vertex per occupied cell
    of a grid, placed so that edges and corners stay, per-vertex attributes averaged (``ops.mesh_simplify``: ``snr_simplify_*``);
  * ``mesh_adjacency(meshes)``: which vertices are neighbours -- a CSR with the number of faces on every edge, vertex degrees, the rim
    (boundary) and non-manifold vertices and edge counts, whether the mesh is closed (``ops.mesh_adjacency``: ``snr_smooth_edge_keys``,
    one sort); ``smooth_mesh(meshes, iterations)``: Taubin lambda|mu smoothing of vertices and per-vertex attributes over it, the rim
    pinned by default (``ops.mesh_smooth``: one ``snr_smooth_step`` launch per half-step); ``mesh_laplacian(meshes)`` and
    ``laplacian_energy(meshes)``: the umbrella vectors and their mean square per object, with autograd to the vertices (``ops.MeshLaplacian``)
    and so, through ``extract_mesh(..., differentiable=True)``, to the grid or the shape codes -- a smoothness regulariser;
  * ``rasterize(meshes, obj_to_cam, K, size)``: the meshes as a pinhole camera sees them -- per pixel the nearest face, the object it belongs
    to, its depth and barycentric weights, all objects in one scene image or one image each (``ops.rasterize``: ``snr_raster_*``);
    ``interpolate(raster, attributes)``: per-vertex normals, colours or any data of up to 16 channels at the pixels;
    ``mesh_view(mesh, cam_pose, obj_diag, K, roi)``: one object on the pixel grid of ``utils.get_rays``, metric depth comparable with
    ``surface_depth``; ``scene_view(meshes, obj_poses, obj_diags, K, H, W)``: a whole scene with depth and instance ids;
  * ``paint_mesh(mesh, views, normals=...)``: vertex colours from the photographs of an instance's views -- bilinear samples through the
    rasteriser's depth buffer and the occupancy mask, weighed by how squarely each view faces the vertex, the unseen rest filled from its
    neighbours (``ops.paint_view`` / ``paint_finish`` / ``paint_fill``: ``snr_paint_*``; rules restated in tests/paint_restatement.py);
  * ``closest_point(meshes, points)``: for every query point the closest point of its object's surface -- face, barycentric weights and
    distance, exact (the brute-force answer, pruned by a uniform grid; ``ops.mesh_nearest_query``: ``snr_nearest_*``), with autograd to
    the points and the vertices; ``mesh_index(meshes, cell)``: that grid, built once; ``sample_surface(meshes, n)``: stratified
    area-uniform surface samples (``snr_surface_sample``); ``mesh_distance(a, b)``: mean, RMS and maximum distance in both directions
    on such samples, Chamfer, Hausdorff and, with a threshold, precision, recall and F-score (rules restated in
    tests/nearest_restatement.py);
  * ``winding_number(meshes, points)``: on which side of its object's surface a point lies -- the integer winding number along +z, exact
    (the brute-force sum over all faces, pruned by the grid of ``mesh_index``; ``ops.mesh_inside_query``: ``snr_inside_query``);
    ``contains(meshes, points, rule=...)``: that as a bool; ``signed_distance(meshes, points)``: ``closest_point``'s distance with that
    sign, one index for both searches; ``voxelize(meshes, resolution, bound)``: the occupancy of a mesh on the lattice ``density_grid``
    uses (``snr_inside_lattice``); ``occupancy_iou(a, b)`` and ``mesh_iou(a, b, resolution)``: the volumetric intersection over union
    of two occupancy grids or two meshes, with exact counts (rules restated in tests/inside_restatement.py);
  * ``ray_mesh(meshes, rays_o, rays_d)``: where each ray hits its object's mesh first -- depth, face, barycentric weights, side, point
    and normal (``MeshHits``), exact (the brute-force answer over all faces, pruned by the grid of ``mesh_index``;
    ``ops.mesh_raycast_first``: ``snr_raycast_first``), with autograd to the rays and the vertices; ``ray_crossings(meshes, rays_o,
    rays_d)``: the signed and the total number of faces a ray crosses (``snr_raycast_crossings``); ``visible(meshes, points, eye)``:
    whether the segment from a point to an eye crosses no face; ``mesh_depth(mesh, cam_pose, obj_diag, K, roi)``: the mesh twin of
    ``surface_depth``, metric depth on a camera grid or at listed pixels with autograd to the pose and the vertices (rules restated in
    tests/raycast_restatement.py);
  * ``to_object_frame(verts, obj_diag, family)``: decoder coordinates back to the object's metric frame (``direction=True``: normals);
    ``to_decoder_frame``: its inverse;
  * ``write_ply(path, verts, faces, normals=None, colors=None)``: binary little-endian PLY (host code).

The density kernels run the exact fp32 chain of the decoder forward up to its density head and stop there (no view direction, no colour
branch): sigma is bit-identical to ``ops.decoder_fwd(..., precision="fp32")``.  Latent terms come from ``model.latent_terms`` with a zero
texture code (the texture rows feed nothing the density reads).  The mesh rules (vertex order, quad split, winding) are those of
include/supnerf_hip.h, restated in tests/iso_restatement.py.  The density backward runs the fp32 backward kernel from d sigma alone (no colour
branch): d xyz and the shape-code gradient are bit for bit those of the full backward with a zero colour gradient.  The ray rules (march,
first crossing, refinement, depth, implicit gradient) are the header's too, restated in tests/ray_restatement.py; a ray search reads nothing
back to the host.  The component rules (connectivity by vertex index, ids in the order of the smallest vertex index, float64 measures
summed in a fixed order) are the header's as well, restated in tests/mesh_restatement.py; so are the rasteriser's (projection, snapping
to 1/256 pixel, exact integer coverage with a tie rule, perspective-correct depth, the nearest face by an integer atomic min), restated in
tests/raster_restatement.py: no host read, no autograd, the same bits from run to run.  The smoothing rules (neighbours by index, each
once and in ascending order, float64 sums in that order, Jacobi steps between two buffers) are the header's too, restated in
tests/smooth_restatement.py, which the kernels match bit for bit.  There is no CPU path: CPU tensors raise ``SnrError``."""
from typing import NamedTuple

import numpy as np
import torch

from . import model as M
from . import ops
from . import utils as U
from ._lib import Lattice, SnrError

MAX_RESOLUTION = 512
BRICK = 8                # narrow band: bricks of 8^3 lattice points (512, a whole number of the density kernel's workgroups)


def _decoder(model):
    if not isinstance(model, M._DecoderBase):
        raise SnrError(f"supnerf_amd.geometry needs a supnerf_amd decoder (CodeNeRF / SUPNeRF, or a reference class under install()), "
                       f"got {type(model).__name__}")
    return model


def _gpu(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise SnrError(f"supnerf_amd.geometry: {what} must be a tensor on the GPU (no CPU fallback)")
    return t


def _codes(shapecode, keep_graph=False):
    sc = _gpu(shapecode, "shapecode")
    if sc.dim() == 1:
        sc = sc.unsqueeze(0)
    if sc.dim() != 2 or sc.shape[1] != 256:
        raise SnrError(f"shapecode must be (256,) or (B, 256), got {tuple(shapecode.shape)}")
    return sc.float() if keep_graph else sc.detach().float().contiguous()


def _latent(model, sc):
    """(B, NLAT, 256) latent terms of the shape codes (texture code zero: the density never reads the texture terms)."""
    with torch.no_grad():
        return model.latent_terms(sc, torch.zeros_like(sc)).detach().float().contiguous()


def _decoder_inputs(model, shapecode, differentiable=None):
    """What every density launch takes from (model, shapecode): (codes (B, 256), latent terms (B, NLAT, 256), packed weights).  The latent
    terms are ``_latent``'s.  ``differentiable``: the caller's name, for the variant that keeps the autograd graph from ``shapecode`` to the
    latent terms; the decoder's weights are constants on it, so under grad mode it notes the run as such and refuses
    ``train_decoder_weights``."""
    model = _decoder(model)
    if differentiable:
        if torch.is_grad_enabled() and model.train_decoder_weights:
            raise SnrError(f"{differentiable} does not differentiate the decoder weights: with train_decoder_weights set, run it under "
                           "torch.no_grad() or use the model's forward")
        sc = _codes(shapecode, keep_graph=True)
        model._note_decoder_run(constant=True)
        latent = model.latent_terms(sc, torch.zeros_like(sc))
    else:
        sc = _codes(shapecode)
        latent = _latent(model, sc)
    return sc, _gpu(latent, "the model's latent terms"), _gpu(model.packed_weights(), "the model's weights")


def lattice(resolution, bound=(-0.5, 0.5)):
    """The ``Lattice`` (lo, h, n per axis) of ``resolution`` (int or triple) points over ``bound``: a scalar pair (lo, hi) or a per-axis
    pair (lo[3], hi[3]).  h = (hi - lo) / (n - 1) in fp32 (0 where n = 1); the kernels place point i at lo + h i (fp32 multiply, add)."""
    n = np.broadcast_to(np.asarray(resolution, dtype=np.int64), (3,))
    if (n < 1).any() or (n > MAX_RESOLUTION).any():
        raise SnrError(f"resolution must be 1..{MAX_RESOLUTION} points per axis, got {tuple(int(x) for x in n)}")
    lo, hi = bound
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (3,)).astype(np.float32)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (3,)).astype(np.float32)
    h = np.where(n > 1, (hi - lo) / np.maximum(n - 1, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    lat = Lattice()
    for a in range(3):
        lat.lo[a], lat.h[a], lat.n[a] = float(lo[a]), float(h[a]), int(n[a])
    return lat


def lattice_points(lat, device=None):
    """(nx*ny*nz, 3) fp32 points of a ``Lattice`` in the kernels' order (x-major, z fastest), computed on the host by the same formula."""
    axes = [torch.tensor(lat.lo[a], dtype=torch.float32) + torch.tensor(lat.h[a], dtype=torch.float32) *
            torch.arange(lat.n[a], dtype=torch.float32) for a in range(3)]
    X, Y, Z = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([X, Y, Z], dim=-1).reshape(-1, 3).to(device)


def query_density(model, xyz, shapecode):
    """sigma (P,) at decoder-frame points ``xyz`` (P, 3), object-major over the B codes of ``shapecode`` (B, 256): P / B points each."""
    _, latent, packed = _decoder_inputs(model, shapecode)
    return ops.density_fwd(_gpu(xyz, "xyz").detach(), latent, packed, model.shape_blocks, model.texture_blocks)[0]


def density(model, xyz, shapecode):
    """sigma (P,) at decoder-frame points ``xyz`` (P, 3), object-major over the B codes of ``shapecode`` (B, 256) -- the values of
    ``query_density`` -- with autograd to ``xyz`` and ``shapecode`` (through ``model.latent_terms(shapecode, 0)``).  The decoder's
    weights are constants here: with grad mode on and ``model.train_decoder_weights`` set this raises rather than leave them without
    a gradient."""
    _, latent, packed = _decoder_inputs(model, shapecode, differentiable="geometry.density")
    return ops.DensityPoints.apply(_gpu(xyz, "xyz"), latent, packed, model.shape_blocks, model.texture_blocks)


def density_gradient(model, xyz, shapecode):
    """(sigma (P,), d sigma / d xyz (P, 3)) at decoder-frame points ``xyz``, object-major over ``shapecode`` (B, 256); no autograd.  Two
    launches: the density forward saving its ReLU bits, then its backward with d sigma = 1."""
    _, latent, packed = _decoder_inputs(model, shapecode)
    xyz = _gpu(xyz, "xyz").detach().float().contiguous()
    sb, tb = model.shape_blocks, model.texture_blocks
    sig, masks = ops.density_fwd(xyz, latent, packed, sb, tb, save_masks=True)
    _, grad = ops.density_bwd(xyz, latent, packed, masks, sig, torch.ones_like(sig), sb, tb, need_latent=False)
    return sig, grad


def _meshes(meshes):
    if isinstance(meshes, tuple) and len(meshes) == 2 and torch.is_tensor(meshes[0]):
        raise SnrError("meshes is the list extract_mesh returns, one (verts, faces) pair per object")
    out = []
    for m in meshes:
        if not isinstance(m, (tuple, list)) or len(m) != 2:
            raise SnrError("meshes is the list extract_mesh returns, one (verts, faces) pair per object")
        v, f = m
        _gpu(v, "verts")
        _gpu(f, "faces")
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise SnrError(f"a mesh is verts (V, 3) and faces (F, 3), got {tuple(v.shape)} and {tuple(f.shape)}")
        out.append((v, f))
    return out


def _per_object(codes, n, what):
    c = _codes(codes)
    if c.shape[0] != n:
        raise SnrError(f"{n} meshes but {c.shape[0]} {what}s")
    return c


def face_normal_sums(verts, faces):
    """(V, 3): per vertex the sum of the cross products (v1 - v0) x (v2 - v0) of its faces, i.e. the area-weighted mean face normal up to
    a positive factor; outward for the winding of ``extract_mesh``."""
    v = verts.detach().float()
    f = faces.long()
    out = torch.zeros_like(v)
    if f.shape[0]:
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        fn = torch.cross(b - a, c - a, dim=1)
        for k in range(3):
            out.index_add_(0, f[:, k], fn)
    return out


def vertex_normals(model, meshes, shapecode):
    """One (V, 3) tensor of unit normals per mesh of ``meshes`` (the list ``extract_mesh`` returns for ``shapecode`` (B, 256)):
    n = -grad sigma / |grad sigma|, the outward normal of the decoder's surface, from ``density_gradient`` (one launch pair per object).
    Where |grad sigma| is zero or not finite, the area-weighted mean of the adjacent face normals stands in."""
    model = _decoder(model)
    meshes = _meshes(meshes)
    sc = _per_object(shapecode, len(meshes), "shape code")
    out = []
    for b, (v, f) in enumerate(meshes):
        if v.shape[0] == 0:
            out.append(torch.empty(0, 3, device=v.device))
            continue
        _, g = density_gradient(model, v, sc[b:b + 1])
        norm = g.norm(dim=1, keepdim=True)
        good = torch.isfinite(norm) & (norm > 0)
        n = torch.where(good, -g / torch.where(good, norm, torch.ones_like(norm)), torch.zeros_like(g))
        if not bool(good.all()):
            fn = face_normal_sums(v, f)
            fn = fn / fn.norm(dim=1, keepdim=True).clamp_min(1e-30)
            n = torch.where(good, n, fn)
        out.append(n)
    return out


def vertex_colors(model, meshes, normals, shapecode, texturecode):
    """One (V, 3) tensor per mesh: the decoder's raw rgb (no sigmoid, as the decoder returns it) at each vertex, seen head-on (view direction
    -normal), through the exact fp32 decoder forward with ``model.latent_terms(shapecode, texturecode)`` of that object."""
    model = _decoder(model)
    meshes = _meshes(meshes)
    if len(normals) != len(meshes):
        raise SnrError(f"{len(meshes)} meshes but {len(normals)} normal tensors")
    sc = _per_object(shapecode, len(meshes), "shape code")
    tc = _per_object(texturecode, len(meshes), "texture code")
    with torch.no_grad():
        lat = model.latent_terms(sc, tc).detach().float().contiguous()
    packed = model.packed_weights()
    out = []
    for b, ((v, _), n) in enumerate(zip(meshes, normals)):
        n = _gpu(n, "normals")
        if tuple(n.shape) != tuple(v.shape):
            raise SnrError(f"normals of mesh {b} must be {tuple(v.shape)}, got {tuple(n.shape)}")
        if v.shape[0] == 0:
            out.append(torch.empty(0, 3, device=v.device))
            continue
        _, rgb, _ = ops.decoder_fwd(v.detach(), -n.detach(), lat[b:b + 1], packed, model.shape_blocks, model.texture_blocks, precision="fp32")
        out.append(rgb)
    return out


def density_grid(model, shapecode, resolution, bound=(-0.5, 0.5)):
    """sigma (B, nx, ny, nz) of each code on the lattice ``lattice(resolution, bound)``, generated in the kernel (no point array)."""
    _, latent, packed = _decoder_inputs(model, shapecode)
    return ops.density_grid(lattice(resolution, bound), latent, packed, model.shape_blocks, model.texture_blocks)


def coarse_lattice(lat):
    """The coarse ``Lattice`` of a fine one for the narrow band: its points at multiples of ``BRICK``, one more per axis past the far
    edge (ceil(n / 8) + 1 points, same lo, spacing 8 h).  8 h is exact in fp32, and (8 h) I and h (8 I) are the same real product rounded
    once, so ``lo + (8h) I`` and ``lo + h (8I)`` are the same fp32 number: a plain ``snr_density_grid`` on this lattice gives bit for bit
    the fine grid's value at every coarse point inside the grid, and no kernel of its own is needed."""
    c = Lattice()
    for a in range(3):
        c.lo[a] = lat.lo[a]
        c.h[a] = float(np.float32(BRICK) * np.float32(lat.h[a]))
        c.n[a] = (lat.n[a] + BRICK - 1) // BRICK + 1
    return c


class NarrowBand(NamedTuple):
    grid: torch.Tensor       # (B, nx, ny, nz): decoder values in the active bricks, fill values elsewhere
    active: torch.Tensor     # (B, bx, by, bz) bool: the bricks the decoder ran on
    rounds: int              # growth rounds that added bricks
    points: int              # decoder points evaluated: the coarse lattice's plus 512 per active brick


def narrow_band_grid(model, shapecode, resolution, *, level, band=0.0, bound=(-0.5, 0.5), initial_bricks=None):
    """sigma (B, nx, ny, nz) of each code on ``lattice(resolution, bound)`` like ``density_grid``, with the decoder run only near the
    surface {sigma = level}.  Returns a ``NarrowBand`` (grid, active, rounds, points).

    The grid is cut into bricks of 8^3 points (brick (I, J, K) owns the points [8I, 8I+8) x ... inside the grid).  A coarse pass evaluates
    the brick corners (``coarse_lattice``); a brick is active when its corners are not all on one side of the level (inside: sigma > level),
    when a corner lies within ``band`` of the level, or when a corner is not finite.  Active bricks are evaluated exactly (the brick mode of
    the density kernel: bit-identical to ``density_grid``); every other brick is filled with its corner value farthest from the level, a
    density the decoder produced, on the same side.  Two such bricks holding adjacent points share a corner, so no grid edge between two
    filled points crosses the level.  Then growth: each grid edge of the iso rules (7 Kuhn directions) that crosses the level with an
    endpoint in an unevaluated brick activates that brick, which is evaluated, until no such edge is left (one host read per round).

    At the fixpoint both ends of every crossing edge hold exact decoder values, so ``extract_mesh`` of the grid equals the dense mesh bit
    for bit (vertices, faces, order) whenever the coarse pass finds every component of the surface.  It can miss a component that lies
    wholly inside bricks whose corners are all on one side -- a feature thinner than a brick between coarse points, e.g. a sphere smaller
    than 8 grid steps between lattice points at multiples of 8.  ``band`` > 0 activates bricks whose corners come near the level, for
    such features.

    ``initial_bricks``: a (B, bx, by, bz) mask that replaces the coarse classification (a previous ``active``, or a seed for tests).
    Unlisted bricks are filled by the corner rule; one whose corners straddle the level takes its smallest corner (outside until growth
    reaches it), one with a non-finite corner NaN (``extract_mesh`` then raises rather than mesh a guess)."""
    model = _decoder(model)
    sc = _codes(shapecode)
    lat = lattice(resolution, bound)
    if min(lat.n) < 2:
        raise SnrError(f"narrow_band_grid needs at least 2 points per axis, got {tuple(lat.n)}")
    band = float(np.float32(band))
    if not band >= 0.0:
        raise SnrError(f"band must be >= 0, got {band}")
    level = float(np.float32(level))
    dev, B = sc.device, sc.shape[0]
    clat = coarse_lattice(lat)
    nb = tuple(clat.n[a] - 1 for a in range(3))
    ib = None
    if initial_bricks is not None:
        ib = torch.as_tensor(initial_bricks)
        if tuple(ib.shape) != (B,) + nb:
            raise SnrError(f"initial_bricks must be a {(B,) + nb} mask, got {tuple(ib.shape)}")
        ib = ib.to(dev) != 0
    if B == 0:
        return NarrowBand(torch.empty(0, *lat.n, device=dev), torch.zeros(0, *nb, dtype=torch.bool, device=dev), 0, 0)
    _, latent, packed = _decoder_inputs(model, sc)
    sb, tb = model.shape_blocks, model.texture_blocks
    with torch.cuda.device(dev):
        coarse = ops.density_grid(clat, latent, packed, sb, tb)

    def evaluate(bricks, n, grid):
        ops.density_bricks(lat, bricks, n, latent, packed, sb, tb, grid)

    grid, state, _, rounds, evaluated = _band_rounds(lat, B, coarse, evaluate, level, band, ib)
    points = B * clat.n[0] * clat.n[1] * clat.n[2] + BRICK ** 3 * evaluated
    return NarrowBand(grid, state != 0, rounds, points)


def _band_rounds(lat, B, coarse, evaluate, level, band, initial_bricks):
    """The narrow band's loop on the coarse grids ``coarse`` (B, nb0+1, nb1+1, nb2+1) of any field, B >= 1: classify, compact, fill, the
    first evaluation and the seam rounds.  ``evaluate(bricks, n, grid)`` writes the field's values at the points of the first ``n`` bricks
    (object, I, J, K) of the int32 list ``bricks`` into ``grid``, as ``ops.density_bricks`` does; nothing else fills a brick.
    ``initial_bricks``: None or a (B, nb0, nb1, nb2) bool mask on the device that replaces the classification.  Returns (grid, state,
    fill, rounds, evaluated bricks): ``state`` (B, nb0, nb1, nb2) int32 with its stamps (0: filled, 1: the first evaluation, s: growth
    round s - 1), ``fill`` the fill value of every brick."""
    dev = coarse.device
    nb = tuple((lat.n[a] + BRICK - 1) // BRICK for a in range(3))
    grid = torch.empty(B, lat.n[0], lat.n[1], lat.n[2], device=dev)
    state = torch.zeros(B, *nb, dtype=torch.int32, device=dev)
    fill = torch.empty(B, *nb, device=dev)
    bricks = torch.empty(B * nb[0] * nb[1] * nb[2], 4, dtype=torch.int32, device=dev)
    n_new = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ops.band_classify(coarse, lat, level, band, state, fill)
        if initial_bricks is not None:
            state.copy_(initial_bricks.to(torch.int32))
        scan = torch.cumsum((state == 1).view(-1), 0, dtype=torch.int32)
        ops.band_compact(state, scan, lat, bricks)
        ops.band_fill(grid, lat, state, fill)
        evaluated = int(scan[-1])                      # host read: the size of the first brick list
        if evaluated:
            evaluate(bricks, evaluated, grid)
        rounds, stamp = 0, 2
        while True:
            ops.band_seam(grid, lat, level, stamp, state, bricks, n_new)
            k = int(n_new.item())                      # host read: the bricks this round added
            if k == 0:
                break
            evaluate(bricks, k, grid)
            evaluated += k
            rounds += 1
            stamp += 1
    return grid, state, fill, rounds, evaluated


def extract_mesh(model_or_grid, shapecode=None, *, level, resolution=128, bound=(-0.5, 0.5), narrow_band=False, band=0.0,
                 differentiable=False, keep=None):
    """Iso-surface {sigma = level} per object: a list of (verts (V, 3) fp32, faces (F, 3) int32) on the GPU, faces counter-clockwise
    seen from the low side (outward normals around a dense object), vertices in ``bound``'s decoder coordinates (``to_object_frame``
    maps them to the object's frame).  ``model_or_grid``: a decoder (then ``shapecode`` (B, 256) and ``resolution`` make the grid with
    ``density_grid``) or a grid tensor (B, nx, ny, nz) / (nx, ny, nz) over ``bound`` (the decoder is skipped).  A non-finite grid value
    raises ``SnrError``.  One host synchronisation: the sizes of the output.  ``narrow_band=True`` (decoder only): the grid comes from
    ``narrow_band_grid(..., band=band)`` -- the same mesh wherever its coarse pass finds the surface, for a fraction of the decoder work.

    ``differentiable=True`` (under grad mode): the vertices carry a ``grad_fn`` -- to the grid tensor (``ops.IsoVertices``), or to
    ``shapecode`` through ``model.latent_terms(shapecode, 0)`` (``ops.IsoVerticesLatent``: the backward runs the density decoder at the
    grid points the surface touches only).  The derivative is that of the vertex formula at the forward's topology: topology changes
    carry no gradient, nor does ``level``; an edge whose two values nearly agree gives a large one.  Vertices and faces are the same as
    without it.  On a narrow-band grid the gradient is exact wherever its mesh equals the dense mesh (see ``narrow_band_grid``).  The
    decoder's weights are constants: with ``model.train_decoder_weights`` set and grad mode on this raises, as ``density`` does.

    ``keep="largest"``: each object's mesh is reduced to its largest connected component by area, closed pockets inside it dropped too:
    the (verts, faces) of ``largest_component``; differentiable vertices keep their ``grad_fn``.  ``None`` (the default) returns the
    whole iso-surface."""
    if keep not in (None, "largest"):
        raise SnrError(f"extract_mesh: keep is None or 'largest', got {keep!r}")
    if narrow_band and torch.is_tensor(model_or_grid):
        raise SnrError("extract_mesh(narrow_band=True) builds its grid with the decoder: pass the model and the shape codes")
    grad = bool(differentiable) and torch.is_grad_enabled()
    if torch.is_tensor(model_or_grid):
        grid = _gpu(model_or_grid, "the grid")
        if not grad:
            grid = grid.detach()
        if grid.dim() == 3:
            grid = grid.unsqueeze(0)
        if grid.dim() != 4:
            raise SnrError(f"a grid is (B, nx, ny, nz) or (nx, ny, nz), got {tuple(model_or_grid.shape)}")
        grid = grid.float().contiguous()
        lat = lattice(tuple(grid.shape[1:]), bound)
    else:
        if shapecode is None:
            raise SnrError("extract_mesh(model, shapecode, ...): the shape codes are missing")
        model = model_or_grid
        if grad:
            _, latent, packed = _decoder_inputs(model, shapecode, differentiable="extract_mesh(differentiable=True)")
        if narrow_band:
            grid = narrow_band_grid(model, shapecode, resolution, level=level, band=band, bound=bound).grid
        else:
            grid = density_grid(model, shapecode, resolution, bound)
        lat = lattice(resolution, bound)
    if min(lat.n) < 2:
        raise SnrError(f"extract_mesh needs at least 2 points per axis, got {tuple(lat.n)}")
    B = grid.shape[0]
    if B == 0:
        return []
    level = float(np.float32(level))
    if not grad:
        m = ops.iso_extract(grid, lat, level)
        verts, faces, nvs, nts = m.verts, m.faces, m.n_verts, m.n_faces
    else:
        if torch.is_tensor(model_or_grid):
            verts, faces, sizes = ops.IsoVertices.apply(grid, lat, level)
        else:
            verts, faces, sizes = ops.IsoVerticesLatent.apply(latent, packed, grid, lat, level, model.shape_blocks, model.texture_blocks)
        nvs, nts = sizes.tolist()
    out, v0, f0 = [], 0, 0
    for b in range(B):
        out.append((verts[v0:v0 + nvs[b]], faces[f0:f0 + nts[b]]))
        v0 += nvs[b]
        f0 += nts[b]
    if keep == "largest":
        return [(v, f) for v, f, _, _ in largest_component(out)]
    return out


class Components(NamedTuple):
    vert_label: torch.Tensor     # (V,) int32: the component of each vertex
    face_label: torch.Tensor     # (F,) int32: the component of each face
    n_verts: torch.Tensor        # (C,) int64
    n_faces: torch.Tensor        # (C,) int64
    area: torch.Tensor           # (C,) float64
    volume: torch.Tensor         # (C,) float64, signed: positive for a closed dense piece, negative for a closed cavity
    bbox_lo: torch.Tensor        # (C, 3) fp32
    bbox_hi: torch.Tensor        # (C, 3) fp32


def _one_or_many(meshes):
    """(list of (verts, faces) pairs, whether the caller passed a single pair)."""
    single = isinstance(meshes, (tuple, list)) and len(meshes) == 2 and torch.is_tensor(meshes[0])
    return _meshes([tuple(meshes)] if single else meshes), single


def _packed(ms):
    """(verts, faces, n_verts, n_faces) of a list of (verts, faces) pairs that is not empty: the packed form ``ops`` takes."""
    for _, f in ms:
        if f.dtype != torch.int32:
            raise SnrError(f"faces are int32, got {f.dtype}")
    nvs, nfs = [v.shape[0] for v, _ in ms], [f.shape[0] for _, f in ms]
    if len(ms) == 1:
        return ms[0][0].detach(), ms[0][1], nvs, nfs
    return torch.cat([v.detach().float() for v, _ in ms]), torch.cat([f for _, f in ms]), nvs, nfs


def _object_slices(*sizes):
    """Per object one slice per list of ``sizes``: where the object's items lie in the packed array those sizes add up to."""
    starts = [0] * len(sizes)
    for ns in zip(*sizes):
        yield tuple(slice(s, s + n) for s, n in zip(starts, ns))
        starts = [s + n for s, n in zip(starts, ns)]


def mesh_components(meshes):
    """The connected components of each mesh of ``meshes`` -- the list ``extract_mesh`` returns (vertices with a ``grad_fn`` are fine: the
    analysis reads their values), or one (verts, faces) pair.  Returns one ``Components`` per object (a single one for a single pair).

    Two vertices are connected iff a chain of faces links them through shared vertex indices (equal positions do not connect; a vertex no
    face names is a component of its own with no faces).  Component ids are fully determined by the mesh: component c is the one whose
    smallest vertex index is the c-th smallest.  ``volume`` is the signed sum of (a - p0) . ((b - p0) x (c - p0)) / 6 over the faces, p0 the
    component's first vertex: ``extract_mesh`` winds faces counter-clockwise seen from the low side, so a closed dense blob is positive
    and a closed cavity negative.  For a closed component the value does not depend on p0; a component the border of the grid cuts open
    gets this formula's value and no more -- its ``bbox`` reaching ``bound`` is how to tell.  ``area`` and ``volume`` are float64 sums in a
    fixed order (the same bits from run to run); counts and boxes are exact.

    All objects go through the same launches; one host read (the component counts).  An empty mesh has C = 0.  A face index outside the
    mesh raises ``SnrError``, as do CPU tensors."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    verts, faces, nvs, nfs = _packed(ms)
    m = ops.mesh_components(verts, faces, nvs, nfs)
    out = [Components(m.vert_label[v], m.face_label[f], m.n_verts[c], m.n_faces[c], m.area[c], m.volume[c], m.bbox_lo[c], m.bbox_hi[c])
           for v, f, c in _object_slices(nvs, nfs, m.n_comps)]
    return out[0] if single else out


def _keep_mask(keep, C, dev):
    if torch.is_tensor(keep) and keep.dtype == torch.bool:
        if tuple(keep.shape) != (C,):
            raise SnrError(f"a keep mask of {C} components must be ({C},), got {tuple(keep.shape)}")
        return keep.to(dev)
    ids = [int(i) for i in (keep.tolist() if torch.is_tensor(keep) else keep)]
    if any(i < 0 or i >= C for i in ids):
        raise SnrError(f"component ids must lie in [0, {C}), got {ids}")
    mask = torch.zeros(C, dtype=torch.bool, device=dev)
    if ids:
        mask[torch.tensor(ids, dtype=torch.int64).to(dev)] = True
    return mask


def select_components(mesh, components, keep):
    """The sub-mesh of the components ``keep`` (a bool mask (C,) or a list of ids) of ``mesh`` = (verts, faces) with its ``Components``:
    (verts, faces, vert_index, face_index) -- the kept vertices and faces in their original order, face indices renumbered;
    ``vert_index`` / ``face_index`` (int64) point into the original arrays, so per-vertex data of the full mesh (normals, colours) is
    gathered with them.  ``verts`` is ``mesh[0][vert_index]``, a torch index: the ``grad_fn`` of a differentiable mesh carries through."""
    v, f = _meshes([tuple(mesh)])[0]
    c = components
    if tuple(c.vert_label.shape) != (v.shape[0],) or tuple(c.face_label.shape) != (f.shape[0],):
        raise SnrError(f"these components label {c.vert_label.shape[0]} vertices and {c.face_label.shape[0]} faces, the mesh has "
                       f"{v.shape[0]} and {f.shape[0]}")
    mask = _keep_mask(keep, c.n_verts.shape[0], v.device)
    vkeep, fkeep = mask[c.vert_label.long()], mask[c.face_label.long()]
    vert_index, face_index = torch.nonzero(vkeep).view(-1), torch.nonzero(fkeep).view(-1)
    renumber = torch.cumsum(vkeep, 0, dtype=torch.int32) - 1
    faces = renumber[f[face_index].long()].view(-1, 3)
    return v[vert_index], faces, vert_index, face_index


def largest_keep(components, by="area", drop_cavities=True):
    """The (C,) bool mask ``largest_component`` keeps: the component with the most area (``by="area"``), the largest |volume|
    (``"volume"``) or the most faces (``"faces"``), ties to the lowest id; with ``drop_cavities=False`` also every component of negative
    volume whose bounding box lies inside the winner's."""
    if by not in ("area", "volume", "faces"):
        raise SnrError(f"by is 'area', 'volume' or 'faces', got {by!r}")
    c = components
    score = {"area": c.area, "volume": c.volume.abs(), "faces": c.n_faces}[by]
    mask = torch.zeros(score.shape[0], dtype=torch.bool, device=score.device)
    if score.shape[0] == 0:
        return mask
    w = torch.nonzero(score == score.max()).view(-1)[:1]                      # (the lowest id among equals)
    mask[w] = True
    if not drop_cavities:
        inside = (c.bbox_lo >= c.bbox_lo[w]).all(1) & (c.bbox_hi <= c.bbox_hi[w]).all(1)
        mask |= inside & (c.volume < 0)
    return mask


def largest_component(meshes, by="area", drop_cavities=True):
    """Each object's mesh without its floaters: ``select_components`` of the component ``largest_keep`` picks, per object of ``meshes``
    (the list ``extract_mesh`` returns, or one pair -> one tuple).  ``drop_cavities=True`` keeps that component alone, so closed pockets of
    low density inside the body go too; ``False`` keeps them (negative volume, bounding box inside the winner's)."""
    if by not in ("area", "volume", "faces"):
        raise SnrError(f"by is 'area', 'volume' or 'faces', got {by!r}")
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    comps = mesh_components(ms)
    out = [select_components(m, c, largest_keep(c, by, drop_cavities)) for m, c in zip(ms, comps)]
    return out[0] if single else out


class Simplified(NamedTuple):
    verts: torch.Tensor          # (V', 3) fp32, no grad_fn
    faces: torch.Tensor          # (F', 3) int32
    vert_map: torch.Tensor       # (V,) int32: the new index of every old vertex; -1 where its cluster was dropped
    face_index: torch.Tensor     # (F',) int64: the kept faces, as indices into the old faces
    members: torch.Tensor        # (V',) int32: how many old vertices each new one stands for
    attributes: object           # (V', C) fp32 or None


def _drop_unreferenced(s):
    """``s`` without the vertices no face names, renumbered; ``vert_map`` is -1 for the old vertices whose cluster went."""
    used = torch.zeros(s.verts.shape[0], dtype=torch.bool, device=s.verts.device)
    used[s.faces.view(-1).long()] = True
    renumber = torch.where(used, torch.cumsum(used, 0, dtype=torch.int32) - 1, torch.full_like(used, -1, dtype=torch.int32))
    index = torch.nonzero(used).view(-1)
    return Simplified(s.verts[index], renumber[s.faces.long()].view(-1, 3), renumber[s.vert_map.long()], s.face_index, s.members[index],
                      None if s.attributes is None else s.attributes[index])


def simplify_mesh(meshes, cell, *, origin=None, placement="quadric", attributes=None, drop_unreferenced=True):
    """Each mesh of ``meshes`` -- the list ``extract_mesh`` returns, or one (verts, faces) pair -- with fewer faces, by quadric vertex
    clustering (Lindstrom 2000; include/supnerf_hip.h, "Mesh simplification").  A grid of cubic cells of edge ``cell`` (a float, or one
    per object), anchored at ``origin`` (3,) or (B, 3), zeros by default, is laid over each object; all vertices in one cell become one
    vertex and a face survives iff its corners land in three different cells.  Cells of two grid steps of the extraction lattice leave
    about a twelfth of the faces, four steps a fiftieth.  Returns one ``Simplified`` per object, or a single one for a single pair.

    * Clusters go by position alone.  Connectivity plays no part: two sheets that pass through one cell merge there, so choose ``cell``
      below the thinnest wall worth keeping.  The map is simplicial: a closed surface stays closed (every directed edge a->b keeps as
      many b->a), though faces that come out equal (or as opposite flaps) are all kept and ``mesh_components`` counts them as often.
    * ``placement="quadric"`` puts each new vertex where the planes of the original faces around its cluster meet, least squares with a
      small pull to the members' mean, clamped to the cell: edges and corners stay where they are.  ``"mean"`` takes the mean, which
      shrinks them.
    * ``attributes``: a (V, C) tensor (C <= 16) or a list of them, one per object (normals, colours): each new vertex gets the mean of its
      members' rows.  Normals want renormalising afterwards.
    * ``drop_unreferenced`` removes the new vertices no kept face names; ``vert_map`` is then -1 for the old vertices whose cluster
      went.  A floater that lies inside one cell disappears entirely instead of surviving as a vertex without faces.
    * New vertices are numbered by cell, ascending (qx, qy, qz); kept faces keep their order and winding.  The result is fully determined
      by the mesh and has the same bits from run to run.

    Vertices with a ``grad_fn`` are read by value and the output carries none: simplification is not differentiable.  All objects go
    through the same launches with one host read (``drop_unreferenced`` adds one per object: how many vertices stay).
    CPU tensors, faces that are not int32, a non-positive ``cell``, an unknown ``placement``, a non-finite vertex, a vertex 2^20 cells or
    more from ``origin`` and a face index outside its mesh raise ``SnrError``."""
    if placement not in ops.SIMPLIFY_PLACEMENTS:
        raise SnrError(f"placement is 'mean' or 'quadric', got {placement!r}")
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    B = len(ms)
    verts, faces, nvs, nfs = _packed(ms)
    if attributes is not None:
        attributes = [attributes] if torch.is_tensor(attributes) else list(attributes)
        if len(attributes) != B:
            raise SnrError(f"{B} meshes but {len(attributes)} attribute tensors")
        for a, (v, _) in zip(attributes, ms):
            _gpu(a, "attributes")
            if a.dim() != 2 or a.shape[0] != v.shape[0] or a.shape[1] != attributes[0].shape[1]:
                raise SnrError(f"attributes are (V, C) per object with one C, got {tuple(a.shape)} for {v.shape[0]} vertices")
        attributes = torch.cat([a.detach().float() for a in attributes])
    if origin is None:
        origin = torch.zeros(B, 3)
    s = ops.mesh_simplify(verts, faces, nvs, nfs, cell, origin, placement, attributes)
    out = []
    for v, f, c, k in _object_slices(nvs, nfs, s.n_verts, s.n_faces):
        one = Simplified(s.verts[c], s.faces[k], s.vert_map[v], s.face_index[k] - f.start, s.members[c],
                         None if s.attributes is None else s.attributes[c])
        out.append(_drop_unreferenced(one) if drop_unreferenced else one)
    return out[0] if single else out


class Adjacency(NamedTuple):
    nbr_start: torch.Tensor      # (V + 1,) int64: vertex i's neighbours at nbr[nbr_start[i] : nbr_start[i + 1]]
    nbr: torch.Tensor            # (E2,) int32, ascending within each vertex
    edge_faces: torch.Tensor     # (E2,) int32: how many faces name the undirected edge; the same in both directions
    degree: torch.Tensor         # (V,) int32
    boundary: torch.Tensor       # (V,) bool: the vertex lies on an edge with exactly one face (a rim)
    nonmanifold: torch.Tensor    # (V,) bool: the vertex lies on an edge with more than two faces
    boundary_edges: int          # undirected edges with one face
    nonmanifold_edges: int       # undirected edges with more than two faces
    closed: bool                 # faces > 0 and both counts are 0


class Smoothed(NamedTuple):
    verts: torch.Tensor          # (V, 3) fp32, no grad_fn
    attributes: object           # (V, C) fp32 or None


def _unpack_adjacency(a, nvs, nfs):
    """One ``Adjacency`` per object from the packed ``ops.MeshAdjacency`` of the whole call."""
    out = []
    for b, (v,) in enumerate(_object_slices(nvs)):
        e0, e1 = a.edge_offset[b], a.edge_offset[b + 1]
        be, ne = a.boundary_edges[b], a.nonmanifold_edges[b]
        out.append(Adjacency(a.nbr_start[v.start:v.stop + 1] - e0, a.nbr[e0:e1], a.edge_faces[e0:e1], a.degree[v], a.boundary[v],
                             a.nonmanifold[v], be, ne, nfs[b] > 0 and be == 0 and ne == 0))
    return out


def _pack_adjacency(adjs, nvs, dev):
    """The packed ``ops.MeshAdjacency`` of per-object ``Adjacency`` values (what ``mesh_adjacency`` returned for these meshes): torch
    concatenations, nothing read back."""
    for a, n in zip(adjs, nvs):
        if not isinstance(a, Adjacency) or a.degree.shape[0] != n or a.nbr_start.shape[0] != n + 1:
            raise SnrError(f"adjacency is what mesh_adjacency returns for these meshes: one Adjacency per object, here of {n} vertices")
        _gpu(a.nbr_start, "adjacency")
    if len(adjs) != len(nvs):
        raise SnrError(f"{len(nvs)} meshes but {len(adjs)} adjacencies")
    e_off = ops._host_offsets([a.nbr.shape[0] for a in adjs])
    if len(adjs) == 1:
        nbr_start = adjs[0].nbr_start.contiguous()
    else:
        nbr_start = torch.cat([a.nbr_start[:-1] + e for a, e in zip(adjs, e_off)] + [torch.tensor(e_off[-1:], dtype=torch.int64).to(dev)])
    cat = (lambda name: getattr(adjs[0], name).contiguous()) if len(adjs) == 1 else (lambda name: torch.cat([getattr(a, name) for a in adjs]))
    return ops.MeshAdjacency(nbr_start, cat("nbr"), cat("edge_faces"), cat("degree"), cat("boundary"), cat("nonmanifold"),
                             [a.boundary_edges for a in adjs], [a.nonmanifold_edges for a in adjs], list(nvs),
                             ops._offsets(nvs, dev)[1], e_off)


def _adjacency(ms, adjacency):
    """(the packed vertices with their graph, the packed ``ops.MeshAdjacency``, n_verts) of a list of meshes that is not empty; the
    adjacency is built unless the caller brings it."""
    verts, faces, nvs, nfs = _packed(ms)
    if adjacency is None:
        packed = ops.mesh_adjacency(verts, faces, nvs, nfs)
    else:
        packed = _pack_adjacency([adjacency] if isinstance(adjacency, Adjacency) else list(adjacency), nvs, verts.device)
    live = ms[0][0].float() if len(ms) == 1 else torch.cat([v.float() for v, _ in ms])
    return live, packed, nvs


def mesh_adjacency(meshes):
    """Which vertices of each mesh of ``meshes`` -- the list ``extract_mesh`` returns, or one (verts, faces) pair -- are neighbours
    (include/supnerf_hip.h, "Mesh smoothing", rules 1 to 3; ``ops.mesh_adjacency``).  One ``Adjacency`` per object, or a single one for a
    single pair: a CSR (``nbr_start``, ``nbr`` ascending within each vertex, ``edge_faces`` = the faces on each edge), the ``degree`` of
    every vertex, which vertices lie on the rim (``boundary``: an edge with one face -- where an iso-surface meets the border of its grid)
    or on a non-manifold edge (more than two faces -- where ``simplify_mesh`` merged two sheets), how many such edges there are, and
    ``closed`` = the mesh has faces and neither kind of edge.  Connectivity is by index: coincident vertices are not neighbours unless a
    face joins them.  All objects go through the same launches with one host read.  Integers only: exact, the same from run to run.
    CPU tensors, faces that are not int32 and a face index outside its mesh raise ``SnrError``."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    verts, faces, nvs, nfs = _packed(ms)
    out = _unpack_adjacency(ops.mesh_adjacency(verts, faces, nvs, nfs), nvs, nfs)
    return out[0] if single else out


def _per_object_rows(values, ms, what, dtype=None):
    """``values`` -- one (V, ...) tensor or a list of them, one per object -- checked against the meshes; a list."""
    values = [values] if torch.is_tensor(values) else list(values)
    if len(values) != len(ms):
        raise SnrError(f"{len(ms)} meshes but {len(values)} {what} tensors")
    for a, (v, _) in zip(values, ms):
        _gpu(a, what)
        if a.dim() < 1 or a.shape[0] != v.shape[0] or (dtype is not None and a.dtype != dtype):
            raise SnrError(f"{what} are one tensor of V rows per object{'' if dtype is None else f' ({dtype})'}, got {tuple(a.shape)} "
                           f"{a.dtype} for {v.shape[0]} vertices")
    return values


def smooth_mesh(meshes, iterations=10, *, lam=0.5, mu=-0.53, pin="boundary", attributes=None, adjacency=None):
    """Each mesh of ``meshes`` -- the list ``extract_mesh`` returns, or one (verts, faces) pair -- with its vertices smoothed by
    ``iterations`` Taubin lambda|mu iterations (Taubin 1995; include/supnerf_hip.h, "Mesh smoothing"): every vertex moves by ``lam`` times
    the umbrella vector U = (mean of its neighbours) - itself, then by ``mu`` times the U of the result.  The defaults (pass-band 0.1)
    take out the lattice print of marching tetrahedra and the facets of ``simplify_mesh`` while a closed shape keeps its volume within a
    few percent; ``mu=None`` is plain Laplacian smoothing, which shrinks.  Faces are untouched.  Returns one ``Smoothed(verts,
    attributes)`` per object, or a single one for a single pair.

    * ``pin``: the vertices that do not move (they still pull their neighbours).  ``"boundary"``: those on an edge with one face -- the
      rim where the surface meets the border of its grid, which would otherwise shrink inwards; ``None``: nothing; a bool mask (V,), or a
      list of them, one per object: exactly those.
    * ``attributes``: a (V, C) tensor (C <= 16) or a list of them, one per object: they go through the same steps with the same pins.
    * ``adjacency``: what ``mesh_adjacency`` returned for these meshes, to save building it again (and its host read).
    * A Jacobi iteration: every vertex reads the previous positions.  One launch per half-step for all objects, float64 sums over the
      neighbours in ascending order, no atomics: the same bits from run to run.  ``iterations=0`` returns a copy.

    Vertices with a ``grad_fn`` are read by value and the output carries none (``mesh_laplacian`` / ``laplacian_energy`` are the
    differentiable route).  A ``lam`` or ``mu`` that is not finite, ``iterations < 0``, CPU tensors, faces that are not int32 and a face
    index outside its mesh raise ``SnrError``."""
    factors = [float(lam)] + ([] if mu is None else [float(mu)])
    if not all(np.isfinite(f) for f in factors):
        raise SnrError(f"lam and mu must be finite, got {lam} and {mu}")
    if int(iterations) < 0:
        raise SnrError(f"iterations must not be negative, got {iterations}")
    if not (pin is None or torch.is_tensor(pin) or isinstance(pin, (list, tuple)) or pin == "boundary"):
        raise SnrError(f"pin is None, 'boundary' or a bool mask per object, got {pin!r}")
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    live, adj, nvs = _adjacency(ms, adjacency)
    if pin is None:
        pinned = None
    elif isinstance(pin, str):
        pinned = adj.boundary
    else:
        masks = _per_object_rows(pin, ms, "pin masks", torch.bool)
        pinned = masks[0] if len(masks) == 1 else torch.cat(masks)
    verts = ops.mesh_smooth(live.detach(), adj, iterations, lam, mu, pinned)
    att = None
    if attributes is not None:
        rows = _per_object_rows(attributes, ms, "attributes")
        if any(a.dim() != 2 or a.shape[1] != rows[0].shape[1] for a in rows):
            raise SnrError(f"attributes are (V, C) per object with one C, got {[tuple(a.shape) for a in rows]}")
        att = ops.mesh_smooth(torch.cat([a.detach().float() for a in rows]), adj, iterations, lam, mu, pinned)
    out = [Smoothed(verts[v], None if att is None else att[v]) for (v,) in _object_slices(nvs)]
    return out[0] if single else out


def mesh_laplacian(meshes, adjacency=None):
    """The umbrella vectors U_i = (mean of the neighbours of vertex i) - x_i of each mesh of ``meshes``, (V, 3) per object (one tensor for
    a single pair), zero at a vertex without neighbours (include/supnerf_hip.h, "Mesh smoothing", rules 4 and 7).  Differentiable wrt the
    vertices (``ops.MeshLaplacian``: the backward is the transposed operator, a gather over the same adjacency), and so, through
    ``extract_mesh(..., differentiable=True)``, wrt the grid or the shape codes; the adjacency is a constant."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    live, adj, nvs = _adjacency(ms, adjacency)
    u = ops.MeshLaplacian.apply(live, adj)
    out = [u[v] for (v,) in _object_slices(nvs)]
    return out[0] if single else out


def laplacian_energy(meshes, adjacency=None):
    """(B,) fp32: per mesh the mean of |U_i|^2 over its vertices that have neighbours (0 for none), U = ``mesh_laplacian``: the standard
    first smoothness regulariser of a mesh, differentiable like ``mesh_laplacian`` -- ``laplacian_energy(extract_mesh(model, codes, ...,
    differentiable=True)).sum().backward()`` fills ``codes.grad``.  Per-object slices and ``sum()``: no atomics, the same bits from run to
    run."""
    ms, _ = _one_or_many(meshes)
    if not ms:
        return torch.zeros(0)
    live, adj, nvs = _adjacency(ms, adjacency)
    u = ops.MeshLaplacian.apply(live, adj)
    out = []
    for (v,) in _object_slices(nvs):
        count = (adj.degree[v] > 0).sum().clamp(min=1)
        out.append((u[v] ** 2).sum() / count)
    return torch.stack(out)


class MeshIndex(NamedTuple):
    mesh: ops.PackedMesh         # the meshes the index was built over, packed
    grid: ops.NearestIndex       # the grid of D3: cells, offsets and the sorted face lists


class Closest(NamedTuple):
    point: torch.Tensor          # (Q, 3) fp32: the closest point of the surface; with autograd to the vertices
    face: torch.Tensor           # (Q,) int32: the face it lies on; -1 where the query has no answer
    weights: torch.Tensor        # (Q, 3) fp32: its barycentric weights in that face
    distance: torch.Tensor       # (Q,) fp32: |points - point|; +inf where the query has no answer


class SurfaceSamples(NamedTuple):
    points: torch.Tensor         # (n, 3) fp32
    face: torch.Tensor           # (n,) int32; -1 for a mesh without area
    weights: torch.Tensor        # (n, 3) fp32: the barycentric weights of each point in its face


class MeshDistance(NamedTuple):
    """Per object (B,) float64; 0-dim for a single pair.  ``forward`` is from the samples of ``a`` to the surface of ``b``."""
    forward_mean: torch.Tensor
    forward_rms: torch.Tensor
    forward_max: torch.Tensor
    backward_mean: torch.Tensor
    backward_rms: torch.Tensor
    backward_max: torch.Tensor
    chamfer: torch.Tensor        # forward_mean + backward_mean
    hausdorff: torch.Tensor      # the larger of the two maxima, on the samples
    precision: object            # the share of a's samples within ``threshold`` of b; None without a threshold
    recall: object               # the share of b's samples within ``threshold`` of a
    fscore: object               # their harmonic mean (0 where both are 0)


def _packed_mesh(ms):
    verts, faces, nvs, nfs = _packed(ms)
    return ops.pack_mesh(verts, faces, nvs, nfs)


def mesh_index(meshes, cell=None) -> MeshIndex:
    """The search grid of ``closest_point`` over ``meshes`` -- the list ``extract_mesh`` returns, or one (verts, faces) pair -- built once
    and reusable for any number of queries (include/supnerf_hip.h, "Mesh distance", D3; ``ops.mesh_nearest_index``).  Every object gets
    cubic cells of edge ``cell`` (a float or one per object), anchored at the minimum of its vertices, at most 256 per axis; every face is
    listed in the cells its bounding box touches.  ``cell=None``: ``ops.NEAREST_CELL_FACTOR`` times the square root of the object's mean
    face area, but no less than 1/256 of its largest extent (``ops.mesh_default_cell``; the factor comes from the sweep in DESIGN 4.7.9).  The grid decides only how fast a query is answered, never what
    the answer is.  One host read (the pair count).  More than ``ops.NEAREST_MAX_PAIRS`` (cell, face) pairs raise ``SnrError`` with the
    cell size that fits; so do CPU tensors, faces that are not int32, a face index outside its mesh, a non-finite vertex and a ``cell``
    that is not positive and finite."""
    ms, _ = _one_or_many(meshes)
    if not ms:
        raise SnrError("mesh_index: no meshes")
    mesh = _packed_mesh(ms)
    B, dev = len(ms), mesh.verts.device
    if cell is None:
        cell = ops.mesh_default_cell(mesh)
    elif not torch.is_tensor(cell) or not cell.is_cuda:
        cell_h = torch.as_tensor(cell, dtype=torch.float32).reshape(-1)
        if not bool(((cell_h > 0) & torch.isfinite(cell_h)).all()):
            raise SnrError(f"mesh_index: cell must be positive and finite, got {cell_h.tolist()}")
    return MeshIndex(mesh, ops.mesh_nearest_index(mesh, cell))


def _index_for(ms, index, cell=None):
    if index is None:
        return mesh_index(ms, cell)
    if not isinstance(index, MeshIndex) or index.mesh.n_verts != [v.shape[0] for v, _ in ms] or index.mesh.n_faces != [f.shape[0] for _, f in ms]:
        raise SnrError("index is what mesh_index returned for these meshes")
    return index


def _per_object_points(points, B, single):
    if torch.is_tensor(points):
        if B != 1:
            raise SnrError(f"points are a list of (Q, 3) tensors, one per object: {B} meshes")
        points = [points]
    points = list(points)
    if len(points) != B:
        raise SnrError(f"{B} meshes but {len(points)} point tensors")
    for p in points:
        _gpu(p, "points")
        if p.dim() != 2 or p.shape[1] != 3:
            raise SnrError(f"points are (Q, 3) per object, got {tuple(p.shape)}")
    return points


def closest_point(meshes, points, index=None):
    """For every query point the closest point of its object's surface: ``meshes`` is the list ``extract_mesh`` returns with ``points`` a
    list of (Q, 3) tensors, one per object, or one (verts, faces) pair with one (Q, 3) tensor.  Returns one ``Closest(point, face,
    weights, distance)`` per object (a single one for a single pair).  ``index``: what ``mesh_index`` returned for these meshes, to save
    building it again (and its host read).

    The answer is exact: over all faces of the object the smallest float64 squared distance of Ericson's point-triangle walk, ties to
    the lowest face index (include/supnerf_hip.h, "Mesh distance"; ``snr_nearest_query``); the grid only prunes, bit for bit.  ``point``
    = sum_k weights_k verts[faces[face, k]] and ``distance`` = |points - point| are formed in torch, so autograd reaches ``points`` and
    the vertices (those of ``extract_mesh(..., differentiable=True)`` carry it on to the grid or the shape codes); face and weights are
    constants of that graph, as in the rasteriser.  When nothing requires grad, ``distance`` is the square root of the kernel's float64
    squared distance, rounded to fp32.  A query with a non-finite coordinate, and any query of a mesh without a usable face, has face
    -1, weights 0, point 0 and distance +inf.  CPU tensors raise ``SnrError``."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    pts = _per_object_points(points, len(ms), single)
    index = _index_for(ms, index)
    nqs = [p.shape[0] for p in pts]
    packed = pts[0] if len(pts) == 1 else torch.cat([p.float() for p in pts])
    face, weights, dist2 = ops.mesh_nearest_query(index.mesh, index.grid, packed, nqs)
    out = []
    for (v, f), p, (q,) in zip(ms, pts, _object_slices(nqs)):
        fa, w, d2 = face[q], weights[q], dist2[q]
        none = fa < 0
        live = torch.is_grad_enabled() and (p.requires_grad or v.requires_grad)
        if f.shape[0] and v.shape[0]:
            corners = v.float()[f.long()[fa.clamp(min=0).long()]]                 # (Q, 3 corners, 3)
            point = (w[:, :, None] * corners).sum(1)
        else:
            point = torch.zeros(p.shape[0], 3, device=p.device)
        if live:
            dist = torch.linalg.vector_norm(p.float() - point, dim=1)
            dist = torch.where(none, torch.full_like(dist, float("inf")), dist)
        else:
            dist = torch.sqrt(d2).float()
        out.append(Closest(point, fa, w, dist))
    return out[0] if single else out


def sample_surface(meshes, n, generator=None):
    """``n`` points per object spread evenly over the surface of each mesh of ``meshes`` -- the list ``extract_mesh`` returns, or one
    (verts, faces) pair: one ``SurfaceSamples(points, face, weights)`` per object (a single one for a single pair).  The draw is
    area-uniform and stratified along the faces (include/supnerf_hip.h, "Mesh distance", D5; ``snr_surface_sample``): the number of samples
    on a face differs from n area_f / area by less than 2, and a face without area gets none.  The randomness is ``torch.rand`` of
    (B n, 3) float64 from ``generator`` (on the meshes' device, or a CPU generator), so a seeded generator gives the same samples again.
    A mesh without area gets face -1 and points 0.  No host read.  CPU tensors and ``n < 0`` raise ``SnrError``."""
    if int(n) < 0:
        raise SnrError(f"n must not be negative, got {n}")
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    out = _sample(_packed_mesh(ms), int(n), generator)
    return out[0] if single else out


def _sample(mesh, n, generator):
    B, dev = len(mesh.n_verts), mesh.verts.device
    gdev = dev if generator is None else generator.device
    u = torch.rand(B * n, 3, dtype=torch.float64, device=gdev, generator=generator).to(dev)
    points, face, weights = ops.mesh_surface_sample(mesh, ops.mesh_cumulative_area(mesh), u, [n] * B)
    return [SurfaceSamples(points[s], face[s], weights[s]) for (s,) in _object_slices([n] * B)]


def mesh_distance(a, b, n=10000, generator=None, threshold=None, index_a=None, index_b=None) -> MeshDistance:
    """How far apart two surfaces are, object by object: ``a`` and ``b`` are lists of meshes of the same length (or one pair each), paired
    in order.  ``n`` surface samples are drawn on each side (``sample_surface`` of ``a``, then of ``b``, from ``generator``) and each is
    taken to the closest point of the OTHER surface (``closest_point``).  Per object and direction the mean, the root mean square and the
    maximum of those distances; ``chamfer`` = the sum of the two means; ``hausdorff`` = the larger maximum (on the samples: a lower bound
    of the true Hausdorff distance).  With ``threshold``: ``precision`` = the share of a's samples within it of b, ``recall`` = the share
    of b's samples within it of a, and their harmonic mean ``fscore`` (a = the reconstruction, b = the truth).  All values are (B,)
    float64 (0-dim for a single pair).  The sums of d and d^2 go through the fixed-order segmented sum, so the same generator state
    gives the same bits; nothing is read back beyond the two index builds.  A side without area gives +inf."""
    if int(n) < 1:
        raise SnrError(f"n must be positive, got {n}")
    if threshold is not None and not float(threshold) >= 0:
        raise SnrError(f"threshold must not be negative, got {threshold}")
    shape = [(1, True) if isinstance(m, (tuple, list)) and len(m) == 2 and torch.is_tensor(m[0]) else (len(m), False) for m in (a, b)]
    if shape[0] != shape[1]:
        raise SnrError(f"mesh_distance pairs the meshes of a and b object by object: got {shape[0][0]} and {shape[1][0]}"
                       f"{'' if shape[0][1] == shape[1][1] else ' (one pair and one list)'}")
    ma, single_a = _one_or_many(a)
    mb, _ = _one_or_many(b)
    if not ma:
        raise SnrError("mesh_distance: no meshes")
    n, B = int(n), len(ma)
    ia, ib = _index_for(ma, index_a), _index_for(mb, index_b)
    sa, sb = _sample(ia.mesh, n, generator), _sample(ib.mesh, n, generator)
    stats = []
    for samples, index in ((sa, ib), (sb, ia)):
        pts = torch.cat([s.points for s in samples]) if B > 1 else samples[0].points
        drawn = torch.cat([s.face for s in samples]) if B > 1 else samples[0].face
        _, _, d2 = ops.mesh_nearest_query(index.mesh, index.grid, pts, [n] * B)
        d2 = torch.where(drawn < 0, torch.full_like(d2, float("inf")), d2)       # (a side without area has no samples to measure from)
        d = torch.sqrt(d2)
        sum_d, sum_d2 = ops.object_sums(d, d2, [n] * B)
        within = None if threshold is None else (d.view(B, n) <= float(threshold)).sum(1).double() / n
        stats.append((sum_d / n, torch.sqrt(sum_d2 / n), d.view(B, n).amax(1), within))
    (fm, fr, fx, p), (bm, br, bx, r) = stats
    f = None if p is None else torch.where(p + r > 0, 2 * p * r / (p + r).clamp(min=1e-300), torch.zeros_like(p))
    out = (fm, fr, fx, bm, br, bx, fm + bm, torch.maximum(fx, bx), p, r, f)
    return MeshDistance(*[None if t is None else (t[0] if single_a else t) for t in out])


class SignedDistance(NamedTuple):
    distance: torch.Tensor       # (Q,) fp32: closest.distance, negated where the point is contained; +inf where the query has no answer
    closest: Closest             # what closest_point returns for the same queries
    winding: torch.Tensor        # (Q,) int32: the winding number the sign was taken from


class IoU(NamedTuple):
    """Per object (B,); 0-dim for a single grid or pair."""
    iou: torch.Tensor            # float64: intersection / union, 0 where the union is empty
    intersection: torch.Tensor   # int64: voxels set in both
    union: torch.Tensor          # int64: voxels set in either
    count_a: torch.Tensor        # int64: voxels set in a
    count_b: torch.Tensor        # int64


CONTAIN_RULES = ("nonzero", "positive", "odd")


def _contained(winding, rule):
    if rule == "nonzero":
        return winding != 0
    if rule == "positive":
        return winding > 0
    if rule == "odd":
        return (winding & 1) != 0
    raise SnrError(f"rule is one of {CONTAIN_RULES}, got {rule!r}")


def _winding(ms, pts, index):
    nqs = [p.shape[0] for p in pts]
    packed = pts[0] if len(pts) == 1 else torch.cat([p.detach().float() for p in pts])
    w = ops.mesh_inside_query(index.mesh, index.grid, packed, nqs)
    return [w[q] for (q,) in _object_slices(nqs)]


def winding_number(meshes, points, index=None):
    """For every query point the integer winding number of its object's mesh along +z -- the signed number of faces that the ray from the
    point in direction +z crosses: ``meshes`` is the list ``extract_mesh`` returns with ``points`` a list of (Q, 3) tensors, one per
    object, or one (verts, faces) pair with one (Q, 3) tensor.  Returns one (Q,) int32 tensor per object (a single one for a single
    pair).  ``index``: what ``mesh_index`` returned for these meshes -- the grid ``closest_point`` walks serves this search too.

    ``extract_mesh`` winds faces counter-clockwise seen from the low-density side, so for a closed mesh a point inside a solid piece gets
    +1, a point inside a closed cavity of it 0, a point where two pieces overlap 2, a point outside 0.  The value is exact: the
    brute-force sum over all faces by the rules of include/supnerf_hip.h ("Mesh containment", W1 - W5; ``snr_inside_query``), which give
    a point exactly under an edge or a vertex to exactly one face and a point on the surface to the side the rules name (for an
    axis-parallel box: the half-open box); the grid only prunes.  A mesh that is not closed -- one the border of the grid cut open --
    gets the value of these rules and no more: ``mesh_adjacency(...).closed`` is the check, and it is not run for the caller.  A query
    with a non-finite coordinate, and any query of a mesh without faces, gets 0.  No autograd; CPU tensors raise ``SnrError``."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    pts = _per_object_points(points, len(ms), single)
    out = _winding(ms, pts, _index_for(ms, index))
    return out[0] if single else out


def contains(meshes, points, index=None, rule="nonzero"):
    """Whether each query point lies inside its object's mesh: ``winding_number`` turned into a (Q,) bool tensor per object by ``rule`` --
    "nonzero" (inside any piece), "positive" (a cavity that overlaps a solid piece cancels it) or "odd" (the parity rule: the overlap of
    two pieces is outside).  For a closed mesh without overlaps the three agree.  An open mesh gets what ``winding_number`` gives it."""
    _contained(torch.zeros(0, dtype=torch.int32), rule)
    w = winding_number(meshes, points, index)
    return _contained(w, rule) if torch.is_tensor(w) else [_contained(x, rule) for x in w]


def signed_distance(meshes, points, index=None, rule="nonzero"):
    """The signed distance from every query point to its object's surface: one ``SignedDistance(distance, closest, winding)`` per object (a
    single one for a single pair).  ``closest`` is what ``closest_point`` returns; ``distance`` = ``closest.distance``, negated where
    ``contains(..., rule)`` holds.  The magnitude carries ``closest_point``'s autograd to the points and the vertices; the sign is a
    constant of that graph.  One index serves both searches (``index``: what ``mesh_index`` returned, or built here once).  A query
    without an answer (a non-finite coordinate, a mesh without faces) keeps +inf.  An open mesh gets the sign ``winding_number`` gives."""
    _contained(torch.zeros(0, dtype=torch.int32), rule)
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    pts = _per_object_points(points, len(ms), single)
    index = _index_for(ms, index)
    closest = closest_point(ms, pts, index=index)
    out = [SignedDistance(torch.where(_contained(w, rule), -c.distance, c.distance), c, w)
           for c, w in zip(closest, _winding(ms, pts, index))]
    return out[0] if single else out


def _bounds(bound, B, what):
    """One ``bound`` of ``lattice`` for every object (a tuple), or one per object (a list of B of them)."""
    if isinstance(bound, list):
        if len(bound) != B:
            raise SnrError(f"{what}: {B} meshes but {len(bound)} bounds")
        return bound
    return [bound] * B


def voxelize(meshes, resolution, bound=(-0.5, 0.5), index=None, rule="nonzero"):
    """The occupancy of each mesh on ``lattice(resolution, bound)`` -- the lattice ``density_grid`` uses, so ``voxelize(mesh, R) ==
    (density_grid(model, shapecode, R) > level)`` compares like with like: a (B, nx, ny, nz) bool tensor, (nx, ny, nz) for a single
    (verts, faces) pair.  ``bound`` is one bound for every object (a tuple, as ``lattice`` takes it) or a list of one per object.  A
    voxel is set where ``contains(..., rule)`` holds at its lattice point; the winding numbers come from ``snr_inside_lattice``
    (include/supnerf_hip.h, "Mesh containment", W6), which gives the integers of ``winding_number`` at ``lattice_points`` with the work
    that does not depend on z done once per face.  An open mesh gets what ``winding_number`` gives it.  No host read beyond the index
    build; CPU tensors raise ``SnrError``."""
    _contained(torch.zeros(0, dtype=torch.int32), rule)
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    lats = [lattice(resolution, b) for b in _bounds(bound, len(ms), "voxelize")]
    index = _index_for(ms, index)
    lo = torch.tensor([[lat.lo[a] for a in range(3)] for lat in lats], dtype=torch.float32)
    h = torch.tensor([[lat.h[a] for a in range(3)] for lat in lats], dtype=torch.float32)
    occ = _contained(ops.mesh_inside_lattice(index.mesh, index.grid, lo, h, [lats[0].n[a] for a in range(3)]), rule)
    return occ[0] if single else occ


def occupancy_iou(a, b) -> IoU:
    """The volumetric intersection over union of two bool occupancy grids of equal shape, (B, nx, ny, nz) or (nx, ny, nz) -- what
    ``voxelize`` returns, or ``density_grid(...) > level``: ``IoU(iou, intersection, union, count_a, count_b)`` per object.  The four
    counts are exact int64; ``iou`` = intersection / union in float64, 0 where the union is empty.  Plain tensor sums on the grids'
    device."""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dtype != torch.bool or b.dtype != torch.bool or a.shape != b.shape or \
            a.dim() not in (3, 4):
        raise SnrError("occupancy_iou takes two bool grids of equal shape, (B, nx, ny, nz) or (nx, ny, nz)")
    dims = (-3, -2, -1)
    inter, union = (a & b).sum(dims, dtype=torch.int64), (a | b).sum(dims, dtype=torch.int64)
    iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.zeros_like(inter, dtype=torch.float64))
    return IoU(iou, inter, union, a.sum(dims, dtype=torch.int64), b.sum(dims, dtype=torch.int64))


def iou_lattice(box_lo, box_hi, resolution):
    """(lo, h) (B, 3) fp32 of the lattice ``mesh_iou`` uses over the boxes ``box_lo`` .. ``box_hi`` (B, 3) fp32: the centres of
    ``resolution``^3 equal boxes.  In fp32, each operation rounded:  h = (box_hi - box_lo) / resolution;  lo = box_lo + h * 0.5;  point i
    is then lo + h * i (a multiply, then an add), as on every lattice of this module."""
    h = (box_hi.float() - box_lo.float()) / torch.tensor(float(int(resolution)), dtype=torch.float32, device=box_lo.device)
    return box_lo.float() + h * 0.5, h


def mesh_iou(a, b, resolution=64, bound=None, rule="nonzero", index_a=None, index_b=None) -> IoU:
    """The volumetric IoU of two meshes, object by object: ``a`` and ``b`` are lists of meshes of the same length (or one pair each),
    paired in order as ``mesh_distance`` pairs them.  Both are voxelised (``snr_inside_lattice``, ``rule`` as in ``contains``) on one
    lattice per object: the centres of ``resolution``^3 equal boxes that fill ``bound`` -- one bound as ``lattice`` takes it (a tuple), a
    list of one per object, or ``None``: per object the union of the two meshes' bounding boxes (the exact fp32 minimum and maximum of
    their vertices; a mesh without vertices adds nothing).  With the box [lo_box, hi_box], in fp32 with every operation rounded:
    h = (hi_box - lo_box) / resolution, lo = lo_box + h * 0.5, point i = lo + h * i (``iou_lattice``).  Returns ``occupancy_iou`` of
    the two grids: exact counts, so the volumes are count * h_x h_y h_z.  Open meshes get what ``winding_number`` gives them.  No host
    read beyond the index builds."""
    _contained(torch.zeros(0, dtype=torch.int32), rule)
    R = int(resolution)
    if R < 1 or R > MAX_RESOLUTION:
        raise SnrError(f"resolution must be 1..{MAX_RESOLUTION}, got {resolution}")
    shape = [(1, True) if isinstance(m, (tuple, list)) and len(m) == 2 and torch.is_tensor(m[0]) else (len(m), False) for m in (a, b)]
    if shape[0] != shape[1]:
        raise SnrError(f"mesh_iou pairs the meshes of a and b object by object: got {shape[0][0]} and {shape[1][0]}"
                       f"{'' if shape[0][1] == shape[1][1] else ' (one pair and one list)'}")
    ma, single = _one_or_many(a)
    mb, _ = _one_or_many(b)
    if not ma:
        raise SnrError("mesh_iou: no meshes")
    B = len(ma)
    ia, ib = _index_for(ma, index_a), _index_for(mb, index_b)
    dev = ia.mesh.verts.device
    if bound is None:
        box_lo, box_hi = [], []
        for k in range(B):
            sides = [i.grid for i, ms in ((ia, ma), (ib, mb)) if ms[k][0].shape[0]]
            box_lo.append(torch.stack([g.grid_lo[k] for g in sides]).amin(0) if sides else torch.zeros(3, device=dev))
            box_hi.append(torch.stack([g.grid_hi[k] for g in sides]).amax(0) if sides else torch.zeros(3, device=dev))
        box_lo, box_hi = torch.stack(box_lo), torch.stack(box_hi)
    else:
        pairs = [(np.broadcast_to(np.asarray(lo, np.float32), (3,)), np.broadcast_to(np.asarray(hi, np.float32), (3,)))
                 for lo, hi in _bounds(bound, B, "mesh_iou")]
        box_lo = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        box_hi = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    lo, h = iou_lattice(box_lo, box_hi, R)
    grids = [_contained(ops.mesh_inside_lattice(i.mesh, i.grid, lo, h, (R, R, R)), rule) for i in (ia, ib)]
    out = occupancy_iou(*grids)
    return IoU(*[t[0] for t in out]) if single else out


def to_object_frame(verts, obj_diag, family="a", shapenet_obj_cood=False, kitti2nusc=False, direction=False):
    """Decoder-frame points (..., 3) -> the object's metric frame, inverting the package's point mappings:
    family "a" (``utils`` render paths, ``_render_shared_z``): x = F (p / obj_diag);
    family "b" (``renderer.NeRFRenderer``): x = F (p / (obj_diag / 2)), obj_diag = |(l, w, h)|;
    F = ``utils._frame(False, kitti2nusc, shapenet_obj_cood)``, the frame both paths hand the kernels (a signed permutation: F^-1 = F^T).
    ``direction=True``: directions such as normals, F applied without the scale (unit vectors stay unit)."""
    if family not in ("a", "b"):
        raise SnrError(f"family is 'a' (utils render paths) or 'b' (NeRFRenderer), got {family!r}")
    v = torch.as_tensor(verts)
    m = torch.tensor(U._frame(False, kitti2nusc, shapenet_obj_cood), dtype=v.dtype, device=v.device).view(3, 3)
    if direction:
        return v @ m
    scale = float(obj_diag) if family == "a" else float(obj_diag) / 2
    return (v @ m) * scale


def _frame_scale(obj_diag, family):
    if family not in ("a", "b"):
        raise SnrError(f"family is 'a' (utils render paths) or 'b' (NeRFRenderer), got {family!r}")
    return float(obj_diag) if family == "a" else float(obj_diag) / 2


def to_decoder_frame(points, obj_diag, family="a", shapenet_obj_cood=False, kitti2nusc=False, direction=False):
    """The inverse of ``to_object_frame``: points (..., 3) of the object's metric frame -> the decoder frame, p = F^T (x / scale) with
    the same frame matrix and scale (obj_diag for family "a", obj_diag / 2 for "b"); ``direction=True``: directions, without the scale.
    Plain torch operations: differentiable wrt ``points``."""
    scale = _frame_scale(obj_diag, family)
    v = torch.as_tensor(points)
    m = torch.tensor(U._frame(False, kitti2nusc, shapenet_obj_cood), dtype=v.dtype, device=v.device).view(3, 3)
    if direction:
        return v @ m.T
    return (v / scale) @ m.T


class Raster(NamedTuple):
    face: torch.Tensor       # (n_images, H, W) int32: the packed index of the face each pixel sees; -1 where empty
    obj: torch.Tensor        # (n_images, H, W) int32: the object that face belongs to; -1 where empty
    depth: torch.Tensor      # (n_images, H, W): camera z of the surface at the pixel centre; 0 where empty
    weights: torch.Tensor    # (n_images, H, W, 3): perspective-correct barycentric weights of the face's three vertices; 0 where empty
    mesh: ops.PackedMesh     # the packed mesh ``face`` indexes


def _camera(K):
    """(fx, fy, cx, cy) as host floats from a 3x3 intrinsic matrix or from the four numbers themselves.  The camera travels to the kernels
    by value, so ``K`` is a host value (numpy, a tuple, a CPU tensor); a ``K`` on the GPU costs one synchronising copy, as in
    ``utils._cam_table``."""
    k = K.detach().cpu() if torch.is_tensor(K) else K
    k = np.asarray(k, dtype=np.float64)
    if k.shape == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if k.shape == (4,):
        return tuple(float(v) for v in k)
    raise SnrError(f"K is a 3x3 intrinsic matrix or (fx, fy, cx, cy), got shape {k.shape}")


def _det3(m):
    """Determinant of (..., 3, 3+) matrices' left 3x3 blocks by the rule of Sarrus' cofactors (plain arithmetic: no host read)."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, i = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)


def _pack(meshes):
    ms, _ = _one_or_many(meshes)
    if not ms:
        raise SnrError("no mesh to draw")
    return ops.pack_mesh(*_packed(ms))


def rasterize(meshes, obj_to_cam, K, size, *, cull=None, z_near=1e-3, per_object=False):
    """Draw ``meshes`` -- the list ``extract_mesh`` returns, or one (verts, faces) pair -- as a pinhole camera sees them: per pixel the
    nearest face, its depth and barycentric weights (include/supnerf_hip.h, "Mesh rasteriser"; ``snr_raster_*``).

    ``obj_to_cam``: (B, 3, 4), one matrix per object that maps its stored vertices to the camera frame (x right, y down, z forward); a
    (3, 4) matrix with one mesh.  ``K``: the 3x3 intrinsic matrix or (fx, fy, cx, cy); pixel centres lie at integer coordinates, pixel
    (px, py) looks along ((px - cx) / fx, (py - cy) / fy, 1) as in ``utils.get_rays``.  ``size = (H, W)``.  ``per_object=False``: all
    objects into one scene image (n_images = 1); ``True``: one image per object.  ``cull="back"`` drops the faces seen from inside
    (``extract_mesh`` winds faces counter-clockwise seen from outside; a mirroring ``obj_to_cam`` is accounted for by the sign of its
    determinant); ``None`` draws both sides.

    Vertices are snapped to 1/256 pixel; coverage is exact with a tie rule that gives a pixel centre on a shared edge to exactly one
    face; of the covering faces the nearest wins, ties to the lowest face index: the same bits from run to run.  A face with a vertex
    nearer than ``z_near``, not finite, or 2^22 pixels or more off the image origin is dropped WHOLE: nothing is clipped against the near
    plane, the objects this is for lie in front of the camera.  No anti-aliasing.

    Returns a ``Raster``.  The outputs carry no autograd (hard visibility gives the silhouette no gradient; ``ray_surface`` is the
    differentiable depth).  ``K``, ``size`` and ``z_near`` are host values (a ``K`` on the GPU is copied to the host first, one
    synchronising read); with those on the host the call is asynchronous on the current stream and reads nothing back: meshes and
    ``obj_to_cam`` stay on the device.  CPU meshes raise ``SnrError``."""
    mesh = _pack(meshes)
    B, dev = len(mesh.n_verts), mesh.verts.device
    if cull not in (None, "back"):
        raise SnrError(f"cull is None or 'back', got {cull!r}")
    if not float(z_near) > 0:
        raise SnrError(f"z_near must be positive, got {z_near}")
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise SnrError(f"size is (H, W) with at least one pixel each way, got {tuple(size)}")
    m = torch.as_tensor(obj_to_cam).detach()
    if m.dim() == 2 and B == 1:
        m = m.unsqueeze(0)
    if tuple(m.shape) != (B, 3, 4):
        raise SnrError(f"obj_to_cam must be ({B}, 3, 4), one matrix per object, got {tuple(m.shape)}")
    cull_sign = None
    if cull == "back":
        cull_sign = torch.sign(_det3(m.double())).to(torch.int32).to(dev)
    n_images = B if per_object else 1
    image_of = torch.arange(B, dtype=torch.int32).to(dev) if per_object else torch.zeros(B, dtype=torch.int32, device=dev)
    face, depth, weights, _ = ops.rasterize(mesh, m.float().to(dev), _camera(K), image_of, n_images, H, W, z_near, cull_sign)
    obj = torch.bucketize(face, mesh.face_offset[1:], right=True, out_int32=True)
    return Raster(face, torch.where(face < 0, face, obj), depth, weights, mesh)


def interpolate(raster, attributes, background=0.0):
    """Per-vertex ``attributes`` of the meshes of a ``Raster`` -- a per-object list of (V, C) tensors, or one packed (sum V, C) tensor, C
    up to 16 (normals, colours ...) -- interpolated to its pixels with the perspective-correct weights: (n_images, H, W, C), ``background``
    where no face is seen.  No autograd."""
    a = attributes
    if not torch.is_tensor(a):
        a = [_gpu(x, "attributes") for x in a]
        if len(a) != len(raster.mesh.n_verts) or any(x.dim() != 2 or x.shape[0] != n for x, n in zip(a, raster.mesh.n_verts)):
            raise SnrError(f"attributes are one (V, C) tensor per object, V = {raster.mesh.n_verts}")
        a = torch.cat([x.detach().float() for x in a]) if len(a) > 1 else a[0]
    return ops.raster_interpolate(raster.mesh, raster.face, raster.weights, _gpu(a, "attributes"), background)


class MeshView(NamedTuple):
    depth: torch.Tensor      # (H, W): metres along the unit view direction of the pixel, as ``surface_depth``; 0 where empty
    mask: torch.Tensor       # (H, W) bool: a face is seen
    face: torch.Tensor       # (H, W) int32: its packed index; -1 where empty
    normal: torch.Tensor     # (H, W, 3) unit, object frame (None without ``normals``); 0 where empty
    color: torch.Tensor      # (H, W, 3) (None without ``colors``); 0 where empty


def _frame_matrix(shapenet_obj_cood, kitti2nusc, like):
    """(3, 3) float64 F^T with x_object = scale F^T p for decoder-frame p: ``to_object_frame`` as a matrix, on ``like``'s device."""
    return torch.tensor(U._frame(False, kitti2nusc, shapenet_obj_cood), dtype=torch.float64, device=like.device).view(3, 3).T


def _inverse3(r):
    """Inverse of a (3, 3) matrix by cofactors (plain arithmetic: no host read)."""
    c = torch.stack([torch.linalg.cross(r[1], r[2]), torch.linalg.cross(r[2], r[0]), torch.linalg.cross(r[0], r[1])], dim=1)
    return c / (r[0] * torch.linalg.cross(r[1], r[2])).sum()


def _view_camera(cam_pose, obj_diag, K, roi, im_sz, family, shapenet_obj_cood, kitti2nusc):
    """What ``mesh_view`` and ``paint_mesh`` draw a decoder-frame mesh with: (the (3, 4) float64 decoder -> camera matrix on ``cam_pose``'s
    device, the effective (fx, fy, cx, cy) of the pixel grid over ``roi``, its size (ny, nx)).  The decoder -> object map of
    ``to_object_frame`` (frame matrix and scale), the inverse of ``cam_pose`` and the affine pixel grid (offset x0, y0 and the step of
    ``im_sz``) are composed in float64."""
    scale = _frame_scale(obj_diag, family)
    pose = torch.as_tensor(cam_pose).detach().double()[:3]
    if tuple(pose.shape) != (3, 4):
        raise SnrError(f"cam_pose is (3, 4) or (4, 4), got {tuple(torch.as_tensor(cam_pose).shape)}")
    r_inv = _inverse3(pose[:, :3])
    m = torch.cat([r_inv @ _frame_matrix(shapenet_obj_cood, kitti2nusc, pose) * scale, -(r_inv @ pose[:, 3:4])], dim=1)
    fx, fy, cx, cy = _camera(K)
    x0, y0, x1, y1 = [int(v) for v in roi]
    nx, ny = (int(im_sz), int(im_sz)) if im_sz is not None else (x1 - x0, y1 - y0)
    sx = (x1 - 1 - x0) / (nx - 1) if nx > 1 else 1.0
    sy = (y1 - 1 - y0) / (ny - 1) if ny > 1 else 1.0
    return m, (fx / sx, fy / sy, (cx - x0) / sx, (cy - y0) / sy), (ny, nx)


def mesh_view(meshes, cam_pose, obj_diag, K, roi, *, im_sz=None, cull="back", family="a", shapenet_obj_cood=False, kitti2nusc=False,
              normals=None, colors=None, z_near=1e-3):
    """One object's decoder-frame mesh (a (verts, faces) pair, or a list of pieces that share the pose) on the pixel grid of
    ``utils.get_rays(K, cam_pose, roi, uv_steps)``: the mesh-speed mirror of ``surface_depth``.  ``cam_pose``: the camera in the object's
    frame, (3, 4).  Pixel (i, j) of the result is the pixel ``get_rays`` shoots ray i nx + j through; ``im_sz``: an ``im_sz`` x ``im_sz``
    grid over ``roi`` instead of one ray per pixel.

    The decoder -> object map of ``to_object_frame`` (frame matrix and scale), the inverse of ``cam_pose`` and the affine pixel grid
    (offset x0, y0 and the step of ``im_sz``) are composed in float64 into one matrix and one effective (fx, fy, cx, cy), then
    ``rasterize`` draws.  Returns a ``MeshView``: depth in metres along the unit view direction (camera z times
    |((px - cx) / fx, (py - cy) / fy, 1)|), comparable with ``surface_depth``; the hit mask; the face index; with ``normals`` / ``colors``
    (per-vertex, as ``vertex_normals`` / ``vertex_colors`` return them) the interpolated normals, renormalised and mapped to the object's
    frame with ``to_object_frame(direction=True)``, and colours.  ``obj_diag``, ``K``, ``roi`` and ``im_sz`` are host values; ``cam_pose``
    stays on its device.  No autograd."""
    m, cam, (ny, nx) = _view_camera(cam_pose, obj_diag, K, roi, im_sz, family, shapenet_obj_cood, kitti2nusc)
    ms, single = _one_or_many(meshes)
    r = rasterize(ms, m.unsqueeze(0).expand(len(ms), 3, 4), cam, (ny, nx), cull=cull, z_near=z_near)
    dev = r.depth.device
    px = (torch.arange(nx, dtype=torch.float64, device=dev) - cam[2]) / cam[0]
    py = (torch.arange(ny, dtype=torch.float64, device=dev) - cam[3]) / cam[1]
    length = torch.sqrt(px[None, :] ** 2 + py[:, None] ** 2 + 1.0).float()
    normal = color = None
    if normals is not None:
        n = torch.nn.functional.normalize(interpolate(r, [normals] if single else list(normals))[0], dim=-1)
        normal = to_object_frame(n, obj_diag, family, shapenet_obj_cood, kitti2nusc, direction=True)
    if colors is not None:
        color = interpolate(r, [colors] if single else list(colors))[0]
    return MeshView(r.depth[0] * length, r.face[0] >= 0, r.face[0], normal, color)


class Painted(NamedTuple):
    colors: torch.Tensor     # (V, 3) fp32: the painted colour; fallback / background where nothing reached the vertex
    weight: torch.Tensor     # (V,) fp32: the sum of the views' weights ("weighted") or the best view's weight ("best"); 0 where unseen
    seen: torch.Tensor       # (V,) int32: how many views see the vertex
    best: torch.Tensor       # (V,) int32: the view that faces it most squarely (ties: the lowest index); -1 where unseen
    filled: torch.Tensor     # (V,) int32: 0 seen by a view; r >= 1 filled from neighbours in round r; -1 neither


def _paint_views(views):
    """The views of ``paint_mesh``, checked as far as the host can: [(img, mask or None, (h, w))]."""
    if isinstance(views, dict) or not isinstance(views, (list, tuple)) or not views:
        raise SnrError("views is a non-empty list of the dicts an instance of optimize_instances carries (img, mask, cam_pose, obj_diag, "
                       "K, roi)")
    out = []
    for v, view in enumerate(views):
        missing = [k for k in ("img", "cam_pose", "obj_diag", "K", "roi") if k not in view]
        if missing:
            raise SnrError(f"paint_mesh: view {v} has no {missing}")
        x0, y0, x1, y1 = [int(t) for t in view["roi"]]
        h, w = y1 - y0, x1 - x0
        img, mask = torch.as_tensor(view["img"]), view.get("mask")
        mask = None if mask is None else torch.as_tensor(mask)
        if h < 1 or w < 1 or tuple(img.shape) != (h, w, 3) or (mask is not None and mask.numel() != h * w):
            raise SnrError(f"paint_mesh: view {v}: img {tuple(img.shape)} / mask {None if mask is None else tuple(mask.shape)} are not the "
                           f"native {h} x {w} crop of its roi")
        out.append((img, mask, (h, w)))
    return out


def paint_mesh(meshes, views, *, normals=None, blend="weighted", facing=True, tol=None, fill=0, adjacency=None, fallback=None,
               background=0.0, cull="back", family="a", shapenet_obj_cood=False, kitti2nusc=False, z_near=1e-3):
    """Vertex colours from the photographs: one object's decoder-frame mesh (a (verts, faces) pair, or a list of pieces that share the
    pose, as in ``mesh_view``) painted from ``views``, the list an instance of ``optimize_instances`` carries -- per view ``img`` (h, w, 3),
    the native crop of its ``roi``; optionally ``mask`` (h w values: > 0 the object, 0 background, -1 another object in front);
    ``cam_pose``, ``obj_diag``, ``K``, ``roi`` as ``mesh_view`` takes them (include/supnerf_hip.h, "Mesh painting"; ``snr_paint_*``).

    Per view the mesh is drawn on the crop's pixel grid exactly as ``mesh_view`` draws it (one composition in float64, then
    ``ops.rasterize``); its depth buffer decides which vertices the view sees.  A vertex samples the image bilinearly at its projection
    (pixel centres at integers) over those of its four taps that show the mesh no nearer than the vertex (within ``tol``) and lie inside
    the mask, renormalised by their weights: the whitened background and an occluder never bleed in.  A view weighs cos^2 of the angle
    between the vertex normal and the direction to its camera (``facing=True``, which needs ``normals`` as ``vertex_normals`` returns them;
    a view that faces away does not see the vertex), or 1 (``facing=False``: ``normals`` are ignored).

    * ``blend``: ``"weighted"`` = the weighted mean over the views that see the vertex; ``"best"`` = the colour of the view with the
      largest weight, ties to the lowest view index.
    * ``tol``: how far behind the depth buffer (metres of camera z) a vertex may lie and still be seen.  Default ``0.01 * obj_diag`` of the
      view: a stated choice, not a measured optimum -- at 20 m with fx ~ 1266 one pixel spans about 1.6 cm, so for a 4.7 m car it is
      about the depth a 45-degree surface gains over three pixels.  Smaller values drop grazing vertices, larger ones let vertices
      just behind a rim take the rim's colour.
    * ``fill=R``: R rounds in which every uncoloured vertex with coloured neighbours takes their mean (``adjacency``: what
      ``mesh_adjacency`` returned for these meshes, else it is built here, with its one host read).
    * A vertex still uncoloured takes its row of ``fallback`` ((V, 3), or a list of them per piece; for example ``vertex_colors``), else
      ``background``; its ``filled`` stays -1.

    Returns a ``Painted`` (a list of them for a list of pieces).  Views are painted in ascending order, one launch each, plain fp32
    sums: the same bits from run to run.  Host values (``K``, ``roi``, ``obj_diag``; a ``cam_pose`` on the GPU is copied to the host, one
    synchronising read, for the camera centre) aside, the call is asynchronous on the current stream and reads nothing back.  No
    autograd.  CPU meshes raise ``SnrError``."""
    if blend not in ops.PAINT_BLENDS:
        raise SnrError(f"blend is one of {ops.PAINT_BLENDS}, got {blend!r}")
    if int(fill) < 0:
        raise SnrError(f"fill must not be negative, got {fill}")
    if facing and normals is None:
        raise SnrError("facing=True weighs the views by the vertex normals: pass normals (vertex_normals), or facing=False")
    if tol is not None and not (float(tol) >= 0 and np.isfinite(float(tol))):
        raise SnrError(f"tol must be finite and not negative, got {tol}")
    if cull not in (None, "back"):
        raise SnrError(f"cull is None or 'back', got {cull!r}")
    if not float(z_near) > 0:
        raise SnrError(f"z_near must be positive, got {z_near}")
    _frame_scale(1.0, family)
    crops = _paint_views(views)
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    mesh = ops.pack_mesh(*_packed(ms))
    B, dev, nV = len(ms), mesh.verts.device, mesh.verts.shape[0]
    nrm = None
    if facing:
        rows = _per_object_rows(normals, ms, "normals")
        if any(tuple(n.shape) != (v.shape[0], 3) for n, (v, _) in zip(rows, ms)):
            raise SnrError(f"normals are (V, 3) per object, got {[tuple(n.shape) for n in rows]}")
        nrm = (rows[0] if B == 1 else torch.cat(rows)).detach().float().contiguous()
    fb = None
    if fallback is not None:
        rows = _per_object_rows(fallback, ms, "fallback colours")
        if any(tuple(c.shape) != (v.shape[0], 3) for c, (v, _) in zip(rows, ms)):
            raise SnrError(f"fallback colours are (V, 3) per object, got {[tuple(c.shape) for c in rows]}")
        fb = (rows[0] if B == 1 else torch.cat(rows)).detach().float()
    adj = _adjacency(ms, adjacency)[1] if int(fill) > 0 else None
    state = ops.paint_state(nV, dev)
    image_of = torch.zeros(B, dtype=torch.int32, device=dev)
    for k, (view, (img, mask, (h, w))) in enumerate(zip(views, crops)):
        m, cam, _ = _view_camera(view["cam_pose"], view["obj_diag"], view["K"], view["roi"], None, family, shapenet_obj_cood, kitti2nusc)
        cull_sign = torch.sign(_det3(m)).to(torch.int32).to(dev).expand(B).contiguous() if cull == "back" else None
        _, depth, _, screen = ops.rasterize(mesh, m.unsqueeze(0).expand(B, 3, 4).float().to(dev), cam, image_of, 1, h, w, z_near, cull_sign)
        centre = to_decoder_frame(torch.as_tensor(view["cam_pose"]).detach().double().cpu()[:3, 3], view["obj_diag"], family,
                                  shapenet_obj_cood, kitti2nusc).tolist()
        ops.paint_view(mesh, screen, nrm, img.detach().float().contiguous().to(dev),
                       None if mask is None else mask.detach().float().reshape(h, w).contiguous().to(dev), depth[0], centre,
                       0.01 * float(view["obj_diag"]) if tol is None else float(tol), z_near, k, state)
    colors, filled = ops.paint_finish(state, blend, background)
    if adj is not None:
        colors, filled = ops.paint_fill(colors, filled, adj, int(fill))
    if fb is not None:
        colors = torch.where((filled < 0)[:, None], fb, colors)
    weight = state.sum_w if blend == "weighted" else state.best_w
    out = [Painted(colors[v], weight[v], state.seen[v], state.best[v], filled[v]) for (v,) in _object_slices(mesh.n_verts)]
    return out[0] if single else out


class SceneView(NamedTuple):
    depth: torch.Tensor      # (H, W): camera z of the nearest surface; 0 where empty
    obj: torch.Tensor        # (H, W) int32: the instance (index into ``meshes``) each pixel sees; -1 where empty
    face: torch.Tensor       # (H, W) int32: packed face index; -1 where empty
    normal: torch.Tensor     # (H, W, 3) unit, CAMERA frame (None without ``normals``)
    color: torch.Tensor      # (H, W, 3) (None without ``colors``)


def scene_view(meshes, obj_poses, obj_diags, K, H, W, *, cull="back", family="a", shapenet_obj_cood=False, kitti2nusc=False, normals=None,
               colors=None, z_near=1e-3):
    """All objects of a scene in one full H x W image: the mesh-speed counterpart of ``scene.vis_scene``.  ``meshes``: one decoder-frame
    mesh per object; ``obj_poses`` (B, 3, 4): object -> camera, ``scene``'s convention; ``obj_diags`` (B,): each object's diagonal
    (``to_object_frame``'s scale).  Returns a ``SceneView``: z-buffer depth (camera z, metres), the instance id per pixel, the face index
    and, with per-object lists ``normals`` / ``colors``, the interpolated normals (renormalised, rotated to the camera frame) and colours.
    ``K``, ``H`` and ``W`` are host values; poses and diagonals may live on either side.  No autograd."""
    ms = _meshes(meshes)
    poses = torch.as_tensor(obj_poses).detach().double()
    diags = torch.as_tensor(obj_diags).detach().double().to(poses.device).reshape(-1)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] != len(ms) or diags.shape[0] != len(ms):
        raise SnrError(f"{len(ms)} meshes take obj_poses ({len(ms)}, 3, 4) and {len(ms)} obj_diags, got {tuple(poses.shape)} and "
                       f"{tuple(diags.shape)}")
    rot = poses[:, :, :3] @ _frame_matrix(shapenet_obj_cood, kitti2nusc, poses)
    m = torch.cat([rot * (diags * _frame_scale(1.0, family)).view(-1, 1, 1), poses[:, :, 3:4]], dim=2)
    r = rasterize(ms, m, K, (H, W), cull=cull, z_near=z_near)
    normal = color = None
    if normals is not None:
        # rotate each object's normals to the camera frame before they are interpolated: one attribute pass for the whole scene
        rot = rot.float().to(r.depth.device)
        cam_n = [_gpu(n, "normals").detach().float() @ rot[b].T for b, n in enumerate(normals)]
        normal = torch.nn.functional.normalize(interpolate(r, cam_n)[0], dim=-1)
    if colors is not None:
        color = interpolate(r, list(colors))[0]
    return SceneView(r.depth[0], r.obj[0], r.face[0], normal, color)


class RayHits(NamedTuple):
    depth: torch.Tensor      # (B, N): t of the first crossing (units of |rays_d|); near where the ray starts inside; 0 on a miss
    state: torch.Tensor      # (B, N) uint8: 0 miss, 1 hit, 2 the ray starts inside
    normal: torch.Tensor     # (B, N, 3): unit outward normal -grad sigma / |grad sigma| at the hit point; zero where state != 1
    width: torch.Tensor      # (B, N): width of the final bracket, which holds both the depth and the true crossing; 0 where state != 1


DEFAULT_REFINE = (4, 5)          # the fastest of the four settings that shrink the bracket 256 times, as measured


def _ray_bound(v, what, shape, dev):
    """near / far as a dense (B N,) fp32 device tensor: a python float, a 0-dim tensor or a tensor of the rays' leading shape."""
    if torch.is_tensor(v):
        if v.dim() == 0:
            return v.detach().to(dev, torch.float32).expand(shape).reshape(-1).contiguous()
        _gpu(v, what)
        if tuple(v.shape) != tuple(shape):
            raise SnrError(f"{what} must be a float, a 0-dim tensor or {tuple(shape)}, got {tuple(v.shape)}")
        return v.detach().float().reshape(-1).contiguous()
    return torch.full((int(np.prod(shape)),), float(v), device=dev)


def ray_surface(model, rays_o, rays_d, near, far, shapecode, *, level, n_samples=64, refine=DEFAULT_REFINE):
    """Along each ray rays_o + t rays_d, t in [near, far], the first point where the density of its object's shape code rises through
    ``level``.  ``rays_o``, ``rays_d``: (B, N, 3) decoder-frame rays of the B codes of ``shapecode`` (B, 256), or (N, 3) with one code;
    ``rays_d`` need not be unit (t is in units of |rays_d|).  ``near`` / ``far``: python floats, 0-dim tensors or (B, N).

    The search: ``n_samples`` equidistant samples of [near, far]; a sample is inside iff sigma >= level; the first outside -> inside pair
    is the ray's bracket.  ``refine = (levels, samples)``: ``levels`` times, the bracket is sampled again with ``samples`` points and
    replaced by its first crossing -- (levels, 3) is bisection; the bracket shrinks by (samples - 1) ** levels.  The depth interpolates
    linearly in the final bracket.  A surface thinner than a step of the first march between two samples is not seen.

    Returns ``RayHits`` (depth, state, normal, width) shaped like the rays.  ``depth`` carries autograd to ``rays_o``, ``rays_d`` and
    ``shapecode``: the derivative of the root of sigma(o + t d; code) = level at the point found (implicit function theorem), whatever
    the bracket -- not that of the interpolation formula.  ``near``, ``far`` and ``level`` get no gradient, nor do changes of topology
    (hit <-> miss, which crossing is first); a grazing ray (grad sigma . d -> 0) gets a large one, unclamped.  Misses and rays that start
    inside get exactly zero.  The normals carry no gradient.  The decoder's weights are constants: with ``train_decoder_weights`` set and
    grad mode on this raises, as ``density`` does.  Asynchronous on the current stream; nothing is read back to the host."""
    o, d = _gpu(rays_o, "rays_o"), _gpu(rays_d, "rays_d")
    if o.dim() not in (2, 3) or o.shape[-1] != 3 or tuple(d.shape) != tuple(o.shape):
        raise SnrError(f"rays_o and rays_d must both be (B, N, 3) or (N, 3), got {tuple(o.shape)} and {tuple(d.shape)}")
    n_samples = int(n_samples)
    if n_samples < 2:
        raise SnrError(f"n_samples must be at least 2, got {n_samples}")
    levels, samples = (0, 2) if refine is None else refine
    levels = int(levels)
    samples = 2 if (levels == 0 and samples is None) else int(samples)
    if levels < 0 or samples < 2:
        raise SnrError(f"refine is (levels >= 0, samples >= 2), got {refine!r}")
    if not torch.is_tensor(near) and not torch.is_tensor(far) and float(far) < float(near):
        raise SnrError(f"far {far} lies before near {near}")
    sc, latent, packed = _decoder_inputs(model, shapecode, differentiable="geometry.ray_surface")
    lead = tuple(o.shape[:-1])
    B = sc.shape[0]
    if (o.dim() == 2 and B != 1) or (o.dim() == 3 and o.shape[0] != B):
        raise SnrError(f"rays {tuple(o.shape)} do not match {B} shape code(s): (B, N, 3) rays, or (N, 3) with one code")
    dev = o.device
    ta, tb = _ray_bound(near, "near", lead, dev), _ray_bound(far, "far", lead, dev)
    t, state, normal, width = ops.RaySurface.apply(o.reshape(-1, 3), d.reshape(-1, 3), ta, tb, latent, packed, float(np.float32(level)),
                                                   n_samples, levels, samples, model.shape_blocks, model.texture_blocks)
    return RayHits(t.view(lead), state.view(lead), normal.view(*lead, 3), width.view(lead))


def surface_depth(model, cam_pose, obj_diag, K, roi, shapecode, *, level, im_sz=None, pixels=None, n_samples=64, refine=DEFAULT_REFINE,
                  family="a", shapenet_obj_cood=False, kitti2nusc=False):
    """The surface {sigma = level} of one object as a camera sees it, in metric units: ``ray_surface`` on the rays of ``utils.get_rays``
    (a grid over ``roi``, ``im_sz`` x ``im_sz`` steps or one per pixel) or of ``utils.get_rays_specified`` (``pixels = (x_vec, y_vec)`` in
    image coordinates: lidar returns), between the bounds of ``utils._sphere_bounds``.  ``cam_pose``: the camera in the object's frame
    (3, 4), on the GPU.  Returns ``RayHits``: depth and width in metres along the unit view direction, normals in the object's frame
    (``to_object_frame(direction=True)``), shaped (H, W[, 3]) for a grid and (n[, 3]) for listed pixels.  Gradients reach ``cam_pose``
    through the ray operators and ``shapecode`` through ``ray_surface``; the bounds are detached, as in the render paths."""
    scale = _frame_scale(obj_diag, family)
    _gpu(cam_pose, "cam_pose")
    if pixels is not None:
        rays_o, viewdir = U.get_rays_specified(K, cam_pose, pixels[0], pixels[1])
        shape = (rays_o.shape[0],)
    else:
        steps = None if im_sz is None else [int(im_sz), int(im_sz)]
        rays_o, viewdir = U.get_rays(K, cam_pose, roi, uv_steps=steps)
        x0, y0, x1, y1 = [int(v) for v in roi]
        shape = (int(im_sz), int(im_sz)) if im_sz is not None else (y1 - y0, x1 - x0)
    near, far = U._sphere_bounds(cam_pose, obj_diag)
    o = to_decoder_frame(rays_o, obj_diag, family, shapenet_obj_cood, kitti2nusc)
    d = to_decoder_frame(viewdir, obj_diag, family, shapenet_obj_cood, kitti2nusc, direction=True)
    hits = ray_surface(model, o, d, near / scale, far / scale, shapecode, level=level, n_samples=n_samples, refine=refine)
    normal = to_object_frame(hits.normal, obj_diag, family, shapenet_obj_cood, kitti2nusc, direction=True)
    return RayHits((hits.depth * scale).view(shape), hits.state.view(shape), normal.view(*shape, 3), (hits.width * scale).view(shape))


class MeshHits(NamedTuple):
    t: torch.Tensor          # (N,) fp32: the ray parameter of the first hit (units of |rays_d|); +inf on a miss
    face: torch.Tensor       # (N,) int32: the face that was hit, local to the object; -1 on a miss
    weights: torch.Tensor    # (N, 3) fp32: the barycentric weights of the hit in that face; 0 on a miss
    side: torch.Tensor       # (N,) int8: +1 the face was hit from its front (d . n < 0), -1 from its back, 0 on a miss
    point: torch.Tensor      # (N, 3) fp32: rays_o + t rays_d; +inf on a miss
    normal: torch.Tensor     # (N, 3) fp32: the unit geometric normal of the face; 0 on a miss


RAY_CULL = {None: 0, "back": 1, "front": 2}


def _ray_cull(cull):
    if cull not in RAY_CULL:
        raise SnrError(f"cull is None, 'back' or 'front', got {cull!r}")
    return RAY_CULL[cull]


def _mesh_count(meshes):
    """How many meshes the caller passed -- 1 for a single (verts, faces) pair -- before anything else about them is checked."""
    single = isinstance(meshes, (tuple, list)) and len(meshes) == 2 and torch.is_tensor(meshes[0])
    return 1 if single else len(meshes)


def _per_object_rays(rays_o, rays_d, B, names=("rays_o", "rays_d")):
    """Per-object lists of (N, 3) origins and directions: one tensor each with one mesh, else one per object."""
    if torch.is_tensor(rays_o) != torch.is_tensor(rays_d):
        raise SnrError(f"{names[0]} and {names[1]} are both tensors or both lists with one tensor per object")
    if torch.is_tensor(rays_o):
        if B != 1:
            raise SnrError(f"rays are lists of (N, 3) tensors, one per object: {B} meshes")
        rays_o, rays_d = [rays_o], [rays_d]
    rays_o, rays_d = list(rays_o), list(rays_d)
    if len(rays_o) != B or len(rays_d) != B:
        raise SnrError(f"{B} meshes but {len(rays_o)} {names[0]} and {len(rays_d)} {names[1]} tensors")
    for o, d in zip(rays_o, rays_d):
        if o.dim() != 2 or o.shape[1] != 3 or tuple(d.shape) != tuple(o.shape):
            raise SnrError(f"{names[0]} and {names[1]} are (N, 3) per object, got {tuple(o.shape)} and {tuple(d.shape)}")
        _gpu(o, names[0]), _gpu(d, names[1])
    return rays_o, rays_d


def _ray_bounds(v, what, ns, dev):
    """t_min / t_max packed over the objects (sum N,) fp32: a float or a 0-dim tensor for every ray, a (N,) tensor with one mesh, or a
    list with one of those per object."""
    per = list(v) if isinstance(v, (list, tuple)) else [v] * len(ns)
    if len(per) != len(ns):
        raise SnrError(f"{what}: {len(ns)} meshes but {len(per)} values")
    parts = [_ray_bound(x, what, (n,), dev) for x, n in zip(per, ns)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _ray_cast(ms, os_, ds, t_min, t_max, index, cull=None):
    """The packed kernel call of ``ray_mesh`` / ``visible`` (``cull`` a number) or of ``ray_crossings`` (``cull=None``), cut per object."""
    ns = [o.shape[0] for o in os_]
    dev = os_[0].device
    o = os_[0] if len(os_) == 1 else torch.cat([x.detach().float() for x in os_])
    d = ds[0] if len(ds) == 1 else torch.cat([x.detach().float() for x in ds])
    lo, hi = _ray_bounds(t_min, "t_min", ns, dev), _ray_bounds(t_max, "t_max", ns, dev)
    if cull is None:
        out = ops.mesh_raycast_crossings(index.mesh, index.grid, o, d, lo, hi, ns)
    else:
        out = ops.mesh_raycast_first(index.mesh, index.grid, o, d, lo, hi, ns, cull)
    return [tuple(x[q] for x in out) for (q,) in _object_slices(ns)]


def ray_mesh(meshes, rays_o, rays_d, *, t_min=0.0, t_max=float("inf"), cull=None, index=None, face_forward=False):
    """Where each ray rays_o + t rays_d hits its object's mesh first, t_min < t < t_max: ``meshes`` is the list ``extract_mesh`` returns
    with ``rays_o`` and ``rays_d`` lists of (N, 3) tensors, one per object, or one (verts, faces) pair with one tensor each.  The rays
    need not start at a camera and ``rays_d`` need not be unit (t is in units of |rays_d|).  ``t_min`` / ``t_max``: floats, 0-dim tensors
    or per-ray (N,) tensors (with several meshes also a list, one entry per object).  ``cull``: None, "back" (faces seen from behind are
    passed through) or "front".  ``index``: what ``mesh_index`` returned for these meshes.  Returns one ``MeshHits(t, face, weights, side,
    point, normal)`` per object (a single one for a single pair).

    The answer is exact: over all faces of the object the watertight ray/triangle test of Woop, Benthin and Wald in float64, the
    smallest t, ties to the lowest face index (include/supnerf_hip.h, "Mesh ray casting", R1 - R6; ``snr_raycast_first``); the grid only
    prunes, bit for bit.  A ray through a shared edge or vertex hits exactly one of the faces around it; a ray that starts on a face
    does not hit that face at ``t_min = 0``.  ``normal`` is the unit geometric normal (b - a) x (c - a) of the hit face, turned to face
    the ray only with ``face_forward=True``.  Face, weights and side are constants of the graph.  When grad mode is on and ``rays_o``,
    ``rays_d`` or the vertices require grad, ``t`` is formed again in torch from the chosen face as n . (a - o) / (n . d), so autograd
    reaches the rays and the vertices (those of ``extract_mesh(..., differentiable=True)`` carry it on to the shape codes); misses get
    exactly zero.  Otherwise ``t`` is the kernel's float64 value rounded once to fp32.  A mesh cut open by the border of the grid is cast
    as it is: a ray through the opening hits what lies behind it or nothing, and ``side`` = -1 tells a hit from inside.  A ray with a
    non-finite component or a zero direction, and any ray of a mesh without faces, misses.  CPU tensors raise ``SnrError``."""
    c = _ray_cull(cull)
    os_, ds = _per_object_rays(rays_o, rays_d, _mesh_count(meshes))
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    index = _index_for(ms, index)
    out = []
    for (v, f), o, d, (fa, t64, w, side) in zip(ms, os_, ds, _ray_cast(ms, os_, ds, t_min, t_max, index, c)):
        hit = fa >= 0
        live = torch.is_grad_enabled() and (o.requires_grad or d.requires_grad or v.requires_grad)
        o, d = o.float(), d.float()
        if f.shape[0] and v.shape[0]:
            a, b, cc = v.float()[f.long()[fa.clamp(min=0).long()]].unbind(1)
            n = torch.linalg.cross(b - a, cc - a)
        else:
            a = n = torch.zeros_like(o)
        if live:
            nd = torch.where(hit, (n * d).sum(1), torch.ones_like(t64, dtype=torch.float32))
            t = torch.where(hit, (n * (a - o)).sum(1) / nd, torch.full_like(nd, float("inf")))
        else:
            t = t64.float()
        inf3 = torch.full_like(o, float("inf"))
        point = torch.where(hit[:, None], o + torch.where(hit, t, torch.zeros_like(t))[:, None] * d, inf3)
        normal = torch.nn.functional.normalize(n, dim=1)
        if face_forward:
            normal = torch.where((side < 0)[:, None], -normal, normal)
        normal = torch.where(hit[:, None], normal, torch.zeros_like(normal))
        out.append(MeshHits(t, fa, w, side, point, normal))
    return out[0] if single else out


def ray_crossings(meshes, rays_o, rays_d, *, t_min=0.0, t_max=float("inf"), index=None):
    """The faces each ray rays_o + t rays_d crosses with t_min < t < t_max: ``(signed, total)``, (N,) int32 each, per object (lists with
    several meshes, as ``ray_mesh`` takes them).  ``signed`` counts +1 where the ray leaves through a face and -1 where it enters,
    ``total`` counts both as 1.  For a closed mesh wound as ``extract_mesh`` winds it, ``signed`` of a ray to infinity is the winding
    number of its origin, in any direction (``winding_number`` is the case +z); ``total`` is its parity check.  Exact as ``ray_mesh``
    is (R1 - R6; ``snr_raycast_crossings``): a ray through a shared edge or vertex crosses exactly one of the faces around it.  A mesh
    cut open by the border of the grid gets the counts of these rules and no more.  No autograd; CPU tensors raise ``SnrError``."""
    os_, ds = _per_object_rays(rays_o, rays_d, _mesh_count(meshes))
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    out = _ray_cast(ms, os_, ds, t_min, t_max, _index_for(ms, index))
    return out[0] if single else out


def visible(meshes, points, eye, *, offset=0.0, index=None):
    """Whether each point sees ``eye``: a (N,) bool tensor per object, true where no face of the object's mesh is crossed on the open
    segment from the point to the eye.  ``points``: (N, 3) per object as ``closest_point`` takes them; ``eye``: (3,), or (N, 3) with one
    row per point (with several meshes also a list, one entry per object).  It is one first-hit call of ``ray_mesh``'s kernel with
    d = eye - p and t in (offset, 1): ``offset`` is in units of the segment's length (0.01 skips the first hundredth of the way) and
    lifts the start off a noisy surface.  At ``offset = 0`` a point that lies on the surface -- a vertex, say -- is not hidden by its own
    faces, because a ray that starts on a face does not hit that face (R4); a vertex on the silhouette is hidden or not by the edge rule
    R2, the same from run to run.  No autograd; CPU tensors raise ``SnrError``."""
    ms, single = _one_or_many(meshes)
    if not ms:
        return []
    pts = _per_object_points(points, len(ms), single)
    eyes = list(eye) if isinstance(eye, (list, tuple)) else [eye] * len(ms)
    if len(eyes) != len(ms):
        raise SnrError(f"{len(ms)} meshes but {len(eyes)} eyes")
    ds = []
    for p, e in zip(pts, eyes):
        e = _gpu(e, "eye")
        if tuple(e.shape) not in ((3,), tuple(p.shape)):
            raise SnrError(f"eye is (3,) or one row per point {tuple(p.shape)}, got {tuple(e.shape)}")
        ds.append((e.detach().float() - p.detach().float()).contiguous())
    pts = [p.detach() for p in pts]
    out = [r[0] < 0 for r in _ray_cast(ms, pts, ds, float(offset), 1.0, _index_for(ms, index), 0)]
    return out[0] if single else out


def mesh_depth(meshes, cam_pose, obj_diag, K, roi, *, im_sz=None, pixels=None, cull="back", family="a", shapenet_obj_cood=False,
               kitti2nusc=False, index=None):
    """One object's decoder-frame mesh (a (verts, faces) pair) as a camera sees it, in metric units: the mesh twin of ``surface_depth``.
    ``ray_mesh`` on the very rays ``surface_depth`` casts -- ``utils.get_rays`` (a grid over ``roi``, ``im_sz`` x ``im_sz`` steps or one
    per pixel) or ``utils.get_rays_specified`` (``pixels = (x_vec, y_vec)`` in image coordinates: lidar returns), taken to the decoder
    frame with ``to_decoder_frame`` -- from the camera centre to infinity.  ``cam_pose``: the camera in the object's frame (3, 4), on
    the GPU.  Returns ``(depth, hits)``: depth in metres along the unit view direction, +inf where the pixel sees no face, and
    ``MeshHits`` with ``point`` and ``normal`` in the object's metric frame (``to_object_frame``), shaped (H, W[, 3]) for a grid and
    (n[, 3]) for listed pixels.  Unlike ``mesh_view`` nothing is snapped to a pixel grid: the depth is that of the exact ray.  Gradients
    reach ``cam_pose`` through the ray operators and the vertices through ``ray_mesh``."""
    scale = _frame_scale(obj_diag, family)
    _ray_cull(cull)
    if _mesh_count(meshes) != 1 or not torch.is_tensor(meshes[0]):
        raise SnrError("mesh_depth takes one (verts, faces) pair: the mesh of the object the camera pose belongs to")
    ms, _ = _one_or_many(meshes)
    _gpu(cam_pose, "cam_pose")
    if pixels is not None:
        rays_o, viewdir = U.get_rays_specified(K, cam_pose, pixels[0], pixels[1])
        shape = (rays_o.shape[0],)
    else:
        steps = None if im_sz is None else [int(im_sz), int(im_sz)]
        rays_o, viewdir = U.get_rays(K, cam_pose, roi, uv_steps=steps)
        x0, y0, x1, y1 = [int(v) for v in roi]
        shape = (int(im_sz), int(im_sz)) if im_sz is not None else (y1 - y0, x1 - x0)
    o = to_decoder_frame(rays_o, obj_diag, family, shapenet_obj_cood, kitti2nusc).reshape(-1, 3)
    d = to_decoder_frame(viewdir, obj_diag, family, shapenet_obj_cood, kitti2nusc, direction=True).reshape(-1, 3)
    h = ray_mesh(ms[0], o, d, cull=cull, index=index)
    point = to_object_frame(h.point, obj_diag, family, shapenet_obj_cood, kitti2nusc)
    normal = to_object_frame(h.normal, obj_diag, family, shapenet_obj_cood, kitti2nusc, direction=True)
    hits = MeshHits(h.t.view(shape), h.face.view(shape), h.weights.view(*shape, 3), h.side.view(shape), point.view(*shape, 3),
                    normal.view(*shape, 3))
    return (h.t * scale).view(shape), hits


def quantize_colors(colors):
    """(V, 3) colours -> uint8 as ``write_ply`` stores them: round(clamp(c, 0, 1) * 255), half to even; NaN counts as 0."""
    c = np.nan_to_num(np.asarray(torch.as_tensor(colors).detach().cpu().numpy(), dtype=np.float64), nan=0.0)
    return np.rint(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x, y, z per vertex (then float nx, ny, nz with ``normals``, uchar red, green, blue with ``colors``:
    ``quantize_colors``), a uchar-counted int list per triangle."""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    rec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, f
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None or colors is not None:
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        cols = [("x", v[:, 0]), ("y", v[:, 1]), ("z", v[:, 2])]
        if normals is not None:
            n = np.asarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4")
            if n.shape != v.shape:
                raise SnrError(f"normals must be {v.shape}, got {n.shape}")
            fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
            cols += [("nx", n[:, 0]), ("ny", n[:, 1]), ("nz", n[:, 2])]
            props += "property float nx\nproperty float ny\nproperty float nz\n"
        if colors is not None:
            c = quantize_colors(colors)
            if c.shape != v.shape:
                raise SnrError(f"colors must be {v.shape}, got {c.shape}")
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            cols += [("red", c[:, 0]), ("green", c[:, 1]), ("blue", c[:, 2])]
            props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        vrec = np.empty(v.shape[0], dtype=np.dtype(fields))
        for name, col in cols:
            vrec[name] = col
        v = vrec
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\n{props}"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())
