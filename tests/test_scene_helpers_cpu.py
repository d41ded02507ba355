"""CPU tests of the host-side helpers between the object poses and the scene kernels, each stated once: ``utils.invert_pose``,
``scene.corners_of_box_batch`` with its cached sign table, ``scene.roi_pixels``, and the roi ``scene.scene_ray_rows`` takes from
``scene.scene_rois`` for float64 poses with a manipulation."""
import pytest
import torch

import scene_rows_restatement as R
from oracle_bands import amd  # noqa: F401  (a fixture)


@pytest.fixture(scope="module")
def scene(golden):
    return golden("scene")


# ------------------------------------------------------------------------------------------------ invert_pose
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_invert_pose_is_the_restatement_and_the_other_spelling(amd, scene, dtype):
    poses = scene["obj_poses"].to(dtype)
    got = amd.utils.invert_pose(poses)
    assert got.dtype == dtype and got.shape == poses.shape
    assert torch.equal(got, R.cam2obj_of(poses))
    Rt = poses[:, :, :3].transpose(1, 2)
    assert torch.equal(got, torch.cat([Rt, (-Rt) @ poses[:, :, 3:]], dim=2))       # negation is exact: at most the sign of a zero differs


def test_invert_pose_shapes(amd, scene):
    poses = scene["obj_poses"].double()                                             # (Nb,3,4)
    Nb = poses.shape[0]
    stack = torch.stack([poses, poses.flip(0)])                                     # (T,Nb,3,4)
    one, batch, table = amd.utils.invert_pose(poses[1]), amd.utils.invert_pose(poses), amd.utils.invert_pose(stack)
    assert one.shape == (3, 4) and batch.shape == (Nb, 3, 4) and table.shape == (2, Nb, 3, 4)
    assert torch.equal(one, batch[1]) and torch.equal(table[0], batch) and torch.equal(table[1], batch.flip(0))
    # twice is the identity, for a rotation that is orthogonal to float64 rounding (the fixture's is to fp32 rounding only)
    P = torch.cat([amd.driver.axis_angle_to_matrix(torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64)), poses[0, :, 3:]], dim=1)
    assert float((amd.utils.invert_pose(amd.utils.invert_pose(P)) - P).abs().max()) < 1e-12


def test_invert_pose_gradcheck(amd, scene):
    poses = scene["obj_poses"][:2].double().clone().requires_grad_()
    assert torch.autograd.gradcheck(amd.utils.invert_pose, (poses,))


# ------------------------------------------------------------------------------------------------ corners_of_box_batch
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_corners_are_the_literal_corners(amd, scene, dtype):
    """The eight corners (+-l/2, +-w/2, +-h/2) in nuScenes order (x forward, y left, z up), R @ c + t."""
    poses, wlh = scene["obj_poses"][:3].to(dtype), scene["obj_wlh"][:3].to(dtype)
    assert poses.shape[0] == 3
    want = []
    for P, (w, l, h) in zip(poses, wlh):
        c = torch.stack([torch.stack([l / 2, w / 2, h / 2]), torch.stack([l / 2, -(w / 2), h / 2]), torch.stack([l / 2, -(w / 2), -(h / 2)]),
                         torch.stack([l / 2, w / 2, -(h / 2)]), torch.stack([-(l / 2), w / 2, h / 2]), torch.stack([-(l / 2), -(w / 2), h / 2]),
                         torch.stack([-(l / 2), -(w / 2), -(h / 2)]), torch.stack([-(l / 2), w / 2, -(h / 2)])], dim=1)        # (3,8)
        want.append(P[:, :3] @ c + P[:, 3:])
    got = amd.scene.corners_of_box_batch(poses, wlh)
    assert got.dtype == dtype and got.shape == (3, 3, 8)
    assert torch.equal(got, torch.stack(want))


def test_corners_sign_table_is_made_once(amd, scene):
    poses, wlh = scene["obj_poses"].float(), scene["obj_wlh"].float()
    cache = amd.scene._BOX_SIGNS
    amd.scene.corners_of_box_batch(poses, wlh)
    n, table = len(cache), cache[(wlh.device, torch.float32)]
    amd.scene.corners_of_box_batch(poses, wlh)
    amd.scene.scene_rois(poses, wlh, scene["K"], int(scene["H"]), int(scene["W"]))
    assert len(cache) == n and cache[(wlh.device, torch.float32)] is table
    amd.scene.corners_of_box_batch(poses.double(), wlh.double())
    assert (wlh.device, torch.float64) in cache and len(cache) >= 2
    assert cache[(wlh.device, torch.float64)].dtype == torch.float64


# ------------------------------------------------------------------------------------------------ roi_pixels
H_, W_ = 6, 8
ROI_CASES = {
    "one": [[2, 1, 5, 4]],
    "two_overlapping": [[1, 1, 4, 4], [3, 2, 7, 5]],
    "right_and_bottom_edge": [[5, 3, W_ - 1, H_ - 1]],                      # exclusive upper bounds: the last row and column stay uncovered
    "dead_x": [[2, 1, 5, 4], [3, 0, 3, 5]],                                # x1 == x0
    "dead_y_live_x": [[2, 1, 5, 4], [0, 5, 7, 4]],                         # y1 < y0, x range live
    "all_dead": [[3, 0, 3, 5], [0, 5, 7, 4], [4, 2, 2, 2]],
}


@pytest.mark.parametrize("name", list(ROI_CASES))
def test_roi_pixels_against_a_loop_over_all_pixels(amd, name):
    rois = torch.tensor(ROI_CASES[name], dtype=torch.int32)
    want = [[x, y] for y in range(H_) for x in range(W_)                    # row-major
            if any(x1 > x0 and y1 > y0 and x0 <= x < x1 and y0 <= y < y1 for x0, y0, x1, y1 in ROI_CASES[name])]
    got = amd.scene.roi_pixels(rois, H_, W_)
    assert got.dim() == 2 and got.shape[1] == 2 and not got.dtype.is_floating_point
    assert got.tolist() == want                                             # the set and its order
    if name == "all_dead":
        assert got.shape == (0, 2)
    else:
        assert got.shape[0] > 0
    if name == "right_and_bottom_edge":
        assert int(got[:, 0].max()) == W_ - 2 and int(got[:, 1].max()) == H_ - 2
    if name in ("dead_x", "dead_y_live_x"):
        assert got.tolist() == amd.scene.roi_pixels(rois[:1], H_, W_).tolist()


# ------------------------------------------------------------------------------------------------ the roi of scene_ray_rows
MANIPULATION = (0.3, -0.1, 0.5)


@pytest.mark.parametrize("rend_aabb", [True, False])
def test_scene_ray_rows_float64_roi_is_scene_rois_of_the_manipulated_poses(amd, scene, rend_aabb):
    """float64 poses with a manipulation: the manipulation is added in float64, then the poses are cast to fp32 for the roi."""
    g = scene
    H, W = int(g["H"]), int(g["W"])
    poses = g["obj_poses"].double()
    moved = poses.clone()
    moved[:, :, 3] += torch.tensor(MANIPULATION, dtype=torch.float64)
    rois = amd.scene.scene_rois(moved.float(), g["obj_wlh"], g["K"], H, W)
    # precondition: on this fixture "add in float64, then cast" and "cast, then add in fp32" give the same rois, all live and not all alike
    assert torch.equal(rois, amd.scene.scene_rois(poses.float(), g["obj_wlh"], g["K"], H, W, MANIPULATION))
    assert bool(((rois[:, 2] > rois[:, 0]) & (rois[:, 3] > rois[:, 1])).all())
    assert not torch.equal(rois, amd.scene.scene_rois(poses.float(), g["obj_wlh"], g["K"], H, W))
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    rows, _ = amd.scene.scene_ray_rows(poses, g["obj_wlh"], g["K"], pixels, H, W, MANIPULATION, rend_aabb)
    assert rows.dtype == torch.float64
    px, py = pixels[:, 0:1], pixels[:, 1:2]
    in_roi = (px >= rois[:, 0]) & (px < rois[:, 2]) & (py >= rois[:, 1]) & (py < rois[:, 3])          # (Nr,Nb)
    assert torch.equal(~(rows == -1).all(-1), in_roi)
    assert 0 < int(in_roi.sum()) < in_roi.numel()
