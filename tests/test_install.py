"""The zero-edit boundary: ``supnerf_amd.install()`` makes the reference's named callers pick up the HIP path without an
edited line -- src/optimizer_nuscenes.py:14-21 (``from utils import render_rays_v2 ...``, ``from model_supnerf import SUPNeRF``), :1785
(``SUPNeRF(**hpams['net_hyperparams'])``), :1796 (strict ``load_state_dict``), :603,617 (``encode_img``), :526 (``pose_update``),
src/trainer_unified_nuscenes.py:227-229 (``nn.DataParallel``).

The callers are a stand-in tree written by the test itself: files named like the reference's, with the same public names and layer names
but trivially small bodies -- enough to be recognised and rebound, nothing of the reference's text.  What the reference's own classes build
is pinned by the fixture ``tests/golden/supnerf_layout.json`` (recorded from the reference by ``tests/golden/gen_golden_install.py``): its
nuScenes ``net_hyperparams`` and every state-dict entry of the ``SUPNeRF`` they make, which the stand-in encoder reproduces entry for entry.
"""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------- stand-in tree
STANDIN_MODEL = '''
import torch, torch.nn as nn
class BasicBlock(nn.Module):
    expansion = 1
class ImgEncoder(nn.Module):                      # stand-in for the caller's stock encoder: same call convention, tiny body
    def __init__(self, block, layers, num_classes=128, norm_layer=None, pred_wlh=False):
        super().__init__()
        self.pred_wlh = pred_wlh
        self.conv1 = nn.Conv2d(3, 8, 3, padding=1)
        self.bn1 = (norm_layer or nn.BatchNorm2d)(8)
        self.fc_shape, self.fc_texture, self.fc_pose = nn.Linear(8, num_classes), nn.Linear(8, num_classes), nn.Linear(8, num_classes)
        self.fc_uv = nn.Linear(8, 16)
    def forward(self, x, pose_shortcut=False):
        f = torch.relu(self.bn1(self.conv1(x))).mean((2, 3))
        return self.fc_shape(f), self.fc_texture(f), self.fc_pose(f), self.fc_uv(f)
def _decoder_layers(self, shape_blocks, texture_blocks, W, latent_dim, d_xyz=63, d_dir=27):
    self.shape_blocks, self.texture_blocks, self.num_xyz_freq, self.num_dir_freq = shape_blocks, texture_blocks, 10, 4
    self.encoding_xyz = nn.Sequential(nn.Linear(d_xyz, W), nn.ReLU())
    for j in range(shape_blocks):
        setattr(self, f"shape_latent_layer_{j+1}", nn.Sequential(nn.Linear(latent_dim, W), nn.ReLU()))
        setattr(self, f"shape_layer_{j+1}", nn.Sequential(nn.Linear(W, W), nn.ReLU()))
    self.encoding_shape = nn.Linear(W, W)
    self.sigma = nn.Sequential(nn.Linear(W, 1), nn.Softplus())
    self.encoding_viewdir = nn.Sequential(nn.Linear(W + d_dir, W), nn.ReLU())
    for j in range(texture_blocks):
        setattr(self, f"texture_latent_layer_{j+1}", nn.Sequential(nn.Linear(latent_dim, W), nn.ReLU()))
        setattr(self, f"texture_layer_{j+1}", nn.Sequential(nn.Linear(W, W), nn.ReLU()))
    self.rgb = nn.Sequential(nn.Linear(W, W // 2), nn.ReLU(), nn.Linear(W // 2, 3))
class SUPNeRF(nn.Module):
    def __init__(self, shape_blocks=5, texture_blocks=5, pose_blocks=3, regress_blocks=3, latent_dim=256, pose_dim=16,
                 num_xyz_freq=10, num_dir_freq=4, norm_layer_type='BatchNorm2d', pose_shortcut=False, pred_wlh=False):
        super().__init__()
        self.img_encoder = ImgEncoder(BasicBlock, [3, 4, 6, 3], num_classes=latent_dim, norm_layer=nn.BatchNorm2d, pred_wlh=pred_wlh)
        self.pose_shortcut, self.pred_wlh, self.pose_blocks, self.regress_blocks = pose_shortcut, pred_wlh, pose_blocks, regress_blocks
        _decoder_layers(self, shape_blocks, texture_blocks, latent_dim, latent_dim)
        for j in range(pose_blocks):
            setattr(self, f"pose_layer_{j}", nn.Sequential(nn.Linear(pose_dim if j == 0 else latent_dim, latent_dim), nn.ReLU(inplace=True)))
        for j in range(regress_blocks):
            setattr(self, f"regress_layer_{j}", nn.Sequential(nn.Linear(2 * latent_dim if j == 0 else latent_dim, latent_dim), nn.ReLU(inplace=True)))
        self.out_delta_layer = nn.Linear(latent_dim, 6)
    def encode_img(self, img):
        return (*self.img_encoder(img, self.pose_shortcut), None)
    def pose_update(self, im_feat, box_uv_src):
        f = box_uv_src
        for j in range(self.pose_blocks):
            f = getattr(self, f"pose_layer_{j}")(f)
        d = torch.cat([im_feat, f], -1)
        for j in range(self.regress_blocks):
            d = getattr(self, f"regress_layer_{j}")(d)
        return self.out_delta_layer(d)
    def forward(self, xyz, viewdir, shape_latent, texture_latent):
        raise RuntimeError("stand-in forward: the install did not take")
'''
STANDIN_CODENERF = '''
import torch.nn as nn
from model_supnerf import _decoder_layers
class CodeNeRF(nn.Module):
    def __init__(self, shape_blocks=2, texture_blocks=1, W=256, num_xyz_freq=10, num_dir_freq=4, latent_dim=256):
        super().__init__()
        _decoder_layers(self, shape_blocks, texture_blocks, W, latent_dim)
    def forward(self, xyz, viewdir, shape_latent, texture_latent):
        raise RuntimeError("stand-in forward: the install did not take")
'''
_UTILS_NAMES = ["render_rays", "render_rays_v2", "render_rays_specified", "render_full_img", "render_virtual_imgs", "prepare_pixel_samples",
                "volume_rendering_batch", "volume_rendering2", "volume_rendering", "get_rays", "get_rays_specified", "sample_from_rays",
                "sample_from_rays_v2", "ray_box_intersection", "ray_box_intersection_tensor"]
STANDIN_UTILS = "\n".join(f"def {n}(*a, **k):\n    raise RuntimeError('stand-in {n}: the install did not take')" for n in _UTILS_NAMES) + \
    "\ndef str2bool(v):\n    return str(v).lower() in ('1', 'true', 'yes')\n"
STANDIN_RENDERER = '''
class NeRFRenderer:
    def __init__(self, n_samples=64, noise_std=0.0, white_bkgd=True):
        raise RuntimeError("stand-in NeRFRenderer: the install did not take")
def render_rays_v3(*a, **k):
    raise RuntimeError("stand-in")
def volume_rendering3(*a, **k):
    raise RuntimeError("stand-in")
'''
# the caller: binds the names at import time, exactly the statements of src/optimizer_nuscenes.py:14-21,1785-1796
STANDIN_CALLER = '''
import torch
from utils import render_rays, render_rays_v2, render_rays_specified, render_full_img
from model_codenerf import CodeNeRF
from model_supnerf import SUPNeRF
def make_and_load(hpams, saved):
    model = SUPNeRF(**hpams['net_hyperparams'])
    model.load_state_dict(saved['model_params'])          # strict
    return model
'''
HPAMS = {"net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "pose_blocks": 3, "regress_blocks": 3, "latent_dim": 256,
                             "pose_dim": 16, "num_xyz_freq": 10, "num_dir_freq": 4, "norm_layer_type": "BatchNorm2d",
                             "pose_shortcut": False, "pred_wlh": False}}


def _write_tree(tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    (src / "model_supnerf.py").write_text(STANDIN_MODEL)
    (src / "model_codenerf.py").write_text(STANDIN_CODENERF)
    (src / "utils.py").write_text(STANDIN_UTILS)
    (src / "renderer.py").write_text(STANDIN_RENDERER)
    (src / "caller_optimizer.py").write_text(STANDIN_CALLER)
    return str(src)


@pytest.fixture
def standin_tree(tmp_path):
    """The stand-in ``src/`` on sys.path, and a clean-up that removes its modules and the install afterwards."""
    import supnerf_amd
    src = _write_tree(tmp_path)
    names = ("utils", "renderer", "model_supnerf", "model_codenerf", "caller_optimizer")
    stash = {n: sys.modules.pop(n) for n in names if n in sys.modules}
    sys.path.insert(0, src)
    try:
        yield src
    finally:
        supnerf_amd.uninstall()
        sys.path.remove(src)
        for n in names:
            sys.modules.pop(n, None)
        sys.modules.update(stash)


def _checkpoint_like_the_reference(ref_model_cls):
    """What ``save_models`` writes (src/trainer_unified_nuscenes.py:476-490): the state-dict of a model built by the caller's own class."""
    torch.manual_seed(3)
    m = ref_model_cls(**HPAMS["net_hyperparams"])
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert any(k.startswith("img_encoder.") for k in sd) and any(k.startswith("pose_layer_") for k in sd) \
        and any(k.startswith("regress_layer_") for k in sd)
    return {"model_params": sd}


def test_install_after_the_callers_imports_rebinds_by_identity(standin_tree):
    """The caller module was imported BEFORE install(): its ``from utils import render_rays_v2`` global is re-pointed by identity."""
    import supnerf_amd as A
    import caller_optimizer as C                       # binds the stand-in functions
    import model_supnerf as MS
    import utils as RU
    orig_cls = MS.SUPNeRF
    saved = _checkpoint_like_the_reference(orig_cls)
    rep = A.install()
    assert "utils" in rep["patched"] and "model_supnerf" in rep["patched"] and rep["rebound"] >= 5
    assert RU.render_rays_v2 is A.utils.render_rays_v2 and C.render_rays_v2 is A.utils.render_rays_v2
    assert C.render_rays_specified is A.utils.render_rays_specified and C.render_full_img is A.utils.render_full_img
    assert issubclass(MS.SUPNeRF, orig_cls) and issubclass(MS.SUPNeRF, A.model._DecoderBase) and C.SUPNeRF is MS.SUPNeRF
    model = C.make_and_load(HPAMS, saved)              # constructor of the caller's class, strict load incl. img_encoder.* keys
    assert set(model.state_dict()) == set(saved["model_params"])
    assert type(model.img_encoder).__module__ == "model_supnerf"          # the caller's stock encoder, built by the caller's constructor
    feats = model.encode_img(torch.zeros(2, 3, 8, 8))
    assert len(feats) == 5 and feats[0].shape == (2, 256) and feats[4] is None
    assert model.pose_update(feats[2], torch.zeros(2, 16)).shape == (2, 6)
    assert model.precision == "auto" and model.train_decoder_weights is False and model.last_precision is None
    # the HIP forward is what runs: CPU tensors fail loudly (no CPU fallback) instead of reaching the stand-in's forward
    with pytest.raises(A.SnrError):
        model(torch.zeros(4, 2, 3), torch.zeros(4, 2, 3), torch.zeros(1, 256), torch.zeros(1, 256))
    A.uninstall()
    assert RU.render_rays_v2 is not A.utils.render_rays_v2 and C.render_rays_v2 is RU.render_rays_v2 and MS.SUPNeRF is orig_cls
    assert C.SUPNeRF is orig_cls and not hasattr(RU, "__supnerf_amd_originals__")


def test_install_before_the_callers_imports_uses_the_import_hook(standin_tree):
    """install() first (what ``python -m supnerf_amd.run`` does), imports afterwards: the modules are patched as they load."""
    import supnerf_amd as A
    rep = A.install()
    assert rep["hook"] and rep["patched"] == {}
    import caller_optimizer as C
    import renderer as RR
    assert C.render_rays_v2 is A.utils.render_rays_v2 and C.render_rays is A.utils.render_rays
    assert RR.NeRFRenderer is A.renderer.NeRFRenderer and RR.render_rays_v3 is A.renderer.render_rays_v3
    assert issubclass(C.SUPNeRF, A.model._DecoderBase) and issubclass(C.CodeNeRF, A.model._DecoderBase)
    assert C.SUPNeRF.__supnerf_amd_original__.__module__ == "model_supnerf"
    assert set(A.installed()) >= {"utils", "renderer", "model_supnerf", "model_codenerf"}
    import utils as RU
    assert RU.str2bool("True") is True                 # everything else in the module is the caller's own
    assert A.install()["patched"] == {}                # idempotent
    m = C.CodeNeRF(shape_blocks=3, texture_blocks=1)
    assert isinstance(m, A.model._DecoderBase) and "img_encoder.conv1.weight" not in m.state_dict()


def test_package_supnerf_resolves_the_callers_encoder(standin_tree):
    """``supnerf_amd.SUPNeRF(**net_hyperparams)`` without an ``img_encoder`` builds the caller's ImgEncoder as src/model_supnerf.py:168-175."""
    import supnerf_amd as A
    import model_supnerf as MS
    saved = _checkpoint_like_the_reference(MS.SUPNeRF)
    model = A.SUPNeRF(**HPAMS["net_hyperparams"])
    assert type(model.img_encoder) is MS.ImgEncoder
    model.load_state_dict(saved["model_params"])       # strict
    assert model.encode_img(torch.zeros(1, 3, 8, 8))[1].shape == (1, 256)
    bare = A.SUPNeRF(**HPAMS["net_hyperparams"], img_encoder=False)
    with pytest.raises(A.SnrError):
        bare.encode_img(torch.zeros(1, 3, 8, 8))


def test_package_supnerf_without_any_reference_fails_loudly():
    import supnerf_amd as A
    stash = {n: sys.modules.pop(n) for n in ("model_supnerf", "src.model_supnerf") if n in sys.modules}
    try:
        with pytest.raises(A.SnrError, match="ImgEncoder"):
            A.SUPNeRF(**HPAMS["net_hyperparams"])
    finally:
        sys.modules.update(stash)


def test_launcher_runs_an_unmodified_script(tmp_path):
    """``python -m supnerf_amd.run script.py args`` == install + runpy: the script's own import statements get the HIP names."""
    src = _write_tree(tmp_path)
    script = tmp_path / "optimize_standin.py"
    script.write_text(textwrap.dedent('''
        import sys, os, json
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'src'))
        from caller_optimizer import render_rays_v2, SUPNeRF
        import supnerf_amd
        print(json.dumps({"argv": sys.argv[1:], "main": __name__, "v2": render_rays_v2 is supnerf_amd.utils.render_rays_v2,
                          "cls": issubclass(SUPNeRF, supnerf_amd.model._DecoderBase), "prec": SUPNeRF(shape_blocks=3, texture_blocks=1).precision,
                          "gpu_touched": bool(__import__("torch").cuda.is_initialized())}))
    '''))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "supnerf_amd.run", "--precision", "fp32", str(script), "--gpu", "0"], capture_output=True,
                         text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec == {"argv": ["--gpu", "0"], "main": "__main__", "v2": True, "cls": True, "prec": "fp32", "gpu_touched": False}


# ---------------------------------------------------------------------------------------------------------------- the reference's layout
# fixture supnerf_layout.json (tests/golden/gen_golden_install.py): the reference's nuScenes net_hyperparams and every state-dict entry of
# the SUPNeRF they build.  The stand-in encoder below carries exactly the recorded img_encoder.* entries, so a checkpoint of the recorded
# layout loads strictly into the stand-in caller's class, the installed class and the package's own SUPNeRF.
LAYOUT = os.path.join(ROOT, "tests", "golden", "supnerf_layout.json")
STANDIN_LAYOUT_ENCODER = '''
import json as _json
import torch.nn.functional as _F
_ENC = [e for e in _json.load(open(LAYOUT_PATH))["state_dict"] if e[0].startswith("img_encoder.")]
class ImgEncoder(nn.Module):                      # the recorded encoder's entries; a forward through its four heads only
    def __init__(self, block, layers, num_classes=128, norm_layer=None, pred_wlh=False):
        super().__init__()
        self.pred_wlh = pred_wlh
        for name, shape, dtype, kind in _ENC:
            *path, leaf = name[len("img_encoder."):].split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            t = torch.randn(shape) * 0.01 if dtype == "float32" else torch.zeros(shape, dtype=getattr(torch, dtype))
            if kind == "parameter":
                mod.register_parameter(leaf, nn.Parameter(t))
            else:
                mod.register_buffer(leaf, t)
    def forward(self, x, pose_shortcut=False):
        head = lambda m, f: _F.linear(_F.pad(f, (0, m.weight.shape[1] - f.shape[1])), m.weight, m.bias)
        f = x.mean((2, 3))
        pose = head(self.fc_pose, f)
        return head(self.fc_shape, f), head(self.fc_texture, f), pose, head(self.fc_uv, pose)
'''


def _checkpoint_of_the_recorded_layout(layout):
    """What the reference's ``save_models`` writes for ``SUPNeRF(**net_hyperparams)``: every recorded entry, recorded shape and dtype."""
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.randn(shape, generator=g) * 0.05 if dtype == "float32" else torch.zeros(shape, dtype=getattr(torch, dtype)))
          for k, shape, dtype, _ in layout["state_dict"]}
    return {"model_params": sd}


def test_reference_layout_callers_run_with_zero_edits(standin_tree):
    """With the reference's own recorded configuration and checkpoint layout: install(), ``SUPNeRF(**hpams['net_hyperparams'])`` from its
    nuScenes json, strict load of a state-dict of ITS layout (img_encoder.*, pose_layer_*, regress_layer_* keys) into the installed class and
    into the package's own SUPNeRF, ``encode_img`` / ``pose_update`` through the caller's modules, and the import hook."""
    import supnerf_amd as A
    layout = json.load(open(LAYOUT))
    hp = {"net_hyperparams": layout["net_hyperparams"]}
    with open(os.path.join(standin_tree, "model_supnerf.py"), "w") as f:
        f.write(STANDIN_MODEL + STANDIN_LAYOUT_ENCODER.replace("LAYOUT_PATH", repr(LAYOUT)))
    saved = _checkpoint_of_the_recorded_layout(layout)
    sd = saved["model_params"]
    enc_keys = sum(k.startswith("img_encoder.") for k in sd)
    pose_keys = sum(k.startswith(("pose_layer_", "regress_layer_", "out_delta_layer")) for k in sd)
    assert enc_keys > 100 and pose_keys >= 14 and len(sd) > enc_keys + pose_keys
    # (1) the caller's modules imported FIRST, like a script that imports supnerf_amd late
    import utils as RU
    import model_supnerf as MS
    import model_codenerf as MC
    import renderer as RR
    orig_v2, orig_cls = RU.render_rays_v2, MS.SUPNeRF
    orig_cls(**hp["net_hyperparams"]).load_state_dict(sd)          # strict: the stand-in caller builds exactly the recorded layout
    rep = A.install()
    assert set(rep["patched"]) == {"utils", "renderer", "model_supnerf", "model_codenerf"}, rep
    assert RU.render_rays_v2 is A.utils.render_rays_v2
    assert all(getattr(RU, n) is getattr(A.utils, n) for n in ("render_rays", "render_rays_specified", "render_full_img", "render_virtual_imgs",
                                                                "prepare_pixel_samples", "volume_rendering_batch", "volume_rendering2"))
    assert RR.NeRFRenderer is A.renderer.NeRFRenderer and RR.render_rays_v3 is A.renderer.render_rays_v3
    assert RR.volume_rendering3 is A.renderer.volume_rendering3
    model = MS.SUPNeRF(**hp["net_hyperparams"])                      # src/optimizer_nuscenes.py:1785
    model.load_state_dict(sd)                                          # :1796, strict
    assert isinstance(model, A.model._DecoderBase) and isinstance(model, orig_cls)
    assert type(model.img_encoder).__module__ + "." + type(model.img_encoder).__name__ == "model_supnerf.ImgEncoder"
    model.eval()
    with torch.no_grad():
        feats = model.encode_img(torch.zeros(*layout["encode_img_input"]))          # :603,617
        assert [None if t is None else list(t.shape) for t in feats] == layout["encode_img_shapes"]
        assert list(model.pose_update(feats[2], torch.zeros(1, 16)).shape) == layout["pose_update_shape"]      # :526
    with pytest.raises(A.SnrError):                                    # the HIP forward: CPU tensors fail loudly
        model(torch.zeros(4, 2, 3), torch.zeros(4, 2, 3), torch.zeros(1, 256), torch.zeros(1, 256))
    # supnerf_amd.SUPNeRF itself resolves the caller's encoder and has the reference's layout entry for entry
    m2 = A.SUPNeRF(**hp["net_hyperparams"])
    m2.load_state_dict(sd)
    assert type(m2.img_encoder) is MS.ImgEncoder
    assert {k: list(v.shape) for k, v in m2.state_dict().items()} == {k: shape for k, shape, _, _ in layout["state_dict"]}
    assert issubclass(MC.CodeNeRF, A.model._DecoderBase)
    # nn.DataParallel wraps it like src/trainer_unified_nuscenes.py:227-229 (construction + state-dict only)
    assert set(k[len("module."):] for k in torch.nn.DataParallel(model).state_dict()) == set(sd)
    A.uninstall()
    assert RU.render_rays_v2 is orig_v2 and MS.SUPNeRF is orig_cls
    # (2) a module imported AFTER install() goes through the hook
    for n in ("utils", "renderer", "model_supnerf", "model_codenerf"):
        sys.modules.pop(n, None)
    A.install()
    import utils as RU2
    from model_supnerf import SUPNeRF as S2
    assert RU2.render_rays_v2 is A.utils.render_rays_v2 and issubclass(S2, A.model._DecoderBase) and RU2 is not RU


# ---------------------------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_installed_callers_render_the_references_numbers(standin_tree, golden, oracle_params, precision):
    """The whole zero-edit route on the card: the caller module binds names at import, install() re-points them, the model is built by
    ``SUPNeRF(**hpams['net_hyperparams'])`` and strictly loaded from a checkpoint that carries img_encoder.* / pose keys, wrapped in
    ``nn.DataParallel`` like the trainer does, and ``render_rays_v2`` called through the CALLER's global gives the reference's own
    numbers (fixture ``render_a_nusc``, made by the imported reference) with gradients to codes and pose."""
    import numpy as np
    import supnerf_amd as A
    import caller_optimizer as C
    import model_supnerf as MS
    dev = torch.device("cuda:0")
    saved = _checkpoint_like_the_reference(MS.SUPNeRF)
    for k, v in oracle_params.items():                  # the decoder the fixture was rendered with; encoder / pose keys stay the checkpoint's
        assert saved["model_params"][k].shape == v.shape
        saved["model_params"][k] = v.clone()
    A.install()
    model = C.make_and_load(HPAMS, saved).to(dev)
    model.precision = precision
    g = golden("render_a_nusc")
    A.utils.JITTER_OVERRIDE = g["jitter"]
    try:
        sc, tc = g["shapecode"].to(dev).requires_grad_(), g["texturecode"].to(dev).requires_grad_()
        pose = g["cam_pose"].to(dev).requires_grad_()
        out = C.render_rays_v2(model, dev, g["img"], g["mask_occ"], pose, np.float32(g["obj_diag"]), g["K"], g["roi"], int(g["n_samples"]), sc, tc,
                               int(g["shapenet_obj_cood"]), 0, im_sz=int(g["im_sz"]))
        (out[0].sum() + out[2].sum()).backward()
    finally:
        A.utils.JITTER_OVERRIDE = None
    md = lambda a, b: float((a.detach().cpu().double() - b.double()).abs().max())
    assert md(out[0], g["rgb"]) < 5e-5 and md(out[1], g["depth"]) < 2e-4 and md(out[2], g["acc"]) < 5e-5
    assert sc.grad is not None and tc.grad is not None and pose.grad is not None and float(sc.grad.abs().sum()) > 0
    assert model.last_precision is not None and model.last_precision["forward"] in ("fp32", "bf16x3")
    # the decoder module itself, entered the way ParallelModel.forward does under nn.DataParallel (src/trainer_unified_nuscenes.py:120-123,227-229)
    dp = torch.nn.DataParallel(model, device_ids=[0])
    xyz = (torch.rand(64, 32, 3, device=dev) - 0.5)
    vd = torch.nn.functional.normalize(torch.randn(64, 32, 3, device=dev), dim=-1)
    with torch.no_grad():
        sig, rgb = dp(xyz, vd, g["shapecode"].to(dev), g["texturecode"].to(dev))
    from oracle import supnerf_oracle as O
    s_ref, c_ref = O.decoder_forward(oracle_params, xyz.cpu(), vd.cpu(), g["shapecode"], g["texturecode"])
    assert md(sig, s_ref) < 2e-5 and md(rgb, c_ref) < 2e-5
    # the pose head and the encoder are the caller's stock modules, on the GPU
    feats = model.encode_img(torch.zeros(2, 3, 8, 8, device=dev))
    assert model.pose_update(feats[2], torch.zeros(2, 16, device=dev)).shape == (2, 6)
