"""Training under ``supnerf_amd.install()`` with zero edited lines: the reference's trainers (src/trainer_unified_nuscenes.py,
src/trainer_nerf_nuscenes.py, driven by train_nuscenes.py) wrap the decoder in ``nn.DataParallel(ParallelModel(model, hpams))`` (:227-229),
call ``loss_total.mean().backward()`` (:334) and step an ``AdamW`` over ``model.parameters()`` (:414-421).  The install rebinds their
``ParallelModel`` so that the decoder it wraps trains (``train_decoder_weights``); a trainer it does not recognise gets an ``SnrError`` from
``optimizer.step()`` instead of a decoder that silently never moves.

The trainer modules here are stand-ins written by the test, next to the stand-in tree of tests/test_install.py: the reference's module and
class names, tiny bodies.  Their ``ParallelModel.forward`` is the NeRF half of the trainer's (decoder -> ``volume_rendering_batch`` ->
masked rgb and occupancy losses per object), the quantity ``oracle.training_losses`` restates.
"""
import os
import sys

import pytest
import torch

from test_install import HPAMS, _write_tree

TRAINER_HPAMS = dict(HPAMS, loss_occ_coef=0.1, lr=1e-3)

_PARALLEL_MODEL_FORWARD = '''
    def forward(self, shapecode_batch, texturecode_batch, xyz_batch, viewdir_batch, z_vals_batch, rgb_tgt_batch, occ_pixels_batch):
        sigmas, rgbs = self.model(xyz_batch.flatten(0, 1), viewdir_batch.flatten(0, 1), shapecode_batch, texturecode_batch)
        b = xyz_batch.shape[0]
        n, s, _ = sigmas.shape
        rgb_rays, _, acc = volume_rendering_batch(sigmas.view(b, n // b, s, -1), rgbs.view(b, n // b, s, -1), z_vals_batch)
        a = occ_pixels_batch.abs()
        denom = a.sum(dim=[-2, -1]) + 1e-9
        loss_rgb = ((rgb_rays - rgb_tgt_batch) ** 2 * a).sum(dim=[-2, -1]) / denom
        loss_occ = (torch.exp(-occ_pixels_batch * (0.5 - acc.unsqueeze(-1))) * a).sum(dim=[-2, -1]) / denom
        return loss_rgb.mean() + self.hpams["loss_occ_coef"] * loss_occ.mean()
'''
STANDIN_TRAINER_UNIFIED = '''
import torch
import torch.nn as nn
from utils import volume_rendering_batch
from model_supnerf import SUPNeRF
class ParallelModel(nn.Module):
    def __init__(self, model=None, hpams=None, im_enc_rate=1.0, pred_wlh: bool = False):
        super().__init__()
        self.model, self.hpams, self.im_enc_rate, self.pred_wlh = model, hpams, im_enc_rate, pred_wlh
''' + _PARALLEL_MODEL_FORWARD + '''
class TrainerUnifiedNuscenes:
    def __init__(self, hpams, device, gpus=1):
        self.hpams, self.device = hpams, device
        self.model = SUPNeRF(**hpams["net_hyperparams"]).to(device)
        self.parallel_model = nn.DataParallel(ParallelModel(self.model, hpams), device_ids=list(range(gpus)))
        self.opts = torch.optim.AdamW([{"params": self.model.parameters(), "lr": hpams["lr"]}])
'''
STANDIN_TRAINER_NERF = '''
import torch
import torch.nn as nn
from utils import volume_rendering_batch
from model_codenerf import CodeNeRF
class ParallelModel(nn.Module):
    def __init__(self, model=None, hpams=None, im_enc_rate=1.0):
        super().__init__()
        self.model, self.hpams, self.im_enc_rate = model, hpams, im_enc_rate
''' + _PARALLEL_MODEL_FORWARD

TRAINERS = ("trainer_unified_nuscenes", "trainer_nerf_nuscenes")
_MODULES = ("utils", "renderer", "model_supnerf", "model_codenerf", "caller_optimizer", "src") + TRAINERS + tuple("src." + n for n in TRAINERS)


@pytest.fixture
def trainer_tree(tmp_path):
    """The stand-in ``src/`` of tests/test_install.py plus the two trainer modules, importable top-level (``src/`` on sys.path, as
    train_nuscenes.py:1-3 arranges) and as ``src.<name>`` (its parent on sys.path, as train_nuscenes.py:9-10 imports them)."""
    import supnerf_amd
    src = _write_tree(tmp_path)
    with open(os.path.join(src, "trainer_unified_nuscenes.py"), "w") as f:
        f.write(STANDIN_TRAINER_UNIFIED)
    with open(os.path.join(src, "trainer_nerf_nuscenes.py"), "w") as f:
        f.write(STANDIN_TRAINER_NERF)
    stash = {n: sys.modules.pop(n) for n in _MODULES if n in sys.modules}
    sys.path[0:0] = [src, str(tmp_path)]
    try:
        yield src
    finally:
        supnerf_amd.uninstall()
        supnerf_amd.model.DEFAULT_PRECISION = "auto"
        for p in (src, str(tmp_path)):
            sys.path.remove(p)
        for n in _MODULES:
            sys.modules.pop(n, None)
        sys.modules.update(stash)


def _import_trainer(name, prefix, install_first):
    import importlib
    import supnerf_amd as A
    if install_first:
        A.install()
        return importlib.import_module(prefix + name)
    mod = importlib.import_module(prefix + name)
    rep = A.install()
    assert (prefix + name) in rep["patched"] and "ParallelModel" in rep["patched"][prefix + name], rep
    return mod


def _global_step_pre_hooks():
    from torch.optim.optimizer import _global_optimizer_pre_hooks
    return list(_global_optimizer_pre_hooks.values())


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("install_first", [True, False], ids=["install_first", "import_first"])
@pytest.mark.parametrize("prefix", ["", "src."], ids=["top_level", "src_package"])
def test_unified_trainer_trains_the_decoder(trainer_tree, prefix, install_first):
    """``ParallelModel(SUPNeRF(**hpams['net_hyperparams']), hpams)`` from the trainer module turns the decoder's training mode on."""
    import supnerf_amd as A
    T = _import_trainer("trainer_unified_nuscenes", prefix, install_first)
    orig = T.ParallelModel.__supnerf_amd_original__
    assert issubclass(T.ParallelModel, orig) and T.ParallelModel is not orig and orig.__module__ == prefix + "trainer_unified_nuscenes"
    assert issubclass(T.SUPNeRF, A.model._DecoderBase)              # the module is a "model" importer as well: its SUPNeRF is the HIP class
    model = T.SUPNeRF(**HPAMS["net_hyperparams"])
    assert model.train_decoder_weights is False
    pm = T.ParallelModel(model, TRAINER_HPAMS)
    assert model.train_decoder_weights is True and pm.model is model and pm.hpams is TRAINER_HPAMS
    m2 = T.SUPNeRF(**HPAMS["net_hyperparams"])
    T.ParallelModel(model=m2, hpams=TRAINER_HPAMS, im_enc_rate=0.5)  # (keyword form)
    assert m2.train_decoder_weights is True


@pytest.mark.parametrize("install_first", [True, False], ids=["install_first", "import_first"])
@pytest.mark.parametrize("prefix", ["", "src."], ids=["top_level", "src_package"])
def test_nerf_trainer_trains_the_decoder(trainer_tree, prefix, install_first):
    import supnerf_amd as A
    T = _import_trainer("trainer_nerf_nuscenes", prefix, install_first)
    assert issubclass(T.CodeNeRF, A.model._DecoderBase)
    model = T.CodeNeRF(shape_blocks=3, texture_blocks=1)
    T.ParallelModel(model, TRAINER_HPAMS)
    assert model.train_decoder_weights is True


def test_other_models_are_left_alone(trainer_tree):
    """A stock module, or none at all, passes through the rebound ParallelModel untouched."""
    import supnerf_amd as A
    A.install()
    import trainer_unified_nuscenes as T
    plain = torch.nn.Linear(2, 2)
    pm = T.ParallelModel(plain, TRAINER_HPAMS)
    assert pm.model is plain and not hasattr(plain, "train_decoder_weights")
    assert T.ParallelModel().model is None


def test_optimiser_models_stay_constant(trainer_tree):
    """The optimisers' model (src/optimizer_nuscenes.py:1785) keeps the decoder a constant, with the trainers imported alongside."""
    import supnerf_amd as A
    A.install()
    import trainer_unified_nuscenes  # noqa: F401
    import trainer_nerf_nuscenes  # noqa: F401
    import caller_optimizer as C
    import model_supnerf as MS
    saved = {"model_params": MS.SUPNeRF(**HPAMS["net_hyperparams"]).state_dict()}
    model = C.make_and_load(HPAMS, saved)
    assert isinstance(model, A.model._DecoderBase) and model.train_decoder_weights is False


def test_uninstall_restores_the_trainers(trainer_tree):
    import supnerf_amd as A
    import trainer_unified_nuscenes as TU
    import src.trainer_nerf_nuscenes as TN
    originals = (TU.ParallelModel, TN.ParallelModel)
    before = _global_step_pre_hooks()
    A.install()
    assert TU.ParallelModel is not originals[0] and TN.ParallelModel is not originals[1]
    assert len(_global_step_pre_hooks()) == len(before) + 1
    assert set(A.installed()) >= {"trainer_unified_nuscenes", "src.trainer_nerf_nuscenes"}
    A.install()                                                            # idempotent: one hook, one wrapper class
    assert len(_global_step_pre_hooks()) == len(before) + 1
    A.uninstall()
    assert (TU.ParallelModel, TN.ParallelModel) == originals
    assert _global_step_pre_hooks() == before and A.model._CONSTANT_RUNS is None
    model = A.CodeNeRF(shape_blocks=3, texture_blocks=1)            # (the package's own decoder: the original ParallelModel leaves it be)
    TU.ParallelModel(model, TRAINER_HPAMS)
    assert model.train_decoder_weights is False


def test_step_hook_logic(trainer_tree):
    """The safety net on the host: what a constant-decoder forward notes (``_note_decoder_run``, called by ``forward`` / ``fused_render``)
    and what the step hook makes of it.  The launches themselves are exercised on the GPU below."""
    import supnerf_amd as A
    A.install()
    import model_supnerf as MS
    model = MS.SUPNeRF(**HPAMS["net_hyperparams"])
    names = {n for n, _ in model.named_parameters()}
    codes = torch.zeros(2, 256, requires_grad=True)

    def constant_forward():
        model._note_decoder_run(constant=True)
        codes.sum().backward()

    with torch.no_grad():                                   # no gradient recorded, nothing noted
        model._note_decoder_run(constant=True)
    torch.optim.AdamW(model.parameters()).step()
    constant_forward()                                      # the optimisers' shape: codes only
    torch.optim.AdamW([codes]).step()
    opt = torch.optim.AdamW(model.parameters(), lr=1.0)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(A.SnrError, match=r"decoder parameter '(\w+\.)+(weight|bias)'.*train_decoder_weights = True") as e:
        opt.step()
    assert str(e.value).split("'")[1] in names
    assert all(torch.equal(p, before[n]) for n, p in model.named_parameters())
    with pytest.raises(A.SnrError):                         # still refused: the note stays until a step passes
        opt.step()
    model.train_decoder_weights = True                      # a training-mode forward drops the notes
    model._note_decoder_run(constant=False)
    opt.step()
    model.train_decoder_weights = False
    constant_forward()
    A.uninstall()
    opt.step()                                              # uninstalled: today's behaviour


# ---------------------------------------------------------------------------------------------------------------- GPU
DECODER_REL = 2e-4             # of each tensor's largest entry (+ 1e-7 absolute), as tests/test_driver_gpu.py holds the training step


def _batch(dev, B=2, n=64, S=64, seed=31):
    g = torch.Generator().manual_seed(seed)
    b = dict(sc=torch.randn(B, 256, generator=g) * 0.3, tc=torch.randn(B, 256, generator=g) * 0.3,
             xyz=torch.rand(B, n, S, 3, generator=g) - 0.5,
             vd=torch.nn.functional.normalize(torch.randn(B, n, 1, 3, generator=g), dim=-1).repeat(1, 1, S, 1),
             z=torch.sort(torch.rand(B, S, generator=g) * 4 + 9, dim=-1)[0], rgb=torch.rand(B, n, 3, generator=g),
             occ=(torch.randint(0, 3, (B, n, 1), generator=g) - 1).float())
    return {k: v.to(dev) for k, v in b.items()}


def _args(b, codes=None, objs=slice(None)):
    sc, tc = codes if codes is not None else (b["sc"], b["tc"])
    return tuple(t[objs] for t in (sc, tc, b["xyz"], b["vd"], b["z"], b["rgb"], b["occ"]))


def _trainer(oracle_params, precision, dev):
    """The stand-in trainer, installed, its decoder loaded with the oracle's weights; ``precision`` as ``run.py --precision`` sets it."""
    import supnerf_amd as A
    A.model.DEFAULT_PRECISION = precision
    A.install()
    import trainer_unified_nuscenes as T
    tr = T.TrainerUnifiedNuscenes(TRAINER_HPAMS, dev)
    with torch.no_grad():
        for k, v in oracle_params.items():
            tr.model.get_parameter(k).copy_(v)
    return T, tr


def _decoder(model, names):
    return {k: model.get_parameter(k) for k in names}


def _grads(params):
    return {k: p.grad.detach().clone() for k, p in params.items()}


def _zero(model, *extra):
    model.zero_grad(set_to_none=True)
    for t in extra:
        t.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_zero_edit_training_step(trainer_tree, oracle_params, precision):
    """The trainer's step with no attribute edit: every decoder tensor receives its gradient (mask-matched against the oracle's autograd
    in float64) and the trainer's AdamW moves all 28."""
    from oracle import supnerf_oracle as O
    from relu_bits import relu_bits_of
    dev = torch.device("cuda:0")
    T, tr = _trainer(oracle_params, precision, dev)
    dec = _decoder(tr.model, oracle_params)
    assert len(dec) == 28
    b = _batch(dev)
    seen = {}

    def keep_masks(module, inputs, out):                   # (read before backward frees what the operator saved; returns None)
        seen["masks"] = relu_bits_of(out[0], 3, 1)
    hook = tr.model.register_forward_hook(keep_masks)
    loss = tr.parallel_model(*_args(b))
    hook.remove()
    loss.mean().backward()
    missing = [k for k, p in dec.items() if p.grad is None or not bool(p.grad.abs().sum() > 0)]
    assert not missing, f"decoder tensors without a gradient: {missing}"
    p64 = {k: v.double().requires_grad_() for k, v in oracle_params.items()}
    c = {k: v.detach().cpu().double() for k, v in b.items()}
    with O.given_relu_masks(seen["masks"]):
        ref = O.training_losses(p64, c["xyz"], c["vd"], c["sc"], c["tc"], c["z"], c["rgb"], c["occ"], TRAINER_HPAMS["loss_occ_coef"])[0]
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    worst = 0.0
    for k, p in dec.items():
        want = p64[k].grad
        err = float((p.grad.cpu().double() - want).abs().max())
        worst = max(worst, err / float(want.abs().max()))
        assert err <= DECODER_REL * float(want.abs().max()) + 1e-7, (k, err, float(want.abs().max()))
    print(f"[zero-edit step, {precision}] worst decoder gradient entry, relative to its tensor's largest: {worst:.2e}")
    before = {k: p.detach().clone() for k, p in dec.items()}
    tr.opts.step()
    assert not [k for k, p in dec.items() if torch.equal(p, before[k])]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_replica_backward_reaches_the_source(trainer_tree, oracle_params, precision):
    """Forward + backward through ``torch.nn.parallel.replicate`` (what ``nn.DataParallel`` runs on two or more devices): the replica's
    weights are ``Broadcast`` outputs, not leaves, and the gradients reach the source parameters through ``Broadcast.backward``."""
    from torch.nn.parallel import gather, parallel_apply, replicate
    dev = torch.device("cuda:0")
    T, tr = _trainer(oracle_params, precision, dev)
    pm = tr.parallel_model.module
    dec = _decoder(tr.model, oracle_params)
    b = _batch(dev)
    sc, tc = b["sc"].clone().requires_grad_(), b["tc"].clone().requires_grad_()
    # the direct call
    pm(*_args(b, (sc, tc))).backward()
    direct, direct_codes = _grads(dec), (sc.grad.clone(), tc.grad.clone())
    # one replica: the same launches, so the same bits (Broadcast.backward on one device hands the gradients on unchanged)
    _zero(tr.model, sc, tc)
    rep = replicate(pm, [0])[0]
    assert rep.model._is_replica and not rep.model.encoding_xyz[0].weight.is_leaf and rep.model.train_decoder_weights
    rep(*_args(b, (sc, tc))).backward()
    for k, p in dec.items():
        assert torch.equal(p.grad, direct[k]), k
    assert torch.equal(sc.grad, direct_codes[0]) and torch.equal(tc.grad, direct_codes[1])
    # two replicas on one device, one object each, in two threads: the sum of the two halves' direct gradients
    _zero(tr.model, sc, tc)
    for o in range(2):
        pm(*_args(b, (sc, tc), slice(o, o + 1))).backward()
    halves = _grads(dec)
    _zero(tr.model, sc, tc)
    try:
        reps = replicate(pm, [0, 0])
    except Exception as e:                                  # noqa: BLE001
        pytest.skip(f"this torch refuses two replicas on one device: {type(e).__name__}: {e}")
    outs = parallel_apply(reps, [_args(b, (sc, tc), slice(o, o + 1)) for o in range(2)], devices=[0, 0])
    gather([o.reshape(1) for o in outs], 0).sum().backward()
    for k, p in dec.items():
        err = float((p.grad - halves[k]).abs().max()) / float(halves[k].abs().max())
        assert err <= 1e-6, (k, err)


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: nn.DataParallel over devices 0 and 1")
def test_dataparallel_two_devices_matches_one(trainer_tree, oracle_params):
    """A real ``nn.DataParallel(ParallelModel, device_ids=[0, 1])`` step (one thread per device; the split forward's LDS grant on device 1)
    against the single-device step."""
    dev = torch.device("cuda:0")
    T, tr = _trainer(oracle_params, "auto", dev)
    pm = tr.parallel_model.module
    dec = _decoder(tr.model, oracle_params)
    b = _batch(dev)
    pm(*_args(b)).backward()
    one = _grads(dec)
    _zero(tr.model)
    torch.nn.DataParallel(pm, device_ids=[0, 1])(*_args(b)).mean().backward()
    for k, p in dec.items():
        err = float((p.grad - one[k]).abs().max()) / float(one[k].abs().max())
        assert err <= 1e-5, (k, err)


def _plain_training_step(model, b, codes, opt, replica=False):
    """An unrecognised trainer: a plain function, its own forward, an AdamW over the model's parameters and the codes, the flag never set.
    Through a replica it also differentiates the pose head, the way the reference's forward differentiates its encoder: ``Broadcast.backward``
    then hands the decoder weights zeros instead of None."""
    import supnerf_amd as A
    from torch.nn.parallel import replicate
    m = replicate(model, [b["xyz"].device.index])[0] if replica else model
    B, n, S = b["xyz"].shape[:3]
    sig, rgb = m(b["xyz"].flatten(0, 1), b["vd"].flatten(0, 1), *codes)
    rgb_rays, _, acc = A.utils.volume_rendering_batch(sig.view(B, n, S, 1), rgb.view(B, n, S, 3), b["z"])
    loss = ((rgb_rays - b["rgb"]) ** 2).mean() + acc.mean()
    if replica:
        loss = loss + 1e-3 * m.pose_update(codes[0], codes[0][:, :16]).square().mean()
    loss.backward()
    opt.step()


@pytest.mark.gpu
def test_unrecognised_trainer_fails_loudly(trainer_tree):
    """The safety net on the card: an unrecognised trainer is refused before its step changes anything (directly and through a
    replica); the optimisers' shape (AdamW over codes and pose, decoder ``requires_grad`` left on) and a model with the flag set step."""
    import supnerf_amd as A
    dev = torch.device("cuda:0")
    A.install()
    import model_supnerf as MS
    model = MS.SUPNeRF(**HPAMS["net_hyperparams"]).to(dev)
    b = _batch(dev)
    names = {n for n, _ in model.named_parameters()}
    sc, tc = b["sc"].clone().requires_grad_(), b["tc"].clone().requires_grad_()
    for replica in (False, True):
        opt = torch.optim.AdamW(list(model.parameters()) + [sc, tc], lr=1e-3)
        before = {n: p.detach().clone() for n, p in list(model.named_parameters()) + [("sc", sc), ("tc", tc)]}
        with pytest.raises(A.SnrError, match="train_decoder_weights = True") as e:
            _plain_training_step(model, b, (sc, tc), opt, replica=replica)
        assert str(e.value).split("'")[1] in names, str(e.value)
        assert all(torch.equal(p, before[n]) for n, p in list(model.named_parameters()) + [("sc", sc), ("tc", tc)]), replica
        _zero(model, sc, tc)
    # the reference optimisers' shape: codes and pose in the AdamW, the decoder left requiring grad
    pose = torch.zeros(2, 6, device=dev, requires_grad=True)
    opt = torch.optim.AdamW([sc, tc, pose], lr=1e-2)
    assert all(p.requires_grad for p in model.parameters())
    sig, rgb = model((b["xyz"] + pose[:, None, None, 3:]).flatten(0, 1), b["vd"].flatten(0, 1), sc, tc)
    (sig.mean() + rgb.mean()).backward()
    sc0, pose0 = sc.detach().clone(), pose.detach().clone()
    opt.step()
    assert not torch.equal(sc, sc0) and not torch.equal(pose, pose0)
    # the flag set: the decoder trains, and the same plain trainer steps
    _zero(model, sc, tc)
    model.train_decoder_weights = True
    w0 = model.encoding_xyz[0].weight.detach().clone()
    _plain_training_step(model, b, (sc, tc), torch.optim.AdamW(list(model.parameters()) + [sc, tc], lr=1e-3))
    assert not torch.equal(model.encoding_xyz[0].weight, w0)
