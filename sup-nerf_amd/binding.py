"""``supnerf_amd.install()`` -- switch the reference's own modules to the MI355X path with ZERO edited lines in the caller.

The reference has no plugin layer: its drivers bind the hot path by name, ``sys.path.insert(0, 'src')`` (optimize_nuscenes.py:1-3) and
then ``from utils import render_rays, render_rays_v2, render_rays_specified, render_full_img, ...`` (src/optimizer_nuscenes.py:14-18,
src/optimizer_kitti.py:13-16, src/optimizer_waymo.py:13-16), ``from utils import ... prepare_pixel_samples, volume_rendering_batch``
(src/trainer_unified_nuscenes.py:14-15, src/data_nuscenes.py:18-19), ``from model_supnerf import SUPNeRF`` (src/optimizer_nuscenes.py:21),
``from src.renderer import volume_rendering3, render_rays_v3`` (scripts/demo.py:16).  ``install()`` rebinds exactly those names:

  * in the caller's ``utils`` / ``src.utils``: the render functions and their building blocks -> ``supnerf_amd.utils``;
  * in ``renderer`` / ``src.renderer``: ``NeRFRenderer``, ``render_rays_v3``, ``volume_rendering3`` -> ``supnerf_amd.renderer``;
  * in ``model_supnerf`` / ``model_codenerf`` / ``model_autorf``: ``SUPNeRF`` / ``CodeNeRF`` / ``AutoRFMix`` -> the reference's OWN class
    with this package's HIP ``forward`` grafted on (``model.hip_decoder_class``): its constructor builds the stock ``ImgEncoder`` as
    src/model_supnerf.py:168-175 does, the state-dict is the reference's key for key (strict ``load_state_dict`` of
    src/optimizer_nuscenes.py:1796 passes), ``encode_img`` / ``pose_update`` stay stock PyTorch;
  * in ``trainer_unified_nuscenes`` / ``trainer_nerf_nuscenes`` (train_nuscenes.py:9-10; recognised as the modules that define an
    ``nn.Module`` named ``ParallelModel``): ``ParallelModel`` -> a subclass of the reference's own class (``training_wrapper_class``) whose
    constructor runs the original and then sets ``train_decoder_weights = True`` on the decoder it wraps
    (src/trainer_unified_nuscenes.py:227-229), so that the trainers' ``loss_total.mean().backward()`` reaches the 28 decoder tensors their
    AdamW steps (:414-421).  ``nn.DataParallel`` replicas copy the flag with their shallow ``__dict__`` copy.

The reference's optimisers (src/optimizer_nuscenes.py:1762-1769) keep the decoder a constant: its weights still ``requires_grad``, but their
AdamW holds codes and pose only.  A trainer that is NOT recognised would step a decoder that never receives a gradient, silently; while
installed, one global ``torch.optim`` step pre-hook raises ``SnrError`` instead, before the step changes anything, when the stepping optimizer
holds a decoder weight that a constant-decoder forward (``train_decoder_weights`` False, grad mode) saw requiring a gradient and whose
``grad`` is None (or, seen through an ``nn.DataParallel`` replica, only the zeros ``Broadcast.backward`` fills in).  The message names the
parameter; the fix is ``model.train_decoder_weights = True``.

Modules that are already imported are patched in place, and every module that did ``from utils import render_rays_v2`` BEFORE the
install is re-pointed too (its global is the original function object: found by identity).  Modules that are imported LATER are patched
as they load, through one ``sys.meta_path`` hook -- so ``python -m supnerf_amd.run optimize_nuscenes.py ...`` (``run.py``) installs first
and then runs the unmodified script.  ``uninstall()`` restores everything.  Nothing of the reference is stored in this package: classes and
functions are looked up in the caller's modules at run time.
"""
import importlib
import importlib.abc
import sys
import threading
import types

import torch.nn as nn
from torch.optim.optimizer import register_optimizer_step_pre_hook

from . import model as M
from . import renderer as R
from . import utils as U
from ._lib import SnrError

# what is rebound, by the KIND of reference module (recognised by content, under whichever name the caller imported it)
UTILS_NAMES = ("render_rays", "render_rays_v2", "render_rays_specified", "render_full_img", "render_virtual_imgs", "prepare_pixel_samples",
               "volume_rendering_batch", "volume_rendering2", "volume_rendering", "get_rays", "get_rays_specified", "get_rays_srn",
               "sample_from_rays", "sample_from_rays_v2", "ray_box_intersection", "ray_box_intersection_tensor")
RENDERER_NAMES = ("NeRFRenderer", "render_rays_v3", "volume_rendering3")
DECODER_CLASSES = ("SUPNeRF", "CodeNeRF", "AutoRFMix")
TRAINER_CLASS = "ParallelModel"
# module names the reference's scripts use for its files (top-level after sys.path.insert(0, 'src'), or through the src package)
TARGET_MODULES = tuple(p + n for n in ("utils", "renderer", "model_supnerf", "model_codenerf", "model_autorf", "trainer_unified_nuscenes",
                                       "trainer_nerf_nuscenes") for p in ("", "src."))

_ORIG = "__supnerf_amd_originals__"
_LOCK = threading.RLock()
_state = {"hook": None, "step_hook": None, "patched": [], "rebound": []}


def _kind(mod):
    d = getattr(mod, "__dict__", {})
    if "render_rays_v2" in d and "volume_rendering2" in d and "get_rays" in d:
        return "utils"
    if "NeRFRenderer" in d and "volume_rendering3" in d:
        return "renderer"
    if any(isinstance(d.get(c), type) and hasattr(d[c], "forward") for c in DECODER_CLASSES):
        return "model"
    return None


def _trainer_class(mod):
    """The reference's own ``ParallelModel`` if ``mod`` defines one (src/trainer_unified_nuscenes.py:19, src/trainer_nerf_nuscenes.py:18),
    else None.  Independent of ``_kind``: trainer_unified_nuscenes also holds ``SUPNeRF`` and is a "model" importer as well."""
    c = getattr(mod, "__dict__", {}).get(TRAINER_CLASS)
    if isinstance(c, type) and issubclass(c, nn.Module) and c.__module__ == getattr(mod, "__name__", None):
        return c.__dict__.get("__supnerf_amd_original__", c)
    return None


_WRAPPERS = {}


def training_wrapper_class(ref_cls):
    """A subclass of the reference's ``ParallelModel`` whose constructor runs the original one and then, if the ``model`` it received (the
    reference's first parameter, src/trainer_unified_nuscenes.py:20) is one of this package's decoders, sets ``train_decoder_weights = True``
    on it: the reference's trainers differentiate the decoder weights and step them.  Any other model (a stock ``nn.Module``, ``None``) is
    left alone.  Built from the caller's class object at run time, like ``model.hip_decoder_class``; nothing of the reference is stored."""
    hit = _WRAPPERS.get(ref_cls)
    if hit is not None:
        return hit

    def __init__(self, *args, **kwargs):
        ref_cls.__init__(self, *args, **kwargs)
        model = kwargs["model"] if "model" in kwargs else (args[0] if args else None)
        if isinstance(model, M._DecoderBase):
            model.train_decoder_weights = True

    cls = type(ref_cls.__name__, (ref_cls,), {
        "__init__": __init__, "__module__": ref_cls.__module__, "__qualname__": ref_cls.__qualname__,
        "__doc__": f"{ref_cls.__module__}.{ref_cls.__name__} that trains a supnerf_amd decoder (supnerf_amd.binding.training_wrapper_class).",
        "__supnerf_amd_original__": ref_cls})
    _WRAPPERS[ref_cls] = cls
    return cls


def _step_pre_hook(optimizer, args, kwargs):
    """Global ``torch.optim`` step pre-hook while installed (module docstring): raise before a step over a decoder weight that a constant-
    decoder forward left without a gradient.  Per step: one membership test per parameter of the optimizer."""
    runs = M._CONSTANT_RUNS
    if not runs:
        return None
    held = [p for group in optimizer.param_groups for p in group["params"] if id(p) in runs]
    for p in held:
        ref, name, via_replica = runs.get(id(p), (None, None, False))
        if ref is not None and ref() is p and (p.grad is None or via_replica):
            raise SnrError(f"supnerf_amd: {type(optimizer).__name__}.step() would update the decoder parameter '{name}' "
                           f"{tuple(p.shape)}, which has no gradient: the decoder ran as a constant (model.train_decoder_weights is "
                           "False), so it would never train.  Set model.train_decoder_weights = True before the forward to train the "
                           "decoder, or leave the decoder's weights out of the optimizer to optimise codes / poses only.")
    for p in held:                  # seen by a step: "since the last step" starts again for these
        runs.pop(id(p), None)
    return None


def _is_ours(mod):
    return getattr(mod, "__name__", "").split(".")[0] == "supnerf_amd"


def patch_module(mod):
    """Rebind the hot-path names of ONE reference module (see the module docstring).  Returns {name: (original, replacement)}; a module
    that is not one of the reference's files named above (or is this package's own) is left alone."""
    if mod is None or _is_ours(mod):
        return {}
    kind, trainer = _kind(mod), _trainer_class(mod)
    if kind is None and trainer is None:
        return {}
    with _LOCK:
        saved = mod.__dict__.setdefault(_ORIG, {})
        done = {}

        def rebind(name, new):
            old = mod.__dict__[name]
            if old is new:
                return
            saved.setdefault(name, old)
            setattr(mod, name, new)
            done[name] = (saved[name], new)

        if kind == "utils":
            for n in UTILS_NAMES:
                if n in mod.__dict__ and hasattr(U, n):
                    rebind(n, getattr(U, n))
        elif kind == "renderer":
            for n in RENDERER_NAMES:
                if n in mod.__dict__:
                    rebind(n, getattr(R, n))
        elif kind == "model":
            for n in DECODER_CLASSES:
                c = mod.__dict__.get(n)
                # only a class this module DEFINES: optimizer_*.py also hold ``SUPNeRF`` as an imported name (re-pointed by identity below)
                if isinstance(c, type) and c.__module__ == mod.__name__ and not issubclass(c, M._DecoderBase):
                    rebind(n, M.hip_decoder_class(c))
        if trainer is not None:
            rebind(TRAINER_CLASS, training_wrapper_class(trainer))
        if done and mod not in _state["patched"]:
            _state["patched"].append(mod)
        return done


def _rebind_importers(pairs):
    """``from utils import render_rays_v2`` executed before the install left the ORIGINAL object in the importer's globals: re-point every
    such global (found by identity, in every loaded module)."""
    by_id = {id(old): (old, new) for old, new in pairs}
    n = 0
    for mod in list(sys.modules.values()):
        d = getattr(mod, "__dict__", None)
        if not isinstance(d, dict) or _is_ours(mod):
            continue
        for name, val in list(d.items()):
            if name == _ORIG:
                continue
            hit = by_id.get(id(val))
            if hit is not None and hit[0] is val:
                d[name] = hit[1]
                _state["rebound"].append((mod, name, val))
                n += 1
    return n


class _PatchLoader(importlib.abc.Loader):
    """Runs the module's real loader, then ``patch_module`` (and re-points earlier importers of what it just replaced)."""

    def __init__(self, inner):
        self._inner = inner

    def create_module(self, spec):
        return self._inner.create_module(spec) if hasattr(self._inner, "create_module") else None

    def exec_module(self, module):
        self._inner.exec_module(module)
        done = patch_module(module)
        if done:
            _rebind_importers(list(done.values()))

    def __getattr__(self, name):            # get_source, get_filename, is_package ... of the wrapped loader
        return getattr(self._inner, name)


class _PatchFinder(importlib.abc.MetaPathFinder):
    """First on ``sys.meta_path``: finds the real spec of a target module with the finders behind it and wraps its loader."""

    def find_spec(self, fullname, path=None, target=None):
        if fullname not in TARGET_MODULES:
            return None
        for finder in sys.meta_path:
            if finder is self or not hasattr(finder, "find_spec"):
                continue
            spec = finder.find_spec(fullname, path, target)
            if spec is not None:
                if spec.loader is not None and hasattr(spec.loader, "exec_module") and not isinstance(spec.loader, _PatchLoader):
                    spec.loader = _PatchLoader(spec.loader)
                return spec
        return None


def install(model_module=None, utils_module=None, renderer_module=None, *, extra_modules=(), import_now=False, hook=True):
    """Switch the reference's modules to the HIP path (module docstring).  The three module arguments name the caller's
    ``model_supnerf`` / ``utils`` / ``renderer`` modules explicitly (module objects or names); by default every one of the reference's
    module names that is already in ``sys.modules`` is patched, and -- ``hook=True`` -- every one imported later.  ``import_now=True``
    additionally imports ``utils``, ``renderer``, ``model_supnerf``, ``model_codenerf`` right away (they must be on ``sys.path``).
    Returns a report: {"patched": {module name: [names]}, "rebound": n, "hook": bool}.  Idempotent."""
    with _LOCK:
        mods = []
        for m in (model_module, utils_module, renderer_module, *extra_modules):
            if m is not None:
                mods.append(importlib.import_module(m) if isinstance(m, str) else m)
        if import_now:
            for name in ("utils", "renderer", "model_supnerf", "model_codenerf"):
                if name not in sys.modules and ("src." + name) not in sys.modules:
                    mods.append(importlib.import_module(name))
        mods += [sys.modules[n] for n in TARGET_MODULES if n in sys.modules]
        report, pairs = {}, []
        seen = set()
        for mod in mods:
            if id(mod) in seen or not isinstance(mod, types.ModuleType):
                continue
            seen.add(id(mod))
            done = patch_module(mod)
            if done:
                report[mod.__name__] = sorted(done)
                pairs += list(done.values())
        n = _rebind_importers(pairs) if pairs else 0
        if hook and _state["hook"] is None:
            _state["hook"] = _PatchFinder()
            sys.meta_path.insert(0, _state["hook"])
        if _state["step_hook"] is None:
            M._CONSTANT_RUNS = {}
            _state["step_hook"] = register_optimizer_step_pre_hook(_step_pre_hook)
        return {"patched": report, "rebound": n, "hook": _state["hook"] is not None}


def uninstall():
    """Undo ``install``: restore every rebound name and remove the import hook and the optimizer step hook."""
    with _LOCK:
        if _state["hook"] is not None and _state["hook"] in sys.meta_path:
            sys.meta_path.remove(_state["hook"])
        _state["hook"] = None
        if _state["step_hook"] is not None:
            _state["step_hook"].remove()
            _state["step_hook"] = None
        M._CONSTANT_RUNS = None
        for mod, name, old in reversed(_state["rebound"]):
            mod.__dict__[name] = old
        _state["rebound"].clear()
        for mod in _state["patched"]:
            for name, old in mod.__dict__.get(_ORIG, {}).items():
                setattr(mod, name, old)
            mod.__dict__.pop(_ORIG, None)
        _state["patched"].clear()


def installed():
    """{module name: [rebound names]} of what is currently switched over."""
    return {m.__name__: sorted(m.__dict__.get(_ORIG, {})) for m in _state["patched"]}
