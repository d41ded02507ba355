#!/usr/bin/env python3
"""Fixture ``supnerf_layout.json`` for tests/test_install.py, taken from the reference (needs a checkout of it):

    python tests/golden/gen_golden_install.py REFERENCE_CHECKOUT

Records what a checkpoint written by the reference's ``SUPNeRF(**hpams['net_hyperparams'])`` looks like: the ``net_hyperparams`` of
``jsonfiles/supnerf.nusc.vehicle.car.json``, every state-dict entry of the model they build (name, shape, dtype, parameter or buffer),
and the shapes ``encode_img`` / ``pose_update`` return.  The reference's ``cv2`` / ``torchvision`` imports get inert stand-ins
(torchvision's public ``BasicBlock``), as in the reference's own environment the encoder is that ResNet.  Data only: names and numbers."""
import json
import os
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub_imports():
    sys.modules["cv2"] = types.ModuleType("cv2")
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvm, tvr = types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")

    class Resize:
        def __init__(self, size):
            self.size = size

        def __call__(self, x):
            return F.interpolate(x, size=self.size, mode="bilinear", align_corners=False)

    def conv3x3(i, o, stride=1, groups=1, dilation=1):
        return nn.Conv2d(i, o, 3, stride, dilation, groups=groups, bias=False, dilation=dilation)

    def conv1x1(i, o, stride=1):
        return nn.Conv2d(i, o, 1, stride, bias=False)

    class BasicBlock(nn.Module):                   # torchvision's residual block (public API)
        expansion = 1

        def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
            super().__init__()
            norm_layer = norm_layer or nn.BatchNorm2d
            self.conv1, self.bn1 = conv3x3(inplanes, planes, stride), norm_layer(planes)
            self.relu = nn.ReLU(inplace=True)
            self.conv2, self.bn2 = conv3x3(planes, planes), norm_layer(planes)
            self.downsample, self.stride = downsample, stride

        def forward(self, x):
            idt = x if self.downsample is None else self.downsample(x)
            return self.relu(self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x))))) + idt)

    class Bottleneck(BasicBlock):
        expansion = 4

    tvt.Resize = Resize
    tvr.BasicBlock, tvr.Bottleneck, tvr.conv1x1, tvr.conv3x3 = BasicBlock, Bottleneck, conv1x1, conv3x3
    tv.transforms, tv.models, tvm.resnet = tvt, tvm, tvr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.models": tvm, "torchvision.models.resnet": tvr})


def main(ref):
    _stub_imports()
    sys.path.insert(0, os.path.join(ref, "src"))
    import model_supnerf as MS
    hp = json.load(open(os.path.join(ref, "jsonfiles", "supnerf.nusc.vehicle.car.json")))["net_hyperparams"]
    torch.manual_seed(0)
    model = MS.SUPNeRF(**hp).eval()
    params = {n for n, _ in model.named_parameters()}
    entries = [[k, list(v.shape), str(v.dtype).replace("torch.", ""), "parameter" if k in params else "buffer"]
               for k, v in model.state_dict().items()]
    with torch.no_grad():
        feats = model.encode_img(torch.zeros(1, 3, 64, 64))
        delta = model.pose_update(feats[2], torch.zeros(1, 16))
    out = {"source": "jsonfiles/supnerf.nusc.vehicle.car.json net_hyperparams; state_dict of src/model_supnerf.py SUPNeRF(**net_hyperparams)",
           "net_hyperparams": hp, "state_dict": entries,
           "encode_img_shapes": [None if t is None else list(t.shape) for t in feats], "encode_img_input": [1, 3, 64, 64],
           "pose_update_shape": list(delta.shape)}
    path = os.path.join(HERE, "supnerf_layout.json")
    with open(path, "w") as f:      # one state-dict entry per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: " + (json.dumps(v) if k != "state_dict" else
                                    "[\n" + ",\n".join(json.dumps(e) for e in v) + "\n]") for k, v in out.items()) + "\n}\n")
    print(f"{len(entries)} state-dict entries -> {path}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
