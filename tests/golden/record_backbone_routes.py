"""Record which path the forward of every backbone takes over a grid of inputs and switch settings, for
tests/test_backbone_route_host.py:

    PYTHONPATH=. python tests/golden/record_backbone_routes.py tests/golden/backbone_routes.json
    (from the root of a checkout of the commit to record -- this file itself may come from a later one -- on a machine with the
    device)

The forwards are run with _forward_nhwc_train / _forward_nhwc_infer and the first step of the module sequence replaced by stubs
that say which one was reached, so no backbone kernel is launched; the device is needed only because the gates of the recorded
commit read `x.is_cuda`.  The networks stay on the CPU (no gate reads their device) and the folded copies are made before
anything has asked their sources for a route.

backbone_routes.json was recorded from commit 4a58d79 (the seven hand-written gates, before backbone_route replaced them).  It
must never be recorded from the tree it is used to test."""
import itertools
import json
import sys
from unittest import mock

import torch
import torch.nn as nn

MODELS = ("resnet18", "resnet50", "CIFAR_ResNet18", "densenet121", "densenet161", "CIFAR_DenseNet121")
FOLDED = ("resnet18", "CIFAR_ResNet18", "densenet121")              # fold_batchnorm copies, recorded as "<name>+fold"
SWITCHES = ("NHWC_TRAINING", "RESNET_NHWC_TRAINING", "CIFAR_DENSENET_NHWC_TRAINING", "NHWC_INFERENCE")
AXES = {"training": (True, False), "grad": (True, False), "device_type": ("cuda", "cpu"), "dtype": ("float32", "float16")}
SHAPES = ((2, 3, 32, 32), (2, 1, 32, 32), (3, 32, 32))
DENSE_SHAPE = (2, 3, 36, 36)        # maps 36 -> 18 -> 9: odd in front of the second transition
LETTER = {"nhwc_train": "t", "nhwc_infer": "i", "modules": "m"}


def shapes_of(name):
    return SHAPES + ((DENSE_SHAPE,) if "dense" in name.lower() else ())


def inputs_of(name):
    """The inputs of one network in the order of its route string: (training, grad, device_type, dtype name, shape)."""
    return list(itertools.product(*AXES.values(), shapes_of(name)))


def switch_settings():
    """Every assignment of the switches, as (key, {name: value}): key "1011" = the values in the order of SWITCHES."""
    for vals in itertools.product((True, False), repeat=len(SWITCHES)):
        yield "".join("1" if v else "0" for v in vals), dict(zip(SWITCHES, vals))


def build_models(backbones):
    torch.manual_seed(0)
    models = {name: getattr(backbones, name)() for name in MODELS}
    with mock.patch.object(backbones, "NHWC_INFERENCE", False):
        models.update({name + "+fold": backbones.fold_batchnorm(models[name]) for name in FOLDED})
    return models


class _Reached(Exception):
    pass


def _stub(route):
    def reached(*args, **kwargs):
        raise _Reached(route)
    return reached


def record():
    from nwhead_amd import ops
    from nwhead_amd.model import backbones
    models = build_models(backbones)
    patches = [mock.patch.object(cls, "_forward_nhwc_train", _stub("nhwc_train"))
               for cls in (backbones.ResNet, backbones.CIFAR_ResNet, backbones.DenseNet, backbones.CIFAR_DenseNet)]
    patches += [mock.patch.object(cls, "_forward_nhwc_infer", _stub("nhwc_infer")) for cls in (backbones.CIFAR_ResNet, backbones.DenseNet)]
    # the module sequence begins with the stem convolution, DenseNet's `features` or the folded ResNets' fused stem
    patches += [mock.patch.object(cls, "forward", _stub("modules")) for cls in (nn.Conv2d, backbones.ConvBiasAct, nn.Sequential)]
    patches.append(mock.patch.object(ops, "stem_conv_relu_maxpool_nhwc", _stub("modules")))
    patches.append(mock.patch.object(backbones.ConvBiasAct, "_split_weight", _stub("modules")))      # (that call's argument)
    routes = {}
    for p in patches:
        p.start()
    try:
        for name, model in models.items():
            routes[name] = {}
            for key, setting in switch_settings():
                with mock.patch.multiple(backbones, **setting):
                    out = []
                    for training, grad, device_type, dtype, shape in inputs_of(name):
                        model.train(training)
                        x = torch.zeros(shape, dtype=getattr(torch, dtype), device=device_type)
                        try:
                            with torch.set_grad_enabled(grad):
                                model(x)
                            raise AssertionError("a forward reached no stub")
                        except _Reached as e:
                            out.append(LETTER[str(e)])
                    routes[name][key] = "".join(out)
    finally:
        for p in patches:
            p.stop()
    return routes


if __name__ == "__main__":
    table = {"switches": SWITCHES, "axes": [[k, v] for k, v in AXES.items()], "shapes": {name: shapes_of(name) for name in MODELS},
             "routes": record()}
    with open(sys.argv[1], "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
