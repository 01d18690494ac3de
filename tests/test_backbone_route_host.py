"""Host tests of what nwhead_amd/model/backbones.py decides in front of its launches: which path a forward takes
(backbone_route), what fold_batchnorm's copy starts with, the eval-mode BatchNorm fold's arithmetic, the weight bank of the
training forward and the inference plans' cache.  No device: nothing here launches a kernel."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn as nn

from nwhead_amd import ops
from nwhead_amd.model import backbones as bb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("record_backbone_routes", os.path.join(GOLDEN, "record_backbone_routes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def models():
    return rec.build_models(bb)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "backbone_routes.json")) as fh:
        return json.load(fh)


def test_route_table_is_the_grid_of_the_recorder(table):
    assert tuple(table["switches"]) == rec.SWITCHES
    assert [(k, tuple(v)) for k, v in table["axes"]] == list(rec.AXES.items())
    assert {k: tuple(map(tuple, v)) for k, v in table["shapes"].items()} == {k: rec.shapes_of(k) for k in rec.MODELS}
    assert set(table["routes"]) == set(rec.MODELS) | {k + "+fold" for k in rec.FOLDED}
    keys = {k for k, _ in rec.switch_settings()}
    for name, by_switch in table["routes"].items():
        assert set(by_switch) == keys
        assert all(len(s) == len(rec.inputs_of(name)) for s in by_switch.values())


@pytest.mark.parametrize("name", rec.MODELS + tuple(k + "+fold" for k in rec.FOLDED))
def test_backbone_route_decides_what_the_hand_written_gates_decided(name, models, table, monkeypatch):
    """backbone_route against the recorded decisions of the commit before it (tests/golden/record_backbone_routes.py): every
    network, train / eval x grad / no-grad x device x dtype x shape, under every assignment of the four switches."""
    model = models[name]
    for key, setting in rec.switch_settings():
        for sw, val in setting.items():
            monkeypatch.setattr(bb, sw, val)
        want = table["routes"][name][key]
        for (training, grad, device_type, dtype, shape), letter in zip(rec.inputs_of(name), want):
            got = bb.backbone_route(model, device_type=device_type, dtype=getattr(torch, dtype), shape=shape, grad=grad,
                                    training=training)
            assert rec.LETTER[got] == letter, (name, key, training, grad, device_type, dtype, shape, got)
            if name.endswith("+fold") or name == "densenet161":     # (by the code: a stem with a bias; a growth of 48)
                assert got == "modules"
    seen = set("".join(table["routes"][name].values()))
    if name in ("resnet18", "resnet50", "CIFAR_DenseNet121"):
        assert seen == set("tm")
    elif name in ("CIFAR_ResNet18", "densenet121"):
        assert seen == set("tim")
    else:
        assert seen == set("m")


def test_backbone_route_reads_training_from_the_model_and_for_reads_the_batch(models, monkeypatch):
    net = models["CIFAR_ResNet18"]
    facts = dict(device_type="cuda", dtype=torch.float32, shape=(2, 3, 32, 32))
    net.train()
    assert bb.backbone_route(net, grad=True, **facts) == "nhwc_train"
    net.eval()
    assert bb.backbone_route(net, grad=False, **facts) == "nhwc_infer"
    assert bb.backbone_route(net, grad=False, training=True, **facts) == "modules"
    assert bb.backbone_route(nn.Conv2d(3, 8, 3), grad=False, **facts) == "modules"
    x = torch.zeros(2, 3, 32, 32)
    seen = []
    monkeypatch.setattr(bb, "backbone_route", lambda model, **kw: seen.append(kw) or "modules")
    with torch.no_grad():
        assert bb.backbone_route_for(net, x) == "modules"
    assert seen == [dict(device_type="cpu", dtype=torch.float32, shape=x.shape, grad=False)]
    # DenseNet's maps: 36 -> 18 -> 9 is odd in front of the second transition, 64 halves cleanly
    dnet = models["densenet121"].eval()
    monkeypatch.undo()
    assert bb.backbone_route(dnet, grad=False, device_type="cuda", dtype=torch.float32, shape=(2, 3, 64, 64)) == "nhwc_infer"
    assert bb.backbone_route(dnet, grad=False, device_type="cuda", dtype=torch.float32, shape=(2, 3, 36, 36)) == "modules"
    assert bb.backbone_route(dnet, grad=False, device_type="cuda", dtype=torch.float32, shape=None) == "nhwc_infer"


def test_fold_batchnorm_copy_starts_without_the_routes_state(monkeypatch):
    """The structural answer, the weight bank and the inference plan are kept on the network; fold_batchnorm's deep copy must
    not inherit them: its modules are rewritten (a stem with a bias, Identity BatchNorms), so a True from the source is wrong."""
    monkeypatch.setattr(bb, "NHWC_INFERENCE", False)       # so that all three are rewritten
    state = ("_nw_nhwc_ok", "_nw_bank", "_nw_infer_plan")
    for make in (bb.CIFAR_ResNet18, bb.resnet18, bb.densenet121):
        src = make()
        assert bb._nhwc_structure(src) is True and src._nw_nhwc_ok is True
        src._nw_bank, src._nw_infer_plan = object(), {"sig": None}
        inner = next(m for m in src.modules() if m is not src)
        inner._nw_bank = object()                            # (wherever it sits)
        copy = bb.fold_batchnorm(src)
        stem = copy.features.conv0 if isinstance(copy, bb.DenseNet) else copy.conv1
        assert isinstance(stem, bb.ConvBiasAct) and stem.bias is not None
        for m in copy.modules():
            assert not any(hasattr(m, k) for k in state), (type(m).__name__, [k for k in state if hasattr(m, k)])
        assert bb._nhwc_structure(copy) is False
        assert bb.backbone_route(copy, device_type="cuda", dtype=torch.float32, shape=(2, 3, 32, 32), grad=False) == "modules"
        assert all(hasattr(src, k) for k in state) and src._nw_nhwc_ok is True and hasattr(inner, "_nw_bank")


def test_fold_batchnorm_keep_rule_leaves_no_state_on_a_copy_it_then_rewrites(monkeypatch):
    """The keep rule asks backbone_route of the still-unrewritten copy, which fills the structural answer with True.  A network
    whose structure is fine but whose inference module test fails (dropout) is then rewritten: the True must not stay on it.
    The device fact is forced, the networks stay on the host."""
    real = bb._kernel_input
    monkeypatch.setattr(bb, "_kernel_input", lambda device_type, dtype, shape, rgb=True: real("cuda", dtype, shape, rgb))
    monkeypatch.setattr(bb, "NHWC_INFERENCE", True)
    state = ("_nw_nhwc_ok", "_nw_bank", "_nw_infer_plan")
    facts = dict(device_type="cuda", dtype=torch.float32, shape=(2, 3, 64, 64))
    for filled in (False, True):
        src = bb.densenet121(drop_rate=0.1)
        if filled:
            assert bb._nhwc_structure(src) is True
            src._nw_bank, src._nw_infer_plan = object(), {"sig": None}
        assert bb.backbone_route(src, grad=False, training=False, **facts) == "modules"     # (dropout: not the inference path's)
        copy = bb.fold_batchnorm(src)
        assert isinstance(copy.features.conv0, bb.ConvBiasAct) and isinstance(copy.features.norm0, nn.Identity)      # rewritten
        for m in copy.modules():
            assert not any(hasattr(m, k) for k in state), (type(m).__name__, [k for k in state if hasattr(m, k)])
        for training in (True, False):
            assert bb.backbone_route(copy, grad=training, training=training, **facts) == "modules"
        assert bb._nhwc_structure(copy) is False
        assert bb.backbone_route(src, grad=True, training=True, **facts) == "nhwc_train"      # the source is untouched
    # ... and a network the inference path serves is kept as it is, also without inherited state
    for make in (bb.densenet121, bb.CIFAR_ResNet18):
        src = make()
        assert bb._nhwc_structure(src) is True
        src._nw_bank, src._nw_infer_plan = object(), {"sig": None}
        copy = bb.fold_batchnorm(src)
        assert not any(isinstance(m, (bb.ConvBiasAct, bb.ScaleShiftReLU, bb.Conv1x1Fused, bb.Conv3x3Fused)) for m in copy.modules())
        assert not any(hasattr(m, k) for m in copy.modules() for k in state)
        assert bb.backbone_route(copy, grad=False, **facts) == "nhwc_infer" and all(hasattr(src, k) for k in state)


def _random_bn(c=8):
    bn = nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c))
        bn.running_var.copy_(torch.rand(c) * 2.7 + 0.3)
        bn.weight.copy_(torch.randn(c))
        bn.bias.copy_(torch.randn(c))
    return bn.eval()


def test_batchnorm_fold_arithmetic_is_the_written_out_formula_bit_for_bit():
    """a = gamma * rsqrt(var + eps); shift = beta - mean * a; folded pair (w * a over the output channel, beta + (b - mean) * a)
    with b = 0 where the convolution has no bias: the helpers and everything built from them, torch.equal (no tolerance)."""
    torch.manual_seed(3)
    bn, pre = _random_bn(), _random_bn()
    g, beta, mean, var = bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var
    a = g * torch.rsqrt(var + bn.eps)
    shift = beta - mean * a
    assert torch.equal(bb._bn_scale(bn), a) and torch.equal(bb._bn_scale(bn, f32=True), a)
    assert all(torch.equal(x, y) for x, y in zip(bb._bn_scale_shift(bn), (a, shift)))
    assert torch.equal(beta + (torch.zeros_like(a) - mean) * a, shift)          # the two spellings agree where b = 0
    pa = pre.weight.detach() * torch.rsqrt(pre.running_var + pre.eps)
    pshift = pre.bias.detach() - pre.running_mean * pa

    ssr = bb.ScaleShiftReLU(bn)
    assert torch.equal(ssr.scale, a) and torch.equal(ssr.shift, shift)
    args = bb._bn_apply_args(bn)
    want = (mean, torch.rsqrt(var + bn.eps), g, beta)
    assert len(args) == 4 and all(torch.equal(x, y) and x.is_contiguous() and x.dtype == torch.float32 for x, y in zip(args, want))
    assert torch.equal(ops.bn_table(bn), torch.cat((mean, a, beta)))

    for k, bias in ((3, True), (3, False), (1, False), (1, True)):
        conv = nn.Conv2d(8, 8, k, padding=k // 2, bias=bias)
        w, b = conv.weight.detach(), (conv.bias.detach() if bias else torch.zeros(8))
        wf, bf = w * a.view(-1, 1, 1, 1), beta + (b - mean) * a
        for f32 in (False, True):
            got_w, got_b = bb._fold_conv_bn(conv, bn, f32=f32)
            assert torch.equal(got_w, wf) and torch.equal(got_b, bf)
        pair = bb._fold_pair(conv, bn)
        assert type(pair) is bb.ConvBiasAct and torch.equal(pair.weight.detach(), wf) and torch.equal(pair.bias.detach(), bf)
        if k == 3:
            fused = bb.Conv3x3Fused(conv, post_bn=bn, post_relu=True)
            assert torch.equal(fused.weight, wf) and torch.equal(fused.bias, bf)
            plain = bb.Conv3x3Fused(conv)
            assert torch.equal(plain.weight, w) and (torch.equal(plain.bias, b) if bias else plain.bias is None)
        else:
            fused = bb.Conv1x1Fused(conv, pre_bn=pre, post_bn=bn, post_relu=True)
            assert torch.equal(fused.weight, wf.reshape(8, 8)) and torch.equal(fused.bias, bf)
            assert torch.equal(fused.weight_t[:8], wf.reshape(8, 8).t()) and not fused.weight_t[8:].any()
            assert torch.equal(fused.pre_scale, pa) and torch.equal(fused.pre_shift, pshift)
            plain = bb.Conv1x1Fused(conv, pre_bn=pre)
            assert torch.equal(plain.weight, w.reshape(8, 8)) and (torch.equal(plain.bias, b) if bias else plain.bias is None)


def test_weight_bank_follows_every_convolution_weight():
    """One bank per network until ANY convolution's weight Parameter is replaced (not only the stem's): the next training
    forward then finds the new Parameter's operands instead of a KeyError."""
    net = bb.CIFAR_ResNet18()
    bank = bb._weight_bank(net, net.conv1)
    assert bb._weight_bank(net, net.conv1) is bank and net._nw_bank is bank
    assert [id(w) for w in bank.weights] == [id(m.weight) for m in net.modules() if isinstance(m, nn.Conv2d)]
    fwd, dgrad = bank.operands(net.conv1.weight)
    assert fwd is not None and dgrad is None                        # the stem's input needs no gradient
    assert all(bank.operands(m.weight)[1] is not None for m in net.modules() if isinstance(m, nn.Conv2d) and m is not net.conv1
               and m.stride == (1, 1))
    conv = net.layer1[0].conv1
    conv.weight = nn.Parameter(conv.weight.detach().clone())
    bank2 = bb._weight_bank(net, net.conv1)
    assert bank2 is not bank and bank2.operands(conv.weight)[0] is not None and bb._weight_bank(net, net.conv1) is bank2
    net.conv1.weight = nn.Parameter(net.conv1.weight.detach().clone())
    bank3 = bb._weight_bank(net, net.conv1)
    assert bank3 is not bank2 and bank3.operands(net.conv1.weight)[1] is None


def test_cached_plan_is_rebuilt_when_a_tensor_or_the_device_changes():
    net = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4))
    calls = []

    def build():
        calls.append(1)
        return {"n": len(calls)}
    p1 = bb._cached_plan(net, "cuda:0", build)
    assert bb._cached_plan(net, "cuda:0", build) is p1 and len(calls) == 1 and p1["n"] == 1 and net._nw_infer_plan is p1
    ts = list(net.parameters()) + list(net.buffers())
    assert p1["sig"] == ("cuda:0", len(ts), sum(t._version for t in ts), sum(t.data_ptr() & 0xffffff for t in ts))
    net[1].running_mean.add_(1.0)
    p2 = bb._cached_plan(net, "cuda:0", build)
    assert p2 is not p1 and len(calls) == 2
    p3 = bb._cached_plan(net, "cuda:1", build)
    assert p3 is not p2 and len(calls) == 3 and bb._cached_plan(net, "cuda:1", build) is p3
