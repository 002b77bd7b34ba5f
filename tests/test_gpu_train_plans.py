"""The tape layouts and the gradient layouts of the three training paths, pinned: they are the contract between the forward pass,
the backward pass, the optimiser, the dropout keep-masks and the l2 reduction order, so every name, shape, offset and total must
stay what tests/golden/train_plans.json recorded.  Net creation and plan calls only: no forward pass runs.

The fixture is NOT made from the code under test.  It was written by hand, on the GPU, at the commit before the tape planner and
the gradient-object core got their single owners, from the repository root:
    PYTHONPATH=.:wsss-analysis_amd python -c "from tests import test_gpu_train_plans as t; t.generate()"
Run that again only at a commit whose layouts are known good, and only when a layout is meant to change.

The "cls" key (the 01_train stacks: tape plans, `layout`, `param_layout` and the two totals) was merged in later, by
generate_cls(), with the library of commit 44ad860 -- the commit before the parameter codec and the trainer core got their single
owners.  It uses only Net.cls_tape_plan, ClsGrad.layout and ClsGrad.param_layout, and leaves the recorded "seg" and "irn" values
untouched."""
import json
import os

import pytest

from tests import deeplab_ref as ref
from tests import test_gpu_cls_sgd as cls_sgd
from tests.test_gpu_irn_grad import model
from wsscam import _lib, secdsrg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plans.json")
SEG_C, SEG_HW = 5, (64, 48)            # the thin nets of test_gpu_seg_grad.test_tape_is_the_forward_pass
SEG_PLANS = [(2, 65, 65), (1, 33, 49)]  # (B, H, W)
IRN_ARCHS = ["resnet50", "vgg16", "m7"]  # every net test_gpu_irn_grad.model builds
IRN_PLANS = [(2, 64), (1, 96)]          # (N, S)
CLS_NETS = list(cls_sgd.NETS)           # VGG16 with and without BatchNorm, M7 on a Keras session's pools
CLS_PLANS = [(2, 33, 33), (1, 40, 56)]  # (B, H, W)


def _plan(entries, elems):
    return {"entries": [[e["name"], e["Ho"], e["Wo"], e["C"], e["offset"]] for e in entries], "elems": elems}


def seg_plans(ctx, method):
    net = secdsrg.SegNet(method, ref.thin_case(method, SEG_C, SEG_HW)[0], SEG_C, precision=_lib.PREC_F16X3, ctx=ctx)
    try:
        sg = _lib.SegGrad(net.net, net._sd)
        try:
            layout = [[name, e["k"], e["Cin"], e["Cout"], e["w_off"], e["b_off"]] for name, e in sg.layout.items()]
            return {"tape": {"%dx%dx%d" % p: _plan(*net.net.seg_tape_plan(*p)) for p in SEG_PLANS}, "layout": layout,
                    "grad_elems": sg.grad_elems}
        finally:
            sg.close()
    finally:
        net.close()


def irn_plans(arch):
    m, _ = model(arch, _lib.PREC_F16X3 if arch == "resnet50" else None)
    net, grad = m._ensure_net(), m.irn_grad()
    layout = [[e["name"], e["conv"], list(e["shape"]), e["offset"], e["size"]] for e in grad.layout]
    return {"tape": {"%dx%d" % p: _plan(*net.edge_tape_plan(*p)) for p in IRN_PLANS}, "layout": layout, "grad_elems": grad.grad_elems}


def cls_plans(ctx, net):
    m = cls_sgd.fresh_model(net, cls_sgd.base_sd(net), _lib.PREC_F16X3, ctx=ctx)
    try:
        dev, grad = m._ensure_net(), m.cls_grad()
        layout = [[e["name"], e["conv"], list(e["shape"]), e["offset"], e["size"]] for e in grad.layout]
        params = [[e["name"], e["conv"], e["linear"], list(e["shape"]), e["offset"], e["size"]] for e in grad.param_layout]
        return {"tape": {"%dx%dx%d" % p: _plan(*dev.cls_tape_plan(*p)) for p in CLS_PLANS}, "layout": layout, "grad_elems": grad.grad_elems,
                "param_layout": params, "param_elems": grad.param_elems}
    finally:
        m._release_net()


def generate_cls():
    """(by hand, see the module docstring) merges the "cls" key into the fixture; "seg" and "irn" stay as recorded"""
    ctx = _lib.Context(0)
    with open(GOLDEN) as f:
        out = json.load(f)
    out["cls"] = {net: cls_plans(ctx, net) for net in CLS_NETS}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    return out


def generate():
    """(by hand, see the module docstring) writes the fixture from the library this tree has built"""
    ctx = _lib.Context(0)
    out = {"seg": {method: seg_plans(ctx, method) for method in ("SEC", "DSRG")}, "irn": {arch: irn_plans(arch) for arch in IRN_ARCHS}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    return out


@pytest.fixture(scope="module")
def golden_plans():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want, what):
    assert sorted(got["tape"]) == sorted(want["tape"]), what
    for shape, plan in want["tape"].items():
        assert got["tape"][shape]["elems"] == plan["elems"], (what, shape)
        assert len(got["tape"][shape]["entries"]) == len(plan["entries"]), (what, shape)
        for g, w in zip(got["tape"][shape]["entries"], plan["entries"]):
            assert g == w, (what, shape, g, w)
    assert got["grad_elems"] == want["grad_elems"], what
    assert len(got["layout"]) == len(want["layout"]), what
    for g, w in zip(got["layout"], want["layout"]):
        assert g == w, (what, g, w)


@pytest.mark.parametrize("method", ["SEC", "DSRG"])
def test_seg_plans(ctx, golden_plans, method):
    _same(json.loads(json.dumps(seg_plans(ctx, method))), golden_plans["seg"][method], method)


@pytest.mark.parametrize("arch", IRN_ARCHS)
def test_irn_plans(golden_plans, arch):
    _same(json.loads(json.dumps(irn_plans(arch))), golden_plans["irn"][arch], arch)


@pytest.mark.parametrize("net", CLS_NETS)
def test_cls_plans(ctx, golden_plans, net):
    got, want = json.loads(json.dumps(cls_plans(ctx, net))), golden_plans["cls"][net]
    _same(got, want, net)
    assert got["param_elems"] == want["param_elems"], net
    assert len(got["param_layout"]) == len(want["param_layout"]), net
    for g, w in zip(got["param_layout"], want["param_layout"]):
        assert g == w, (net, g, w)
