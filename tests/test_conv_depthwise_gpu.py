"""Depthwise KxK conv kernels (csrc/conv_depthwise.hip) on the GPU: exact
arithmetic against a float64 CPU reference on lattice data, weight-grad
determinism, the autograd bridge, NASNet at model level and the binding
guards."""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import exact_mismatches, lattice

pytestmark = pytest.mark.gpu

_CL = torch.channels_last

# (N, C, H, W, K, stride), pad K/2
SHAPES = [
    (2, 44, 9, 11, 5, 1),     # V = 4 path; image smaller than one tile
    (1, 88, 19, 21, 7, 1),    # ragged tiles both ways, 6 tiles, chunk tail
    (2, 176, 14, 13, 7, 2),   # stride 2, even H, odd W: all 4 dgrad classes
    (2, 8, 15, 16, 5, 2),     # stride 2, one channel vector
    (1, 16, 3, 3, 7, 1),      # image smaller than the kernel
    (3, 24, 6, 37, 3, 2),     # K = 3; OW = 19 > the 16-wide tile
    (1, 72, 8, 8, 5, 1),      # C = 2 chunks of 32 + 8
    # 1200 tiles against 1024 blocks: grid-stride loops, and 1024 slabs
    # make every one of the combine's 8 groups add 128 of them
    (1200, 8, 4, 4, 5, 1),
]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _out_hw(shape):
    N, C, H, W, K, stride = shape
    return (H + 2 * (K // 2) - K) // stride + 1, \
        (W + 2 * (K // 2) - K) // stride + 1


@functools.lru_cache(maxsize=None)
def _case(shape, exact=True):
    """Seeded bf16 inputs (CPU; lattice or randn) and, for the lattice, the
    float64 reference; computed once and shared read-only."""
    N, C, H, W, K, stride = shape
    OH, OW = _out_hw(shape)
    assert 9 * max(K * K, N * OH * OW) < 2 ** 24
    g = torch.Generator().manual_seed(5200 + SHAPES.index(shape))
    dims = ((N, C, H, W), (C, 1, K, K), (N, C, OH, OW))
    if not exact:
        return [torch.randn(d, generator=g).to(torch.bfloat16) for d in dims]
    x, w, dy = (lattice(d, g) for d in dims)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, K // 2, 1, C)
    y64.backward(dy.double())
    return {"x": x, "w": w, "dy": dy, "fwd": y64.detach(), "dgrad": x64.grad,
            "wgrad": w64.grad}


def _run(direction, x, w, dy, shape):
    N, C, H, W, K, stride = shape
    ext = _ext()
    if direction == "fwd":
        return ext.conv_depthwise_fwd(x, w, stride)
    if direction == "dgrad":
        return ext.conv_depthwise_dgrad(dy, w, N, C, H, W, stride)
    return ext.conv_depthwise_wgrad(x, dy, K, stride)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("direction", ["fwd", "dgrad", "wgrad"])
def test_depthwise_exact(direction, shape):
    """Lattice data: every partial sum is an integer below 2^24, so the
    fp32 accumulation is exact in any order and each output must equal the
    float64 reference rounded once to bf16 — 0 mismatches."""
    c = _case(shape)
    if shape[0] == 1200:
        plan = _ext().dwk_plan(*shape)
        assert all(plan[d]["tiles"] > plan[d]["slots"]
                   for d in ("fwd", "dgrad", "wgrad"))
        assert plan["wgrad"]["slots"] > 8
    got = _run(direction, _gpu(c["x"]), c["w"].to(_dev()), _gpu(c["dy"]),
               shape)
    if direction != "wgrad":
        assert got.is_contiguous(memory_format=_CL)
    bad = exact_mismatches(got, c[direction], torch.bfloat16)
    print(f"{direction} {shape}: {bad} mismatches of {got.numel()}")
    assert bad == 0


def test_depthwise_wgrad_deterministic():
    shape = SHAPES[1]
    x, w, dy = (_gpu(t) for t in _case(shape, exact=False))
    a = _run("wgrad", x, w, dy, shape)
    b = _run("wgrad", x, w, dy, shape)
    assert torch.equal(a, b)


def test_depthwise_bridge(monkeypatch):
    """nn.Conv2d -> convert_convs(depthwise="native") -> autograd: y, dx
    and weight.grad exact; no dgrad when x needs no gradient."""
    from ddlbench_amd.ops.conv import Conv2dDepthwise, convert_convs
    shape = SHAPES[2]
    N, C, H, W, K, stride = shape
    c = _case(shape)
    net = nn.Sequential(nn.Conv2d(C, C, K, stride, K // 2, groups=C,
                                  bias=False))
    net[0].weight.data.copy_(c["w"])
    net = net.to(_dev()).to(torch.bfloat16).to(memory_format=_CL)
    weight = net[0].weight
    assert convert_convs(net, depthwise="native") == 1
    assert isinstance(net[0], Conv2dDepthwise) and net[0].weight is weight
    x = _gpu(c["x"]).requires_grad_(True)
    y = net(x)
    y.backward(_gpu(c["dy"]))
    assert exact_mismatches(y.detach(), c["fwd"], torch.bfloat16) == 0
    assert exact_mismatches(x.grad, c["dgrad"], torch.bfloat16) == 0
    assert exact_mismatches(weight.grad, c["wgrad"], torch.bfloat16) == 0
    assert weight.grad.stride() == weight.stride()
    # x without a gradient: the data-grad kernel is never reached
    def no_dgrad(*args):
        raise AssertionError("dgrad ran for an input without a gradient")
    monkeypatch.setattr(_ext(), "conv_depthwise_dgrad", no_dgrad)
    weight.grad = None
    x2 = _gpu(c["x"])
    net(x2).backward(_gpu(c["dy"]))
    assert x2.grad is None
    assert exact_mismatches(weight.grad, c["wgrad"], torch.bfloat16) == 0


def _rel(a, b64):
    return ((a.detach().double().cpu() - b64).norm() / b64.norm()).item()


def test_depthwise_model_level():
    """NASNet-A mobile (CIFAR stem), one forward + backward at batch 8:
    against a float64 CPU copy, the native model's relative L2 error of the
    logits and of three depthwise weight gradients is at most 3x the
    library model's — the library's own bf16 error is the yardstick, 3x
    allows for a different but equally valid summation order."""
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops.conv import Conv2dDepthwise, convert_convs
    from ddlbench_amd.ops.modules import BNAct
    torch.manual_seed(0)
    ref = build_model("cifar10", "nasnetamobile").to(torch.bfloat16)
    x = torch.randn(8, 3, 32, 32).to(torch.bfloat16)
    dy = torch.randn(8, 10).to(torch.bfloat16)
    models = {}
    for mode in ("library", "native"):
        m = copy.deepcopy(ref).to(_dev()).to(memory_format=_CL)
        convert_convs(m, depthwise=mode)
        models[mode] = m
    assert any(isinstance(m, Conv2dDepthwise)
               for m in models["native"].modules())
    names = ["cells.0.b1_r.dw1.weight", "cells.4.b0_l.dw1.weight",
             "cells.13.b2_r.dw2.weight"]
    ref = ref.double()
    for b in ref.modules():  # BNAct keeps itself fp32 under .double()
        if isinstance(b, BNAct):
            for t in (b.weight, b.bias, b.running_mean, b.running_var):
                t.data = t.data.double()
    out64 = ref(x.double())
    out64.backward(dy.double())
    p64 = dict(ref.named_parameters())
    errs = {}
    for mode, m in models.items():
        out = m(_gpu(x))
        out.backward(dy.to(_dev()))
        p = dict(m.named_parameters())
        errs[mode] = [_rel(out, out64.detach())] + [
            _rel(p[n].grad, p64[n].grad) for n in names]
    for what, lib, nat in zip(["logits"] + names, errs["library"],
                              errs["native"]):
        print(f"{what}: library {lib:.3e} native {nat:.3e}")
        assert nat <= 3 * lib


@pytest.mark.parametrize("case", ["fp32", "nchw", "c6", "k4", "stride3",
                                  "dy_size"])
def test_depthwise_argument_checks(case):
    ext = _ext()
    bf = dict(device=_dev(), dtype=torch.bfloat16)
    x = torch.randn(1, 8, 9, 9, **bf)
    assert not x.is_contiguous(memory_format=_CL)
    xcl = x.contiguous(memory_format=_CL)
    w = torch.randn(8, 1, 5, 5, **bf)
    with pytest.raises(RuntimeError):
        if case == "fp32":
            ext.conv_depthwise_fwd(xcl.float(), w.float(), 1)
        elif case == "nchw":
            ext.conv_depthwise_fwd(x, w, 1)
        elif case == "c6":
            ext.conv_depthwise_fwd(_gpu(torch.randn(1, 6, 9, 9, **bf)),
                                   torch.randn(6, 1, 5, 5, **bf), 1)
        elif case == "k4":
            ext.conv_depthwise_fwd(xcl, torch.randn(8, 1, 4, 4, **bf), 1)
        elif case == "stride3":
            ext.conv_depthwise_fwd(xcl, w, 3)
        else:
            dy = _gpu(torch.randn(1, 8, 9, 8, **bf))
            ext.conv_depthwise_dgrad(dy, w, 1, 8, 9, 9, 1)
    torch.cuda.synchronize()
