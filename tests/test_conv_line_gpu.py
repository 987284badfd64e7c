"""(1,T) / (T,1) conv kernels (csrc/conv_line.hip) on the GPU: exact
arithmetic against a float64 CPU reference on lattice data, weight-grad
determinism, the autograd bridge, an InceptionC block at model level and
the binding guards."""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import exact_mismatches, lattice

pytestmark = pytest.mark.gpu

_CL = torch.channels_last

# (N, C, K, H, W, orient, T): "w" is a (1,T) filter, "h" a (T,1) filter
SHAPES = [
    (2, 32, 32, 5, 3, "w", 7),      # line shorter than the filter; one chunk
    (2, 32, 64, 3, 5, "h", 7),      # the same along H; C != K
    (3, 128, 192, 12, 12, "w", 7),  # the model's geometry; ragged last tile
    (3, 128, 192, 12, 12, "h", 7),  # the same, along H
    (1, 160, 160, 17, 13, "h", 7),  # five 32-chunks; H != W
    (2, 64, 32, 7, 30, "w", 7),     # highres line; BL*L no multiple of 16
    (1, 32, 32, 4, 64, "w", 3),     # L at the limit; T = 3
    # 2400 lines: grid-stride loops in every direction, many wgrad slabs
    (600, 32, 32, 4, 4, "h", 7),
]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _filter(shape):
    """(kernel_size, padding) of the shape's conv."""
    T = shape[6]
    return ((1, T), (0, T // 2)) if shape[5] == "w" else ((T, 1), (T // 2, 0))


@functools.lru_cache(maxsize=None)
def _case(shape, exact=True):
    """Seeded bf16 inputs (CPU; lattice or randn) and, for the lattice, the
    float64 reference; computed once and shared read-only."""
    N, C, K, H, W, orient, T = shape
    ks, pad = _filter(shape)
    assert 9 * max(T * C, T * K, N * H * W) < 2 ** 24
    g = torch.Generator().manual_seed(7100 + SHAPES.index(shape))
    dims = ((N, C, H, W), (K, C) + ks, (N, K, H, W))
    if not exact:
        return [torch.randn(d, generator=g).to(torch.bfloat16) for d in dims]
    x, w, dy = (lattice(d, g) for d in dims)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, 1, pad)
    y64.backward(dy.double())
    return {"x": x, "w": w, "dy": dy, "fwd": y64.detach(), "dgrad": x64.grad,
            "wgrad": w64.grad}


def _run(direction, x, w, dy):
    ext = _ext()
    if direction == "fwd":
        return ext.conv_line_fwd(x, w)
    if direction == "dgrad":
        return ext.conv_line_dgrad(dy, ext.conv_weight_dgrad_layout(w),
                                   *x.shape)
    return ext.conv_line_wgrad(x, dy, w.shape[2], w.shape[3])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("direction", ["fwd", "dgrad", "wgrad"])
def test_line_exact(direction, shape):
    """Lattice data: every partial sum is an integer below 2^24, so the
    fp32 accumulation is exact in any order and each output must equal the
    float64 reference rounded once to bf16 — 0 mismatches."""
    c = _case(shape)
    if shape[0] == 600:
        plan = _ext().line_plan(*shape)
        assert all(plan[d]["tiles"] > plan[d]["slots"]
                   for d in ("fwd", "dgrad", "wgrad"))
        assert plan["wgrad"]["slots"] > 8
    got = _run(direction, _gpu(c["x"]), _gpu(c["w"]), _gpu(c["dy"]))
    assert got.is_contiguous(memory_format=_CL)
    bad = exact_mismatches(got, c[direction], torch.bfloat16)
    print(f"{direction} {shape}: {bad} mismatches of {got.numel()}")
    assert bad == 0


def test_line_wgrad_deterministic():
    x, w, dy = (_gpu(t) for t in _case(SHAPES[2], exact=False))
    assert torch.equal(_run("wgrad", x, w, dy), _run("wgrad", x, w, dy))


def test_line_bridge(monkeypatch):
    """nn.Conv2d -> convert_convs(line="native") -> autograd: y, dx and
    weight.grad exact; no dgrad when x needs no gradient."""
    from ddlbench_amd.ops.conv import Conv2dLine, convert_convs
    shape = SHAPES[2]
    N, C, K, H, W, orient, T = shape
    c = _case(shape)
    net = nn.Sequential(nn.Conv2d(C, K, (1, 7), padding=(0, 3), bias=False))
    net[0].weight.data.copy_(c["w"])
    net = net.to(_dev()).to(torch.bfloat16).to(memory_format=_CL)
    weight = net[0].weight
    assert convert_convs(net, line="native") == 1
    assert isinstance(net[0], Conv2dLine) and net[0].weight is weight
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
    monkeypatch.setattr(_ext(), "conv_line_dgrad", no_dgrad)
    weight.grad = None
    x2 = _gpu(c["x"])
    net(x2).backward(_gpu(c["dy"]))
    assert x2.grad is None
    assert exact_mismatches(weight.grad, c["wgrad"], torch.bfloat16) == 0


def _rel(a, b64):
    return ((a.detach().double().cpu() - b64).norm() / b64.norm()).item()


def test_line_model_level():
    """One InceptionC(64, 32) block at 12x12, batch 4, forward + backward:
    against a float64 CPU copy, the native block's relative L2 error of the
    output and of two line-conv weight gradients is at most 3x the library
    block's — the library's own bf16 error is the yardstick, 3x allows for
    a different but equally valid summation order."""
    from ddlbench_amd.models.extra import InceptionC
    from ddlbench_amd.ops.conv import Conv2dLine, convert_convs
    from ddlbench_amd.ops.modules import BNAct
    torch.manual_seed(0)
    ref = InceptionC(64, 32).to(torch.bfloat16)
    x = torch.randn(4, 64, 12, 12).to(torch.bfloat16)
    dy = torch.randn(4, ref.out_channels, 12, 12).to(torch.bfloat16)
    models = {}
    for mode in ("library", "native"):
        m = copy.deepcopy(ref).to(_dev()).to(memory_format=_CL)
        convert_convs(m, line=mode)
        models[mode] = m
    assert sum(isinstance(m, Conv2dLine)
               for m in models["native"].modules()) == 6
    names = [n for n, p in ref.named_parameters()
             if p.dim() == 4 and p.shape[2] != p.shape[3]]
    names = [names[0], names[-1]]   # a (1,7) of b7 and the last of b7d
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
        out.backward(_gpu(dy))
        p = dict(m.named_parameters())
        errs[mode] = [_rel(out, out64.detach())] + [
            _rel(p[n].grad, p64[n].grad) for n in names]
    for what, lib, nat in zip(["output"] + names, errs["library"],
                              errs["native"]):
        print(f"{what}: library {lib:.3e} native {nat:.3e}")
        assert nat <= 3 * lib


@pytest.mark.parametrize("case", ["fp32", "nchw", "c24", "t5", "l65",
                                  "square", "dy_size"])
def test_line_argument_checks(case):
    ext = _ext()
    bf = dict(device=_dev(), dtype=torch.bfloat16)
    x = torch.randn(1, 32, 6, 9, **bf)
    assert not x.is_contiguous(memory_format=_CL)
    xcl = x.contiguous(memory_format=_CL)
    w = _gpu(torch.randn(32, 32, 1, 7, **bf))
    with pytest.raises(RuntimeError):
        if case == "fp32":
            ext.conv_line_fwd(xcl.float(), w.float())
        elif case == "nchw":
            ext.conv_line_fwd(x, w)
        elif case == "c24":
            ext.conv_line_fwd(_gpu(torch.randn(1, 24, 6, 9, **bf)),
                              _gpu(torch.randn(32, 24, 1, 7, **bf)))
        elif case == "t5":
            ext.conv_line_fwd(xcl, _gpu(torch.randn(32, 32, 1, 5, **bf)))
        elif case == "l65":
            ext.conv_line_fwd(_gpu(torch.randn(1, 32, 2, 65, **bf)), w)
        elif case == "square":
            ext.conv_line_fwd(xcl, _gpu(torch.randn(32, 32, 7, 7, **bf)))
        else:
            dy = _gpu(torch.randn(1, 32, 6, 8, **bf))
            ext.conv_line_dgrad(dy, ext.conv_weight_dgrad_layout(w),
                                1, 32, 6, 9)
    torch.cuda.synchronize()
