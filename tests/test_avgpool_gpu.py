"""Average-pool kernels (csrc/avgpool.hip) on the GPU: exact arithmetic
against a float64 CPU reference on lattice data, a derived bound and
run-to-run bit equality on random data, the bridge at model level and the
binding guards.

Exactness: lattice values are integers in [-3, 3], so a window sum is an
integer s with |s| <= 3d, exact in fp32 in any order, and for every such s
and every divisor d used here fp32(s) * fp32(1/d) rounds to the same bf16
as the float64 s / d."""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import exact_mismatches, lattice

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
_BF = torch.bfloat16

# (N, C, H, W, k, stride, pad)
WINDOWED = [
    (2, 8, 1, 1, 3, 1, 1),      # a window that is all padding but one tap
    (1, 44, 5, 7, 3, 1, 1),     # 8-byte lanes, NASNet's own C, H != W
    (1, 220, 6, 6, 3, 1, 1),    # many 4-channel vectors, no wave multiple
    (1, 8, 40, 70, 3, 1, 1),    # several tiles both ways, ragged last tile
    (2, 16, 9, 9, 3, 2, 1),     # odd extent at stride 2
    (2, 16, 8, 8, 3, 2, 1),     # even extent at stride 2
    (2, 24, 7, 7, 2, 2, 0),     # uncovered trailing row and column: dx = 0
    (2, 24, 8, 8, 2, 2, 0),
    (300, 8, 3, 3, 3, 1, 1),    # grid-stride
]
# (N, C, H, W)
GLOBAL = [
    (1, 8, 1, 1),
    (3, 44, 7, 7),
    (2, 2048, 7, 7),
    (2, 16, 17, 17),            # split, pixels no multiple of the slices
    (1, 8, 64, 64),             # pixel split, 16 pixels per thread
    (520, 8, 2, 2),             # no split, several blocks
]
RANDOM = [(2, 44, 13, 11, 3, 2, 1), (3, 40, 9, 9)]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _pool64(x, geom):
    return F.avg_pool2d(x, *geom) if geom else F.adaptive_avg_pool2d(x, 1)


@functools.lru_cache(maxsize=None)
def _case(shape, exact=True):
    """Seeded bf16 x and dy (CPU; lattice or randn), the float64 reference
    y and dx, and the same pool of |x| and |dy| (ay, adx) for the random
    bound; computed once and shared read-only."""
    geom = shape[4:]
    g = torch.Generator().manual_seed(1600 + sum(shape))

    def make(s):
        return lattice(s, g) if exact else torch.randn(s, generator=g).to(_BF)
    x = make(shape[:4])
    x64 = x.double().requires_grad_()
    y64 = _pool64(x64, geom)
    dy = make(tuple(y64.shape))
    # float64 autograd scales every dy by 1/k^2 before it sums them, which
    # leaves 2^-54-sized residues where the sum is 0; on the lattice it gets
    # k^2 dy instead, so its sums are the integers s, divided once
    scale = geom[0] ** 2 if exact and geom else 1
    y64.backward(dy.double() * scale)
    if scale > 1:
        assert torch.equal(x64.grad, x64.grad.round())
        x64.grad /= scale
    a64 = x.double().abs().requires_grad_()
    ay = _pool64(a64, geom)
    ay.backward(dy.double().abs())
    return {"x": x, "dy": dy, "fwd": y64.detach(), "bwd": x64.grad,
            "afwd": ay.detach(), "abwd": a64.grad}


def _run(shape, d, direction):
    from ddlbench_amd.ops.pool import avgpool2d_nhwc, global_avgpool_nhwc
    x = _gpu(d["x"]).requires_grad_()
    y = avgpool2d_nhwc(x, *shape[4:]) if shape[4:] else global_avgpool_nhwc(x)
    if direction == "fwd":
        return y.detach()
    y.backward(_gpu(d["dy"]))
    return x.grad


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("shape", WINDOWED + GLOBAL, ids=str)
def test_avgpool_exact(shape, direction):
    d = _case(shape)
    got = _run(shape, d, direction)
    assert got.is_contiguous(memory_format=_CL)
    bad = exact_mismatches(got, d[direction], _BF)
    print(f"avgpool {shape} {direction}: {bad}/{got.numel()} mismatches")
    assert bad == 0


def test_global_plan_paths():
    ext = _ext()
    plans = [ext.avgpool_plan(*s)["global"] for s in GLOBAL[3:]]
    assert [p["split"] for p in plans] == [True, True, False]
    assert 17 * 17 % plans[0]["psplit"] != 0
    assert plans[1]["psplit"] * 16 == 64 * 64
    assert plans[2]["fwd_blocks"] > 1
    tiled = ext.avgpool_plan(1, 8, 40, 70, 3, 1, 1)["fwd"]
    assert tiled["grid"][0] > 1 and tiled["grid"][1] > 1
    assert 70 % tiled["tile"][1] != 0
    strided = ext.avgpool_plan(300, 8, 3, 3, 3, 1, 1)["fwd"]
    assert strided["tiles"] > strided["blocks"]


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("shape", RANDOM, ids=str)
def test_avgpool_random(shape, direction):
    """|err| <= 2^-8 |ref| + n 2^-23 A: one bf16 rounding plus the fp32
    summation bound over n terms of mean magnitude A."""
    d = _case(shape, exact=False)
    got = _run(shape, d, direction)
    n = shape[4] ** 2 if shape[4:] else shape[2] * shape[3]
    ref = d[direction]
    bound = 2.0 ** -8 * ref.abs() + n * 2.0 ** -23 * d["a" + direction]
    excess = ((got.double().cpu() - ref).abs() - bound).max().item()
    print(f"avgpool {shape} {direction}: worst err - bound {excess:.3e}")
    assert excess <= 0
    assert torch.equal(got, _run(shape, d, direction))


def _rel(a, b64):
    return ((a.detach().double().cpu() - b64).norm() / b64.norm()).item()


def _block(kind):
    """(module, inputs, name of a parameter whose gradient passes through
    the pools' backward or reads their forward)."""
    torch.manual_seed(0)
    if kind == "inception":
        from ddlbench_amd.models.extra import InceptionA, _PoolFC
        a = InceptionA(64, 32)
        m = nn.Sequential(a, _PoolFC(nn.Linear(a.out_channels, 10)))
        return m, [torch.randn(4, 64, 9, 9)], "0.bp.conv.weight"
    from ddlbench_amd.models.nasnet import NormalCell
    m = NormalCell(32, 32, 44, False)
    return m, [torch.randn(4, 32, 8, 8) for _ in range(2)], \
        "fit_hp.conv.weight"


@pytest.mark.parametrize("kind,pools", [("inception", 2), ("nasnet", 1)])
def test_avgpool_model_level(kind, pools):
    """Forward + backward through autograd: against a float64 CPU copy the
    native block's relative L2 error of the output, of one parameter
    gradient and of the input gradient is at most 3x the library block's —
    the library's own bf16 error is the yardstick, 3x allows for a
    different but equally valid summation order."""
    from ddlbench_amd.ops.conv import convert_convs
    from ddlbench_amd.ops.modules import BNAct
    from ddlbench_amd.ops.pool import AvgPool2dNHWC, GlobalAvgPoolNHWC
    ref, xs, pname = _block(kind)
    ref = ref.to(_BF)
    xs = [x.to(_BF) for x in xs]
    models, counts = {}, {}
    for mode in ("library", "native"):
        m = copy.deepcopy(ref).to(_dev()).to(memory_format=_CL)
        counts[mode] = convert_convs(m, avgpool=mode)
        models[mode] = m
    assert counts["native"] - counts["library"] == pools
    swapped = [type(m) for m in models["native"].modules()
               if isinstance(m, (AvgPool2dNHWC, GlobalAvgPoolNHWC))]
    assert swapped == [AvgPool2dNHWC, GlobalAvgPoolNHWC][:pools]
    ref = ref.double()
    for b in ref.modules():  # BNAct keeps itself fp32 under .double()
        if isinstance(b, BNAct):
            for t in (b.weight, b.bias, b.running_mean, b.running_var):
                t.data = t.data.double()
    xs64 = [x.double().requires_grad_() for x in xs]
    out64 = ref(*xs64)
    dy = torch.randn(out64.shape).to(_BF)
    out64.backward(dy.double())
    want = [out64.detach(), dict(ref.named_parameters())[pname].grad,
            xs64[0].grad]
    errs = {}
    for mode, m in models.items():
        gx = [_gpu(x).requires_grad_() for x in xs]
        out = m(*gx)
        out.backward(dy.to(_dev()))
        got = [out, dict(m.named_parameters())[pname].grad, gx[0].grad]
        errs[mode] = [_rel(g, w) for g, w in zip(got, want)]
    for what, lib, nat in zip(["output", pname, "dx"], errs["library"],
                              errs["native"]):
        print(f"{kind} {what}: library {lib:.3e} native {nat:.3e}")
        assert nat <= 3 * lib


@pytest.mark.parametrize("case", ["fp32", "nchw", "c6", "k5", "pad0",
                                  "dy_size"])
def test_avgpool_argument_checks(case):
    ext = _ext()
    x = torch.randn(1, 8, 6, 9, device=_dev(), dtype=_BF)
    assert not x.is_contiguous(memory_format=_CL)
    xcl = x.contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):
        if case == "fp32":
            ext.avgpool_fwd(xcl.float(), 3, 1, 1)
        elif case == "nchw":
            ext.global_avgpool_fwd(x)
        elif case == "c6":
            ext.avgpool_fwd(_gpu(x[:, :6]), 3, 1, 1)
        elif case == "k5":
            ext.avgpool_fwd(xcl, 5, 1, 2)
        elif case == "pad0":
            ext.avgpool_fwd(xcl, 3, 1, 0)
        else:
            ext.avgpool_bwd(xcl, 12, 19, 3, 2, 1)   # OW would be 10, not 9
