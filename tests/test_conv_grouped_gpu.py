"""Grouped 3x3 conv kernels (csrc/conv_grouped.hip) on the GPU: exact
arithmetic against a float64 CPU reference on lattice data, weight-grad
determinism, the bridge at block level and the binding guards."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from conv_cases import exact_mismatches, lattice

pytestmark = pytest.mark.gpu

_CL = torch.channels_last

# (N, C, H, W, groups, stride, pad), 3x3
SHAPES = [
    (2, 16, 7, 5, 4, 1, 1),      # Cg 4, one slab, fewer pixels than a tile
    (1, 80, 19, 21, 20, 1, 1),   # Cg 4, channel tail, ragged tiles, 6 slabs
    (2, 32, 13, 14, 4, 2, 1),    # Cg 8, stride 2, odd H and even W
    (2, 16, 10, 11, 4, 2, 0),    # Cg 4, stride 2, pad 0
    (2, 48, 12, 9, 3, 1, 1),     # Cg 16, odd group count
    (1, 64, 17, 17, 2, 2, 1),    # Cg 32, stride 2
    (3, 64, 6, 6, 2, 1, 0),      # Cg 32, pad 0, three images
    (2, 128, 23, 9, 32, 1, 1),   # ResNeXt's own groups=32
    (1, 16, 9, 37, 4, 2, 1),     # stride 2 with OW > 16: two tile columns
    # more tiles than blocks: every block loops over 2+ tiles (1536 fwd and
    # dgrad blocks, 512 wgrad blocks at one channel tile)
    (1600, 16, 3, 3, 4, 1, 1),
]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


@functools.lru_cache(maxsize=None)
def _case(shape, exact=True):
    """Seeded bf16 inputs (CPU; lattice or randn) and, for the lattice, the
    float64 reference; computed once and shared read-only."""
    N, C, H, W, G, stride, pad = shape
    OH, OW = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    assert 9 * max(288, N * OH * OW) < 2 ** 24
    g = torch.Generator().manual_seed(4100 + SHAPES.index(shape))
    dims = ((N, C, H, W), (C, C // G, 3, 3), (N, C, OH, OW))
    if not exact:
        return [torch.randn(d, generator=g).to(torch.bfloat16) for d in dims]
    x, w, dy = (lattice(d, g) for d in dims)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, pad, 1, G)
    y64.backward(dy.double())
    return {"x": x, "w": w, "dy": dy, "fwd": y64.detach(), "dgrad": x64.grad,
            "wgrad": w64.grad}


def _run(direction, x, w, dy, shape):
    N, C, H, W, G, stride, pad = shape
    ext = _ext()
    if direction == "fwd":
        return ext.conv_grouped_fwd(x, w, G, stride, pad)
    if direction == "dgrad":
        return ext.conv_grouped_dgrad(dy, w, N, C, H, W, G, stride, pad)
    return ext.conv_grouped_wgrad(x, dy, G, stride, pad)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("direction", ["fwd", "dgrad", "wgrad"])
def test_grouped_exact(direction, shape):
    """Lattice data: every partial sum is an integer below 2^24, so the
    fp32 accumulation is exact in any order and each output must equal the
    float64 reference rounded once to bf16 — 0 mismatches."""
    c = _case(shape)
    got = _run(direction, _gpu(c["x"]), _gpu(c["w"]), _gpu(c["dy"]), shape)
    assert got.is_contiguous(memory_format=_CL)
    bad = exact_mismatches(got, c[direction], torch.bfloat16)
    print(f"{direction} {shape}: {bad} mismatches of {got.numel()}")
    assert bad == 0


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[5]])
def test_grouped_wgrad_deterministic(shape):
    x, w, dy = (_gpu(t) for t in _case(shape, exact=False))
    a = _run("wgrad", x, w, dy, shape)
    b = _run("wgrad", x, w, dy, shape)
    assert torch.equal(a, b)


def test_grouped_block_level():
    """One BottleneckX(256, 64) block, native against library grouped
    conv2, at the tolerances of test_stem_model_level."""
    from ddlbench_amd.models.resnet import BottleneckX
    from ddlbench_amd.ops.conv import Conv2dGrouped, convert_convs
    torch.manual_seed(0)
    lib = BottleneckX(256, 64).to(_dev()).to(torch.bfloat16) \
        .to(memory_format=_CL)
    nat = copy.deepcopy(lib)
    n_lib = convert_convs(lib, grouped="library")
    assert convert_convs(nat, grouped="native") == n_lib + 1
    assert sum(isinstance(m, Conv2dGrouped) for m in nat.modules()) == 1
    assert isinstance(nat.conv2, Conv2dGrouped)
    x = _gpu(torch.randn(4, 256, 14, 14).to(torch.bfloat16))
    dy = _gpu(torch.randn(4, 256, 14, 14).to(torch.bfloat16))
    outs = []
    for m in (lib, nat):
        out = m(x)
        out.backward(dy)
        outs.append(out.detach().float())
    g_lib = lib.conv2.weight.grad.float()
    g_nat = nat.conv2.weight.grad.float()
    assert nat.conv2.weight.grad.dtype == torch.bfloat16
    atol = 0.02 * g_lib.abs().max().item()
    print("block: max |dout|", (outs[1] - outs[0]).abs().max().item(),
          "max |dgrad|", (g_nat - g_lib).abs().max().item(), "atol", atol)
    torch.testing.assert_close(g_nat, g_lib, rtol=5e-2, atol=atol)
    torch.testing.assert_close(outs[1], outs[0], rtol=5e-2, atol=5e-2)


def test_grouped_binding_guards():
    ext = _ext()
    x = torch.randn(1, 32, 9, 9, device=_dev(), dtype=torch.bfloat16)
    w = _gpu(torch.randn(32, 8, 3, 3).to(torch.bfloat16))
    w2 = _gpu(torch.randn(32, 2, 3, 3).to(torch.bfloat16))
    xcl = x.contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):     # Cg = 2
        ext.conv_grouped_fwd(xcl, w2, 16, 1, 1)
    with pytest.raises(RuntimeError):     # fp32 input
        ext.conv_grouped_fwd(xcl.float(), w.float(), 4, 1, 1)
    assert not x.is_contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):     # NCHW-contiguous x
        ext.conv_grouped_fwd(x, w, 4, 1, 1)
    ext.conv_grouped_fwd(xcl, w, 4, 1, 1)
    torch.cuda.synchronize()
