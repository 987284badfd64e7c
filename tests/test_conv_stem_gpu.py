"""Stem-conv kernels (csrc/conv_stem.hip) on the GPU: forward and
weight-grad against a float64 CPU reference computed from the same bf16
values, determinism, the autograd bridge, binding guards and a model-level
comparison against the library stem."""

import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_CL = torch.channels_last

# (N, C, H, W, K, R, stride, pad)
SHAPES = [
    (2, 3, 23, 23, 64, 7, 2, 3),    # ImageNet geometry, odd W, OW=12
    (1, 3, 9, 9, 8, 7, 2, 3),       # fewer pixels than a tile, K=8
    (2, 3, 17, 19, 24, 3, 2, 1),    # H != W, K tail vs 16-wide columns
    (3, 1, 13, 13, 64, 3, 1, 1),    # C=1, odd W, Kd=9
    (2, 4, 12, 12, 16, 5, 1, 2),    # C=4, R=5
    (2, 3, 15, 15, 32, 3, 2, 0),    # pad 0
    (2, 2, 10, 11, 128, 3, 1, 1),   # C=2, widest K
]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded bf16 inputs (CPU) and the float64 CPU reference for one
    shape; computed once and shared read-only between the tests."""
    N, C, H, W, K, R, stride, pad = shape
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(K, C, R, R, generator=g).to(torch.bfloat16)
    OH = (H + 2 * pad - R) // stride + 1
    OW = (W + 2 * pad - R) // stride + 1
    dy = torch.randn(N, K, OH, OW, generator=g).to(torch.bfloat16)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, pad)
    y64.backward(dy.double())
    return {"x": x, "w": w, "dy": dy, "y": y64.detach(),
            "dx": x64.grad, "dw": w64.grad, "P": N * OH * OW}


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _dw_logical(dw32, shape):
    """(K, R*R*C) kernel output -> logical (K,C,R,R) on the CPU."""
    N, C, H, W, K, R, stride, pad = shape
    return dw32.view(K, R, R, C).permute(0, 3, 1, 2).cpu().double()


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_fwd(shape):
    """One rounding to bf16 (2^-9 relative) is the only real error: fp32
    accumulation of <= 196 exact products is ~1e-5. rtol 2^-7, atol 1e-3."""
    N, C, H, W, K, R, stride, pad = shape
    c = _case(shape)
    y = _ext().conv_stem_fwd(_gpu(c["x"]), _gpu(c["w"]), stride, pad)
    assert y.dtype == torch.bfloat16
    assert y.shape == c["y"].shape
    assert y.is_contiguous(memory_format=_CL)
    err = (y.cpu().double() - c["y"]).abs().max().item()
    print(f"fwd {shape}: max abs err {err:.3e}")
    torch.testing.assert_close(y.cpu().double(), c["y"], rtol=2 ** -7,
                               atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_wgrad(shape):
    """fp32 summation over P pixels: worst case (P-1) 2^-24 sum|t| with
    E|t| ~ 0.64 is ~3.8e-8 P^2, under 1e-5 P up to P = 263; the two shapes
    above that (P = 288, 507) rely on rounding errors not all aligning
    (measured max error 7.1e-6 at P = 507 against atol 5.1e-3)."""
    N, C, H, W, K, R, stride, pad = shape
    c = _case(shape)
    dw32 = _ext().conv_stem_wgrad(_gpu(c["x"]), _gpu(c["dy"]), R, R, stride,
                                  pad)
    assert dw32.dtype == torch.float32
    assert dw32.shape == (K, R * R * C)
    got = _dw_logical(dw32, shape)
    err = (got - c["dw"]).abs().max().item()
    print(f"wgrad {shape}: P={c['P']} max abs err {err:.3e}")
    torch.testing.assert_close(got, c["dw"], rtol=1e-4,
                               atol=1e-5 * c["P"])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_stem_wgrad_deterministic(shape):
    N, C, H, W, K, R, stride, pad = shape
    c = _case(shape)
    x, dy = _gpu(c["x"]), _gpu(c["dy"])
    a = _ext().conv_stem_wgrad(x, dy, R, R, stride, pad)
    b = _ext().conv_stem_wgrad(x, dy, R, R, stride, pad)
    assert torch.equal(a, b)


def test_stem_autograd_bridge():
    """Conv2dStem end to end with an input that requires grad: native
    forward + weight-grad, library data-grad."""
    from ddlbench_amd.ops.conv import Conv2dStem
    shape = SHAPES[2]
    N, C, H, W, K, R, stride, pad = shape
    c = _case(shape)
    conv = torch.nn.Conv2d(C, K, R, stride=stride, padding=pad, bias=False)
    conv = conv.to(_dev()).to(torch.bfloat16).to(memory_format=_CL)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    stem = Conv2dStem(conv)
    x = _gpu(c["x"]).requires_grad_(True)
    y = stem(x)
    y.backward(_gpu(c["dy"]))
    torch.testing.assert_close(y.detach().cpu().double(), c["y"],
                               rtol=2 ** -7, atol=1e-3)
    assert conv.weight.grad.dtype == torch.bfloat16
    assert conv.weight.grad.shape == conv.weight.shape
    torch.testing.assert_close(conv.weight.grad.cpu().double(), c["dw"],
                               rtol=2 ** -7, atol=1e-5 * c["P"] + 1e-3)
    # dx tolerance of test_kernels_gpu.py::test_conv_mfma_fwd_dgrad
    tol = 0.03 * ((R * R * C) ** 0.5) / 8
    torch.testing.assert_close(x.grad.cpu().double(), c["dx"], rtol=5e-2,
                               atol=max(tol, 0.05))


def test_stem_binding_guards():
    ext = _ext()
    dev = _dev()
    x8 = torch.randn(1, 8, 9, 9, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=_CL)
    w8 = torch.randn(16, 8, 3, 3, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):
        ext.conv_stem_fwd(x8, w8, 1, 1)
    x3 = torch.randn(1, 3, 9, 9, device=dev, dtype=torch.bfloat16)
    w3 = torch.randn(16, 3, 3, 3, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):     # fp32 input
        ext.conv_stem_fwd(x3.float().contiguous(memory_format=_CL),
                          w3.float(), 1, 1)
    assert not x3.is_contiguous(memory_format=_CL)
    with pytest.raises(RuntimeError):     # NCHW-contiguous x
        ext.conv_stem_fwd(x3, w3, 1, 1)
    # the same tensors pass once x is channels_last
    ext.conv_stem_fwd(x3.contiguous(memory_format=_CL), w3, 1, 1)
    torch.cuda.synchronize()


def test_stem_model_level():
    """cifar10 resnet18 with the native stem against the library stem."""
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops.conv import Conv2dStem, convert_convs
    dev = _dev()
    torch.manual_seed(0)
    lib = build_model("cifar10", "resnet18").to(dev).to(torch.bfloat16) \
        .to(memory_format=_CL)
    nat = copy.deepcopy(lib)
    n_lib = convert_convs(lib, stem="library")
    n_nat = convert_convs(nat, stem="native")
    assert n_nat == n_lib + 1
    stems = [(n, m) for n, m in nat.named_modules()
             if isinstance(m, Conv2dStem)]
    assert len(stems) == 1
    name = stems[0][0]

    x = torch.randn(8, 3, 32, 32, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=_CL)
    t = torch.randint(10, (8,), device=dev)
    outs = []
    for m in (lib, nat):
        out = m(x)
        loss = F.cross_entropy(out.float(), t)
        loss.backward()
        assert torch.isfinite(loss).item()
        outs.append(out.detach().float())
    g_lib = lib.get_submodule(name).weight.grad.float()
    g_nat = nat.get_submodule(name).weight.grad.float()
    atol = 0.02 * g_lib.abs().max().item()
    torch.testing.assert_close(g_nat, g_lib, rtol=5e-2, atol=atol)
    torch.testing.assert_close(outs[1], outs[0], rtol=5e-2, atol=5e-2)
