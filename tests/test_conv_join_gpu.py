"""Residual-join gradient add fused into the conv data-grad epilogue.

``conv_igemm_dgrad(..., add=a)`` must equal ``conv_igemm_dgrad(...) + a``
bit for bit (the epilogue rounds the accumulator to bf16 first, then does
the one bf16 add the eager kernel does), for both kernel structures and
for the stride-2 paths; blocks wired through ``forward_join`` must compute
what the unfused blocks compute. All @gpu."""

import contextlib
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_CL = torch.channels_last


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"


@contextlib.contextmanager
def _env(name, value):
    prev = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = prev


# (N, C, H, W, K, R, stride, pad): dgrad GEMM is M=N*H*W, Nd=C, Kd=R*R*K
_SHAPES = [
    # M=98 < one tile; Nd=256 -> 128x128 tile, two column blocks; LIN Kd=64
    (2, 256, 7, 7, 64, 1, 1, 0),
    # M=162 crosses the 128-row tile with a ragged last tile; 3x3 gather,
    # Kd=576
    (2, 256, 9, 9, 64, 3, 1, 1),
    # Nd=64 -> 256x64 tile, M=162 inside one tile; gather Kd=576
    (2, 64, 9, 9, 64, 3, 1, 1),
    # M=300 crosses the 256-row tile, ragged; LIN Kd=64
    (3, 64, 10, 10, 64, 1, 1, 0),
    # Nd=128, one column block, LIN with Kd=576 (nine K-tiles)
    (2, 128, 9, 9, 576, 1, 1, 0),
    # Nd=40: the deep-pipeline structure declines -> 128-tile structure
    (2, 40, 9, 9, 64, 1, 1, 0),
    (3, 40, 10, 10, 64, 3, 1, 1),
    # 3x3 stride 2 (parity classes, even and odd spatial size)
    (2, 64, 10, 10, 128, 3, 2, 1),
    (2, 128, 9, 9, 64, 3, 2, 1),
    # 1x1 stride 2: classes no tap reaches -> the binding adds
    (2, 64, 10, 10, 128, 1, 2, 0),
]


def _dgrad_inputs(shape):
    N, C, H, W, K, R, stride, pad = shape
    torch.manual_seed(0)
    dev = _dev()
    OH = (H + 2 * pad - R) // stride + 1
    dy = torch.randn(N, K, OH, OH, device=dev,
                     dtype=torch.bfloat16).contiguous(memory_format=_CL)
    w = torch.randn(K, C, R, R, device=dev, dtype=torch.bfloat16)
    w_perm = w.permute(1, 2, 3, 0).contiguous()
    a = torch.randn(N, C, H, W, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=_CL)
    return dy, w_perm, a


@pytest.mark.parametrize("v2", ["1", "0"])
@pytest.mark.parametrize("shape", _SHAPES)
def test_dgrad_addend_is_exact(shape, v2):
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    N, C, H, W, K, R, stride, pad = shape
    dy, w_perm, a = _dgrad_inputs(shape)
    a0 = a.clone()
    with _env("DDLB_CONV_V2", v2):
        plain = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad)
        none = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                                    add=None)
        fused = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                                     add=a)
    assert torch.equal(none, plain), "add=None differs from no argument"
    assert fused.data_ptr() != a.data_ptr()
    assert fused.is_contiguous(memory_format=_CL)
    assert torch.equal(a, a0), "the addend was written"
    assert torch.equal(fused, plain + a), "fused add is not the eager add"


def test_dgrad_addend_is_checked():
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    shape = (2, 64, 9, 9, 64, 1, 1, 0)
    N, C, H, W, K, R, stride, pad = shape
    dy, w_perm, a = _dgrad_inputs(shape)
    with pytest.raises(RuntimeError):
        ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                             add=a.float())
    with pytest.raises(RuntimeError):
        ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                             add=a.contiguous())
    with pytest.raises(RuntimeError):
        ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                             add=a[:1])


# ------------------------------------------------------------ block level
def _run_block(block, x0, dy, join):
    """One forward+backward from the block's current (identical) state."""
    blk = copy.deepcopy(block)
    x = x0.clone().requires_grad_(True)
    with _env("DDLB_JOIN", "1" if join else "0"):
        y = blk(x)
        y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, dict(
        (n, p.grad) for n, p in blk.named_parameters())


@pytest.mark.parametrize("kind", ["identity", "downsample"])
def test_block_join_matches_unfused(kind, monkeypatch):
    from ddlbench_amd.models.resnet import Bottleneck
    from ddlbench_amd.ops import require_extension
    from ddlbench_amd.ops.conv import Conv2dMFMA, convert_convs
    from ddlbench_amd.ops.modules import set_default_backend
    ext = require_extension()
    dev = _dev()
    torch.manual_seed(0)
    if kind == "identity":
        block, cin = Bottleneck(64, 16), 64
        assert block.downsample is None
    else:
        block, cin = Bottleneck(32, 16, stride=2), 32
        assert block.downsample is not None
    block = block.to(dev).to(torch.bfloat16).to(memory_format=_CL)
    assert convert_convs(block) >= 3
    assert isinstance(block.conv1, Conv2dMFMA)
    x0 = torch.randn(2, cin, 8, 8, device=dev,
                     dtype=torch.bfloat16).contiguous(memory_format=_CL)

    addends = []
    real = ext.conv_igemm_dgrad

    def counting(*args, **kw):
        add = kw.get("add", args[8] if len(args) > 8 else None)
        addends.append(add is not None)
        return real(*args, **kw)

    monkeypatch.setattr(ext, "conv_igemm_dgrad", counting)
    set_default_backend("native")
    try:
        with torch.no_grad():
            dy = torch.randn_like(block(x0))
        y_f, dx_f, g_f = _run_block(block, x0, dy, join=True)
        fused_calls = list(addends)
        del addends[:]
        y_u, dx_u, g_u = _run_block(block, x0, dy, join=False)
        unfused_calls = list(addends)
    finally:
        set_default_backend("auto")

    assert sum(fused_calls) == 1, fused_calls    # one join per block
    assert sum(unfused_calls) == 0, unfused_calls
    assert len(fused_calls) == len(unfused_calls)
    assert torch.equal(y_f, y_u)
    # tolerances of tests/test_kernels_gpu.py: bf16 conv dx / dw and the
    # bf16 BN parameter gradients
    torch.testing.assert_close(dx_f.float(), dx_u.float(), rtol=5e-2,
                               atol=0.05)
    assert g_f.keys() == g_u.keys()
    for name in g_f:
        assert g_f[name] is not None, name
        if g_f[name].dim() == 4:
            torch.testing.assert_close(g_f[name].float(), g_u[name].float(),
                                       rtol=5e-2, atol=1.0)
        else:
            torch.testing.assert_close(g_f[name].float(), g_u[name].float(),
                                       rtol=2e-2, atol=2e-2)


def test_join_with_unused_shortcut_and_no_input_grad():
    """forward_join's skip left unused takes the plain dgrad; an input
    that needs no gradient skips dgrad altogether."""
    from ddlbench_amd.ops.conv import Conv2dMFMA
    dev = _dev()
    torch.manual_seed(0)
    conv = Conv2dMFMA(torch.nn.Conv2d(64, 32, 1, bias=False)
                      .to(dev).to(torch.bfloat16).to(memory_format=_CL))
    x = torch.randn(2, 64, 7, 7, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=_CL)
    xa = x.clone().requires_grad_(True)
    y, skip = conv.forward_join(xa)
    assert skip.data_ptr() == xa.data_ptr()      # alias, not a copy
    dy = torch.randn_like(y)
    y.backward(dy)
    xb = x.clone().requires_grad_(True)
    conv.weight.grad = None
    conv(xb).backward(dy)
    assert torch.equal(xa.grad, xb.grad)
    # shortcut only
    xc = x.clone().requires_grad_(True)
    _, skip = conv.forward_join(xc)
    skip.backward(torch.ones_like(skip))
    assert torch.equal(xc.grad, torch.ones_like(xc))
    # no input grad: weight grad still arrives
    conv.weight.grad = None
    y, skip = conv.forward_join(x)
    (y.float().sum() + skip.float().sum()).backward()
    assert conv.weight.grad is not None
