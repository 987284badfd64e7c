"""HIP kernel numerics vs plain-PyTorch fp32 references. All @gpu.

Every native op is compared against the torch composition of the same op
at fp32 (tight tolerance) and bf16 (loose tolerance)."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"


# ------------------------------------------------------------- BN+act
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5),
                                       (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("act", ["none", "relu", "relu6"])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_act_forward_backward(dtype, tol, act, with_res):
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(0)
    N, C, H, W = 8, 32, 14, 14
    dev = _dev()

    def make_inputs(dt):
        x = torch.randn(N, C, H, W, device=dev, dtype=dt, requires_grad=True)
        res = (torch.randn(N, C, H, W, device=dev, dtype=dt,
                           requires_grad=True) if with_res else None)
        g = torch.rand(C, device=dev) + 0.5
        b = torch.randn(C, device=dev)
        g.requires_grad_(True)
        b.requires_grad_(True)
        return x, res, g, b

    x1, r1, g1, b1 = make_inputs(dtype)
    rm1 = torch.zeros(C, device=dev)
    rv1 = torch.ones(C, device=dev)
    y1 = NF.bn_act(x1, g1, b1, rm1, rv1, True, 0.1, 1e-5, act, r1,
                   backend="native")
    dy = torch.randn_like(y1)
    y1.backward(dy)

    # fp32 torch reference with identical inputs
    x2 = x1.detach().float().clone().requires_grad_(True)
    r2 = (r1.detach().float().clone().requires_grad_(True)
          if with_res else None)
    g2 = g1.detach().clone().requires_grad_(True)
    b2 = b1.detach().clone().requires_grad_(True)
    rm2 = torch.zeros(C, device=dev)
    rv2 = torch.ones(C, device=dev)
    y2 = torch.nn.functional.batch_norm(x2, rm2, rv2, g2, b2, True, 0.1, 1e-5)
    if with_res:
        y2 = y2 + r2
    if act == "relu":
        y2 = torch.relu(y2)
    elif act == "relu6":
        y2 = torch.clamp(y2, 0, 6)
    y2.backward(dy.float())

    torch.testing.assert_close(y1.float(), y2, rtol=tol, atol=tol)
    torch.testing.assert_close(rm1, rm2, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(rv1, rv2, rtol=1e-4, atol=1e-4)
    # relu/relu6 clamp-boundary elements can land on opposite sides of
    # the threshold after bf16 rounding (mask 0 vs 1 on ~1 element per
    # 50k) — exclude a thin boundary band from the dx comparison
    band = torch.ones_like(y2, dtype=torch.bool)
    if act != "none" and dtype is torch.bfloat16:
        band = (y2 - 0.0).abs() > 0.05
        if act == "relu6":
            # bf16 ulp near 6.0 is 0.03125 and the bf16-input BN output
            # can differ from the fp32 reference by a few 1e-2 — any
            # element within 0.3 of the clamp can land on either side
            band &= (y2 - 6.0).abs() > 0.3
    torch.testing.assert_close(x1.grad.float()[band], x2.grad[band],
                               rtol=tol, atol=tol * 10)
    # dgamma/dbeta: a clamp-boundary element whose mask flips between
    # the bf16 kernel and the fp32 reference moves the whole channel's
    # reduction by up to |dy*xhat| of that element — bound the diff by
    # the out-of-band contributions instead of a flat tolerance
    with torch.no_grad():
        invstd_ref = 1.0 / torch.sqrt(x2.view(N, C, -1).float().var(
            dim=(0, 2), unbiased=False).clamp_min(1e-5) + 1e-5)
        xhat_ref = (x2 - x2.mean(dim=(0, 2, 3), keepdim=True)) \
            * invstd_ref.view(1, C, 1, 1)
        oob = (~band).float()
        slack_g = (dy.float().abs() * xhat_ref.abs() * oob) \
            .sum(dim=(0, 2, 3)) + 1e-2 + 1e-3 * g2.grad.abs()
        slack_b = (dy.float().abs() * oob).sum(dim=(0, 2, 3)) \
            + 1e-2 + 1e-3 * b2.grad.abs()
    assert ((g1.grad - g2.grad).abs() <= slack_g + 0.05 *
            g2.grad.abs().max()).all()
    assert ((b1.grad - b2.grad).abs() <= slack_b + 0.05 *
            b2.grad.abs().max()).all()
    if with_res:
        torch.testing.assert_close(r1.grad.float()[band], r2.grad[band],
                                   rtol=tol, atol=tol * 10)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5),
                                       (torch.bfloat16, 2e-2)])
def test_bn_act_channels_last(dtype, tol):
    """NHWC (channels_last) path vs the NCHW fp32 reference."""
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(0)
    N, C, H, W = 8, 64, 14, 14
    dev = _dev()
    x1 = torch.randn(N, C, H, W, device=dev, dtype=dtype).contiguous(
        memory_format=torch.channels_last).requires_grad_(True)
    g1 = (torch.rand(C, device=dev) + 0.5).requires_grad_(True)
    b1 = torch.randn(C, device=dev).requires_grad_(True)
    rm1 = torch.zeros(C, device=dev)
    rv1 = torch.ones(C, device=dev)
    y1 = NF.bn_act(x1, g1, b1, rm1, rv1, True, 0.1, 1e-5, "relu", None,
                   backend="native")
    assert y1.is_contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(y1)
    y1.backward(dy)

    x2 = x1.detach().float().contiguous().requires_grad_(True)
    g2 = g1.detach().clone().requires_grad_(True)
    b2 = b1.detach().clone().requires_grad_(True)
    rm2 = torch.zeros(C, device=dev)
    rv2 = torch.ones(C, device=dev)
    y2 = torch.relu(torch.nn.functional.batch_norm(
        x2, rm2, rv2, g2, b2, True, 0.1, 1e-5))
    y2.backward(dy.float().contiguous())
    torch.testing.assert_close(y1.float().contiguous(), y2, rtol=tol,
                               atol=tol)
    torch.testing.assert_close(rm1, rm2, rtol=1e-4, atol=1e-4)
    band = y2.abs() > 0.05 if dtype is torch.bfloat16 \
        else torch.ones_like(y2, dtype=torch.bool)
    torch.testing.assert_close(x1.grad.float().contiguous()[band],
                               x2.grad[band], rtol=tol, atol=tol * 10)
    torch.testing.assert_close(g1.grad, g2.grad, rtol=1e-3, atol=1e-3)


def test_bn_act_eval_mode():
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(1)
    N, C, H, W = 4, 16, 8, 8
    dev = _dev()
    x = torch.randn(N, C, H, W, device=dev)
    g = torch.rand(C, device=dev) + 0.5
    b = torch.randn(C, device=dev)
    rm = torch.randn(C, device=dev)
    rv = torch.rand(C, device=dev) + 0.5
    y = NF.bn_act(x, g, b, rm.clone(), rv.clone(), False, 0.1, 1e-5, "relu",
                  backend="native")
    ref = torch.relu(torch.nn.functional.batch_norm(
        x, rm, rv, g, b, False, 0.1, 1e-5))
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------- cross entropy
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5),
                                       (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("K", [10, 1000])
def test_cross_entropy(dtype, tol, K):
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(0)
    B = 64
    dev = _dev()
    x1 = torch.randn(B, K, device=dev, dtype=dtype, requires_grad=True)
    t = torch.randint(K, (B,), device=dev)
    loss1 = NF.cross_entropy(x1, t, backend="native")
    loss1.backward()

    x2 = x1.detach().float().clone().requires_grad_(True)
    loss2 = torch.nn.functional.cross_entropy(x2, t)
    loss2.backward()
    torch.testing.assert_close(loss1.float(), loss2, rtol=tol, atol=tol)
    torch.testing.assert_close(x1.grad.float(), x2.grad, rtol=tol,
                               atol=tol)


# ------------------------------------------------- depthwise conv 3x3
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4),
                                       (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_conv(dtype, tol, stride):
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(0)
    N, C, H, W = 4, 24, 15, 15
    dev = _dev()
    x1 = torch.randn(N, C, H, W, device=dev, dtype=dtype, requires_grad=True)
    w1 = torch.randn(C, 1, 3, 3, device=dev, dtype=dtype, requires_grad=True)
    y1 = NF.depthwise_conv3x3(x1, w1, stride, backend="native")
    dy = torch.randn_like(y1)
    y1.backward(dy)

    x2 = x1.detach().float().clone().requires_grad_(True)
    w2 = w1.detach().float().clone().requires_grad_(True)
    y2 = torch.nn.functional.conv2d(x2, w2, None, stride, 1, 1, groups=C)
    y2.backward(dy.float())
    torch.testing.assert_close(y1.float(), y2, rtol=tol, atol=tol)
    torch.testing.assert_close(x1.grad.float(), x2.grad, rtol=tol, atol=tol)
    torch.testing.assert_close(w1.grad.float(), w2.grad, rtol=tol,
                               atol=tol * 10)


# ----------------------------------------------- MFMA implicit-GEMM conv
@pytest.mark.parametrize("shape", [
    # (N, C, H, W, K, R, stride, pad)
    (4, 64, 14, 14, 128, 1, 1, 0),      # 1x1
    (4, 64, 14, 14, 64, 3, 1, 1),       # 3x3 s1
    (4, 64, 15, 15, 128, 3, 2, 1),      # 3x3 s2, odd spatial
    (4, 64, 14, 14, 128, 1, 2, 0),      # 1x1 s2 (degenerate dgrad classes)
    (2, 128, 7, 7, 120, 3, 1, 1),       # Nd not multiple of tile
    (2, 16, 9, 9, 24, 3, 2, 1),         # small C/K (mobilenet-ish)
    # deep-pipeline (v2) coverage: Nd >= 96 both directions, M/Kd tails,
    # multi-column-block Nd, stride-2 parity classes at v2 widths
    (3, 96, 13, 13, 104, 3, 1, 1),      # v2 both dirs, every tail odd
    (2, 128, 9, 9, 512, 1, 1, 0),       # v2 fwd 4 column blocks
    (2, 256, 9, 9, 96, 3, 2, 1),        # v2 dgrad parity classes
    (2, 96, 16, 16, 96, 1, 1, 0),       # v2, Kd=96 (not mult of 64)
    (2, 16, 10, 10, 16, 3, 3, 1),       # stride-3 dgrad: 128-tile gather
])
def test_conv_mfma_fwd_dgrad(shape):
    from ddlbench_amd.ops.conv import conv2d_mfma
    N, C, H, W, K, R, stride, pad = shape
    torch.manual_seed(0)
    dev = _dev()
    x1 = torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w1 = torch.randn(K, C, R, R, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y1 = conv2d_mfma(x1, w1, stride, pad)
    dy = torch.randn_like(y1)
    y1.backward(dy)

    x2 = x1.detach().float().contiguous().requires_grad_(True)
    w2 = w1.detach().float().contiguous().requires_grad_(True)
    y2 = torch.nn.functional.conv2d(x2, w2, None, stride, pad)
    y2.backward(dy.float().contiguous())

    kd = R * R * C
    tol = 0.03 * (kd ** 0.5) / 8  # bf16 accum noise grows with sqrt(K)
    torch.testing.assert_close(y1.float().contiguous(), y2,
                               rtol=5e-2, atol=max(tol, 0.05))
    torch.testing.assert_close(x1.grad.float().contiguous(), x2.grad,
                               rtol=5e-2, atol=max(tol, 0.05))
    torch.testing.assert_close(w1.grad.float().contiguous(), w2.grad,
                               rtol=5e-2, atol=1.0)


@pytest.mark.parametrize("shape", [
    (4, 64, 14, 14, 64, 3, 1, 1),
    (4, 64, 15, 15, 128, 3, 2, 1),
    (2, 32, 9, 9, 24, 1, 1, 0),
])
def test_conv_wgrad_native(shape):
    """Native MFMA weight-grad kernel vs the fp32 torch reference."""
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    N, C, H, W, K, R, stride, pad = shape
    torch.manual_seed(0)
    dev = _dev()
    x = torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    OH = (H + 2 * pad - R) // stride + 1
    dy = torch.randn(N, K, OH, OH, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    dw32 = ext.conv_igemm_wgrad(x, dy, R, R, stride, pad)
    dw = dw32.view(K, R, R, C).permute(0, 3, 1, 2)

    x2 = x.detach().float().contiguous().requires_grad_(True)
    w2 = torch.zeros(K, C, R, R, device=dev, requires_grad=True)
    y2 = torch.nn.functional.conv2d(x2, w2, None, stride, pad)
    y2.backward(dy.float().contiguous())
    # reduction over N*OH*OW in bf16 products: tolerance grows with P
    p = N * OH * OH
    tol = 0.02 * (p ** 0.5)
    torch.testing.assert_close(dw.float(), w2.grad, rtol=5e-2, atol=tol)


def test_conv_mfma_resnet_block_trains():
    """convert_convs on a resnet block; one train step, finite loss."""
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops.conv import convert_convs
    torch.manual_seed(0)
    dev = _dev()
    m = build_model("cifar10", "resnet18").to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    n = convert_convs(m)
    assert n > 10
    x = torch.randn(8, 3, 32, 32, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    y = torch.randint(10, (8,), device=dev)
    out = m(x)
    loss = torch.nn.functional.cross_entropy(out.float(), y)
    loss.backward()
    assert torch.isfinite(loss)


def test_mobilenet_channels_last_train_step():
    """MobileNetV2 bf16 channels_last: full fwd+bwd+fused-SGD step (the
    depthwise weight-grad layout must match the converted param)."""
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops import functional as NF
    from ddlbench_amd.ops.sgd import FusedSGD
    torch.manual_seed(0)
    dev = _dev()
    m = build_model("cifar10", "mobilenetv2").to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, backend="native")
    x = torch.randn(16, 3, 32, 32, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    y = torch.randint(10, (16,), device=dev)
    loss = NF.cross_entropy(m(x), y, backend="native")
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_nhwc_matches_nchw(stride):
    """NHWC depthwise kernels vs the fp32 torch reference."""
    from ddlbench_amd.ops import functional as NF
    torch.manual_seed(0)
    dev = _dev()
    N, C, H, W = 4, 32, 14, 14
    x1 = torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w1 = torch.randn(C, 1, 3, 3, device=dev, dtype=torch.bfloat16,
                     requires_grad=True)
    y1 = NF.depthwise_conv3x3(x1, w1, stride, backend="native")
    assert y1.is_contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(y1)
    y1.backward(dy)
    x2 = x1.detach().float().contiguous().requires_grad_(True)
    w2 = w1.detach().float().clone().requires_grad_(True)
    y2 = torch.nn.functional.conv2d(x2, w2, None, stride, 1, 1, groups=C)
    y2.backward(dy.float().contiguous())
    torch.testing.assert_close(y1.float().contiguous(), y2, rtol=3e-2,
                               atol=3e-2)
    torch.testing.assert_close(x1.grad.float().contiguous(), x2.grad,
                               rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(w1.grad.float(), w2.grad, rtol=3e-2,
                               atol=0.3)


# ------------------------------------------------------------ fused SGD
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_sgd_matches_torch(dtype):
    from ddlbench_amd.ops.sgd import FusedSGD
    torch.manual_seed(0)
    dev = _dev()
    a = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(),
                            torch.nn.Linear(32, 8)).to(dev, dtype)
    b = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(),
                            torch.nn.Linear(32, 8)).to(dev, dtype)
    b.load_state_dict(a.state_dict())
    oa = FusedSGD(a.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4,
                  backend="native")
    ob = FusedSGD(b.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4,
                  backend="torch")
    for _ in range(4):
        x = torch.randn(8, 16, device=dev, dtype=dtype)
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).float().pow(2).sum().backward()
            o.step()
    tol = 1e-6 if dtype == torch.float32 else 2e-2
    for pa, pb in zip(a.parameters(), b.parameters()):
        torch.testing.assert_close(pa, pb, rtol=tol, atol=tol)


# -------------------------------------------------- end-to-end training
def test_model_trains_on_native_kernels():
    """One fwd+bwd+step of resnet18 on the native path; loss is finite
    and decreases over a few steps on a fixed batch."""
    from ddlbench_amd.config import BenchConfig
    from ddlbench_amd.engine import Trainer, make_optimizer
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops import functional as NF
    from ddlbench_amd.ops.modules import set_default_backend

    set_default_backend("native")
    try:
        torch.manual_seed(0)
        dev = _dev()
        model = build_model("cifar10", "resnet18").to(dev)
        cfg = BenchConfig(dataset="cifar10", kernel_backend="native")
        opt = make_optimizer(cfg, model)
        x = torch.randn(16, 3, 32, 32, device=dev)
        y = torch.randint(10, (16,), device=dev)
        losses = []
        for _ in range(8):
            out = model(x)
            loss = NF.cross_entropy(out, y, backend="native")
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert all(torch.isfinite(torch.tensor(losses)))
        assert losses[-1] < losses[0]
    finally:
        set_default_backend("auto")


@pytest.mark.parametrize("shape", [
    (3, 96, 13, 13, 104, 3, 1, 1),
    (2, 128, 9, 9, 512, 1, 1, 0),
    (2, 256, 10, 10, 128, 3, 2, 1),
    (3, 64, 19, 19, 64, 3, 1, 1),    # narrow (256x64 combined-B) variant
    (2, 64, 10, 10, 56, 1, 1, 0),    # narrow, Nd=56 tail
])
def test_conv_v2_matches_v1(shape):
    """The deep-pipeline (v2) and 128-tile (v1) structures accumulate
    the identical K-ordered f32 MFMA chain -> bitwise-equal outputs."""
    import os
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    N, C, H, W, K, R, stride, pad = shape
    torch.manual_seed(0)
    dev = _dev()
    cl = torch.channels_last
    x = torch.randn(N, C, H, W, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=cl)
    w = torch.randn(K, C, R, R, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=cl)
    OH = (H + 2 * pad - R) // stride + 1
    dy = torch.randn(N, K, OH, OH, device=dev,
                     dtype=torch.bfloat16).contiguous(memory_format=cl)
    w_perm = w.permute(1, 2, 3, 0).contiguous()
    prev = os.environ.get("DDLB_CONV_V2")
    try:
        os.environ["DDLB_CONV_V2"] = "1"
        y2 = ext.conv_igemm_fwd(x, w, stride, pad)
        dx2 = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad)
        os.environ["DDLB_CONV_V2"] = "0"
        y1 = ext.conv_igemm_fwd(x, w, stride, pad)
        dx1 = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad)
    finally:
        if prev is None:
            os.environ.pop("DDLB_CONV_V2", None)
        else:
            os.environ["DDLB_CONV_V2"] = prev
    assert torch.equal(y1, y2), "fwd structures disagree"
    assert torch.equal(dx1, dx2), "dgrad structures disagree"


# ------------------------------------------------------- NHWC max-pool
@pytest.mark.parametrize("shape,kgeom", [
    ((4, 64, 112, 112), (3, 2, 1)),     # resnet stem
    ((2, 32, 15, 15), (3, 2, 1)),       # odd spatial
    ((2, 16, 9, 9), (2, 2, 0)),         # even kernel, no pad
    ((2, 24, 14, 14), (3, 1, 1)),       # stride 1 (inception pools)
])
def test_maxpool_nhwc(shape, kgeom):
    from ddlbench_amd.ops.pool import maxpool2d_nhwc
    N, C, H, W = shape
    k, s, p = kgeom
    torch.manual_seed(0)
    dev = _dev()
    x1 = torch.randn(N, C, H, W, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y1 = maxpool2d_nhwc(x1, k, s, p)
    dy = torch.randn_like(y1)
    y1.backward(dy)

    x2 = x1.detach().float().contiguous().requires_grad_(True)
    y2 = torch.nn.functional.max_pool2d(x2, k, s, p)
    y2.backward(dy.float().contiguous())
    # forward max over bf16 values is exact
    torch.testing.assert_close(y1.float().contiguous(), y2, rtol=0,
                               atol=0)
    # dx sums overlapping windows' dy in bf16 vs the reference's fp32
    # accumulate — rounding-level tolerance
    torch.testing.assert_close(x1.grad.float().contiguous(), x2.grad,
                               rtol=2e-2, atol=5e-2)


def test_maxpool_module_swap():
    from ddlbench_amd.ops.conv import convert_convs
    from ddlbench_amd.ops.pool import MaxPool2dNHWC
    from ddlbench_amd.models import build_model
    m = build_model("imagenet", "resnet50").to(_dev()) \
        .to(torch.bfloat16).to(memory_format=torch.channels_last)
    convert_convs(m)
    assert any(isinstance(mm, MaxPool2dNHWC) for mm in m.modules())
    x = torch.randn(2, 3, 224, 224, device=_dev(),
                    dtype=torch.bfloat16).contiguous(
                        memory_format=torch.channels_last)
    out = m(x)
    loss = out.float().sum()
    loss.backward()
    assert torch.isfinite(loss)
