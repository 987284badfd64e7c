"""The shortcut gradient of a residual join is handed over as the join's
output gradient plus its 1-bit ReLU mask and never written.

``conv_igemm_dgrad(..., add=a, gate=m)`` must equal the same call on the
materialised ``bf16(a * bits(m))``, ``bn_act_bwd`` with a foreign gate must
equal ``bn_act_bwd`` on the materialised ``dy * bits(m)``, and blocks must
compute the same gradients with DDLB_GATE=1 and DDLB_GATE=0 — all bit for
bit (compared on the raw 16/32-bit patterns, so zero signs count). A
shortcut gradient that was tampered with must raise. All @gpu."""

import contextlib
import copy
import os

import pytest
import torch

from test_conv_join_gpu import _SHAPES

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


def _bits_nchw(mask, like):
    """The packed mask (byte i/8, bit i&7 over ``like``'s channels_last
    memory order) as a 0/1 fp32 tensor of ``like``'s logical shape."""
    N, C, H, W = like.shape
    shifts = torch.arange(8, device=mask.device, dtype=torch.int32)
    flat = ((mask.to(torch.int32)[:, None] >> shifts) & 1).reshape(
        N, H, W, C)
    return flat.permute(0, 3, 1, 2).float()


def _gated(t, mask):
    """bf16(float(t) * bit): what the join's BN backward stores as dres."""
    return (t.float() * _bits_nchw(mask, t)).to(t.dtype) \
        .contiguous(memory_format=_CL)


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    view = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _masks(numel, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    rnd = torch.randint(0, 256, (numel // 8,), generator=g,
                        dtype=torch.uint8).to(dev)
    return {"random": rnd, "zeros": torch.zeros_like(rnd),
            "ones": torch.full_like(rnd, 255)}


def _signed_zero_mix(t):
    """Every 5th element +0, every 7th -0 (in memory order)."""
    flat = t.permute(0, 2, 3, 1).reshape(-1)
    flat[::5] = 0.0
    flat[::7] = -0.0
    return t


# ----------------------------------------------------------- dgrad kernel
def _int_dgrad_inputs(shape):
    """Small-integer dy and w: every product and partial sum is exact, so
    cancelling terms give accumulator lanes that are exactly zero; a few
    all-zero dy pixels make whole zero rows as well."""
    N, C, H, W, K, R, stride, pad = shape
    g = torch.Generator(device="cpu").manual_seed(0)
    OH = (H + 2 * pad - R) // stride + 1
    dy = torch.randint(-2, 3, (N, K, OH, OH), generator=g).float()
    dy[:, :, ::3, ::2] = 0.0
    w = torch.randint(-2, 3, (K, C, R, R), generator=g).float()
    a = torch.randn(N, C, H, W, generator=g)
    dev = _dev()
    dy = dy.to(dev, torch.bfloat16).contiguous(memory_format=_CL)
    w_perm = w.to(dev, torch.bfloat16).permute(1, 2, 3, 0).contiguous()
    a = _signed_zero_mix(
        a.to(dev, torch.bfloat16).contiguous(memory_format=_CL))
    return dy, w_perm, a


@pytest.mark.parametrize("v2", ["1", "0"])
@pytest.mark.parametrize("shape", _SHAPES)
def test_dgrad_gated_addend_is_exact(shape, v2):
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    N, C, H, W, K, R, stride, pad = shape
    dy, w_perm, a = _int_dgrad_inputs(shape)
    assert (a < 0).any()
    a16 = a.view(torch.int16)
    assert (a16 == 0).any() and (a16 == -32768).any()   # +0 and -0
    a0 = a.clone()
    with _env("DDLB_CONV_V2", v2):
        plain = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad)
        assert (plain == 0).any(), "no accumulator lane is zero"
        for name, m in _masks(a.numel(), a.device).items():
            m0 = m.clone()
            fused = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride,
                                         pad, add=a, gate=m)
            ref = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W, stride, pad,
                                       add=_gated(a, m))
            assert fused.is_contiguous(memory_format=_CL)
            assert torch.equal(fused, ref), name
            assert _same_bits(fused, ref), name
            assert torch.equal(m, m0), "the gate was written"
            if name == "ones":
                with_add = ext.conv_igemm_dgrad(dy, w_perm, N, C, H, W,
                                                stride, pad, add=a)
                assert _same_bits(fused, with_add)
    assert _same_bits(a, a0), "the addend was written"


def test_dgrad_gate_is_checked():
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    shape = (2, 64, 9, 9, 64, 1, 1, 0)
    N, C, H, W, K, R, stride, pad = shape
    dy, w_perm, a = _int_dgrad_inputs(shape)
    m = _masks(a.numel(), a.device)["random"]
    args = (dy, w_perm, N, C, H, W, stride, pad)
    with pytest.raises(RuntimeError):      # legal only together with add
        ext.conv_igemm_dgrad(*args, gate=m)
    with pytest.raises(RuntimeError):      # numel/8 bytes
        ext.conv_igemm_dgrad(*args, add=a, gate=m[:-1])
    with pytest.raises(RuntimeError):      # uint8
        ext.conv_igemm_dgrad(*args, add=a, gate=m.to(torch.int32))
    with pytest.raises(RuntimeError):      # on the device
        ext.conv_igemm_dgrad(*args, add=a, gate=m.cpu())


# -------------------------------------------------------- BN foreign gate
# 8-wide fp32-slab reduce (C <= 512) and the scalar reduce with double
# slabs (C = 1024)
@pytest.mark.parametrize("shape", [(2, 64, 9, 9), (2, 256, 5, 5),
                                   (2, 1024, 3, 3)])
def test_bn_foreign_gate_matches_materialised(shape):
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    dev = _dev()
    N, C, H, W = shape
    torch.manual_seed(0)
    x = torch.randn(shape, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=_CL)
    dy = _signed_zero_mix(torch.randn(
        shape, device=dev, dtype=torch.bfloat16).contiguous(
            memory_format=_CL))
    gamma = torch.randn(C, device=dev).abs() + 0.5
    beta = torch.randn(C, device=dev)
    y, mean, invstd = ext.bn_act_fwd(x, None, gamma, beta, None, None, True,
                                     0.1, 1e-5, 0, True)[:3]
    plan = ext.bn_plan(N, C, H * W, True, 2, 1, True, True)
    assert plan["reduce"] == ("nhwc_vec" if C <= 512 else "nhwc_scalar")
    assert plan["slab"] == ("f32" if C <= 512 else "f64")
    for name, m in _masks(x.numel(), dev).items():
        ref = ext.bn_act_bwd(_gated(dy, m), y, x, mean, invstd, gamma, 0,
                             True, False, True, None)
        got = ext.bn_act_bwd(dy, None, x, mean, invstd, gamma, 0, True,
                             False, True, None, gate=m)
        assert len(got) == len(ref) == 3
        for what, g, r in zip(("dx", "dgamma", "dbeta"), got, ref):
            assert _same_bits(g, r), (name, what)


def test_bn_foreign_gate_is_checked():
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    dev = _dev()
    shape = (2, 64, 5, 5)
    x = torch.randn(shape, device=dev,
                    dtype=torch.bfloat16).contiguous(memory_format=_CL)
    gamma = torch.ones(64, device=dev)
    y, mean, invstd = ext.bn_act_fwd(x, None, gamma, gamma, None, None,
                                     True, 0.1, 1e-5, 0, True)[:3]
    m = _masks(x.numel(), dev)["random"]

    def bwd(t=x, act=0, nhwc=True, msk=None, gate=m, need_dres=False):
        return ext.bn_act_bwd(t, y, t, mean, invstd, gamma, act, True,
                              need_dres, nhwc, msk, gate=gate)
    bwd()                                   # the well-formed call passes
    with pytest.raises(RuntimeError):       # mask size
        bwd(gate=m[:-1])
    with pytest.raises(RuntimeError):       # the layer has its own act
        bwd(act=1)
    with pytest.raises(RuntimeError):       # ... or its own mask
        bwd(msk=m)
    with pytest.raises(RuntimeError):       # bf16 only
        xf = x.float()
        ext.bn_act_bwd(xf, xf, xf, mean, invstd, gamma, 0, True, False,
                       True, None, gate=m)
    with pytest.raises(RuntimeError):       # NHWC only
        xc = x.contiguous()
        ext.bn_act_bwd(xc, xc, xc, mean, invstd, gamma, 0, True, False,
                       False, None, gate=m)


# ------------------------------------------------------------ block level
def _make_block(kind, form):
    from ddlbench_amd.models.resnet import BasicBlock, Bottleneck
    if kind == "bottleneck":
        block, cin = {"identity": (Bottleneck(256, 64), 256),
                      "down1": (Bottleneck(64, 32), 64),
                      "down2": (Bottleneck(64, 32, stride=2), 64)}[form]
    else:
        block, cin = {"identity": (BasicBlock(64, 64), 64),
                      "down1": (BasicBlock(32, 64), 32),
                      "down2": (BasicBlock(32, 64, stride=2), 32)}[form]
    assert (block.downsample is None) == (form == "identity")
    return block, cin


@pytest.fixture
def native_backend():
    from ddlbench_amd.ops.modules import set_default_backend
    set_default_backend("native")
    yield
    set_default_backend("auto")


@pytest.fixture
def takes(monkeypatch):
    """Counts the gates consumers took."""
    from ddlbench_amd.ops import functional as NF
    calls = []
    real = NF.GateSlot.take

    def counting(self, grad):
        calls.append(1)
        return real(self, grad)

    monkeypatch.setattr(NF.GateSlot, "take", counting)
    return calls


def _prepared(kind, form):
    from ddlbench_amd.ops.conv import Conv2dMFMA, convert_convs
    dev = _dev()
    torch.manual_seed(0)
    block, cin = _make_block(kind, form)
    block = block.to(dev).to(torch.bfloat16).to(memory_format=_CL)
    assert convert_convs(block) >= 2
    assert isinstance(block.conv1, Conv2dMFMA)
    x0 = torch.randn(2, cin, 9, 9, device=dev,
                     dtype=torch.bfloat16).contiguous(memory_format=_CL)
    with torch.no_grad():
        dy = torch.randn_like(copy.deepcopy(block)(x0))
    return block, x0, dy


def _grads(blk, x):
    out = {"x": x.grad.clone()}
    for n, p in blk.named_parameters():
        assert p.grad is not None, n
        out[n] = p.grad.clone()
    return out


def _run_block(block, x0, dy, gate, twice=False):
    blk = copy.deepcopy(block)
    x = x0.clone().requires_grad_(True)
    with _env("DDLB_GATE", "1" if gate else "0"):
        y = blk(x)
        y.backward(dy, retain_graph=twice)
        first = _grads(blk, x)
        second = None
        if twice:
            x.grad = None
            blk.zero_grad(set_to_none=True)
            y.backward(dy)
            second = _grads(blk, x)
    torch.cuda.synchronize()
    return y.detach(), first, second


@pytest.mark.parametrize("form", ["identity", "down1", "down2"])
@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_gated_matches_materialised(kind, form, native_backend,
                                          takes):
    block, x0, dy = _prepared(kind, form)
    y_g, g_g, g_g2 = _run_block(block, x0, dy, gate=True, twice=True)
    assert len(takes) == 2, "one gate per backward"
    del takes[:]
    y_m, g_m, _ = _run_block(block, x0, dy, gate=False)
    assert len(takes) == 0
    assert _same_bits(y_g, y_m)
    assert g_g.keys() == g_m.keys() == g_g2.keys()
    for name in g_m:
        assert torch.equal(g_g[name], g_m[name]), name
        assert _same_bits(g_g[name], g_m[name]), name
        # retain_graph: the slot re-arms, the second backward repeats
        assert _same_bits(g_g2[name], g_g[name]), name


def test_join_disabled_leaves_the_slot_unarmed(native_backend, takes):
    block, x0, dy = _prepared("bottleneck", "identity")
    with _env("DDLB_JOIN", "0"):
        _, g_j, _ = _run_block(block, x0, dy, gate=True)
    assert len(takes) == 0
    _, g_m, _ = _run_block(block, x0, dy, gate=False)
    # the unfused join adds in another order: the tolerances of
    # tests/test_conv_join_gpu.py
    torch.testing.assert_close(g_j["x"].float(), g_m["x"].float(),
                               rtol=5e-2, atol=0.05)


# ---------------------------------------------------------------- contract
@pytest.mark.parametrize("form", ["identity", "down2"])
def test_tampered_shortcut_gradient_raises(form, native_backend):
    """A hook that adds to the shortcut gradient: the consumer must refuse
    it (a Python exception before its kernel is launched)."""
    from ddlbench_amd.ops import functional as NF
    blk, x0, dy = _prepared("bottleneck", form)
    x = x0.clone().requires_grad_(True)
    slot = NF.GateSlot()
    if form == "identity":
        out, identity = blk.conv1.forward_join(x, gate=slot)
    else:
        out, skip = blk.conv1.forward_join(x)
        identity = blk.downsample(skip, gate=slot)
    assert slot.claimed
    identity.register_hook(lambda g: g + 1)
    out = blk.bn2(blk.conv2(blk.bn1(out)))
    z = blk.bn3(blk.conv3(out), res=identity, gate=slot)
    with pytest.raises(RuntimeError, match="gated shortcut gradient"):
        z.backward(dy)
    assert not slot.armed
    torch.cuda.synchronize()
