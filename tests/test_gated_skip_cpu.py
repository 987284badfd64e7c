"""The gate-slot plumbing leaves every path without a native mask alone:
fp32 CPU blocks and a small ResNet still compute what plain autograd
computes, a slot nobody arms changes nothing, and the packed-bit convention
of the gate (byte i/8, bit i&7) is pinned by a pure-torch emulation."""

import pytest
import torch
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.models import resnet as R
from ddlbench_amd.ops import functional as NF


# ------------------------------------------------- plain-autograd reference
def _ref_bn(bn, x, res=None):
    y = F.batch_norm(x, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
    if res is not None:
        y = y + res
    return F.relu(y) if bn.act == "relu" else y


def _ref_conv(conv, x):
    return F.conv2d(x, conv.weight, None, conv.stride, conv.padding)


def _ref_block(blk, x):
    identity = x
    if blk.downsample is not None:
        identity = _ref_bn(blk.downsample.bn,
                           _ref_conv(blk.downsample.conv, x))
    out = _ref_bn(blk.bn1, _ref_conv(blk.conv1, x))
    if isinstance(blk, R.Bottleneck):
        out = _ref_bn(blk.bn2, _ref_conv(blk.conv2, out))
        return _ref_bn(blk.bn3, _ref_conv(blk.conv3, out), identity)
    return _ref_bn(blk.bn2, _ref_conv(blk.conv2, out), identity)


def _ref_resnet(m, x):
    x = _ref_bn(m.stem.bn, _ref_conv(m.stem.conv, x))
    assert m.stem.pool is None
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            x = _ref_block(blk, x)
    return m.head.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))


def _grads_of(module, x, fn):
    module.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    out = fn(xi)
    loss = out.square().mean()
    loss.backward()
    return loss.detach(), xi.grad, {n: p.grad.clone()
                                    for n, p in module.named_parameters()}


def _assert_same(got, want):
    torch.testing.assert_close(got[0], want[0])
    torch.testing.assert_close(got[1], want[1])
    assert got[2].keys() == want[2].keys()
    for n in want[2]:
        torch.testing.assert_close(got[2][n], want[2][n], msg=n)


_BLOCKS = {
    "bottleneck-identity": lambda: (R.Bottleneck(32, 8), 32),
    "bottleneck-down1": lambda: (R.Bottleneck(16, 8), 16),
    "bottleneck-down2": lambda: (R.Bottleneck(16, 8, stride=2), 16),
    "basic-identity": lambda: (R.BasicBlock(16, 16), 16),
    "basic-down1": lambda: (R.BasicBlock(8, 16), 8),
    "basic-down2": lambda: (R.BasicBlock(8, 16, stride=2), 8),
}


@pytest.mark.parametrize("name", sorted(_BLOCKS))
def test_cpu_block_matches_plain_autograd(name):
    torch.manual_seed(0)
    blk, cin = _BLOCKS[name]()
    x = torch.randn(2, cin, 6, 6)
    _assert_same(_grads_of(blk, x, blk),
                 _grads_of(blk, x, lambda t: _ref_block(blk, t)))


@pytest.mark.parametrize("name", ["bottleneck-identity", "basic-down2"])
def test_cpu_block_with_an_unclaimed_slot(name, monkeypatch):
    """The fork taken with a conv that offers forward_join but falls back
    (a CPU input): the slot is created and passed along, nobody claims or
    arms it, and the block computes what plain autograd computes."""
    from ddlbench_amd.ops.conv import Conv2dMFMA
    torch.manual_seed(0)
    blk, cin = _BLOCKS[name]()
    blk.conv1 = Conv2dMFMA(blk.conv1)
    x = torch.randn(2, cin, 6, 6)
    slots = []
    real = R.GateSlot

    def recording():
        slots.append(real())
        return slots[-1]

    monkeypatch.setattr(R, "_joins", lambda conv1, t: True)
    monkeypatch.setattr(R, "GateSlot", recording)
    got = _grads_of(blk, x, blk)
    assert len(slots) == 1
    assert not slots[0].claimed and not slots[0].armed
    monkeypatch.setenv("DDLB_GATE", "0")
    off = _grads_of(blk, x, blk)
    assert len(slots) == 1, "DDLB_GATE=0 still made a slot"
    want = _grads_of(blk, x, lambda t: _ref_block(blk, t))
    _assert_same(got, want)
    _assert_same(off, want)


def test_cpu_resnet_matches_plain_autograd():
    torch.manual_seed(0)
    m = build_model("cifar10", "resnet18")
    x = torch.randn(2, 3, 16, 16)
    _assert_same(_grads_of(m, x, m),
                 _grads_of(m, x, lambda t: _ref_resnet(m, t)))


# ------------------------------------------------------------ the slot
def test_gate_slot_contract():
    slot = NF.GateSlot()
    assert not slot.claimed and not slot.armed
    slot.claim()
    mask = torch.zeros(2, dtype=torch.uint8)
    dy = torch.randn(16)
    slot.arm(mask, dy)
    assert slot.armed
    assert slot.take(dy) is mask              # the very tensor passes
    assert not slot.armed
    slot.arm(mask, dy)                        # re-arms (retain_graph)
    assert slot.take(dy.view(16)) is mask     # same storage, shape, dtype
    for tampered in (dy + 1, dy.clone(), dy[:8], None):
        slot.arm(mask, dy)
        with pytest.raises(RuntimeError, match="gated shortcut gradient"):
            slot.take(tampered)
        assert not slot.armed
    slot.arm(mask, dy)
    dy.add_(1)                                # accumulated into in place
    with pytest.raises(RuntimeError, match="gated shortcut gradient"):
        slot.take(dy)


def test_gate_env_is_read_per_call(monkeypatch):
    monkeypatch.delenv("DDLB_GATE", raising=False)
    assert NF.gate_enabled()
    monkeypatch.setenv("DDLB_GATE", "0")
    assert not NF.gate_enabled()
    monkeypatch.setenv("DDLB_GATE", "1")
    assert NF.gate_enabled()


# ------------------------------------------------------ bit convention
def test_packed_gate_emulation_keeps_zero_signs():
    """Element i of the addend (memory order) is gated by bit i&7 of byte
    i/8; a gated-off lane is a zero carrying the addend's sign, exactly
    ``bf16(float(dy) * bit)``."""
    torch.manual_seed(0)
    n = 4096
    dy = torch.randn(n).bfloat16()
    dy[::5] = 0.0
    dy[::7] = -0.0
    keep = torch.rand(n) < 0.5
    # pack: bit i&7 of byte i/8
    weights = (1 << torch.arange(8)).to(torch.int32)
    packed = (keep.view(-1, 8).to(torch.int32) * weights).sum(1) \
        .to(torch.uint8)
    assert packed.numel() == n // 8
    # unpack and check the convention element by element
    idx = torch.arange(n)
    bit = (packed.to(torch.int32)[idx // 8] >> (idx & 7)) & 1
    assert torch.equal(bit.bool(), keep)
    want = (dy.float() * keep.float()).bfloat16()
    # the emulation on raw bit patterns: a kept lane passes unchanged, a
    # gated-off lane keeps only the sign bit
    raw = dy.view(torch.int16).to(torch.int32) & 0xFFFF
    emu = torch.where(bit.bool(), raw, raw & 0x8000)
    want_raw = want.view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(emu, want_raw)
    off = ~keep
    assert (want_raw[off & (dy < 0)] == 0x8000).all()      # -0
    assert (want_raw[off & (dy > 0)] == 0).all()           # +0
    assert (want_raw[off] & 0x7FFF == 0).all()
    # the sign of a gated-off zero is visible in the sum with a -0 lane
    acc = torch.full((n,), -0.0).bfloat16()
    s = (acc.float() + want.float()).bfloat16().view(torch.int16)
    assert ((s[off & (dy < 0)].to(torch.int32) & 0xFFFF) == 0x8000).all()
    assert ((s[off & (dy > 0)].to(torch.int32) & 0xFFFF) == 0).all()
