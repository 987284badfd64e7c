"""The residual-join wiring leaves the CPU / library path alone: blocks
whose conv1 offers no ``forward_join`` (or whose input is not a bf16
device tensor) run the plain fork, and parameter names are unchanged."""

import json
import os

import pytest
import torch

from ddlbench_amd.models import build_model
from ddlbench_amd.models.resnet import BasicBlock, Bottleneck, _joins

_GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                       "resnet_state_dict_keys.json")


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_state_dict_keys_unchanged(arch):
    with open(_GOLDEN) as f:
        want = json.load(f)[arch]
    assert list(build_model("cifar10", arch).state_dict().keys()) == want


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_resnet_cpu_forward_backward(arch):
    torch.manual_seed(0)
    m = build_model("cifar10", arch)
    x = torch.randn(2, 3, 32, 32, requires_grad=True)
    out = m(x)
    assert out.shape == (2, 10)
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    for name, p in m.named_parameters():
        assert p.grad is not None, name
    n_blocks = sum(isinstance(b, (BasicBlock, Bottleneck))
                   for b in m.modules())
    assert len(m.to_sequential()) == n_blocks + 2


def test_plain_convs_and_cpu_inputs_do_not_join():
    from ddlbench_amd.ops.conv import Conv2dMFMA
    conv = torch.nn.Conv2d(8, 8, 1, bias=False)
    x = torch.randn(1, 8, 4, 4)
    assert not _joins(conv, x)
    assert not _joins(Conv2dMFMA(conv), x)
    assert not _joins(Conv2dMFMA(conv), x.bfloat16())


def test_converted_block_on_cpu_input_falls_back():
    """A converted conv still takes F.conv2d for a CPU fp32 input, and
    forward_join hands back the input itself."""
    from ddlbench_amd.ops.conv import Conv2dMFMA
    torch.manual_seed(0)
    blk = Bottleneck(64, 16)
    ref_in = torch.randn(2, 64, 8, 8)
    ref = blk(ref_in)
    blk.conv1 = Conv2dMFMA(blk.conv1)
    y, skip = blk.conv1.forward_join(ref_in)
    assert skip is ref_in
    out = blk(ref_in)
    torch.testing.assert_close(out, ref)
