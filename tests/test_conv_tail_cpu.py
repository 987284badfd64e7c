"""The conv backward's native tail (ops.conv.NATIVE_TAIL) leaves the CPU /
library path alone: a converted conv given a CPU tensor, bf16 included,
runs F.conv2d forward and backward and never asks for the extension,
whichever way the switch stands."""

import pytest
import torch

from ddlbench_amd import ops
from ddlbench_amd.ops import conv as convmod


def test_native_tail_is_the_default():
    assert convmod.NATIVE_TAIL is True


@pytest.mark.parametrize("tail", [True, False], ids=["native", "eager"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_cpu_input_falls_back_without_extension(monkeypatch, tail, dtype):
    def no_ext():
        raise AssertionError("the CPU path must not load the extension")

    monkeypatch.setattr(ops, "require_extension", no_ext)
    monkeypatch.setattr(convmod, "NATIVE_TAIL", tail)
    torch.manual_seed(0)
    ref = torch.nn.Conv2d(16, 24, 3, 1, 1, bias=False).to(dtype)
    ref = ref.to(memory_format=torch.channels_last)
    x0 = torch.randn(2, 16, 6, 7).to(dtype)

    x1 = x0.clone().requires_grad_(True)
    y1 = ref(x1)
    dy = torch.randn_like(y1)
    y1.backward(dy)
    want = (y1.detach(), x1.grad.clone(), ref.weight.grad.clone())

    ref.weight.grad = None
    m = convmod.Conv2dMFMA(ref)
    x2 = x0.clone().requires_grad_(True)
    y2 = m(x2)
    y2.backward(dy)
    assert torch.equal(y2.detach(), want[0])
    assert torch.equal(x2.grad, want[1])
    assert torch.equal(m.weight.grad, want[2])
    y3, skip = m.forward_join(x0)
    assert skip is x0 and torch.equal(y3, want[0])
