"""Average-pool bridge without a GPU: eligibility, the converter's counts
and keys, bit-equal values against the functional form the models used
before their pools became modules, and the drop-ins' CPU fallback."""

import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.ops.conv import convert_convs
from ddlbench_amd.ops.pool import (AvgPool2dNHWC, GlobalAvgPoolNHWC,
                                   avgpool_eligible, convert_avgpools)


@pytest.mark.parametrize("module,want", [
    (nn.AvgPool2d(3, 1, 1), True),
    (nn.AvgPool2d(3, 2, 1), True),
    (nn.AvgPool2d(2), True),
    (nn.AvgPool2d((3, 3), (2, 2), (1, 1)), True),
    (nn.AvgPool2d((2, 2)), True),
    (nn.AdaptiveAvgPool2d(1), True),
    (nn.AdaptiveAvgPool2d((1, 1)), True),
    (nn.AvgPool2d(3, 1, 1, count_include_pad=False), False),
    (nn.AvgPool2d(3, 2, 1, ceil_mode=True), False),
    (nn.AvgPool2d(2, divisor_override=3), False),
    (nn.AvgPool2d(3, 1, 0), False),
    (nn.AvgPool2d(5, 1, 2), False),
    (nn.AvgPool2d((3, 2), 1, 1), False),
    (nn.AvgPool2d(3, (2, 1), 1), False),
    (nn.AdaptiveAvgPool2d(7), False),
    (nn.AdaptiveAvgPool2d((1, 2)), False),
    (nn.MaxPool2d(3, 1, 1), False),
])
def test_avgpool_eligible(module, want):
    assert avgpool_eligible(module) is want


class _Functional(nn.Module):
    """The functional call a model made before its pool became ``m``."""

    def __init__(self, m):
        super().__init__()
        self.geom = None if isinstance(m, nn.AdaptiveAvgPool2d) else (
            m.kernel_size, m.stride, m.padding)

    def forward(self, x):
        if self.geom is None:
            return F.adaptive_avg_pool2d(x, 1)
        return F.avg_pool2d(x, *self.geom)


@pytest.mark.parametrize("arch,size,pools", [
    ("inception3", 96, 7), ("nasnetamobile", 32, 17), ("densenet121", 64, 4)])
def test_convert_counts_keys_values(arch, size, pools):
    torch.manual_seed(0)
    model = build_model("imagenet", arch).eval()
    keys = list(model.state_dict())
    assert sum(avgpool_eligible(m) for m in model.modules()) == pools
    twins = {mode: copy.deepcopy(model) for mode in
             ("default", "library", "native")}
    base = convert_convs(twins["default"])
    assert convert_convs(twins["library"], avgpool="library") == base
    assert convert_convs(twins["native"], avgpool="native") == base + pools
    swapped = [m for m in twins["native"].modules()
               if isinstance(m, (AvgPool2dNHWC, GlobalAvgPoolNHWC))]
    assert len(swapped) == pools
    for parent in twins["default"].modules():
        for name, child in list(parent.named_children()):
            if avgpool_eligible(child):
                setattr(parent, name, _Functional(child))
    x = torch.randn(2, 3, size, size)
    with torch.no_grad():
        want = twins["default"](x)
        for mode in ("library", "native"):
            assert list(twins[mode].state_dict()) == keys
            assert torch.equal(twins[mode](x), want)
            assert torch.equal(twins[mode].to_sequential()(x), want)


def test_shared_instance_counts_once():
    model = build_model("imagenet", "densenet121")
    seq = model.to_sequential()
    both = nn.ModuleList([model, seq])   # model.pool is seq[-1].pool
    assert convert_avgpools(both) == 4
    assert seq[-1].pool is model.pool
    assert isinstance(model.pool, GlobalAvgPoolNHWC)


def test_unknown_backend_is_value_error():
    with pytest.raises(ValueError):
        convert_convs(nn.Sequential(nn.AvgPool2d(2)), avgpool="fastest")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dropins_fall_back_on_cpu(dtype):
    x = torch.randn(2, 8, 7, 9).to(dtype)
    for geom in ((3, 1, 1), (3, 2, 1), (2, 2, 0)):
        m = AvgPool2dNHWC(nn.AvgPool2d(*geom))
        assert torch.equal(m(x), F.avg_pool2d(x, *geom))
    assert torch.equal(GlobalAvgPoolNHWC()(x), F.adaptive_avg_pool2d(x, 1))
