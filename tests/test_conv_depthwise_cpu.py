"""Depthwise-conv Python layer (no GPU): eligibility, the Conv2dDepthwise
module's CPU fallback and the opt-in wiring of convert_convs."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.ops.conv import (Conv2dDepthwise, convert_convs,
                                   depthwise_eligible)

BF = torch.bfloat16


def _conv(c=44, k=None, r=5, groups=None, **kw):
    kw.setdefault("padding", r // 2)
    kw.setdefault("bias", False)
    return nn.Conv2d(c, k or c, r, groups=groups or c, **kw)


@pytest.mark.parametrize("conv,dtype,want", [
    (_conv(44, r=5), BF, True),                        # C % 4, NASNet's own
    (_conv(42, r=5), BF, False),                       # C % 4 != 0
    (_conv(88, r=7, stride=2), BF, True),              # stride 2
    (_conv(88, r=7, stride=3), BF, False),             # stride 3
    (_conv(8, r=3), BF, True),                         # K = 3
    (_conv(8, r=1), BF, False),                        # K = 1
    (_conv(8, r=9), BF, False),                        # K = 9
    (_conv(8, r=4, padding=2), BF, False),             # even K
    (nn.Conv2d(8, 8, (3, 5), padding=(1, 2), groups=8, bias=False), BF,
     False),                                           # not square
    (_conv(8, r=5, padding=1), BF, False),             # pad != K/2
    (_conv(8, r=5, padding="same"), BF, False),        # pad given by name
    (_conv(8, r=3, padding=2, dilation=2), BF, False),
    (_conv(8, r=5, bias=True), BF, False),
    (_conv(16, groups=8), BF, False),                  # 2 channels a group
    (_conv(8, 16), BF, False),                         # channel multiplier 2
    (_conv(8, groups=1), BF, False),                   # dense
    (_conv(44, r=5), torch.float32, False),            # fp32 input
])
def test_depthwise_eligible(conv, dtype, want):
    assert depthwise_eligible(conv, dtype) is want


def test_convert_convs_nasnet():
    base = build_model("cifar10", "nasnetamobile")
    keys = list(base.state_dict().keys())
    n_dw = sum(isinstance(m, nn.Conv2d) and m.groups == m.in_channels > 1
               and m.kernel_size in ((5, 5), (7, 7)) for m in base.modules())
    assert n_dw == 64

    def convert(**kw):
        m = build_model("cifar10", "nasnetamobile")
        n = convert_convs(m, **kw)
        assert list(m.state_dict().keys()) == keys
        return n, sum(isinstance(c, Conv2dDepthwise) for c in m.modules())

    n_default, d_default = convert()
    assert (n_default, d_default) == (107, 0)   # the count before the opt-in
    assert convert(depthwise="library") == (n_default, 0)
    assert convert(depthwise="native") == (n_default + n_dw, n_dw)
    with pytest.raises(ValueError):
        convert(depthwise="fastest")


def test_conv2ddepthwise_cpu_fallback_and_shared_weight():
    torch.manual_seed(0)
    conv = _conv(12, r=7, stride=2)
    mod = Conv2dDepthwise(conv)
    assert mod.weight is conv.weight
    x = torch.randn(2, 12, 11, 9)
    want = F.conv2d(x, conv.weight, None, 2, 3, 1, 12)
    assert torch.equal(mod(x), want)
    assert repr(mod).rstrip(")").endswith("[depthwise]")
