"""Line-conv Python layer (no GPU): eligibility, the Conv2dLine module's CPU
fallback and the opt-in wiring of convert_convs."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.ops.conv import Conv2dLine, convert_convs, line_eligible

BF = torch.bfloat16


def _conv(c=128, k=192, ks=(1, 7), **kw):
    kw.setdefault("padding", (ks[0] // 2, ks[1] // 2))
    kw.setdefault("bias", False)
    return nn.Conv2d(c, k, ks, **kw)


@pytest.mark.parametrize("conv,dtype,want", [
    (_conv(ks=(1, 7)), BF, True),
    (_conv(ks=(7, 1)), BF, True),
    (_conv(ks=(1, 3)), BF, True),
    (_conv(ks=(3, 1)), BF, True),
    (_conv(stride=2), BF, False),
    (_conv(bias=True), BF, False),
    (_conv(ks=(1, 3), padding=(0, 2), dilation=(1, 2)), BF, False),
    (_conv(padding=(0, 0)), BF, False),
    (_conv(c=24), BF, False),
    (_conv(groups=2), BF, False),
    (_conv(ks=(1, 5)), BF, False),                     # T = 5
    (_conv(ks=(7, 7)), BF, False),                     # square
    (_conv(), torch.float32, False),                   # fp32 input
])
def test_line_eligible(conv, dtype, want):
    assert line_eligible(conv, dtype) is want


def test_convert_convs_inception():
    keys = list(build_model("imagenet", "inception3").state_dict().keys())

    def convert(**kw):
        m = build_model("imagenet", "inception3")
        n = convert_convs(m, **kw)
        assert list(m.state_dict().keys()) == keys
        return n, sum(isinstance(c, Conv2dLine) for c in m.modules())

    n_default, l_default = convert()
    assert l_default == 0
    assert convert(line="library") == (n_default, 0)
    assert convert(line="native") == (n_default + 18, 18)
    with pytest.raises(ValueError):
        convert(line="fast")


@pytest.mark.parametrize("ks", [(1, 7), (7, 1)])
def test_conv2dline_cpu_fallback_and_shared_weight(ks):
    torch.manual_seed(0)
    conv = _conv(32, 64, ks)
    mod = Conv2dLine(conv)
    assert mod.weight is conv.weight
    assert mod.kernel_size == ks and mod.padding == conv.padding
    x = torch.randn(2, 32, 9, 11)
    assert torch.equal(mod(x), F.conv2d(x, conv.weight, None, 1,
                                        conv.padding))
    assert repr(mod).rstrip(")").endswith("[line]")
