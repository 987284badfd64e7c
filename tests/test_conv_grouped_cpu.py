"""Grouped-conv Python layer (no GPU): eligibility, the Conv2dGrouped
module's CPU fallback and the opt-in wiring of convert_convs."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.ops.conv import (Conv2dGrouped, convert_convs,
                                   grouped_eligible)


def _conv(c=128, k=None, groups=32, r=3, **kw):
    kw.setdefault("padding", 1)
    kw.setdefault("bias", False)
    return nn.Conv2d(c, k or c, r, groups=groups, **kw)


@pytest.mark.parametrize("conv,dtype,want", [
    (_conv(128, groups=32), torch.bfloat16, True),             # Cg 4
    (_conv(256, groups=32, stride=2), torch.bfloat16, True),   # Cg 8, s2
    (_conv(48, groups=3, padding=0), torch.bfloat16, True),    # Cg 16, pad 0
    (_conv(1024, groups=32), torch.bfloat16, True),            # Cg 32
    (_conv(128, groups=32), torch.float32, False),             # fp32 input
    (_conv(128, groups=1), torch.bfloat16, False),             # dense
    (_conv(64, groups=64), torch.bfloat16, False),             # depthwise
    (_conv(64, groups=32), torch.bfloat16, False),             # Cg 2
    (_conv(128, groups=2), torch.bfloat16, False),             # Cg 64
    (_conv(24, groups=3), torch.bfloat16, False),              # C % 16
    (_conv(96, groups=3), torch.bfloat16, True),               # Cg 32, C % 32
    (_conv(64, 128, groups=16), torch.bfloat16, False),        # K != C
    (_conv(128, groups=32, bias=True), torch.bfloat16, False),
    (_conv(128, groups=32, stride=3), torch.bfloat16, False),
    (_conv(128, groups=32, padding=2), torch.bfloat16, False),
    (_conv(128, groups=32, padding=2, dilation=2), torch.bfloat16, False),
    (_conv(128, groups=32, r=5), torch.bfloat16, False),
    (_conv(128, groups=32, r=1, padding=0), torch.bfloat16, False),
])
def test_grouped_eligible(conv, dtype, want):
    assert grouped_eligible(conv, dtype) is want


def test_convert_convs_resnext50(monkeypatch):
    monkeypatch.delenv("DDLB_GROUPED", raising=False)
    base = build_model("imagenet", "resnext50_32x4d")
    keys = list(base.state_dict().keys())

    def convert(**kw):
        m = build_model("imagenet", "resnext50_32x4d")
        n = convert_convs(m, **kw)
        assert list(m.state_dict().keys()) == keys
        return n, sum(isinstance(c, Conv2dGrouped) for c in m.modules())

    n_default, g_default = convert()
    assert (n_default, g_default) == convert(grouped="library")
    assert g_default == 0
    assert convert(grouped="native") == (n_default + 16, 16)
    # the environment variable is read at call time; the argument wins
    monkeypatch.setenv("DDLB_GROUPED", "native")
    assert convert() == (n_default + 16, 16)
    assert convert(grouped="library") == (n_default, 0)
    with pytest.raises(ValueError):
        convert(grouped="fast")


def test_conv2dgrouped_cpu_fallback_and_shared_weight():
    torch.manual_seed(0)
    conv = _conv(32, groups=4, stride=2)
    mod = Conv2dGrouped(conv)
    assert mod.weight is conv.weight
    x = torch.randn(2, 32, 11, 9)
    want = F.conv2d(x, conv.weight, None, 2, 1, 1, 4)
    torch.testing.assert_close(mod(x), want, rtol=0, atol=0)
    assert repr(mod).rstrip(")").endswith("[grouped]")
