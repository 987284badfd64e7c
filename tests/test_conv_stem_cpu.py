"""Stem-conv Python layer (no GPU): eligibility, the Conv2dStem module's
CPU fallback and the opt-in wiring of convert_convs."""

import pytest
import torch
import torch.nn as nn

from ddlbench_amd.ops.conv import (Conv2dMFMA, Conv2dStem, convert_convs,
                                   stem_eligible)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("R", [3, 7])
def test_stem_eligible_true(C, R):
    assert stem_eligible(nn.Conv2d(C, 64, R, padding=R // 2, bias=False))
    assert stem_eligible(nn.Conv2d(C, 64, R, stride=2, padding=R // 2,
                                   bias=False))


def test_stem_eligible_pad0_stride2():
    assert stem_eligible(nn.Conv2d(3, 64, 3, stride=2, padding=0,
                                   bias=False))


@pytest.mark.parametrize("conv", [
    nn.Conv2d(8, 64, 3, padding=1, bias=False),               # C=8
    nn.Conv2d(3, 12, 3, padding=1, bias=False),               # K=12
    nn.Conv2d(3, 64, 3, padding=1, bias=True),                # bias
    nn.Conv2d(3, 24, 3, padding=1, groups=3, bias=False),     # groups
    nn.Conv2d(3, 64, 3, padding=2, dilation=2, bias=False),   # dilation
    nn.Conv2d(3, 64, 9, padding=4, bias=False),               # R=9
    nn.Conv2d(3, 64, 3, stride=3, padding=1, bias=False),     # stride 3
    nn.Conv2d(3, 64, (3, 5), padding=1, bias=False),          # non-square
], ids=["C8", "K12", "bias", "groups", "dilation", "R9",
        "stride3", "nonsquare"])
def test_stem_eligible_false(conv):
    assert not stem_eligible(conv)


def test_stem_eligible_other_limits():
    # K above the kernel's limit, pad above R/2, non-bf16 input
    assert not stem_eligible(nn.Conv2d(3, 136, 3, padding=1, bias=False))
    assert not stem_eligible(nn.Conv2d(3, 64, 3, padding=2, bias=False))
    assert not stem_eligible(nn.Conv2d(3, 64, 3, padding=1, bias=False),
                             torch.float32)


def test_conv2dstem_cpu_fallback_and_shared_weight():
    torch.manual_seed(0)
    conv = nn.Conv2d(3, 16, 7, stride=2, padding=3, bias=False)
    stem = Conv2dStem(conv)
    assert stem.weight is conv.weight
    x = torch.randn(2, 3, 19, 17)
    torch.testing.assert_close(stem(x), conv(x), rtol=0, atol=0)
    assert repr(stem).rstrip(")").endswith("[stem]")


def _two_convs():
    return nn.Sequential(nn.Conv2d(3, 16, 3, bias=False),
                         nn.Conv2d(16, 16, 3, bias=False))


def test_convert_convs_default_is_library(monkeypatch):
    monkeypatch.delenv("DDLB_STEM", raising=False)
    m = _two_convs()
    assert convert_convs(m) == 1
    assert type(m[0]) is nn.Conv2d
    assert isinstance(m[1], Conv2dMFMA)


def test_convert_convs_stem_native_argument(monkeypatch):
    monkeypatch.delenv("DDLB_STEM", raising=False)
    m = _two_convs()
    assert convert_convs(m, stem="native") == 2
    assert isinstance(m[0], Conv2dStem)
    assert isinstance(m[1], Conv2dMFMA)


def test_convert_convs_stem_env_read_at_call_time(monkeypatch):
    monkeypatch.setenv("DDLB_STEM", "native")
    m = _two_convs()
    assert convert_convs(m) == 2
    assert isinstance(m[0], Conv2dStem)
    # the argument overrides the environment
    m = _two_convs()
    assert convert_convs(m, stem="library") == 1
    assert type(m[0]) is nn.Conv2d


def test_convert_convs_rejects_unknown_stem_mode():
    with pytest.raises(ValueError):
        convert_convs(_two_convs(), stem="fast")


def test_convert_convs_keeps_state_dict_keys():
    m = _two_convs()
    before = list(m.state_dict().keys())
    w0 = m[0].weight
    convert_convs(m, stem="native")
    assert list(m.state_dict().keys()) == before
    assert m[0].weight is w0
