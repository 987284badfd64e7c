"""Native NHWC max-pool and average pools: autograd bridges + module swaps.

Average pools (csrc/avgpool.hip, opt-in through
``convert_convs(avgpool="native")``): nn.AvgPool2d of (k, stride, pad) in
{(3,1,1), (3,2,1), (2,2,0)} with PyTorch's defaults and
nn.AdaptiveAvgPool2d(1); bf16 channels_last, C % 4 == 0; backward needs
nothing but the geometry.

Max-pool: the resnet stem's MaxPool2d was the last sizeable torch-library
kernel on the ResNet step (at::max_pool_backward_nhwc ~0.8 ms of ~30 ms).
Forward stores a per-channel argmax byte; backward gathers dy per input
pixel from its covering windows (no zero-init + scatter).
Eligibility: bf16 channels_last, square kernel/stride/pad, dilation 1,
C % 8 == 0."""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd import ops as _ops

_CL = torch.channels_last


class _MaxPoolNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        y, idx = ext.maxpool_fwd(x, k, stride, pad)
        ctx.save_for_backward(idx)
        ctx.geom = (x.shape[2], x.shape[3], k, stride, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        (idx,) = ctx.saved_tensors
        H, W, k, stride, pad = ctx.geom
        dx = ext.maxpool_bwd(dy.contiguous(memory_format=_CL), idx,
                             H, W, k, stride, pad)
        return dx, None, None, None


def maxpool2d_nhwc(x, k, stride, pad):
    return _MaxPoolNHWC.apply(x, k, stride, pad)


def maxpool_eligible(m: nn.MaxPool2d) -> bool:
    def _sq(v):
        return v if isinstance(v, int) else (
            v[0] if v[0] == v[1] else None)
    k = _sq(m.kernel_size)
    s = _sq(m.stride if m.stride is not None else m.kernel_size)
    p = _sq(m.padding)
    d = _sq(m.dilation)
    return None not in (k, s, p) and d in (1, None) \
        and not m.ceil_mode and k <= 5


class MaxPool2dNHWC(nn.Module):
    """Drop-in for an eligible nn.MaxPool2d on the native kernel."""

    def __init__(self, m: nn.MaxPool2d):
        super().__init__()

        def _sq(v):
            return v if isinstance(v, int) else v[0]
        self.k = _sq(m.kernel_size)
        self.stride = _sq(m.stride if m.stride is not None
                          else m.kernel_size)
        self.pad = _sq(m.padding)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16 \
                and x.shape[1] % 8 == 0:
            return maxpool2d_nhwc(x, self.k, self.stride, self.pad)
        return F.max_pool2d(x, self.k, self.stride, self.pad)

    def extra_repr(self):
        return f"k={self.k}, stride={self.stride}, pad={self.pad} [nhwc]"


class _AvgPoolNHWC(torch.autograd.Function):
    """Windowed average pool on csrc/avgpool.hip; saves only the
    geometry."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        ctx.geom = (x.shape[2], x.shape[3], k, stride, pad)
        return ext.avgpool_fwd(x, k, stride, pad)

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        dx = ext.avgpool_bwd(dy.contiguous(memory_format=_CL), *ctx.geom)
        return dx, None, None, None


class _GlobalAvgPoolNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        ctx.hw = (x.shape[2], x.shape[3])
        return ext.global_avgpool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        return ext.global_avgpool_bwd(dy.contiguous(memory_format=_CL),
                                      *ctx.hw)


def avgpool2d_nhwc(x, k, stride, pad):
    """F.avg_pool2d(x, k, stride, pad) for (k, stride, pad) in
    {(3,1,1), (3,2,1), (2,2,0)} on the native kernels."""
    return _AvgPoolNHWC.apply(x, k, stride, pad)


def global_avgpool_nhwc(x):
    """F.adaptive_avg_pool2d(x, 1) on the native kernels."""
    return _GlobalAvgPoolNHWC.apply(x)


_AVG_GEOMS = ((3, 1, 1), (3, 2, 1), (2, 2, 0))


def _avg_geom(m: nn.AvgPool2d):
    def _sq(v):
        return v if isinstance(v, int) else (
            v[0] if len(v) == 2 and v[0] == v[1] else None)
    return (_sq(m.kernel_size),
            _sq(m.stride if m.stride is not None else m.kernel_size),
            _sq(m.padding))


def avgpool_eligible(m: nn.Module) -> bool:
    """True for an nn.AvgPool2d of a supported geometry with PyTorch's
    defaults (count_include_pad, no ceil_mode, no divisor override) and for
    an nn.AdaptiveAvgPool2d of output size 1."""
    if isinstance(m, nn.AdaptiveAvgPool2d):
        return m.output_size in (1, (1, 1))
    return (isinstance(m, nn.AvgPool2d) and _avg_geom(m) in _AVG_GEOMS
            and m.count_include_pad and not m.ceil_mode
            and m.divisor_override is None)


def _native_avg(x) -> bool:
    return x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 \
        and x.shape[1] % 4 == 0


class AvgPool2dNHWC(nn.Module):
    """Drop-in for an avgpool_eligible nn.AvgPool2d on the native
    kernel."""

    def __init__(self, m: nn.AvgPool2d):
        super().__init__()
        self.k, self.stride, self.pad = _avg_geom(m)

    def forward(self, x):
        if _native_avg(x):
            return avgpool2d_nhwc(x, self.k, self.stride, self.pad)
        return F.avg_pool2d(x, self.k, self.stride, self.pad)

    def extra_repr(self):
        return f"k={self.k}, stride={self.stride}, pad={self.pad} [nhwc]"


class GlobalAvgPoolNHWC(nn.Module):
    """Drop-in for nn.AdaptiveAvgPool2d(1) on the native kernel."""

    def forward(self, x):
        if _native_avg(x):
            return global_avgpool_nhwc(x)
        return F.adaptive_avg_pool2d(x, 1)


def convert_avgpools(model: nn.Module) -> int:
    """Swap avgpool_eligible children. Returns conversion count; a module
    instance that several parents hold is swapped in each and counted
    once."""
    swapped = {}
    for parent in model.modules():
        for name, child in list(parent.named_children()):
            if isinstance(child, (nn.AvgPool2d, nn.AdaptiveAvgPool2d)) \
                    and avgpool_eligible(child):
                if id(child) not in swapped:
                    swapped[id(child)] = (
                        GlobalAvgPoolNHWC()
                        if isinstance(child, nn.AdaptiveAvgPool2d)
                        else AvgPool2dNHWC(child))
                setattr(parent, name, swapped[id(child)])
    return len(swapped)


def convert_maxpools(model: nn.Module) -> int:
    """Swap eligible nn.MaxPool2d children. Returns conversion count."""
    count = 0
    for parent in model.modules():
        for name, child in list(parent.named_children()):
            if isinstance(child, nn.MaxPool2d) and maxpool_eligible(child):
                setattr(parent, name, MaxPool2dNHWC(child))
                count += 1
    return count
