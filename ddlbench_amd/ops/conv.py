"""MFMA implicit-GEMM convolution: autograd bridge + model converter.

Forward and data-grad run on the hand-written NHWC bf16 kernels
(csrc/conv_mfma*.hip) and the weight-grad on the transpose-read kernel
(csrc/conv_wgrad.hip) — the full conv triple is in-tree.

Eligibility: bf16, channels_last, groups=1, dilation=1, C%8==0, K%8==0.
``convert_convs(model)`` swaps every eligible nn.Conv2d for Conv2dMFMA.

Stem convs (C < 8) stay on the library path by default; with
``DDLB_STEM=native`` (or ``convert_convs(model, stem="native")``) they run
the small-C kernels of csrc/conv_stem.hip (forward + weight-grad) through
``Conv2dStem``.

Grouped 3x3 convs (ResNeXt's conv2) likewise stay on the library by
default; ``DDLB_GROUPED=native`` (or ``convert_convs(model,
grouped="native")``) runs the forward, data-grad and weight-grad kernels of
csrc/conv_grouped.hip through ``Conv2dGrouped``.

Depthwise KxK convs (NASNet's 5x5 / 7x7 separable convs) stay on the
library too; ``convert_convs(model, depthwise="native")`` runs the forward,
data-grad and weight-grad kernels of csrc/conv_depthwise.hip through
``Conv2dDepthwise``. That choice is an argument only: no environment
variable selects it.

The (1,7) / (7,1) convs of Inception's factorised blocks (and (1,3) /
(3,1)) are not square, so ``mfma_eligible`` leaves them to the library;
``convert_convs(model, line="native")`` runs the forward, data-grad and
weight-grad kernels of csrc/conv_line.hip through ``Conv2dLine``. Also an
argument only.

Every DDLB_* switch here is a row of ``ops.switches``: DDLB_CONV_TAIL is
resolved once at import (``NATIVE_TAIL``), DDLB_JOIN per forward, and
DDLB_STEM, DDLB_GROUPED and DDLB_MAXPOOL per ``convert_convs`` call."""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd import ops as _ops
from ddlbench_amd.ops.switches import check, enabled, resolve

# The backward's layout/dtype tail runs in native kernels: the dgrad
# weight layout is one tiled transpose (conv_weight_dgrad_layout) and the
# weight-grad kernels write the weight's dtype and layout themselves
# (conv_igemm_wgrad_bf16). False restores the eager-tensor tail (a strided
# permute copy, fp32 dw + cast) — same values, kept for comparison.
NATIVE_TAIL = resolve("conv_tail") == "native"

_CL = torch.channels_last


def _dw_to_weight_layout(dw32, weight):
    """fp32 (K, R*S*C) memory -> logical (K,C,R,S) channels_last in the
    weight's dtype."""
    K, C, R, S = weight.shape
    return dw32.view(K, R, S, C).permute(0, 3, 1, 2).to(weight.dtype)


def _conv_backward(ctx, dy, add=None, gate=None):
    """dx (+ add, fused into the dgrad epilogue) and dw of a native conv.
    ``gate`` is the 1-bit mask still to be applied to ``add``."""
    ext = _ops.require_extension()
    x, weight = ctx.saved_tensors
    dy = dy.contiguous(memory_format=_CL)
    dx = dw = None
    if ctx.needs_input_grad[0]:
        # (K,C,R,S) logical -> (C,R,S,K) memory for the dgrad B tile
        if NATIVE_TAIL and (weight.is_contiguous(memory_format=_CL)
                            or weight.is_contiguous()):
            w_perm = ext.conv_weight_dgrad_layout(weight)
        else:
            w_perm = weight.permute(1, 2, 3, 0).contiguous()
        dx = ext.conv_igemm_dgrad(dy, w_perm, x.size(0), x.size(1),
                                  x.size(2), x.size(3), ctx.stride,
                                  ctx.pad, add, gate)
    if ctx.needs_input_grad[1]:
        if NATIVE_TAIL and weight.dtype == torch.bfloat16:
            dw = ext.conv_igemm_wgrad_bf16(x, dy, weight.shape[2],
                                           weight.shape[3], ctx.stride,
                                           ctx.pad)
        else:
            dw = _dw_to_weight_layout(
                ext.conv_igemm_wgrad(x, dy, weight.shape[2],
                                     weight.shape[3], ctx.stride,
                                     ctx.pad), weight)
    return dx, dw


class _ConvMFMA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        w = weight.contiguous(memory_format=_CL)
        y = ext.conv_igemm_fwd(x, w, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dw = _conv_backward(ctx, dy)
        return dx, dw, None, None


def conv2d_mfma(x, weight, stride=1, pad=0):
    return _ConvMFMA.apply(x, weight, stride, pad)


class _ConvMFMAJoin(torch.autograd.Function):
    """Conv at a residual fork: returns ``(y, x)`` — the conv output and
    the input passed through as the shortcut's source (an alias, no copy).
    Both gradients that meet at ``x`` then arrive at this one node, and
    the backward hands the shortcut's to the dgrad kernel as its epilogue
    addend instead of leaving a separate bf16 add to autograd. The caller
    guarantees ``x`` is channels_last (``Conv2dMFMA.forward_join``), so
    nothing beyond what ``_ConvMFMA`` saves is kept alive.

    ``slot`` (a ``functional.GateSlot`` or None) makes this node the
    consumer of the join's gated shortcut gradient: an armed slot means
    ``dskip`` is the join's own output gradient, and the dgrad epilogue
    applies the slot's mask to it."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad, slot=None):
        ext = _ops.require_extension()
        w = weight.contiguous(memory_format=_CL)
        y = ext.conv_igemm_fwd(x, w, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.pad = pad
        ctx.slot = slot
        if slot is not None:
            slot.claim()
        # an unused shortcut arrives as dskip=None, not as a zero tensor
        ctx.set_materialize_grads(False)
        return y, x

    @staticmethod
    def backward(ctx, dy, dskip):
        gate = None
        if ctx.slot is not None and ctx.slot.armed:
            gate = ctx.slot.take(dskip)
        if dy is None:
            if gate is not None:
                raise RuntimeError(
                    "gated shortcut gradient: the conv output of a "
                    "forward_join with a gate slot must be used")
            # only the shortcut was used: its gradient passes through
            return dskip, None, None, None, None
        if dskip is not None:
            dskip = dskip.contiguous(memory_format=_CL)
        dx, dw = _conv_backward(ctx, dy, dskip, gate)
        return dx, dw, None, None, None


def join_enabled() -> bool:
    """DDLB_JOIN=0 (read per call) restores the unfused residual join."""
    return enabled("join")


def mfma_eligible(conv: nn.Conv2d, x_dtype=torch.bfloat16) -> bool:
    return (x_dtype == torch.bfloat16
            and conv.groups == 1
            and conv.dilation == (1, 1)
            and conv.bias is None
            and conv.in_channels % 8 == 0
            and conv.out_channels % 8 == 0
            and conv.stride[0] == conv.stride[1]
            and conv.padding[0] == conv.padding[1]
            and conv.kernel_size[0] == conv.kernel_size[1])


class _NativeConv2d(nn.Module):
    """Drop-in for a square, bias-free nn.Conv2d. Shares the conv's weight
    Parameter, so state_dict keys are unchanged; bf16 device inputs run
    the subclass's native kernel, anything else F.conv2d."""

    tag = ""

    def __init__(self, conv: nn.Conv2d):
        super().__init__()
        self.in_channels = conv.in_channels
        self.out_channels = conv.out_channels
        self.kernel_size = conv.kernel_size
        self.stride = conv.stride[0]
        self.padding = conv.padding[0]
        self.weight = conv.weight

    def native(self, x):
        raise NotImplementedError

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16:
            return self.native(x)
        return F.conv2d(x, self.weight, None, self.stride, self.padding)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, "
                f"k={self.kernel_size}, stride={self.stride}, "
                f"pad={self.padding} [{self.tag}]")


class Conv2dMFMA(_NativeConv2d):
    """Drop-in for an eligible nn.Conv2d, running the MFMA kernel."""

    tag = "mfma"

    def native(self, x):
        return conv2d_mfma(x, self.weight, self.stride, self.padding)

    def forward_join(self, x, gate=None):
        """``(conv(x), skip)`` for a block whose input also feeds its
        shortcut: take the shortcut from ``skip`` and the two gradients
        meeting at ``x`` are summed in the dgrad epilogue. Inputs the
        fused path does not cover (not a channels_last bf16 device
        tensor, or DDLB_JOIN=0) get the plain conv and ``x`` itself.

        ``gate`` is the block's ``functional.GateSlot`` when ``skip``
        goes straight into the residual join: the fused path claims it
        and its backward applies the join's mask to the shortcut
        gradient; the plain path leaves it unclaimed."""
        if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.is_contiguous(memory_format=_CL) and join_enabled()):
            return _ConvMFMAJoin.apply(x, self.weight, self.stride,
                                       self.padding, gate)
        return self.forward(x), x


class _ConvStem(torch.autograd.Function):
    """Small-C stem conv: native forward and weight-grad (cast back to the
    weight dtype). There is no native data-grad — stem inputs are data; if
    the input does require a gradient, dx comes from the library
    (aten.convolution_backward)."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        w = weight.contiguous(memory_format=_CL)
        y = ext.conv_stem_fwd(x, w, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.ops.aten.convolution_backward(
                dy, x, weight, None, [ctx.stride, ctx.stride],
                [ctx.pad, ctx.pad], [1, 1], False, [0, 0], 1,
                [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            dw = _dw_to_weight_layout(
                ext.conv_stem_wgrad(x, dy, weight.shape[2], weight.shape[3],
                                    ctx.stride, ctx.pad), weight)
        return dx, dw, None, None


def conv2d_stem(x, weight, stride=1, pad=0):
    return _ConvStem.apply(x, weight, stride, pad)


def stem_eligible(conv: nn.Conv2d, x_dtype=torch.bfloat16) -> bool:
    """True for the shapes csrc/conv_stem.hip supports: C in 1..4, square
    3/5/7 kernel, stride 1 or 2, 0 <= pad <= R/2, K % 8 == 0, K <= 128,
    no bias, groups=1, dilation=1."""
    return (x_dtype == torch.bfloat16
            and conv.groups == 1
            and conv.dilation == (1, 1)
            and conv.bias is None
            and 1 <= conv.in_channels <= 4
            and conv.out_channels % 8 == 0
            and 8 <= conv.out_channels <= 128
            and conv.kernel_size[0] == conv.kernel_size[1]
            and conv.kernel_size[0] in (3, 5, 7)
            and conv.stride[0] == conv.stride[1]
            and conv.stride[0] in (1, 2)
            and not isinstance(conv.padding, str)
            and conv.padding[0] == conv.padding[1]
            and 0 <= conv.padding[0] <= conv.kernel_size[0] // 2)


class Conv2dStem(_NativeConv2d):
    """Drop-in for a stem_eligible nn.Conv2d, running the stem kernels."""

    tag = "stem"

    def native(self, x):
        return conv2d_stem(x, self.weight, self.stride, self.padding)


class _ConvGrouped(torch.autograd.Function):
    """Grouped 3x3 conv on the kernels of csrc/conv_grouped.hip: forward,
    data-grad and weight-grad (bf16, in the weight's layout), each
    backward direction only when its gradient is needed."""

    @staticmethod
    def forward(ctx, x, weight, groups, stride, pad):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        w = weight.contiguous(memory_format=_CL)
        y = ext.conv_grouped_fwd(x, w, groups, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.groups = groups
        ctx.stride = stride
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = ext.conv_grouped_dgrad(
                dy, weight.contiguous(memory_format=_CL), x.size(0),
                x.size(1), x.size(2), x.size(3), ctx.groups, ctx.stride,
                ctx.pad)
        if ctx.needs_input_grad[1]:
            dw = ext.conv_grouped_wgrad(x, dy, ctx.groups, ctx.stride,
                                        ctx.pad)
        return dx, dw, None, None, None


def conv2d_grouped(x, weight, groups, stride=1, pad=0):
    return _ConvGrouped.apply(x, weight, groups, stride, pad)


def grouped_eligible(conv: nn.Conv2d, x_dtype=torch.bfloat16) -> bool:
    """True for the problems csrc/conv_grouped.hip supports: groups > 1,
    as many output as input channels, C/groups in {4, 8, 16, 32}, C a
    multiple of 16 (32 for C/groups = 32), 3x3, stride 1 or 2, pad 0 or 1,
    dilation 1, no bias."""
    cg = conv.in_channels // conv.groups
    return (x_dtype == torch.bfloat16
            and conv.groups > 1
            and conv.in_channels == conv.out_channels
            and cg in (4, 8, 16, 32)
            and conv.in_channels % (32 if cg == 32 else 16) == 0
            and conv.dilation == (1, 1)
            and conv.bias is None
            and conv.kernel_size == (3, 3)
            and conv.stride in ((1, 1), (2, 2))
            and conv.padding in ((0, 0), (1, 1)))


class Conv2dGrouped(_NativeConv2d):
    """Drop-in for a grouped_eligible nn.Conv2d, running the grouped
    kernels."""

    tag = "grouped"

    def __init__(self, conv: nn.Conv2d):
        super().__init__(conv)
        self.groups = conv.groups

    def native(self, x):
        return conv2d_grouped(x, self.weight, self.groups, self.stride,
                              self.padding)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16:
            return self.native(x)
        return F.conv2d(x, self.weight, None, self.stride, self.padding,
                        1, self.groups)


class _ConvDepthwise(torch.autograd.Function):
    """Depthwise KxK conv (pad K/2) on the kernels of
    csrc/conv_depthwise.hip: forward, data-grad and weight-grad (bf16, the
    weight's (C,1,K,K) memory), each backward direction only when its
    gradient is needed."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        y = ext.conv_depthwise_fwd(x, weight.contiguous(), stride)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = ext.conv_depthwise_dgrad(dy, weight.contiguous(), x.size(0),
                                          x.size(1), x.size(2), x.size(3),
                                          ctx.stride)
        if ctx.needs_input_grad[1]:
            # (C,1,K,K): dense memory is the same in every layout, so the
            # weight's own strides describe the kernel's output
            dw = ext.conv_depthwise_wgrad(x, dy, weight.shape[2], ctx.stride) \
                .as_strided(weight.shape, weight.stride())
        return dx, dw, None


def conv2d_depthwise(x, weight, stride=1):
    return _ConvDepthwise.apply(x, weight, stride)


def depthwise_eligible(conv: nn.Conv2d, x_dtype=torch.bfloat16) -> bool:
    """True for the problems csrc/conv_depthwise.hip supports: groups == C
    in == C out, C % 4 == 0, square 3/5/7 kernel, pad K/2, stride 1 or 2,
    dilation 1, no bias."""
    k = conv.kernel_size[0]
    return (x_dtype == torch.bfloat16
            and conv.groups == conv.in_channels == conv.out_channels
            and conv.in_channels % 4 == 0
            and conv.dilation == (1, 1)
            and conv.bias is None
            and conv.kernel_size in ((3, 3), (5, 5), (7, 7))
            and conv.stride in ((1, 1), (2, 2))
            and conv.padding == (k // 2, k // 2))


class Conv2dDepthwise(_NativeConv2d):
    """Drop-in for a depthwise_eligible nn.Conv2d, running the depthwise
    kernels."""

    tag = "depthwise"

    def __init__(self, conv: nn.Conv2d):
        super().__init__(conv)
        self.groups = conv.groups

    def native(self, x):
        return conv2d_depthwise(x, self.weight, self.stride)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.bfloat16:
            return self.native(x)
        return F.conv2d(x, self.weight, None, self.stride, self.padding,
                        1, self.groups)


class _ConvLine(torch.autograd.Function):
    """(1,T) / (T,1) conv (stride 1, pad T/2 along the filter) on the
    kernels of csrc/conv_line.hip: forward, data-grad (the forward kernel
    on the (C,R,S,K) weight image, taps reversed) and weight-grad (bf16, in
    the weight's layout), each backward direction only when its gradient is
    needed."""

    @staticmethod
    def forward(ctx, x, weight):
        ext = _ops.require_extension()
        x = x.contiguous(memory_format=_CL)
        y = ext.conv_line_fwd(x, weight.contiguous(memory_format=_CL))
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            w_perm = ext.conv_weight_dgrad_layout(
                weight.contiguous(memory_format=_CL))
            dx = ext.conv_line_dgrad(dy, w_perm, x.size(0), x.size(1),
                                     x.size(2), x.size(3))
        if ctx.needs_input_grad[1]:
            dw = ext.conv_line_wgrad(x, dy, weight.shape[2], weight.shape[3])
        return dx, dw


def conv2d_line(x, weight):
    return _ConvLine.apply(x, weight)


def line_eligible(conv: nn.Conv2d, x_dtype=torch.bfloat16) -> bool:
    """True for the problems csrc/conv_line.hip supports: a (1,T) or (T,1)
    kernel with T in {3, 7}, padding T/2 along the filter and 0 across it,
    stride 1, dilation 1, groups 1, no bias, C % 32 == 0 and K % 32 == 0.
    (The line length, at most 64, is only known at run time; the binding
    checks it.)"""
    r, s = conv.kernel_size
    return (x_dtype == torch.bfloat16
            and conv.groups == 1
            and conv.dilation == (1, 1)
            and conv.bias is None
            and conv.stride == (1, 1)
            and (r, s) in ((1, 3), (3, 1), (1, 7), (7, 1))
            and conv.padding == (r // 2, s // 2)
            and conv.in_channels % 32 == 0
            and conv.out_channels % 32 == 0)


class Conv2dLine(_NativeConv2d):
    """Drop-in for a line_eligible nn.Conv2d, running the line kernels."""

    tag = "line"

    def __init__(self, conv: nn.Conv2d):
        super().__init__(conv)
        self.stride = conv.stride
        self.padding = conv.padding

    def native(self, x):
        return conv2d_line(x, self.weight)


def convert_convs(model: nn.Module, dtype=torch.bfloat16,
                  stem=None, grouped=None, depthwise="library",
                  line="library", avgpool="library",
                  linear="library") -> int:
    """Replace eligible nn.Conv2d children with Conv2dMFMA and eligible
    nn.MaxPool2d with the native NHWC pool. Returns the number of
    conversions.

    ``stem`` selects the path of small-C stem convs: "library" (default)
    leaves them as nn.Conv2d, "native" swaps stem_eligible ones for
    Conv2dStem and counts them. ``stem=None`` reads DDLB_STEM at call
    time. ``grouped`` does the same for grouped_eligible 3x3 convs
    (Conv2dGrouped, DDLB_GROUPED). ``depthwise="native"`` swaps
    depthwise_eligible convs for Conv2dDepthwise; it has no environment
    variable and defaults to "library". ``line="native"`` does the same
    for line_eligible (1,T) / (T,1) convs (Conv2dLine), and
    ``avgpool="native"`` for avgpool_eligible nn.AvgPool2d /
    nn.AdaptiveAvgPool2d(1) children (ops.pool.convert_avgpools), and
    ``linear="native"`` for linear_eligible nn.Linear children
    (ops.modules.convert_linears)."""
    stem = resolve("stem", stem)
    grouped = resolve("grouped", grouped)
    check("depthwise", depthwise, ("native", "library"))
    check("line", line, ("native", "library"))
    check("avgpool", avgpool, ("native", "library"))
    check("linear", linear, ("native", "library"))
    count = 0
    for parent in model.modules():
        for name, child in list(parent.named_children()):
            if not isinstance(child, nn.Conv2d):
                continue
            if mfma_eligible(child, dtype):
                setattr(parent, name, Conv2dMFMA(child))
                count += 1
            elif stem == "native" and stem_eligible(child, dtype):
                setattr(parent, name, Conv2dStem(child))
                count += 1
            elif grouped == "native" and grouped_eligible(child, dtype):
                setattr(parent, name, Conv2dGrouped(child))
                count += 1
            elif depthwise == "native" and depthwise_eligible(child, dtype):
                setattr(parent, name, Conv2dDepthwise(child))
                count += 1
            elif line == "native" and line_eligible(child, dtype):
                setattr(parent, name, Conv2dLine(child))
                count += 1
    if dtype == torch.bfloat16 and enabled("maxpool"):
        from ddlbench_amd.ops.pool import convert_maxpools
        count += convert_maxpools(model)
    if dtype == torch.bfloat16 and avgpool == "native":
        from ddlbench_amd.ops.pool import convert_avgpools
        count += convert_avgpools(model)
    if linear == "native":
        from ddlbench_amd.ops.modules import convert_linears
        count += convert_linears(model, dtype)
    return count
