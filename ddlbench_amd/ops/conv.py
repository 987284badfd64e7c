"""MFMA implicit-GEMM convolution: autograd bridge + model converter.

Forward and data-grad run on the hand-written NHWC bf16 kernels
(csrc/conv_mfma*.hip) and the weight-grad on the transpose-read kernel
(csrc/conv_wgrad.hip) — the full conv triple is in-tree by default.

Eligibility: bf16, channels_last, groups=1, dilation=1, C%8==0, K%8==0.
``convert_convs(model)`` swaps every eligible nn.Conv2d for Conv2dMFMA.

Stem convs (C < 8) stay on the library path by default; with
``DDLB_STEM=native`` (or ``convert_convs(model, stem="native")``) they run
the small-C kernels of csrc/conv_stem.hip (forward + weight-grad) through
``Conv2dStem``."""

from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd import ops as _ops

# weight-grad backend: the native kernel (conv_wgrad.hip) by default —
# DDLB_WGRAD=library opts back into aten's conv backward
_WGRAD = os.environ.get("DDLB_WGRAD", "mfma")

# The backward's layout/dtype tail runs in native kernels: the dgrad
# weight layout is one tiled transpose (conv_weight_dgrad_layout) and the
# weight-grad kernels write the weight's dtype and layout themselves
# (conv_igemm_wgrad_bf16). False restores the eager-tensor tail (a strided
# permute copy, fp32 dw + cast) — same values, kept for comparison.
NATIVE_TAIL = os.environ.get("DDLB_CONV_TAIL", "native") != "eager"

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
        if _WGRAD == "mfma" and NATIVE_TAIL \
                and weight.dtype == torch.bfloat16:
            dw = ext.conv_igemm_wgrad_bf16(x, dy, weight.shape[2],
                                           weight.shape[3], ctx.stride,
                                           ctx.pad)
        elif _WGRAD == "mfma":
            dw = _dw_to_weight_layout(
                ext.conv_igemm_wgrad(x, dy, weight.shape[2],
                                     weight.shape[3], ctx.stride,
                                     ctx.pad), weight)
        else:
            dw = torch.ops.aten.convolution_backward(
                dy, x, weight, None, [ctx.stride, ctx.stride],
                [ctx.pad, ctx.pad], [1, 1], False, [0, 0], 1,
                [False, True, False])[1]
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
    return os.environ.get("DDLB_JOIN", "1") != "0"


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


def convert_convs(model: nn.Module, dtype=torch.bfloat16,
                  stem=None) -> int:
    """Replace eligible nn.Conv2d children with Conv2dMFMA and eligible
    nn.MaxPool2d with the native NHWC pool. Returns the number of
    conversions.

    ``stem`` selects the path of small-C stem convs: "library" (default)
    leaves them as nn.Conv2d, "native" swaps stem_eligible ones for
    Conv2dStem and counts them. ``stem=None`` reads DDLB_STEM at call
    time."""
    if stem is None:
        stem = os.environ.get("DDLB_STEM", "library")
    if stem not in ("native", "library"):
        raise ValueError(f"stem must be 'native' or 'library', got {stem!r}")
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
    if dtype == torch.bfloat16 and \
            os.environ.get("DDLB_MAXPOOL", "1") != "0":
        from ddlbench_amd.ops.pool import convert_maxpools
        count += convert_maxpools(model)
    return count
