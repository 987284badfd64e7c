"""Autograd bridges for the native CDNA4 kernels, with plain-PyTorch
reference implementations (the CPU path and the numerics-test oracle).

Dispatch: ``ddlbench_amd.ops.use_native`` — native on HIP devices (hard
error there if the extension is missing), torch composition on CPU."""

from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from ddlbench_amd import ops as _ops

_ACT = {"none": 0, "relu": 1, "relu6": 2}


def _is_nhwc(t: torch.Tensor) -> bool:
    return (t.dim() == 4
            and t.is_contiguous(memory_format=torch.channels_last)
            and not t.is_contiguous())


def _layout_contiguous(t: torch.Tensor, nhwc: bool) -> torch.Tensor:
    if nhwc:
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def _apply_act(v: torch.Tensor, act: str) -> torch.Tensor:
    if act == "relu":
        return F.relu(v, inplace=True)
    if act == "relu6":
        return F.relu6(v, inplace=True)
    return v


# ------------------------------------------------- gated shortcut gradient
def gate_enabled() -> bool:
    """DDLB_GATE=0 (read per call) restores the materialised shortcut
    gradient at the residual joins."""
    return os.environ.get("DDLB_GATE", "1") != "0"


class GateSlot:
    """Hand-over of one residual join's shortcut gradient without writing
    it. At ``z = relu(bn(y) + res)`` the gradient of ``res`` is ``dz`` with
    the ReLU mask applied and nothing else, and it is read exactly once. A
    block creates one slot per forward and gives it to the join's BN (the
    producer) and to the one op whose backward receives that gradient (the
    consumer: the block's first conv through ``forward_join``, or the
    downsample BN).

    forward   the consumer claims the slot when it takes the path that can
              apply a gate; the producer, which runs after it, uses the slot
              only if it is claimed and its own forward wrote a mask.
    backward  the producer returns ``dz`` itself as the gradient of ``res``
              (an alias, nothing is written) and arms the slot with the mask
              and that tensor; the consumer, finding the slot armed, checks
              that the gradient it received is that very tensor, applies the
              mask inside its kernel and disarms the slot. Each backward
              re-arms, so ``retain_graph=True`` works.

    Anything that replaces or accumulates into the shortcut gradient on the
    way (a tensor hook, a second use of the shortcut) breaks the contract:
    the ungated sum cannot be repaired, so ``take`` raises. An unarmed slot
    changes nothing."""

    __slots__ = ("claimed", "mask", "dy", "version")

    def __init__(self):
        self.claimed = False
        self.mask = None
        self.dy = None
        self.version = 0

    def claim(self) -> None:
        self.claimed = True

    @property
    def armed(self) -> bool:
        return self.mask is not None

    def arm(self, mask: torch.Tensor, dy: torch.Tensor) -> None:
        self.mask, self.dy, self.version = mask, dy, dy._version

    def take(self, grad: Optional[torch.Tensor]) -> torch.Tensor:
        """The mask for ``grad``, which must be the armed tensor; disarms."""
        mask, dy, version = self.mask, self.dy, self.version
        self.mask = self.dy = None
        if (grad is None or grad.data_ptr() != dy.data_ptr()
                or grad.shape != dy.shape or grad.dtype != dy.dtype
                or grad.stride() != dy.stride()
                or grad._version != version):
            raise RuntimeError(
                "gated shortcut gradient: the residual join handed its "
                "output gradient over ungated, to be masked by the op that "
                "consumes it, but the gradient that arrived is not that "
                "tensor (a hook or a second use of the shortcut replaced or "
                "accumulated into it). Set DDLB_GATE=0 to materialise the "
                "shortcut gradient instead.")
        return mask


# ---------------------------------------------------------------- BN+act
class _FusedBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, res, running_mean, running_var,
                training, momentum, eps, act_code, slot=None):
        ext = _ops.require_extension()
        nhwc = _is_nhwc(x)
        x = _layout_contiguous(x, nhwc)
        res = _layout_contiguous(res, nhwc) if res is not None else None
        outs = ext.bn_act_fwd(x, res, gamma, beta, running_mean,
                              running_var, training, momentum,
                              eps, act_code, nhwc)
        y, mean, invstd = outs[0], outs[1], outs[2]
        if len(outs) > 3:
            # 1-bit activation mask: backward never reads y (saves two
            # full-tensor passes AND the y activation memory)
            ctx.save_for_backward(x, mean, invstd, gamma, outs[3])
            ctx.masked = True
        else:
            ctx.save_for_backward(x, mean, invstd, gamma, y)
            ctx.masked = False
        ctx.training = training
        ctx.act_code = act_code
        ctx.has_res = res is not None
        ctx.nhwc = nhwc
        # GateSlot roles: with a residual this BN is the join (producer, if
        # the consumer claimed the slot and a mask was written); an act-free
        # BN without one is the downsample BN (consumer, if the masked
        # kernels cover its tensors)
        ctx.gate_out = ctx.gate_in = None
        if slot is not None:
            if res is not None:
                if slot.claimed and ctx.masked:
                    ctx.gate_out = slot
            elif (act_code == 0 and nhwc and x.dtype == torch.bfloat16
                  and x.size(1) % 8 == 0):
                slot.claim()
                ctx.gate_in = slot
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, mean, invstd, gamma, aux = ctx.saved_tensors
        y, mask = (None, aux) if ctx.masked else (aux, None)
        gate = None
        if ctx.gate_in is not None and ctx.gate_in.armed:
            gate = ctx.gate_in.take(dy)
        dy = _layout_contiguous(dy, ctx.nhwc)
        # the join hands dy itself on as the shortcut gradient: no dres
        hand_over = ctx.gate_out is not None
        out = ext.bn_act_bwd(dy, y, x, mean, invstd, gamma, ctx.act_code,
                             ctx.training, ctx.has_res and not hand_over,
                             ctx.nhwc, mask, gate)
        dx, dgamma, dbeta = out[0], out[1], out[2]
        if hand_over:
            dres = None
            if ctx.needs_input_grad[3]:
                ctx.gate_out.arm(mask, dy)
                dres = dy
        else:
            dres = out[3] if ctx.has_res else None
        return (dx, dgamma, dbeta, dres, None, None, None, None, None, None,
                None)


def bn_act(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
           running_mean: Optional[torch.Tensor],
           running_var: Optional[torch.Tensor], training: bool,
           momentum: float = 0.1, eps: float = 1e-5, act: str = "relu",
           res: Optional[torch.Tensor] = None,
           backend: str = "auto",
           gate: Optional[GateSlot] = None) -> torch.Tensor:
    """BatchNorm2d + activation (+ residual add), fused on GPU. ``gate``
    is the block's GateSlot: with ``res`` this BN produces the gated
    shortcut gradient, without it (``act="none"``) it consumes one."""
    if _ops.use_native(x, backend):
        return _FusedBNAct.apply(x, gamma.float(), beta.float(), res,
                                 running_mean, running_var, training,
                                 momentum, eps, _ACT[act], gate)
    y = F.batch_norm(x, running_mean, running_var, gamma, beta, training,
                     momentum, eps)
    if res is not None:
        y = y + res
    return _apply_act(y, act)


# ----------------------------------------------------------- cross entropy
class _FusedCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        ext = _ops.require_extension()
        logits = logits.contiguous()
        loss_sum, lse = ext.ce_fwd(logits, target)
        ctx.save_for_backward(logits, target, lse)
        return (loss_sum / logits.size(0)).squeeze(0)

    @staticmethod
    def backward(ctx, grad_out):
        ext = _ops.require_extension()
        logits, target, lse = ctx.saved_tensors
        gscale = (grad_out.detach().float() / logits.size(0)).reshape(1)
        dx = ext.ce_bwd(logits, target, lse, gscale.contiguous())
        return dx, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor,
                  backend: str = "auto") -> torch.Tensor:
    if _ops.use_native(logits, backend):
        return _FusedCrossEntropy.apply(logits, target)
    return F.cross_entropy(logits, target)


# ---------------------------------------- label-smoothed cross entropy
class _FusedLSCrossEntropy(torch.autograd.Function):
    """Everything stays on the device: the valid-token count the backward
    scale needs is a saved tensor the kernel reads, never a host value."""

    @staticmethod
    def forward(ctx, logits, target, smoothing, ignore_index, mean):
        ext = _ops.require_extension()
        loss, lse, n_valid = ext.ls_ce_fwd(logits, target, smoothing,
                                           ignore_index, mean)
        ctx.save_for_backward(logits, target, lse, n_valid)
        ctx.cfg = (smoothing, ignore_index, mean)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        ext = _ops.require_extension()
        logits, target, lse, n_valid = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        dx = ext.ls_ce_bwd(logits, target, lse, n_valid, g, *ctx.cfg)
        return dx, None, None, None, None


def label_smoothing_cross_entropy(logits: torch.Tensor, target: torch.Tensor,
                                  smoothing: float = 0.1,
                                  ignore_index: int = -100,
                                  reduction: str = "mean",
                                  backend: str = "auto") -> torch.Tensor:
    """Per-token label-smoothed cross-entropy over (..., K) logits and
    (...) int64 targets; tokens equal to ``ignore_index`` contribute
    nothing. ``reduction="mean"`` divides by the number of non-ignored
    tokens clamped to 1 (all ignored -> 0, not NaN); ``"sum"`` does not
    divide. Returns an fp32 scalar for fp32 / bf16 logits."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got "
                         f"{reduction!r}")
    K = logits.size(-1)
    logits = logits.reshape(-1, K)
    target = target.reshape(-1)
    mean = reduction == "mean"
    if _ops.use_native(logits, backend):
        logits = logits.contiguous()
        target = target.contiguous()
        if torch.is_grad_enabled() and logits.requires_grad:
            return _FusedLSCrossEntropy.apply(
                logits, target, float(smoothing), int(ignore_index), mean)
        # nothing to differentiate: keep neither the logits nor lse
        return _ops.require_extension().ls_ce_fwd(
            logits.detach(), target, float(smoothing), int(ignore_index),
            mean)[0]
    if logits.dtype != torch.float64:
        logits = logits.float()
    non_pad = target != ignore_index
    logp = F.log_softmax(logits, dim=-1)
    nll = -logp.gather(1, target.clamp_min(0).unsqueeze(1)).squeeze(1)
    smooth = -logp.mean(dim=-1)
    loss = (1 - smoothing) * nll + smoothing * smooth
    total = (loss * non_pad).sum()
    if not mean:
        return total
    n_tokens = non_pad.sum().clamp_min(1)
    return total / n_tokens


# ------------------------------------------- Bahdanau attention score
MASKED_SCORE = -65504.0


class _FusedAttnScore(torch.autograd.Function):
    """Saves only the inputs: backward recomputes tanh, so the
    (B, Tq, Tk, H) tensor of the eager composition never exists."""

    @staticmethod
    def forward(ctx, q, k, bias, vn, mask):
        ext = _ops.require_extension()
        ctx.save_for_backward(q, k, bias, vn, mask)
        return ext.attn_score_fwd(q, k, bias, vn, mask)

    @staticmethod
    def backward(ctx, ds):
        ext = _ops.require_extension()
        q, k, bias, vn, mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        # one sweep over the q rows makes dq, dbias and dvn together
        need_q, need_k = need[0] or need[2] or need[3], need[1]
        dq, dk, dbias, dvn = ext.attn_score_bwd(
            ds.contiguous(), q, k, bias, vn, mask, need_q, need_k)
        return (dq if need[0] else None, dk, dbias if need[2] else None,
                dvn if need[3] else None, None)


def attention_score(q: torch.Tensor, k: torch.Tensor, bias: torch.Tensor,
                    vn: torch.Tensor, mask: Optional[torch.Tensor] = None,
                    backend: str = "auto") -> torch.Tensor:
    """Additive attention scores ``sum_h vn[h] * tanh(q[b,i,h] + k[b,j,h]
    + bias[h])`` for q (B, Tq, H) and k (B, Tk, H), as (B, Tq, Tk) in the
    inputs' dtype. ``mask`` is (B, Tk) bool, True for a valid key; a masked
    key scores ``MASKED_SCORE`` and takes no gradient."""
    if _ops.use_native(q, backend):
        q, k = q.contiguous(), k.contiguous()
        bias, vn = bias.contiguous(), vn.contiguous()
        if mask is not None:
            mask = mask.contiguous()
        if torch.is_grad_enabled() and (
                q.requires_grad or k.requires_grad or bias.requires_grad
                or vn.requires_grad):
            return _FusedAttnScore.apply(q, k, bias, vn, mask)
        # nothing to differentiate (beam search, Tq = 1): keep nothing
        return _ops.require_extension().attn_score_fwd(
            q.detach(), k.detach(), bias.detach(), vn.detach(), mask)
    s = torch.tanh(q.unsqueeze(2) + k.unsqueeze(1) + bias)
    scores = torch.einsum("bqkh,h->bqk", s, vn)
    if mask is not None:
        scores = scores.masked_fill(~mask.unsqueeze(1), MASKED_SCORE)
    return scores


# ------------------------------------------------------------------ LSTM
def _aligned16(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _NativeLSTM(torch.autograd.Function):
    """Single-layer time-major bf16 LSTM. The two input-side GEMMs and the
    weight-gradient GEMMs are library calls outside the time loop; the
    recurrence is one native kernel per step, forward and backward. Saved
    for backward: x, y, the fp32 cell states and the four activated gates
    in bf16 (T*B*4H)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0):
        ext = _ops.require_extension()
        T, B, I = x.shape
        H = w_hh.size(1)
        x = x.contiguous()
        w_hh = _aligned16(w_hh)
        xproj = torch.mm(x.view(T * B, I), w_ih.t()).view(T, B, 4 * H)
        bias = b_ih.float() + b_hh.float()
        h0 = _aligned16(h0) if h0 is not None else None
        c0f = c0.float().contiguous() if c0 is not None else None
        y, cs, gates = ext.lstm_fwd(_aligned16(xproj), w_hh, bias, h0, c0f,
                                    True)
        ctx.save_for_backward(x, w_ih, w_hh, y, cs, gates, h0, c0f)
        ctx.set_materialize_grads(False)
        ctx.bias_dtypes = (b_ih.dtype, b_hh.dtype)
        ctx.c0_dtype = c0.dtype if c0 is not None else None
        return y, y[-1:].clone(), cs[-1:].to(x.dtype)

    @staticmethod
    def backward(ctx, dy, dh_T, dc_T):
        ext = _ops.require_extension()
        x, w_ih, w_hh, y, cs, gates, h0, c0f = ctx.saved_tensors
        T, B, I = x.shape
        H = w_hh.size(1)
        need = ctx.needs_input_grad
        dy = _aligned16(dy) if dy is not None else torch.zeros_like(y)
        if dh_T is not None:
            dh_T = _aligned16(dh_T.reshape(B, H))
        if dc_T is not None:
            dc_T = dc_T.reshape(B, H).float().contiguous()
        dgates, dc0 = ext.lstm_bwd(dy, dh_T, dc_T, w_hh, gates, cs, c0f)
        dg2 = dgates.view(T * B, 4 * H)
        dx = torch.mm(dg2, w_ih).view(T, B, I) if need[0] else None
        dw_ih = torch.mm(dg2.t(), x.view(T * B, I)) if need[1] else None
        dw_hh = None
        if need[2]:
            dw_hh = torch.mm(dg2[B:].t(), y[:-1].view((T - 1) * B, H))
            if h0 is not None:
                dw_hh = dw_hh.addmm_(dgates[0].t(), h0)
        db = dgates.float().sum((0, 1)) if need[3] or need[4] else None
        db_ih = db.to(ctx.bias_dtypes[0]) if need[3] else None
        db_hh = db.to(ctx.bias_dtypes[1]) if need[4] else None
        dh0 = torch.mm(dgates[0], w_hh) if need[5] else None
        dc0 = dc0.to(ctx.c0_dtype) if need[6] else None
        return dx, dw_ih, dw_hh, db_ih, db_hh, dh0, dc0


def _lstm_native_reject(x, w_hh) -> Optional[str]:
    """Why the native recurrence cannot run these tensors, or None."""
    if x.device.type != "cuda":
        return f"a {x.device.type} tensor (the kernels are HIP only)"
    if x.dtype != torch.bfloat16 or w_hh.dtype != torch.bfloat16:
        return (f"{x.dtype} input with {w_hh.dtype} weights (bf16 only; "
                "there is no fp32 MFMA path)")
    if w_hh.size(1) % 8 != 0:
        return f"hidden size {w_hh.size(1)} (must be a multiple of 8)"
    return None


def _lstm_torch(x, w_ih, w_hh, b_ih, b_hh, h, c):
    xproj = x @ w_ih.t() + (b_ih + b_hh)
    w_hh_t = w_hh.t()
    ys = []
    for t in range(x.size(0)):
        i, f, g, o = (xproj[t] + h @ w_hh_t).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys), (h.unsqueeze(0), c.unsqueeze(0))


def lstm(x: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
         b_ih: torch.Tensor, b_hh: torch.Tensor, hx=None,
         backend: str = "auto"):
    """Single-layer unidirectional LSTM over time-major x (T, B, I) with
    PyTorch's parameter layout (gate rows i, f, g, o). ``hx`` is None or
    ``(h0, c0)``, each (1, B, H). Returns ``(y, (h_T, c_T))`` with y
    (T, B, H) and h_T, c_T (1, B, H) in x's dtype, like ``nn.LSTM``.

    The native path (bf16 on a GPU, H a multiple of 8) runs the recurrence
    in the HIP step kernels and raises NotImplementedError for anything it
    cannot run; ``backend="torch"`` is the plain time-loop composition in
    whatever dtype it is given."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError("lstm backend must be auto, native or torch, got "
                         f"{backend!r}")
    if x.dim() != 3:
        raise ValueError(f"lstm: x must be (T, B, I), got {tuple(x.shape)}")
    T, B, _ = x.shape
    H = w_hh.size(1)
    if T < 1 or B < 1:
        raise ValueError("lstm: T and B must be at least 1")
    h0 = c0 = None
    if hx is not None:
        h0, c0 = hx
        h0, c0 = h0.reshape(B, H), c0.reshape(B, H)
    native = backend == "native" or (backend == "auto"
                                     and x.device.type == "cuda")
    if native:
        why = _lstm_native_reject(x, w_hh)
        if why is not None:
            raise NotImplementedError(
                f"native LSTM does not support {why}; pass "
                "backend=\"torch\" for the composition")
        _ops.require_extension()
        tensors = (x, w_ih, w_hh, b_ih, b_hh, h0, c0)
        if torch.is_grad_enabled() and any(
                t is not None and t.requires_grad for t in tensors):
            y, h_T, c_T = _NativeLSTM.apply(*tensors)
            return y, (h_T, c_T)
        # nothing to differentiate (greedy / beam decode): the gates are
        # not even written
        ext = _ops.require_extension()
        x = x.detach().contiguous()
        xproj = torch.mm(x.view(T * B, -1), w_ih.detach().t())
        y, cs, _ = ext.lstm_fwd(
            _aligned16(xproj.view(T, B, 4 * H)), _aligned16(w_hh.detach()),
            b_ih.detach().float() + b_hh.detach().float(),
            _aligned16(h0.detach()) if h0 is not None else None,
            c0.detach().float().contiguous() if c0 is not None else None,
            False)
        return y, (y[-1:].clone(), cs[-1:].to(x.dtype))
    if h0 is None:
        h0 = x.new_zeros(B, H)
        c0 = x.new_zeros(B, H)
    return _lstm_torch(x, w_ih, w_hh, b_ih, b_hh, h0, c0)


# ------------------------------------------------------- depthwise conv3x3
class _FusedDWConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride):
        ext = _ops.require_extension()
        nhwc = _is_nhwc(x) and x.dtype == torch.bfloat16 \
            and x.size(1) % 8 == 0
        x = _layout_contiguous(x, nhwc)
        w32 = weight.detach().float().contiguous()
        y = ext.dw3x3_fwd(x, w32, stride, nhwc)
        ctx.save_for_backward(x, w32)
        ctx.stride = stride
        ctx.wdtype = weight.dtype
        ctx.w_cl = weight.is_contiguous(memory_format=torch.channels_last) \
            and not weight.is_contiguous()
        ctx.nhwc = nhwc
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ops.require_extension()
        x, w32 = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx, dw = ext.dw3x3_bwd(x, w32,
                               _layout_contiguous(dy, ctx.nhwc),
                               ctx.stride, need_dx, need_dw, ctx.nhwc)
        if need_dw:
            dw = dw.to(ctx.wdtype)
            if ctx.w_cl:  # match a channels_last weight's layout
                dw = dw.contiguous(memory_format=torch.channels_last)
        return (dx if need_dx else None), (dw if need_dw else None), None


def depthwise_conv3x3(x: torch.Tensor, weight: torch.Tensor,
                      stride: int = 1, backend: str = "auto") -> torch.Tensor:
    """3x3 depthwise conv, pad 1, groups == channels."""
    if _ops.use_native(x, backend):
        return _FusedDWConv3x3.apply(x, weight, stride)
    return F.conv2d(x, weight, None, stride, 1, 1, groups=x.size(1))
