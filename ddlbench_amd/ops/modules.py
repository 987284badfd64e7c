"""nn.Module wrappers over the fused kernels.

``BNAct`` replaces the BatchNorm2d → ReLU (→ residual add) chains of the
model zoo with one fused op; ``DepthwiseConv3x3`` replaces
Conv2d(groups=channels). Both keep plain-PyTorch semantics (state dict
compatible with nn.BatchNorm2d / nn.Conv2d field names). ``LSTM`` is
nn.LSTM with a choice of recurrence backend."""

from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from ddlbench_amd.ops import functional as NF

# module-level default backend — engines set this once from the config
_DEFAULT_BACKEND = "auto"


def set_default_backend(backend: str) -> None:
    global _DEFAULT_BACKEND
    assert backend in ("auto", "native", "torch")
    _DEFAULT_BACKEND = backend


def default_backend() -> str:
    return _DEFAULT_BACKEND


class BNAct(nn.Module):
    """BatchNorm2d + activation (+ optional residual add), fused on GPU.

    forward(x, res=None, gate=None): y = act(bn(x) + res); gate is the
    block's NF.GateSlot at a residual join (see there).
    Running stats and affine params stay fp32 regardless of model dtype
    (they are re-cast at dispatch; fp32 optimizer-state discipline)."""

    def __init__(self, num_features: int, act: str = "relu",
                 eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        assert act in ("none", "relu", "relu6")
        self.num_features = num_features
        self.act = act
        self.eps = eps
        self.momentum = momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked",
                             torch.tensor(0, dtype=torch.long))
        self._nbt = 0

    def _apply(self, fn, recurse=True):
        # keep BN params/stats fp32 under model.to(bf16): re-cast after
        super()._apply(fn, recurse)
        for name in ("weight", "bias"):
            p = getattr(self, name)
            if p is not None and p.dtype != torch.float32:
                p.data = p.data.float()
                if p.grad is not None:
                    p.grad = p.grad.float()
        for name in ("running_mean", "running_var"):
            b = getattr(self, name)
            if b is not None and b.dtype != torch.float32:
                setattr(self, name, b.float())
        return self

    def forward(self, x: torch.Tensor,
                res: Optional[torch.Tensor] = None,
                gate: Optional[NF.GateSlot] = None) -> torch.Tensor:
        if self.training:
            # python-side counter; synced to the buffer on state_dict()
            # (a per-step GPU add showed up as 51 launches/step)
            self._nbt += 1
        return NF.bn_act(x, self.weight, self.bias, self.running_mean,
                         self.running_var, self.training, self.momentum,
                         self.eps, self.act, res,
                         backend=_DEFAULT_BACKEND, gate=gate)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        if self._nbt:
            self.num_batches_tracked += self._nbt
            self._nbt = 0
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def extra_repr(self) -> str:
        return f"{self.num_features}, act={self.act}"


class DepthwiseConv3x3(nn.Module):
    """3x3 depthwise conv (groups == channels), pad 1, no bias."""

    def __init__(self, channels: int, stride: int = 1):
        super().__init__()
        assert stride in (1, 2)
        self.channels = channels
        self.stride = stride
        self.weight = nn.Parameter(torch.empty(channels, 1, 3, 3))
        nn.init.kaiming_normal_(self.weight, mode="fan_out")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return NF.depthwise_conv3x3(x, self.weight, self.stride,
                                    backend=_DEFAULT_BACKEND)

    def extra_repr(self) -> str:
        return f"{self.channels}, stride={self.stride}"


class LSTM(nn.LSTM):
    """``torch.nn.LSTM`` with a choice of recurrence: same parameters, same
    registration order (so the same seeded initial values) and the same
    ``state_dict`` keys. ``backend`` is "auto", "native" or "library";
    while it is "auto", DDLB_LSTM picks one per call, and "auto" itself is
    the library path. "native" runs ``NF.lstm``'s HIP step kernels and
    raises NotImplementedError for anything they cannot run."""

    def __init__(self, *args, backend: str = "auto", **kwargs):
        super().__init__(*args, **kwargs)
        self.backend = backend

    def resolve_backend(self) -> str:
        """The backend the next forward uses; the environment is read here,
        per call, and only while the module's own setting is "auto"."""
        backend = self.backend
        if backend == "auto":
            backend = os.environ.get("DDLB_LSTM", "auto")
        if backend not in ("auto", "native", "library"):
            raise ValueError("LSTM backend must be auto, native or library, "
                             f"got {backend!r}")
        return "library" if backend == "auto" else backend

    def _native_reject(self, x) -> Optional[str]:
        if isinstance(x, nn.utils.rnn.PackedSequence):
            return "a PackedSequence input"
        if self.num_layers != 1:
            return f"num_layers={self.num_layers}"
        if self.bidirectional:
            return "bidirectional=True"
        if self.proj_size != 0:
            return f"proj_size={self.proj_size}"
        if self.dropout != 0:
            return f"inner dropout={self.dropout}"
        if self.batch_first:
            return "batch_first=True"
        if not self.bias:
            return "bias=False"
        if x.dim() != 3:
            return "unbatched input"
        return None

    def forward(self, input, hx=None):
        if self.resolve_backend() == "library":
            return super().forward(input, hx)
        why = self._native_reject(input)
        if why is not None:
            raise NotImplementedError(
                f"native LSTM does not support {why}; use "
                "backend=\"library\"")
        return NF.lstm(input, self.weight_ih_l0, self.weight_hh_l0,
                       self.bias_ih_l0, self.bias_hh_l0, hx,
                       backend="native")


class CrossEntropyLoss(nn.Module):
    """Fused softmax cross-entropy (mean reduction)."""

    def forward(self, logits: torch.Tensor,
                target: torch.Tensor) -> torch.Tensor:
        return NF.cross_entropy(logits, target, backend=_DEFAULT_BACKEND)


class LabelSmoothingCrossEntropy(nn.Module):
    """Fused label-smoothed cross-entropy over (..., K) logits; targets
    equal to ``ignore_index`` are skipped. ``reduction`` is "mean" (over
    the non-ignored tokens, count clamped to 1) or "sum"."""

    def __init__(self, smoothing: float = 0.1, ignore_index: int = -100,
                 reduction: str = "mean"):
        super().__init__()
        assert reduction in ("mean", "sum")
        self.smoothing = smoothing
        self.ignore_index = ignore_index
        self.reduction = reduction

    def forward(self, logits: torch.Tensor,
                target: torch.Tensor) -> torch.Tensor:
        return NF.label_smoothing_cross_entropy(
            logits, target, self.smoothing, self.ignore_index,
            self.reduction, backend=_DEFAULT_BACKEND)

    def extra_repr(self) -> str:
        return (f"smoothing={self.smoothing}, "
                f"ignore_index={self.ignore_index}, "
                f"reduction={self.reduction}")
