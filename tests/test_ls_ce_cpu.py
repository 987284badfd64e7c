"""The torch branch of NF.label_smoothing_cross_entropy (the CPU path and
the GPU tests' oracle) against torch's own F.cross_entropy, in float64 —
so the oracle does not rest on the project's formula alone."""

import pytest
import torch
import torch.nn.functional as F

from ddlbench_amd.ops import functional as NF

IGN = 3


def _case(R=11, K=37, seed=0, ignored=(0, 4, 10)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g, dtype=torch.float64) * 3
    t = torch.randint(K, (R,), generator=g)
    t[t == IGN] = IGN + 1
    t[list(ignored)] = IGN
    return x, t


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_matches_torch_cross_entropy(eps, reduction):
    x, t = _case()
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    got = NF.label_smoothing_cross_entropy(x1, t, eps, IGN, reduction,
                                           backend="torch")
    ref = F.cross_entropy(x2, t, ignore_index=IGN, label_smoothing=eps,
                          reduction=reduction)
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    got.backward()
    ref.backward()
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-12, atol=1e-12)
    assert (x1.grad[t == IGN] == 0).all()


def test_negative_ignore_index_matches_torch():
    x, t = _case()
    t[t == IGN] = -100
    got = NF.label_smoothing_cross_entropy(x, t, 0.1, -100, backend="torch")
    ref = F.cross_entropy(x, t, ignore_index=-100, label_smoothing=0.1)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


def test_equals_gnmt_label_smoothing_loss_tbv():
    from ddlbench_amd.models.gnmt import PAD, LabelSmoothingLoss
    g = torch.Generator().manual_seed(1)
    T, B, V = 5, 3, 29
    x = torch.randn(T, B, V, generator=g)
    t = torch.randint(V, (T, B), generator=g)
    t[t == PAD] = PAD + 1
    t[3:, 1] = PAD
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    mod = LabelSmoothingLoss(0.1)(x1, t)
    fn = NF.label_smoothing_cross_entropy(x2, t, 0.1, ignore_index=PAD,
                                          backend="torch")
    assert mod.dim() == 0 and mod.dtype == torch.float32
    assert torch.equal(mod, fn)
    mod.backward()
    fn.backward()
    assert torch.equal(x1.grad, x2.grad)
    # and against torch's own loss, at fp32 accuracy
    ref = F.cross_entropy(x.reshape(-1, V).double(), t.reshape(-1),
                          ignore_index=PAD, label_smoothing=0.1)
    torch.testing.assert_close(mod.double(), ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_all_ignored_is_zero_with_zero_gradient(reduction):
    x, t = _case()
    t[:] = IGN
    x = x.requires_grad_(True)
    loss = NF.label_smoothing_cross_entropy(x, t, 0.1, IGN, reduction,
                                            backend="torch")
    assert loss.item() == 0.0
    loss.backward()
    assert (x.grad == 0).all()


def test_reduces_to_cross_entropy():
    x, t = _case(ignored=())
    got = NF.label_smoothing_cross_entropy(x, t, 0.0, backend="torch")
    ref = NF.cross_entropy(x, t, backend="torch")
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


def test_module_and_argument_checks():
    from ddlbench_amd.ops.modules import LabelSmoothingCrossEntropy
    x, t = _case()
    mod = LabelSmoothingCrossEntropy(0.1, IGN, "sum")
    ref = NF.label_smoothing_cross_entropy(x, t, 0.1, IGN, "sum",
                                           backend="torch")
    assert torch.equal(mod(x, t), ref)
    with pytest.raises(ValueError):
        NF.label_smoothing_cross_entropy(x, t, reduction="none")
