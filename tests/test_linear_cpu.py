"""Linear Python layer (no GPU): eligibility, convert_linears, the opt-in
wiring of convert_convs and NF.linear's CPU path."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models import build_model
from ddlbench_amd.models.gnmt import GNMT
from ddlbench_amd.ops import functional as NF
from ddlbench_amd.ops.conv import convert_convs
from ddlbench_amd.ops.modules import Linear, convert_linears, linear_eligible

BF = torch.bfloat16


@pytest.mark.parametrize("m,dtype,want", [
    (nn.Linear(2048, 1000), BF, True),         # ImageNet heads
    (nn.Linear(1024, 32320), BF, True),        # GNMT classifier
    (nn.Linear(1024, 1024, bias=False), BF, True),
    (nn.Linear(512, 10), BF, False),           # CIFAR-10 / MNIST heads
    (nn.Linear(20, 64), BF, False),            # K % 8 != 0
    (nn.Linear(2048, 1000), torch.float32, False),
    (nn.Conv2d(8, 8, 1), BF, False),
])
def test_linear_eligible(m, dtype, want):
    assert linear_eligible(m, dtype) is want


def test_convert_linears_gnmt():
    torch.manual_seed(0)
    model = GNMT(vocab_size=96, hidden_size=64, num_layers=2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = list(model.parameters())
    assert convert_linears(model) == 3   # linear_q, linear_k, the classifier
    natives = [m for m in model.modules() if isinstance(m, Linear)]
    assert len(natives) == 3 and all(m.backend == "native" for m in natives)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert all(a is b for a, b in zip(model.parameters(), params))
    assert convert_linears(model) == 0   # nothing left to convert


def test_convert_convs_linear_keyword():
    with pytest.raises(ValueError):
        convert_convs(build_model("imagenet", "resnet18"), linear="fast")
    n_default = convert_convs(build_model("imagenet", "resnet18"))
    model = build_model("imagenet", "resnet18")
    assert convert_convs(model, linear="library") == n_default
    assert not any(isinstance(m, Linear) for m in model.modules())
    model = build_model("imagenet", "resnet18")
    assert convert_convs(model, linear="native") == n_default + 1
    # a 10-class head stays a library call
    n10 = convert_convs(build_model("cifar10", "resnet18"))
    assert convert_convs(build_model("cifar10", "resnet18"),
                         linear="native") == n10


@pytest.mark.parametrize("bias", [True, False])
def test_functional_linear_cpu(bias):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 5, 16, generator=g)
    w = torch.randn(24, 16, generator=g)
    b = torch.randn(24, generator=g) if bias else None
    assert torch.equal(NF.linear(x, w, b), F.linear(x, w, b))
    assert torch.equal(NF.linear(x, w, b, backend="torch"), F.linear(x, w, b))


def test_linear_module_backend():
    with pytest.raises(ValueError):
        Linear(8, 8, backend="fast")
    torch.manual_seed(1)
    ours = Linear(16, 8)
    torch.manual_seed(1)
    ref = nn.Linear(16, 8)
    assert ours.backend == "library"
    assert list(ours.state_dict().keys()) == list(ref.state_dict().keys())
    x = torch.randn(4, 16)
    assert torch.equal(ours(x), ref(x))
