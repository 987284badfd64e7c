"""The torch path of NF.attention_score and its wiring into
BahdanauAttention, on the CPU: both must reproduce, bit for bit, the
composition the attention module used before the fused score existed (kept
verbatim below)."""

import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from ddlbench_amd.models.gnmt import BahdanauAttention
from ddlbench_amd.ops import functional as NF


class _EagerBahdanauAttention(nn.Module):
    """The attention module as it stood before attention_score."""

    def __init__(self, query_size, key_size, hidden):
        super().__init__()
        self.linear_q = nn.Linear(query_size, hidden, bias=False)
        self.linear_k = nn.Linear(key_size, hidden, bias=False)
        self.v = nn.Parameter(torch.empty(hidden))
        self.b = nn.Parameter(torch.zeros(hidden))
        self.g = nn.Parameter(torch.tensor(math.sqrt(1.0 / hidden)))
        nn.init.uniform_(self.v, -1.0 / math.sqrt(hidden),
                         1.0 / math.sqrt(hidden))

    def score(self, q, k):
        vn = self.g * self.v / self.v.norm()
        s = torch.tanh(q.unsqueeze(2) + k.unsqueeze(1) + self.b)
        return torch.einsum("bqkh,h->bqk", s, vn)

    def forward(self, query, keys, mask=None):
        q = self.linear_q(query)
        k = self.linear_k(keys)
        scores = self.score(q, k)
        if mask is not None:
            scores = scores.masked_fill(~mask.unsqueeze(1), -65504.0)
        attn = F.softmax(scores.float(), dim=-1).to(keys.dtype)
        ctx = torch.bmm(attn, keys)
        return ctx, attn


def _mask(B, Tk):
    lengths = torch.tensor([Tk, 1, (Tk + 1) // 2])[:B]
    return torch.arange(Tk).unsqueeze(0) < lengths.unsqueeze(1)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_torch_path_is_the_eager_composition(dtype, masked):
    B, Tq, Tk, H = 3, 5, 7, 24
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, Tq, H, generator=g).to(dtype)
    k = torch.randn(B, Tk, H, generator=g).to(dtype)
    bias = (0.1 * torch.randn(H, generator=g)).to(dtype)
    vn = torch.randn(H, generator=g).to(dtype)
    mask = _mask(B, Tk) if masked else None
    want = torch.einsum(
        "bqkh,h->bqk", torch.tanh(q.unsqueeze(2) + k.unsqueeze(1) + bias), vn)
    if masked:
        want = want.masked_fill(~mask.unsqueeze(1), -65504.0)
    got = NF.attention_score(q, k, bias, vn, mask, backend="torch")
    assert got.dtype == dtype and got.shape == (B, Tq, Tk)
    assert torch.equal(got, want)
    # on CPU "auto" is the same path
    assert torch.equal(NF.attention_score(q, k, bias, vn, mask), want)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_module_matches_the_previous_class(masked):
    torch.manual_seed(3)
    new = BahdanauAttention(12, 10, 16)
    torch.manual_seed(3)
    old = _EagerBahdanauAttention(12, 10, 16)
    assert list(new.state_dict()) == list(old.state_dict()) == \
        ["v", "b", "g", "linear_q.weight", "linear_k.weight"]
    for a, b in zip(new.state_dict().values(), old.state_dict().values()):
        assert torch.equal(a, b)
    g = torch.Generator().manual_seed(4)
    query = torch.randn(3, 4, 12, generator=g)
    keys = torch.randn(3, 6, 10, generator=g)
    mask = _mask(3, 6) if masked else None
    ctx_n, attn_n = new(query, keys, mask)
    ctx_o, attn_o = old(query, keys, mask)
    assert torch.equal(ctx_n, ctx_o) and torch.equal(attn_n, attn_o)
    (ctx_n.sum() + attn_n[..., 0].sum()).backward()
    (ctx_o.sum() + attn_o[..., 0].sum()).backward()
    for (n, a), (_, b) in zip(new.named_parameters(),
                              old.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_backend_resolution(monkeypatch):
    monkeypatch.delenv("DDLB_ATTN_SCORE", raising=False)
    attn = BahdanauAttention(4, 4, 8)
    assert attn.backend == "auto" and attn.resolve_backend() == "auto"
    monkeypatch.setenv("DDLB_ATTN_SCORE", "torch")
    assert attn.resolve_backend() == "torch"
    # the module's own explicit setting wins over the environment
    assert BahdanauAttention(4, 4, 8, backend="native").resolve_backend() \
        == "native"
    monkeypatch.setenv("DDLB_ATTN_SCORE", "eager")
    with pytest.raises(ValueError, match="DDLB_ATTN_SCORE|backend"):
        attn.resolve_backend()


def test_env_torch_reaches_the_torch_path(monkeypatch):
    seen = []
    real = NF.attention_score

    def spy(q, k, bias, vn, mask=None, backend="auto"):
        seen.append(backend)
        return real(q, k, bias, vn, mask, backend)

    monkeypatch.setattr(NF, "attention_score", spy)
    monkeypatch.setenv("DDLB_ATTN_SCORE", "torch")
    attn = BahdanauAttention(4, 4, 8)
    attn(torch.randn(2, 3, 4), torch.randn(2, 5, 4))
    assert seen == ["torch"]
