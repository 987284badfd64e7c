"""The torch path of NF.attention_context and the default of
BahdanauAttention's context selector, on the CPU."""

import pytest
import torch
import torch.nn.functional as F

from ddlbench_amd.models.gnmt import BahdanauAttention
from ddlbench_amd.ops import functional as NF


def _inputs(B, Tq, Tk, H):
    g = torch.Generator().manual_seed(B * 1000 + Tq * 100 + Tk)
    scores = torch.randn(B, Tq, Tk, generator=g)
    values = torch.randn(B, Tk, H, generator=g)
    mask = torch.arange(Tk).unsqueeze(0) % 3 != 1
    return scores, values, mask.expand(B, Tk).clone()


@pytest.mark.parametrize("shape", [(3, 5, 6, 8), (3, 17, 33, 128),
                                   (3, 3, 70, 100)])
def test_torch_path_matches_float64(shape):
    scores, values, mask = _inputs(*shape)
    mask[1] = False                       # the empty row
    s = scores.double().masked_fill(~mask.unsqueeze(1), float("-inf"))
    p = torch.softmax(s, -1).nan_to_num(0.0)
    want = p @ (values.double() * mask.unsqueeze(2))
    values[~mask] = float("nan")          # a masked row is not read
    ctx, attn = NF.attention_context(scores, values, mask, backend="torch")
    assert ctx.dtype == attn.dtype == torch.float32
    assert (attn[1] == 0).all() and (ctx[1] == 0).all()
    assert (attn[(~mask).unsqueeze(1).expand_as(attn)] == 0).all()
    torch.testing.assert_close(attn.double(), p, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(ctx.double(), want, rtol=1e-5, atol=1e-5)
    # auto on a CPU tensor is the same composition
    assert torch.equal(NF.attention_context(scores, values, mask)[0], ctx)


def test_torch_path_matches_the_eager_lines():
    scores, values, mask = _inputs(3, 17, 20, 128)
    filled = scores.masked_fill(~mask.unsqueeze(1), NF.MASKED_SCORE)
    attn = F.softmax(filled.float(), dim=-1).to(values.dtype)
    ctx = torch.bmm(attn, values)
    got_ctx, got_attn = NF.attention_context(scores, values, mask, "torch")
    torch.testing.assert_close(got_attn, attn, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(got_ctx, ctx, rtol=1e-5, atol=1e-6)


def test_module_default_runs_the_library_lines(monkeypatch):
    monkeypatch.delenv("DDLB_ATTN_CTX", raising=False)
    monkeypatch.setattr(
        NF, "attention_context",
        lambda *a, **k: pytest.fail("the default must not call the new op"))
    torch.manual_seed(3)
    module = BahdanauAttention(16, 16, 16)
    assert module.resolve_ctx_backend() == "library"
    query, keys = torch.randn(2, 4, 16), torch.randn(2, 5, 16)
    mask = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0]]).bool()
    ctx, attn = module(query, keys, mask)
    scores = module.score(module.linear_q(query), module.linear_k(keys), mask)
    want = F.softmax(scores.float(), dim=-1).to(keys.dtype)
    assert torch.equal(attn, want) and torch.equal(ctx, torch.bmm(want, keys))
    with pytest.raises(ValueError, match="library, native or torch"):
        BahdanauAttention(16, 16, 16, ctx_backend="fast")(query, keys, mask)
