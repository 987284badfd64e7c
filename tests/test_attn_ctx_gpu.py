"""Native fused attention softmax + context (attn_ctx_* kernels) against a
float64 CPU oracle computed from the same, already dtype-rounded inputs.

Shapes are the smallest at which a path changes: H = 8 (under one 16-column
tile), 100 (rows that are no 16 B multiple), 128, 520 (ragged wave split),
1024 at (3, 17, 20); (Tq, Tk) = (1, 1), (1, 20) the one-row tile, (5, 6),
(16, 32) exact tiles, (17, 33) one past them, (3, 70) two softmax chunks and
a ragged third K step, at H = 128. B >= 2 runs without a mask, with key
lengths [Tk, 1, ceil(Tk / 2)], and with every third key invalid plus a
wholly invalid batch row 1 (the empty row).

Bounds per element, from the oracle's p and magnitude sums A. bf16: attn
2^-8 p; the others 2^-8 |ref| (the output rounding) + 2^-8 A (P's 2^-9
rounding, doubled for the fp32 accumulation), A = sum_j p |V|,
p (|g| + sum_j' p |g|) with g = dctx V^T + dattn, sum_i p |dctx|. fp32:
C32 A (A = p for attn), C32 = four times the eager fp32 composition's worst
err/A on the GPU (printed by test_values; profiles/attn_ctx_r12.md),
rounded up to one digit. A = 0 demands exactness."""

import functools
import warnings

import pytest
import torch

from ddlbench_amd.ops import functional as NF

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
C32 = 8e-6
H_CASES = [(3, 17, 20, H) for H in (8, 100, 128, 520, 1024)]
T_CASES = [(B, Tq, Tk, 128) for B in (1, 3)
           for Tq, Tk in ((1, 1), (1, 20), (5, 6), (16, 32), (17, 33),
                          (3, 70))]
CASES = list(dict.fromkeys(H_CASES + T_CASES))
NAMES = ("attn", "ctx", "dscores", "dvalues")


def _masks(B, Tk):
    if B == 1:
        return {"nomask": None}
    ar = torch.arange(Tk).unsqueeze(0)
    lengths = torch.tensor([Tk, 1, (Tk + 1) // 2])[:B].unsqueeze(1)
    holes = (ar % 3 != 1).expand(B, Tk).clone()
    holes[1] = False
    return {"nomask": None, "lengths": ar < lengths, "holes": holes}


def _oracle(scores, values, dctx, dattn, mask):
    """float64 (attn, ctx, dscores, dvalues) and the bounds' A terms."""
    s, v, dc, da = (t.double() for t in (scores, values, dctx, dattn))
    keep = torch.ones_like(s, dtype=torch.bool) if mask is None \
        else mask.unsqueeze(1).expand_as(s)
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1).nan_to_num(0.0)
    if mask is not None:
        v = v * mask.unsqueeze(2)
    g = (dc @ v.transpose(1, 2) + da) * keep
    pg = (p * g).sum(-1, keepdim=True)
    pt = p.transpose(1, 2)
    refs = (p, p @ v, p * (g - pg), pt @ dc)
    A = (p, p @ v.abs(),
         p * (g.abs() + (p * g.abs()).sum(-1, keepdim=True)), pt @ dc.abs())
    return refs, A


@functools.lru_cache(maxsize=None)
def _case(B, Tq, Tk, H, dtype):
    """Inputs, masks and oracles, built once per shape (read-only)."""
    g = torch.Generator().manual_seed(((B * 100 + Tq) * 100 + Tk) * 10000 + H)
    ins = tuple(torch.randn(*shape, generator=g).to(dtype)
                for shape in ((B, Tq, Tk), (B, Tk, H), (B, Tq, H),
                              (B, Tq, Tk)))
    masks = _masks(B, Tk)
    return ins, masks, {k: _oracle(*ins, m) for k, m in masks.items()}


def _run(scores, values, dctx, dattn, mask, backend="native", to=None,
         need=(True, True), transposed=False):
    """(attn, ctx, dscores, dvalues) on the CPU; a gradient that is not
    needed comes back as None."""
    dev = torch.device("cuda", 0)
    s = scores.to(dev, dtype=to, copy=True).requires_grad_(need[0])
    v = values.to(dev, dtype=to, copy=True)
    if transposed:      # the same values as a view of a (Tk, B, H) tensor
        v = v.transpose(0, 1).contiguous().transpose(0, 1)
    v.requires_grad_(need[1])
    md = None if mask is None else mask.to(dev)
    ctx, attn = NF.attention_context(s, v, md, backend=backend)
    ((ctx * dctx.to(dev, dtype=to)).sum()
     + (attn * dattn.to(dev, dtype=to)).sum()).backward()
    cpu = lambda t: None if t is None else t.detach().cpu()
    return cpu(attn), cpu(ctx), cpu(s.grad), cpu(v.grad)


def _worst(got, oracle, dtype, mask):
    """Worst err/bound per output; masked entries must be exactly 0."""
    refs, A = oracle
    out = []
    for name, x, ref, a in zip(NAMES, got, refs, A):
        assert x.shape == ref.shape and torch.isfinite(x.float()).all(), name
        if dtype == torch.bfloat16:
            bound = 2.0 ** -8 * a
            if name != "attn":
                bound = bound + 2.0 ** -8 * ref.abs()
        else:
            bound = C32 * a
        e = (x.double() - ref).abs()
        r = torch.where(bound > 0, e / bound.clamp_min(1e-300),
                        torch.where(e == 0, 0.0, float("inf")))
        out.append(r.max().item())
    if mask is not None:
        dead = (~mask).unsqueeze(1).expand_as(got[0])
        assert (got[0][dead] == 0).all() and (got[2][dead] == 0).all()
        assert (got[3][~mask] == 0).all()
    return out


def _id(c):
    return "B{}-{}x{}-H{}".format(*c)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_values(case, dtype):
    ins, masks, oracles = _case(*case, dtype)
    for key, m in masks.items():
        got = _run(*ins, m)
        assert all(x.dtype == dtype for x in got)
        worst = _worst(got, oracles[key], dtype, m)
        line = f"{_id(case)} {key} native err/bound " + "  ".join(
            f"{n} {w:.3g}" for n, w in zip(NAMES, worst))
        if key != "holes":  # eager autograd gives the empty row NaN grads
            eager = _worst(_run(*ins, m, backend="torch", to=torch.float32),
                           oracles[key], torch.float32, m)
            line += f"; eager fp32 worst err/A {max(eager) * C32:.3g}"
        print(line)
        assert max(worst) <= 1.0, line


def test_strided_values_give_the_same_bits():
    ins, masks, _ = _case(3, 17, 20, 1024, torch.bfloat16)
    for m in masks.values():
        for x, y in zip(_run(*ins, m), _run(*ins, m, transposed=True)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 17, 20, 100), (3, 17, 33, 128),
                                  (3, 1, 20, 128)], ids=_id)
def test_masked_data_is_never_read(case, dtype):
    (s, v, dc, da), masks, oracles = _case(*case, dtype)
    for key in ("lengths", "holes"):
        m = masks[key]
        clean = _run(s, v, dc, da, m)
        dead = (~m).unsqueeze(1).expand_as(s)
        sp, vp, dap = s.clone(), v.clone(), da.clone()
        sp[dead] = float("nan")
        vp[~m] = float("nan")
        dap[dead] = float("inf")
        got = _run(sp, vp, dc, dap, m)
        for name, x, y in zip(NAMES, got, clean):
            assert torch.equal(x, y), (key, name)
        assert max(_worst(got, oracles[key], dtype, m)) <= 1.0


def test_bitwise_reproducible():
    ins, masks, _ = _case(3, 17, 20, 1024, torch.bfloat16)
    for x, y in zip(_run(*ins, masks["holes"]), _run(*ins, masks["holes"])):
        assert torch.equal(x, y)


def test_no_host_synchronisation():
    ins, masks, _ = _case(3, 17, 20, 1024, torch.bfloat16)
    dev = torch.device("cuda", 0)
    s, v = (t.to(dev).requires_grad_(True) for t in ins[:2])
    dc, da, md = ins[2].to(dev), ins[3].to(dev), masks["lengths"].to(dev)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        # torch announces the debug mode as a prototype
        warnings.simplefilter("ignore", UserWarning)
        torch.cuda.set_sync_debug_mode("error")
    try:
        ctx, attn = NF.attention_context(s, v, md, backend="native")
        torch.autograd.backward((ctx, attn), (dc, da))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(s.grad.float()).all()


def test_no_grad_and_partial_grads():
    ins, masks, _ = _case(3, 17, 20, 128, torch.float32)
    m = masks["lengths"]
    attn, ctx, ds, dv = _run(*ins, m)
    dev = torch.device("cuda", 0)
    s, v, md = ins[0].to(dev), ins[1].to(dev), m.to(dev)
    plain = NF.attention_context(s, v, md, backend="native")
    with torch.no_grad():
        ng = NF.attention_context(s.clone().requires_grad_(True), v, md,
                                  backend="native")
    for c, a in (plain, ng):
        assert c.grad_fn is None and a.grad_fn is None
        assert torch.equal(c.cpu(), ctx) and torch.equal(a.cpu(), attn)
    only_s = _run(*ins, m, need=(True, False))
    assert torch.equal(only_s[2], ds) and only_s[3] is None
    only_v = _run(*ins, m, need=(False, True))
    assert torch.equal(only_v[3], dv) and only_v[2] is None


def test_keeps_no_fp32_copies():
    B, T, H = 4, 32, 1024
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.bfloat16)
    scores, values, dctx = mk(B, T, T), mk(B, T, H), mk(B, T, H)

    def eager(s, v):
        attn = torch.softmax(s.float(), dim=-1).to(v.dtype)
        return torch.bmm(attn, v), attn

    def native(s, v):
        return NF.attention_context(s, v, backend="native")

    peaks = {}
    for name, fn in (("native", native), ("eager", eager)):
        s = scores.clone().requires_grad_(True)
        v = values.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(s, v)[0].backward(dctx)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - before
        del s, v
    fp32_copy = B * T * T * 4
    print(f"peak beyond inputs: native {peaks['native']} B, eager "
          f"{peaks['eager']} B, one fp32 (B,Tq,Tk) copy {fp32_copy} B")
    assert peaks["native"] < peaks["eager"]
    # the probe sees eager's fp32 copies of the scores
    assert peaks["eager"] - peaks["native"] >= fp32_copy


def test_arguments_are_checked():
    from ddlbench_amd import ops
    ext = ops.require_extension()
    dev = torch.device("cuda", 0)
    s = torch.zeros(2, 3, 5, device=dev)
    v = torch.zeros(2, 5, 16, device=dev)
    m = torch.ones(2, 5, dtype=torch.bool, device=dev)
    ctx, attn = ext.attn_ctx_fwd(s, v, m)
    assert ctx.shape == (2, 3, 16) and attn.shape == (2, 3, 5)
    with pytest.raises(RuntimeError, match="share one dtype"):
        ext.attn_ctx_fwd(s, v.bfloat16(), None)
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        ext.attn_ctx_fwd(s.half(), v.half(), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ext.attn_ctx_fwd(s.cpu(), v, None)
    with pytest.raises(RuntimeError, match=r"values must be \(B, Tk, H\)"):
        ext.attn_ctx_fwd(s, torch.zeros(2, 4, 16, device=dev), None)
    with pytest.raises(RuntimeError, match="h stride 1"):
        ext.attn_ctx_fwd(s, torch.zeros(2, 5, 32, device=dev)[..., ::2], None)
    with pytest.raises(RuntimeError, match=r"mask must be \(B, Tk\)"):
        ext.attn_ctx_fwd(s, v, m[:, :4].contiguous())
    with pytest.raises(RuntimeError, match=r"dctx must be \(B, Tq, H\)"):
        ext.attn_ctx_bwd(torch.zeros(2, 3, 8, device=dev), None, attn, v, m)
    big = torch.zeros(1, 1, NF.ATTN_CTX_MAX_TK + 1, device=dev)
    bigv = torch.zeros(1, NF.ATTN_CTX_MAX_TK + 1, 8, device=dev)
    with pytest.raises(RuntimeError, match="over the cap"):
        ext.attn_ctx_fwd(big, bigv, None)
    with pytest.raises(NotImplementedError, match="cap is 1024"):
        NF.attention_context(big, bigv, backend="native")
    ctx, attn = NF.attention_context(big, bigv)     # auto: the composition
    assert attn.shape == big.shape and ctx.shape == (1, 1, 8)


def test_attention_module_runs_the_native_kernels(monkeypatch):
    from ddlbench_amd import ops
    from ddlbench_amd.models.gnmt import BahdanauAttention
    ext = ops.require_extension()
    calls = []
    real = ext.attn_ctx_fwd

    def spy(*args):
        calls.append(tuple(args[0].shape))
        return real(*args)

    monkeypatch.setattr(ext, "attn_ctx_fwd", spy)
    monkeypatch.delenv("DDLB_ATTN_CTX", raising=False)
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    native = BahdanauAttention(128, 128, 128, ctx_backend="native").to(dev)
    library = BahdanauAttention(128, 128, 128, ctx_backend="library").to(dev)
    auto = BahdanauAttention(128, 128, 128).to(dev)
    library.load_state_dict(native.state_dict())
    g = torch.Generator().manual_seed(12)
    query = torch.randn(3, 17, 128, generator=g).to(dev)
    keys = torch.randn(20, 3, 128, generator=g).to(dev).transpose(0, 1)
    lengths = torch.tensor([20, 1, 10]).unsqueeze(1)
    mask = (torch.arange(20).unsqueeze(0) < lengths).to(dev)
    up = torch.randn(3, 17, 128, generator=g).to(dev)
    ctx_n, attn_n = native(query, keys, mask)
    assert calls == [(3, 17, 20)]
    ctx_l, attn_l = library(query, keys, mask)
    auto(query, keys, mask)         # nothing set: the library lines
    assert calls == [(3, 17, 20)]
    torch.testing.assert_close(ctx_n, ctx_l, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(attn_n, attn_l, rtol=1e-5, atol=1e-5)
    (ctx_n * up).sum().backward()
    (ctx_l * up).sum().backward()
    for (name, a), (_, b) in zip(native.named_parameters(),
                                 library.named_parameters()):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    monkeypatch.setenv("DDLB_ATTN_CTX", "native")
    auto(query, keys, mask)
    assert calls == [(3, 17, 20)] * 2


def test_greedy_decode_agrees_between_backends():
    from ddlbench_amd.models.gnmt import GNMT
    from ddlbench_amd.translation import Translator
    dev = torch.device("cuda", 0)
    torch.manual_seed(21)
    model = GNMT(vocab_size=96, hidden_size=64, num_layers=2).to(dev)
    src = torch.randint(3, 96, (9, 4), device=dev)
    src_len = torch.tensor([9, 7, 4, 2], device=dev)
    outs = {}
    for backend in ("native", "library"):
        model.decoder.att_rnn.attn.ctx_backend = backend
        outs[backend] = Translator(model, max_len=6).greedy(src, src_len)
    assert torch.equal(outs["native"], outs["library"])
