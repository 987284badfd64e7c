"""Native fused attention score (attn_score_* kernels) against a float64 CPU
oracle computed from the same, already dtype-rounded inputs. All @gpu.

Shapes are the smallest that reach each code path. Widths H, each at
(B, Tq, Tk) = (3, 17, 20):
  8     less than one wave of columns; fp32 takes 16 B loads, bf16 one 16 B
        load per row in a single lane
  100   bf16 rows are not 16 B multiples: the scalar forward path, two
        64-column chunks with a ragged tail; two backward column blocks
  128   the width of the GNMT train-step test
  520   just above the bf16 forward chunk (64 lanes x 8 = 512) and two
        fp32 chunks (256) plus a ragged third; nine backward column blocks
  1024  GNMT
(Tq, Tk), each at H = 128 and B in {1, 3}:
  (1, 1)    one score
  (1, 20)   the decode step: the one-row forward tile
  (3, 5)    one-row forward tiles, more than one of them; ragged key tile
  (5, 6)    just above the 4 x 4 forward tile: both tiling loops run twice
            with a ragged last tile; backward waves take a second row
  (17, 20)  ragged in q, exact in k
Every case runs without a mask and with key lengths [Tk, 1, ceil(Tk / 2)]
cut to B.

Bounds. Forward fp32: |err| <= 4e-6 * sum_h |vn[h]|. The argument
q + k + bias carries two fp32 roundings of a value up to ~6 (<= 7e-7), which
tanh' <= 1 passes through; the exp / reciprocal form adds <= ~3e-7 to tanh;
the fp32 sum (a per-lane chain of H / 64 terms and a 6-step butterfly) adds
<= ~1.3e-6 relative to sum |vn * t|: ~2.3e-6 per unit of sum |vn|, rounded up
to 4e-6. Forward bf16 adds 2^-8 |ref|: one round-to-nearest into 8
significant bits. Each gradient element is held to 8e-6 * A (+ 2^-8 |ref| in
bf16), A being the float64 sum of the magnitudes of its terms with the
factors tanh and 1 - tanh^2 bounded by 1: |vn[h]| * sum_j |ds[b,i,j]| for
dq[b,i,h], |vn[h]| * sum_i |ds[b,i,j]| for dk[b,j,h], |vn[h]| * sum |ds| for
dbias[h] and sum |ds| for dvn[h], over valid keys only. So small gradients
are held to account as well as large ones."""

import functools
import warnings

import pytest
import torch

from ddlbench_amd.ops import functional as NF

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
MASKED = -65504.0
H_CASES = [(3, 17, 20, H) for H in (8, 100, 128, 520, 1024)]
T_CASES = [(B, Tq, Tk, 128) for B in (1, 3)
           for Tq, Tk in ((1, 1), (1, 20), (3, 5), (5, 6), (17, 20))]
CASES = list(dict.fromkeys(H_CASES + T_CASES))
NAMES = ("dq", "dk", "dbias", "dvn")


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"


def _lengths_mask(B, Tk):
    lengths = torch.tensor([Tk, 1, (Tk + 1) // 2])[:B]
    return torch.arange(Tk).unsqueeze(0) < lengths.unsqueeze(1)


def _oracle(q, k, bias, vn, ds, mask):
    """float64 scores and gradients with their bounds' A terms."""
    q, k, bias, vn, ds = (t.double() for t in (q, k, bias, vn, ds))
    t = torch.tanh(q.unsqueeze(2) + k.unsqueeze(1) + bias)  # (B,Tq,Tk,H)
    scores = (t * vn).sum(-1)
    if mask is not None:
        keep = mask.unsqueeze(1).expand_as(ds)
        ds = ds * keep          # masked_fill passes no gradient
    d4 = ds.unsqueeze(-1)
    w = d4 * vn * (1 - t * t)
    grads = (w.sum(2), w.sum(1), w.sum((0, 1, 2)), (d4 * t).sum((0, 1, 2)))
    a = ds.abs()
    avn = vn.abs()
    A = (a.sum(2).unsqueeze(-1) * avn, a.sum(1).unsqueeze(-1) * avn,
         a.sum() * avn, a.sum().expand_as(vn))
    return scores, grads, A


@functools.lru_cache(maxsize=None)
def _case(B, Tq, Tk, H, dtype):
    """Inputs and both oracles, built once per shape and shared
    (read-only)."""
    g = torch.Generator().manual_seed(((B * 100 + Tq) * 100 + Tk) * 10000 + H)
    q = torch.randn(B, Tq, H, generator=g).to(dtype)
    k = torch.randn(B, Tk, H, generator=g).to(dtype)
    bias = (0.1 * torch.randn(H, generator=g)).to(dtype)
    vn = torch.randn(H, generator=g)
    vn = (vn / vn.norm()).to(dtype)
    ds = torch.randn(B, Tq, Tk, generator=g).to(dtype)
    mask = _lengths_mask(B, Tk)
    ins = (q, k, bias, vn, ds)
    return ins, mask, {False: _oracle(*ins, None), True: _oracle(*ins, mask)}


def _native(q, k, bias, vn, ds, mask, backend="native", to=None):
    dev = _dev()
    leaves = [t.to(dev, dtype=to, copy=True).requires_grad_(True)
              for t in (q, k, bias, vn)]
    s = NF.attention_score(*leaves, None if mask is None else mask.to(dev),
                           backend=backend)
    s.backward(ds.to(dev, dtype=to))
    return s.detach().cpu(), tuple(t.grad.cpu() for t in leaves)


def _fwd_bound(ref, vn, dtype):
    bound = 4e-6 * vn.double().abs().sum() * torch.ones_like(ref)
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return bound


def _check(s, grads, oracle, vn, mask, dtype, tag):
    """Asserts the bounds; returns the worst err/bound, forward and
    backward."""
    ref_s, ref_g, A = oracle
    assert s.dtype == dtype and all(g.dtype == dtype for g in grads)
    assert torch.isfinite(s.float()).all()
    err = (s.double() - ref_s).abs()
    ratio = err / _fwd_bound(ref_s, vn, dtype)
    if mask is not None:
        dead = (~mask).unsqueeze(1).expand_as(s)
        assert (s[dead] == torch.tensor(MASKED).to(dtype)).all()
        assert (grads[1][~mask] == 0).all()      # dk of masked keys
        ratio = ratio[~dead]
    worst_f = ratio.max().item()
    worst_b = 0.0
    line = f"{tag}: fwd worst err/bound {worst_f:.3g}"
    for name, got, ref, a in zip(NAMES, grads, ref_g, A):
        assert got.shape == ref.shape, name
        assert torch.isfinite(got.float()).all(), name
        bound = 8e-6 * a
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * ref.abs()
        e = (got.double() - ref).abs()
        # a key or row with no valid term has A = 0 and must be exact
        r = torch.where(bound > 0, e / bound.clamp_min(1e-300),
                        torch.where(e == 0, 0.0, float("inf")))
        worst_b = max(worst_b, r.max().item())
        line += f"  {name} {r.max().item():.3g}"
    print(line)
    assert worst_f <= 1.0, line
    assert worst_b <= 1.0, line
    return worst_f, worst_b


def _id(c):
    return "B{}-{}x{}-H{}".format(*c)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_values(case, dtype):
    ins, mask, oracles = _case(*case, dtype)
    for m in (None, mask):
        tag = f"{_id(case)} {'mask' if m is not None else 'nomask'}"
        # the eager fp32 composition on the GPU, against the same oracle
        se, ge = _native(*ins, m, backend="torch", to=torch.float32)
        ref_s = oracles[m is not None][0]
        keep = torch.ones_like(ref_s, dtype=torch.bool) if m is None \
            else m.unsqueeze(1).expand_as(ref_s)
        eager = ((se.double() - ref_s).abs()
                 / _fwd_bound(ref_s, ins[3], torch.float32))[keep].max()
        print(f"{tag}: eager fp32 fwd worst err/bound {eager.item():.3g}")
        s, grads = _native(*ins, m)
        _check(s, grads, oracles[m is not None], ins[3], m, dtype,
               f"{tag} native")


# ------------------------------------------------ masked keys are not read
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 17, 20, 100), (3, 17, 20, 1024),
                                  (3, 1, 20, 128)], ids=_id)
def test_masked_keys_are_never_read(case, dtype):
    (q, k, bias, vn, ds), mask, oracles = _case(*case, dtype)
    s0, g0 = _native(q, k, bias, vn, ds, mask)
    kp, dsp = k.clone(), ds.clone()
    kp[~mask] = float("nan")
    dsp[(~mask).unsqueeze(1).expand_as(ds)] = float("inf")
    s1, g1 = _native(q, kp, bias, vn, dsp, mask)
    assert torch.equal(s1, s0)
    for name, a, b in zip(NAMES, g1, g0):
        assert torch.equal(a, b), name
    assert (g1[1][~mask] == 0).all()
    assert (s1[(~mask).unsqueeze(1).expand_as(s1)]
            == torch.tensor(MASKED).to(dtype)).all()
    _check(s1, g1, oracles[True], vn, mask, dtype, f"{_id(case)} poisoned")


# -------------------------------------------------------------- saturation
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_saturation(dtype):
    (q, k, bias, vn, ds), mask, _ = _case(3, 17, 20, 128, dtype)
    q = q.clone()
    q[0, 0] = 100.0
    q[0, 1] = -100.0
    q[1, 2, ::2] = 100.0
    q[1, 2, 1::2] = -100.0
    s, grads = _native(q, k, bias, vn, ds, None)
    oracle = _oracle(q, k, bias, vn, ds, None)
    _check(s, grads, oracle, vn, None, dtype, "saturated")
    total = vn.double().sum()
    bound = _fwd_bound(total, vn, dtype)
    assert ((s[0, 0].double() - total).abs() <= bound).all()
    assert ((s[0, 1].double() + total).abs() <= bound).all()
    assert (grads[0][0, :2] == 0).all() and (grads[0][1, 2] == 0).all()


# -------------------------------------------------------------- determinism
def test_bitwise_reproducible():
    ins, mask, _ = _case(3, 17, 20, 1024, torch.bfloat16)
    a = _native(*ins, mask)
    b = _native(*ins, mask)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


# ------------------------------------------------------ no 4-D intermediate
def test_no_4d_intermediate():
    B, T, H = 4, 32, 1024
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev, torch.bfloat16)
    ins = [mk(B, T, H), mk(B, T, H), mk(H), mk(H)]
    ds = mk(B, T, T)
    full = B * T * T * H * 2
    peaks = {}
    for backend in ("native", "torch"):
        leaves = [t.clone().requires_grad_(True) for t in ins]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        NF.attention_score(*leaves, backend=backend).backward(ds)
        torch.cuda.synchronize()
        peaks[backend] = torch.cuda.max_memory_allocated() - before
        del leaves
    print(f"peak beyond inputs: native {peaks['native']} B, "
          f"eager {peaks['torch']} B, 4-D tensor {full} B")
    assert peaks["native"] < full // 4
    assert peaks["torch"] > full     # the probe sees the 4-D tensor


# --------------------------------------------------------- no host sync
def test_no_host_synchronisation():
    ins, mask, _ = _case(3, 17, 20, 1024, torch.bfloat16)
    dev = _dev()
    leaves = [t.to(dev).requires_grad_(True) for t in ins[:4]]
    ds, md = ins[4].to(dev), mask.to(dev)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        # torch announces the debug mode as a prototype
        warnings.simplefilter("ignore", UserWarning)
        torch.cuda.set_sync_debug_mode("error")
    try:
        s = NF.attention_score(*leaves, md, backend="native")
        s.backward(ds)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(s.float()).all()


# ------------------------------------------------- no_grad and partial grads
def test_no_grad_and_partial_grads():
    ins, mask, _ = _case(3, 17, 20, 128, torch.float32)
    dev = _dev()
    q, k, bias, vn, ds = (t.to(dev) for t in ins)
    md = mask.to(dev)
    full, grads = _native(*ins, mask)
    plain = NF.attention_score(q, k, bias, vn, md, backend="native")
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain.cpu(), full)
    qg = q.clone().requires_grad_(True)
    with torch.no_grad():
        ng = NF.attention_score(qg, k, bias, vn, md, backend="native")
    assert ng.grad_fn is None and torch.equal(ng.cpu(), full)
    # only q requires grad: the key sweep is skipped, dq is unchanged
    s = NF.attention_score(qg, k, bias, vn, md, backend="native")
    s.backward(ds)
    assert torch.equal(s.detach().cpu(), full)
    assert torch.equal(qg.grad.cpu(), grads[0])
    # only k
    kg = k.clone().requires_grad_(True)
    NF.attention_score(q, kg, bias, vn, md, backend="native").backward(ds)
    assert torch.equal(kg.grad.cpu(), grads[1])


# ---------------------------------------------------------- argument checks
def test_arguments_are_checked():
    from ddlbench_amd import ops
    ext = ops.require_extension()
    dev = _dev()
    q = torch.zeros(2, 3, 16, device=dev)
    k = torch.zeros(2, 5, 16, device=dev)
    b = torch.zeros(16, device=dev)
    vn = torch.zeros(16, device=dev)
    ds = torch.zeros(2, 3, 5, device=dev)
    m = torch.ones(2, 5, dtype=torch.bool, device=dev)
    assert ext.attn_score_fwd(q, k, b, vn, m).shape == (2, 3, 5)
    with pytest.raises(RuntimeError, match="share one dtype"):
        ext.attn_score_fwd(q, k.bfloat16(), b, vn, None)
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        ext.attn_score_fwd(q.half(), k.half(), b.half(), vn.half(), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ext.attn_score_fwd(q.cpu(), k, b, vn, None)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.attn_score_fwd(torch.zeros(2, 3, 32, device=dev)[..., ::2], k, b,
                           vn, None)
    with pytest.raises(RuntimeError, match=r"vn must be \(H,\)"):
        ext.attn_score_fwd(q, k, b, torch.zeros(8, device=dev), None)
    with pytest.raises(RuntimeError, match=r"k must be \(B, Tk, H\)"):
        ext.attn_score_fwd(q, torch.zeros(2, 5, 8, device=dev), b, vn, None)
    with pytest.raises(RuntimeError, match=r"mask must be \(B, Tk\)"):
        ext.attn_score_fwd(q, k, b, vn, m[:, :4].contiguous())
    with pytest.raises(RuntimeError, match="bool or uint8"):
        ext.attn_score_fwd(q, k, b, vn, m.long())
    with pytest.raises(RuntimeError, match=r"ds must be \(B, Tq, Tk\)"):
        ext.attn_score_bwd(ds[:, :2].contiguous(), q, k, b, vn, None)
    with pytest.raises(RuntimeError, match="ds must have q's dtype"):
        ext.attn_score_bwd(ds.bfloat16(), q, k, b, vn, None)


# ------------------------------------------------------------------ wiring
def test_attention_module_runs_the_native_kernels(monkeypatch):
    from ddlbench_amd import ops
    from ddlbench_amd.models.gnmt import BahdanauAttention
    ext = ops.require_extension()
    calls = []
    real = ext.attn_score_fwd

    def spy(*args):
        calls.append(tuple(args[0].shape))
        return real(*args)

    monkeypatch.setattr(ext, "attn_score_fwd", spy)
    monkeypatch.delenv("DDLB_ATTN_SCORE", raising=False)
    dev = _dev()
    torch.manual_seed(11)
    native = BahdanauAttention(128, 128, 128).to(dev)
    eager = BahdanauAttention(128, 128, 128, backend="torch").to(dev)
    eager.load_state_dict(native.state_dict())
    with torch.no_grad():       # a bias that is not all zeros
        native.b.normal_(0, 0.1)
        eager.b.copy_(native.b)
    g = torch.Generator().manual_seed(12)
    query = torch.randn(3, 17, 128, generator=g).to(dev)
    keys = torch.randn(3, 20, 128, generator=g).to(dev)
    mask = _lengths_mask(3, 20).to(dev)
    up = torch.randn(3, 17, 128, generator=g).to(dev)
    ctx_n, attn_n = native(query, keys, mask)
    assert calls == [(3, 17, 128)]
    ctx_e, attn_e = eager(query, keys, mask)
    assert calls == [(3, 17, 128)]
    torch.testing.assert_close(ctx_n, ctx_e, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(attn_n, attn_e, rtol=1e-5, atol=1e-5)
    (ctx_n * up).sum().backward()
    (ctx_e * up).sum().backward()
    for (name, a), (_, b) in zip(native.named_parameters(),
                                 eager.named_parameters()):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    # the environment switches an "auto" module to the torch path
    monkeypatch.setenv("DDLB_ATTN_SCORE", "torch")
    native(query, keys, mask)
    assert calls == [(3, 17, 128)]


def test_greedy_decode_agrees_between_backends():
    from ddlbench_amd.models.gnmt import GNMT
    from ddlbench_amd.translation import Translator
    dev = _dev()
    torch.manual_seed(21)
    model = GNMT(vocab_size=96, hidden_size=64, num_layers=2).to(dev)
    src = torch.randint(3, 96, (9, 4), device=dev)
    src_len = torch.tensor([9, 7, 4, 2], device=dev)
    outs = {}
    for backend in ("native", "torch"):
        model.decoder.att_rnn.attn.backend = backend
        outs[backend] = Translator(model, max_len=6).greedy(src, src_len)
    assert torch.equal(outs["native"], outs["torch"])
