"""Native label-smoothed cross-entropy (ls_ce_* kernels) against a float64
CPU oracle computed from the same, already dtype-rounded inputs. All @gpu.

Widths are the smallest that reach each code path:
  8      one wave per row
  1000   one wave per row, ragged tail
  4096   first four-wave row; 512 vectors = an exact multiple of the block
  4104   four waves, ragged vector tail
  4100   bf16 without 16 B loads (odd rows are not 16 B aligned)
  32320  GNMT's width
Rows: 1, and 7 with the first, the last and one middle row ignored.

Tolerances. The arithmetic is fp32 for both dtypes, so the loss is held to
rtol = atol = 1e-5. Gradients are compared after the reduction's scale is
divided out (dx * max(n_valid, 1) for "mean"), so a zeroed or mis-scaled
gradient cannot hide under the absolute term: fp32 at rtol = atol = 1e-5,
bf16 at |err| <= 2^-8 |ref| + 1e-5: dx is rounded to nearest once, into 8
significant bits, which moves it by half an ulp = 2^-9 of its binade's upper
end, so by at most 2^-8 |ref| for a value just above a power of two; the
absolute term covers the fp32 error of the value that is rounded."""

import functools
import warnings

import pytest
import torch

from ddlbench_amd.ops import functional as NF

pytestmark = pytest.mark.gpu

WIDTHS = [8, 1000, 4096, 4104, 4100, 32320]
DTYPES = [torch.float32, torch.bfloat16]


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"


def _oracle(x, t, eps, ign):
    """float64 loss sum and its gradient (the unscaled per-row gradient)."""
    x64 = x.double().requires_grad_(True)
    s = NF.label_smoothing_cross_entropy(x64, t, eps, ign, "sum",
                                         backend="torch")
    s.backward()
    return s.detach(), x64.grad


def _targets(R, K, ign, ignored, g):
    t = torch.randint(1, K, (R,), generator=g) if K > 1 \
        else torch.zeros(R, dtype=torch.long)
    t[t == ign] = 1
    t[-1 if R == 1 else 1] = K - 1          # last element of a row
    if R > 2:
        t[2] = 1                            # first vector of a row
    t[list(ignored)] = ign
    return t


@functools.lru_cache(maxsize=None)
def _case(K, R, dtype, ign=0, ignored=None):
    """Inputs and oracle, built once per shape and shared (read-only)."""
    if ignored is None:
        ignored = (0, 3, 6) if R == 7 else ()
    g = torch.Generator().manual_seed(1000 * K + R)
    x = (torch.randn(R, K, generator=g) * 2).to(dtype)
    t = _targets(R, K, ign, ignored, g)
    ref = {eps: _oracle(x, t, eps, ign) for eps in (0.0, 0.1)}
    return x, t, ref, int((t != ign).sum())


def _native(x, t, eps, ign, reduction, upstream=None):
    xd = x.to(_dev(), copy=True).requires_grad_(True)
    loss = NF.label_smoothing_cross_entropy(xd, t.to(_dev()), eps, ign,
                                            reduction, backend="native")
    (loss if upstream is None else upstream * loss).backward()
    return loss.detach().cpu(), xd.grad.cpu()


def _check(loss, dx, ref, n_valid, reduction, dtype, rows=None, tag=""):
    ref_sum, ref_g = ref
    div = max(n_valid, 1) if reduction == "mean" else 1
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert dx.dtype == dtype
    got = dx.double() * div
    if rows is not None:
        got, ref_g = got[rows], ref_g[rows]
    err = (got - ref_g).abs()
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-5
    bound = rel * ref_g.abs() + 1e-5
    print(f"{tag} {reduction}: loss {loss.item():.8g} ref "
          f"{(ref_sum / div).item():.8g}  max grad err {err.max().item():.3g}"
          f"  worst err/bound {(err / bound).max().item():.3g}")
    if rows is None:
        torch.testing.assert_close(loss.double(), ref_sum / div, rtol=1e-5,
                                   atol=1e-5)
    assert torch.isfinite(got).all()
    assert (err <= bound).all()


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("R", [1, 7])
@pytest.mark.parametrize("K", WIDTHS)
def test_values(K, R, dtype):
    x, t, ref, n_valid = _case(K, R, dtype)
    for eps in (0.0, 0.1):
        for reduction in ("mean", "sum"):
            loss, dx = _native(x, t, eps, 0, reduction)
            _check(loss, dx, ref[eps], n_valid, reduction, dtype,
                   tag=f"K={K} R={R} eps={eps}")
            assert (dx[t == 0] == 0).all()


# --------------------------------------------------------------- rescaling
@functools.lru_cache(maxsize=None)
def _rescale_case(K, dtype):
    x = torch.full((4, K), -200.0)
    x[0, 0] = 200.0                          # maximum first
    x[1, K - 1] = 200.0                      # maximum last
    x[2] = torch.linspace(-200.0, 200.0, K)  # the running max moves at
    x[3] = torch.linspace(200.0, -200.0, K)  # every step / never again
    x = x.to(dtype)
    t = torch.tensor([0, 5, K - 1, K - 2])
    return x, t, {eps: _oracle(x, t, eps, -100) for eps in (0.0, 0.1)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [4104, 32320])
def test_rescaling(K, dtype):
    x, t, ref = _rescale_case(K, dtype)
    for eps in (0.0, 0.1):
        loss, dx = _native(x, t, eps, -100, "mean")
        assert torch.isfinite(loss) and torch.isfinite(dx.float()).all()
        _check(loss, dx, ref[eps], 4, "mean", dtype,
               tag=f"rescale K={K} eps={eps}")


# ------------------------------------------------- ignored rows are not read
@pytest.mark.parametrize("K,dtype", [(1000, torch.float32),
                                     (4104, torch.bfloat16),
                                     (4100, torch.bfloat16)])
def test_ignored_rows_are_not_read(K, dtype):
    x, t, ref, n_valid = _case(K, 7, dtype)
    loss0, dx0 = _native(x, t, 0.1, 0, "mean")
    xp = x.clone()
    xp[0] = float("nan")
    xp[3] = float("inf")
    xp[6] = float("nan")
    loss1, dx1 = _native(xp, t, 0.1, 0, "mean")
    assert torch.isfinite(loss1)
    assert torch.equal(loss1, loss0)
    assert torch.equal(dx1, dx0)
    assert torch.isfinite(dx1.float()).all()
    assert (dx1[[0, 3, 6]] == 0).all()
    _check(loss1, dx1, ref[0.1], n_valid, "mean", dtype, tag=f"nan K={K}")


# -------------------------------------------------------------- all ignored
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("K,dtype", [(8, torch.float32),
                                     (4104, torch.bfloat16)])
def test_all_ignored(K, dtype, reduction):
    x = _case(K, 7, dtype)[0]
    t = torch.zeros(7, dtype=torch.long)
    loss, dx = _native(x, t, 0.1, 0, reduction)
    assert loss.item() == 0.0
    assert not torch.isnan(dx.float()).any()
    assert (dx == 0).all()


# ---------------------------------------------------- negative ignore_index
@pytest.mark.parametrize("K,dtype", [(1000, torch.float32),
                                     (4104, torch.bfloat16)])
def test_negative_ignore_index(K, dtype):
    x, t, ref, n_valid = _case(K, 7, dtype, -100, (2, 3))
    assert n_valid == 5
    for reduction in ("mean", "sum"):
        loss, dx = _native(x, t, 0.1, -100, reduction)
        _check(loss, dx, ref[0.1], n_valid, reduction, dtype,
               tag=f"ign=-100 K={K}")
        assert (dx[[2, 3]] == 0).all()


# --------------------------------------------------------------- bad target
@pytest.mark.parametrize("K,dtype", [(1000, torch.float32),
                                     (4104, torch.bfloat16),
                                     (4100, torch.bfloat16)])
def test_bad_target(K, dtype):
    # bad targets in middle rows only: even an unguarded x[t] would stay
    # inside the allocation
    x, t, ref, _ = _case(K, 7, dtype, 0, ())
    tb = t.clone()
    tb[2] = K
    tb[4] = -1
    good = [0, 1, 3, 5, 6]
    for reduction in ("mean", "sum"):
        loss, dx = _native(x, tb, 0.1, 0, reduction)
        assert torch.isnan(loss)
        assert torch.isnan(dx[[2, 4]].float()).all()
        # bad rows are not the ignore index, so they count as tokens
        _check(loss, dx, ref[0.1], 7, reduction, dtype, rows=good,
               tag=f"bad target K={K}")


# -------------------------------------------------------------- determinism
def test_bitwise_reproducible():
    x, t, _, _ = _case(32320, 7, torch.bfloat16)
    a = _native(x, t, 0.1, 0, "mean")
    b = _native(x, t, 0.1, 0, "mean")
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])


# -------------------------------------------------------- upstream gradient
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_upstream_gradient_scales(reduction):
    x, t, _, n_valid = _case(1000, 7, torch.float32)
    _, g1 = _native(x, t, 0.1, 0, reduction)
    _, g3 = _native(x, t, 0.1, 0, reduction, upstream=3.0)
    div = n_valid if reduction == "mean" else 1
    assert (g1 * div).abs().max() > 0.5
    # the fp32 tolerance of the value tests, on gradients with the
    # reduction's scale divided out (entries up to 3 in magnitude)
    torch.testing.assert_close(g3 * div, 3 * g1 * div, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------- layout
def test_tbv_noncontiguous_and_no_grad():
    T, B, V = 5, 3, 1000
    x, t, ref, n_valid = _case(V, T * B, torch.float32, 0, (0, 7, 14))
    dev = _dev()
    # (T, B, V) logits that are a slice of a wider tensor
    wide = torch.zeros(T, B, V + 8, device=dev)
    wide[..., :V] = x.view(T, B, V).to(dev)
    xv = wide[..., :V].requires_grad_(True)
    assert not xv.is_contiguous()
    td = t.view(T, B).to(dev)
    loss = NF.label_smoothing_cross_entropy(xv, td, 0.1, 0,
                                            backend="native")
    loss.backward()
    assert xv.grad.shape == (T, B, V)
    _check(loss.detach().cpu(), xv.grad.cpu().view(T * B, V), ref[0.1],
           n_valid, "mean", torch.float32, tag="(T,B,V) view")
    with torch.no_grad():
        l2 = NF.label_smoothing_cross_entropy(xv, td, 0.1, 0,
                                              backend="native")
    assert l2.grad_fn is None and not l2.requires_grad
    assert torch.equal(l2, loss.detach())


# --------------------------------------------------------- no host sync
def test_no_host_synchronisation():
    x, t, _, _ = _case(4104, 7, torch.bfloat16)
    xd = x.to(_dev()).requires_grad_(True)
    td = t.to(_dev())
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        # torch announces the debug mode as a prototype
        warnings.simplefilter("ignore", UserWarning)
        torch.cuda.set_sync_debug_mode("error")
    try:
        loss = NF.label_smoothing_cross_entropy(xd, td, 0.1, 0,
                                                backend="native")
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss).item()


# ---------------------------------------------------------- argument checks
def test_target_dtype_and_device_are_checked():
    from ddlbench_amd import ops
    ext = ops.require_extension()
    x = torch.zeros(4, 16, device=_dev())
    t = torch.ones(4, dtype=torch.long, device=_dev())
    with pytest.raises(RuntimeError, match="int64"):
        ext.ls_ce_fwd(x, t.int(), 0.1, 0, True)
    with pytest.raises(RuntimeError, match="HIP device"):
        ext.ls_ce_fwd(x, t.cpu(), 0.1, 0, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.ls_ce_fwd(x[:, ::2], t, 0.1, 0, True)


# -------------------------------------------------------------- GNMT wiring
def test_gnmt_loss_runs_the_native_kernels(monkeypatch):
    from ddlbench_amd import ops
    from ddlbench_amd.models.gnmt import PAD, LabelSmoothingLoss
    ext = ops.require_extension()
    calls = []
    real = ext.ls_ce_fwd

    def spy(*args):
        calls.append(args[0].shape)
        return real(*args)

    monkeypatch.setattr(ext, "ls_ce_fwd", spy)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(5, 3, 512, generator=g).to(_dev())
    t = torch.randint(1, 512, (5, 3), generator=g)
    t[3:, 1] = PAD
    t = t.to(_dev())
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    l1 = LabelSmoothingLoss()(x1, t)
    assert calls == [(15, 512)]
    l2 = LabelSmoothingLoss(backend="torch")(x2, t)
    assert calls == [(15, 512)]
    l1.backward()
    l2.backward()
    torch.testing.assert_close(l1, l2, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-5, atol=1e-5)
