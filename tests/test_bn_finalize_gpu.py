"""BN finalize kernel (slabs -> per-channel results in one launch) through
ext.bn_act_fwd / ext.bn_act_bwd, NHWC.

Shapes are the smallest that reach each finalize geometry:
  (8,64,64,64)   S=2048, fp32 slabs, 64 slab chunks per channel chunk
  (8,512,16,16)  S=128, the widest vec block, 16 channel chunks
  (4,1024,8,8)   C > 512: scalar reduce, double slabs, cblocks > 1
  (2,8,4,4)      S=2: fewer slabs than one chunk (no hand-off)
  (3,24,5,7)     odd row count, C no multiple of the 32-channel chunk
fp32 inputs take the double-slab path at any C.

Exact cases: x in {-2..2}, dy in {-1..1}, act=none — every partial sum is
an integer, exact in fp32 and double in any order, so mean / dbeta /
running_mean must match the float64 reference bit for bit; invstd and
running_var go through the device's double rsqrt (and a possibly fused
multiply-add) and may differ by one float32 ulp.
Random cases: float64 reference from the same inputs and the kernel's own
activation mask, rtol=atol=1e-4 (the tolerance test_kernels_gpu.py uses
for the running statistics); two calls must agree bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOM = 0.1
CL = torch.channels_last

SHAPES = [(8, 64, 64, 64), (8, 512, 16, 16), (4, 1024, 8, 8), (2, 8, 4, 4),
          (3, 24, 5, 7)]
BF16 = [(s, torch.bfloat16) for s in SHAPES]
FP32 = [((3, 24, 5, 7), torch.float32), ((8, 64, 16, 16), torch.float32)]


def _id(p):
    shape, dtype = p
    return "x".join(map(str, shape)) + ("-bf16" if dtype is torch.bfloat16
                                        else "-fp32")


@pytest.fixture(scope="module")
def ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"
    return ops.require_extension()


def _dev():
    return torch.device("cuda", 0)


def _ints(shape, lo, hi, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).to(dtype)
    return t.to(_dev()).contiguous(memory_format=CL)


def _randn(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(_dev()) \
        .contiguous(memory_format=CL)


def _fwd(ext, x, res, gamma, beta, act):
    C = x.size(1)
    rm = torch.zeros(C, device=x.device)
    rv = torch.ones(C, device=x.device)
    out = ext.bn_act_fwd(x, res, gamma, beta, rm, rv, True, MOM, EPS, act,
                         True)
    return out, rm, rv


def _bwd(ext, dy, y, x, mean, invstd, gamma, act, msk=None):
    return ext.bn_act_bwd(dy, y, x, mean, invstd, gamma, act, True, False,
                          True, msk)


def _stats64(x):
    """float64 per-channel sums -> the kernel's documented formulas."""
    x64 = x.double()
    count = x64.numel() // x64.size(1)
    s = x64.sum(dim=(0, 2, 3))
    ss = (x64 * x64).sum(dim=(0, 2, 3))
    m = s / count
    var = (ss / count - m * m).clamp_min(0.0)
    invstd = torch.rsqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))
    unbiased = var * count / (count - 1) if count > 1 else var
    return m, var, invstd, unbiased


def _running(prev, new32):
    """(1 - momentum) * running + momentum * new, in float32 as the kernel
    computes it."""
    mom = torch.tensor(MOM, dtype=torch.float32, device=prev.device)
    return (1 - mom) * prev + mom * new32


def _within_one_ulp(got, ref):
    up = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    dn = torch.nextafter(ref, torch.full_like(ref, float("-inf")))
    return bool(((got == ref) | (got == up) | (got == dn)).all())


# --------------------------------------------------------------- exact
def _check_exact(ext, shape, dtype, seed=1):
    C = shape[1]
    x = _ints(shape, -2, 2, dtype, seed)
    dy = _ints(shape, -1, 1, dtype, seed + 100)
    gamma = torch.ones(C, device=_dev())
    beta = torch.zeros(C, device=_dev())
    (y, mean, invstd, *_), rm, rv = _fwd(ext, x, None, gamma, beta, 0)
    m64, var64, is64, unb64 = _stats64(x)
    assert torch.equal(mean, m64.float()), "mean not exact"
    assert _within_one_ulp(invstd, is64.float()), "invstd beyond 1 ulp"
    assert torch.equal(rm, _running(torch.zeros_like(rm), m64.float())), \
        "running_mean not exact"
    assert _within_one_ulp(
        rv, _running(torch.ones_like(rv), unb64.float())), \
        "running_var beyond 1 ulp"
    dx, dgamma, dbeta = _bwd(ext, dy, y, x, mean, invstd, gamma, 0)
    want_dbeta = dy.double().sum(dim=(0, 2, 3))
    assert torch.equal(dbeta, want_dbeta.float()), "dbeta not exact"
    # dgamma = sum dy * (x - mean) * invstd is not integer-valued
    xhat = (x.double() - mean.double().view(1, C, 1, 1)) \
        * invstd.double().view(1, C, 1, 1)
    want_dgamma = (dy.double() * xhat).sum(dim=(0, 2, 3))
    torch.testing.assert_close(dgamma, want_dgamma.float(), rtol=1e-4,
                               atol=1e-4)


@pytest.mark.parametrize("case", BF16 + FP32, ids=_id)
def test_exact_integer_inputs(ext, case):
    _check_exact(ext, *case)


# -------------------------------------------------------------- random
def _run_random(ext, shape, dtype, with_res, seed):
    C = shape[1]
    x = _randn(shape, dtype, seed)
    res = _randn(shape, dtype, seed + 1) if with_res else None
    dy = _randn(shape, dtype, seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    gamma = (torch.rand(C, generator=g) + 0.5).to(_dev())
    beta = torch.randn(C, generator=g).to(_dev())
    fwd, rm, rv = _fwd(ext, x, res, gamma, beta, 1)
    y, mean, invstd = fwd[0], fwd[1], fwd[2]
    msk = fwd[3] if len(fwd) > 3 else None
    dx, dgamma, dbeta = _bwd(ext, dy, y, x, mean, invstd, gamma, 1, msk)
    return dict(x=x, dy=dy, y=y, mean=mean, invstd=invstd, rm=rm, rv=rv,
                dgamma=dgamma, dbeta=dbeta)


def _check_random(r):
    x, C = r["x"], r["x"].size(1)
    m64, var64, is64, unb64 = _stats64(x)
    tol = dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(r["mean"], m64.float(), **tol)
    torch.testing.assert_close(r["invstd"], is64.float(), **tol)
    torch.testing.assert_close(
        r["rm"], _running(torch.zeros_like(r["rm"]), m64.float()), **tol)
    torch.testing.assert_close(
        r["rv"], _running(torch.ones_like(r["rv"]), unb64.float()), **tol)
    gate = (r["y"] > 0).double()          # the kernel's own mask
    g = r["dy"].double() * gate
    xhat = (x.double() - m64.view(1, C, 1, 1)) * is64.view(1, C, 1, 1)
    torch.testing.assert_close(r["dbeta"], g.sum(dim=(0, 2, 3)).float(),
                               **tol)
    torch.testing.assert_close(r["dgamma"],
                               (g * xhat).sum(dim=(0, 2, 3)).float(), **tol)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("case", BF16 + FP32[:1], ids=_id)
def test_random_inputs_and_determinism(ext, case, with_res):
    shape, dtype = case
    a = _run_random(ext, shape, dtype, with_res, seed=7)
    b = _run_random(ext, shape, dtype, with_res, seed=7)
    _check_random(a)
    for name in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta"):
        assert torch.equal(a[name], b[name]), f"{name} differs between calls"


# ------------------------------------------------- back-to-back layers
def test_back_to_back_layers_share_workspace(ext):
    """Large C*S, then a small layer, then another large one on the same
    stream with no sync in between: the slab workspace, the second-level
    partials and the ticket words are reused call after call."""
    shapes = [(8, 64, 64, 64), (2, 8, 4, 4), (8, 512, 16, 16),
              (4, 1024, 8, 8), (8, 64, 64, 64)]
    runs = [_run_random(ext, s, torch.bfloat16, False, seed=20 + i)
            for i, s in enumerate(shapes)]
    torch.cuda.synchronize()
    for r in runs:
        _check_random(r)
