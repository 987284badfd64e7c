"""Every dispatch path of the fused BN+act kernels through ext.bn_act_fwd /
ext.bn_act_bwd, case by case from tests/bn_cases.py. Each case first
asserts, from the launchers' own plan, the kernel kinds it was chosen for.

Reference check: float64 BN(+res)+act and its autograd from the same
inputs, at the tolerances test_kernels_gpu.py uses: 2e-5 (fp32) / 2e-2
(bf16) on y, dx and dres, with the clamp-boundary band excluded for bf16
activations; 1e-4 on the running statistics; dgamma/dbeta bounded by the
out-of-band contributions.
Exactness: x in {-2..2}, dy in {-1..1}, act none — every partial sum is an
integer, so mean, dbeta and running_mean equal the float64 values bit for
bit on every reduce kind.
Cross-check: for relu, backward from the 1-bit mask equals backward from y
bit for bit (the two instantiations differ only in where the gate comes
from). Not asserted for relu6: the mask is taken from the fp32 value and
bf16(v) can round up to 6.0."""

import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in bc.CASES]


@pytest.fixture(scope="module")
def ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"
    return ops.require_extension()


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def results(ext):
    """Each case runs once; the tests share the outputs read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bc.run_case(ext, bc.CASE_BY_NAME[name], _dev())
        return cache[name]
    return get


def _band(case, y64):
    band = torch.ones_like(y64, dtype=torch.bool)
    if case.act != "none" and case.dtype is bc.BF:
        band = y64.abs() > 0.05
        if case.act == "relu6":
            band &= (y64 - 6.0).abs() > 0.3
    return band


@pytest.mark.parametrize("name", NAMES)
def test_case_against_float64_reference(ext, results, name):
    case = bc.CASE_BY_NAME[name]
    missing = set(case.claims) - bc.reached(ext, case)
    assert not missing, f"{name} no longer reaches {sorted(missing)}"
    pl = bc.plan(ext, case)
    r, ref = results(name), bc.reference64(name)
    assert ("mask" in r) == pl["writes_mask"] == bc.writes_mask(case)

    tol = 2e-2 if case.dtype is bc.BF else 2e-5
    y = r["y"].cpu().double().contiguous()
    print(f"{name}: max |y - ref| = {(y - ref['y']).abs().max().item():.3e}")
    torch.testing.assert_close(y, ref["y"], rtol=tol, atol=tol)
    for k in ("mean", "invstd", "rm", "rv"):
        torch.testing.assert_close(r[k].cpu().double(), ref[k], rtol=1e-4,
                                   atol=1e-4)

    band = _band(case, ref["y"])
    dy64 = bc.case_inputs(name)["dy"].double().contiguous()
    oob = (~band).double()
    slack_g = (dy64.abs() * ref["xhat"].abs() * oob).sum(dim=(0, 2, 3)) \
        + 1e-2 + 1e-3 * ref["dgamma"].abs()
    slack_b = (dy64.abs() * oob).sum(dim=(0, 2, 3)) \
        + 1e-2 + 1e-3 * ref["dbeta"].abs()
    for gate in case.bwd:
        dx = r[f"dx@{gate}"].cpu().double().contiguous()
        print(f"{name}@{gate}: max in-band |dx - ref| = "
              f"{(dx - ref['dx'])[band].abs().max().item():.3e}")
        torch.testing.assert_close(dx[band], ref["dx"][band], rtol=tol,
                                   atol=tol * 10)
        dg = r[f"dgamma@{gate}"].cpu().double()
        db = r[f"dbeta@{gate}"].cpu().double()
        assert ((dg - ref["dgamma"]).abs() <= slack_g + 0.05 *
                ref["dgamma"].abs().max()).all()
        assert ((db - ref["dbeta"]).abs() <= slack_b + 0.05 *
                ref["dbeta"].abs().max()).all()
        if case.res:
            dres = r[f"dres@{gate}"].cpu().double().contiguous()
            torch.testing.assert_close(dres[band], ref["dres"][band],
                                       rtol=tol, atol=tol * 10)


EXACT = sorted({(c.shape, c.dtype, c.nhwc) for c in bc.CASES},
               key=lambda t: (str(t[1]), t[2], t[0]))


@pytest.mark.parametrize(
    "shape,dtype,nhwc", EXACT,
    ids=["x".join(map(str, s)) + "-" + bc.dtype_name(d) +
         ("-nhwc" if n else "-nchw") for s, d, n in EXACT])
def test_integer_inputs_are_exact(ext, shape, dtype, nhwc):
    C = shape[1]
    x, dy = (t.to(_dev()) for t in bc.integer_inputs(shape, dtype, nhwc))
    gamma = torch.ones(C, device=_dev())
    beta = torch.zeros(C, device=_dev())
    rm = torch.zeros(C, device=_dev())
    rv = torch.ones(C, device=_dev())
    y, mean, invstd = ext.bn_act_fwd(x, None, gamma, beta, rm, rv, True,
                                     bc.MOM, bc.EPS, 0, nhwc)
    dx, dgamma, dbeta = ext.bn_act_bwd(dy, y, x, mean, invstd, gamma, 0,
                                       True, False, nhwc, None)
    x64, dy64 = x.cpu().double(), dy.cpu().double()
    m64 = x64.mean(dim=(0, 2, 3))
    assert torch.equal(mean.cpu(), m64.float()), "mean not exact"
    mom = torch.tensor(bc.MOM, dtype=torch.float32)
    assert torch.equal(rm.cpu(), (1 - mom) * torch.zeros(C)
                       + mom * m64.float()), "running_mean not exact"
    assert torch.equal(dbeta.cpu(), dy64.sum(dim=(0, 2, 3)).float()), \
        "dbeta not exact"


@pytest.mark.parametrize("name", bc.CROSS_CHECK)
def test_masked_backward_equals_backward_from_y(ext, results, name):
    case = bc.CASE_BY_NAME[name]
    assert bc.plan(ext, case, masked=True)["dx_gate"] == "mask"
    assert bc.plan(ext, case, masked=False)["dx_gate"] == "y"
    r = results(name)
    for k in ("dx", "dgamma", "dbeta") + (("dres",) if case.res else ()):
        assert torch.equal(r[f"{k}@mask"], r[f"{k}@y"]), \
            f"{name}: {k} differs between the mask and y"


# --------------------------------------------------------- bad arguments
@pytest.fixture(scope="module")
def fwd8(ext):
    """A small masked forward whose backward the guard tests call."""
    case = bc.CASE_BY_NAME["c8_relu_train"]
    d = bc.case_inputs(case.name)
    dev = _dev()
    x, dy, gamma = d["x"].to(dev), d["dy"].to(dev), d["gamma"].to(dev)
    y, mean, invstd, mask = ext.bn_act_fwd(
        x, None, gamma, d["beta"].to(dev), None, None, True, bc.MOM, bc.EPS,
        1, True)

    def bwd(dy=dy, y=y, mask=None):
        return ext.bn_act_bwd(dy, y, x, mean, invstd, gamma, 1, True, False,
                              True, mask)
    bwd(mask=mask, y=None)          # the well-formed calls pass
    bwd()
    return bwd, dy, mask


def test_bwd_rejects_dy_of_another_size(fwd8):
    bwd, dy, mask = fwd8
    bad = torch.zeros(2, 8, 4, 5, device=dy.device, dtype=dy.dtype) \
        .contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="size"):
        bwd(dy=bad)


def test_bwd_rejects_dy_of_another_dtype(fwd8):
    bwd, dy, mask = fwd8
    with pytest.raises(RuntimeError, match="dtype"):
        bwd(dy=dy.float())


def test_bwd_rejects_dy_of_another_layout(fwd8):
    bwd, dy, mask = fwd8
    bad = dy.contiguous()           # NCHW strides for an NHWC x
    assert not bad.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="layout"):
        bwd(dy=bad)


def test_bwd_rejects_mask_of_wrong_length(fwd8):
    bwd, dy, mask = fwd8
    with pytest.raises(RuntimeError, match="mask"):
        bwd(y=None, mask=mask[:-1].contiguous())


def test_bwd_needs_y_where_no_masked_kernel_exists(ext):
    """C % 8 != 0 has no masked kernel: a mask alone is not enough."""
    dev = _dev()
    x = torch.randn(2, 12, 4, 4, device=dev, dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.ones(12, device=dev), torch.zeros(12, device=dev)
    y, mean, invstd = ext.bn_act_fwd(x, None, gamma, beta, None, None, True,
                                     bc.MOM, bc.EPS, 1, True)
    mask = torch.zeros(x.numel() // 8, device=dev, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="y is needed"):
        ext.bn_act_bwd(x, None, x, mean, invstd, gamma, 1, True, False, True,
                       mask)
