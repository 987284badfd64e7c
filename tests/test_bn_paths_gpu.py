"""Every dispatch path of the fused BN+act kernels through ext.bn_act_fwd /
ext.bn_act_bwd, case by case from tests/bn_cases.py. Each case first
asserts, from the launchers' own plan, the kernel kinds it was chosen for.

Reference check: float64 BN(+res)+act from the same inputs, 2e-5 (fp32) /
2e-2 (bf16) on y (the tolerances of test_kernels_gpu.py) and 1e-4 on the
statistics. The backward reference is the float64 formulas with the gate
the kernel itself used (the returned y, or the unpacked returned mask), so
every element of dx and dres is compared, and dgamma/dbeta at
rtol = atol = 1e-4, the tolerance of test_bn_finalize_gpu.py.
Dyadic data (bn_cases.dyadic_inputs; proven sound on the CPU by
test_bn_cases_cpu.py): the whole computation is exact, so the statistics,
y, the mask bits, dgamma, dbeta, dres and (for a power-of-two row count)
dx equal the float64 values bit for bit on every path, and backward from
the mask equals backward from y for relu and relu6.
Exactness: x in {-2..2}, dy in {-1..1}, act none — every partial sum is an
integer, so mean, dbeta and running_mean equal the float64 values bit for
bit on every reduce kind.
Cross-check on random data: for relu, backward from the 1-bit mask equals
backward from y bit for bit (the two instantiations differ only in where
the gate comes from). Not asserted for relu6 there: the mask is taken from
the fp32 value and bf16(v) can round up to 6.0.
Large means: invstd and y against the library's batch norm on inputs whose
mean is up to 16 (reported: 64) standard deviations."""

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


@pytest.fixture(scope="module")
def dyadic(ext):
    """Each case once on the dyadic data."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bc.run_dyadic(ext, bc.CASE_BY_NAME[name], _dev())
        return cache[name]
    return get


def _f64(t):
    return t.cpu().double().contiguous()


@pytest.mark.parametrize("name", NAMES)
def test_case_against_float64_reference(ext, results, name):
    case = bc.CASE_BY_NAME[name]
    missing = set(case.claims) - bc.reached(ext, case)
    assert not missing, f"{name} no longer reaches {sorted(missing)}"
    pl = bc.plan(ext, case)
    r, ref = results(name), bc.reference64(name)
    assert ("mask" in r) == pl["writes_mask"] == bc.writes_mask(case)

    tol = 2e-2 if case.dtype is bc.BF else 2e-5
    y = _f64(r["y"])
    print(f"{name}: max |y - ref| = {(y - ref['y']).abs().max().item():.3e}")
    torch.testing.assert_close(y, ref["y"], rtol=tol, atol=tol)
    for k in ("mean", "invstd", "rm", "rv"):
        torch.testing.assert_close(r[k].cpu().double(), ref[k], rtol=1e-4,
                                   atol=1e-4)

    d = bc.case_inputs(name)
    for gate in case.bwd:
        # float64 statistics, the kernel's own gate: nothing to exclude
        b = bc.formulas64(case, d, ref["mean"], ref["invstd"],
                          bc.kernel_gate(case, r, gate))
        dx = _f64(r[f"dx@{gate}"])
        dg, db = _f64(r[f"dgamma@{gate}"]), _f64(r[f"dbeta@{gate}"])
        print(f"{name}@{gate}: max |dx - ref| = "
              f"{(dx - b['dx']).abs().max().item():.3e}, |dgamma - ref| = "
              f"{(dg - b['dgamma']).abs().max().item():.3e}, |dbeta - ref| "
              f"= {(db - b['dbeta']).abs().max().item():.3e}")
        torch.testing.assert_close(dx, b["dx"], rtol=tol, atol=tol * 10)
        torch.testing.assert_close(dg, b["dgamma"], rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(db, b["dbeta"], rtol=1e-4, atol=1e-4)
        if case.res:
            torch.testing.assert_close(_f64(r[f"dres@{gate}"]), b["dres"],
                                       rtol=tol, atol=tol * 10)


# ---------------------------------------------------------- dyadic data
def _mismatches(got, ref64):
    """Elements of got that differ from the float64 reference rounded once
    to got's dtype."""
    want = ref64.to(got.dtype)
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return int((got.cpu() != want).sum().item())


def _is_pow2(n):
    return n & (n - 1) == 0


@pytest.mark.parametrize("name", NAMES)
def test_dyadic_exact(ext, dyadic, name):
    case = bc.CASE_BY_NAME[name]
    d, r = bc.dyadic_inputs(name), dyadic(name)
    N, C, H, W = case.shape
    R, P, m = d["R"], d["P"], d["m"]
    half = torch.full((C,), 0.5, dtype=torch.float32)
    bf = case.dtype is bc.BF
    rel32 = 4.0 * 2.0 ** -24

    # ---- forward statistics
    mean, invstd = r["mean"].cpu(), r["invstd"].cpu()
    assert torch.equal(mean, m.float()), "mean is not m_c"
    if case.training:
        assert torch.equal(invstd, half), "invstd is not 0.5"
        assert torch.equal(r["rm"].cpu(),
                           (0.5 * d["rm"].double() + 0.5 * m).float()), \
            "running_mean not exact"
        unbiased = 8.0 * P / (R - 1) if R > 1 else 0.0
        want_rv = torch.full((C,), 0.5 * unbiased,
                             dtype=torch.float64).float()
        assert bc.within_one_ulp(r["rv"].cpu(), want_rv), \
            "running_var beyond 1 ulp"
        exact = True
    else:
        assert bc.within_one_ulp(invstd, half), "invstd beyond 1 ulp of 0.5"
        assert torch.equal(r["rm"].cpu(), d["rm"]), "eval wrote running_mean"
        assert torch.equal(r["rv"].cpu(), d["rv"]), "eval wrote running_var"
        exact = bool((invstd == half).all())
        if not exact:
            print(f"{name}: the library rsqrt(4) is not 0.5: y and dx are "
                  f"compared at half a bf16 ulp / 4*2^-24 relative")
    f = bc.formulas64(case, d, mean.double(), invstd.double())

    def close(got, ref64):
        bound = rel32 * ref64.abs() + (bc.half_ulp_bf16(ref64) if bf else 0)
        return bool(((_f64(got) - ref64).abs() <= bound).all())

    # ---- y and the mask: every element
    if exact:
        assert _mismatches(r["y"], f["y"]) == 0, "y not exact"
    else:
        assert close(r["y"], f["y"])
    assert ("mask" in r) == bc.writes_mask(case)
    if "mask" in r:
        assert r["mask"].numel() == N * C * H * W // 8
        wrong = int((bc.unpack_mask(r["mask"], case) != f["gate"]).sum())
        assert wrong == 0, f"{wrong} mask bits differ from the gate of v"

    # ---- backward, from every gate source
    gates = bc.dyadic_gates(case)
    for gate in gates:
        dg, db = _f64(r[f"dgamma@{gate}"]), _f64(r[f"dbeta@{gate}"])
        assert torch.equal(db, f["dbeta"]), f"dbeta@{gate} not exact"
        if exact:
            assert torch.equal(dg, f["dgamma"]), f"dgamma@{gate} not exact"
        else:
            assert ((dg - f["dgamma"]).abs()
                    <= 2.0 ** -22 * f["dgamma"].abs()).all()
        if case.res:
            assert _mismatches(r[f"dres@{gate}"], f["dres"]) == 0, \
                f"dres@{gate} is not dy * gate"
        dx = r[f"dx@{gate}"]
        if not exact:
            assert close(dx, f["dx"])
        elif _is_pow2(R) or not case.training:
            # k2 and k3 are dyadic (or 0): one rounding, to the dtype
            assert _mismatches(dx, f["dx"]) == 0, f"dx@{gate} not exact"
        else:
            # float32(k2), float32(k3) and the two subtractions round
            def ch(t):
                return t.abs().view(1, C, 1, 1)
            bound = rel32 * ch(f["k1"]) * (f["g"].abs() + ch(f["k2"])
                                           + ch(f["k3"]))
            if bf:
                bound = bound + bc.half_ulp_bf16(f["dx"])
            err = (_f64(dx) - f["dx"]).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"{name}@{gate}: max dx error = {worst:.3f} of the bound")
            assert (err <= bound).all(), f"dx@{gate} beyond the bound"

    # ---- the mask against y, relu and relu6: v is never within rounding
    # of 6 on these data
    if len(gates) == 2:
        for k in ("dx", "dgamma", "dbeta") + (("dres",) if case.res else ()):
            assert torch.equal(r[f"{k}@mask"], r[f"{k}@y"]), \
                f"{name}: {k} differs between the mask and y"


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


# ------------------------------------------------------------ large means
# The variance is the one-pass E[x^2] - mean^2, whose error grows with
# (mean/std)^2, and the 8-wide bf16 reduce holds fp32 partials. Yardstick:
# the library's batch norm on the same tensor. The factor 3 on invstd is the
# allowance for another summation order (test_line_model_level); the floor
# is a sixteenth of bf16's half-ulp, 2^-12, below anything a bf16 y can
# show (2^-20 for fp32).
RATIOS = (0, 4, 16, 64)          # mean / std per channel; 64 is reported only
OFFSET = [((8, 64, 16, 16), bc.BF, True, "nhwc_vec", 2.0 ** -12),
          ((4, 1024, 8, 8), bc.BF, True, "nhwc_scalar", 2.0 ** -12),
          ((8, 32, 14, 14), bc.FP, False, "nchw", 2.0 ** -20)]


@pytest.mark.parametrize("shape,dtype,nhwc,reduce,floor", OFFSET,
                         ids=[o[3] for o in OFFSET])
def test_offset_mean_against_library(ext, shape, dtype, nhwc, reduce, floor):
    N, C, H, W = shape
    assert ext.bn_plan(N, C, H * W, nhwc, 2 if dtype is bc.BF else 4, 0,
                       True, False)["reduce"] == reduce
    g = torch.Generator().manual_seed(6300)
    ratio = torch.tensor([RATIOS[c % len(RATIOS)] for c in range(C)])
    x = (ratio.view(1, C, 1, 1) + torch.randn(shape, generator=g)).to(dtype)
    xd = bc._layout(x, nhwc).to(_dev())
    gamma, beta = torch.ones(C, device=_dev()), torch.zeros(C, device=_dev())
    y, _, invstd = ext.bn_act_fwd(xd, None, gamma, beta, None, None, True,
                                  bc.MOM, bc.EPS, 0, nhwc)[:3]
    lib_y, _, lib_invstd = torch.native_batch_norm(
        xd, gamma, beta, None, None, True, bc.MOM, bc.EPS)

    x64 = x.double()
    mean = x64.mean(dim=(0, 2, 3))
    ref_is = torch.rsqrt(x64.var(dim=(0, 2, 3), unbiased=False) + bc.EPS)
    ref_y = (x64 - mean.view(1, C, 1, 1)) * ref_is.view(1, C, 1, 1)

    def errors(got_is, got_y, sel):
        e_is = ((got_is.cpu().double() - ref_is).abs() / ref_is)[sel].max()
        e_y = (_f64(got_y) - ref_y).abs()[:, sel].max()
        return e_is.item(), e_y.item()

    failures = []
    for rt in RATIOS:
        sel = ratio == rt
        (n_is, n_y), (l_is, l_y) = errors(invstd, y, sel), \
            errors(lib_invstd, lib_y, sel)
        print(f"{'x'.join(map(str, shape))} {bc.dtype_name(dtype)} {reduce} "
              f"mean/std={rt:2d}: invstd rel err native {n_is:.2e} library "
              f"{l_is:.2e}; y abs err native {n_y:.2e} library {l_y:.2e}")
        if rt <= 16:
            if n_is > max(3 * l_is, floor):
                failures.append(f"invstd at mean/std = {rt}")
            if n_y > 2 * l_y:
                failures.append(f"y at mean/std = {rt}")
    assert not failures, failures


# --------------------------------------------------------- bad arguments
@pytest.fixture(scope="module")
def fwd_args(ext):
    """A small well-formed forward with a residual; the guard tests swap
    one argument each. The guards run before any launch."""
    case = bc.CASE_BY_NAME["c24_relu_res"]
    d = bc.case_inputs(case.name)
    dev = _dev()
    good = {k: d[k].to(dev) for k in ("x", "res", "gamma", "beta", "rm",
                                      "rv")}

    def fwd(**swap):
        a = dict(good, **swap)
        return ext.bn_act_fwd(a["x"], a["res"], a["gamma"], a["beta"],
                              a["rm"], a["rv"], True, bc.MOM, bc.EPS, 1,
                              True)
    fwd()                           # the well-formed call passes
    return fwd, good


def test_fwd_rejects_res_of_another_size(fwd_args):
    fwd, good = fwd_args
    bad = torch.zeros(3, 24, 5, 8, device=_dev(), dtype=torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="res and x differ in size"):
        fwd(res=bad)


def test_fwd_rejects_res_of_another_dtype(fwd_args):
    fwd, good = fwd_args
    with pytest.raises(RuntimeError, match="res and x differ in dtype"):
        fwd(res=good["res"].float())


def test_fwd_rejects_res_on_another_device(fwd_args):
    fwd, good = fwd_args
    with pytest.raises(RuntimeError, match="res and x differ in device"):
        fwd(res=good["res"].cpu())


def test_fwd_rejects_res_of_another_layout(fwd_args):
    fwd, good = fwd_args
    bad = good["res"].contiguous()  # NCHW strides for an NHWC x
    assert not bad.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="res layout"):
        fwd(res=bad)


def test_fwd_rejects_x_of_another_dtype(fwd_args):
    fwd, good = fwd_args
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        fwd(x=good["x"].half(), res=good["res"].half())


_BAD_VEC = {
    "dtype": lambda t: t.double(),
    "length": lambda t: t[:-1].contiguous(),
    "stride": lambda t: torch.stack([t, t], dim=1)[:, 0],
    "device": lambda t: t.cpu(),
}


@pytest.mark.parametrize("kind", sorted(_BAD_VEC))
@pytest.mark.parametrize("arg,word", [("gamma", "gamma"), ("beta", "beta"),
                                      ("rm", "running_mean"),
                                      ("rv", "running_var")])
def test_fwd_rejects_a_bad_channel_vector(fwd_args, arg, word, kind):
    fwd, good = fwd_args
    bad = _BAD_VEC[kind](good[arg])
    with pytest.raises(RuntimeError, match=word + " must be a contiguous"):
        fwd(**{arg: bad})


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

    def bwd(dy=dy, y=y, mask=None, mean=mean, invstd=invstd, gamma=gamma):
        return ext.bn_act_bwd(dy, y, x, mean, invstd, gamma, 1, True, False,
                              True, mask)
    bwd(mask=mask, y=None)          # the well-formed calls pass
    bwd()
    bwd.good = {"y": y, "mean": mean, "invstd": invstd, "gamma": gamma}
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


def test_bwd_rejects_y_of_another_size(fwd8):
    bwd, dy, mask = fwd8
    bad = torch.zeros(2, 8, 4, 5, device=dy.device, dtype=dy.dtype) \
        .contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="y and x differ in size"):
        bwd(y=bad)


def test_bwd_rejects_y_of_another_dtype(fwd8):
    bwd, dy, mask = fwd8
    with pytest.raises(RuntimeError, match="y and x differ in dtype"):
        bwd(y=bwd.good["y"].float())


def test_bwd_rejects_y_of_another_layout(fwd8):
    bwd, dy, mask = fwd8
    bad = bwd.good["y"].contiguous()
    assert not bad.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="y layout"):
        bwd(y=bad)


@pytest.mark.parametrize("kind", ["dtype", "length"])
@pytest.mark.parametrize("arg", ["mean", "invstd", "gamma"])
def test_bwd_rejects_a_bad_channel_vector(fwd8, arg, kind):
    bwd, dy, mask = fwd8
    bad = _BAD_VEC[kind](bwd.good[arg])
    with pytest.raises(RuntimeError, match=arg + " must be a contiguous"):
        bwd(**{arg: bad})


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
