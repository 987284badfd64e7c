"""Exact and edge-shape tests of the first-generation kernels: NHWC
max-pool (csrc/maxpool.hip), depthwise 3x3 (csrc/depthwise_conv.hip), plain
cross-entropy (the ce_* kernels of csrc/cross_entropy.hip), the
multi-tensor SGD/Adam step (csrc/fused_sgd.hip, ops/sgd.py, ops/adam.py)
and the sequence utilities (csrc/seq_utils.hip).

Cases, data and float64 references come from op_cases.py; its docstring
maps every gap to a case, and test_op_cases_cpu.py proves the exact cases
representable. Max-pool, depthwise, SGD and the sequence copies compare with
``==``; cross-entropy and Adam carry the tolerances stated at their tests.

In the pointer-cache tests every tensor whose address an optimizer may have
cached stays referenced until the test ends, so a stale pointer lands in
live memory and shows as a wrong value."""

import pytest
import torch

import op_cases as oc

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
BF16, FP32 = oc.BF16, oc.FP32


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _cl(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


# ================================================================= max-pool
@pytest.mark.parametrize("name", [c.name for c in oc.POOL_CASES])
def test_maxpool_exact(name):
    """y and dx equal the float64 reference bit for bit: ties go to the
    first maximum in row-major order, a padding tap never wins, pixels no
    window covers get exactly zero."""
    from ddlbench_amd.ops.pool import maxpool2d_nhwc
    case = oc.POOL_BY_NAME[name]
    d = oc.pool_data(name)
    x = _cl(d["x"]).requires_grad_(True)
    y = maxpool2d_nhwc(x, *case.geom)
    y.backward(_cl(d["dy"]))
    bad_y = oc.exact_mismatches(y.detach(), d["y"], BF16)
    bad_dx = oc.exact_mismatches(x.grad, d["dx"], BF16)
    print(f"maxpool {name}: y {bad_y}/{y.numel()}, dx {bad_dx}/{x.numel()}")
    assert bad_y == 0 and bad_dx == 0
    unc = oc.pool_uncovered(case)
    assert (x.grad.cpu()[:, :, unc] == 0).all()


def _pool_windows(H, W, k, s, p):
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    for oh in range(OH):
        for ow in range(OW):
            inside = torch.zeros(H, W, dtype=torch.bool)
            inside[max(oh * s - p, 0):oh * s - p + k,
                   max(ow * s - p, 0):ow * s - p + k] = True
            yield oh, ow, inside


def _assert_dy_conserved(x, y, H, W, k, s, p):
    """Each window's dy, sent alone, arrives at exactly one in-bounds pixel
    of that window, per channel, unchanged."""
    C = x.shape[1]
    dyv = (torch.arange(C, dtype=torch.float32) % 4 + 1).view(1, C, 1, 1)
    for oh, ow, inside in _pool_windows(H, W, k, s, p):
        dy = torch.zeros(y.shape, dtype=torch.float32)
        dy[:, :, oh, ow] = dyv[:, :, 0, 0]
        (dx,) = torch.autograd.grad(y, x, _cl(dy.to(BF16)),
                                    retain_graph=True)
        dx = dx.float().cpu()
        hits = (dx != 0).sum(dim=(2, 3))
        print(f"  window ({oh},{ow}): pixels hit per channel "
              f"{sorted(set(hits.flatten().tolist()))}, outside window "
              f"{int((dx[:, :, ~inside] != 0).sum())}")
        assert (hits == 1).all(), (oh, ow)
        assert (dx[:, :, ~inside] == 0).all(), (oh, ow)
        assert torch.equal(dx.sum(dim=(2, 3)),
                           dyv[:, :, 0, 0].expand(x.shape[0], C)), (oh, ow)


_NONFINITE_GEOMS = [((4, 4), (3, 2, 1)), ((5, 5), (3, 3, 1)),
                    ((3, 4), (2, 2, 0))]


@pytest.mark.parametrize("hw,geom", _NONFINITE_GEOMS)
def test_maxpool_nan_tap_gives_nan(hw, geom):
    """A window with a NaN tap gives NaN in y; the other windows are
    untouched; every dy still reaches exactly one pixel of its window.
    Measured with the old ``best = -3.4e38f; if (f > best)``: 0 of the 19,
    17 and 9 NaN windows of the three geometries came out NaN."""
    from ddlbench_amd.ops.pool import maxpool2d_nhwc
    H, W = hw
    g = torch.Generator().manual_seed(77)
    xc = torch.randint(-3, 4, (2, 8, H, W), generator=g).to(BF16)
    # NaN as first tap, as last tap and in the middle of some window
    xc[0, :, 0, 0] = float("nan")
    xc[1, :, H - 1, W - 1] = float("nan")
    xc[1, 3, 1, 1] = float("nan")
    x = _cl(xc).requires_grad_(True)
    y = maxpool2d_nhwc(x, *geom)
    want = torch.nn.functional.max_pool2d(xc.double(), *geom)
    assert want.isnan().any() and not want.isnan().all()
    got = y.detach().cpu()
    print(f"maxpool NaN {hw} {geom}: NaN windows want "
          f"{int(want.isnan().sum())}, got {int(got.isnan().sum())}")
    assert oc.exact_mismatches(y.detach(), want, BF16) == 0
    _assert_dy_conserved(x, y, H, W, *geom)


@pytest.mark.parametrize("hw,geom", _NONFINITE_GEOMS)
def test_maxpool_neg_inf_window_gives_neg_inf(hw, geom):
    """An all -inf window gives -inf, not a finite number, and its dy
    still reaches one in-bounds pixel (slot 0 may be a padding position).
    Measured with the old ``barg = 0`` start: y was -inf (-3.4e38 rounds to
    -inf in bf16), but window (0,0) of the two padded geometries delivered
    its dy to no pixel at all."""
    from ddlbench_amd.ops.pool import maxpool2d_nhwc
    H, W = hw
    xc = torch.full((1, 8, H, W), float("-inf")).to(BF16)
    xc[0, 4:, H - 1, W - 1] = 1.0       # some channels keep a finite tap
    x = _cl(xc).requires_grad_(True)
    y = maxpool2d_nhwc(x, *geom)
    want = torch.nn.functional.max_pool2d(xc.double(), *geom)
    got = y.detach().cpu()
    print(f"maxpool -inf {hw} {geom}: y values "
          f"{sorted(set(got.float().flatten().tolist()))}")
    assert oc.exact_mismatches(y.detach(), want, BF16) == 0
    _assert_dy_conserved(x, y, H, W, *geom)


# ============================================================ depthwise 3x3
@pytest.mark.parametrize("name", [c.name for c in oc.DW_CASES])
def test_depthwise_exact(name):
    from ddlbench_amd.ops import functional as NF
    case = oc.DW_BY_NAME[name]
    d = oc.dw_data(name)
    dev = _dev()
    put = _cl if case.layout == "nhwc" else (lambda t: t.to(dev))
    x = put(d["x"]).requires_grad_(True)
    w = d["w"].to(dev).requires_grad_(True)
    y = NF.depthwise_conv3x3(x, w, case.stride, backend="native")
    if case.layout == "nhwc":
        assert y.is_contiguous(memory_format=_CL)
    y.backward(put(d["dy"]))
    bad = [oc.exact_mismatches(y.detach(), d["y"], case.dtype),
           oc.exact_mismatches(x.grad, d["dx"], case.dtype)]
    if oc.dw_via(case) == "grad":
        assert w.grad.shape == w.shape
        bad.append(oc.exact_mismatches(w.grad, d["dw"], case.dtype))
    else:
        nhwc = NF._is_nhwc(x) and case.dtype is BF16
        _, dw32 = _ext().dw3x3_bwd(
            x.detach(), w.detach().float().contiguous(), put(d["dy"]),
            case.stride, False, True, nhwc)
        bad.append(oc.exact_mismatches(dw32, d["dw"], FP32))
    print(f"depthwise {name}: mismatches y/dx/dw = {bad} "
          f"(dw via {oc.dw_via(case)})")
    assert bad == [0, 0, 0]


# ============================================================ cross-entropy
@pytest.mark.parametrize("name", [c.name for c in oc.CE_CASES])
def test_cross_entropy_edges(name):
    """Plain cross-entropy against float64 F.cross_entropy on the same
    (already rounded) logits.

    loss   rtol = atol = 1e-5, the fp32 tolerance of test_cross_entropy:
           the loss is an fp32 number for both logit dtypes.
    dx     bf16: rtol = 2^-7 (four half-ulps of the bf16 output) plus
           atol = 1e-6 * gscale. fp32: rtol = 1e-5 plus the same atol — the
           exponent (x - max) - log(sum) carries fp32 roundings of at most
           2^-23 of its own magnitude, 2e-6 relative in the probability
           while that magnitude is below 16 (beyond it the probability is
           under the atol), and a few ulps of the fast exponential.
    Rows of -inf logits take dx == 0 exactly, and nothing is NaN.

    Measured before the row maximum and the log-sum were stored apart: the
    row of equal logits at 3e4 had dx off by 5.6e-4 (K = 65) and 9.6e-4
    (K = 3) relative, the rounding of lse = 3e4 + log K at ulp(3e4)."""
    from ddlbench_amd.ops import functional as NF
    case = oc.CE_BY_NAME[name]
    d = oc.ce_data(name)
    dev = _dev()
    x = d["x"].to(dev).requires_grad_(True)
    loss = NF.cross_entropy(x, d["t"].to(dev), backend="native")
    (loss * oc.CE_GRAD_OUT).backward()
    gscale = oc.CE_GRAD_OUT / case.B
    got_loss = loss.detach().double().cpu()
    got_dx = x.grad.double().cpu()
    err = (got_dx - d["dx"]).abs()
    rel = (err / d["dx"].abs().clamp_min(1e-30))[err > 1e-6 * gscale]
    print(f"ce {name}: loss {got_loss.item():.9g} ref "
          f"{d['loss'].item():.9g} (abs err "
          f"{(got_loss - d['loss']).abs().item():.3g}); dx max abs err "
          f"{err.max().item():.3g}, max rel err beyond atol "
          f"{rel.max().item() if rel.numel() else 0.0:.3g}")
    assert x.grad.dtype == case.dtype
    assert not got_dx.isnan().any() and not got_loss.isnan()
    assert (got_dx[d["x"].double() == float("-inf")] == 0).all()
    torch.testing.assert_close(got_loss, d["loss"], rtol=1e-5, atol=1e-5)
    rtol = 2.0 ** -7 if case.dtype is BF16 else 1e-5
    torch.testing.assert_close(got_dx, d["dx"], rtol=rtol,
                               atol=1e-6 * gscale)


# ================================================================ fused SGD
def _params(ps):
    return [torch.nn.Parameter(p.to(_dev())) for p in ps]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.to(_dev())


def _run_sgd_exact(sizes, dtype, hyper, seed):
    from ddlbench_amd.ops.sgd import FusedSGD
    dtypes = oc.list_dtypes(sizes, dtype)
    ps, gs = oc.sgd_lattice(sizes, dtypes, seed)
    ref = oc.sgd_reference(ps, gs, **hyper)
    params = _params(ps)
    opt = FusedSGD(params, backend="native", **hyper)
    for k, (step, (want_p, want_m)) in enumerate(zip(gs, ref)):
        _set_grads(params, step)
        opt.step()
        bad_p = sum(oc.exact_mismatches(p.detach(), w.double(), dt)
                    for p, w, dt in zip(params, want_p, dtypes))
        bad_m = 0
        if hyper["momentum"]:
            bad_m = sum(oc.exact_mismatches(
                opt.state[p]["momentum_buffer"], m, FP32)
                for p, m in zip(params, want_m))
        else:
            assert all("momentum_buffer" not in opt.state[p]
                       for p in params)
        print(f"sgd step {k + 1}: mismatches p {bad_p}, momentum {bad_m}")
        assert bad_p == 0 and bad_m == 0, f"step {k + 1}"


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lname", sorted(oc.LISTS))
def test_fused_sgd_exact(lname, dtype):
    """Three lattice steps (the first with m = d, then two with momentum)
    equal float64 bit for bit, parameters and momentum buffers, for every
    tensor list: the prefix search, one-element tensors, and the capped
    grid's second trip with a tensor boundary inside it ("big")."""
    _run_sgd_exact(oc.LISTS[lname], dtype, oc.SGD_HYPER, 7)


@pytest.mark.parametrize("variant", ["momentum0", "wd0", "mixed"])
@pytest.mark.parametrize("lname", ["n5", "n37"])
def test_fused_sgd_variants_exact(lname, variant):
    """momentum = 0 (null momentum pointers), weight_decay = 0, and bf16
    and fp32 parameters mixed in one group (two launches, one per dtype)."""
    hyper = dict(oc.SGD_HYPER)
    dtype = BF16
    if variant == "momentum0":
        hyper["momentum"] = 0.0
    elif variant == "wd0":
        hyper["weight_decay"] = 0.0
    else:
        dtype = "mixed"
    _run_sgd_exact(oc.LISTS[lname], dtype, hyper, 17)


# =============================================================== fused Adam
_ADAM = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)


def _adam_tol(dtype):
    """fp32: the tolerance of test_fused_adam_native_matches_cpu_reference.
    bf16: the float64 reference is rounded to bf16 once per step as the
    kernel's store is; an fp32-vs-float64 difference can move that rounding
    by one bf16 ulp, at most 2^-7 relative to the step's result."""
    return dict(rtol=1e-4, atol=1e-5) if dtype is FP32 \
        else dict(rtol=2.0 ** -7, atol=1e-5)


@pytest.mark.parametrize("wd,decoupled", [(1e-2, False), (1e-2, True),
                                          (0.0, False)],
                         ids=["adam", "adamw", "wd0"])
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lname", sorted(oc.LISTS))
def test_fused_adam_lists(lname, dtype, wd, decoupled):
    from ddlbench_amd.ops.adam import FusedAdam
    sizes = oc.LISTS[lname]
    dtypes = oc.list_dtypes(sizes, dtype)
    ps, gs = oc.adam_data(sizes, dtypes, 23)
    ref = oc.AdamRef(ps, weight_decay=wd, decoupled_wd=decoupled, **_ADAM)
    params = _params(ps)
    opt = FusedAdam(params, weight_decay=wd, decoupled_wd=decoupled,
                    backend="native", **_ADAM)
    for step in gs:
        # each step on its own, from the parameters the kernel holds: a
        # one-ulp bf16 rounding difference of an earlier step is an
        # absolute error that a later, cancelling step would turn into a
        # large relative one (measured: 2 of 300 000 elements, 0.16
        # relative, when the reference ran its own trajectory)
        want = ref.step(step, [p.detach().cpu() for p in params])
        _set_grads(params, step)
        opt.step()
        for p, w in zip(params, want):
            torch.testing.assert_close(p.detach().double().cpu(),
                                       w.double(), **_adam_tol(dtype))


# ==================================================== pointer-cache tests
def _make_opt(kind, params):
    if kind == "sgd":
        from ddlbench_amd.ops.sgd import FusedSGD
        return FusedSGD(params, backend="native", **oc.SGD_HYPER)
    from ddlbench_amd.ops.adam import FusedAdam
    return FusedAdam(params, weight_decay=1e-2, backend="native", **_ADAM)


def _opt_reference(kind, ps, gs):
    """Parameters after every step, for the steps in ``gs``."""
    if kind == "sgd":
        return [p for p, _ in oc.sgd_reference(ps, gs, **oc.SGD_HYPER)]
    return oc.adam_reference(ps, gs, weight_decay=1e-2, decoupled_wd=False,
                             **_ADAM)


def _assert_params(kind, got, want):
    for p, w in zip(got, want):
        if kind == "sgd":
            assert oc.exact_mismatches(p.detach(), w.double(), FP32) == 0
        else:
            torch.testing.assert_close(p.detach().double().cpu(),
                                       w.double(), **_adam_tol(FP32))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_rebound_storage(kind):
    """p.data rebound after the first step (what model.to(memory_format=)
    or a weight-stashing wrapper does): the second update lands in the new
    storage, and the old storage keeps its bits."""
    sizes = [6, 1, 9]
    ps, gs = oc.sgd_lattice(sizes, [FP32] * 3, 31, steps=2)
    ref = _opt_reference(kind, ps, gs)
    params = _params(ps)
    opt = _make_opt(kind, params)
    _set_grads(params, gs[0])
    opt.step()
    _assert_params(kind, params, ref[0])
    old = params[1].data                 # stays referenced: live memory
    old_bits = old.clone()
    params[1].data = old.clone()
    _set_grads(params, gs[1])
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(old, old_bits), "the update went to the old storage"
    _assert_params(kind, params, ref[1])


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_changed_membership_same_count(kind):
    """After a step one parameter's grad becomes None and a parameter that
    had none gets one: the list has the same length and other members. Only
    the parameters with grads change, and they change correctly. (Adam's
    bias correction takes the step count of the list's first parameter; the
    reference does the same, the per-parameter count is a known gap.)"""
    sizes = [5, 4, 4]
    ps, gs = oc.sgd_lattice(sizes, [FP32] * 3, 37, steps=2)
    a, b, c = params = _params(ps)
    opt = _make_opt(kind, params)
    a.grad, b.grad = gs[0][0].to(_dev()), gs[0][1].to(_dev())
    opt.step()                           # members: a, b
    first = _opt_reference(kind, ps[:2], [gs[0][:2]])[0]
    _assert_params(kind, [a, b], first)
    assert torch.equal(c.detach().cpu(), ps[2])
    b_bits = b.detach().clone()
    b.grad = None
    c.grad = gs[1][2].to(_dev())
    a.grad = gs[1][0].to(_dev())
    opt.step()                           # members: a, c
    torch.cuda.synchronize()
    assert torch.equal(b.detach(), b_bits), "a grad-less parameter changed"
    want_a = _opt_reference(kind, ps[:1], [gs[0][:1], gs[1][:1]])[1]
    _assert_params(kind, [a], want_a)
    if kind == "sgd":       # c's first step: m = d
        want_c = _opt_reference(kind, ps[2:], [gs[1][2:]])[0]
    else:                   # zero moments, bias-corrected with t = 2
        b1, b2 = _ADAM["betas"]
        g64 = gs[1][2].double() + 1e-2 * ps[2].double()
        m, v = (1 - b1) * g64, (1 - b2) * g64 * g64
        upd = (m / (1 - b1 ** 2)) / ((v / (1 - b2 ** 2)).sqrt()
                                     + _ADAM["eps"])
        want_c = [(ps[2].double() - _ADAM["lr"] * upd).float()]
    _assert_params(kind, [c], want_c)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_grad_layout_copy(kind):
    """A channels_last parameter with a contiguous grad that is a view
    into a flat buffer (a data-parallel bucket): the step uses a
    layout-matched copy and leaves p.grad bound to the bucket."""
    g = torch.Generator().manual_seed(41)
    shape = (4, 6, 3, 3)
    p0 = (torch.randint(-3, 4, shape, generator=g) * 2).float()
    g0 = torch.randint(-3, 4, shape, generator=g).float()
    p = torch.nn.Parameter(_cl(p0))
    assert not p.is_contiguous()
    flat = torch.zeros(p0.numel() + 8, device=_dev())
    view = flat[8:].view(shape)
    view.copy_(g0.to(_dev()))
    p.grad = view
    opt = _make_opt(kind, [p])
    opt.step()
    torch.cuda.synchronize()
    assert p.grad.data_ptr() == flat.data_ptr() + 32
    assert p.grad.stride() == view.stride()
    assert torch.equal(view.cpu(), g0), "the bucket's grad changed"
    want = _opt_reference(kind, [p0], [[g0]])[0]
    _assert_params(kind, [p], want)
    assert p.is_contiguous(memory_format=_CL)


# ======================================================= sequence utilities
def _seq_input(case, dtype):
    g = torch.Generator().manual_seed(53)
    return torch.randint(1, 120, (case.T, case.B, case.F),
                         generator=g).to(dtype)      # never 0: padding is


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in oc.SEQ_CASES])
def test_revert_varlen_exact(name, dtype):
    case = oc.SEQ_BY_NAME[name]
    x = _seq_input(case, dtype)
    lengths = torch.tensor(case.lengths, device=_dev())
    out = _ext().revert_varlen(x.to(_dev()), lengths)
    assert out.dtype == dtype
    assert torch.equal(out.cpu(), oc.revert_reference(x, case.lengths))


@pytest.mark.parametrize("name", ["rv_small", "rv_f1"])
def test_revert_varlen_wrapper_non_contiguous(name):
    """models.gnmt.revert_varlen on a non-contiguous input (a slice of a
    wider tensor, and a transposed one), forward and backward."""
    from ddlbench_amd.models.gnmt import revert_varlen
    case = oc.SEQ_BY_NAME[name]
    x = _seq_input(case, FP32)
    lengths = torch.tensor(case.lengths, device=_dev())
    wide = torch.cat([x, x + 500], dim=2).to(_dev())
    sl = wide[:, :, :case.F].requires_grad_(True)
    tr = x.transpose(0, 1).contiguous().to(_dev()).transpose(0, 1)
    assert not sl.is_contiguous()
    assert case.B == 1 or case.T == 1 or not tr.is_contiguous()
    want = oc.revert_reference(x, case.lengths)
    out = revert_varlen(sl, lengths)
    assert torch.equal(out.detach().cpu(), want)
    assert torch.equal(revert_varlen(tr, lengths).cpu(), want)
    (dx,) = torch.autograd.grad(out, sl, wide[:, :, case.F:])
    assert torch.equal(dx.cpu(),
                       oc.revert_reference(x + 500, case.lengths))


@pytest.mark.parametrize("name", [c.name for c in oc.SEQ_CASES])
def test_varlen_mask_exact(name):
    case = oc.SEQ_BY_NAME[name]
    lengths = torch.tensor(case.lengths, device=_dev())
    for T in (case.T, max(case.lengths), 1):
        if T < max(case.lengths) or T < 1:
            continue
        m = _ext().varlen_mask(lengths, T)
        assert m.shape == (T, case.B) and m.dtype == torch.uint8
        assert torch.equal(m.bool().cpu(),
                           oc.mask_reference(case.lengths, T))
