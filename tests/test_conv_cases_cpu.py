"""The exact-arithmetic conv tests' own machinery, checked without a GPU:
the case table against the model zoo, the float64 reference against an
independent integer computation, the comparator's sensitivity to a single
wrong term, and the launchers' dispatch plans (pure host functions of the
built extension) against hand-computed rows."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_cases as cc


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


# ------------------------------------------------------------- zoo coverage
def test_case_table_covers_model_zoo_geometries():
    """(R, stride, pad) of every mfma_eligible conv over ARCHS x datasets
    occurs in the case table, with H != W for every non-1x1 class."""
    from ddlbench_amd.models import ARCHS, build_model
    from ddlbench_amd.ops.conv import mfma_eligible
    zoo = {}
    for dataset in ("imagenet", "cifar10", "mnist"):
        for arch in ARCHS:
            if arch == "inception3" and dataset != "imagenet":
                continue        # build_model rejects it (stem downsampling)
            with torch.device("meta"):
                model = build_model(dataset, arch)
            for m in model.modules():
                if isinstance(m, nn.Conv2d) and mfma_eligible(m):
                    zoo.setdefault((m.kernel_size[0], m.stride[0],
                                    m.padding[0]), f"{dataset}/{arch}")
    # the classes known today; a new one must get a case, not pass unseen
    assert {(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0),
            (3, 2, 0), (5, 1, 2)} <= set(zoo)
    igemm = [c for c in cc.CASES if "fwd" in c.passes]
    table = {cc.geometry(c.shape) for c in igemm}
    rect = {cc.geometry(c.shape) for c in igemm
            if c.shape[2] != c.shape[3]}
    for geom, where in zoo.items():
        assert geom in table, f"{geom} ({where}) has no exact-test case"
        if geom[0] > 1:
            assert geom in rect, f"{geom} ({where}) has no H != W case"
    assert rect, "the case table has no H != W entries"


def test_cases_are_well_formed():
    for case in cc.CASES:
        N, C, H, W, K, R, stride, pad = case.shape
        assert C % 8 == 0 and K % 8 == 0, case.name
        assert set(case.passes) <= set(cc.ALL) and case.passes
        assert set(case.claims) <= set(cc.REQUIRED), case.name
        cc.check_sum_guard(case)


def test_sum_guard_rejects_an_inexact_case():
    big = cc.Case("too_deep", (64, 8, 200, 200, 8, 1, 1, 0), cc.WG,
                  (0, 0, 0), ())       # P = 2 560 000: 9 P > 2^24
    with pytest.raises(AssertionError):
        cc.check_sum_guard(big)
    scaled = cc.Case("too_scaled", (1, 8, 4, 5, 8, 1, 1, 0), ("fwd",),
                     (12, 10, 0), ())   # 9 * 8 * 2^22 > 2^24
    with pytest.raises(AssertionError):
        cc.check_sum_guard(scaled)


# --------------------------------------- reference and comparator self-test
def _int_reference(x, w, dy, stride, pad):
    """y, dx, dw by unfold + int64 matmul — no conv, no floating point.
    Inputs are unscaled lattice tensors (exact small integers)."""
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    OH, OW = dy.shape[2:]
    xi, wi, dyi = (t.double().round().long() for t in (x, w, dy))
    cols = F.unfold(xi.double(), (R, S), padding=pad, stride=stride) \
        .long()                                      # (N, C*R*S, OH*OW)
    wm = wi.reshape(K, C * R * S)
    y = torch.einsum("kq,nqp->nkp", wm, cols).reshape(N, K, OH, OW)
    dym = dyi.reshape(N, K, OH * OW)
    dw = torch.einsum("nkp,nqp->kq", dym, cols).reshape(K, C, R, S)
    dcols = torch.einsum("kq,nkp->nqp", wm, dym)     # (N, C*R*S, OH*OW)
    dx = F.fold(dcols.double(), (H, W), (R, S), padding=pad,
                stride=stride).round().long()
    return y, dx, dw


@pytest.mark.parametrize("shape", [
    (2, 8, 7, 10, 16, 3, 2, 1),     # stride 2, H != W, odd and even
    (2, 8, 6, 9, 8, 5, 1, 2),       # 5x5 pad 2
    (1, 16, 5, 4, 8, 3, 1, 0),      # pad 0
])
def test_float64_reference_equals_integer_matmul(shape):
    N, C, H, W, K, R, stride, pad = shape
    OH, OW = cc.out_hw(shape)
    g = torch.Generator().manual_seed(7)
    x = cc.lattice((N, C, H, W), g)
    w = cc.lattice((K, C, R, R), g)
    dy = cc.lattice((N, K, OH, OW), g)
    ref = cc.reference64(x, w, dy, stride, pad)
    y, dx, dw = _int_reference(x, w, dy, stride, pad)
    assert torch.equal(ref["y"], y.double())
    assert torch.equal(ref["dx"], dx.double())
    assert torch.equal(ref["dw"], dw.double())


def test_lattice_values():
    g = torch.Generator().manual_seed(3)
    t = cc.lattice((4, 8, 16, 16), g, exp=-2)
    assert t.dtype == torch.bfloat16
    v = t.double() * 4
    assert torch.equal(v, v.round()) and v.abs().max().item() == 3
    zeros = (v == 0).double().mean().item()
    assert abs(zeros - 1 / 7) < 0.02       # 8192 draws: sigma = 0.004


@pytest.mark.parametrize("flip", [1, -1])
def test_comparator_sees_a_single_wrong_term(flip):
    """One input element off by +-1 changes exactly the outputs that
    element feeds, and the exact comparator reports them — a kernel that
    drops, duplicates or mis-addresses one product cannot pass."""
    case = cc.CASE_BY_NAME["k136_c104_3x3"]
    N, C, H, W, K, R, stride, pad = case.shape
    d = cc.case_data(case.name)
    sx, sw, sdy = case.scale
    good = {"y": d["y"].to(torch.bfloat16), "dx": d["dx"].to(torch.bfloat16),
            "dw": d["dw"].float()}
    for k, dt in (("y", torch.bfloat16), ("dx", torch.bfloat16),
                  ("dw", torch.float32)):
        assert cc.exact_mismatches(good[k], d[k], dt) == 0

    # flip one weight element by one lattice step
    w = d["w"].clone()
    k0, c0 = 5, 17
    w[k0, c0, 1, 2] += flip * 2.0 ** sw
    bad = cc.reference64(d["x"], w, d["dy"], stride, pad, ("fwd", "dgrad"))
    # fp32 outputs would show every changed term ...
    assert (bad["y"] != d["y"]).sum().item() > 0
    assert (bad["y"] != d["y"])[:, k0].sum() == (bad["y"] != d["y"]).sum()
    # ... and so does the bf16 comparison, despite its one rounding
    n = cc.exact_mismatches(bad["y"].to(torch.bfloat16), d["y"],
                            torch.bfloat16)
    print(f"flip {flip}: {n} bf16 outputs differ")
    assert n > 0
    assert cc.exact_mismatches(bad["dx"].to(torch.bfloat16), d["dx"],
                               torch.bfloat16) > 0

    # one dy element off: exactly the dw entries it feeds change, and the
    # fp32 comparison reports every one of them
    dy = d["dy"].clone()
    dy[1, k0, 4, 6] += flip * 2.0 ** sdy
    bad = cc.reference64(d["x"], d["w"], dy, stride, pad, ("wgrad",))
    changed = (bad["dw"] != d["dw"])
    assert changed.sum().item() > 0 and changed[k0].sum() == changed.sum()
    assert cc.exact_mismatches(bad["dw"].float(), d["dw"],
                               torch.float32) == changed.sum().item()


# ------------------------------------------------------------ dispatch plans
def test_wgrad_plan_hand_computed_rows():
    """split = min(2048/(nk*nr), ceil(P/64), 256, cap/(K*RSC)) with the
    8M-float workspace; steps = ceil(ceil(P/split)/64)."""
    ext = _ext()

    def plan(N, C, H, W, K, R, s, p):
        return ext.conv_wgrad_plan(N, C, H, W, K, R, R, s, p)

    # P = 784, 64x128 tiles: nk=1, nr=ceil(576/128)=5 ->
    # min(409, 13, 256, 227) = 13; ceil(784/13) = 61 pixels, one step
    pl = plan(4, 64, 14, 14, 64, 3, 1, 1)
    assert (pl["TK"], pl["TR"], pl["ring"], pl["r1"]) == (64, 128, 3, False)
    assert (pl["split"], pl["steps"], pl["tail"], pl["psb"]) == (13, 1, 61, 1)
    # P = 4*8*8 = 256: nk=1, nr=5 -> min(409, 4, ...) = 4; 64 pixels each
    pl = plan(4, 64, 15, 15, 128, 3, 2, 1)
    assert (pl["TK"], pl["TR"], pl["ring"]) == (128, 128, 2)
    assert (pl["split"], pl["steps"], pl["tail"]) == (4, 1, 64)
    # P = 162, 1x1: r1, 64x64 tile, split = ceil(162/64) = 3, 54 pixels
    pl = plan(2, 32, 9, 9, 24, 1, 1, 0)
    assert (pl["TK"], pl["TR"], pl["r1"]) == (64, 64, True)
    assert (pl["split"], pl["steps"], pl["tail"], pl["psb"]) == (3, 1, 54, 1)
    # P = 507: nk=1, nr=ceil(864/128)=7 -> min(292, 8, ...) = 8
    pl = plan(3, 96, 13, 13, 104, 3, 1, 1)
    assert (pl["split"], pl["steps"]) == (8, 1)
    # P = 162, K=512, C=128: nk=4, nr=1 -> min(512, 3, ...) = 3
    pl = plan(2, 128, 9, 9, 512, 1, 1, 0)
    assert (pl["TK"], pl["TR"], pl["ring"], pl["r1"]) == (128, 128, 2, True)
    assert (pl["split"], pl["steps"]) == (3, 1)
    # steady state: P = 57600, K*RSC = 36864 -> workspace cap 227;
    # ceil(57600/227) = 254 = 3*64 + 62; 227 slabs -> 4 combine rows
    pl = plan(4, 64, 120, 120, 64, 3, 1, 1)
    assert (pl["split"], pl["steps"], pl["tail"], pl["psb"]) == (227, 4, 62, 4)
    # K*RSC = 1M -> cap 8; ceil(2178/8) = 273 = 4*64 + 17
    pl = plan(2, 512, 33, 33, 2048, 1, 1, 0)
    assert (pl["split"], pl["steps"], pl["tail"], pl["psb"]) == (8, 5, 17, 1)
    # K*RSC = 4.7M floats > half the workspace: no split, no combine
    pl = plan(7, 512, 5, 6, 1024, 3, 1, 1)
    assert (pl["split"], pl["steps"], pl["tail"], pl["psb"]) == (1, 4, 18, 0)


def test_igemm_plan_hand_computed_rows(monkeypatch):
    ext = _ext()
    monkeypatch.setenv("DDLB_CONV_V2", "1")

    def keys(e, *names):
        return tuple(e[n] for n in names)

    # fwd 3x3, K = 104 >= 96: v2 128x128 gather; M = 3*13*13, Kd = 9*96
    (e,) = ext.conv_igemm_plan(3, 96, 13, 13, 104, 3, 3, 1, 1, False)
    assert keys(e, "structure", "mode", "BM", "BN", "LIN", "M", "Nd",
                "Kd") == ("v2", 0, 128, 128, False, 507, 104, 864)
    # fwd 1x1 stride 1: LIN; K = 64 in [48, 96): 256x64
    (e,) = ext.conv_igemm_plan(2, 96, 16, 16, 64, 1, 1, 1, 0, False)
    assert keys(e, "structure", "BM", "BN", "LIN") == ("v2", 256, 64, True)
    # Nd = 24 < 48: v2 declines; M = 2*5*5 = 50 < 256 -> 128x64
    (e,) = ext.conv_igemm_plan(2, 16, 9, 9, 24, 3, 3, 2, 1, False)
    assert keys(e, "structure", "BM", "BN", "M") == ("v1", 128, 64, 50)
    # stride-2 3x3 pad-1 dgrad on 9x9: four parity classes. Class (a,b)
    # has ceil((9-a)/2) x ceil((9-b)/2) pixels per image and taps
    # r = r0, r0+2 < 3 with r0 = (a+1)&1: two for a odd, one for a even
    plan = ext.conv_igemm_plan(2, 256, 9, 9, 96, 3, 3, 2, 1, True)
    assert [keys(e, "cls", "taps", "M", "Kd") for e in plan] == [
        ((0, 0), (1, 1), 50, 96), ((0, 1), (1, 2), 40, 192),
        ((1, 0), (2, 1), 40, 192), ((1, 1), (2, 2), 32, 384)]
    assert all(keys(e, "structure", "mode", "BM", "BN", "Nd")
               == ("v2", 2, 128, 128, 256) for e in plan)
    # stride-2 1x1: only the (even, even) class has a tap
    plan = ext.conv_igemm_plan(4, 64, 14, 14, 128, 1, 1, 2, 0, True)
    assert [keys(e, "cls", "taps", "M") for e in plan] == [
        ((0, 0), (1, 1), 4 * 7 * 7)]
    # stride 3: plain gather dgrad, never v2
    (e,) = ext.conv_igemm_plan(2, 72, 10, 10, 16, 3, 3, 3, 1, True)
    assert keys(e, "structure", "mode", "BM", "BN") == ("v1", 1, 128, 128)
    # DDLB_CONV_V2=0 forces the 128-tile structure, read per call
    monkeypatch.setenv("DDLB_CONV_V2", "0")
    (e,) = ext.conv_igemm_plan(3, 96, 13, 13, 104, 3, 3, 1, 1, False)
    assert keys(e, "structure", "BM", "BN", "LIN") == ("v1", 128, 128, False)
    (e,) = ext.conv_igemm_plan(4, 64, 14, 14, 64, 3, 3, 1, 1, False)
    assert keys(e, "structure", "BM", "BN", "M") == ("v1", 256, 64, 784)


def test_plan_functions_reject_bad_geometry():
    ext = _ext()
    with pytest.raises(RuntimeError):
        ext.conv_wgrad_plan(2, 8, 9, 9, 8, 3, 3, 0, 1)       # stride 0
    with pytest.raises(RuntimeError):
        ext.conv_igemm_plan(2, 8, 2, 9, 8, 3, 3, 1, 0, False)  # H < R


def test_case_table_reaches_every_variant():
    """Each case reaches the paths it claims, and the union of all plans
    covers conv_cases.REQUIRED (the plans need no device)."""
    union = cc.check_claims(_ext())
    unreached = sorted(set(cc.REQUIRED) - union)
    assert not unreached, f"no case reaches {unreached}"
