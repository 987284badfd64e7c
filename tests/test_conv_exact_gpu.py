"""Exact-arithmetic tests of the MFMA conv triple (csrc/conv_mfma2.hip,
conv_mfma.hip, conv_wgrad.hip) on every dispatch path.

Lattice inputs (conv_cases.py: small integers times powers of two, as
bf16) make the fp32 accumulation exact in any order, so forward, data-grad
and weight-grad are compared with ``==`` against a float64 CPU reference
— no tolerance that a dropped, duplicated or mis-addressed product could
hide under. Each case asserts through the launchers' own plan functions
that it reaches the kernel variant it was chosen for, and the last test
asserts the table as a whole reaches every variant in
conv_cases.REQUIRED. Forward and data-grad run under both conv structures
(DDLB_CONV_V2=1 and 0).

Also here: the autograd bridge on lattice data and the shape guards of
the conv_igemm bindings."""

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
_BF16 = torch.bfloat16

_IGEMM_CASES = [c.name for c in cc.CASES if "fwd" in c.passes]
_WGRAD_CASES = [c.name for c in cc.CASES if "wgrad" in c.passes]


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _gpu(t):
    return t.to(_dev()).contiguous(memory_format=_CL)


def _assert_claims(case):
    missing = set(case.claims) - cc.reached(_ext(), case)
    assert not missing, f"{case.name} no longer reaches {sorted(missing)}"


def test_premise_mfma_integer_accumulation_is_exact():
    """The premise everything below rests on, at the smallest case (one
    K-step, one tile, unscaled): MFMA accumulation of small-integer bf16
    data is exact. Measured on the MI355X: it is (0 mismatches)."""
    case = cc.CASES[0]
    N, C, H, W, K, R, stride, pad = case.shape
    d = cc.case_data(case.name)
    ext = _ext()
    y = ext.conv_igemm_fwd(_gpu(d["x"]), _gpu(d["w"]), stride, pad)
    w_perm = d["w"].to(_dev()).permute(1, 2, 3, 0).contiguous()
    dx = ext.conv_igemm_dgrad(_gpu(d["dy"]), w_perm, N, C, H, W, stride, pad)
    dw = ext.conv_igemm_wgrad(_gpu(d["x"]), _gpu(d["dy"]), R, R, stride, pad)
    bad = (cc.exact_mismatches(y, d["y"], _BF16),
           cc.exact_mismatches(dx, d["dx"], _BF16),
           cc.exact_mismatches(
               dw.view(K, R, R, C).permute(0, 3, 1, 2), d["dw"],
               torch.float32))
    print(f"premise {case.shape}: mismatches fwd/dgrad/wgrad = {bad}")
    assert bad == (0, 0, 0)


@pytest.mark.parametrize("v2", ["1", "0"])
@pytest.mark.parametrize("name", _IGEMM_CASES)
def test_fwd_dgrad_exact(name, v2, monkeypatch):
    case = cc.CASE_BY_NAME[name]
    _assert_claims(case)
    N, C, H, W, K, R, stride, pad = case.shape
    d = cc.case_data(name)
    ext = _ext()
    monkeypatch.setenv("DDLB_CONV_V2", v2)
    y = ext.conv_igemm_fwd(_gpu(d["x"]), _gpu(d["w"]), stride, pad)
    assert y.is_contiguous(memory_format=_CL)
    bad = cc.exact_mismatches(y, d["y"], _BF16)
    print(f"fwd {name} v2={v2}: {bad} of {y.numel()} differ")
    assert bad == 0
    # (K,C,R,S) logical -> (C,R,S,K) memory, as the autograd bridge does
    w_perm = d["w"].to(_dev()).permute(1, 2, 3, 0).contiguous()
    dx = ext.conv_igemm_dgrad(_gpu(d["dy"]), w_perm, N, C, H, W, stride, pad)
    assert dx.is_contiguous(memory_format=_CL)
    bad = cc.exact_mismatches(dx, d["dx"], _BF16)
    print(f"dgrad {name} v2={v2}: {bad} of {dx.numel()} differ")
    assert bad == 0


@pytest.mark.parametrize("name", _WGRAD_CASES)
def test_wgrad_exact(name):
    case = cc.CASE_BY_NAME[name]
    _assert_claims(case)
    N, C, H, W, K, R, stride, pad = case.shape
    d = cc.case_data(name)
    dw32 = _ext().conv_igemm_wgrad(_gpu(d["x"]), _gpu(d["dy"]), R, R, stride,
                                   pad)
    assert dw32.shape == (K, R * R * C)
    got = dw32.view(K, R, R, C).permute(0, 3, 1, 2)
    bad = cc.exact_mismatches(got, d["dw"], torch.float32)
    print(f"wgrad {name}: {cc.wgrad_plan(_ext(), case.shape)} "
          f"{bad} of {got.numel()} differ")
    assert bad == 0


@pytest.mark.parametrize("name", ["k136_c104_3x3", "s2_c80_3x3_p1"])
def test_autograd_bridge_exact(name):
    """conv2d_mfma + .backward with H != W: the w_perm permute and
    _dw_to_weight_layout carry exact values end to end; dw reaches the
    weight rounded once to bf16."""
    from ddlbench_amd.ops.conv import conv2d_mfma
    case = cc.CASE_BY_NAME[name]
    N, C, H, W, K, R, stride, pad = case.shape
    assert H != W
    d = cc.case_data(name)
    x = _gpu(d["x"]).requires_grad_(True)
    w = _gpu(d["w"]).requires_grad_(True)
    y = conv2d_mfma(x, w, stride, pad)
    y.backward(_gpu(d["dy"]))
    assert cc.exact_mismatches(y.detach(), d["y"], _BF16) == 0
    assert cc.exact_mismatches(x.grad, d["dx"], _BF16) == 0
    assert w.grad.shape == w.shape
    assert cc.exact_mismatches(w.grad, d["dw"], _BF16) == 0


def _raises(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)


def test_igemm_binding_guards():
    """Every mismatched call throws before any launch."""
    ext = _ext()
    dev = _dev()

    def t(*shape):
        return torch.zeros(*shape, device=dev, dtype=_BF16) \
            .contiguous(memory_format=_CL)

    x, w = t(2, 16, 9, 11), t(24, 16, 3, 3)        # stride 1, pad 1
    dy = t(2, 24, 9, 11)
    w_perm = torch.zeros(16, 3, 3, 24, device=dev, dtype=_BF16)
    fwd, dgrad, wgrad = (ext.conv_igemm_fwd, ext.conv_igemm_dgrad,
                         ext.conv_igemm_wgrad)
    # the consistent calls pass
    fwd(x, w, 1, 1)
    dgrad(dy, w_perm, 2, 16, 9, 11, 1, 1)
    wgrad(x, dy, 3, 3, 1, 1)
    torch.cuda.synchronize()

    # ---- forward
    _raises(fwd, x[0], w, 1, 1)                    # rank
    _raises(fwd, x, w[0], 1, 1)
    _raises(fwd, x, t(24, 8, 3, 3), 1, 1)          # w C != x C
    _raises(fwd, x, t(24, 32, 3, 3), 1, 1)
    _raises(fwd, x, w, 0, 1)                       # stride < 1
    _raises(fwd, x, w, 1, -1)                      # pad < 0
    _raises(fwd, t(2, 16, 2, 11), w, 1, 0)         # H + 2 pad < R
    _raises(fwd, t(2, 16, 9, 2), w, 1, 0)          # W + 2 pad < S
    # ---- data-grad
    _raises(dgrad, dy[0], w_perm, 2, 16, 9, 11, 1, 1)         # rank
    _raises(dgrad, dy, w_perm[0], 2, 16, 9, 11, 1, 1)
    _raises(dgrad, dy, w_perm, 3, 16, 9, 11, 1, 1)            # N
    _raises(dgrad, dy, w_perm, 2, 32, 9, 11, 1, 1)            # C
    _raises(dgrad, dy, torch.zeros(16, 3, 3, 32, device=dev, dtype=_BF16),
            2, 16, 9, 11, 1, 1)                               # K
    _raises(dgrad, dy, w_perm.float(), 2, 16, 9, 11, 1, 1)    # dtype
    _raises(dgrad, dy, w_perm, 2, 16, 11, 9, 1, 1)            # H/W swapped
    _raises(dgrad, dy, w_perm, 2, 16, 9, 11, 1, 0)            # OH vs pad
    _raises(dgrad, dy, w_perm, 2, 16, 9, 11, 2, 1)            # OH vs stride
    _raises(dgrad, dy, torch.zeros(16, 5, 5, 24, device=dev, dtype=_BF16),
            2, 16, 9, 11, 1, 1)                               # OH vs R
    _raises(dgrad, dy, w_perm, 2, 16, 9, 11, 0, 1)            # stride < 1
    _raises(dgrad, dy, w_perm, 2, 16, 9, 11, 1, -1)           # pad < 0
    _raises(dgrad, t(2, 24, 1, 1), w_perm, 2, 16, 2, 2, 1, 0)  # H+2pad < R
    # ---- weight-grad
    _raises(wgrad, x[0], dy, 3, 3, 1, 1)                      # rank
    _raises(wgrad, x, dy[0], 3, 3, 1, 1)
    _raises(wgrad, x, t(3, 24, 9, 11), 3, 3, 1, 1)            # N
    _raises(wgrad, x, t(2, 24, 11, 9), 3, 3, 1, 1)            # OH/OW swapped
    _raises(wgrad, x, dy, 3, 3, 1, 0)                         # OH vs pad
    _raises(wgrad, x, dy, 3, 3, 2, 1)                         # OH vs stride
    _raises(wgrad, x, dy, 5, 5, 1, 1)                         # OH vs R
    _raises(wgrad, x, dy, 3, 3, 0, 1)                         # stride < 1
    _raises(wgrad, x, dy, 3, 3, 1, -1)                        # pad < 0
    _raises(wgrad, t(2, 16, 2, 2), t(2, 24, 1, 1), 3, 3, 1, 0)  # H+2pad < R
    # nothing above left an error behind, and the device still works
    torch.cuda.synchronize()
    fwd(x, w, 1, 1)
    torch.cuda.synchronize()


def test_case_table_reaches_every_variant():
    """The union of all cases' plans covers conv_cases.REQUIRED."""
    union = cc.check_claims(_ext())
    unreached = sorted(set(cc.REQUIRED) - union)
    assert not unreached, f"no case reaches {unreached}"
