"""The conv backward's native tail: weight-grad written straight to the
weight's dtype and layout (ext.conv_igemm_wgrad_bf16) and the dgrad weight
layout as one tiled transpose (ext.conv_weight_dgrad_layout), against the
eager-tensor tail they replace.

The reference of the weight-grad is the parent path itself,
``_dw_to_weight_layout(conv_igemm_wgrad(...))``: where that path is
deterministic (psb <= 1: no combine, or a single-row combine) the new
result must be torch.equal for any input; where it accumulates with
atomics (psb > 1) torch.equal is required for integer inputs (every sum
exact in any order), and for random inputs the new path must repeat bit
for bit and stay within one bf16 ulp of the parent's result (both are one
rounding of fp32 sums that differ by reordering only).

The one-ulp comparison draws x and dy from [0.5, 1.5): every term is
positive, so two summation orders differ by a few 2^-24 of the result,
far below its bf16 ulp of 2^-8, and one ulp (a rounding boundary crossed)
is the most reordering can cause. Zero-mean inputs give no such bound: an
element whose terms cancel to ~1e-3 while its 64-slab chunk sums are
~1e2 moves by several bf16 ulps of itself whenever the parent's atomics
land in another order (measured once: a largest distance of 4 ulps over
the 9216 elements of wg_128x64_gather with randn inputs, 1 or less on
the other psb > 1 shapes) — that is the parent's own run-to-run noise,
not a property of the new path. randn inputs therefore check what is order-free: torch.equal where
the parent is deterministic, bit-identical repeats where it is not."""

import pytest
import torch

from conv_cases import CASE_BY_NAME, out_hw

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# shape = (N, C, H, W, K, R, stride, pad), from tests/conv_cases.py where
# one exists; the comment is what ext.conv_wgrad_plan must say (asserted in
# test_cases_reach_every_branch)
SHAPES = {
    "tiny_1x1": CASE_BY_NAME["tiny_1x1"].shape,          # split 1, 64/64 r1
    "s2_c64_1x1": CASE_BY_NAME["s2_c64_1x1"].shape,      # split 1, 128/64
    "wg_split1_multistep":                               # split 1, 128/128
        CASE_BY_NAME["wg_split1_multistep"].shape,
    "c40_3x3_p1": CASE_BY_NAME["c40_3x3_p1"].shape,      # split 4, 64/128
    "k96_c64_1x1": CASE_BY_NAME["k96_c64_1x1"].shape,    # split 8, 64/64 r1
    "wg_64x64_gather": CASE_BY_NAME["wg_64x64_gather"].shape,   # split 256
    "wg_64x128_r1": CASE_BY_NAME["wg_64x128_r1"].shape,
    "wg_128x64_gather": CASE_BY_NAME["wg_128x64_gather"].shape,
    "wg_128x128_r1": CASE_BY_NAME["wg_128x128_r1"].shape,
    "c64_k64_hw56": (8, 64, 56, 56, 64, 1, 1, 0),        # split 256, psb 4
    # 6384 pixels = 100 steps: 64 < split < 256, a ragged last slab chunk
    "c64_k64_split100": (2, 64, 56, 57, 64, 1, 1, 0),
}


@pytest.fixture(scope="module")
def ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"
    return ops.require_extension()


def _dev():
    return torch.device("cuda", 0)


def _plan(ext, shape):
    N, C, H, W, K, R, stride, pad = shape
    return ext.conv_wgrad_plan(N, C, H, W, K, R, R, stride, pad)


def _inputs(shape, kind, seed):
    N, C, H, W, K, R, stride, pad = shape
    OH, OW = out_hw(shape)
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        x = torch.randint(-1, 2, (N, C, H, W), generator=g).float()
        dy = torch.randint(-1, 2, (N, K, OH, OW), generator=g).float()
    elif kind == "positive":
        x = torch.rand((N, C, H, W), generator=g) + 0.5
        dy = torch.rand((N, K, OH, OW), generator=g) + 0.5
    else:
        x = torch.randn((N, C, H, W), generator=g)
        dy = torch.randn((N, K, OH, OW), generator=g)
    to = dict(device=_dev(), dtype=torch.bfloat16)
    return (x.to(**to).contiguous(memory_format=CL),
            dy.to(**to).contiguous(memory_format=CL))


def _both(ext, shape, x, dy):
    from ddlbench_amd.ops.conv import _dw_to_weight_layout
    N, C, H, W, K, R, stride, pad = shape
    weight = torch.empty(K, C, R, R, device=_dev(), dtype=torch.bfloat16)
    old = _dw_to_weight_layout(
        ext.conv_igemm_wgrad(x, dy, R, R, stride, pad), weight)
    new = ext.conv_igemm_wgrad_bf16(x, dy, R, R, stride, pad)
    return old, new


def _ordered_bits(t):
    """bf16 -> integers in value order (adjacent values differ by 1)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def test_cases_reach_every_branch(ext):
    plans = {n: _plan(ext, s) for n, s in SHAPES.items()}
    assert any(p["split"] == 1 for p in plans.values())
    assert any(1 < p["split"] <= 64 for p in plans.values())
    assert any(64 < p["split"] < 256 for p in plans.values())
    assert plans["c64_k64_hw56"]["split"] > 64
    assert plans["c64_k64_hw56"]["psb"] > 1
    tiles = {(p["TK"], p["TR"]) for p in plans.values()}
    assert tiles == {(64, 64), (64, 128), (128, 64), (128, 128)}
    # each combine kind (none / one row / several rows) with and without r1
    kinds = {(min(p["psb"], 2), p["r1"]) for p in plans.values()}
    assert kinds == {(b, r) for b in (0, 1, 2) for r in (False, True)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_wgrad_bf16_matches_parent_path(ext, name):
    shape = SHAPES[name]
    N, C, H, W, K, R, stride, pad = shape
    psb = _plan(ext, shape)["psb"]

    x, dy = _inputs(shape, "int", 11)
    old, new = _both(ext, shape, x, dy)
    assert new.dtype == torch.bfloat16 and old.dtype == torch.bfloat16
    assert tuple(new.shape) == (K, C, R, R)
    assert new.stride() == old.stride() == (R * R * C, 1, R * C, C)
    assert new.is_contiguous(memory_format=CL)
    assert torch.equal(new, old), "integer inputs: sums are exact"

    x, dy = _inputs(shape, "randn", 12)
    old, new = _both(ext, shape, x, dy)
    if psb <= 1:
        assert torch.equal(new, old)
    else:
        again = ext.conv_igemm_wgrad_bf16(x, dy, R, R, stride, pad)
        assert torch.equal(new, again), "ordered combine must repeat"
        x, dy = _inputs(shape, "positive", 13)
        old, new = _both(ext, shape, x, dy)
        again = ext.conv_igemm_wgrad_bf16(x, dy, R, R, stride, pad)
        assert torch.equal(new, again), "ordered combine must repeat"
        step = (_ordered_bits(new) - _ordered_bits(old)).abs().max().item()
        print(f"{name}: max {step} bf16 steps from the parent path")
        assert step <= 1, f"{step} bf16 steps from the parent path"


# ------------------------------------------------- dgrad weight layout
@pytest.mark.parametrize("K,C,R", [(64, 64, 1), (256, 64, 1), (64, 256, 1),
                                   (128, 128, 3), (8, 8, 3), (24, 40, 3),
                                   (512, 2048, 1)])
@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
def test_weight_dgrad_layout_is_a_pure_copy(ext, K, C, R, layout):
    g = torch.Generator().manual_seed(K * 7 + C * 3 + R)
    w = torch.randn(K, C, R, R, generator=g).to(_dev(), torch.bfloat16)
    if layout == "channels_last":
        w = w.contiguous(memory_format=CL)
    got = ext.conv_weight_dgrad_layout(w)
    want = w.permute(1, 2, 3, 0).contiguous()
    assert tuple(got.shape) == (C, R, R, K) and got.is_contiguous()
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, want)


def test_weight_dgrad_layout_rejects_other_inputs(ext):
    w = torch.randn(32, 32, 3, 3, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="channels_last or contiguous"):
        ext.conv_weight_dgrad_layout(w[:, ::2])
    with pytest.raises(RuntimeError, match="channels_last or contiguous"):
        ext.conv_weight_dgrad_layout(w.permute(1, 0, 2, 3))
    with pytest.raises(RuntimeError, match="bf16"):
        ext.conv_weight_dgrad_layout(w.float())
    with pytest.raises(RuntimeError, match="% 8"):
        ext.conv_weight_dgrad_layout(w[:12].contiguous())
    with pytest.raises(RuntimeError, match="4-D"):
        ext.conv_weight_dgrad_layout(w[0])


# --------------------------------------------------- module end to end
@pytest.mark.parametrize("K,C,R,stride,pad", [(24, 16, 3, 1, 1),
                                              (64, 32, 1, 1, 0),
                                              (32, 16, 3, 2, 1)])
def test_module_gradients_equal_eager_tail(ext, monkeypatch, K, C, R,
                                           stride, pad):
    from ddlbench_amd.ops import conv as convmod
    shape = (2, C, 10, 11, K, R, stride, pad)
    assert _plan(ext, shape)["psb"] <= 1  # the eager tail repeats too
    g = torch.Generator().manual_seed(5)
    ref = torch.nn.Conv2d(C, K, R, stride, pad, bias=False)
    ref = ref.to(_dev(), torch.bfloat16).to(memory_format=CL)
    x0 = torch.randn(2, C, 10, 11, generator=g).to(_dev(), torch.bfloat16) \
        .contiguous(memory_format=CL)
    dy = None
    grads = {}
    for tail in (True, False):
        monkeypatch.setattr(convmod, "NATIVE_TAIL", tail)
        m = convmod.Conv2dMFMA(ref)
        m.weight.grad = None
        x = x0.clone().requires_grad_(True)
        y = m(x)
        if dy is None:
            dy = torch.randn(y.shape, generator=g).to(_dev(), torch.bfloat16)
        y.backward(dy)
        grads[tail] = (x.grad.clone(), m.weight.grad.clone())
    assert torch.equal(grads[True][0], grads[False][0])
    assert torch.equal(grads[True][1], grads[False][1])
    assert grads[True][1].stride() == grads[False][1].stride()
