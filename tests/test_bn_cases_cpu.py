"""The dyadic data of tests/bn_cases.py is what test_dyadic_exact takes it
for: on every case, float64 arithmetic with the kernels' documented
formulas shows invstd == 0.5 after the cast to fp32, every x, v, y and
gated dy representable in the case's dtype, every partial sum below 2^24
in magnitude (so exact in fp32 in any order), and no v on a gate threshold.
These are conditions on the inputs: a shape that misses one needs other
values, not a looser test. No device and no extension needed."""

import pytest
import torch

import bn_cases as bc

NAMES = [c.name for c in bc.CASES]
LIMIT = float(1 << 24)


def _exact_in(t64, dtype):
    return torch.equal(t64.to(dtype).double(), t64)


@pytest.mark.parametrize("name", NAMES)
def test_dyadic_data_is_sound(name):
    case = bc.CASE_BY_NAME[name]
    d64, d = bc.dyadic64(name), bc.dyadic_inputs(name)
    N, C, H, W = case.shape
    R, P, m = d64["R"], d64["P"], d64["m"]
    assert R == N * H * W and P == R // 4

    # the construction: P rows at +2 and P at -2 in every channel
    dev = d64["x"] - m.view(1, C, 1, 1)
    assert ((dev == 2).sum(dim=(0, 2, 3)) == P).all()
    assert ((dev == -2).sum(dim=(0, 2, 3)) == P).all()
    assert ((dev == 0).sum(dim=(0, 2, 3)) == R - 2 * P).all()
    assert ((m >= -3) & (m <= 3) & (m == m.round())).all()
    assert (d64["gamma"] == -1).any()
    assert ((d64["beta"] * 4) % 2 == 1).all() and (d64["beta"].abs() < 3).all()
    assert ((d64["dy"].abs() <= 2) & (d64["dy"] == d64["dy"].round())).all()

    # the cast to the case's dtype and layout loses nothing
    for k in ("x", "dy", "res"):
        if d64[k] is None:
            assert d[k] is None
            continue
        assert _exact_in(d64[k], case.dtype), k
        assert d[k].dtype is case.dtype and bc._layout(d[k], case.nhwc) \
            .data_ptr() == d[k].data_ptr(), k
        assert torch.equal(d[k].double().contiguous(), d64[k]), k
    for k in ("gamma", "beta", "rm", "rv"):
        assert d[k].dtype is torch.float32
        assert torch.equal(d[k].double(), d64[k]), k
    eps32 = torch.tensor(d["eps"], dtype=torch.float32)
    assert float(eps32) == d["eps"], "eps is not a float32 value"

    # statistics by the finalize kernel's formulas
    s = d64["x"].sum(dim=(0, 2, 3))
    ss = (d64["x"] * d64["x"]).sum(dim=(0, 2, 3))
    if case.training:
        mean = s / R
        var = (ss / R - mean * mean).clamp_min(0.0)
        assert torch.equal(mean, m)
        assert torch.equal(ss, R * m * m + 8 * P)
        invstd = torch.rsqrt(var + float(eps32.double()))
        rm1 = 0.5 * d64["rm"] + 0.5 * mean
        assert _exact_in(rm1, torch.float32)
        assert (d64["rm"] % 2 == 0).all() and (d64["rv"] == 0).all()
    else:
        mean = d64["rm"]
        assert torch.equal(mean, m)
        invstd = torch.rsqrt(d64["rv"] + float(eps32.double()))
    assert (invstd.float() == 0.5).all(), invstd

    f = bc.formulas64(case, d64, mean, invstd.float().double())
    assert ((f["xhat"].abs() == 1) | (f["xhat"] == 0)).all()
    for k in ("v", "y", "g"):
        assert _exact_in(f[k], case.dtype), k
    assert ((f["v"] * 4) % 2 == 1).all(), "v is no odd multiple of 0.25"
    assert (f["v"] != 0).all() and (f["v"] != 6).all()
    if case.act == "relu6" and P > 0:
        assert (f["v"] > 6).any(), "the upper clamp is never reached"
    if case.act != "none":
        assert (f["v"] < 0).any() and f["gate"].any()
    # k1 is a power of two; dgamma and dbeta are integers
    k1 = f["k1"].abs()
    assert (torch.frexp(k1)[0] == 0.5).all()
    assert torch.equal(f["dgamma"], f["dgamma"].round())
    assert torch.equal(f["dbeta"], f["dbeta"].round())

    # every partial sum of every reduce is exact in fp32: bounded by the
    # sum of magnitudes, and every term an integer
    for terms in (d64["x"], d64["x"] * d64["x"], f["g"], f["g"] * f["xhat"]):
        assert torch.equal(terms, terms.round())
        assert (terms.abs().sum(dim=(0, 2, 3)) < LIMIT).all()


def test_dyadic_gate_sets_cover_relu6_with_a_mask():
    """The dyadic run crosses the mask with y on every case whose forward
    writes one, relu6 included."""
    both = [c for c in bc.CASES if bc.dyadic_gates(c) == ("mask", "y")]
    assert {c.act for c in both} == {"relu", "relu6"}
    assert set(bc.CROSS_CHECK) <= {c.name for c in both}


def test_unpack_mask_bit_order():
    case = bc.CASE_BY_NAME["c8_relu_train"]
    N, C, H, W = case.shape
    want = torch.zeros(N, H, W, C, dtype=torch.bool)
    mask = torch.zeros(N * H * W * C // 8, dtype=torch.uint8)
    # element i = 8 * 5 + 3 in memory order: row 5, channel 3
    mask[5] = 1 << 3
    want.view(-1)[8 * 5 + 3] = True
    assert torch.equal(bc.unpack_mask(mask, case), want.permute(0, 3, 1, 2))


def test_half_ulp_bf16():
    ref = torch.tensor([0.0, 1.0, 1.5, -2.0, 0.75, 255.0],
                       dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9,
                         0.5], dtype=torch.float64)
    assert torch.equal(bc.half_ulp_bf16(ref), want)
