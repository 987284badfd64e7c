"""bf16 Linear kernels (csrc/linear.hip) on the GPU: exact arithmetic
against a float64 CPU reference on lattice data in all three directions,
the bias variants, weight-grad determinism, the nn.Linear bridge and the
binding guards."""

import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import exact_mismatches, lattice

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (M, N, K)
SHAPES = [
    (1, 8, 8),          # one row, one chunk: the decode step
    (5, 8, 40),         # M < 16; K = 32 + 8, a partial MFMA k-step
    (130, 136, 72),     # just past a tile in M and N; K crosses one BK
    (257, 24, 8),       # dgrad reduces 24, wgrad an odd 257; minimum K
    (64, 1000, 2048),   # ResNet-50 head: ragged N tile, the LDS ring wraps
    (4100, 16, 16),     # many m-slabs in the weight-grad
    (300, 136, 264),    # the 128 weight-grad tile with slabs (dW and db)
    (2050, 2056, 2184),  # the 128 tile in every direction, ragged everywhere
]
SPLIT_SHAPE = (4100, 16, 16)


def _dev():
    return torch.device("cuda", 0)


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


@functools.lru_cache(maxsize=None)
def _case(shape, bias=BF):
    """Seeded lattice inputs (CPU) and the float64 reference of F.linear and
    its autograd; computed once and shared read-only."""
    M, N, K = shape
    assert 9 * max(M, N, K) + 3 < 2 ** 24   # every partial sum exact in fp32
    g = torch.Generator().manual_seed(8200 + SHAPES.index(shape))
    x, w, dy = (lattice(d, g) for d in ((M, K), (N, K), (M, N)))
    b = lattice((N,), g).to(bias) if bias is not None else None
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    y64 = F.linear(x64, w64, b64)
    y64.backward(dy.double())
    return {"x": x, "w": w, "b": b, "dy": dy, "y": y64.detach(),
            "dx": x64.grad, "dw": w64.grad,
            "db": b64.grad if b is not None else None}


def _gpu(t):
    return t.to(_dev()) if t is not None else None


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("direction", ["fwd", "dgrad", "wgrad"])
def test_linear_exact(direction, shape):
    ext = _ext()
    c = _case(shape)
    if shape == SPLIT_SHAPE:
        assert ext.linear_plan(*shape)["wgrad"]["split"] >= 2
    x, w, b, dy = (_gpu(c[k]) for k in ("x", "w", "b", "dy"))
    if direction == "fwd":
        assert exact_mismatches(ext.linear_fwd(x, w, b), c["y"], BF) == 0
    elif direction == "dgrad":
        assert exact_mismatches(ext.linear_dgrad(dy, w), c["dx"], BF) == 0
    else:
        dw, db = ext.linear_wgrad(dy, x, True, BF)
        assert exact_mismatches(dw, c["dw"], BF) == 0
        assert exact_mismatches(db, c["db"], BF) == 0


@pytest.mark.parametrize("shape", [(130, 136, 72), (300, 136, 264)], ids=str)
@pytest.mark.parametrize("bias", [None, BF, torch.float32], ids=str)
def test_linear_bias_variants(bias, shape):
    ext = _ext()
    c = _case(shape, bias)
    x, w, b, dy = (_gpu(c[k]) for k in ("x", "w", "b", "dy"))
    assert exact_mismatches(ext.linear_fwd(x, w, b), c["y"], BF) == 0
    dw, db = ext.linear_wgrad(dy, x, bias is not None, bias or BF)
    assert exact_mismatches(dw, c["dw"], BF) == 0
    if bias is None:
        assert db is None
    else:
        assert exact_mismatches(db, c["db"], bias) == 0


def test_linear_wgrad_deterministic():
    ext = _ext()
    M, N, K = SPLIT_SHAPE
    assert ext.linear_plan(M, N, K)["wgrad"]["split"] >= 2
    g = torch.Generator().manual_seed(11)
    dy = _gpu(torch.randn(M, N, generator=g).to(BF))
    x = _gpu(torch.randn(M, K, generator=g).to(BF))
    dw1, db1 = ext.linear_wgrad(dy, x, True, torch.float32)
    dw2, db2 = ext.linear_wgrad(dy, x, True, torch.float32)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


def _view(kind, x):
    """The (B, T, K) input x as the view the bridge has to cope with."""
    if kind == "transposed":   # what RecurrentAttention hands to linear_q
        return x.transpose(0, 1).contiguous().transpose(0, 1)
    if kind == "misaligned":   # a storage offset of one element
        flat = x.new_empty(x.numel() + 1)
        flat[1:].copy_(x.reshape(-1))
        return flat[1:].view(x.shape)
    return x


@pytest.mark.parametrize("kind", ["plain", "transposed", "misaligned"])
def test_linear_bridge(kind, monkeypatch):
    from ddlbench_amd.ops.modules import Linear, convert_linears
    shape = (130, 136, 72)
    M, N, K = shape
    c = _case(shape)
    model = nn.Sequential(nn.Linear(K, N)).to(_dev()).to(BF)
    with torch.no_grad():
        model[0].weight.copy_(c["w"])
        model[0].bias.copy_(c["b"])
    params = list(model.parameters())
    assert convert_linears(model) == 1 and isinstance(model[0], Linear)
    assert all(a is b for a, b in zip(model.parameters(), params))

    x = _view(kind, _gpu(c["x"]).view(10, 13, K)).requires_grad_(True)
    assert (kind == "plain") == (x.is_contiguous()
                                 and x.data_ptr() % 16 == 0)
    y = model(x)
    y.backward(_gpu(c["dy"]).view(10, 13, N))
    assert exact_mismatches(y.detach().reshape(M, N), c["y"], BF) == 0
    assert exact_mismatches(x.grad.reshape(M, K), c["dx"], BF) == 0
    assert exact_mismatches(model[0].weight.grad, c["dw"], BF) == 0
    assert exact_mismatches(model[0].bias.grad, c["db"], BF) == 0

    # x needs no gradient: the data-grad kernel is not launched
    def no_dgrad(*a):
        raise AssertionError("linear_dgrad launched without need")
    monkeypatch.setattr(_ext(), "linear_dgrad", no_dgrad)
    model.zero_grad(set_to_none=True)
    model(x.detach()).backward(_gpu(c["dy"]).view(10, 13, N))
    assert exact_mismatches(model[0].weight.grad, c["dw"], BF) == 0


@pytest.mark.parametrize("name", ["fp32 x", "K % 8", "N % 8", "K mismatch",
                                  "cpu tensor"])
def test_linear_binding_guards(name):
    ext = _ext()

    def t(*shape, dtype=BF, device=None):
        return torch.zeros(shape, dtype=dtype, device=device or _dev())

    calls = {
        "fp32 x": lambda: ext.linear_fwd(t(4, 16, dtype=torch.float32),
                                         t(8, 16)),
        "K % 8": lambda: ext.linear_fwd(t(4, 12), t(8, 12)),
        "N % 8": lambda: ext.linear_fwd(t(4, 16), t(12, 16)),
        "K mismatch": lambda: ext.linear_fwd(t(4, 16), t(8, 24)),
        "cpu tensor": lambda: ext.linear_wgrad(t(4, 8, device="cpu"),
                                               t(4, 16), False, BF),
    }
    with pytest.raises(RuntimeError, match="linear: "):
        calls[name]()
