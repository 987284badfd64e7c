"""Native LSTM recurrence (lstm_step_* kernels) on the GPU. All @gpu.

Shapes and the forward bound are in lstm_cases.py: every step is recomputed
in float64 from the kernel's own previous y and c, so the bound is per step
and derived from the fp32 rounding model, not fitted.

Backward is held to the library's own bf16 error: for every gradient,
e = ||got - ref||_2 / ||ref||_2 against torch.nn.LSTM in float64 on the CPU
(same bf16-rounded inputs), and e_native <= 3 e_library, the library being
nn.LSTM in bf16 on the same GPU in the same test. The margin of 3 pays for
the gates and dgates the native path keeps in bf16. Where ||ref|| is zero
(dW_hh at T = 1 without an initial state) the native gradient must be
exactly zero. Measured e_library / e_native per tensor are recorded in
profiles/lstm_r10.md."""

import functools

import pytest
import torch
import torch.nn as nn

import lstm_cases as lc
from ddlbench_amd.ops import functional as NF
from ddlbench_amd.ops.modules import LSTM

pytestmark = pytest.mark.gpu

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    from ddlbench_amd import ops
    assert ops.extension_available(), \
        "native extension must be present on the GPU box"


def _module(case, backend, dtype=torch.bfloat16, device=None):
    T, B, I, H = case
    d = lc.inputs(*case)
    m = LSTM(I, H, backend=backend)
    with torch.no_grad():
        for name, key in zip(PARAMS, ("w_ih", "w_hh", "b_ih", "b_hh")):
            getattr(m, name).copy_(d[key].float())
    return m.to(dtype).to(device or _dev())


def _run(case, with_hx, backend, dtype=torch.bfloat16, device=None):
    """y, h_T, c_T and the gradients (x, four parameters, h0, c0 when
    given) of sum(y dy) + sum(h_T dh_T) + sum(c_T dc_T)."""
    device = device or _dev()
    d = lc.inputs(*case)
    m = _module(case, backend, dtype, device)
    to = lambda t: t.to(dtype).to(device)
    leaves = [to(d["x"]).requires_grad_(True)]
    leaves += [getattr(m, n) for n in PARAMS]
    hx = None
    if with_hx:
        hx = (to(d["h0"]).requires_grad_(True),
              to(d["c0"]).requires_grad_(True))
        leaves += list(hx)
    y, (h_T, c_T) = m(leaves[0], hx)
    loss = (y.float() * to(d["dy"]).float()).sum() \
        + (h_T.float() * to(d["dh_T"]).float()).sum() \
        + (c_T.float() * to(d["dc_T"]).float()).sum()
    grads = torch.autograd.grad(loss, leaves)
    return [y, h_T, c_T], list(grads)


@functools.lru_cache(maxsize=None)
def _reference(case, with_hx):
    """float64 CPU nn.LSTM on the bf16-rounded inputs; computed once."""
    outs, grads = _run(case, with_hx, "library", torch.float64,
                       torch.device("cpu"))
    return [g.detach() for g in grads]


def _rel_l2(got, ref):
    return float((got.detach().double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("with_hx", [False, True])
@pytest.mark.parametrize("case", lc.CASES, ids=str)
def test_forward_stepwise_against_float64(case, with_hx):
    from ddlbench_amd import ops
    ext = ops.require_extension()
    T, B, I, H = case
    dev = _dev()
    d = {k: v.to(dev) for k, v in lc.inputs(*case).items()}
    xproj = torch.mm(d["x"].view(T * B, I), d["w_ih"].t()).view(T, B, 4 * H)
    bias = d["b_ih"].float() + d["b_hh"].float()
    h0 = d["h0"][0].contiguous() if with_hx else None
    c0 = d["c0"][0].float().contiguous() if with_hx else None
    y, cs, gates = ext.lstm_fwd(xproj, d["w_hh"], bias, h0, c0, True)
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu() if t is not None else None
    worst = lc.stepwise_ratios(cpu(xproj), cpu(d["w_hh"]), cpu(bias),
                               cpu(h0), cpu(c0), cpu(y), cpu(cs), cpu(gates))
    print(f"lstm fwd {case} hx={with_hx} worst err/bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst

    # the public entry point runs the same kernels on the same operands
    hx = (d["h0"], d["c0"]) if with_hx else None
    y2, (h_T, c_T) = NF.lstm(d["x"], d["w_ih"], d["w_hh"], d["b_ih"],
                             d["b_hh"], hx, backend="native")
    assert torch.equal(y2, y)
    assert h_T.shape == c_T.shape == (1, B, H)
    assert h_T.dtype == c_T.dtype == torch.bfloat16
    assert torch.equal(h_T[0], y[-1])
    assert torch.equal(c_T[0], cs[-1].bfloat16())
    # skipping the gates changes nothing else
    y3, cs3, none = ext.lstm_fwd(xproj, d["w_hh"], bias, h0, c0, False)
    assert none is None and torch.equal(y3, y) and torch.equal(cs3, cs)


@pytest.mark.parametrize("with_hx", [False, True])
@pytest.mark.parametrize("case", lc.CASES, ids=str)
def test_backward_against_the_library_error(case, with_hx):
    ref = _reference(case, with_hx)
    _, g_nat = _run(case, with_hx, "native")
    _, g_lib = _run(case, with_hx, "library")
    names = ("dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0", "dc0")
    failures = []
    for name, r, gn, gl in zip(names, ref, g_nat, g_lib):
        assert gn.shape == r.shape and gn.dtype == torch.bfloat16
        if float(r.norm()) == 0.0:
            print(f"lstm bwd {case} hx={with_hx} {name}: reference is zero")
            assert float(gn.float().abs().max()) == 0.0
            continue
        e_nat, e_lib = _rel_l2(gn, r), _rel_l2(gl, r)
        print(f"lstm bwd {case} hx={with_hx} {name}: "
              f"e_library {e_lib:.3e} e_native {e_nat:.3e} "
              f"ratio {e_nat / e_lib:.2f}")
        if not e_nat <= 3 * e_lib:
            failures.append((name, e_nat, e_lib))
    assert not failures, failures


def test_bitwise_reproducible():
    a = _run(lc.REPRO_CASE, True, "native")
    b = _run(lc.REPRO_CASE, True, "native")
    for s, t in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(s, t)


def test_no_grad_decode_step_matches_grad_forward():
    case = (1, 3, 128, 128)
    dev = _dev()
    d = lc.inputs(*case)
    m = _module(case, "native")
    x = d["x"].to(dev)
    hx = (d["h0"].to(dev), d["c0"].to(dev))
    y, (h_T, c_T) = m(x, hx)
    assert y.requires_grad
    with torch.no_grad():
        y2, (h2, c2) = m(x, hx)
    assert not y2.requires_grad
    assert torch.equal(y, y2) and torch.equal(h_T, h2) \
        and torch.equal(c_T, c2)


def test_explicit_native_rejects_what_it_cannot_run():
    dev = _dev()
    m = LSTM(16, 16, backend="native").to(dev)          # fp32
    with pytest.raises(NotImplementedError, match="float32"):
        m(torch.randn(2, 3, 16, device=dev))
    m = LSTM(16, 12, backend="native").to(dev).bfloat16()
    with pytest.raises(NotImplementedError, match="12"):
        m(torch.randn(2, 3, 16, device=dev, dtype=torch.bfloat16))
    m = LSTM(16, 16, backend="native").to(dev).double()
    with pytest.raises(NotImplementedError, match="float64"):
        m(torch.randn(2, 3, 16, device=dev, dtype=torch.float64))


def _gnmt_loss(dtype, backend, monkeypatch, backward=False):
    from ddlbench_amd.models.gnmt import GNMT, LabelSmoothingLoss
    monkeypatch.setenv("DDLB_LSTM", backend)
    dev = _dev()
    torch.manual_seed(0)
    model = GNMT(vocab_size=96, hidden_size=128, num_layers=4,
                 dropout=0.0).to(dev).to(dtype)
    g = torch.Generator().manual_seed(1)
    src = torch.randint(3, 96, (7, 3), generator=g).to(dev)
    src_len = torch.tensor([7, 5, 2], device=dev)
    tgt = torch.randint(3, 96, (6, 3), generator=g).to(dev)
    loss = LabelSmoothingLoss()(model(src, src_len, tgt[:-1]), tgt[1:])
    if backward:
        loss.backward()
        for name, p in model.named_parameters():
            assert p.grad is not None, name
            assert bool(torch.isfinite(p.grad).all()), name
    return float(loss)


def test_gnmt_train_step_within_the_bf16_noise_floor(monkeypatch):
    native = _gnmt_loss(torch.bfloat16, "native", monkeypatch, backward=True)
    lib_bf16 = _gnmt_loss(torch.bfloat16, "library", monkeypatch)
    lib_fp32 = _gnmt_loss(torch.float32, "library", monkeypatch)
    print(f"gnmt loss: native bf16 {native:.6f}, library bf16 "
          f"{lib_bf16:.6f}, library fp32 {lib_fp32:.6f}")
    assert abs(native - lib_bf16) <= 2 * abs(lib_bf16 - lib_fp32)


def test_greedy_decode_agrees_between_backends(monkeypatch):
    from ddlbench_amd.models.gnmt import GNMT
    from ddlbench_amd.translation import Translator
    dev = _dev()
    torch.manual_seed(21)
    model = GNMT(vocab_size=96, hidden_size=64, num_layers=2) \
        .to(dev).bfloat16()
    src = torch.randint(3, 96, (9, 4), device=dev)
    src_len = torch.tensor([9, 7, 4, 2], device=dev)
    outs = {}
    for backend in ("native", "library"):
        monkeypatch.setenv("DDLB_LSTM", backend)
        outs[backend] = Translator(model, max_len=6).greedy(src, src_len)
    assert torch.equal(outs["native"], outs["library"])
