"""Shapes, inputs and the step-wise float64 checker shared by the LSTM
tests (test_lstm_cpu.py checks the checker itself, test_lstm_gpu.py holds
the step kernels to it).

Cases (T, B, I, H), the smallest that reach each path of the step kernels
(16 units x 16 batch rows per block, K dealt to four waves in 32-wide
steps, 128 per round):
  widths, at T = 2, B = 3
    H = 8     below one MFMA K step and one N tile
    H = 40    ragged in K and in N (I = 24: the input width is free)
    H = 128   the width of the GNMT train-step test; one full K round
    H = 520   ragged above several tiles and K rounds
    H = 1024  GNMT; eight XCD slices
  batch sizes, at T = 2, H = 128: B = 1, 3, 17 (ragged M, two tiles), 64
  lengths, at B = 3, H = 128: T = 1, 2, 5
  (5, 17, 520, 520): the reproducibility case
each without and with an initial state.

The step-wise bound. Step t is recomputed in float64 from the kernel's own
y[t-1] (bf16) and cs[t-1] (fp32), both exact in float64, so the bound is
per step and nothing compounds. With u = 2^-24 (fp32 unit roundoff):
  A_pre = |xproj| + |bias| + sum_k |h_k w_k|
  E_pre = (H + 4) u A_pre     H products, exact in fp32 (bf16 x bf16), summed
                              in fp32 in any order, plus the xproj and bias
                              adds: at most H + 2 roundings, each relative
                              to a partial sum bounded by A_pre
  E_s = E_pre / 4 + 1e-6      sigma' <= 1/4; 1e-6 covers the exp2 /
                              reciprocal evaluation of a value in [0, 1]
  E_g = E_pre + 1e-6          tanh' <= 1
  E_c = |c_prev| E_f + E_i + E_g + 2^-22 (1 + |c_prev|)
                              |i|, |g| <= 1; two products and one add, each
                              rounded once, on terms bounded by |c_prev|
                              and 1
  E_h = E_o + E_c + 1e-6      |tanh c| <= 1, tanh' <= 1, |o| <= 1
A value v stored as bf16 with |v - ref| <= E moves by one round-to-nearest
to 8 significant bits (7 stored + the implicit one): half a unit in the
last place is 2^-8 of the leading power of two, so at most 2^-8 |v| <=
2^-8 (|ref| + E). (2^-9, the starting point the design note gave, is half
of that: it would be right for 9 significant bits, and the fp32 model of
the kernel alone already reaches 1.85x of it just above a power of two.)
  stored y, gates:  E (1 + 2^-8) + 2^-8 |ref|
  stored cs (fp32): E_c"""

import functools

import torch

U = 2.0 ** -24
W_CASES = [(2, 3, 8, 8), (2, 3, 24, 40), (2, 3, 128, 128),
           (2, 3, 520, 520), (2, 3, 1024, 1024)]
B_CASES = [(2, B, 128, 128) for B in (1, 3, 17, 64)]
T_CASES = [(T, 3, 128, 128) for T in (1, 2, 5)]
REPRO_CASE = (5, 17, 520, 520)
CASES = list(dict.fromkeys(W_CASES + B_CASES + T_CASES + [REPRO_CASE]))
NAMES = ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")


@functools.lru_cache(maxsize=None)
def inputs(T, B, I, H):
    """bf16-rounded CPU inputs (held as bf16) and cotangents, built once
    per shape and shared read-only."""
    g = torch.Generator().manual_seed(((T * 100 + B) * 10000 + I) * 10000 + H)
    k = H ** -0.5

    def uni(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * k).bfloat16()

    def nrm(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).bfloat16()

    return {
        "x": nrm(T, B, I), "w_ih": uni(4 * H, I), "w_hh": uni(4 * H, H),
        "b_ih": uni(4 * H), "b_hh": uni(4 * H),
        "h0": nrm(1, B, H, scale=0.5), "c0": nrm(1, B, H),
        "dy": nrm(T, B, H), "dh_T": nrm(1, B, H), "dc_T": nrm(1, B, H),
    }


def kernel_model_f32(xproj, w_hh, bias, h0, c0):
    """The step kernel's arithmetic in fp32 torch ops: xproj (T, B, 4H) and
    w_hh bf16, bias fp32, h0 bf16 / c0 fp32 (B, H) or None. Each step reads
    the previous step's bf16-rounded y and fp32 c. Returns y (bf16),
    cs (fp32), gates (bf16) as the kernel stores them."""
    T, B, _ = xproj.shape
    H = w_hh.size(1)
    h = h0.float() if h0 is not None else torch.zeros(B, H)
    c = c0.float() if c0 is not None else torch.zeros(B, H)
    w_t = w_hh.float().t()
    ys, cs, gs = [], [], []
    for t in range(T):
        pre = h @ w_t + xproj[t].float() + bias
        i, f, g, o = pre.chunk(4, dim=1)
        i, f, g, o = (torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g),
                      torch.sigmoid(o))
        c = f * c + i * g
        y = (o * torch.tanh(c)).bfloat16()
        h = y.float()
        ys.append(y)
        cs.append(c)
        gs.append(torch.cat([i, f, g, o], dim=1).bfloat16())
    return torch.stack(ys), torch.stack(cs), torch.stack(gs)


def stepwise_ratios(xproj, w_hh, bias, h0, c0, y, cs, gates):
    """Worst err / bound over all steps for the stored y, cs and gates
    (CPU tensors in the kernel's dtypes; h0 / c0 (B, H) or None)."""
    T, B, _ = xproj.shape
    H = w_hh.size(1)
    d = torch.float64
    w_t = w_hh.to(d).t()
    bias = bias.to(d)
    worst = {"y": 0.0, "cs": 0.0, "gates": 0.0}

    def ratio(got, ref, bound):
        return float(((got.to(d) - ref).abs() / bound).max())

    for t in range(T):
        if t > 0:
            h, c = y[t - 1].to(d), cs[t - 1].to(d)
        else:
            h = h0.to(d) if h0 is not None else torch.zeros(B, H, dtype=d)
            c = c0.to(d) if c0 is not None else torch.zeros(B, H, dtype=d)
        xp = xproj[t].to(d)
        pre = xp + bias + h @ w_t
        a_pre = xp.abs() + bias.abs() + h.abs() @ w_t.abs()
        e_pre = (H + 4) * U * a_pre
        pi, pf, pg, po = pre.chunk(4, dim=1)
        ei, ef, eg, eo = e_pre.chunk(4, dim=1)
        i, f, g, o = (torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg),
                      torch.sigmoid(po))
        ei, ef, eo = ei / 4 + 1e-6, ef / 4 + 1e-6, eo / 4 + 1e-6
        eg = eg + 1e-6
        c_ref = f * c + i * g
        e_c = c.abs() * ef + ei + eg + 2.0 ** -22 * (1 + c.abs())
        h_ref = o * torch.tanh(c_ref)
        e_h = eo + e_c + 1e-6
        g_ref = torch.cat([i, f, g, o], dim=1)
        e_gate = torch.cat([ei, ef, eg, eo], dim=1)
        r8 = 2.0 ** -8
        worst["y"] = max(worst["y"], ratio(
            y[t], h_ref, e_h * (1 + r8) + r8 * h_ref.abs()))
        worst["cs"] = max(worst["cs"], ratio(cs[t], c_ref, e_c))
        worst["gates"] = max(worst["gates"], ratio(
            gates[t], g_ref, e_gate * (1 + r8) + r8 * g_ref.abs()))
    return worst
