#!/usr/bin/env python3
"""Fused-op microbenchmarks vs eager PyTorch: BN+ReLU(+add), CE,
label-smoothed CE, attention score, LSTM, SGD (--ops picks arms).

Reports ms and achieved HBM GB/s per op over ResNet-50 activation
shapes in both layouts — the evidence for the memory-bound fusion wins
and the input to kernel tuning (MI355X HBM3E ceiling ~6.3 TB/s)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torch  # noqa: E402

SHAPES = [  # (N, C, H, W) resnet50 @224
    (256, 64, 112, 112), (256, 256, 56, 56), (256, 512, 28, 28),
    (256, 1024, 14, 14), (256, 2048, 7, 7),
]


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_ls_ce(dev, iters, warmup, rounds=5):
    """Label-smoothed CE, forward + backward, bf16 logits at GNMT's vocab
    with ~20 % of the rows ignored: the fused op against the eager
    composition (backend="torch"), alternated in rounds in one process.
    GB/s is taken against the byte floor: valid rows read once forward,
    read once and written once backward = 3 * valid_rows * K * 2 bytes
    (the zero fill of ignored dx rows is not counted)."""
    from ddlbench_amd.ops import functional as NF
    K = 32320
    for R in (512, 6400):
        g = torch.Generator(device=dev).manual_seed(R)
        x = torch.randn(R, K, device=dev, dtype=torch.bfloat16,
                        generator=g).requires_grad_(True)
        t = torch.randint(1, K, (R,), device=dev, generator=g)
        t[torch.rand(R, device=dev, generator=g) < 0.2] = 0
        valid = int((t != 0).sum())

        def step(backend):
            x.grad = None
            NF.label_smoothing_cross_entropy(
                x, t, 0.1, 0, "mean", backend=backend).backward()

        times = {"native": [], "torch": []}
        peak = {}
        for backend in times:
            step(backend)
            x.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(backend)
            torch.cuda.synchronize()
            # beyond the logits: dx included, it is part of either arm
            peak[backend] = torch.cuda.max_memory_allocated() - base
        for _ in range(rounds):
            for backend in times:
                times[backend].append(
                    timeit(lambda: step(backend), iters, warmup))
        med = {b: sorted(v)[len(v) // 2] for b, v in times.items()}
        floor = 3 * valid * K * 2
        print(json.dumps({
            "op": "ls_ce_fwd_bwd", "shape": f"{R}x{K}", "dtype": "bfloat16",
            "valid_rows": valid,
            "fused_ms": round(med["native"] * 1e3, 4),
            "fused_ms_min": round(min(times["native"]) * 1e3, 4),
            "eager_ms": round(med["torch"] * 1e3, 4),
            "eager_ms_min": round(min(times["torch"]) * 1e3, 4),
            "speedup": round(med["torch"] / med["native"], 2),
            "fused_GBs": round(floor / med["native"] / 1e9, 0),
            "floor_bytes": floor,
            "fused_peak_MB": round(peak["native"] / 2**20, 1),
            "eager_peak_MB": round(peak["torch"] / 2**20, 1)}), flush=True)
        del x, t


def bench_attn(dev, iters, warmup, rounds=5):
    """Bahdanau attention score, bf16, H = 1024, about a fifth of the keys
    masked through per-sentence lengths: the fused op against the eager
    composition (backend="torch"), alternated in rounds in one process.
    Training shapes run forward + backward through autograd, the decode
    shape (Tq = 1) forward only under no_grad. Gtanh/s is
    valid (b,i,j) * H over the fused time: the size of the problem, not the
    kernels' own evaluation count (a training step evaluates tanh three
    times per element: once forward, twice in the two backward sweeps)."""
    from ddlbench_amd.ops import functional as NF
    H = 1024
    dt = torch.bfloat16
    for B, Tq, Tk, train in ((64, 32, 32, True), (128, 50, 50, True),
                             (64, 1, 50, False)):
        g = torch.Generator(device=dev).manual_seed(B * Tk)
        mk = lambda *s: torch.randn(*s, device=dev, dtype=dt, generator=g)
        q, k = mk(B, Tq, H), mk(B, Tk, H)
        bias = 0.1 * mk(H)
        vn = mk(H)
        vn = vn / vn.float().norm().to(dt)
        ds = mk(B, Tq, Tk)
        # lengths in [0.6 Tk, Tk]: a fifth of the keys masked on average
        lengths = (Tk * (0.6 + 0.4 * torch.rand(B, device=dev, generator=g))
                   ).round().long().clamp(1, Tk)
        mask = torch.arange(Tk, device=dev).unsqueeze(0) \
            < lengths.unsqueeze(1)
        valid = int(mask.sum()) * Tq
        leaves = [t.requires_grad_(train) for t in (q, k, bias, vn)]

        def step(backend):
            if not train:
                with torch.no_grad():
                    NF.attention_score(*leaves, mask, backend=backend)
                return
            for t in leaves:
                t.grad = None
            NF.attention_score(*leaves, mask, backend=backend).backward(ds)

        times = {"native": [], "torch": []}
        peak = {}
        for backend in times:
            step(backend)
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(backend)
            torch.cuda.synchronize()
            # beyond the inputs: outputs and gradients are part of each arm
            peak[backend] = torch.cuda.max_memory_allocated() - base
        for _ in range(rounds):
            for backend in times:
                times[backend].append(
                    timeit(lambda: step(backend), iters, warmup))
        med = {b: sorted(v)[len(v) // 2] for b, v in times.items()}
        print(json.dumps({
            "op": "attn_score_fwd_bwd" if train else "attn_score_fwd",
            "shape": f"B{B} Tq{Tq} Tk{Tk} H{H}", "dtype": "bfloat16",
            "valid_bij": valid,
            "fused_ms": round(med["native"] * 1e3, 4),
            "fused_ms_min": round(min(times["native"]) * 1e3, 4),
            "eager_ms": round(med["torch"] * 1e3, 4),
            "eager_ms_min": round(min(times["torch"]) * 1e3, 4),
            "speedup": round(med["torch"] / med["native"], 2),
            "fused_Gtanh_s": round(valid * H / med["native"] / 1e9, 1),
            "fused_peak_MB": round(peak["native"] / 2**20, 2),
            "eager_peak_MB": round(peak["torch"] / 2**20, 2)}), flush=True)
        del q, k, ds, leaves


def bench_lstm(dev, iters, warmup, rounds=5):
    """One single-layer bf16 LSTM, the native recurrence against the library
    path (ops.modules.LSTM backend "native" / "library"), alternated in
    rounds in one process. Training shapes run forward + backward through
    autograd with gradients to x and all four parameters; the decode shape
    (T = 1, with hx) runs forward only under no_grad."""
    from ddlbench_amd.ops.modules import LSTM
    dt = torch.bfloat16
    for T, B, I, H, train in ((50, 64, 1024, 1024, True),
                              (32, 128, 2048, 1024, True),
                              (1, 64, 2048, 1024, False)):
        torch.manual_seed(T * B)
        m = LSTM(I, H).to(dev).to(dt)
        g = torch.Generator(device=dev).manual_seed(T * B + I)
        mk = lambda *s: torch.randn(*s, device=dev, dtype=dt, generator=g)
        x = mk(T, B, I).requires_grad_(train)
        dy = mk(T, B, H)
        hx = None if train else (mk(1, B, H), mk(1, B, H))

        def step(backend):
            m.backend = backend
            if not train:
                with torch.no_grad():
                    m(x, hx)
                return
            x.grad = None
            m.zero_grad(set_to_none=True)
            m(x)[0].backward(dy)

        times = {"native": [], "library": []}
        peak = {}
        for backend in times:
            step(backend)
            x.grad = None
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(backend)
            torch.cuda.synchronize()
            # beyond x and the weights: outputs, saved state and gradients
            peak[backend] = torch.cuda.max_memory_allocated() - base
        for _ in range(rounds):
            for backend in times:
                times[backend].append(
                    timeit(lambda: step(backend), iters, warmup))
        med = {b: sorted(v)[len(v) // 2] for b, v in times.items()}
        print(json.dumps({
            "op": "lstm_fwd_bwd" if train else "lstm_fwd_decode",
            "shape": f"T{T} B{B} I{I} H{H}", "dtype": "bfloat16",
            "native_ms": round(med["native"] * 1e3, 4),
            "native_ms_min": round(min(times["native"]) * 1e3, 4),
            "library_ms": round(med["library"] * 1e3, 4),
            "library_ms_min": round(min(times["library"]) * 1e3, 4),
            "speedup": round(med["library"] / med["native"], 2),
            "native_peak_MB": round(peak["native"] / 2**20, 2),
            "library_peak_MB": round(peak["library"] / 2**20, 2)}),
            flush=True)
        del m, x, dy, hx


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--dtype", default="bfloat16")
    p.add_argument("--ops", default="bn,ce,ls_ce,attn,lstm,sgd",
                   help="comma-separated arms: bn, ce, ls_ce, attn, lstm, "
                        "sgd")
    args = p.parse_args()
    arms = set(args.ops.split(","))
    assert arms <= {"bn", "ce", "ls_ce", "attn", "lstm", "sgd"}, args.ops
    assert torch.cuda.is_available()
    from ddlbench_amd.ops import functional as NF
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16 if args.dtype == "bfloat16" else torch.float32
    esz = torch.tensor([], dtype=dt).element_size()

    for nhwc in ((False, True) if "bn" in arms else ()):
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        for N, C, H, W in SHAPES:
            x = torch.randn(N, C, H, W, device=dev, dtype=dt) \
                .contiguous(memory_format=fmt)
            res = torch.randn_like(x)
            g = torch.rand(C, device=dev) + 0.5
            b = torch.randn(C, device=dev)
            rm = torch.zeros(C, device=dev)
            rv = torch.ones(C, device=dev)
            nb = N * C * H * W * esz

            def fused_fwd():
                return NF.bn_act(x, g, b, rm, rv, True, 0.1, 1e-5,
                                 "relu", res, backend="native")

            def eager_fwd():
                y = torch.nn.functional.batch_norm(x, rm, rv, g, b, True,
                                                   0.1, 1e-5)
                return torch.relu(y + res)

            t_f = timeit(fused_fwd, args.iters, args.warmup)
            t_e = timeit(eager_fwd, args.iters, args.warmup)
            # fwd traffic: read x (2x: stats+apply), read res, write y
            row = {"op": "bn_add_relu_fwd",
                   "layout": "nhwc" if nhwc else "nchw",
                   "shape": f"{N}x{C}x{H}x{W}",
                   "fused_ms": round(t_f * 1e3, 3),
                   "eager_ms": round(t_e * 1e3, 3),
                   "fused_GBs": round(4 * nb / t_f / 1e9, 0),
                   "speedup": round(t_e / t_f, 2)}
            print(json.dumps(row), flush=True)

            # backward
            xg = x.clone().requires_grad_(True)
            rg = res.clone().requires_grad_(True)
            gg = g.clone().requires_grad_(True)
            bg = b.clone().requires_grad_(True)
            y = NF.bn_act(xg, gg, bg, rm.clone(), rv.clone(), True, 0.1,
                          1e-5, "relu", rg, backend="native")
            dy = torch.randn_like(y)

            def fused_bwd():
                grads = torch.autograd.grad(y, [xg, rg, gg, bg], dy,
                                            retain_graph=True)
                return grads

            x2 = x.clone().requires_grad_(True)
            r2 = res.clone().requires_grad_(True)
            g2 = g.clone().requires_grad_(True)
            b2 = b.clone().requires_grad_(True)
            y2 = torch.relu(torch.nn.functional.batch_norm(
                x2, rm.clone(), rv.clone(), g2, b2, True, 0.1, 1e-5) + r2)

            def eager_bwd():
                return torch.autograd.grad(y2, [x2, r2, g2, b2], dy,
                                           retain_graph=True)

            t_f = timeit(fused_bwd, args.iters, args.warmup)
            t_e = timeit(eager_bwd, args.iters, args.warmup)
            row = {"op": "bn_add_relu_bwd",
                   "layout": "nhwc" if nhwc else "nchw",
                   "shape": f"{N}x{C}x{H}x{W}",
                   "fused_ms": round(t_f * 1e3, 3),
                   "eager_ms": round(t_e * 1e3, 3),
                   "fused_GBs": round(6 * nb / t_f / 1e9, 0),
                   "speedup": round(t_e / t_f, 2)}
            print(json.dumps(row), flush=True)

    # cross entropy
    for B, K in ([(256, 1000), (512, 1000), (512, 32320)]
                 if "ce" in arms else []):
        logits = torch.randn(B, K, device=dev, dtype=dt,
                             requires_grad=True)
        tgt = torch.randint(K, (B,), device=dev)
        t_f = timeit(lambda: NF.cross_entropy(logits, tgt,
                                              backend="native"),
                     args.iters, args.warmup)
        t_e = timeit(lambda: torch.nn.functional.cross_entropy(
            logits, tgt), args.iters, args.warmup)
        print(json.dumps({"op": "cross_entropy_fwd",
                          "shape": f"{B}x{K}",
                          "fused_ms": round(t_f * 1e3, 4),
                          "eager_ms": round(t_e * 1e3, 4),
                          "speedup": round(t_e / t_f, 2)}), flush=True)

    if "ls_ce" in arms:
        bench_ls_ce(dev, args.iters, args.warmup)

    if "attn" in arms:
        bench_attn(dev, args.iters, args.warmup)

    if "lstm" in arms:
        bench_lstm(dev, args.iters, args.warmup)

    if "sgd" not in arms:
        return
    # fused SGD on resnet50-sized param set
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops.sgd import FusedSGD
    m = build_model("imagenet", "resnet50").to(dev).to(dt)
    for p_ in m.parameters():
        p_.grad = torch.randn_like(p_)
    o_f = FusedSGD(m.parameters(), lr=0.1, momentum=0.9,
                   weight_decay=1e-4, backend="native")
    t_f = timeit(o_f.step, args.iters, args.warmup)
    m2 = build_model("imagenet", "resnet50").to(dev).to(dt)
    for p_ in m2.parameters():
        p_.grad = torch.randn_like(p_)
    o_e = torch.optim.SGD(m2.parameters(), lr=0.1, momentum=0.9,
                          weight_decay=1e-4)
    t_e = timeit(o_e.step, args.iters, args.warmup)
    print(json.dumps({"op": "sgd_step_resnet50",
                      "fused_ms": round(t_f * 1e3, 3),
                      "eager_ms": round(t_e * 1e3, 3),
                      "speedup": round(t_e / t_f, 2)}), flush=True)


if __name__ == "__main__":
    main()
