#!/usr/bin/env python3
"""bf16 Linear: the native MFMA kernels (csrc/linear.hip) against the
library GEMM at the dense layers the models run.

Per shape and direction the native and library arms alternate in rounds in
one process; every arm is warmed before it is timed, a timed window is
`iters` calls between two device events, and the lowest window of each arm
is reported. Directions: fwd (y = x W^T + b), dgrad (dx = dy W), wgrad
(dW = dy^T x and db = sum dy) and fwd+bwd through autograd (NF.linear
backend="native" against F.linear). TFLOP/s is 2*M*N*K over the time (three
times that for fwd+bwd). One JSON line per row; there is no CPU path."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# GNMT rows: M = Ttgt * B of run_gnmt's defaults (max_len 50, batch 64)
GNMT_M = 50 * 64
# (layer, M, K, N)
SHAPES = [
    ("gnmt classifier", GNMT_M, 1024, 32320),
    ("lstm input projection", GNMT_M, 1024, 4096),
    ("lstm input projection (attn-fed)", GNMT_M, 2048, 4096),
    ("attention linear_q/k", GNMT_M, 1024, 1024),
    ("resnet50 head", 256, 2048, 1000),
    ("vgg fc1", 256, 25088, 4096),
    ("vgg fc2", 256, 4096, 4096),
]


def event_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("linear_bench needs the GPU: there is nothing to time "
                 "without one")
    from ddlbench_amd.ops import functional as NF, require_extension
    ext = require_extension()
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    for layer, M, K, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(M + N)
        mk = lambda *s: torch.randn(*s, device=dev, dtype=bf, generator=g)
        x, w, b, dy = mk(M, K), mk(N, K) * 0.03, mk(N), mk(M, N)
        xg = x.clone().requires_grad_(True)
        wg = w.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True)

        def train(fn):
            xg.grad = wg.grad = bg.grad = None
            fn(xg, wg, bg).backward(dy)

        arms = {
            "fwd": (lambda: ext.linear_fwd(x, w, b),
                    lambda: F.linear(x, w, b)),
            "dgrad": (lambda: ext.linear_dgrad(dy, w),
                      lambda: torch.mm(dy, w)),
            "wgrad": (lambda: ext.linear_wgrad(dy, x, True, bf),
                      lambda: (torch.mm(dy.t(), x), dy.sum(0))),
            "fwd+bwd": (lambda: train(lambda *a: NF.linear(
                            *a, backend="native")),
                        lambda: train(F.linear)),
        }
        plan = ext.linear_plan(M, N, K)
        for direction, fns in arms.items():
            times = {"native": [], "library": []}
            for _ in range(args.rounds):
                for arm, fn in zip(times, fns):
                    times[arm].append(event_ms(fn, args.iters, args.warmup))
            best = {a: min(v) for a, v in times.items()}
            flop = 2.0 * M * N * K * (3 if direction == "fwd+bwd" else 1)
            row = {"op": "linear", "layer": layer, "M": M, "K": K, "N": N,
                   "direction": direction,
                   "native_ms": round(best["native"], 4),
                   "library_ms": round(best["library"], 4),
                   "ratio": round(best["native"] / best["library"], 2),
                   "native_tflops": round(flop / best["native"] / 1e9, 1),
                   "library_tflops": round(flop / best["library"] / 1e9, 1)}
            if direction in plan:
                row["plan"] = plan[direction]
            print(json.dumps(row), flush=True)
        del x, w, b, dy, xg, wg, bg, arms


if __name__ == "__main__":
    main()
