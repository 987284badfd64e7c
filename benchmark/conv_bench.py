#!/usr/bin/env python3
"""Per-shape conv microbenchmark: MFMA implicit-GEMM kernel vs MIOpen.

Times forward and data-grad over the ResNet-50 layer shapes (bf16,
channels_last) and prints one JSON line per shape with ms and effective
TFLOP/s for both backends — the measurement that drives the conv
dispatch policy.

Each row also carries the residual-join columns: ``mfma2_dgrad_add_ms``
is the data-grad with the shortcut's gradient summed in its epilogue
(``conv_igemm_dgrad(..., add=g)``), ``mfma2_dgrad_add_gated_ms`` the same
with the addend gated by a 1-bit mask (``gate=m``),
``mfma2_dgrad_then_add_ms`` the plain data-grad followed by the torch bf16
add it replaces. ``--join`` prints
only those (plus the plain data-grad) per shape.

``--stem`` instead times the small-C stem convs the model zoo builds
(native csrc/conv_stem.hip vs the library), forward and weight-grad."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import torch  # noqa: E402

# (C, H/W, K, R, stride) — ResNet-50 body at 224^2 (stem excluded: C=3)
RESNET50_SHAPES = [
    (64, 56, 64, 1, 1), (64, 56, 64, 3, 1), (64, 56, 256, 1, 1),
    (256, 56, 64, 1, 1), (256, 56, 128, 1, 1), (128, 56, 128, 3, 2),
    (128, 28, 512, 1, 1), (512, 28, 128, 1, 1), (512, 28, 256, 1, 1),
    (256, 28, 256, 3, 2), (256, 14, 1024, 1, 1), (1024, 14, 256, 1, 1),
    (1024, 14, 512, 1, 1), (512, 14, 512, 3, 2), (512, 7, 2048, 1, 1),
    (2048, 7, 512, 1, 1),
]


def bench_op(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# HBM peak used for the byte-bound floor of the stem rows (MI355X, TB/s)
HBM_TBS = 8.0


def stem_shapes(batch):
    """(dataset, arch, batch, conv, H, W) for every distinct stem the model
    zoo builds, read off the models themselves."""
    import torch.nn as nn
    from ddlbench_amd.config import DATASET_SHAPES
    from ddlbench_amd.models import build_model
    from ddlbench_amd.ops.conv import stem_eligible
    seen, out = set(), []
    for dataset, n in (("imagenet", batch), ("highres", 32),
                       ("cifar10", batch), ("mnist", batch)):
        _, H, W = DATASET_SHAPES[dataset][:3]
        for arch in ("resnet50", "vgg16", "mobilenetv2"):
            model = build_model(dataset, arch)
            conv = next(m for m in model.modules()
                        if isinstance(m, nn.Conv2d))
            if not stem_eligible(conv):
                continue
            key = (dataset, conv.in_channels, conv.out_channels,
                   conv.kernel_size, conv.stride, conv.padding)
            if key not in seen:
                seen.add(key)
                out.append((dataset, arch, n, conv, H, W))
    return out


def bench_stem(args):
    from ddlbench_amd.ops import require_extension
    ext = require_extension()
    dev = torch.device("cuda", 0)
    cl = torch.channels_last
    for dataset, arch, N, conv, H, W in stem_shapes(args.batch):
        C, K, R = conv.in_channels, conv.out_channels, conv.kernel_size[0]
        stride, pad = conv.stride[0], conv.padding[0]
        x = torch.randn(N, C, H, W, device=dev,
                        dtype=torch.bfloat16).contiguous(memory_format=cl)
        w = torch.randn(K, C, R, R, device=dev,
                        dtype=torch.bfloat16).contiguous(memory_format=cl)
        OH = (H + 2 * pad - R) // stride + 1
        OW = (W + 2 * pad - R) // stride + 1
        dy = torch.randn(N, K, OH, OW, device=dev,
                         dtype=torch.bfloat16).contiguous(memory_format=cl)
        fns = {
            "native_fwd": lambda: ext.conv_stem_fwd(x, w, stride, pad),
            "library_fwd": lambda: torch.nn.functional.conv2d(
                x, w, None, stride, pad),
            "native_wgrad": lambda: ext.conv_stem_wgrad(
                x, dy, R, R, stride, pad),
            "library_wgrad": lambda: torch.ops.aten.convolution_backward(
                dy, x, w, None, [stride, stride], [pad, pad], [1, 1],
                False, [0, 0], 1, [False, True, False]),
        }
        res = {"dataset": dataset, "arch": arch,
               "shape": f"C{C}_H{H}_W{W}_K{K}_R{R}_s{stride}_p{pad}",
               "batch": N}
        # native and library alternate; two passes, the lower time counts
        best = {}
        for _ in range(2):
            for name, fn in fns.items():
                t = bench_op(fn, args.iters, args.warmup)
                best[name] = min(best.get(name, t), t)
        for name, t in best.items():
            res[name + "_ms"] = round(t * 1e3, 4)
        # byte-bound floors: fwd x + w + y, wgrad x + dy
        fwd_b = 2 * (x.numel() + w.numel() + dy.numel())
        wg_b = 2 * (x.numel() + dy.numel())
        res["fwd_floor_ms"] = round(fwd_b / (HBM_TBS * 1e12) * 1e3, 4)
        res["wgrad_floor_ms"] = round(wg_b / (HBM_TBS * 1e12) * 1e3, 4)
        res["fwd_floor_share"] = round(
            fwd_b / (HBM_TBS * 1e12) / best["native_fwd"], 3)
        res["wgrad_floor_share"] = round(
            wg_b / (HBM_TBS * 1e12) / best["native_wgrad"], 3)
        print(json.dumps(res), flush=True)


def join_columns(ext, dy, w_perm, x, stride, pad, args):
    """dgrad+add: fused epilogue addend vs dgrad followed by a torch add
    (deep-pipeline structure; g stands in for the shortcut's gradient)."""
    N, C, H, W = x.shape
    g = torch.randn_like(x)
    m = torch.randint(0, 256, (x.numel() // 8,), device=x.device,
                      dtype=torch.uint8)
    os.environ["DDLB_CONV_V2"] = "1"
    fns = {
        "mfma2_dgrad_add_ms": lambda: ext.conv_igemm_dgrad(
            dy, w_perm, N, C, H, W, stride, pad, add=g),
        # the addend gated by a 1-bit mask in the same epilogue
        "mfma2_dgrad_add_gated_ms": lambda: ext.conv_igemm_dgrad(
            dy, w_perm, N, C, H, W, stride, pad, add=g, gate=m),
        "mfma2_dgrad_then_add_ms": lambda: ext.conv_igemm_dgrad(
            dy, w_perm, N, C, H, W, stride, pad) + g,
    }
    # the two alternate; two passes, the lower time counts
    best = {}
    for _ in range(2):
        for name, fn in fns.items():
            t = bench_op(fn, args.iters, args.warmup)
            best[name] = min(best.get(name, t), t)
    return {k: round(t * 1e3, 3) for k, t in best.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--stem", action="store_true",
                   help="time the model zoo's stem convs (native vs "
                        "library, forward and weight-grad) instead")
    p.add_argument("--join", action="store_true",
                   help="per shape, only the data-grad and the dgrad+add "
                        "columns (fused addend vs dgrad then torch add)")
    args = p.parse_args()
    assert torch.cuda.is_available()
    torch.backends.cudnn.benchmark = True
    if args.stem:
        bench_stem(args)
        return
    from ddlbench_amd.ops.conv import conv2d_mfma
    dev = torch.device("cuda", 0)
    cl = torch.channels_last

    for C, HW, K, R, stride in RESNET50_SHAPES:
        pad = (R - 1) // 2
        N = args.batch
        x = torch.randn(N, C, HW, HW, device=dev,
                        dtype=torch.bfloat16).contiguous(memory_format=cl)
        w = torch.randn(K, C, R, R, device=dev,
                        dtype=torch.bfloat16).contiguous(memory_format=cl)
        OH = (HW + 2 * pad - R) // stride + 1
        flops = 2.0 * N * OH * OH * K * C * R * R
        dy = torch.randn(N, K, OH, OH, device=dev,
                         dtype=torch.bfloat16).contiguous(memory_format=cl)
        w_perm = w.permute(1, 2, 3, 0).contiguous()

        from ddlbench_amd.ops import require_extension
        ext = require_extension()
        res = {"shape": f"C{C}_HW{HW}_K{K}_R{R}_s{stride}",
               "batch": N}
        if args.join:
            os.environ["DDLB_CONV_V2"] = "1"
            t = bench_op(lambda: ext.conv_igemm_dgrad(
                dy, w_perm, N, C, HW, HW, stride, pad),
                args.iters, args.warmup)
            res["mfma2_dgrad_ms"] = round(t * 1e3, 3)
            res.update(join_columns(ext, dy, w_perm, x, stride, pad, args))
            print(json.dumps(res), flush=True)
            continue
        # forward: v2 (deep pipeline, default), v1 (128-tile), MIOpen
        os.environ["DDLB_CONV_V2"] = "1"
        t = bench_op(lambda: ext.conv_igemm_fwd(x, w, stride, pad),
                     args.iters, args.warmup)
        res["mfma2_fwd_ms"] = round(t * 1e3, 3)
        res["mfma2_fwd_tf"] = round(flops / t / 1e12, 1)
        os.environ["DDLB_CONV_V2"] = "0"
        t = bench_op(lambda: ext.conv_igemm_fwd(x, w, stride, pad),
                     args.iters, args.warmup)
        res["mfma_fwd_ms"] = round(t * 1e3, 3)
        res["mfma_fwd_tf"] = round(flops / t / 1e12, 1)
        t = bench_op(lambda: torch.nn.functional.conv2d(
            x, w, None, stride, pad), args.iters, args.warmup)
        res["miopen_fwd_ms"] = round(t * 1e3, 3)
        res["miopen_fwd_tf"] = round(flops / t / 1e12, 1)
        # dgrad
        os.environ["DDLB_CONV_V2"] = "1"
        t = bench_op(lambda: ext.conv_igemm_dgrad(
            dy, w_perm, N, C, HW, HW, stride, pad),
            args.iters, args.warmup)
        res["mfma2_dgrad_ms"] = round(t * 1e3, 3)
        res["mfma2_dgrad_tf"] = round(flops / t / 1e12, 1)
        os.environ["DDLB_CONV_V2"] = "0"
        t = bench_op(lambda: ext.conv_igemm_dgrad(
            dy, w_perm, N, C, HW, HW, stride, pad),
            args.iters, args.warmup)
        res["mfma_dgrad_ms"] = round(t * 1e3, 3)
        res["mfma_dgrad_tf"] = round(flops / t / 1e12, 1)
        os.environ["DDLB_CONV_V2"] = "1"
        t = bench_op(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, [stride, stride], [pad, pad], [1, 1], False,
            [0, 0], 1, [True, False, False]), args.iters, args.warmup)
        res["miopen_dgrad_ms"] = round(t * 1e3, 3)
        res["miopen_dgrad_tf"] = round(flops / t / 1e12, 1)
        res.update(join_columns(ext, dy, w_perm, x, stride, pad, args))
        # wgrad: the transpose-read kernel (key name kept from the rows
        # that also timed the retired scalar-gather kernel as mfma_wgrad)
        t = bench_op(lambda: ext.conv_igemm_wgrad(x, dy, R, R, stride,
                                                  pad),
                     args.iters, args.warmup)
        res["mfma2_wgrad_ms"] = round(t * 1e3, 3)
        res["mfma2_wgrad_tf"] = round(flops / t / 1e12, 1)
        t = bench_op(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, [stride, stride], [pad, pad], [1, 1], False,
            [0, 0], 1, [False, True, False]), args.iters, args.warmup)
        res["miopen_wgrad_ms"] = round(t * 1e3, 3)
        res["miopen_wgrad_tf"] = round(flops / t / 1e12, 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
