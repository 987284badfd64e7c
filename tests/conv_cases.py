"""Case table and helpers of the exact-arithmetic conv tests
(test_conv_exact_gpu.py on the GPU, test_conv_cases_cpu.py without one).

Lattice inputs: x, w and dy are integers in [-3, 3] stored as bf16, each
tensor optionally scaled by a power of two. Every bf16 x bf16 product is
then exact in fp32 and every partial sum is (a power of two times) an
integer of magnitude <= 9*Kd or 9*P, below 2^24 — so an fp32 accumulator
is exact in ANY summation order, tile shape, split or atomic order, and
the kernels' outputs must equal the float64 reference bit for bit:
    fwd y, dgrad dx == ref64.to(bfloat16)   (one round-to-nearest-even)
    wgrad dw (fp32) == ref64.float()

Each case names, as coverage tags, the dispatch paths it claims to reach;
``reached`` derives the tags a case really reaches from the launchers' own
plan functions (ext.conv_igemm_plan / ext.conv_wgrad_plan), and
``REQUIRED`` is the list the union of all cases has to cover. A retune of
the dispatch that silently un-covers a path fails those assertions."""

import collections
import functools
import os

import torch
import torch.nn.functional as F

# shape = (N, C, H, W, K, R, stride, pad); passes out of fwd/dgrad/wgrad;
# scale = power-of-two exponents of (x, w, dy); claims = coverage tags
Case = collections.namedtuple("Case", "name shape passes scale claims")

ALL = ("fwd", "dgrad", "wgrad")
WG = ("wgrad",)

CASES = [
    # premise check: one K-step, one tile, unscaled — runs first
    Case("tiny_1x1", (1, 8, 4, 5, 8, 1, 1, 0), ALL, (0, 0, 0),
         ("declined:m0:128x64", "declined:m1:128x64", "Nd=8", "N=1",
          "M<tile", "v1:ksteps=1", "geom:R1s1p0", "OH*OW<32",
          "wgrad:64/64:r1", "wgrad:split1:1step")),
    # ---- v2 declined (Nd < 48): the 128-tile structure's narrow tiles
    Case("c40_3x3_p1", (2, 40, 9, 13, 40, 3, 1, 1), ALL, (-1, 1, 0),
         ("declined:m0:128x64", "declined:m1:128x64", "Nd=40",
          "geom:R3s1p1:HneW", "wgrad:psb==1")),
    Case("c40_3x3_p0", (3, 40, 11, 13, 40, 3, 1, 0), ALL, (1, -2, 1),
         ("declined:m0:256x64", "declined:m1:256x64", "Nd=40",
          "geom:R3s1p0:HneW")),
    # ---- v2 256x64 / 128x128, LIN and gather, K-step counts and tails
    Case("k48_c104_1x1", (2, 104, 7, 9, 48, 1, 1, 0), ALL, (0, -1, 2),
         ("v2:m0:256x64:lin", "v2:m1:128x128:lin", "Nd=48", "Nd=104",
          "v2:ksteps=2", "v2:ksteps=1", "v2:fwd:Kd%32=8",
          "v2:dgrad:Kd%32=16", "v1:m0:128x64", "v1:m1:128x128")),
    Case("k56_c56_3x3", (2, 56, 9, 13, 56, 3, 1, 1), ALL, (-2, 0, 1),
         ("v2:m0:256x64:gather", "v2:m1:256x64:gather", "Nd=56",
          "v2:fwd:Kd%32=24", "v2:dgrad:Kd%32=24")),
    Case("k96_c64_1x1", (5, 64, 9, 11, 96, 1, 1, 0), ALL, (1, 1, -3),
         ("v2:m0:128x128:lin", "v2:m1:256x64:lin", "Nd=96", "Nd=64",
          "v2:ksteps=1", "v2:ksteps=2", "M:multi-ragged",
          "v1:m0:128x128", "v1:m1:256x64")),
    Case("k136_c104_3x3", (2, 104, 9, 13, 136, 3, 1, 1), ALL, (0, 2, -1),
         ("v2:m0:128x128:gather", "v2:m1:128x128:gather", "Nd=136",
          "Nd=104", "v2:fwd:Kd%32=8", "v2:dgrad:Kd%32=8")),
    Case("k48_c136_1x1", (2, 136, 5, 6, 48, 1, 1, 0), ALL, (2, -1, 0),
         ("v2:ksteps=3", "v1:ksteps=3", "Nd=136", "Nd=48", "OH*OW<32")),
    Case("long_kd", (1, 256, 5, 7, 288, 3, 1, 1), ALL, (-1, -1, 1),
         ("Kd>=2304", "Nd>=256", "N=1", "M<tile")),
    # ---- stride 2: parity classes (MODE 2) at v2 and v1 widths
    Case("s2_c80_3x3_p1", (2, 80, 9, 12, 64, 3, 2, 1), ALL, (0, 1, -2),
         ("v2:m2:256x64", "v1:m2:128x128", "v2:fwd:Kd%32=16", "Nd=64",
          "geom:R3s2p1:HneW", "s2:H-odd", "s2:W-even")),
    Case("s2_c96_3x3_p0", (2, 96, 10, 13, 48, 3, 2, 0), ALL, (1, 0, 0),
         ("v2:m2:128x128", "Nd=96", "geom:R3s2p0:HneW", "s2:H-even",
          "s2:W-odd")),
    Case("s2_c64_1x1", (2, 64, 9, 12, 128, 1, 2, 0), ALL, (-1, 2, 1),
         ("v2:m2:256x64", "v1:m2:128x64", "geom:R1s2p0")),
    Case("s2_c16_3x3", (4, 16, 17, 19, 24, 3, 2, 1), ALL, (0, -3, 2),
         ("declined:m2:256x64", "v1:m2:256x64", "v1:m0:256x64")),
    Case("s2_c24_5x5_p2", (1, 24, 7, 6, 32, 5, 2, 2), ALL, (2, 0, -1),
         ("declined:m2:128x64", "geom:R5s2p2:HneW", "OW in {2,3}",
          "OH*OW<32", "N=1")),
    # stride 3 has no parity split: the gather dgrad stays on the
    # 128-tile structure at any width
    Case("s3_c72_3x3", (2, 72, 10, 11, 16, 3, 3, 1), ALL, (0, 0, 1),
         ("declined:m1:128x128", "geom:R3s3p1:HneW")),
    # ---- 5x5 and pad 2
    Case("k64_c48_5x5_p2", (2, 48, 9, 13, 64, 5, 1, 2), ALL, (-1, 0, -1),
         ("geom:R5s1p2:HneW", "v2:fwd:Kd%32=16", "Nd=48", "Nd=64")),
    Case("c32_5x5_p0", (2, 32, 9, 13, 40, 5, 1, 0), ALL, (1, -1, 0),
         ("geom:R5s1p0:HneW",)),
    Case("c40_5x5_p1", (2, 40, 8, 11, 32, 5, 1, 1), ALL, (0, 1, 1),
         ("geom:R5s1p1:HneW",)),
    Case("c24_3x3_p2", (2, 24, 6, 7, 40, 3, 1, 2), ALL, (-2, 2, 0),
         ("geom:R3s1p2:HneW",)),
    # ---- weight-grad steady state: >= 4 steps per chunk with a ragged
    # last step, every tile x {r1, gather}. The 256 cap on split puts the
    # small tiles' steady state at P ~ 50 000 — the smallest such shapes.
    Case("wg_64x64_r1", (4, 64, 112, 113, 64, 1, 1, 0), WG, (0, 0, 0),
         ("wgrad:64/64:r1:steady", "wgrad:psb>1")),
    Case("wg_64x64_gather", (4, 8, 112, 127, 64, 3, 1, 1), WG, (1, 0, -1),
         ("wgrad:64/64:gather:steady", "wgrad:OW>64")),
    Case("wg_64x128_r1", (4, 128, 112, 115, 64, 1, 1, 0), WG, (0, 0, 1),
         ("wgrad:64/128:r1:steady",)),
    Case("wg_64x128_gather", (4, 16, 112, 140, 64, 3, 1, 1), WG, (-1, 0, 0),
         ("wgrad:64/128:gather:steady",)),
    Case("wg_128x64_r1", (4, 64, 112, 130, 128, 1, 1, 0), WG, (1, 0, 0),
         ("wgrad:128/64:r1:steady",)),
    Case("wg_128x64_gather", (4, 8, 112, 120, 128, 3, 1, 1), WG, (0, 0, -2),
         ("wgrad:128/64:gather:steady",)),
    Case("wg_128x128_r1", (4, 128, 112, 113, 128, 1, 1, 0), WG, (0, 0, 0),
         ("wgrad:128/128:r1:steady",)),
    Case("wg_128x128_gather", (4, 16, 112, 135, 128, 3, 1, 1), WG,
         (-1, 0, 1), ("wgrad:128/128:gather:steady",)),
    Case("wg_s2_gather", (4, 8, 223, 225, 64, 3, 2, 1), WG, (0, 0, 0),
         ("wgrad:s2-gather:steps>=4", "wgrad:OW>64")),
    # 30 output pixels per image: every 64-pixel advance of the carry
    # chain crosses two or three images
    Case("wg_multi_image", (1650, 8, 5, 6, 64, 3, 1, 1), WG, (1, 0, 1),
         ("wgrad:gather:multi-image-advance", "wgrad:64/64:gather:steady")),
    # K*RSC > 4M floats: the slab workspace holds one copy, so split == 1
    # and the single chunk walks all of P, straight into dw
    Case("wg_split1_multistep", (7, 512, 5, 6, 1024, 3, 1, 1), WG,
         (0, 0, 0), ("wgrad:split1:multistep",
                     "wgrad:gather:multi-image-advance")),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# (R, stride, pad) classes the case table promises: the seven of the model
# zoo first (test_conv_cases_cpu.py re-derives them from the models), then
# 3x3 and 5x5 at the remaining pads, 5x5 stride 2 and stride 3
_GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 2, 0),
          (5, 1, 2), (3, 1, 2), (5, 1, 0), (5, 1, 1), (5, 2, 2), (3, 3, 1)]

REQUIRED = sorted(set(
    # every instantiation the fwd/dgrad dispatch can select
    [f"v2:m{m}:{t}:{a}" for m in (0, 1) for t in ("128x128", "256x64")
     for a in ("lin", "gather")]
    + [f"v2:m2:{t}" for t in ("128x128", "256x64")]
    + [f"v1:m{m}:{t}" for m in (0, 1, 2)
       for t in ("128x64", "256x64", "128x128")]
    # ... and the 128-tile structure as the default path's fallback
    + [f"declined:m{m}:{t}" for m in (0, 1, 2) for t in ("128x64", "256x64")]
    + ["declined:m1:128x128"]
    + ["M<tile", "M:multi-ragged", "N=1"]
    + [f"Nd={n}" for n in (8, 40, 48, 56, 64, 96, 104, 136)] + ["Nd>=256"]
    + [f"{s}:ksteps={n}" for s in ("v1", "v2") for n in (1, 2, 3)]
    + [f"v2:{d}:Kd%32={r}" for d in ("fwd", "dgrad") for r in (8, 16, 24)]
    + ["Kd>=2304"]
    + [f"geom:R{r}s{s}p{p}" for r, s, p in _GEOMS]
    + [f"geom:R{r}s{s}p{p}:HneW" for r, s, p in _GEOMS if r > 1]
    + ["s2:H-even", "s2:H-odd", "s2:W-even", "s2:W-odd", "OW in {2,3}",
       "OH*OW<32"]
    + [f"wgrad:{t}:{b}{s}" for t in ("64/64", "64/128", "128/64", "128/128")
       for b in ("r1", "gather") for s in ("", ":steady")]
    + ["wgrad:psb>1", "wgrad:psb==1", "wgrad:split1:1step",
       "wgrad:split1:multistep", "wgrad:s2-gather:steps>=4",
       "wgrad:gather:multi-image-advance", "wgrad:OW>64"]))


def out_hw(shape):
    N, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def geometry(shape):
    return shape[5], shape[6], shape[7]


# ------------------------------------------------------------ lattice data
def lattice(shape, generator, exp=0):
    """Integers in [-3, 3] (1/7 of them zero) times 2^exp, as bf16."""
    t = torch.randint(-3, 4, shape, generator=generator).to(torch.float32)
    return (t * 2.0 ** exp).to(torch.bfloat16)


def check_sum_guard(case):
    """9 * max(Kd, P) * scale < 2^24 for every pass the case runs: the
    integer partial sums (times the power-of-two scale) stay exactly
    representable in the fp32 accumulator."""
    N, C, H, W, K, R, stride, pad = case.shape
    OH, OW = out_hw(case.shape)
    sx, sw, sdy = case.scale
    depth = {"fwd": (R * R * C, sx + sw), "dgrad": (R * R * K, sdy + sw),
             "wgrad": (N * OH * OW, sx + sdy)}
    for ps in case.passes:
        n, e = depth[ps]
        assert 9 * n * max(2.0 ** e, 1.0) < 2 ** 24, (case.name, ps, n, e)


def reference64(x, w, dy, stride, pad, need=ALL):
    """float64 F.conv2d and its autograd on the CPU from the bf16 values;
    only the gradients in ``need`` are computed."""
    x64 = x.double().requires_grad_("dgrad" in need)
    w64 = w.double().requires_grad_("wgrad" in need)
    y64 = F.conv2d(x64, w64, None, stride, pad)
    if x64.requires_grad or w64.requires_grad:
        y64.backward(dy.double())
    return {"y": y64.detach(), "dx": x64.grad, "dw": w64.grad}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Seeded lattice inputs (CPU, bf16) and the float64 reference of one
    case; computed once and shared read-only between the tests."""
    case = CASE_BY_NAME[name]
    check_sum_guard(case)
    N, C, H, W, K, R, stride, pad = case.shape
    OH, OW = out_hw(case.shape)
    sx, sw, sdy = case.scale
    g = torch.Generator().manual_seed(20240 + CASES.index(case))
    x = lattice((N, C, H, W), g, sx)
    w = lattice((K, C, R, R), g, sw)
    dy = lattice((N, K, OH, OW), g, sdy)
    d = {"x": x, "w": w, "dy": dy}
    d.update(reference64(x, w, dy, stride, pad, case.passes))
    return d


def exact_mismatches(got, ref64, dtype):
    """Number of elements of ``got`` that differ from the float64
    reference rounded once to ``dtype`` — the tests assert 0."""
    want = ref64.to(dtype)
    assert got.dtype == dtype and got.shape == want.shape, \
        (got.dtype, tuple(got.shape), tuple(want.shape))
    return int((got.cpu() != want).sum().item())


# ------------------------------------------------------- plans -> coverage
def igemm_plans(ext, shape, dgrad, v2):
    """ext.conv_igemm_plan under DDLB_CONV_V2 = v2 ("1" or "0")."""
    N, C, H, W, K, R, stride, pad = shape
    old = os.environ.get("DDLB_CONV_V2")
    os.environ["DDLB_CONV_V2"] = v2
    try:
        return ext.conv_igemm_plan(N, C, H, W, K, R, R, stride, pad, dgrad)
    finally:
        if old is None:
            del os.environ["DDLB_CONV_V2"]
        else:
            os.environ["DDLB_CONV_V2"] = old


def wgrad_plan(ext, shape):
    N, C, H, W, K, R, stride, pad = shape
    return ext.conv_wgrad_plan(N, C, H, W, K, R, R, stride, pad)


def reached(ext, case):
    """Coverage tags the case reaches, from the launchers' own plans."""
    N, C, H, W, K, R, stride, pad = case.shape
    OH, OW = out_hw(case.shape)
    tags = set()
    for ps in ("fwd", "dgrad"):
        if ps not in case.passes:
            continue
        for v2 in ("1", "0"):
            for e in igemm_plans(ext, case.shape, ps == "dgrad", v2):
                tile = f"{e['BM']}x{e['BN']}"
                st = e["structure"]
                if st == "v2":
                    tags.add(f"v2:m{e['mode']}:{tile}" + (
                        "" if e["mode"] == 2 else
                        ":lin" if e["LIN"] else ":gather"))
                    if e["Kd"] % 32:
                        tags.add(f"v2:{ps}:Kd%32={e['Kd'] % 32}")
                else:
                    assert not e["LIN"]
                    tags.add(("declined" if v2 == "1" else "v1")
                             + f":m{e['mode']}:{tile}")
                ksteps = -(-e["Kd"] // 64)
                if ksteps <= 3:
                    tags.add(f"{st}:ksteps={ksteps}")
                if e["Kd"] >= 2304:
                    tags.add("Kd>=2304")
                if e["M"] < e["BM"]:
                    tags.add("M<tile")
                if -(-e["M"] // e["BM"]) >= 3 and e["M"] % e["BM"]:
                    tags.add("M:multi-ragged")
                tags.add("Nd>=256" if e["Nd"] >= 256 else f"Nd={e['Nd']}")
        if N == 1:
            tags.add("N=1")
        geom = f"geom:R{R}s{stride}p{pad}"
        tags.add(geom)
        if H != W:
            tags.add(geom + ":HneW")
        if stride == 2:
            tags.add("s2:H-" + ("odd" if H % 2 else "even"))
            tags.add("s2:W-" + ("odd" if W % 2 else "even"))
        if OW in (2, 3):
            tags.add("OW in {2,3}")
        if OH * OW < 32:
            tags.add("OH*OW<32")
    if "wgrad" in case.passes:
        pl = wgrad_plan(ext, case.shape)
        kind = "r1" if pl["r1"] else "gather"
        tile = f"wgrad:{pl['TK']}/{pl['TR']}:{kind}"
        assert pl["ring"] == (2 if (pl["TK"], pl["TR"]) == (128, 128) else 3)
        tags.add(tile)
        if pl["steps"] >= 4 and pl["tail"] != 64:
            tags.add(tile + ":steady")
        if pl["psb"] > 1:
            tags.add("wgrad:psb>1")
        elif pl["psb"] == 1:
            tags.add("wgrad:psb==1")
        else:
            assert pl["split"] == 1
            tags.add("wgrad:split1:1step" if pl["steps"] == 1
                     else "wgrad:split1:multistep")
        if kind == "gather":
            if stride == 2 and pl["steps"] >= 4:
                tags.add("wgrad:s2-gather:steps>=4")
            if OH * OW < 64 and N >= 4 and pl["steps"] >= 2:
                tags.add("wgrad:gather:multi-image-advance")
            if OW > 64:
                tags.add("wgrad:OW>64")
    return tags


def check_claims(ext):
    """Every case reaches what it claims; returns the union reached."""
    union = set()
    for case in CASES:
        got = reached(ext, case)
        missing = set(case.claims) - got
        assert not missing, f"{case.name} no longer reaches {sorted(missing)}"
        union |= got
    return union
