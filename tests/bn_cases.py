"""Case table and helpers of the BN+act dispatch-path tests
(test_bn_paths_gpu.py on the GPU, test_bn_plan_cpu.py without one).

Which kernel a BN+act layer reaches is decided by one host function,
``ext.bn_plan`` — the function the launchers walk. Each case names, as
coverage tags, the plan kinds it was chosen for; ``reached`` derives the
tags a case really reaches from the plan, and ``REQUIRED`` is the list the
union of all cases has to cover. A retune that silently un-covers a path
fails those assertions.

Every case also runs with act = none on integer inputs (the exactness
test), so the act-none plan of its shape counts towards its tags.

Two data sets per case: ``case_inputs`` (seeded normal data, compared with
float64 at a tolerance) and ``dyadic_inputs`` (data on which the whole
computation is exact in fp32 and bf16 in any summation order, compared bit
for bit; tests/test_bn_cases_cpu.py proves that property on the CPU).

The shapes are the smallest that reach each path:
  rows = N*H*W >= 32768 switches apply/dx to the fixed-channel kernels
  (as does a mask to write or read); C <= 512 with C % 8 == 0 selects the
  8-wide bf16 reduce; C % 8 != 0 (NHWC) or HW % 8 != 0 (NCHW) the scalar
  elementwise kernels; S > 32 slab rows a finalize hand-off (Y > 1)."""

import collections
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
MOM = 0.1
ACT = {"none": 0, "relu": 1, "relu6": 2}

# bwd: gate sources the backward runs with, out of "mask" (the forward's
# 1-bit mask, y withheld) and "y"
Case = collections.namedtuple(
    "Case", "name dtype nhwc shape act res training bwd claims")

BF, FP = torch.bfloat16, torch.float32

CASES = [
    # 1: the masked training path of the model zoo at its smallest
    Case("c8_relu_train", BF, True, (2, 8, 4, 4), "relu", False, True,
         ("mask", "y"),
         ("stats:nhwc_vec:bf16", "S=2", "fin:f32", "fin:Y=1",
          "apply:fixed_channel:mask", "bwd_reduce:nhwc_vec:bf16:mask",
          "dx:fixed_channel:mask", "bwd_reduce:nhwc_vec:bf16:y",
          "dx:vec:y")),
    # 2: no mask, rows < 32768: grid-stride vec apply and dx
    Case("c8_none_train", BF, True, (2, 8, 4, 4), "none", False, True,
         ("y",), ("apply:vec:nhwc:bf16", "dx:vec:nhwc:bf16", "dx:vec:none",
                  "bwd_reduce:nhwc_vec:bf16:none")),
    # 3: rows = 32768: fixed-channel apply/dx with nothing to gate
    Case("rows32k_none", BF, True, (8, 8, 64, 64), "none", False, True,
         ("y",), ("apply:fixed_channel:nomask", "apply:fixed_channel:act0",
                  "dx:fixed_channel:none", "fin:Y>1")),
    # 4: the same rows with relu: fixed-channel dx and vec reduce, gate
    # from y and from the mask
    Case("rows32k_relu", BF, True, (8, 8, 64, 64), "relu", False, True,
         ("y", "mask"),
         ("dx:fixed_channel:y", "dx:fixed_channel:mask",
          "bwd_reduce:nhwc_vec:bf16:y", "bwd_reduce:nhwc_vec:bf16:mask")),
    # 5: C > 512: scalar reduce, double slabs, 16 lane blocks; the
    # fixed-channel apply/dx grid has two lane blocks (C/8 = 128 lanes)
    Case("c1024_relu", BF, True, (4, 1024, 8, 8), "relu", False, True,
         ("mask", "y"),
         ("stats:nhwc_scalar:bf16", "fin:f64", "cblocks=16",
          "fixed:lane_blocks=2", "bwd_reduce:nhwc_scalar:bf16:mask",
          "bwd_reduce:nhwc_scalar:bf16:y")),
    Case("c1024_relu6", BF, True, (4, 1024, 8, 8), "relu6", False, True,
         ("mask",), ("bwd_reduce:nhwc_scalar:mask:act2",)),
    # 6: three 8-channel lanes per block (one idle thread), odd row count,
    # residual add and dres
    Case("c24_relu_res", BF, True, (3, 24, 5, 7), "relu", True, True,
         ("mask", "y"),
         ("apply:fixed_channel:add", "dx:fixed_channel:mask:add",
          "dx:vec:add", "rows:odd")),
    # 7: C % 8 != 0: scalar reduce, no mask, scalar apply/dx
    Case("c12_relu", BF, True, (2, 12, 4, 4), "relu", False, True,
         ("y",), ("stats:nhwc_scalar:bf16", "apply:scalar:nhwc:bf16",
                  "dx:scalar:nhwc:bf16", "dx:scalar:y")),
    Case("c12_relu6_res", BF, True, (2, 12, 4, 4), "relu6", True, True,
         ("y",), ("apply:scalar:act2", "apply:scalar:add", "dx:scalar:act2",
                  "dx:scalar:add", "bwd_reduce:nhwc_scalar:act2")),
    # 8: relu6 on the masked path; relu and relu6 in eval mode, backward
    # with y: the unmasked grid-stride kernels with an activation
    Case("c8_relu6_train", BF, True, (2, 8, 4, 4), "relu6", False, True,
         ("mask",), ("apply:fixed_channel:act2", "dx:fixed_channel:mask:act2",
                     "bwd_reduce:nhwc_vec:mask:act2")),
    Case("c8_relu_eval", BF, True, (2, 8, 4, 4), "relu", False, False,
         ("y",), ("apply:vec:act1", "dx:vec:act1", "dx:vec:y")),
    Case("c8_relu6_eval", BF, True, (2, 8, 4, 4), "relu6", False, False,
         ("y",), ("apply:vec:act2", "dx:vec:act2")),
    # 9: fp32 NHWC: scalar reduce with double slabs at any C
    Case("fp32_c24_relu", FP, True, (3, 24, 5, 7), "relu", False, True,
         ("y",), ("stats:nhwc_scalar:fp32", "apply:vec:nhwc:fp32",
                  "dx:vec:nhwc:fp32", "bwd_reduce:nhwc_scalar:fp32:y")),
    Case("fp32_c12_relu", FP, True, (2, 12, 4, 4), "relu", False, True,
         ("y",), ("apply:scalar:nhwc:fp32", "dx:scalar:nhwc:fp32")),
    # 10: NCHW, HW % 8 == 0 (vec) and HW = 196 (scalar), both dtypes
    Case("nchw_bf16_hw64", BF, False, (4, 16, 8, 8), "relu", False, True,
         ("y",), ("stats:nchw:bf16", "apply:vec:nchw:bf16",
                  "dx:vec:nchw:bf16", "bwd_reduce:nchw:bf16:y")),
    Case("nchw_fp32_hw64_res", FP, False, (4, 16, 8, 8), "relu", True, True,
         ("y",), ("stats:nchw:fp32", "apply:vec:nchw:fp32", "apply:vec:add",
                  "dx:vec:nchw:fp32", "dx:vec:add")),
    Case("nchw_fp32_hw64_relu6", FP, False, (4, 16, 8, 8), "relu6", False,
         True, ("y",), ("bwd_reduce:nchw:act2",)),
    Case("nchw_bf16_hw196_res", BF, False, (8, 32, 14, 14), "relu", True,
         True, ("y",), ("apply:scalar:nchw:bf16", "apply:scalar:add",
                        "dx:scalar:nchw:bf16", "dx:scalar:add")),
    Case("nchw_fp32_hw196", FP, False, (8, 32, 14, 14), "relu", False, True,
         ("y",), ("apply:scalar:nchw:fp32", "dx:scalar:nchw:fp32",
                  "bwd_reduce:nchw:fp32:y")),
    # finalize geometries (the shapes of test_bn_finalize_gpu.py)
    Case("fin_s2048", BF, True, (8, 64, 64, 64), "relu", False, True,
         ("mask",), ("S=2048", "fin:Y=64", "fin:f32")),
    Case("fin_s128_c512", BF, True, (8, 512, 16, 16), "relu", False, True,
         ("mask",), ("S=128", "fin:Y>1", "stats:nhwc_vec:bf16")),
    # edge geometries
    # rows = 1615, S = 100, 17 rows per slice: slices 95..99 start past the
    # last row in the reduce, the fixed-channel apply and its dx
    Case("empty_slices", BF, True, (5, 8, 17, 19), "relu", False, True,
         ("mask", "y"),
         ("slices:empty", "S=100", "rows:odd", "apply:fixed_channel:mask",
          "dx:fixed_channel:mask")),
    # one row: var = 0, the unbiased guard
    Case("count1_nhwc_bf16", BF, True, (1, 8, 1, 1), "relu", False, True,
         ("mask", "y"), ("count=1", "stats:nhwc_vec:bf16")),
    Case("count1_nchw_bf16", BF, False, (1, 8, 1, 1), "relu", False, True,
         ("y",), ("count=1", "stats:nchw:bf16")),
    Case("count1_nhwc_fp32", FP, True, (1, 8, 1, 1), "relu", False, True,
         ("y",), ("count=1", "stats:nhwc_scalar:fp32")),
    Case("count1_nchw_fp32", FP, False, (1, 8, 1, 1), "relu", False, True,
         ("y",), ("count=1", "stats:nchw:fp32")),
    # 3 rows against 128 row-groups
    Case("rows3_c16", BF, True, (1, 16, 1, 3), "relu", False, True,
         ("mask", "y"), ("rows<RG", "stats:nhwc_vec:bf16")),
    # C % 8 == 0 but > 512: scalar reduce reading the mask; 65 lanes = two
    # lane blocks of the fixed-channel grid, the second with one live lane
    Case("c520_relu", BF, True, (2, 520, 3, 3), "relu", False, True,
         ("mask", "y"),
         ("fixed:tail_lane_block", "fixed:lane_blocks=2",
          "bwd_reduce:nhwc_scalar:bf16:mask", "dx:fixed_channel:mask")),
    Case("c4_bf16", BF, True, (2, 4, 3, 3), "relu", False, True,
         ("y",), ("C<8", "apply:scalar:nhwc:bf16", "dx:scalar:nhwc:bf16")),
    Case("c4_fp32", FP, True, (2, 4, 3, 3), "relu", False, True,
         ("y",), ("C<8", "apply:scalar:nhwc:fp32", "dx:scalar:nhwc:fp32")),
    # HW = 1: every element its own (n, c)
    Case("nchw_hw1", BF, False, (16, 8, 1, 1), "relu", False, True,
         ("y",), ("nchw:hw1", "apply:scalar:nchw:bf16")),
    # eval beyond the small NHWC vec kernels: fixed-channel apply with an
    # act and no mask, fixed-channel dx with k2 = k3 = 0; NCHW vec, scalar
    Case("rows32k_relu_eval", BF, True, (8, 8, 64, 64), "relu", False, False,
         ("y",), ("eval:fixed_channel", "apply:fixed_channel:nomask",
                  "apply:fixed_channel:act1", "dx:fixed_channel:y")),
    Case("nchw_fp32_hw64_relu6_eval", FP, False, (4, 16, 8, 8), "relu6",
         False, False, ("y",), ("eval:nchw", "eval:nchw:vec")),
    Case("nchw_bf16_hw196_eval", BF, False, (8, 32, 14, 14), "relu", False,
         False, ("y",), ("eval:nchw", "eval:nchw:scalar")),
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# cases of the masked-vs-unmasked bit-for-bit cross-check (relu only)
CROSS_CHECK = ("c8_relu_train", "rows32k_relu", "c1024_relu", "c24_relu_res",
               "empty_slices", "c520_relu")

_REDUCES = [("nchw", "bf16"), ("nchw", "fp32"), ("nhwc_scalar", "bf16"),
            ("nhwc_scalar", "fp32"), ("nhwc_vec", "bf16")]
_ELTS = [("fixed_channel", "nhwc", "bf16")] + [
    (k, lay, d) for k in ("vec", "scalar") for lay in ("nhwc", "nchw")
    for d in ("bf16", "fp32")]
_KINDS = ("fixed_channel", "vec", "scalar")
# block geometry of the NHWC kernels (bn_act.hip): threads per block and
# the most channel lanes a block holds
BLOCK, LANES = 256, 64

REQUIRED = sorted(set(
    [f"stats:{k}:{d}" for k, d in _REDUCES]
    + [f"bwd_reduce:{k}:{d}:{g}" for k, d in _REDUCES for g in ("none", "y")]
    + [f"bwd_reduce:{k}:bf16:mask" for k in ("nhwc_scalar", "nhwc_vec")]
    + [f"bwd_reduce:{k}:act{a}" for k, _ in _REDUCES for a in (0, 1, 2)]
    + [f"bwd_reduce:{k}:mask:act{a}" for k in ("nhwc_scalar", "nhwc_vec")
       for a in (1, 2)]
    + [f"{p}:{k}:{lay}:{d}" for p in ("apply", "dx") for k, lay, d in _ELTS]
    + [f"{p}:{k}:act{a}" for p in ("apply", "dx") for k in _KINDS
       for a in (0, 1, 2)]
    + [f"{p}:{k}:{r}" for p in ("apply", "dx") for k in _KINDS
       for r in ("add", "noadd")]
    + ["apply:fixed_channel:mask", "apply:fixed_channel:nomask"]
    + [f"dx:fixed_channel:{g}" for g in ("none", "y", "mask")]
    + [f"dx:{k}:{g}" for k in ("vec", "scalar") for g in ("none", "y")]
    + ["dx:fixed_channel:mask:add", "dx:fixed_channel:mask:act1",
       "dx:fixed_channel:mask:act2"]
    + ["fin:f32", "fin:f64", "fin:Y=1", "fin:Y>1", "fin:Y=64",
       "cblocks=16", "fixed:lane_blocks=2", "rows:odd"]
    + ["slices:empty", "count=1", "rows<RG", "fixed:tail_lane_block", "C<8",
       "nchw:hw1", "eval:fixed_channel", "eval:nchw", "eval:nchw:vec",
       "eval:nchw:scalar"]
    + [f"S={s}" for s in (2, 100, 128, 2048)]))


def dtype_name(dtype):
    return "bf16" if dtype is BF else "fp32"


def plan(ext, case, act=None, training=None, masked=False):
    """ext.bn_plan of the case's shape; act/training default to the
    case's own."""
    N, C, H, W = case.shape
    return ext.bn_plan(
        N, C, H * W, case.nhwc, 2 if case.dtype is BF else 4,
        ACT[case.act] if act is None else act,
        case.training if training is None else training, masked)


def writes_mask(case, act=None):
    """The documented rule: training and an activation on bf16 NHWC with
    whole 8-channel groups."""
    a = ACT[case.act] if act is None else act
    return bool(case.training and a != 0 and case.nhwc and case.dtype is BF
                and case.shape[1] % 8 == 0)


def _tags_of(ext, case, act, add, training, gates):
    N, C, H, W = case.shape
    d = dtype_name(case.dtype)
    lay = "nhwc" if case.nhwc else "nchw"
    r = "add" if add else "noadd"
    tags = set()
    for gate in gates:
        # the caller's view: it holds a mask, or it holds y
        pl = plan(ext, case, act, training, gate == "mask")
        red = pl["reduce"]
        if training:
            tags |= {f"stats:{red}:{d}", f"S={pl['S']}",
                     f"cblocks={pl['cblocks']}",
                     "fin:f32" if pl["slab"] == "f32" else "fin:f64",
                     "fin:Y=1" if pl["Y"] == 1 else "fin:Y>1",
                     f"fin:Y={pl['Y']}"}
        ap = pl["apply"]
        tags |= {f"apply:{ap}:{lay}:{d}", f"apply:{ap}:act{act}",
                 f"apply:{ap}:{r}"}
        if ap == "fixed_channel":
            tags.add("apply:fixed_channel:" +
                     ("mask" if pl["writes_mask"] else "nomask"))
            tags.add(f"fixed:lane_blocks={pl['apply_grid'][0]}")
        rg, dg, dx = pl["reduce_gate"], pl["dx_gate"], pl["dx"]
        tags |= {f"bwd_reduce:{red}:{d}:{rg}", f"bwd_reduce:{red}:act{act}",
                 f"dx:{dx}:{lay}:{d}", f"dx:{dx}:act{act}", f"dx:{dx}:{r}",
                 f"dx:{dx}:{dg}"}
        if rg == "mask":
            tags.add(f"bwd_reduce:{red}:mask:act{act}")
        if dg == "mask":
            tags |= {f"dx:{dx}:mask:act{act}", f"dx:{dx}:mask:{r}"}
        # edge geometries, from the plan and the kernels' own slicing
        rows, S = N * H * W, pl["S"]
        if (S - 1) * -(-rows // S) >= rows:
            tags.add("slices:empty")
        if case.nhwc:
            lanes = C // 8 if red == "nhwc_vec" else C
            if rows < BLOCK // min(lanes, LANES):
                tags.add("rows<RG")
        if ap == "fixed_channel" and pl["apply_grid"][0] > 1 \
                and (C // 8) % LANES == 1:
            tags.add("fixed:tail_lane_block")
        if not training:
            if ap == "fixed_channel" and dx == "fixed_channel" and act != 0:
                tags.add("eval:fixed_channel")
            if not case.nhwc:
                tags |= {"eval:nchw", f"eval:nchw:{ap}"}
    rows = N * H * W
    if rows % 2:
        tags.add("rows:odd")
    if rows == 1:
        tags.add("count=1")
    if C < 8 and case.nhwc:
        tags.add("C<8")
    if not case.nhwc and H * W == 1 and N > 1:
        tags.add("nchw:hw1")
    return tags


def reached(ext, case):
    """Coverage tags the case reaches, from the launchers' own plan: its
    own run, and the act-none run of the exactness test."""
    tags = _tags_of(ext, case, ACT[case.act], case.res, case.training,
                    case.bwd)
    tags |= _tags_of(ext, case, 0, False, True, ("y",))
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


# ------------------------------------------------------------------ data
def _layout(t, nhwc):
    return t.contiguous(memory_format=torch.channels_last) if nhwc \
        else t.contiguous()


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """Seeded random inputs of one case, generated on the CPU in the
    case's dtype and layout; shared read-only between the tests."""
    case = CASE_BY_NAME[name]
    C = case.shape[1]
    g = torch.Generator().manual_seed(4100 + CASES.index(case))
    d = {"x": _layout(torch.randn(case.shape, generator=g).to(case.dtype),
                      case.nhwc),
         "dy": _layout(torch.randn(case.shape, generator=g).to(case.dtype),
                       case.nhwc),
         "res": _layout(torch.randn(case.shape, generator=g).to(case.dtype),
                        case.nhwc) if case.res else None,
         "gamma": torch.rand(C, generator=g) + 0.5,
         "beta": torch.randn(C, generator=g),
         "rm": torch.randn(C, generator=g) * 0.1,
         "rv": torch.rand(C, generator=g) + 0.5}
    return d


@functools.lru_cache(maxsize=None)
def integer_inputs(shape, dtype, nhwc):
    """x in {-2..2}, dy in {-1..1}: every partial sum is an integer, exact
    in fp32 and double in any order."""
    g = torch.Generator().manual_seed(977)
    x = torch.randint(-2, 3, shape, generator=g).to(dtype)
    dy = torch.randint(-1, 2, shape, generator=g).to(dtype)
    return _layout(x, nhwc), _layout(dy, nhwc)


# ---------------------------------------------------------- dyadic data
# Data on which BN+act is exact in fp32 and bf16 whatever the summation
# order or fma contraction. With R = N*H*W rows and P = R // 4, channel c
# holds x = m_c + d: m_c an integer in -3..3, d = +2 at P seeded rows, -2
# at P others, 0 elsewhere. So sum x = R*m_c, sum x^2 = R*m_c^2 + 8P, the
# mean is m_c and the biased variance 8P/R; eps = float32(4 - 8P/R) makes
# var + eps = 4 to within 2^-25 and invstd exactly 0.5, hence xhat in
# {-1, 0, 1}. gamma in {0.5, 1, 2, -1} (and 4 for relu6, so that the upper
# clamp is reached), beta an odd multiple of 0.25 below 3 in magnitude, res
# in {-1, -0.5, 0, 0.5, 1}: v = gamma*xhat + beta (+res) is an odd multiple
# of 0.25, never 0 or 6, and y is bf16-exact. dy is an integer in -2..2, so
# dgamma and dbeta are integers. Eval cases take running_mean = m_c,
# running_var = 2 and eps = 2 for the same invstd.
DY_MOM = 0.5
_GAMMAS = (0.5, 1.0, 2.0, -1.0)


def _pick(values, n, g):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(len(values), (n,), generator=g)]


def dyadic64(name):
    """The dyadic data of one case in float64, NCHW-contiguous, before the
    cast to the case's dtype (which test_bn_cases_cpu.py proves lossless)."""
    case = CASE_BY_NAME[name]
    N, C, H, W = case.shape
    R = N * H * W
    P = R // 4
    g = torch.Generator().manual_seed(5200 + CASES.index(case))
    m = torch.randint(-3, 4, (C,), generator=g).double()
    perm = torch.rand(C, R, generator=g).argsort(dim=1)
    dev = torch.zeros(C, R, dtype=torch.float64)
    dev.scatter_(1, perm[:, :P], 2.0)
    dev.scatter_(1, perm[:, P:2 * P], -2.0)
    x = (m.view(C, 1) + dev).view(C, N, H, W).permute(1, 0, 2, 3).contiguous()
    gamma = _pick(_GAMMAS + ((4.0,) if case.act == "relu6" else ()), C, g)
    beta = (2 * torch.randint(-6, 6, (C,), generator=g).double() + 1) / 4
    gamma[C - 1] = -1.0
    if case.act == "relu6":
        gamma[0], beta[0] = 4.0, 2.75      # v = 6.75 where xhat = 1
    d = {"x": x, "m": m, "P": P, "R": R, "gamma": gamma, "beta": beta,
         "dy": torch.randint(-2, 3, case.shape, generator=g).double(),
         "res": torch.randint(-2, 3, case.shape, generator=g).double() / 2
         if case.res else None}
    if case.training:
        d["rm"] = 2 * torch.randint(-2, 3, (C,), generator=g).double()
        d["rv"] = torch.zeros(C, dtype=torch.float64)
        d["eps"] = float(torch.tensor(4.0 - 8.0 * P / R,
                                      dtype=torch.float32))
    else:
        d["rm"], d["rv"], d["eps"] = m.clone(), torch.full_like(m, 2.0), 2.0
    return d


@functools.lru_cache(maxsize=None)
def dyadic_inputs(name):
    """dyadic64 in the case's dtype and layout (gamma, beta and the running
    statistics in fp32); shared read-only between the tests."""
    case = CASE_BY_NAME[name]
    d = dyadic64(name)
    for k in ("x", "dy", "res"):
        if d[k] is not None:
            d[k] = _layout(d[k].to(case.dtype), case.nhwc)
    for k in ("gamma", "beta", "rm", "rv"):
        d[k] = d[k].float()
    return d


def formulas64(case, d, mean, invstd, gate=None):
    """The kernels' documented formulas in float64, from inputs ``d`` (a
    case_inputs / dyadic_inputs dict) and per-channel mean and invstd:
      v = gamma*xhat + beta (+res), y = act(v), g = dy*gate,
      dbeta = sum g, dgamma = sum g*xhat, dres = g,
      dx = k1*(g - k2 - xhat*k3), k1 = gamma*invstd, k2 = dbeta/R and
      k3 = dgamma/R (both 0 in eval mode).
    gate: the 0/1 activation gate to use (the kernel's own); default the
    reference's, v > 0 for relu and 0 < v < 6 for relu6."""
    N, C, H, W = case.shape
    R = N * H * W

    def ch(t):
        return t.double().view(1, C, 1, 1)
    x, dy = d["x"].double().contiguous(), d["dy"].double().contiguous()
    xhat = (x - ch(mean)) * ch(invstd)
    v = ch(d["gamma"]) * xhat + ch(d["beta"])
    if case.res:
        v = v + d["res"].double().contiguous()
    y = {"none": v, "relu": torch.relu(v),
         "relu6": torch.clamp(v, 0, 6)}[case.act]
    own = {"none": torch.ones_like(v, dtype=torch.bool), "relu": v > 0,
           "relu6": (v > 0) & (v < 6)}[case.act]
    g = dy * (own if gate is None else gate).double()
    dbeta = g.sum(dim=(0, 2, 3))
    dgamma = (g * xhat).sum(dim=(0, 2, 3))
    k1 = d["gamma"].double() * invstd.double()
    k2 = dbeta / R if case.training else torch.zeros_like(dbeta)
    k3 = dgamma / R if case.training else torch.zeros_like(dgamma)
    dx = ch(k1) * (g - ch(k2) - xhat * ch(k3))
    return {"xhat": xhat, "v": v, "y": y, "gate": own, "g": g,
            "dbeta": dbeta, "dgamma": dgamma, "k1": k1, "k2": k2, "k3": k3,
            "dx": dx, "dres": g}


def unpack_mask(mask, case):
    """The forward's 1-bit mask as a bool tensor of the case's (N, C, H, W):
    bit i & 7 of byte i / 8, i the element's index in NHWC memory order."""
    N, C, H, W = case.shape
    assert case.nhwc and mask.dtype is torch.uint8 and mask.dim() == 1
    bits = (mask.cpu().to(torch.int32).view(-1, 1)
            >> torch.arange(8, dtype=torch.int32)) & 1
    return bits.view(N, H, W, C).permute(0, 3, 1, 2).bool()


def kernel_gate(case, r, gate):
    """The gate one backward run of ``r`` (a run_case result) used: the
    unpacked mask, or the activation's gate on the returned y."""
    if case.act == "none":
        return torch.ones(case.shape, dtype=torch.bool)
    if gate == "mask":
        return unpack_mask(r["mask"], case)
    y = r["y"].cpu().double().contiguous()
    return (y > 0) & (y < 6) if case.act == "relu6" else y > 0


def within_one_ulp(got, ref):
    """got equals ref or one of its two neighbours in ref's dtype."""
    up = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    dn = torch.nextafter(ref, torch.full_like(ref, float("-inf")))
    return bool(((got == ref) | (got == up) | (got == dn)).all())


def half_ulp_bf16(ref64):
    """Half a bf16 ulp (8 significant bits) at each element of ref64."""
    _, e = torch.frexp(ref64.abs())          # |ref| = mant * 2^e, mant < 1
    h = torch.ldexp(torch.ones_like(ref64), e - 9)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), h)


@functools.lru_cache(maxsize=None)
def reference64(name):
    """float64 BN (+res) + act on the CPU from the case's own inputs, and
    the float64 statistics the backward reference (formulas64, with the
    kernel's own gate) is built from. One row per channel, which
    F.batch_norm refuses in training mode, takes the formulas with var = 0
    and the kernel's unbiased guard (running_var moves towards 0)."""
    case = CASE_BY_NAME[name]
    d = case_inputs(name)
    N, C, H, W = case.shape
    x = d["x"].double().contiguous()
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    if case.training:
        mean = x.mean(dim=(0, 2, 3))
        var = x.var(dim=(0, 2, 3), unbiased=False)
    else:
        mean, var = rm.clone(), rv.clone()
    invstd = torch.rsqrt(var + EPS)
    if case.training and N * H * W == 1:
        y = formulas64(case, d, mean, invstd)["y"]
        rm = (1 - MOM) * rm + MOM * mean
        rv = (1 - MOM) * rv + MOM * var
    else:
        v = F.batch_norm(x, rm, rv, d["gamma"].double(), d["beta"].double(),
                         case.training, MOM, EPS)
        if case.res:
            v = v + d["res"].double().contiguous()
        y = {"none": v, "relu": torch.relu(v),
             "relu6": torch.clamp(v, 0, 6)}[case.act]
    return {"y": y, "rm": rm, "rv": rv, "mean": mean, "invstd": invstd}


# ------------------------------------------------------------------- run
def _run(ext, case, d, dev, mom, eps, gates):
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    res = d["res"].to(dev) if case.res else None
    gamma, beta = d["gamma"].to(dev), d["beta"].to(dev)
    rm, rv = d["rm"].to(dev), d["rv"].to(dev)
    act = ACT[case.act]
    outs = ext.bn_act_fwd(x, res, gamma, beta, rm, rv, case.training, mom,
                          eps, act, case.nhwc)
    out = {"y": outs[0], "mean": outs[1], "invstd": outs[2], "rm": rm,
           "rv": rv}
    if len(outs) > 3:
        out["mask"] = outs[3]
    for gate in gates:
        if gate == "mask":
            assert "mask" in out, f"{case.name}: forward wrote no mask"
            y_arg, m_arg = None, out["mask"]
        else:
            y_arg, m_arg = out["y"], None
        b = ext.bn_act_bwd(dy, y_arg, x, out["mean"], out["invstd"], gamma,
                           act, case.training, case.res, case.nhwc, m_arg)
        for k, t in zip(("dx", "dgamma", "dbeta", "dres"), b):
            out[f"{k}@{gate}"] = t
    return out


def run_case(ext, case, dev):
    """The case through ext.bn_act_fwd and one ext.bn_act_bwd per gate
    source in case.bwd. Returns a flat dict of device tensors (bwd results
    keyed '<name>@<gate>'); uses nothing but the two bindings."""
    return _run(ext, case, case_inputs(case.name), dev, MOM, EPS, case.bwd)


def dyadic_gates(case):
    """Both gate sources wherever the forward writes a mask."""
    return ("mask", "y") if writes_mask(case) else ("y",)


def run_dyadic(ext, case, dev):
    """run_case on the dyadic data, backward from every gate source."""
    d = dyadic_inputs(case.name)
    return _run(ext, case, d, dev, DY_MOM, d["eps"], dyadic_gates(case))

