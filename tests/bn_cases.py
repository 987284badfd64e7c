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
]

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# cases of the masked-vs-unmasked bit-for-bit cross-check (relu only)
CROSS_CHECK = ("c8_relu_train", "rows32k_relu", "c1024_relu", "c24_relu_res")

_REDUCES = [("nchw", "bf16"), ("nchw", "fp32"), ("nhwc_scalar", "bf16"),
            ("nhwc_scalar", "fp32"), ("nhwc_vec", "bf16")]
_ELTS = [("fixed_channel", "nhwc", "bf16")] + [
    (k, lay, d) for k in ("vec", "scalar") for lay in ("nhwc", "nchw")
    for d in ("bf16", "fp32")]
_KINDS = ("fixed_channel", "vec", "scalar")

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
    + [f"S={s}" for s in (2, 128, 2048)]))


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
    if (N * H * W) % 2:
        tags.add("rows:odd")
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


@functools.lru_cache(maxsize=None)
def reference64(name):
    """float64 BN (+res) + act and its autograd on the CPU, from the
    case's own inputs."""
    case = CASE_BY_NAME[name]
    d = case_inputs(name)
    x = d["x"].double().contiguous().requires_grad_(True)
    res = d["res"].double().contiguous().requires_grad_(True) \
        if case.res else None
    gamma = d["gamma"].double().requires_grad_(True)
    beta = d["beta"].double().requires_grad_(True)
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    v = F.batch_norm(x, rm, rv, gamma, beta, case.training, MOM, EPS)
    if case.res:
        v = v + res
    y = {"none": v, "relu": torch.relu(v),
         "relu6": torch.clamp(v, 0, 6)}[case.act]
    y.backward(d["dy"].double().contiguous())
    N, C, H, W = case.shape
    if case.training:
        mean = d["x"].double().mean(dim=(0, 2, 3))
        var = d["x"].double().var(dim=(0, 2, 3), unbiased=False)
    else:
        mean, var = d["rm"].double(), d["rv"].double()
    xhat = (d["x"].double() - mean.view(1, C, 1, 1)) \
        * torch.rsqrt(var + EPS).view(1, C, 1, 1)
    return {"y": y.detach(), "rm": rm, "rv": rv, "mean": mean,
            "invstd": torch.rsqrt(var + EPS), "xhat": xhat,
            "dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad,
            "dres": res.grad if case.res else None}


# ------------------------------------------------------------------- run
def run_case(ext, case, dev):
    """The case through ext.bn_act_fwd and one ext.bn_act_bwd per gate
    source in case.bwd. Returns a flat dict of device tensors (bwd results
    keyed '<name>@<gate>'); uses nothing but the two bindings."""
    d = case_inputs(case.name)
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    res = d["res"].to(dev) if case.res else None
    gamma, beta = d["gamma"].to(dev), d["beta"].to(dev)
    rm, rv = d["rm"].to(dev), d["rv"].to(dev)
    act = ACT[case.act]
    outs = ext.bn_act_fwd(x, res, gamma, beta, rm, rv, case.training, MOM,
                          EPS, act, case.nhwc)
    out = {"y": outs[0], "mean": outs[1], "invstd": outs[2], "rm": rm,
           "rv": rv}
    if len(outs) > 3:
        out["mask"] = outs[3]
    for gate in case.bwd:
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
