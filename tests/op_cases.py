"""Case tables and float64 references of the exact and edge-shape tests of
the first-generation kernels (test_ops_exact_gpu.py on the GPU,
test_op_cases_cpu.py without one): NHWC max-pool, depthwise 3x3, plain
cross-entropy, the multi-tensor SGD/Adam step and the sequence utilities.

The rule for an "exact" case is the one of conv_cases.py: inputs are small
integers times powers of two, every partial sum and every expected output
is representable in the accumulator type and in the output dtype, and the
GPU result is compared with ``==`` against a float64 CPU reference.
test_op_cases_cpu.py proves, for every exact case, that the reference
survives a round trip through the output dtype and that it equals the torch
CPU op in float64.

The launch geometry a case reaches is derived by Python mirrors of the
launchers' host arithmetic (``mp_geom``, ``dw_nhwc_geom``, ``EW_CAP``); the
gap -> case map below is asserted by the CPU test through ``REQUIRED``.

Gap                                               Case(s)
------------------------------------------------  --------------------------
ce_fwd_block_kernel VEC / scalar never run        ce: k4096_bf16, k4100_bf16,
                                                  k4096_fp32
grid-stride second trip: ce_bwd                   ce: b130_k4100
  fused_sgd / fused_adam                          lists: big
  revert_varlen                                   seq: rv_big
  NCHW depthwise fwd / dx                         dw: nchw_*_gridstride
CG8 does not divide 256 (rj >= RG live)           mp: *_c24, *_c104;
                                                  dw: nhwc_c96 .. nhwc_c384
second channel block with a tail (c0 >= C live)   mp: *_c520; dw: nhwc_c576,
                                                  nhwc_c960
row slicing that does not divide                  mp: k2s3_uneven;
                                                  dw: nhwc_slice512,
                                                  nhwc_slice2048
one row in all                                    mp: one_window
prefix binary search beyond four tensors          lists: n1 n2 n3 n5 n37 big
post-ReLU data, ties, gradient routing            mp: every case (tie share
                                                  asserted on the CPU)
padding tap must not win                          mp: neg_s2, neg_k5
NaN tap / all -inf window                         test_maxpool_nan_*,
                                                  test_maxpool_neg_inf_*
NCHW dw: S == 1 and S > 1                         dw: nchw_*_gridstride,
                                                  nchw_*_slice
optimizer pointer caches                          test_*_rebound_storage,
                                                  test_*_changed_membership,
                                                  test_*_grad_layout_copy
"""

import collections
import functools

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
FP32 = torch.float32
EW_CAP = 256 * 8 * 256      # elements one trip of a capped grid covers


def roundtrips(ref64, dtype):
    """True when the float64 tensor is unchanged by a cast to ``dtype``."""
    return torch.equal(ref64.to(dtype).double(), ref64)


def exact_mismatches(got, ref64, dtype):
    """Elements of ``got`` that differ from the float64 reference cast to
    ``dtype`` — the tests assert 0. NaN equals NaN here."""
    want = ref64.to(dtype)
    assert got.dtype == dtype and got.shape == want.shape, \
        (got.dtype, tuple(got.shape), tuple(want.shape))
    got = got.cpu()
    same = (got == want) | (got.isnan() & want.isnan())
    return int((~same).sum().item())


# ================================================================= max-pool
# shape = (N, C, H, W); geom = (k, stride, pad); data = "relu" | "neg"
PoolCase = collections.namedtuple("PoolCase", "name shape geom data")

POOL_CASES = [
    PoolCase("stem_c8", (1, 8, 7, 9), (3, 2, 1), "relu"),
    PoolCase("k2_c24", (2, 24, 7, 9), (2, 2, 0), "relu"),
    PoolCase("s1_c104", (1, 104, 6, 5), (3, 1, 1), "relu"),
    PoolCase("k5_c8", (1, 8, 6, 7), (5, 1, 2), "relu"),
    PoolCase("k3s3_c520", (1, 520, 7, 8), (3, 3, 0), "relu"),
    PoolCase("stem_c520", (1, 520, 5, 5), (3, 2, 1), "relu"),
    PoolCase("k2s3_uneven", (1, 8, 14, 20), (2, 3, 0), "relu"),
    PoolCase("one_window", (1, 8, 2, 2), (3, 2, 1), "relu"),
    PoolCase("h1_c24", (2, 24, 1, 9), (3, 2, 1), "relu"),
    PoolCase("neg_s2", (1, 8, 5, 7), (3, 2, 1), "neg"),
    PoolCase("neg_k5", (1, 8, 4, 5), (5, 1, 2), "neg"),
]
POOL_BY_NAME = {c.name: c for c in POOL_CASES}
assert len(POOL_BY_NAME) == len(POOL_CASES)


def pool_out_hw(case):
    N, C, H, W = case.shape
    k, s, p = case.geom
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def mp_geom(rows, C):
    """(CG8, cblocks, S) as maxpool.hip's mp_geom computes them."""
    cg8 = min(C // 8, 64)
    cblocks = (C // 8 + cg8 - 1) // cg8
    return cg8, cblocks, min(max(rows // 16, 1), max(2048 // cblocks, 1))


def pool_tags(case):
    N, C, H, W = case.shape
    OH, OW = pool_out_hw(case)
    tags = {"mp:geom:k%ds%dp%d" % case.geom, f"mp:C={C}"}
    cg8, cblocks, _ = mp_geom(N * OH * OW, C)
    if 256 % cg8:
        tags.add("mp:rj-guard")
    if cblocks > 1 and (C // 8) % cg8:
        tags.add("mp:c0-guard")
    for which, rows in (("fwd", N * OH * OW), ("bwd", N * H * W)):
        S = mp_geom(rows, C)[2]
        if rows % S:
            tags.add(f"mp:{which}:uneven-slices")
    if N * OH * OW == 1:
        tags.add("mp:rows=1")
    if (OH, OW) == (1, 1) and (H, W) == (2, 2):
        tags.add("mp:2x2->1x1")
    if H == 1 and W > 1:
        tags.add("mp:H=1")
    if case.geom in ((3, 2, 1), (2, 2, 0)) and H % 2 and W % 2:
        tags.add("mp:odd-HW:k%ds%dp%d" % case.geom)
    if case.data == "neg" and case.geom[2] > 0:
        tags.add("mp:neg-with-pad")
    return tags


def pool_reference(x, dy, geom):
    """Max-pool and its gradient in float64, written out: the window's
    in-bounds taps in row-major order, the first maximum takes dy. The CPU
    test holds it against F.max_pool2d and its autograd."""
    k, s, p = geom
    x64, dy64 = x.double(), dy.double()
    N, C, H, W = x64.shape
    OH, OW = dy64.shape[2:]
    y = torch.empty(N, C, OH, OW, dtype=torch.float64)
    dx = torch.zeros(N, C, H * W, dtype=torch.float64)
    for oh in range(OH):
        for ow in range(OW):
            best = where = None
            for kr in range(k):
                for ks in range(k):
                    ih, iw = oh * s - p + kr, ow * s - p + ks
                    if not (0 <= ih < H and 0 <= iw < W):
                        continue
                    v = x64[:, :, ih, iw]
                    if best is None:
                        best = v.clone()
                        where = torch.full((N, C), ih * W + iw)
                    else:
                        upd = v > best
                        best[upd] = v[upd]
                        where[upd] = ih * W + iw
            y[:, :, oh, ow] = best
            dx.scatter_add_(2, where.unsqueeze(2),
                            dy64[:, :, oh, ow].unsqueeze(2))
    return y, dx.view(N, C, H, W)


def pool_tie_share(x, geom):
    """Share of the (n, c, oh, ow) windows whose maximum is attained at two
    or more in-bounds taps."""
    k, s, p = geom
    N, C, H, W = x.shape
    x64 = x.double()
    cols = F.unfold(F.pad(x64, (p, p, p, p), value=float("-inf")), k,
                    stride=s).view(N, C, k * k, -1)
    top = cols.max(dim=2, keepdim=True).values
    return ((cols == top).sum(dim=2) >= 2).double().mean().item()


def pool_uncovered(case):
    """(H, W) bool mask of the input pixels no window covers."""
    N, C, H, W = case.shape
    k, s, p = case.geom
    OH, OW = pool_out_hw(case)
    rows = torch.ones(H, dtype=torch.bool)
    colsm = torch.ones(W, dtype=torch.bool)
    for o in range(OH):
        rows[max(o * s - p, 0):max(o * s - p + k, 0)] = False
    for o in range(OW):
        colsm[max(o * s - p, 0):max(o * s - p + k, 0)] = False
    return rows[:, None] | colsm[None, :]


@functools.lru_cache(maxsize=None)
def pool_data(name):
    """Seeded inputs (CPU, bf16, NCHW-contiguous) and the float64 reference
    of one case; computed once and shared read-only."""
    case = POOL_BY_NAME[name]
    g = torch.Generator().manual_seed(4100 + POOL_CASES.index(case))
    OH, OW = pool_out_hw(case)
    N, C, H, W = case.shape
    if case.data == "relu":     # post-ReLU: zero the most likely level
        levels = torch.tensor([0, 0, 0, 0, 0.5, 1, 2, 3])
    else:                       # every value <= -1: a padding tap would win
        levels = torch.tensor([-1.0, -1, -2, -3, -1.5])
    x = levels[torch.randint(len(levels), case.shape, generator=g)].to(BF16)
    dy = torch.randint(-4, 5, (N, C, OH, OW), generator=g).to(BF16)
    y, dx = pool_reference(x, dy, case.geom)
    return {"x": x, "dy": dy, "y": y, "dx": dx}


# ============================================================ depthwise 3x3
# shape = (N, C, H, W); scale = power-of-two exponents of (x, w, dy)
DwCase = collections.namedtuple("DwCase", "name layout dtype shape stride "
                                "scale")
_COMBOS = (("nchw", FP32), ("nchw", BF16), ("nhwc", BF16))


def _dw_cases():
    out = []
    scales = [(0, 0, 0), (-1, 1, 0), (1, -2, 1), (0, -1, 2)]

    def add(name, layout, dtype, shape, stride):
        out.append(DwCase(name, layout, dtype, shape, stride,
                          scales[len(out) % len(scales)]))

    for C in (8, 96, 144, 192, 384, 576, 960):
        for st in (1, 2):
            add(f"nhwc_c{C}_s{st}", "nhwc", BF16, (1, C, 5, 5), st)
    spatial = [("1x1", (2, 8, 1, 1)), ("1x7", (1, 24, 1, 7)),
               ("2x2", (3, 8, 2, 2)), ("7x7", (1, 24, 7, 7)),
               ("8x6", (2, 8, 8, 6))]
    for layout, dtype in _COMBOS:
        tag = f"{layout}_{'fp32' if dtype is FP32 else 'bf16'}"
        for sp, shape in spatial:
            for st in (1, 2):
                add(f"{tag}_{sp}_s{st}", layout, dtype, shape, st)
        # NCHW dw kernel: S > 1 (C*9 small); NHWC: slices that do not divide
        add(f"{tag}_slice_s1", layout, dtype, (3, 8, 13, 15), 1)
        add(f"{tag}_slice_s2", layout, dtype, (3, 8, 26, 29), 2)
    add("nhwc_slice2048", "nhwc", BF16, (3, 8, 23, 31), 1)
    # more than 524 288 outputs: the capped grid's second trip; C*9 > 2048
    add("nchw_fp32_gridstride", "nchw", FP32, (2, 520, 23, 23), 1)
    add("nchw_bf16_gridstride", "nchw", BF16, (2, 520, 23, 23), 1)
    return out


DW_CASES = _dw_cases()
DW_BY_NAME = {c.name: c for c in DW_CASES}
assert len(DW_BY_NAME) == len(DW_CASES)


def dw_out_hw(case):
    N, C, H, W = case.shape
    return (H - 1) // case.stride + 1, (W - 1) // case.stride + 1


def dw_via(case):
    """Where the weight gradient is compared. "grad": weight.grad through
    the autograd bridge, in the weight's dtype. "ext": the fp32 result of
    ext.dw3x3_bwd, before functional.py casts it — for bf16 weights whose
    dw, a sum over up to N*OH*OW products of magnitude <= 9 * 2^(sx+sdy),
    may need more than bf16's 8 significant bits."""
    if case.dtype is FP32:
        return "grad"
    N = case.shape[0]
    OH, OW = dw_out_hw(case)
    return "grad" if 9 * N * OH * OW <= 256 else "ext"


def dw_nhwc_geom(rows, C, div):
    """(CG8, cblocks, slices) of the NHWC depthwise launchers: div = 256
    for fwd and dx, 1024 (and a 1024 cap) for dw."""
    cg8 = min(C // 8, 64)
    cblocks = (C // 8 + cg8 - 1) // cg8
    cap = 2048 if div == 256 else 1024
    return cg8, cblocks, min(max(rows // div, 1), max(cap // cblocks, 1))


def dw_tags(case):
    N, C, H, W = case.shape
    OH, OW = dw_out_hw(case)
    dt = "fp32" if case.dtype is FP32 else "bf16"
    tags = {f"dw:{case.layout}:{dt}:s{case.stride}"}
    if (H, W) == (1, 1):
        tags.add("dw:1x1")
    if (H, W) == (1, 7):
        tags.add("dw:1x7")
    if (H, W) == (2, 2) and case.stride == 2:
        tags.add("dw:2x2:s2")
    if (H, W) in ((7, 7), (8, 6)):
        tags.add(f"dw:{H}x{W}")
    if case.layout == "nhwc":
        tags.add(f"dw:nhwc:C={C}")
        cg8, cblocks, S = dw_nhwc_geom(N * OH * OW, C, 256)
        if 256 % cg8:
            tags.add("dw:rj-guard")
        if cblocks > 1 and (C // 8) % cg8:
            tags.add("dw:c0-guard")
        if S > 1 and (N * OH * OW) % S:
            tags.add("dw:nhwc:uneven-slices")
        Sg = dw_nhwc_geom(N * OH * OW, C, 1024)[2]
        if Sg > 1 and (N * OH * OW) % Sg:
            tags.add("dw:nhwc:dw-uneven-slices")
    else:
        if N * C * OH * OW > EW_CAP:
            tags.add(f"dw:nchw:{dt}:gridstride")
        S = max(min((N * OH * OW + 255) // 256, max(2048 // (C * 9), 1)), 1)
        tags.add("dw:nchw:dw-S>1" if S > 1 else "dw:nchw:dw-S=1")
    return tags


def dw_lattice(shape, generator, exp, dtype):
    """Integers in [-3, 3] times 2^exp."""
    t = torch.randint(-3, 4, shape, generator=generator).to(FP32)
    return (t * 2.0 ** exp).to(dtype)


def dw_reference(x, w, dy, stride):
    """float64 F.conv2d(groups=C) and its autograd on the CPU."""
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride, 1, 1, groups=x.size(1))
    y64.backward(dy.double())
    return y64.detach(), x64.grad, w64.grad


@functools.lru_cache(maxsize=None)
def dw_data(name):
    case = DW_BY_NAME[name]
    g = torch.Generator().manual_seed(5200 + DW_CASES.index(case))
    N, C, H, W = case.shape
    OH, OW = dw_out_hw(case)
    sx, sw, sdy = case.scale
    x = dw_lattice(case.shape, g, sx, case.dtype)
    w = dw_lattice((C, 1, 3, 3), g, sw, case.dtype)
    dy = dw_lattice((N, C, OH, OW), g, sdy, case.dtype)
    y, dx, dw = dw_reference(x, w, dy, case.stride)
    return {"x": x, "w": w, "dy": dy, "y": y, "dx": dx, "dw": dw}


# ============================================================ cross-entropy
# special: rows 0.. are replaced by the hard rows (needs B >= 3, K >= 3)
CeCase = collections.namedtuple("CeCase", "name B K dtype special")

CE_CASES = [
    CeCase("k4096_bf16", 4, 4096, BF16, True),      # VEC block kernel
    CeCase("k4100_bf16", 3, 4100, BF16, True),      # scalar block kernel
    CeCase("k4096_fp32", 4, 4096, FP32, True),      # scalar block, fp32
    CeCase("k4095_bf16", 3, 4095, BF16, True),      # wave kernel, upper edge
    CeCase("k4095_fp32", 3, 4095, FP32, False),
    CeCase("k65_bf16", 5, 65, BF16, True),
    CeCase("k65_fp32", 5, 65, FP32, True),
    CeCase("k3_bf16", 4, 3, BF16, False),
    CeCase("k3_fp32", 4, 3, FP32, True),
    CeCase("k1_bf16", 3, 1, BF16, False),
    CeCase("k1_fp32", 3, 1, FP32, False),
    CeCase("b1_k4096_bf16", 1, 4096, BF16, False),
    CeCase("b1_k65_fp32", 1, 65, FP32, False),
    CeCase("b130_k4100", 130, 4100, BF16, False),   # bwd second trip
]
CE_BY_NAME = {c.name: c for c in CE_CASES}
assert len(CE_BY_NAME) == len(CE_CASES)
CE_GRAD_OUT = 2.0       # d(loss): gscale = CE_GRAD_OUT / B


@functools.lru_cache(maxsize=None)
def ce_data(name):
    """Logits (in the case's dtype), targets and the float64 F.cross_entropy
    reference (loss and dx for d(loss) = CE_GRAD_OUT) on those logits."""
    case = CE_BY_NAME[name]
    g = torch.Generator().manual_seed(6300 + CE_CASES.index(case))
    B, K = case.B, case.K
    x = (torch.randn(B, K, generator=g) * 2).to(case.dtype)
    t = torch.randint(K, (B,), generator=g)
    if case.special:
        assert B >= 3 and K >= 3
        # one class at +80, the rest at -80, the target on a -80 class
        x[0] = -80.0
        x[0, K // 2] = 80.0
        t[0] = K - 1
        # -inf on non-target classes: finite loss, dx exactly 0 there
        x[1, 1::2] = float("-inf")
        t[1] = 0
        if case.dtype is FP32:      # all logits equal and large
            x[2] = 3e4
    x64 = x.double().requires_grad_(True)
    loss = F.cross_entropy(x64, t)
    (loss * CE_GRAD_OUT).backward()
    return {"x": x, "t": t, "loss": loss.detach(), "dx": x64.grad}


# ======================================================= SGD / Adam lists
LISTS = {
    "n1": [5],
    "n2": [1, 1],
    "n3": [7, 3, 1],
    "n5": [1, 1, 6, 2, 1],
    "n37": [(i * 7) % 11 + 1 for i in range(34)] + [1, 1, 9],
    # the total exceeds one trip of the capped grid, with a tensor
    # boundary (550 009) inside the second trip
    "big": [1, 7, 300000, 1, 250000, 3],
}
LISTS["n37"][-1] = 1        # a one-element tensor last
assert len(LISTS["n37"]) == 37 and sum(LISTS["big"]) > EW_CAP
assert sum(LISTS["big"][:5]) > EW_CAP

SGD_HYPER = dict(lr=0.5, momentum=0.5, weight_decay=0.25)
SGD_STEPS = 3


def list_dtypes(sizes, dtype):
    """``dtype`` for every tensor, or alternating for dtype == "mixed"."""
    if dtype == "mixed":
        return [BF16 if i % 2 else FP32 for i in range(len(sizes))]
    return [dtype] * len(sizes)


def sgd_lattice(sizes, dtypes, seed, steps=SGD_STEPS):
    """Lattice parameters and per-step gradients: integers in [-3, 3]
    (params times 2), exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    ps = [(torch.randint(-3, 4, (n,), generator=g) * 2).to(dt)
          for n, dt in zip(sizes, dtypes)]
    gs = [[torch.randint(-3, 4, (n,), generator=g).to(dt)
           for n, dt in zip(sizes, dtypes)] for _ in range(steps)]
    return ps, gs


def sgd_reference(ps, gs, lr, momentum, weight_decay, check=None):
    """torch.optim.SGD's formula in float64; the parameter is rounded once
    per step to its own dtype, as the kernel's store does. Returns the
    parameters (own dtype) and momentum buffers (float64) after every step.
    ``check(value64, dtype)`` sees every intermediate with the type the
    kernel holds it in."""
    cur = [p.clone() for p in ps]
    mom = [None] * len(ps)
    out = []
    for step in gs:
        for i, g in enumerate(step):
            p64 = cur[i].double()
            wdp = weight_decay * p64
            d = g.double() + wdp
            if momentum:
                mv = d if mom[i] is None else momentum * mom[i] + d
                mom[i] = mv
            else:
                mv = d
            new = p64 - lr * mv
            if check is not None:
                for v in (wdp, d, mv, lr * mv, new):
                    check(v, FP32)
            cur[i] = new.to(ps[i].dtype)
        out.append(([c.clone() for c in cur],
                    [m.clone() if m is not None else None for m in mom]))
    return out


class AdamRef:
    """FusedAdam._step_torch's formula in float64, the parameter rounded
    once per step to its own dtype. ``step(grads, current)`` advances one
    step; with ``current`` the step starts from those parameter values
    instead of the reference's own (the moments stay the reference's), so a
    test can hold each single step of a kernel against float64 without an
    earlier step's rounding carried along."""

    def __init__(self, ps, lr, betas, eps, weight_decay, decoupled_wd):
        self.lr, self.betas, self.eps = lr, betas, eps
        self.wd, self.decoupled = weight_decay, decoupled_wd
        self.cur = [p.clone() for p in ps]
        self.m = [torch.zeros(p.shape, dtype=torch.float64) for p in ps]
        self.v = [torch.zeros(p.shape, dtype=torch.float64) for p in ps]
        self.t = 0

    def step(self, grads, current=None):
        b1, b2 = self.betas
        self.t += 1
        if current is not None:
            self.cur = [c.clone() for c in current]
        for i, g in enumerate(grads):
            p64, g64 = self.cur[i].double(), g.double()
            if self.wd and not self.decoupled:
                g64 = g64 + self.wd * p64
            self.m[i] = b1 * self.m[i] + (1 - b1) * g64
            self.v[i] = b2 * self.v[i] + (1 - b2) * g64 * g64
            upd = (self.m[i] / (1 - b1 ** self.t)) / (
                (self.v[i] / (1 - b2 ** self.t)).sqrt() + self.eps)
            if self.wd and self.decoupled:
                upd = upd + self.wd * p64
            self.cur[i] = (p64 - self.lr * upd).to(self.cur[i].dtype)
        return [c.clone() for c in self.cur]


def adam_reference(ps, gs, lr, betas, eps, weight_decay, decoupled_wd):
    """The parameters after every step of ``gs``."""
    ref = AdamRef(ps, lr, betas, eps, weight_decay, decoupled_wd)
    return [ref.step(step) for step in gs]


def adam_data(sizes, dtypes, seed, steps=3):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).to(dt) for n, dt in zip(sizes, dtypes)]
    gs = [[torch.randn(n, generator=g).to(dt)
           for n, dt in zip(sizes, dtypes)] for _ in range(steps)]
    return ps, gs


# ======================================================= sequence utilities
# (name, T, B, F, lengths)
SeqCase = collections.namedtuple("SeqCase", "name T B F lengths")

SEQ_CASES = [
    SeqCase("rv_small", 6, 4, 5, (0, 1, 6, 3)),
    SeqCase("rv_f1", 5, 3, 1, (5, 0, 2)),
    SeqCase("rv_b1", 7, 1, 3, (4,)),
    SeqCase("rv_b1_full", 3, 1, 9, (3,)),
    SeqCase("rv_t1", 1, 3, 7, (1, 0, 1)),
    SeqCase("rv_big", 9, 33, 1800,
            tuple([0, 1, 9] + [(i * 5) % 10 for i in range(30)])),
]
SEQ_BY_NAME = {c.name: c for c in SEQ_CASES}
assert 9 * 33 * 1800 > EW_CAP


def revert_reference(x, lengths):
    """out[t, b] = x[len_b - 1 - t, b] for t < len_b, else 0."""
    out = torch.zeros_like(x)
    for b, n in enumerate(lengths):
        for t in range(n):
            out[t, b] = x[n - 1 - t, b]
    return out


def mask_reference(lengths, T):
    return torch.tensor([[t < n for n in lengths] for t in range(T)],
                        dtype=torch.bool).reshape(T, len(lengths))


# ================================================================ coverage
REQUIRED = sorted(set(
    ["mp:geom:k%ds%dp%d" % g for g in ((3, 2, 1), (2, 2, 0), (3, 1, 1),
                                       (5, 1, 2), (3, 3, 0), (2, 3, 0))]
    + [f"mp:C={c}" for c in (8, 24, 104, 520)]
    + ["mp:rj-guard", "mp:c0-guard", "mp:fwd:uneven-slices",
       "mp:bwd:uneven-slices", "mp:rows=1", "mp:2x2->1x1", "mp:H=1",
       "mp:odd-HW:k3s2p1", "mp:odd-HW:k2s2p0", "mp:neg-with-pad"]
    + [f"dw:{lay}:{dt}:s{s}" for lay, dt in (("nchw", "fp32"),
                                             ("nchw", "bf16"),
                                             ("nhwc", "bf16"))
       for s in (1, 2)]
    + [f"dw:nhwc:C={c}" for c in (8, 96, 144, 192, 384, 576, 960)]
    + ["dw:1x1", "dw:1x7", "dw:2x2:s2", "dw:7x7", "dw:8x6", "dw:rj-guard",
       "dw:c0-guard", "dw:nhwc:uneven-slices", "dw:nhwc:dw-uneven-slices",
       "dw:nchw:fp32:gridstride", "dw:nchw:bf16:gridstride",
       "dw:nchw:dw-S>1", "dw:nchw:dw-S=1"]))


def reached():
    tags = set()
    for c in POOL_CASES:
        tags |= pool_tags(c)
    for c in DW_CASES:
        tags |= dw_tags(c)
    return tags
