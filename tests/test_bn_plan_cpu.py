"""The BN+act dispatch plan (ext.bn_plan, a pure host function of the built
extension) against hand-computed rows, and the case table of the path
tests against the plan. No device needed.

The constants the rows are worked out from (bn_act.hip): 256 threads and
at most 64 channel lanes per block; 8-wide bf16 reduces for C <= 512;
fixed-channel apply/dx from 32768 rows; S = min(max(rows/16, 1),
max(2048/cblocks, 1)) row slices; grid-stride grids capped at 2048 blocks;
finalize: 32-channel chunks, Y = min(ceil(S/32), 64)."""

import pytest

import bn_cases as bc


def _ext():
    from ddlbench_amd.ops import require_extension
    return require_extension()


def _row(pl, *names):
    return tuple(pl[n] for n in names)


RED = ("reduce", "cblocks", "S", "slab", "slab_bytes")
FIN = ("cchunks", "Y", "part_doubles")
APPLY = ("apply", "apply_grid", "writes_mask")
DX = ("dx", "dx_grid", "dx_gate", "reduce_gate")


def test_plan_hand_computed_rows():
    ext = _ext()
    # case 1: rows = 32, one 8-channel lane; S = min(32/16, 2048) = 2;
    # fp32 slab = 2 slices * 2 * 8 channels * 4 B
    pl = ext.bn_plan(2, 8, 16, True, 2, 1, True, True)
    assert _row(pl, *RED) == ("nhwc_vec", 1, 2, "f32", 128)
    assert _row(pl, *FIN) == (1, 1, 0)
    assert _row(pl, *APPLY) == ("fixed_channel", (1, 2), True)
    assert _row(pl, *DX) == ("fixed_channel", (1, 2), "mask", "mask")
    # the same layer, the caller holding y: rows < 32768 -> grid-stride,
    # 256 elements / 8 per thread = 32 threads = 1 block
    pl = ext.bn_plan(2, 8, 16, True, 2, 1, True, False)
    assert _row(pl, *DX) == ("vec", (1, 1), "y", "y")
    # case 3: rows = 32768 = the threshold; S = min(2048, 2048/1);
    # Y = min(2048/32, 64) = 64, part = 1 chunk * 64 * 2 * 32 doubles
    pl = ext.bn_plan(8, 8, 4096, True, 2, 0, True, False)
    assert _row(pl, *RED) == ("nhwc_vec", 1, 2048, "f32", 2048 * 2 * 8 * 4)
    assert _row(pl, *FIN) == (1, 64, 4096)
    assert _row(pl, *APPLY) == ("fixed_channel", (1, 2048), False)
    assert _row(pl, *DX) == ("fixed_channel", (1, 2048), "none", "none")
    # one row fewer than the threshold: grid-stride, 262136*8/8/256 blocks
    pl = ext.bn_plan(1, 8, 32767, True, 2, 0, True, False)
    assert _row(pl, "apply", "apply_grid", "dx") == ("vec", (128, 1), "vec")
    # case 5: C = 1024 > 512: scalar reduce, 1024/64 = 16 lane blocks,
    # S = min(256/16, 2048/16) = 16, double slab; the fixed-channel grid
    # has 128 lanes / 64 = 2 lane blocks and min(16, 1024) slices
    pl = ext.bn_plan(4, 1024, 64, True, 2, 1, True, True)
    assert _row(pl, *RED) == ("nhwc_scalar", 16, 16, "f64",
                              16 * 2 * 1024 * 8)
    assert _row(pl, *FIN) == (32, 1, 0)
    assert _row(pl, *APPLY) == ("fixed_channel", (2, 16), True)
    assert _row(pl, *DX) == ("fixed_channel", (2, 16), "mask", "mask")
    # C = 512 is still 8-wide: 64 lanes, one lane block
    pl = ext.bn_plan(8, 512, 256, True, 2, 1, True, True)
    assert _row(pl, *RED) == ("nhwc_vec", 1, 128, "f32", 128 * 2 * 512 * 4)
    assert _row(pl, *FIN) == (16, 4, 16 * 4 * 2 * 32)
    # case 7: C = 12: scalar everything, no mask; 384 elements = 2 blocks
    pl = ext.bn_plan(2, 12, 16, True, 2, 1, True, False)
    assert _row(pl, *RED) == ("nhwc_scalar", 1, 2, "f64", 2 * 2 * 12 * 8)
    assert _row(pl, *APPLY) == ("scalar", (2, 1), False)
    assert _row(pl, *DX) == ("scalar", (2, 1), "y", "y")
    # a mask offered where no masked kernel exists is not honoured
    pl = ext.bn_plan(2, 12, 16, True, 2, 1, True, True)
    assert _row(pl, *DX) == ("scalar", (2, 1), "y", "y")
    # fp32 NHWC, C = 24: scalar reduce, 8-wide fp32 apply/dx;
    # 2520 elements / 8 = 315 threads = 2 blocks
    pl = ext.bn_plan(3, 24, 35, True, 4, 1, True, False)
    assert _row(pl, *RED) == ("nhwc_scalar", 1, 6, "f64", 6 * 2 * 24 * 8)
    assert _row(pl, *APPLY) == ("vec", (2, 1), False)
    # NCHW fp32 (8,32,14,14): one block per channel, S = min(ceil(1568/256),
    # 2048/32) = 7; HW = 196 is no multiple of 8 -> scalar, 50176/256 blocks
    pl = ext.bn_plan(8, 32, 196, False, 4, 1, True, False)
    assert _row(pl, *RED) == ("nchw", 32, 7, "f64", 7 * 2 * 32 * 8)
    assert _row(pl, *FIN) == (1, 1, 0)
    assert _row(pl, *APPLY) == ("scalar", (196, 1), False)
    assert _row(pl, *DX) == ("scalar", (196, 1), "y", "y")
    # NCHW bf16 (4,16,8,8): rows = 256 -> S = 1; HW % 8 == 0 -> 8-wide,
    # 4096 elements / 8 = 512 threads = 2 blocks
    pl = ext.bn_plan(4, 16, 64, False, 2, 1, True, True)
    assert _row(pl, *RED) == ("nchw", 16, 1, "f64", 1 * 2 * 16 * 8)
    assert _row(pl, *APPLY) == ("vec", (2, 1), False)
    assert _row(pl, *DX) == ("vec", (2, 1), "y", "y")
    # the 2048-block cap of the grid-stride kernels
    pl = ext.bn_plan(128, 64, 1024, False, 4, 0, False, False)
    assert _row(pl, "apply", "apply_grid") == ("vec", (2048, 1))


def test_plan_rejects_bad_arguments():
    ext = _ext()
    with pytest.raises(RuntimeError):
        ext.bn_plan(0, 8, 16, True, 2, 1, True, False)
    with pytest.raises(RuntimeError):
        ext.bn_plan(2, 8, 16, True, 8, 1, True, False)      # elsize


def test_cases_are_well_formed():
    for case in bc.CASES:
        assert set(case.claims) <= set(bc.REQUIRED), \
            (case.name, sorted(set(case.claims) - set(bc.REQUIRED)))
        assert case.bwd and set(case.bwd) <= {"mask", "y"}, case.name
        if "mask" in case.bwd:
            assert bc.writes_mask(case), case.name
        N, C, H, W = case.shape
        nbytes = N * C * H * W * (2 if case.dtype is bc.BF else 4)
        assert nbytes <= 4 << 20, case.name
    for name in bc.CROSS_CHECK:
        case = bc.CASE_BY_NAME[name]
        assert case.act == "relu" and set(case.bwd) == {"mask", "y"}


def test_case_table_reaches_every_kind():
    """Each case reaches the paths it claims, and the union of all plans
    covers bn_cases.REQUIRED: every value of every kind field, crossed
    with the gate sources, ADD, the three activations and both dtypes
    where the kind exists."""
    union = bc.check_claims(_ext())
    unreached = sorted(set(bc.REQUIRED) - union)
    assert not unreached, f"no case reaches {unreached}"


def test_writes_mask_rule_and_masked_plans_never_read_y():
    ext = _ext()
    for case in bc.CASES:
        for act in (0, 1, 2):
            for training in (False, True):
                pl = bc.plan(ext, case, act, training, False)
                want = bool(training and act != 0 and case.nhwc
                            and case.dtype is bc.BF
                            and case.shape[1] % 8 == 0)
                assert pl["writes_mask"] == want, (case.name, act, training)
                if want:
                    assert pl["apply"] == "fixed_channel"
        if "mask" in case.bwd:
            pl = bc.plan(ext, case, masked=True)
            assert pl["reduce_gate"] == "mask" and pl["dx_gate"] == "mask", \
                case.name
            assert pl["dx"] == "fixed_channel", case.name
