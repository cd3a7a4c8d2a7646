"""The Linear sweep's harness (tests/linear_helpers.py), proved on a CPU.

The oracle library is an independent float32 implementation of ffh_linear_fwd / ffh_linear_bwd_ex: it has to pass the whole edge table (the
shapes of a 256-CU device) and 20 seeds of the random generator under the sweep's own bound, no case skipped -- so the float64 reference, the
generator and the tolerance are sound before a GPU sees them.  The route model has to send every case of the table to the kernel it names, and
the table has to name every family and variant.  And the checker has to be able to fail: each fault below is reported.
"""
import numpy as np
import pytest

import linear_helpers as LH
from linear_helpers import Case, NONE, RELU, SIG, OVERWRITE, ONLY_DX, ONLY_DW, PREMASKED, MASK_BY_X


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


@pytest.mark.parametrize("name", LH.EDGE_NAMES)
def test_oracle_passes_the_edge_table(olib, name):
    be = LH.HostBackend()
    cases = LH.edge_table(LH.TABLE_CUS)[name]
    assert cases
    for case in cases:
        _, rep = LH.run_and_check(olib, be, case, LH.TABLE_CUS)
        assert rep.ok(), f"{case!r}\n{rep}"
    print({k: round(v, 4) for k, v in sorted(LH.WORST.items())})


@pytest.mark.parametrize("seed", range(20))
def test_oracle_passes_the_random_sweep(olib, seed):
    be = LH.HostBackend()
    cases = LH.draw_cases(seed)
    assert len(cases) == 6
    for case in cases:
        assert 1 <= case.in_dim <= 1100 and 1 <= case.out_dim <= 1100 and 1 <= case.batch <= 4100
        _, rep = LH.run_and_check(olib, be, case, LH.TABLE_CUS)
        assert rep.ok(), f"{case!r}\n{rep}"


ROUTES_OF_THE_TABLE = {
    "linear_fwd|skinny", "linear_fwd|thin",
    "linear_fwd gemm|sk_128x128x64", "linear_fwd gemm|sk_64x128x64", "linear_fwd gemm|sk_128x128x64|streamk", "linear_fwd gemm|no_scratch_on_this_stream",
    "linear_fwd gemm (lds-dma)|glds_32x64_s3", "linear_fwd gemm (lds-dma)|glds_64x64_s3", "linear_fwd gemm (lds-dma)|glds_64x64_s2",
    "linear_fwd gemm (lds-dma)|glds_32x64_s2",
    "linear_fwd gemm|f32_128x128_cfg0", "linear_fwd gemm|f32_64x64_cfg1", "linear_fwd gemm|f32_32x32_cfg2",
    "linear_bwd|skinny",
    "linear_bwd dx gemm|sk_128x128x64", "linear_bwd dw gemm|sk_128x128x64", "linear_bwd dx gemm|sk_64x128x64", "linear_bwd dx gemm|sk_128x128x64|streamk",
    "linear_bwd dx gemm|sk_128x128x64|colmap", "linear_bwd dx gemm|sk_64x128x64|colmap", "linear_bwd dx gemm|sk_128x128x64|colmap|streamk",
    "linear_bwd dx gemm|sk_128x128x64|colsum",
    "linear_bwd dx+dw|glds_dual_64x64_s2", "linear_bwd dx gemm (lds-dma)|glds_64x64_s2", "linear_bwd dx gemm (lds-dma)|glds_64x64_s3", "linear_bwd dw gemm (lds-dma)|glds_64x64_s3",
    "linear_bwd dw gemm|f32_128x128_cfg0", "linear_bwd dw gemm|f32_64x64_cfg1", "linear_bwd dw gemm|f32_32x32_cfg2",
    "linear_bwd dx gemm|f32_64x64_cfg1", "linear_bwd dx gemm|f32_32x32_cfg2",
    "linear_bwd dx gemm (masking)|f32_32x32_cfg2", "linear_bwd dx gemm (masking)|f32_64x64_cfg1",
    "linear_bwd dx gemm (column map)|f32_128x128_cfg0", "linear_bwd dx gemm (column map)|f32_64x64_cfg1",
    "linear_bwd dx gemm (masking, column map)|f32_64x64_cfg1",
}


def test_route_model_sends_every_case_to_its_kernel_and_the_table_covers_every_route():
    """At 256 CUs.  The set is asserted, so that an edit of the table that loses a route fails here."""
    reached = set()
    for name, cases in LH.edge_table(LH.TABLE_CUS).items():
        for case in cases:
            assert case.want, f"{case.name} names no kernel"
            assert not LH.model_reaches(case), f"{case.name}: the route model gives {LH.expected_route(case, LH.TABLE_CUS)}, the case is there for {case.want}"
            reached.update(LH.expected_route(case, LH.TABLE_CUS)[0])
    assert reached == ROUTES_OF_THE_TABLE, (sorted(reached - ROUTES_OF_THE_TABLE), sorted(ROUTES_OF_THE_TABLE - reached))
    t = LH.edge_table(LH.TABLE_CUS)
    bwd = [c for cs in t.values() for c in cs if c.kind == "bwd"]
    sk = [c for c in bwd if LH.expected_route(c, LH.TABLE_CUS)[0] == ["linear_bwd|skinny"]]
    assert {c.flags & f for c in sk for f in (ONLY_DX, ONLY_DW, PREMASKED, MASK_BY_X)} >= {ONLY_DX, ONLY_DW, PREMASKED, MASK_BY_X}
    assert {1 if c.in_dim <= 256 else (2 if c.in_dim <= 512 else 4) for c in sk if c.out_dim <= 4} == {1, 2, 4}      # the column-chunk counts
    assert any(c.batch >= 16384 for c in sk) and any(c.act == SIG and c.has(ONLY_DX) for c in sk) and any(c.act == SIG and c.has(ONLY_DW) for c in sk)
    assert any(c.forked for c in bwd) and any(c.det for c in bwd) and any(not c.scratch for cs in t.values() for c in cs)
    assert sum(1 for c in bwd if c.cmap and LH.expected_route(c, LH.TABLE_CUS)[1]) >= 7 and sum(1 for c in bwd if c.cmap and not LH.expected_route(c, LH.TABLE_CUS)[1]) >= 4
    assert sum(1 for c in bwd if c.colsum and LH.expected_route(c, LH.TABLE_CUS)[2]) >= 2 and sum(1 for c in bwd if c.colsum and not LH.expected_route(c, LH.TABLE_CUS)[2]) >= 4
    assert any(c.integer for c in bwd) and any(c.integer for cs in t.values() for c in cs if c.kind == "fwd")


def test_generator_reaches_every_flag_null_and_stride_option():
    cases = [c for s in range(12) for c in LH.draw_cases(s)]
    fwd, bwd = [c for c in cases if c.kind == "fwd"], [c for c in cases if c.kind == "bwd"]
    assert len(fwd) >= 12 and len(bwd) >= 12
    assert {c.act for c in fwd} == set(LH.ACTS_FWD) and {c.act for c in bwd} == set(LH.ACTS_BWD)
    for f in (OVERWRITE, ONLY_DX, ONLY_DW, PREMASKED, MASK_BY_X):
        assert {c.has(f) for c in bwd} == {True, False}, f
    assert not any(c.has(ONLY_DX) and c.has(ONLY_DW) for c in bwd)
    for attr in ("db", "dx", "forked", "scratch"):
        assert {bool(getattr(c, attr)) for c in bwd} == {True, False}, attr
    assert {c.bias for c in fwd} == {True, False}
    for ld, width, off in (("ldx", "in_dim", "x_off"), ("ldy", "out_dim", "y_off"), ("lddy", "out_dim", "dy_off"), ("lddx", "in_dim", "dx_off")):
        pool = bwd if ld in ("lddy", "lddx") else cases
        assert any(getattr(c, ld) == getattr(c, width) for c in pool) and any(getattr(c, ld) % 4 and getattr(c, ld) > getattr(c, width) for c in pool), ld
        assert any(getattr(c, off) % 4 for c in pool) and any(getattr(c, off) == 0 for c in pool), off
    assert any(c.w_off % 4 for c in cases) and any(c.bias_off % 4 for c in fwd if c.bias)
    assert any(c.in_dim % 4 for c in cases) and any(c.out_dim <= 4 for c in cases) and any(c.in_dim % 128 == 0 for c in cases)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker can fail
FWD = Case("strided/fwd", "fwd", 42, 70, 50, SIG, ldx=45, x_off=1, ldy=73, y_off=2)
BWD = Case("strided/bwd", "bwd", 42, 70, 50, SIG, 0, ldx=45, ldy=73, lddy=71, lddx=47, dx_off=1)
BWD_MAP = Case("map/bwd", "bwd", 42, 70, 50, RELU, OVERWRITE | MASK_BY_X, cmap=True, ldx=45)
BWD_SUM = Case("colsum/bwd", "bwd", 42, 70, 50, RELU, OVERWRITE | MASK_BY_X, colsum=True, lddx=44)


def _run(olib, case):
    be = LH.HostBackend()
    res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(olib, be, case)
    check = LH.check_fwd if case.kind == "fwd" else LH.check_bwd
    rep = check(res)
    assert rep.ok(), str(rep)
    return res, rep, check


OUTPUTS = [(FWD, "y"), (BWD, "dy"), (BWD, "dw"), (BWD, "db"), (BWD, "dx"), (BWD_MAP, "dest0"), (BWD_MAP, "dest2"), (BWD_SUM, "colsum")]


@pytest.mark.parametrize("case,out", OUTPUTS, ids=[o for _, o in OUTPUTS])
def test_checker_reports_an_element_off_by_3e5_of_its_mass(olib, case, out):
    res, rep, check = _run(olib, case)
    buf = dict(res.outputs)[out]
    mass = rep.mass[out].reshape(buf.rows, buf.cols)
    r, c = np.unravel_index(int(np.argmax(mass)), mass.shape)
    assert mass[r, c] > 0
    at = buf.flat_index(r, c)
    for sign in (1.0, -1.0):
        keep = buf.host[at]
        buf.host[at] = np.float32(float(keep) + sign * 3e-5 * mass[r, c])
        rep2 = check(res)
        assert any(v.startswith(out + ":") for v in rep2.violations), f"a {out} element moved by 3e-5 of its mass went unnoticed\n{rep2}"
        buf.host[at] = keep
    assert check(res).ok()


@pytest.mark.parametrize("case", [FWD, BWD, BWD_MAP, BWD_SUM], ids=lambda c: c.name)
def test_checker_reports_an_overwritten_padding_element(olib, case):
    res, _, check = _run(olib, case)
    for name, buf in res.outputs:
        pads = np.flatnonzero(~buf.valid)
        assert pads.size >= LH.TAIL
        for at in (pads[0], pads[-1]):
            keep = buf.host[at]
            buf.host[at] = 0.0
            assert any(v.startswith(name + ":") for v in check(res).violations), f"{name}: an overwritten padding element went unnoticed"
            buf.host[at] = keep
    assert check(res).ok()


@pytest.mark.parametrize("case", [FWD, BWD], ids=lambda c: c.name)
def test_checker_reports_a_changed_input(olib, case):
    res, _, check = _run(olib, case)
    for name, buf in res.inputs:
        for at in (int(buf.idx[0]), int(buf.idx[-1]), int(np.flatnonzero(~buf.valid)[0])):
            keep = buf.host[at]
            buf.host[at] = np.float32(1.25)
            assert any(v.startswith(name + ":") for v in check(res).violations), f"{name}: a changed input went unnoticed"
            buf.host[at] = keep
    assert check(res).ok()


@pytest.mark.parametrize("flags,buf_name", [(ONLY_DX, "dw"), (ONLY_DX, "db"), (ONLY_DW, "dx")])
def test_checker_reports_a_write_the_flag_excludes(olib, flags, buf_name):
    res, _, check = _run(olib, Case("excluded", "bwd", 42, 70, 50, RELU, flags))
    buf = dict(res.outputs)[buf_name]
    at = int(buf.idx[3])
    buf.host[at] = np.float32(float(buf.host[at]) + 1e-3)
    assert any(v.startswith(buf_name + ":") for v in check(res).violations)


def test_checker_reports_a_written_plain_dx_under_a_taken_map_and_a_written_destination_under_a_declined_one(olib):
    res, _, check = _run(olib, BWD_MAP)
    assert res.scatter_used == 1
    res.DX.host[int(res.DX.idx[5])] = 0.5
    assert any(v.startswith("dx:") for v in check(res).violations)
    res, _, check = _run(olib, Case("declined", "bwd", 42, 70, 50, RELU, 0, cmap=True, colsum=True))
    assert res.scatter_used == 0 and res.colsum_used == 0
    res.dests[1].host[int(res.dests[1].idx[0])] = 0.5
    assert any(v.startswith("dest1:") for v in check(res).violations)
    res.dests[1].host[:] = res.dests[1].before
    res.CS.host[int(res.CS.idx[0])] += 1.0
    assert any(v.startswith("colsum:") for v in check(res).violations)


def test_checker_rejects_a_nan_and_a_nonzero_where_the_mass_is_zero(olib):
    for case, out in ((BWD_MAP, "dest1"), (BWD_SUM, "dx")):
        res, rep, check = _run(olib, case)
        buf = dict(res.outputs)[out]
        zeros = np.argwhere(rep.mass[out].reshape(buf.rows, buf.cols) == 0)
        assert len(zeros), "a stored, masked dx has elements without any term"
        at = buf.flat_index(*zeros[0])
        for v in (1e-30, -1e-30, np.nan):
            buf.host[at] = v
            assert any(s.startswith(out + ":") for s in check(res).violations), v
        buf.host[at] = 0.0
        assert check(res).ok()


def test_checker_reports_a_relu_masked_dy_that_is_not_exactly_zero(olib):
    res, rep, check = _run(olib, Case("live-relu", "bwd", 42, 70, 50, RELU, 0, lddy=72))
    masked = np.argwhere(res.inp["y"] <= 0)
    assert len(masked)
    at = res.DY.flat_index(*masked[0])
    for v in (1e-38, -1e-30, np.nan):
        res.DY.host[at] = v
        assert any(s.startswith("dy:") for s in check(res).violations), v
    res.DY.host[at] = 0.0
    assert check(res).ok()
    # and a kept element must be the incoming gradient bit for bit
    kept = np.argwhere(res.inp["y"] > 0)
    at = res.DY.flat_index(*kept[0])
    res.DY.host[at] = np.nextafter(res.DY.host[at], np.float32(4.0))
    assert any(s.startswith("dy:") for s in check(res).violations)


def test_integer_cases_are_held_to_exact_equality(olib):
    res, _, check = _run(olib, Case("int", "bwd", 66, 33, 128, RELU, OVERWRITE, integer=True))
    at = int(res.DW.idx[7])
    res.DW.host[at] = np.nextafter(res.DW.host[at], np.float32(1e9))
    assert any(s.startswith("dw:") for s in check(res).violations)


def test_empty_batch_and_refusals_on_the_oracle(olib):
    be = LH.HostBackend()
    for kind in ("fwd", "bwd"):
        res = (LH.run_fwd if kind == "fwd" else LH.run_bwd)(olib, be, Case("empty", kind, 70, 40, 0, RELU))
        assert res.rc == 0 and all(buf.untouched() for _, buf in res.outputs)
    for case in (Case("r", "bwd", 70, 40, 33, LH.GELU), Case("r", "bwd", 70, 40, 33, RELU, ONLY_DX | ONLY_DW), Case("r", "bwd", 70, 40, 33, RELU, lddy=39),
                 Case("r", "fwd", 70, 40, 33, RELU, ldx=69)):
        res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(olib, be, case)
        assert res.rc != 0 and all(buf.untouched() for _, buf in res.outputs), repr(case)
