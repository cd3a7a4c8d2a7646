"""GPU tests (-m gpu): ffh_linear_fwd / ffh_linear_bwd_ex in FFH_MATH_TENSOR_OP_BF16 swept against a float64 reference, route by route.

tests/linear_helpers.py holds the generator, the reference (float64 sums over operands rounded to bfloat16 by rne_bf16, written from
include/ff_hip.h), the twin buffers, the checker and the model of launch_gemm_bf16 / launch_gemm_bf16_dma's dispatch;
tests/test_linear_bf16_sweep_cpu.py proves them on the oracle library.  Here: the fixed edge table, every case on the kernel of csrc/linear_bf16.hip
or csrc/linear_bf16_dma.hip it is in the table for; 12 seeds of random cases; every case with twins once more without them; deterministic
mode, the same bits twice; stale twins; ffh_convert_f32_to_bf16 bit for bit; the empty batch, the refusals and the region limit.  Every bound is
TOL * mass * L + 8 * EPS32 * |ref| of linear_helpers, or exact equality.
"""
import time

import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import linear_helpers as LH
from linear_helpers import Case, RELU, MATH_BF16
from linear_helpers import REFUSALS, RNE_TABLE, NAN_PATTERNS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return LH.TorchBackend()


@pytest.fixture(autouse=True)
def _nothing_left_behind(hip, be):
    """After every test of this file the ctx is as a later test expects it: no registered region, and math mode 0 -- observed, not set: a wide
    layer on half-ulp operands, called without touching the mode, has to meet the fp32 bound against the UNROUNDED reference, which no
    rounding kernel does (test_checker_rejects_the_oracle_against_a_wrong_rounding).  Only after the verdict is the mode put back, so that
    a leak fails here and not in whichever test runs next."""
    yield
    torch.cuda.synchronize()
    try:
        left = 64 - _free_regions(hip)
        probe = Case("mode-probe", "fwd", 192, 136, 64, LH.NONE, dist="ties", bias=False)
        inp = LH.make_inputs(probe)
        X, W, Y = LH.Buf(be, 64, 192, 192, 0, inp["x"]), LH.Buf(be, 136, 192, 192, 0, inp["w"]), LH.Buf(be, 64, 136, 136, 0)
        rc = hip.lib.ffh_linear_fwd(hip.ctx, X.ptr, 192, Y.ptr, 136, W.ptr, None, 192, 136, 64, LH.NONE, None)
        route = (hip.lib.ffh_linear_last_route(hip.ctx) or b"").decode()
        torch.cuda.synchronize()
        Y.fetch()
        rep = LH.check_fwd(LH.Result(probe, inp, rc, route, Y=Y, outputs=[("y", Y)], inputs=[]))
    finally:
        hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0)
    assert left == 0, f"a test left {left} registered bf16 region(s) behind"
    assert rep.ok() and "bf16" not in route, f"a test left the math mode changed: route {route}\n{rep}"


def _free_regions(hip):
    """How many more regions the ctx takes (registered on one dummy allocation, all removed again)."""
    a, t = torch.zeros(64 * 4 + 8, device="cuda:0"), torch.zeros(8, dtype=torch.int16, device="cuda:0")
    n = 0
    try:
        while n < 70 and hip.lib.ffh_ctx_bf16_mirror_set(hip.ctx, a.data_ptr() + 16 * n, 16, t.data_ptr()) == 0:
            n += 1
    finally:
        for k in range(n):
            hip.lib.ffh_ctx_bf16_mirror_set(hip.ctx, a.data_ptr() + 16 * k, 16, None)
    return n


def _report_worst(t0):
    print(f"wall {time.time() - t0:.2f} s; worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(LH.WORST.items())})


def _run(hip, be, case, cus, routes=True):
    res, rep = LH.run_and_check(hip, be, case, cus, routes=routes)
    print(case.name, "route:", res.route, "worst:", {k: round(v, 3) for k, v in rep.worst.items()})
    assert rep.ok(), f"{case!r}\nroute {res.route}\n{rep}"
    return res


@pytest.mark.parametrize("name", LH.BF16_EDGE_NAMES)
def test_linear_bf16_edge_table(hip, be, name):
    """(a) and (c): every case on its kernel; a case with twins once more without them."""
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.bf16_edge_table(cus)[name]:
        res = _run(hip, be, case, cus)
        for out in res.case.stale:
            assert not np.isnan(res.DW.get()).any() and (res.DX is None or not np.isnan(res.DX.host[res.DX.idx]).any()), f"{case.name}: the stale twin of {out} was read"
        if not case.twins:
            continue
        bare = _run(hip, be, case.replace(twins=(), stale=(), want=()), cus)
        dma = "bf16_dma" in res.route + bare.route
        same_family = LH.normalize_route(res.route) == LH.normalize_route(bare.route)
        # y and dx come from one ordered sum per element: the same bits with and without twins, except on the LDS-DMA kernel, which sums in its
        # own order.  db is bit-comparable where one workgroup sums a column in order: deterministic mode only (otherwise the activation pass
        # and the LDS-DMA kernel both add partial sums by atomics).  dw likewise: outside deterministic mode every route splits K (at least
        # the forced two splits) and the splits meet by float atomics, whose order differs from run to run; it is held to the bound in both
        # runs by _run, as db is.  That covers the stale-twin cases too: their dw has splitk=2.
        for name_, buf in res.outputs:
            other = dict(bare.outputs)[name_]
            ordered = name_ in ("y", "dx") or (name_ in ("db", "dw") and case.det and all(t.endswith("splitk=1") for t in (res.route + ";" + bare.route).split(";") if "dw" in t.split("|")[0]))
            if ordered and not dma and (same_family or not case.stale):
                assert buf.get().tobytes() == other.get().tobytes(), f"{case.name}: {name_} differs between the run with twins and the run without"
    _report_worst(t0)


@pytest.mark.parametrize("seed", range(12))
def test_linear_bf16_random_cases(hip, be, seed):
    """(b) numbers, sentinels and twins only: no route is expected of a random case."""
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.draw_cases_bf16(seed):
        _run(hip, be, case, cus, routes=False)
    _report_worst(t0)


def test_linear_bf16_deterministic_mode_gives_the_same_bits_twice(hip, be):
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.bf16_edge_table(cus)["bf16-deterministic"]:
        assert case.det
        runs = [_run(hip, be, case, cus) for _ in range(2)]
        assert runs[0].DW.host.tobytes() == runs[1].DW.host.tobytes(), f"{case.name}: dw differs between two runs"
        if runs[0].DB is not None:
            assert runs[0].DB.host.tobytes() == runs[1].DB.host.tobytes(), f"{case.name}: db differs between two runs"
    _report_worst(t0)


def test_the_edge_table_reaches_every_bf16_pipe_token(hip):
    """At the CU count of this device the model (which test_linear_bf16_edge_table holds the library to) names every family for every GEMM."""
    cus = LH.num_cus(hip)
    seen = {t.split("|splitk")[0] for cs in LH.bf16_edge_table(cus).values() for c in cs for t in LH.expected_route(c, cus)[0]}
    print(cus, "CUs:", sorted(seen))
    if cus != LH.TABLE_CUS:
        return      # the table's shapes are derived for 256 CUs; on another device every case is still held to what the model says of that device
    for gemm in ("linear_fwd gemm (bf16)", "linear_bwd dx gemm (bf16)", "linear_bwd dw gemm (bf16)"):
        for fam in ("bf16_128x128", "bf16_256x256", "bf16_128x128_twins", "bf16_256x256_twins", "bf16_dma_256x256_twins"):
            assert f"{gemm}|{fam}" in seen or (gemm, fam) == ("linear_bwd dw gemm (bf16)", "bf16_256x256_twins"), (gemm, fam)
    assert "linear_bwd dw gemm (bf16)|bf16_dma_256x256_twins|slots" in seen
    assert {t for t in seen if "masking" in t} == {"linear_bwd dx gemm (bf16, masking)|bf16_128x128", "linear_bwd dx gemm (bf16, masking)|bf16_256x256"}


# ---------------------------------------------------------------------------------------------------------------------------
# (d) ffh_convert_f32_to_bf16
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (3, 2), (4, 4)])
def test_convert_f32_to_bf16_bit_for_bit(hip, src_off, dst_off):
    """Source 16-byte aligned or not, destination 8-byte aligned or not (vector path and element path), a sentinel round the destination."""
    rng = np.random.default_rng(src_off * 8 + dst_off)
    rand = rng.standard_normal(100003).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, 30, 100003).astype(np.float32)
    ties = ((rng.integers(0, 1 << 16, 4096).astype(np.uint32) << 16) | np.uint32(0x8000)).view(np.float32)
    table = np.array([a for a, _ in RNE_TABLE] + NAN_PATTERNS, np.uint32).view(np.float32)
    for vals in (table, np.concatenate([rand, ties, table])):
        n, pad = vals.size, 16
        src = torch.from_numpy(np.concatenate([np.zeros(src_off, np.float32), vals])).to("cuda:0")
        dst = torch.from_numpy(np.full(pad + dst_off + n + pad, LH.SENTINEL16, np.uint16).view(np.int16)).to("cuda:0")
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        hip.check(hip.lib.ffh_convert_f32_to_bf16(hip.ctx, dst.data_ptr() + 2 * (pad + dst_off), src.data_ptr() + 4 * src_off, n, None), "convert")
        torch.cuda.synchronize()
        got = dst.cpu().numpy().view(np.uint16)
        body, want = got[pad + dst_off:pad + dst_off + n], LH.rne_bf16_bits(vals)
        assert (got[:pad + dst_off] == LH.SENTINEL16).all() and (got[pad + dst_off + n:] == LH.SENTINEL16).all(), "written outside [dst, dst + count)"
        assert ((body[np.isnan(vals)] & 0x7FFF) > 0x7F80).all(), "a NaN did not stay a NaN"
        bad = np.flatnonzero(body != want)          # (NaN included: the quiet bit set, the upper payload kept, as rne_bf16_bits states it)
        assert bad.size == 0, f"{bad.size} of {n} differ; first: 0x{int(vals.view(np.uint32)[bad[0]]):08x} -> 0x{int(body[bad[0]]):04x}, expected 0x{int(want[bad[0]]):04x}"


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the empty batch, the refusals, the region limit
ALL_TWINS = dict(mode=MATH_BF16, twins=LH.TWIN_NAMES)


def test_linear_bf16_empty_batch_writes_nothing(hip, be):
    cus = LH.num_cus(hip)
    for kind in ("fwd", "bwd"):
        warm = _run(hip, be, Case("warm", kind, 192, 136, 8, RELU, **ALL_TWINS), cus)
        assert "bf16" in warm.route
        res = (LH.run_fwd if kind == "fwd" else LH.run_bwd)(hip, be, Case("empty", kind, 192, 136, 0, RELU, **ALL_TWINS))
        assert res.rc == capi.FFH_OK and res.route == "", (res.rc, res.route)
        for name, buf in res.outputs + list(res.twins.items()):
            assert buf.untouched(), f"{name} written by an empty call"


@pytest.mark.parametrize("reason", list(REFUSALS))
def test_linear_bf16_refusals_touch_nothing(hip, be, reason):
    """The refusals of the fp32 sweep on a wide layer in tensor-op mode with every twin registered: nothing is written, twins included."""
    case, want = REFUSALS[reason]
    pad = lambda ld, w, nw: None if ld is None else nw + (ld - w)
    kw = case._kw
    case = case.replace(in_dim=192, out_dim=136, ldx=pad(kw["ldx"], 70, 192), lddx=pad(kw["lddx"], 70, 192), ldy=pad(kw["ldy"], 40, 136), lddy=pad(kw["lddy"], 40, 136), **ALL_TWINS)
    res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(hip, be, case)
    assert res.rc == want, (reason, res.rc, hip.lib.ffh_last_error_string(hip.ctx))
    for name, buf in res.outputs:
        assert buf.untouched(), f"{reason}: {name} was written by a refused call"
    for name, tw in res.twins.items():
        assert tw.untouched(), f"{reason}: the twin of {name} was written by a refused call"


def test_bf16_region_limit_is_64(hip):
    """kMirrorRegions: the 65th registration is refused, removing one makes room, registering an existing base again replaces it."""
    lib, ctx = hip.lib, hip.ctx
    a = torch.zeros(66 * 8, device="cuda:0")
    t = torch.zeros(66 * 8, dtype=torch.int16, device="cuda:0")
    base, twin = (lambda k: a.data_ptr() + 32 * k), (lambda k: t.data_ptr() + 16 * k)
    try:
        for k in range(64):
            assert lib.ffh_ctx_bf16_mirror_set(ctx, base(k), 32, twin(k)) == 0, k
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(64), 32, twin(64)) == capi.FFH_ERR_UNSUPPORTED
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(7), 32, twin(65)) == 0            # an existing base: replaced, no new slot
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(64), 32, twin(64)) == capi.FFH_ERR_UNSUPPORTED
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(3), 32, None) == 0                # removing one makes room
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(64), 32, twin(64)) == 0
        assert lib.ffh_ctx_bf16_mirror_set(ctx, base(65), 32, twin(65)) == capi.FFH_ERR_UNSUPPORTED
    finally:
        for k in range(66):
            lib.ffh_ctx_bf16_mirror_set(ctx, base(k), 32, None)


def test_a_replaced_registration_is_the_one_in_force(hip, be):
    """Registering the base of y again with another twin: the forward writes the second twin and leaves the first alone."""
    case = Case("re", "fwd", 192, 136, 40, RELU, mode=MATH_BF16)
    inp = LH.make_inputs(case)
    X, W, Y = LH.Buf(be, 40, 192, 192, 0, inp["x"]), LH.Buf(be, 136, 192, 192, 0, inp["w"]), LH.Buf(be, 40, 136, 136, 0)
    first, second = LH.TwinBuf(be, Y), LH.TwinBuf(be, Y)
    ybase = be.addr(Y.h)
    try:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, MATH_BF16) == 0
        assert hip.lib.ffh_ctx_bf16_mirror_set(hip.ctx, ybase, 4 * Y.valid.size, first.base) == 0
        assert hip.lib.ffh_ctx_bf16_mirror_set(hip.ctx, ybase, 4 * Y.valid.size, second.base) == 0
        hip.check(hip.lib.ffh_linear_fwd(hip.ctx, X.ptr, 192, Y.ptr, 136, W.ptr, None, 192, 136, 40, RELU, None), "ffh_linear_fwd")
        torch.cuda.synchronize()
    finally:
        hip.lib.ffh_ctx_bf16_mirror_set(hip.ctx, ybase, 4, None)
        hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0)
    Y.fetch()
    assert first.fetch().untouched(), "the replaced twin was written"
    assert not second.fetch().problems("y", Y.get(), must_write=True)
