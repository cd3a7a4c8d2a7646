"""GPU tests (-m gpu): ffh_linear_fwd / ffh_linear_bwd_ex in FFH_MATH_FP32_SPLIT_BF16X3_ALL swept route by route, exact to the bit.

tests/linear_helpers.py holds the "planes" family (operands on which the six plane products and every partial sum are exact in fp32: y, dx and
dw have to EQUAL the float64 sum of the six kept products of the numpy planes, written from include/ff_hip.h), the three-plane image buffers,
the checker and the model of the split branch of launch_gemm_bf16 / launch_gemm_x3_dma; tests/test_linear_x3_sweep_cpu.py proves them without
the kernels.  Here: the fixed edge table, every case on the kernel of csrc/linear_bf16.hip or csrc/linear_x3_dma.hip it is in the table for
(gemm_bf16x3_kernel on both tiles, gemm_bf16x3_v2_kernel on four and eight waves, gemm_x3_dma_kernel in its three forms, x3_dw_reduce_kernel,
the conversion pass), a case with images once more without them (the same bits in y and dx); 8 seeds of random cases; deterministic mode, the
same bits twice.  The other distributions keep TOL * mass * L + 8 * EPS32 * |ref| of linear_helpers against the unsplit float64 product.
"""
import time

import numpy as np
import pytest
import torch

import linear_helpers as LH
from linear_helpers import Case, MATH_SPLIT_ALL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return LH.TorchBackend()


@pytest.fixture(autouse=True)
def _nothing_left_behind(hip, be):
    """After every test of this file the ctx is as a later test expects it: math mode 0 (observed on a "planes" forward, which an exact-fp32
    kernel computes differently from the split kernels in nearly every output -- and only then put back) and no registered region."""
    yield
    torch.cuda.synchronize()
    try:
        probe = Case("mode-probe", "fwd", 192, 136, 64, LH.NONE, dist="planes", bias=False, mode=MATH_SPLIT_ALL)
        inp = LH.make_inputs(probe)
        X, W, Y = LH.Buf(be, 64, 192, 192, 0, inp["x"]), LH.Buf(be, 136, 192, 192, 0, inp["w"]), LH.Buf(be, 64, 136, 136, 0)
        hip.check(hip.lib.ffh_linear_fwd(hip.ctx, X.ptr, 192, Y.ptr, 136, W.ptr, None, 192, 136, 64, LH.NONE, None), "ffh_linear_fwd")
        route = (hip.lib.ffh_linear_last_route(hip.ctx) or b"").decode()
        torch.cuda.synchronize()
        six = LH.split_product(inp["x"], inp["w"].T).astype(np.float32)
        left = 64 - _free_regions(hip)
    finally:
        hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0)
    assert "bf16" not in route and Y.fetch().get().tobytes() != six.tobytes(), f"a test left the math mode changed: route {route}"
    assert left == 0, f"a test left {left} registered region(s) behind"


def _free_regions(hip):
    """How many more regions the ctx takes (registered on one dummy allocation, all removed again)."""
    a, t = torch.zeros(70 * 32, device="cuda:0"), torch.zeros(70 * 128, dtype=torch.int16, device="cuda:0")
    n = 0
    try:
        while n < 70 and hip.lib.ffh_ctx_bf16x3_mirror_set(hip.ctx, a.data_ptr() + 128 * n, 128, t.data_ptr() + 256 * n) == 0:
            n += 1
    finally:
        for k in range(n):
            hip.lib.ffh_ctx_bf16x3_mirror_set(hip.ctx, a.data_ptr() + 128 * k, 128, None)
    return n


def _report_worst(t0):
    print(f"wall {time.time() - t0:.2f} s; worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(LH.WORST.items())})


def _run(hip, be, case, cus, routes=True):
    res, rep = LH.run_and_check_x3(hip, be, case, cus, routes=routes)
    print(case.name, case.dist, "route:", res.route, "worst:", {k: round(v, 3) for k, v in rep.worst.items()})
    assert rep.ok(), f"{case!r}\nroute {res.route}\n{rep}"
    return res


@pytest.mark.parametrize("name", LH.X3_EDGE_NAMES)
def test_linear_x3_edge_table(hip, be, name):
    """Every case on its kernel, the route asserted; a case with images once more without them."""
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.x3_edge_table(cus)[name]:
        res = _run(hip, be, case, cus)
        for out in res.case.stale:
            assert not np.isnan(res.DW.get()).any() and (res.DX is None or not np.isnan(res.DX.host[res.DX.idx]).any()), f"{case.name}: the stale image of {out} was read"
    _report_worst(t0)


@pytest.mark.parametrize("seed", range(8))
def test_linear_x3_random_cases(hip, be, seed):
    """Numbers, sentinels and images only: no route is expected of a random case."""
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.draw_cases_x3(seed):
        _run(hip, be, case, cus, routes=False)
    _report_worst(t0)


def test_linear_x3_deterministic_mode_gives_the_same_bits_twice(hip, be):
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.x3_edge_table(cus)["x3-deterministic"]:
        assert case.det
        runs = [_run(hip, be, case, cus) for _ in range(2)]
        assert runs[0].DW.host.tobytes() == runs[1].DW.host.tobytes(), f"{case.name}: dw differs between two runs"
        if runs[0].DB is not None:
            assert runs[0].DB.host.tobytes() == runs[1].DB.host.tobytes(), f"{case.name}: db differs between two runs"
    _report_worst(t0)


def test_the_edge_table_reaches_every_split_mode_kernel(hip):
    """At the CU count of this device the model (which test_linear_x3_edge_table holds the library to) names every kernel of the mode, each
    with a "planes" case."""
    cus = LH.num_cus(hip)
    toks = {(t, c.planes_exact) for cs in LH.x3_edge_table(cus).values() for c in cs for t in LH.expected_route(c, cus)[0]}
    print(cus, "CUs:", sorted({t for t, _ in toks}))
    if cus != LH.TABLE_CUS:
        return      # the table's shapes are derived for 256 CUs; on another device every case is still held to what the model says of that device
    for kernel, sub in LH.X3_KERNELS.items():
        assert any(sub in t and exact for t, exact in toks), f"no 'planes' case on {kernel}"
