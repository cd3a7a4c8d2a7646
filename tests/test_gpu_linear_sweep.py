"""GPU tests (-m gpu): ffh_linear_fwd / ffh_linear_bwd_ex swept against a float64 reference, route by route.

tests/linear_helpers.py holds the generator, the reference, the checker and the route model (tests/test_linear_sweep_cpu.py proves them on the
oracle library).  Here: the fixed edge table, every case on the kernel it is in the table for (ffh_linear_last_route against the model of the
dispatch, reached by shape alone); 12 seeds of random cases; deterministic mode, the same bits twice; the persistent, LDS-DMA and
register-staged groups once more in the split math mode at the same bound; a request that must not survive its call; the empty batch and the
refusals, which must not have written anything.
"""
import time

import pytest
import torch

from dlrm_flexflow_amd import capi
import linear_helpers as LH
from linear_helpers import Case, NONE, RELU, SIG, GELU, OVERWRITE, ONLY_DX, ONLY_DW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return LH.TorchBackend()


def _report_worst(t0):
    print(f"wall {time.time() - t0:.2f} s; worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(LH.WORST.items())})


def _run(hip, be, case, cus, routes=True):
    res, rep = LH.run_and_check(hip, be, case, cus, routes=routes)
    print(case.name, "route:", res.route, "worst:", {k: round(v, 3) for k, v in rep.worst.items()})
    assert rep.ok(), f"{case!r}\nroute {res.route}\n{rep}"
    return res


@pytest.mark.parametrize("name", LH.EDGE_NAMES)
def test_linear_edge_table(hip, be, name):
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.edge_table(cus)[name]:
        _run(hip, be, case, cus)
    _report_worst(t0)


@pytest.mark.parametrize("seed", range(12))
def test_linear_random_cases(hip, be, seed):
    """Numbers and sentinels only: no route is expected of a random case."""
    cus, t0 = LH.num_cus(hip), time.time()
    for case in LH.draw_cases(seed):
        _run(hip, be, case, cus, routes=False)
    _report_worst(t0)


def test_linear_deterministic_mode_gives_the_same_bits_twice(hip, be):
    """The skinny, persistent-dW, LDS-DMA-dW and atomic shapes on the ordered routes: within the bound, and dw / db bit for bit the same twice."""
    cus, t0 = LH.num_cus(hip), time.time()
    try:
        for case in LH.edge_table(cus)["bwd-deterministic"]:
            assert case.det
            runs = [_run(hip, be, case, cus) for _ in range(2)]
            assert runs[0].DW.host.tobytes() == runs[1].DW.host.tobytes(), f"{case.name}: dw differs between two runs"
            if runs[0].DB is not None:
                assert runs[0].DB.host.tobytes() == runs[1].DB.host.tobytes(), f"{case.name}: db differs between two runs"
    finally:
        hip.check(hip.lib.ffh_ctx_set_deterministic(hip.ctx, 0), "deterministic")
        torch.cuda.synchronize()
    _report_worst(t0)


@pytest.mark.parametrize("name", LH.SPLIT_MODE_GROUPS)
def test_linear_edge_table_in_the_split_math_mode(hip, be, name):
    """FFH_MATH_FP32_SPLIT_BF16X3_ALL at the same bound; which kernel serves a case is that mode's business."""
    cus, t0 = LH.num_cus(hip), time.time()
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, LH.MATH_SPLIT_ALL) == 0
    try:
        for case in LH.edge_table(cus)[name]:
            _run(hip, be, case, cus, routes=False)
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
        torch.cuda.synchronize()
    _report_worst(t0)


def test_linear_column_map_and_column_sums_do_not_survive_their_call(hip, be):
    """A declined request is spent: the same layer, called again as one that would qualify, stores its plain dx and leaves the old targets alone."""
    cus = LH.num_cus(hip)
    first = _run(hip, be, Case("declined", "bwd", 42, 70, 100, NONE, 0, cmap=True, colsum=True), cus)
    assert first.scatter_used == 0 and first.colsum_used == 0
    second = _run(hip, be, Case("next", "bwd", 42, 70, 100, NONE, OVERWRITE), cus)
    assert second.scatter_used == 0 and second.colsum_used == 0
    for buf in first.dests + [first.CS]:
        assert buf.fetch().untouched(), "a request of the call before was served by this one"


def test_linear_empty_batch_writes_nothing(hip, be):
    cus = LH.num_cus(hip)
    for kind in ("fwd", "bwd"):
        warm = _run(hip, be, Case("warm", kind, 70, 40, 8, RELU), cus)      # a served call first, so that an empty route is the empty call's own
        assert warm.route
        res = (LH.run_fwd if kind == "fwd" else LH.run_bwd)(hip, be, Case("empty", kind, 70, 40, 0, RELU))
        assert res.rc == capi.FFH_OK
        assert res.route == "", res.route
        for name, buf in res.outputs:
            assert buf.untouched(), f"{name} written by an empty call"


BAD_ARG, UNSUPPORTED = capi.FFH_ERR_BAD_ARG, capi.FFH_ERR_UNSUPPORTED
REFUSALS = LH.REFUSALS          # (shared with the tensor-op sweep)


@pytest.mark.parametrize("reason", list(REFUSALS))
def test_linear_refusals_touch_nothing(hip, be, reason):
    case, want = REFUSALS[reason]
    res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(hip, be, case)
    assert res.rc == want, (reason, res.rc, hip.lib.ffh_last_error_string(hip.ctx))
    for name, buf in res.outputs:
        assert buf.untouched(), f"{reason}: {name} was written by a refused call"


@pytest.mark.parametrize("null", ["x", "w", "y", "dy", "dw", "fwd-x", "fwd-w", "fwd-y"])
def test_linear_null_operands_are_refused(hip, be, null):
    lib, z = hip.lib, torch.full((40 * 70 + 8,), float("nan"), device="cuda:0")
    p = {k: z.data_ptr() for k in ("x", "w", "y", "dy", "dw")}
    if null.startswith("fwd-"):
        p[null[4:]] = None
        rc = lib.ffh_linear_fwd(hip.ctx, p["x"], 70, p["y"], 40, p["w"], None, 70, 40, 1, RELU, None)
    else:
        p[null] = None
        rc = lib.ffh_linear_bwd_ex(hip.ctx, p["x"], 70, None, 70, p["y"], 40, p["dy"], 40, p["w"], p["dw"], None, 70, 40, 1, RELU, 0, None, None)
    torch.cuda.synchronize()
    assert rc == BAD_ARG, (null, rc)
    assert bool(torch.isnan(z).all()), "a call with a null operand wrote something"
