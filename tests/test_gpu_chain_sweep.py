"""GPU tests (-m gpu): the fused MLP-chain kernels of csrc/mlp_chain.hip swept against a float64 reference.

tests/chain_helpers.py holds the generator, the reference and the checker (tests/test_chain_sweep_cpu.py proves them on the oracle library).
Here: the fixed edge table (every branch of ffh_mlp_chain_fwd / _bwd that the workload's own widths do not reach), 12 seeds of random shapes,
deterministic mode, the split math mode, the refusals -- which must not have written anything -- and the empty batch.
"""
import pytest
import torch

from dlrm_flexflow_amd import capi
import chain_helpers as CH
from chain_helpers import Case, RELU, SIG, GELU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return CH.TorchBackend()


def _report_worst():
    print("worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(CH.WORST.items())})


@pytest.mark.parametrize("name", CH.EDGE_NAMES)
def test_chain_edge_table(hip, be, name):
    cus = CH.num_cus(hip)
    for case in CH.edge_table(cus)[name]:
        res, rep = CH.run_and_check(hip, be, case, cus)
        print(case.name, "route:", res.route, "worst:", {k: round(v, 3) for k, v in rep.worst.items()})
        assert rep.ok(), f"{case!r}\nroute {res.route}\n{rep}"
    _report_worst()


@pytest.mark.parametrize("seed", range(12))
def test_chain_random_shapes(hip, be, seed):
    cus = CH.num_cus(hip)
    for case in CH.draw_cases(seed, cus):
        res, rep = CH.run_and_check(hip, be, case, cus)
        print(case.name, case.kind, case.widths, case.batch, "route:", res.route)
        assert rep.ok(), f"{case!r}\nroute {res.route}\n{rep}"
    _report_worst()


def test_chain_sweep_in_deterministic_mode(hip, be):
    """The weight-gradient blocks meet in the stream's scratch and are added in split order: within the bound, and the same bits twice."""
    cus = CH.num_cus(hip)
    table = CH.edge_table(cus)
    cases = [table[k][1] for k in ("eight-layers", "strides", "tiny-batch-65")]
    hip.check(hip.lib.ffh_ctx_reserve_scratch(hip.ctx, None), "scratch")          # (the null stream's; idempotent)
    hip.check(hip.lib.ffh_ctx_set_deterministic(hip.ctx, 1), "deterministic")
    try:
        for case in cases:
            assert case.kind == "bwd"
            runs = []
            for rep_no in range(2):
                res, rep = CH.run_and_check(hip, be, case, cus, ordered=True)
                assert rep.ok(), f"{case!r} (run {rep_no})\nroute {res.route}\n{rep}"
                assert "|ordered" in res.route, res.route
                runs.append(res)
            for l in range(case.n):
                assert runs[0].DW[l].host.tobytes() == runs[1].DW[l].host.tobytes(), f"{case.name}: dw{l} differs between two runs"
                if runs[0].DB[l] is not None:
                    assert runs[0].DB[l].host.tobytes() == runs[1].DB[l].host.tobytes(), f"{case.name}: db{l} differs between two runs"
    finally:
        hip.check(hip.lib.ffh_ctx_set_deterministic(hip.ctx, 0), "deterministic")
        torch.cuda.synchronize()


def test_chain_in_split_mode_proper_is_the_fp32_chain(hip, be):
    """FFH_MATH_FP32_SPLIT_BF16X3 (proper) leaves layers this small to the exact kernels: the chain is served, and computes mode 0's bits."""
    cus = CH.num_cus(hip)
    case = Case("split-mode/fwd", "fwd", (24, 136, 260, 16), (RELU, GELU, SIG), 150, ldy=[140, 260, 20])
    ref = CH.run_fwd(hip, be, case)
    assert CH.check_fwd(ref).ok() and not CH.check_route(ref, cus)
    assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 2) == 0
    try:
        res, rep = CH.run_and_check(hip, be, case, cus)
        assert rep.ok(), f"route {res.route}\n{rep}"
        for l in range(case.n):
            assert res.Y[l].host.tobytes() == ref.Y[l].host.tobytes(), f"y{l} in the split mode is not the fp32 chain's"
    finally:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: the return code, and nothing written
BASE = dict(widths=(32, 64, 16), acts=(RELU, RELU), batch=40, want_dx=True, overwrite=True)


def _bwd(**kw):
    d = dict(BASE)
    d.update(kw)
    return Case("refusal", "bwd", d.pop("widths"), d.pop("acts"), d.pop("batch"), **d)


UNSUPPORTED, BAD_ARG = capi.FFH_ERR_UNSUPPORTED, capi.FFH_ERR_BAD_ARG
REFUSALS = {
    # reason: (case, math mode, expected return code)
    "top-out-dim-not-multiple-of-4": (lambda: _bwd(widths=(32, 64, 14)), 0, UNSUPPORTED),
    "inner-in-dim-not-multiple-of-4": (lambda: _bwd(widths=(32, 62, 16)), 0, UNSUPPORTED),
    "first-in-dim-not-multiple-of-4-with-dx": (lambda: _bwd(widths=(30, 64, 16), ldx=32, lddx=32, ldw=[32, 64]), 0, UNSUPPORTED),
    "ldw-not-multiple-of-4": (lambda: _bwd(ldw=[32, 65]), 0, UNSUPPORTED),
    "misaligned-w": (lambda: _bwd(w_off=[0, 1]), 0, UNSUPPORTED),
    "misaligned-dy": (lambda: _bwd(dy_off=[1, 0]), 0, UNSUPPORTED),
    "misaligned-y": (lambda: _bwd(y_off=[0, 1]), 0, UNSUPPORTED),
    "misaligned-dx": (lambda: _bwd(dx_off=1), 0, UNSUPPORTED),
    "lddy-not-multiple-of-4": (lambda: _bwd(lddy=[64, 18]), 0, UNSUPPORTED),
    "lddx-not-multiple-of-4": (lambda: _bwd(lddx=34), 0, UNSUPPORTED),
    "misaligned-x-with-mask-by-x": (lambda: _bwd(x_off=1, mask_by_x=True), 0, UNSUPPORTED),
    "gelu-at-the-top": (lambda: _bwd(acts=(RELU, GELU)), 0, UNSUPPORTED),
    "inner-sigmoid": (lambda: _bwd(acts=(SIG, RELU)), 0, UNSUPPORTED),
    "math-mode-1": (lambda: _bwd(), 1, UNSUPPORTED),
    "math-mode-3": (lambda: _bwd(), 3, UNSUPPORTED),
    "width-513": (lambda: _bwd(widths=(32, 513, 16)), 0, BAD_ARG),
    "nine-layers": (lambda: _bwd(widths=(32,) * 10, acts=(RELU,) * 9), 0, BAD_ARG),
    "ldw-below-in-dim": (lambda: _bwd(ldw=[32, 60]), 0, BAD_ARG),
    "unknown-flag-bit": (lambda: _bwd(extra_flags=64), 0, BAD_ARG),
}


@pytest.mark.parametrize("reason", list(REFUSALS))
def test_chain_refusals_touch_nothing(hip, be, reason):
    mk, mode, want = REFUSALS[reason]
    case = mk()
    cus = CH.num_cus(hip)
    if mode:
        assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, mode) == 0
    try:
        res = CH.run_bwd(hip, be, case)
        if mode or want == BAD_ARG:       # the forward has the same rule
            fcase = Case("refusal/fwd", "fwd", case.widths, case.acts, case.batch, ldw=case.ldw)
            fres = CH.run_fwd(hip, be, fcase) if reason != "unknown-flag-bit" else None
    finally:
        if mode:
            assert hip.lib.ffh_ctx_set_math_mode(hip.ctx, 0) == 0
    assert res.rc == want, (reason, res.rc, hip.lib.ffh_last_error_string(hip.ctx))
    for name, buf in res.outputs:
        assert buf.untouched(), f"{reason}: {name} was written by a refused call"
    if (mode or want == BAD_ARG) and reason != "unknown-flag-bit":
        assert fres.rc == want, (reason, "forward", fres.rc)
        for name, buf in fres.outputs:
            assert buf.untouched(), f"{reason}: {name} was written by a refused forward"
    if reason == "first-in-dim-not-multiple-of-4-with-dx":      # the complement: the same chain is served when its dx is discarded
        served = _bwd(widths=case.widths, ldx=case.ldx, ldw=case.ldw, want_dx=False)
        sres, rep = CH.run_and_check(hip, be, served, cus)
        assert rep.ok(), f"{served!r}\nroute {sres.route}\n{rep}"


def test_chain_empty_batch_writes_nothing(hip, be):
    for kind in ("fwd", "bwd"):
        case = Case("empty", kind, (32, 64, 16), (RELU, RELU), 0, want_dx=(kind == "bwd"), overwrite=True)
        # a served call first, so that an empty route is the empty call's own
        warm = Case("warm", kind, (32, 64, 16), (RELU, RELU), 8, want_dx=(kind == "bwd"), overwrite=True)
        wres, rep = CH.run_and_check(hip, be, warm, CH.num_cus(hip))
        assert rep.ok() and wres.route
        res = (CH.run_fwd if kind == "fwd" else CH.run_bwd)(hip, be, case)
        assert res.rc == capi.FFH_OK
        assert res.route == "", res.route
        for name, buf in res.outputs:
            assert buf.untouched(), f"{name} written by an empty call"
