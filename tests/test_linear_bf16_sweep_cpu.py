"""The tensor-op (bf16) Linear sweep's harness (tests/linear_helpers.py, Case.mode = 1), proved on a CPU.

The oracle library in FFH_MATH_TENSOR_OP_BF16 has to pass every mode-1 edge case (the shapes of a 256-CU device) and six seeds of the random
generator under the sweep's own bound against the float64 reference over nearest-even-rounded operands, which is written from the header and
calls neither the oracle nor a kernel.  The rounding is pinned to a table of bit patterns written by hand.  The route model has to send every
case to the kernel family it names.  And the checker has to be able to fail: against the unrounded reference, a truncating and a half-away
rounding the oracle's own outputs violate the bound, and a write anywhere outside an output's twin block, or a wrong row of it, is reported.
"""
import numpy as np
import pytest

import linear_helpers as LH
from linear_helpers import Case, NONE, RELU, SIG, OVERWRITE, ONLY_DW, MATH_BF16


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


@pytest.mark.parametrize("name", LH.BF16_EDGE_NAMES)
def test_oracle_passes_the_bf16_edge_table(olib, name):
    be = LH.HostBackend()
    cases = LH.bf16_edge_table(LH.TABLE_CUS)[name]
    assert cases
    for case in cases:
        assert case.mode == MATH_BF16
        res, rep = LH.run_and_check(olib, be, case, LH.TABLE_CUS)
        assert rep.ok(), f"{case!r}\n{rep}"
        assert all(tw.untouched() for n, tw in res.twins.items() if n not in res.twin_inputs)      # the oracle's registration is a no-op
    print({k: round(v, 4) for k, v in sorted(LH.WORST.items())})


@pytest.mark.parametrize("seed", range(6))
def test_oracle_passes_the_bf16_random_sweep(olib, seed):
    be = LH.HostBackend()
    cases = LH.draw_cases_bf16(seed)
    assert len(cases) == 6
    for case in cases:
        _, rep = LH.run_and_check(olib, be, case, LH.TABLE_CUS)
        assert rep.ok(), f"{case!r}\n{rep}"


def test_the_mode_does_not_outlive_a_call(olib, monkeypatch):
    """run_fwd / run_bwd put the mode back to 0 whatever happens: the fp32 result of a wide layer, bit for bit, after a mode-1 call that raised."""
    be = LH.HostBackend()
    wide = Case("after", "fwd", 192, 136, 50, NONE)
    first = LH.run_fwd(olib, be, wide)
    in_mode = LH.run_fwd(olib, be, wide.replace(mode=MATH_BF16, twins=("x", "w", "y")))
    assert in_mode.Y.host.tobytes() != first.Y.host.tobytes()
    assert LH.run_fwd(olib, be, wide).Y.host.tobytes() == first.Y.host.tobytes()

    def boom(*a):
        raise RuntimeError("after the call, before the clean-up")
    for run, case in ((LH.run_fwd, wide), (LH.run_bwd, Case("after", "bwd", 192, 136, 50, NONE, det=True))):
        with monkeypatch.context() as m:
            m.setattr(LH, "_finish", boom)
            with pytest.raises(RuntimeError):
                run(olib, be, case.replace(mode=MATH_BF16, twins=("x", "w")))
        assert LH.run_fwd(olib, be, wide).Y.host.tobytes() == first.Y.host.tobytes()


def test_generator_reaches_every_distribution_twin_and_width_class():
    cases = [c for s in range(12) for c in LH.draw_cases_bf16(s)]
    assert {c.dist for c in cases} == set(LH.DISTS) and all(c.mode == MATH_BF16 for c in cases)
    assert {n for c in cases for n in c.twins} == set(LH.TWIN_NAMES) and any(not c.twins for c in cases)
    assert sum(c.bf16_layer for c in cases) >= 12 and sum(not c.bf16_layer for c in cases) >= 8
    for c in cases:
        assert c.ldx >= c.in_dim and c.ldy >= c.out_dim and c.lddy >= c.out_dim and c.lddx >= c.in_dim


def test_route_model_sends_every_bf16_case_to_its_kernel_and_the_table_names_every_family():
    reached = set()
    for name, cases in LH.bf16_edge_table(LH.TABLE_CUS).items():
        for case in cases:
            assert case.want, f"{case.name} names no kernel"
            assert not LH.model_reaches(case), f"{case.name}: the route model gives {LH.expected_route(case, LH.TABLE_CUS)}, the case is there for {case.want}"
            reached.update(t.split("|splitk")[0] for t in LH.expected_route(case, LH.TABLE_CUS)[0])
    fams = ("bf16_128x128", "bf16_256x256", "bf16_128x128_twins", "bf16_256x256_twins", "bf16_dma_256x256_twins")
    for gemm in ("linear_fwd gemm (bf16)", "linear_bwd dx gemm (bf16)", "linear_bwd dw gemm (bf16)"):
        for fam in fams:
            if gemm.startswith("linear_bwd dw") and fam == "bf16_256x256_twins":
                continue      # not reachable: whenever both twins serve a weight gradient of >= 32 tiles and batch >= 8192, the LDS-DMA kernel's own conditions hold as well
            assert f"{gemm}|{fam}" in reached, (gemm, fam)
    assert "linear_bwd dw gemm (bf16)|bf16_dma_256x256_twins|slots" in reached
    masking = {t for t in reached if "masking" in t}         # the twins forms are closed to it (launch_gemm_bf16: !MASK_A)
    assert masking == {"linear_bwd dx gemm (bf16, masking)|bf16_128x128", "linear_bwd dx gemm (bf16, masking)|bf16_256x256"}, masking
    # the forced empty second split, the deterministic single split, and a split that the search chose
    routes = [LH.expected_route(c, LH.TABLE_CUS)[0] for cs in LH.bf16_edge_table().values() for c in cs]
    toks = {t for r in routes for t in r}
    assert {"linear_bwd dw gemm (bf16)|bf16_128x128|splitk=1", "linear_bwd dw gemm (bf16)|bf16_128x128|splitk=2", "linear_bwd dw gemm (bf16)|bf16_128x128|splitk=5",
            "linear_bwd dw gemm (bf16)|bf16_256x256|splitk=13", "linear_bwd dw gemm (bf16)|bf16_128x128_twins|splitk=64"} <= toks


def test_weight_gradient_on_big_twin_tiles_always_goes_to_the_lds_dma_kernel():
    """The predicate behind the one family the table cannot reach (bf16_256x256_twins for dW), tried over a grid of shapes at 256 CUs."""
    for o in (1024, 1032, 2048, 4096):
        for i in (1800, 2048, 4096):
            for B in (8192, 8256, 32768):
                c = Case("p", "bwd", i, o, B, NONE, ONLY_DW, mode=MATH_BF16, twins=("x", "dy"))
                tok = LH.expected_route(c, 256)[0][0]
                assert "bf16_dma_256x256_twins" in tok, tok


# ---------------------------------------------------------------------------------------------------------------------------
# the rounding, against bit patterns written by hand (linear_helpers.RNE_TABLE, NAN_PATTERNS)
RNE_TABLE, NAN_PATTERNS = LH.RNE_TABLE, LH.NAN_PATTERNS


def test_rne_bf16_against_the_hand_written_table():
    src = np.array([a for a, _ in RNE_TABLE], np.uint32).view(np.float32)
    got = LH.rne_bf16_bits(src)
    for (a, want), g in zip(RNE_TABLE, got):
        assert int(g) == want, f"0x{a:08x} -> 0x{int(g):04x}, expected 0x{want:04x}"
    nan = LH.rne_bf16_bits(np.array(NAN_PATTERNS, np.uint32).view(np.float32))
    assert all((int(v) & 0x7FFF) > 0x7F80 for v in nan), [hex(int(v)) for v in nan]
    assert np.isnan(LH.rne_bf16(np.array(NAN_PATTERNS, np.uint32).view(np.float32))).all()
    back = LH.rne_bf16(src)
    assert back[7] == 2.0 and np.isinf(back[10]) and back[10] > 0 and np.isinf(back[11]) and back[11] < 0
    assert np.signbit(back[17]) and back[17] == 0 and not np.signbit(back[16])
    # and the two wrong roundings differ from it where they should
    assert LH.trunc_bf16(src)[4].view(np.uint32) >> 16 == 0x3F81 and LH.half_away_bf16(src)[3].view(np.uint32) >> 16 == 0x3F81


def test_the_oracle_converts_as_rne_bf16(olib):
    src = np.concatenate([np.array([a for a, _ in RNE_TABLE], np.uint32).view(np.float32), np.random.default_rng(3).standard_normal(1001).astype(np.float32)])
    dst = np.zeros(src.size, np.uint16)
    assert olib.lib.ffh_convert_f32_to_bf16(olib.ctx, dst.ctypes.data, src.ctypes.data, src.size, None) == 0
    assert dst.tobytes() == LH.rne_bf16_bits(src).tobytes()


def test_the_ties_distribution_is_what_it_says():
    inp = LH.make_inputs(Case("t", "bwd", 192, 136, 200, NONE, OVERWRITE, dist="ties", mode=MATH_BF16))
    for k in ("x", "w", "g"):
        bits = inp[k].view(np.uint32)
        assert ((bits & 0xFFFF) == 0x8000).all() and np.isfinite(inp[k]).all()
        up = LH.rne_bf16(inp[k]) != LH.trunc_bf16(inp[k])
        assert 0.4 < up.mean() < 0.6                                                   # nearest-even goes up on the odd half
        assert (LH.half_away_bf16(inp[k]) != LH.rne_bf16(inp[k])).mean() > 0.4 and (np.abs(inp[k]) < 4).all()
    wide = LH.make_inputs(Case("w", "fwd", 257, 129, 130, NONE, dist="wide", mode=MATH_BF16))["x"]
    carried = (LH.rne_bf16_bits(wide) & 0x7F) == 0
    assert (carried & ((wide.view(np.uint32) >> 16) & 0x7F == 0x7F)).any(), "no rounding that carries into the exponent"


# ---------------------------------------------------------------------------------------------------------------------------
# the checker discriminates: the oracle's mode-1 outputs against three wrong references
WRONG = {"unrounded": lambda a: a, "truncating": LH.trunc_bf16, "half-away": LH.half_away_bf16}
DISCRIMINATE = [
    (Case("disc/fwd-ties", "fwd", 192, 136, 200, NONE, dist="ties", mode=MATH_BF16), "y", ("unrounded", "truncating", "half-away")),
    (Case("disc/fwd-uniform", "fwd", 192, 136, 200, RELU, mode=MATH_BF16), "y", ("unrounded", "truncating")),
    (Case("disc/bwd-uniform", "bwd", 192, 136, 200, NONE, OVERWRITE, mode=MATH_BF16), "dw dx", ("unrounded", "truncating")),
    (Case("disc/bwd-ties", "bwd", 192, 136, 200, NONE, OVERWRITE, dist="ties", mode=MATH_BF16), "dw dx", ("unrounded", "truncating", "half-away"))]


@pytest.mark.parametrize("case,outs,wrongs", DISCRIMINATE, ids=[c.name for c, _, _ in DISCRIMINATE])
def test_checker_rejects_the_oracle_against_a_wrong_rounding(olib, case, outs, wrongs):
    be = LH.HostBackend()
    res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(olib, be, case)
    check = LH.check_fwd if case.kind == "fwd" else LH.check_bwd
    assert check(res).ok(), str(check(res))
    for wrong in wrongs:
        rep = check(res, rnd=WRONG[wrong])
        for out in outs.split():
            assert any(v.startswith(out + ":") for v in rep.violations), f"{case.name}: {out} passes against the {wrong} reference\n{rep}"


def test_checker_holds_a_narrow_layer_to_the_unrounded_reference(olib):
    """in_dim 127: mode 1 changes nothing, and outputs computed from rounded operands (a kernel that rounds where it must not) are rejected."""
    be = LH.HostBackend()
    case = Case("narrow", "fwd", 127, 256, 100, NONE, mode=MATH_BF16)
    res = LH.run_fwd(olib, be, case)
    assert LH.check_fwd(res).ok()
    rounded = LH.rne_bf16(res.inp["x"]).astype(np.float64) @ LH.rne_bf16(res.inp["w"]).astype(np.float64).T + res.inp["b"]
    res.Y.host[res.Y.idx] = rounded.astype(np.float32).ravel()
    assert any(v.startswith("y:") for v in LH.check_fwd(res).violations)


# ---------------------------------------------------------------------------------------------------------------------------
# TwinBuf on its own
def _twin(ld=13, off=2):
    be = LH.HostBackend()
    data = np.random.default_rng(5).uniform(-1, 1, (7, 10)).astype(np.float32)
    buf = LH.Buf(be, 7, 10, ld, off, data)
    return buf, LH.TwinBuf(be, buf), data


def test_twinbuf_layout_and_fill(olib):
    buf, tw, data = _twin()
    assert tw.before.size == buf.valid.size and (tw.before == LH.SENTINEL16).all() and (LH.SENTINEL16 & 0x7FFF) > 0x7F80
    tw.fill(olib).fetch()
    assert (tw.host[~tw.valid] == LH.SENTINEL16).all() and (~tw.valid).sum() == 2 + 6 * 3 + 3 + LH.TAIL
    assert tw.host[tw.idx].tobytes() == LH.rne_bf16_bits(data).tobytes()
    # the twin of the float at p is twin_base + (p - fp32_base) / 2
    r, c = 4, 7
    p = buf.ptr + 4 * (r * buf.ld + c)
    at = (tw.base + (p - buf.be.addr(buf.h)) // 2 - tw.base) // 2
    assert tw.host[at] == LH.rne_bf16_bits(data[r, c])
    tw.snapshot()
    assert tw.fetch().untouched() and not tw.problems("x")
    tw.poison().fetch()
    assert (tw.host[tw.idx] == 0x7FC0).all() and (tw.host[~tw.valid] == LH.SENTINEL16).all()


def test_twinbuf_reports_a_write_at_padding_offset_tail_and_a_wrong_row():
    buf, tw, data = _twin()
    tw.fetch()
    assert not tw.problems("y", data) and not tw.problems("y", data, must_write=False)
    assert tw.problems("y", data, must_write=True), "an unwritten twin on a bf16 route went unnoticed"
    good = tw.before.copy()
    good[tw.idx] = LH.rne_bf16_bits(data).ravel()
    tw.host = good.copy()
    assert not tw.problems("y", data, must_write=True)
    places = {"offset": 0, "padding": buf.flat_index(2, 10), "last padding column": buf.flat_index(6, 12), "tail": good.size - 1, "behind the last row": buf.flat_index(6, 9) + 1}
    for what, at in places.items():
        assert not tw.valid[at], what
        tw.host = good.copy()
        tw.host[at] = 0x3F80
        assert any("padding" in p for p in tw.problems("y", data)), what
    tw.host = good.copy()
    tw.host[tw.idx.reshape(7, 10)[3]] = good[tw.idx.reshape(7, 10)[4]]          # row 3 holds row 4's values
    assert any("not the nearest-even rounding" in p and "(3, 0)" in p for p in tw.problems("y", data))
    tw.host = good.copy()
    tw.host[tw.idx.reshape(7, 10)[5]] = LH.SENTINEL16                            # a row left out: partly written
    assert any("(5, 0)" in p for p in tw.problems("y", data))
    tw.host = good.copy()
    tw.host[tw.idx[11]] ^= 1                                                     # one element rounded the other way
    assert any("(1, 1)" in p for p in tw.problems("y", data))
    tw.host = good.copy()
    assert any("input" in p for p in tw.problems("x"))                           # an input's twin has to stay as it was


def test_checker_reports_a_twin_written_by_the_wrong_rule_on_a_result(olib):
    """Through check_fwd / check_bwd, with the result marked as the HIP library's: an untouched output twin on a bf16 route, a truncated one."""
    be = LH.HostBackend()
    res = LH.run_fwd(olib, be, Case("tw", "fwd", 192, 136, 40, NONE, mode=MATH_BF16, twins=("x", "w", "y"), ldy=139, y_off=1))
    assert LH.check_fwd(res).ok()
    res.is_hip, res.route = True, "linear_fwd gemm (bf16)|bf16_128x128|splitk=1"
    assert any(v.startswith("y twin: not written") for v in LH.check_fwd(res).violations)
    tw = res.twins["y"]
    tw.host = tw.before.copy()
    tw.host[tw.idx] = (LH.trunc_bf16(res.Y.get()).view(np.uint32) >> 16).astype(np.uint16).ravel()
    assert any(v.startswith("y twin:") and "nearest-even" in v for v in LH.check_fwd(res).violations)
    tw.host[tw.idx] = LH.rne_bf16_bits(res.Y.get()).ravel()
    assert LH.check_fwd(res).ok()
    res.twins["x"].host = res.twins["x"].host.copy()
    res.twins["x"].host[res.twins["x"].idx[3]] ^= 0x10
    assert any(v.startswith("x twin:") for v in LH.check_fwd(res).violations)
    res = LH.run_bwd(olib, be, Case("tw", "bwd", 192, 136, 40, SIG, ONLY_DW, mode=MATH_BF16, twins=("x", "dy", "dx")))
    assert LH.check_bwd(res).ok()
    res.twins["dx"].host = res.twins["dx"].host.copy()
    res.twins["dx"].host[res.twins["dx"].idx[0]] = 0
    assert any(v.startswith("dx twin:") for v in LH.check_bwd(res).violations)      # ONLY_DW: the twin of dx has to stay untouched too
