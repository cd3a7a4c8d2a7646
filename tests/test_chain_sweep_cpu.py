"""The chain sweep's harness (tests/chain_helpers.py), proved on a CPU.

The oracle library is an independent float32 implementation of ffh_mlp_chain_fwd / _bwd: it has to pass the fixed edge table and 20 seeds of the
random generator under the sweep's own bound (1e-5 of the term mass, no absolute floor), no case skipped -- so the float64 reference, the
generator and the tolerance are sound before a GPU sees them.  And the checker has to be able to fail: one element of one output moved by
3e-5 of its term mass, and one overwritten padding element, are both reported.
"""
import numpy as np
import pytest

import chain_helpers as CH


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


@pytest.mark.parametrize("name", CH.EDGE_NAMES)
def test_oracle_passes_the_edge_table(olib, name):
    be, cus = CH.HostBackend(), CH.num_cus(olib)
    cases = CH.edge_table(cus)[name]
    assert cases
    for case in cases:
        _, rep = CH.run_and_check(olib, be, case, cus)
        print(case.name, {k: round(v, 3) for k, v in rep.worst.items()})
        assert rep.ok(), f"{case!r}\n{rep}"


@pytest.mark.parametrize("seed", range(20))
def test_oracle_passes_the_random_sweep(olib, seed):
    be, cus = CH.HostBackend(), CH.num_cus(olib)
    cases = CH.draw_cases(seed, cus)
    assert len(cases) == 6 and cases[0].batch >= 32 * cus and max(cases[0].widths) <= 128
    for case in cases:
        assert 1 <= case.n <= CH.MAX_LAYERS and all(1 <= w <= CH.MAX_WIDTH for w in case.widths)
        _, rep = CH.run_and_check(olib, be, case, cus)
        assert rep.ok(), f"{case!r}\n{rep}"


def test_generator_reaches_what_it_is_meant_to_reach():
    """Over the GPU sweep's 12 seeds: both kinds, one and eight layers, widths that are not multiples of 4 / 16, every tile count per wave, null
    bias and db, padded leading dimensions, misaligned forward operands, every flag."""
    cases = [c for s in range(12) for c in CH.draw_cases(s, 256)]
    fwd, bwd = [c for c in cases if c.kind == "fwd"], [c for c in cases if c.kind == "bwd"]
    assert len(fwd) >= 12 and len(bwd) >= 12
    assert {1, CH.MAX_LAYERS} <= {c.n for c in cases}
    tpw = {(((w + 15) // 16) + 7) // 8 for c in cases for w in c.widths[1:]}
    assert tpw == {1, 2, 3, 4}
    assert any(w % 4 for c in fwd for w in c.widths) and any(w % 16 for c in bwd for w in c.widths[1:])
    assert any(not all(c.bias) for c in fwd) and any(not all(c.db) for c in bwd)
    assert any(c.x_off % 4 for c in fwd) and any(o % 4 for c in fwd for o in c.y_off) and any(o % 4 for c in fwd for o in c.w_off)
    assert any(c.ldx > c.widths[0] for c in cases) and any(ld > w for c in bwd for ld, w in zip(c.lddy, c.widths[1:]))
    assert any(ld > w for c in cases for ld, w in zip(c.ldw, c.widths[:-1])) and any(c.lddx > c.widths[0] for c in bwd if c.want_dx)
    for flag in ("overwrite", "mask_by_x", "premasked", "want_dx"):
        assert {bool(getattr(c, flag)) for c in bwd} == {True, False}, flag
    for c in bwd:       # inside the served contract
        assert all(w % 4 == 0 for w in c.widths[1:]) and all(ld % 4 == 0 for ld in c.ldy + c.lddy) and not any(c.y_off + c.dy_off)
        if c.want_dx:
            assert c.widths[0] % 4 == 0 and c.lddx % 4 == 0 and all(ld % 4 == 0 for ld in c.ldw) and not any(c.w_off)
        if c.mask_by_x:
            assert c.want_dx and c.ldx % 4 == 0 and c.x_off == 0


def _strides_case(olib, kind):
    cus = CH.num_cus(olib)
    return [c for c in CH.edge_table(cus)["strides"] if c.kind == kind][0]


@pytest.mark.parametrize("kind,out", [("fwd", "y0"), ("fwd", "y1"), ("bwd", "dy1"), ("bwd", "dy0"), ("bwd", "dx"), ("bwd", "dw0"), ("bwd", "dw1"),
                                      ("bwd", "db0"), ("bwd", "db1")])
def test_checker_reports_an_element_off_by_3e5_of_its_mass(olib, kind, out):
    be = CH.HostBackend()
    case = _strides_case(olib, kind)
    check = CH.check_fwd if kind == "fwd" else CH.check_bwd
    res = (CH.run_fwd if kind == "fwd" else CH.run_bwd)(olib, be, case)
    rep = check(res)
    assert rep.ok(), str(rep)
    buf = dict(res.outputs)[out]
    mass = rep.mass[out].reshape(buf.rows, buf.cols)
    r, c = np.unravel_index(int(np.argmax(mass)), mass.shape)
    assert mass[r, c] > 0
    for sign in (1.0, -1.0):
        keep = buf.host.copy()
        buf.host[buf.flat_index(r, c)] = np.float32(float(buf.host[buf.flat_index(r, c)]) + sign * 3e-5 * mass[r, c])
        rep2 = check(res)
        assert any(v.startswith(out + ":") for v in rep2.violations), f"a {out} element moved by 3e-5 of its mass went unnoticed\n{rep2}"
        buf.host[:] = keep
    assert check(res).ok()


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_checker_reports_an_overwritten_padding_element(olib, kind):
    be = CH.HostBackend()
    case = _strides_case(olib, kind)
    check = CH.check_fwd if kind == "fwd" else CH.check_bwd
    res = (CH.run_fwd if kind == "fwd" else CH.run_bwd)(olib, be, case)
    assert check(res).ok()
    for name, buf in res.outputs:
        pads = np.flatnonzero(~buf.valid)
        assert pads.size >= CH.TAIL
        for at in (pads[0], pads[-1]):
            keep = buf.host[at]
            buf.host[at] = 0.0
            rep = check(res)
            assert any(v.startswith(name + ":") and "padding" in v for v in rep.violations), f"{name}: an overwritten padding element went unnoticed"
            buf.host[at] = keep
    assert check(res).ok()


def test_checker_rejects_a_nan_and_a_nonzero_where_the_mass_is_zero(olib):
    be = CH.HostBackend()
    case = CH.edge_table(CH.num_cus(olib))["dx-overwrite-maskx-none"][1]
    res = CH.run_bwd(olib, be, case)
    rep = CH.check_bwd(res)
    assert rep.ok()
    dx = res.DX
    mass = rep.mass["dx"]
    zeros = np.argwhere(mass == 0)
    assert len(zeros), "a stored, masked dx has elements without any term"
    r, c = zeros[0]
    dx.host[dx.flat_index(r, c)] = 1e-30
    assert not CH.check_bwd(res).ok()
    dx.host[dx.flat_index(r, c)] = np.nan
    assert not CH.check_bwd(res).ok()
