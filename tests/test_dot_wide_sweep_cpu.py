"""The wide interaction sweep's harness (the wide entries of tests/interaction_helpers.py), proved on a CPU.

The oracle library refuses more than 32 rows, so nothing here runs a kernel: these tests check what tests/test_gpu_dot_wide_sweep.py relies on.
The recomputed dispatch of ffh_dot_interaction_wide_fwd / _bwd has to be reached form by form -- all 19 instantiations by the edge table, each named
entry the forms its comment claims, at least 14 by the random draws --, no case may outgrow 2^24 floats a buffer, the float64 reference has to
equal a plain triple loop beyond 32 rows, and the checker has to report a planted wrong VALUE (a dropped term, a dropped direct path, two swapped
elements of the last rows) in a result that is otherwise the reference's own.
"""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import interaction_helpers as IH
from interaction_helpers import Case

CUS = 256


@pytest.fixture(scope="module")
def table():
    return IH.wide_edge_table(CUS)


def _kernels(cases):
    return {IH.wide_kernel(c) for c in cases}


def test_the_narrow_tables_are_as_they_were():
    assert IH.MAX_C == 32 and len(IH.EDGE_NAMES) == 25 and len(IH.ALL_KERNELS) == 11
    assert not any(c.wide for cases in IH.edge_table(CUS).values() for c in cases)
    assert not any(c.wide for c in IH.draw_cases(0, CUS))


def test_the_edge_table_reaches_every_instantiation(table):
    assert len(IH.ALL_WIDE_KERNELS) == len(set(IH.ALL_WIDE_KERNELS)) == 19
    assert list(table) == IH.WIDE_EDGE_NAMES
    cases = [c for cases in table.values() for c in cases]
    assert all(c.wide and 2 <= c.c <= IH.WIDE_MAX_C for c in cases)
    assert _kernels(cases) == set(IH.ALL_WIDE_KERNELS)
    assert {IH.kernel_of(c) for c in cases} == set(IH.ALL_WIDE_KERNELS)          # what note_worst files them under


def test_each_named_entry_reaches_what_it_claims(table):
    Gf, Gb = (lambda c: IH.wide_grid(CUS, c)), (lambda c: IH.wide_grid(CUS, c, backward=True))
    E = lambda prefix: IH.wide_entries(table, prefix)
    pred = IH.wide_predicates
    # second-image-high: the LDS-DMA forward with a second sample for some workgroup at T = 3 and 4, one chunk; a third sample at c = 128
    hi = E("second-image-high")
    fwd = [c for c in hi if c.kind == "fwd"]
    assert {(c.c, c.d) for c in hi} == {(65, 128), (96, 128), (97, 128), (128, 128)}
    assert all(pred(c)["v4"] and pred(c)["chunks"] == 1 and pred(c)["T"] >= 3 and c.batch > Gf(c.c) for c in fwd)
    assert all(pred(c)["v4"] and c.batch > Gb(c.c) for c in hi if c.kind == "bwd")
    assert any(c.c == 128 and c.batch > 2 * Gf(128) for c in fwd) and any(c.c == 128 and c.batch > 2 * Gb(128) for c in hi if c.kind == "bwd")
    assert {c.dist for c in hi} == {"uniform", "integer"}
    assert {IH.wide_kernel(c) for c in hi if c.kind == "bwd"} == {f"wide_bwd<T={t},VEC=4,ACCUM={a}>" for t in (3, 4) for a in (0, 1)}
    # chunks-vec4: two and three chunks in the LDS-DMA form, the last one whole and partial; a next sample behind an even and an odd count
    ch = E("chunks-vec4")
    assert all(c.d > 128 and pred(c)["v4"] for c in ch)
    assert {(c.c, c.d) for c in ch} == {(c, d) for c in (33, 64, 65, 128) for d in (132, 256, 260)}
    nxt = [c for c in E("chunks-vec4-next-sample") if c.kind == "fwd"]
    assert {(c.c, c.d, pred(c)["chunks"]) for c in nxt} == {(33, 132, 2), (33, 256, 2), (128, 260, 3)} and all(c.batch == Gf(c.c) + 2 for c in nxt)
    # fwd-ov1: both reasons for 4-byte pass-through stores, and the 16-byte store at a nonzero base, all with the LDS-DMA image
    ov = E("fwd-ov1")
    assert all(c.kind == "fwd" and pred(c)["v4"] for c in ov)
    for tag, want, why in (("fwd-ov1 stride", "OV=1", lambda c: c.ldo % 2 == 1 and c.out_off == 0),
                           ("fwd-ov1 base", "OV=1", lambda c: c.ldo % 4 == 0 and c.out_off == 1),
                           ("fwd-ov4-base", "OV=4", lambda c: c.ldo % 4 == 0 and c.out_off == 4)):
        some = [c for c in ov if c.name.startswith(tag)]
        assert {(c.c, c.d) for c in some} == {(c, d) for c in (33, 97) for d in (36, 128, 260)}, tag
        assert all(IH.wide_kernel(c) == f"wide_fwd<VEC=4,{want}>" and why(c) for c in some), tag
    # scalar-every-T: VEC == 1 at T = 1 .. 4, by odd d, by the base, by the stride; zg_off takes the backward alone
    sc = E("scalar-every-T")
    assert all(not pred(c)["v4"] for c in sc)
    assert {IH.wide_kernel(c) for c in sc} == {"wide_fwd<VEC=1,OV=1>"} | {f"wide_bwd<T={t},VEC=1,ACCUM={a}>" for t in (1, 2, 3, 4) for a in (0, 1)}
    for c in (31, 33, 65, 97):
        mine = [x for x in sc if x.c == c]
        assert {x.d for x in mine} == {1, 3, 63, 65, 129, 128}
        assert any(x.z_off == 1 for x in mine) and any(x.ldz % 4 == 2 for x in mine)
        assert {x.kind for x in mine if x.zg_off == 1} == {"bwd"}
        assert all(IH.wide_predicates(Case("", "fwd", x.batch, x.c, x.d))["v4"] for x in mine if x.zg_off == 1)
        assert {x.dist for x in mine} == {"uniform", "scaled"}
    assert {(x.c, x.d) for x in sc} >= {(128, 1), (2, 2)}
    # bwd-column-blocks: the 8-byte backward from 1 to 20 items, a last block of 4 columns
    cb = E("bwd-column-blocks")
    assert all(c.kind == "bwd" and pred(c)["v4"] for c in cb)
    assert {(c.c, c.d) for c in cb} == {(c, d) for c in (33, 128) for d in (4, 60, 64, 68, 124, 132, 192, 260)}
    assert {pred(c)["items"] for c in cb} == {2, 4, 6, 8, 10, 12, 20}
    # c-range
    assert {c.c for c in E("c-range-d8")} == set(range(2, 129)) and all(c.dist == "integer" and c.d == 8 and c.batch == 2 for c in E("c-range-d8"))
    for T in (1, 2, 3, 4):
        assert {pred(c)["T"] for c in table[f"c-range-d8-T{T}"]} == {T}
    assert {c.c for c in table["c-range-d128"]} == set(IH.WIDE_TILE_EDGES) and {c.dist for c in table["c-range-d128"]} == {"uniform", "integer"}
    # strides-differ
    sd = table["strides-differ"]
    assert {(c.c, c.d) for c in sd} == {(40, 12), (100, 128)}
    for c in sd:
        if c.kind == "bwd":
            lds, offs = (c.ldz, c.ldg, c.ldzg), (c.z_off, c.g_off, c.zg_off)
        else:
            lds, offs = (c.ldz, c.ldo), (c.z_off, c.out_off)
        assert len(set(lds)) == len(lds) and len(set(offs)) == len(offs) and all(v % 4 == 0 and v for v in lds + offs)
    both = [x for c, d in ((40, 12), (100, 128)) for x in [IH._differing_strides(c, d)]]
    assert all(len({x["ldz"], x["ldo"], x["ldg"], x["ldzg"]}) == 4 and len({x["z_off"], x["out_off"], x["g_off"], x["zg_off"]}) == 4 for x in both)
    # batches
    assert {c.batch for c in table["batches-128x128"]} == {1, 2, 3, 4, 5}
    assert {c.batch for c in table["batches-33x8"] if c.kind == "fwd"} == {Gf(33) - 1, Gf(33), Gf(33) + 1, 3 * Gf(33) + 2}
    assert {c.batch for c in table["batches-33x8"] if c.kind == "bwd"} == {Gb(33) - 1, Gb(33), Gb(33) + 1, 3 * Gb(33) + 2}


@pytest.mark.parametrize("cus", [8, CUS])
def test_the_random_draws_reach_14_of_the_19_forms(cus):
    cases = [c for s in IH.WIDE_SEEDS for c in IH.draw_wide_cases(s, cus)]
    assert len(cases) == 48 and len(IH.WIDE_SEEDS) == 8
    hit = _kernels(cases)
    assert hit <= set(IH.ALL_WIDE_KERNELS)
    assert len(hit) >= 14, sorted(set(IH.ALL_WIDE_KERNELS) - hit)
    assert {c.dist for c in cases} == set(IH.DISTS)
    edges = sum(c.c in IH.WIDE_TILE_EDGES for c in cases)
    assert 16 <= edges <= 40 and all(2 <= c.c <= 128 and 1 <= c.d <= 300 for c in cases)
    for c in cases:
        G = IH.wide_grid(cus, c.c, backward=c.kind == "bwd")
        assert 1 <= c.batch <= 9 or abs(c.batch - G) <= 3 or abs(c.batch - 2 * G) <= 3, c
    assert IH.draw_wide_cases(3, cus)[2].__dict__ == IH.draw_wide_cases(3, cus)[2].__dict__


@pytest.mark.parametrize("cus", [8, CUS, 304])
def test_no_case_outgrows_the_size_cap(cus):
    cases = [c for cases in IH.wide_edge_table(cus).values() for c in cases] + [c for s in IH.WIDE_SEEDS for c in IH.draw_wide_cases(s, cus)]
    big = [c for c in cases if IH.buffer_elems(c) > IH.WIDE_MAX_ELEMS]
    assert not big, big[:3]


def test_wide_predicates_agree_with_the_api_s_grid():
    for cus in (1, 8, CUS):
        for c in range(2, 129):
            for kind in ("fwd", "bwd"):
                p = IH.wide_predicates(Case("", kind, 1, c, 8))
                G = capi.DotWideApi.grid(cus, 1 << 30, c, backward=kind == "bwd")
                assert G == cus * p["per_cu"] == IH.wide_grid(cus, c, backward=kind == "bwd"), (cus, c, kind)
                assert capi.DotWideApi.grid(cus, 3, c, backward=kind == "bwd") == min(3, G)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference beyond 32 rows, and a checker that can fail there
C40 = dict(batch=2, c=40, d=5)


def _case(kind, dist, overwrite=False):
    case = Case(f"c40 {kind}", kind, dist=dist, overwrite=overwrite, seed=11, **C40)
    case.wide = True
    return case


def _loops(case, inp):
    """The contract of include/ffh_dot_wide.h in plain float64 loops."""
    B, c, d = case.batch, case.c, case.d
    z = inp["z"].astype(np.float64)
    if case.kind == "fwd":
        out = np.zeros((B, case.P))
        for b in range(B):
            for i in range(c):
                for j in range(i):
                    out[b, i * (i - 1) // 2 + j] = sum(z[b, i, k] * z[b, j, k] for k in range(d))
        return out
    g = inp["g"].astype(np.float64)
    dz = np.zeros((B, c, d))
    for b in range(B):
        for i in range(c):
            for j in range(c):
                if i != j:
                    hi, lo = max(i, j), min(i, j)
                    dz[b, i, :] += g[b, d + hi * (hi - 1) // 2 + lo] * z[b, j, :]
        dz[b, 0, :] += g[b, :d]
    return dz if case.overwrite else dz + inp["old"].astype(np.float64)


@pytest.mark.parametrize("kind,overwrite", [("fwd", False), ("bwd", True), ("bwd", False)])
def test_the_reference_equals_a_triple_loop_at_40_rows(kind, overwrite):
    case = _case(kind, "integer", overwrite)
    inp = IH.make_inputs(case)
    ref, _, _ = IH.reference(case, inp, 0, case.batch)
    assert np.array_equal(ref, _loops(case, inp))                 # small integers: both are exact
    case = _case(kind, "uniform", overwrite)
    inp = IH.make_inputs(case)
    ref, mass, _ = IH.reference(case, inp, 0, case.batch)
    assert np.all(np.abs(ref - _loops(case, inp)) <= 64 * np.finfo(np.float64).eps * mass)


def _result_of_the_reference(case):
    """A Result whose output holds the reference's own values rounded to float32, in sentinel buffers like a served call's."""
    be, inp = IH.HostBackend(), IH.make_inputs(case)
    B, c, d = case.batch, case.c, case.d
    ref, _, _ = IH.reference(case, inp, 0, B)
    Z = IH.Buf(be, B, c * d, case.ldz, case.z_off, inp["z"])
    if case.kind == "fwd":
        rows = np.concatenate([inp["z"][:, 0, :], ref.astype(np.float32)], axis=1)
        inputs, outputs = [("z", Z)], [("out", IH.Buf(be, B, case.wo, case.ldo, case.out_off, rows))]
    else:
        Gr = IH.Buf(be, B, case.wo, case.ldg, case.g_off, inp["g"])
        inputs, outputs = [("z", Z), ("out_grad", Gr)], [("z_grad", IH.Buf(be, B, c * d, case.ldzg, case.zg_off, ref.astype(np.float32)))]
    for _, b in inputs:
        b.fetch()
    for _, b in outputs:
        b.fetch()
        b.before = None                                           # (an output: nothing compares it with its upload)
    return IH.Result(case, inp, capi.FFH_OK, inputs, outputs)


def _dropped_term(res):
    """One term z[i, k] z[j, k] taken out of one triangle entry with i >= 32 (the largest one, so that it cannot hide in the bound)."""
    case, z = res.case, res.inp["z"].astype(np.float64)
    b, i, j = 1, 37, 33
    k = int(np.argmax(np.abs(z[b, i] * z[b, j])))
    at = IH.value_index(case, res.out, b, i * (i - 1) // 2 + j)
    res.out.host[at] = np.float32(float(res.out.host[at]) - z[b, i, k] * z[b, j, k])
    return "out:"


def _no_direct_path(res):
    case, g = res.case, res.inp["g"].astype(np.float64)
    b = 1
    col = int(np.argmax(np.abs(g[b, :case.d])))
    at = IH.value_index(case, res.z_grad, b, col)                 # row 0
    res.z_grad.host[at] = np.float32(float(res.z_grad.host[at]) - g[b, col])
    return "z_grad:"


def _last_rows_swapped(res):
    case, zg = res.case, res.z_grad
    b, c, d = 0, case.c, case.d
    rows = zg.get().reshape(case.batch, c, d)[b].astype(np.float64)
    k = int(np.argmax(np.abs(rows[c - 1] - rows[c - 2])))
    a, e = IH.value_index(case, zg, b, (c - 1) * d + k), IH.value_index(case, zg, b, (c - 2) * d + k)
    zg.host[a], zg.host[e] = zg.host[e], zg.host[a]
    return "z_grad:"


MUTATIONS = [("dropped-term", "fwd", False, _dropped_term, 1), ("no-direct-path", "bwd", True, _no_direct_path, 1),
             ("no-direct-path-accumulate", "bwd", False, _no_direct_path, 1), ("last-rows-swapped", "bwd", True, _last_rows_swapped, 2),
             ("last-rows-swapped-accumulate", "bwd", False, _last_rows_swapped, 2)]


@pytest.mark.parametrize("dist", ["uniform", "integer"])
@pytest.mark.parametrize("name,kind,overwrite,plant,elements", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_the_checker_reports_a_planted_wrong_value(name, kind, overwrite, plant, elements, dist):
    case = _case(kind, dist, overwrite)
    res = _result_of_the_reference(case)
    rep = IH.check(res)
    assert rep.ok(), f"the reference's own result does not pass: {rep}"
    names = plant(res)
    rep = IH.check(res)
    assert len(rep.violations) == 1 and rep.violations[0].startswith(f"{names} {elements} element(s)"), f"{name} on {case!r}\n{rep}"
