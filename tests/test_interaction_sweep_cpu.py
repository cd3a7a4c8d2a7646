"""The interaction sweep's harness (tests/interaction_helpers.py), proved on a CPU.

The oracle library is an independent float32 implementation of ffh_dot_interaction_fwd / _bwd (plain loops, k ascending): it has to pass the fixed
edge table and 12 seeds of the random generator under the sweep's own derived bound, bit-exact on the `integer` inputs -- so the float64 reference,
the generator and the bound are sound before a GPU sees them.  The generator has to reach every dispatch predicate both ways and every kernel
instantiation of csrc/interaction.hip.  And the checker has to be able to fail: the oracle library wrapped in one fault at a time -- the faults the
HIP kernels could have -- is reported on a named small case.
"""
import ctypes as C
import types

import numpy as np
import pytest

from dlrm_flexflow_amd import capi
import interaction_helpers as IH

SEEDS = range(12)


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


def _report_worst():
    print("worst |got - ref| / bound so far:", {k: round(v, 4) for k, v in sorted(IH.WORST.items())})


@pytest.mark.parametrize("name", IH.EDGE_NAMES)
def test_oracle_passes_the_edge_table(olib, name):
    be = IH.HostBackend()
    cases = IH.edge_table(IH.num_cus(olib))[name]
    assert cases
    for case in cases:
        _, rep = IH.run_and_check(olib, be, case)
        assert rep.ok(), f"{case!r}\n{rep}"
    _report_worst()


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_passes_the_random_sweep(olib, seed):
    be, cus = IH.HostBackend(), IH.num_cus(olib)
    cases = IH.draw_cases(seed, cus)
    assert len(cases) == 6
    for case in cases:
        assert 2 <= case.c <= IH.MAX_C and 1 <= case.d <= 300 and 1 <= case.batch <= 2 * IH.lds_pass(cus) + 3
        _, rep = IH.run_and_check(olib, be, case)
        assert rep.ok(), f"{case!r}\n{rep}"
    _report_worst()


@pytest.mark.parametrize("cus", [8, 256])
def test_generator_reaches_every_predicate_and_every_kernel(cus):
    """Over the edge table and the GPU sweep's 12 seeds: v4, o4, d == 128 and overwrite both ways, and every (kernel, VEC, ACCUM) instantiation."""
    table = [c for cases in IH.edge_table(cus).values() for c in cases]
    cases = table + [c for s in SEEDS for c in IH.draw_cases(s, cus)]
    missing = []
    for kind, names in (("fwd", ("v4", "o4", "d128")), ("bwd", ("v4", "d128", "overwrite"))):
        preds = [IH.predicates(c) for c in cases if c.kind == kind]
        for n in names:
            missing += [f"{kind}: {n} is never {want}" for want in (True, False) if want not in {p[n] for p in preds}]
    hit = {IH.kernel(c) for c in cases}
    missing += [f"{k} is never launched" for k in IH.ALL_KERNELS if k not in hit]
    assert not hit - set(IH.ALL_KERNELS), hit - set(IH.ALL_KERNELS)
    # what the table itself promises: the branches no random batch reaches
    A, G = IH.lds_pass(cus), IH.GRID_PASS
    lds = [c for c in table if IH.kernel(c).startswith("fwd_lds")]
    if not any(c.batch > 2 * A for c in lds):
        missing.append("no LDS forward with a third sample per wave")
    for k in ("fwd<VEC=4", "fwd<VEC=1", "bwd_d128<ACCUM=0", "bwd_d128<ACCUM=1", "bwd<VEC=4,ACCUM=0", "bwd<VEC=4,ACCUM=1", "bwd<VEC=1,ACCUM=0",
              "bwd<VEC=1,ACCUM=1"):
        if not any(c.batch > 2 * G for c in table if IH.kernel(c).startswith(k)):
            missing.append(f"{k}: no wave takes a third sample")
    if not any(IH.kernel(c).startswith("bwd<VEC=4") and c.d > 256 and c.d % 128 for c in table):
        missing.append("no general VEC == 4 backward with three chunks, the last one partial")
    if not any(c.ldz != c.ldzg and c.ldz != c.c * c.d != c.ldzg for c in table if c.kind == "bwd"):
        missing.append("no backward with ldz != ldzg != c * d")
    assert {c.c for c in table if c.d == 128} >= set(range(2, IH.MAX_C + 1)), "a triangle size is missing at d == 128"
    assert not missing, "\n".join(missing)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker fails when it should: the oracle library wrapped in one fault at a time
def _view(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(int(n),))


def _rows(ptr, batch, ld, width):
    flat = _view(ptr, (batch - 1) * ld + width)
    return np.lib.stride_tricks.as_strided(flat, shape=(batch, width), strides=(4 * ld, 4))


class Faulty:
    """The two entry points of the oracle library with one fault; takes the place of the library in interaction_helpers.run_case."""

    def __init__(self, olib, fault, cus):
        self.o, self.fault, self.ctx, self.A = olib, fault, olib.ctx, IH.lds_pass(cus)
        self.lib = types.SimpleNamespace(ffh_dot_interaction_fwd=self.fwd, ffh_dot_interaction_bwd=self.bwd)

    def fwd(self, ctx, z, ldz, out, ldo, batch, c, d, s):
        f = self.fault
        if f == "beyond-grid-untouched":
            batch = min(batch, IH.GRID_PASS)
        rc = self.o.lib.ffh_dot_interaction_fwd(ctx, z, ldz, out, ldo, batch, c, d, s)
        Z, O = _rows(z, batch, ldz, c * d), _rows(out, batch, ldo, d + c * (c - 1) // 2)
        if f == "drop-last-k":
            il, jl = np.tril_indices(c, -1)
            zz = Z.reshape(batch, c, d)
            O[:, d:] -= zz[:, il, d - 1] * zz[:, jl, d - 1]
        elif f == "transposed-pair":         # pair (3, 1) indexed as (1, 3): 1 * 0 / 2 + 3 is the place of pair (3, 0)
            O[:, [d + 3, d + 4]] = O[:, [d + 4, d + 3]]
        elif f == "third-pass-stale":
            O[2 * self.A:] = O[self.A:batch - self.A].copy()
        elif f == "padding-written":
            _view(out, ldo + 1)[d + c * (c - 1) // 2] = 0.0
        elif f == "input-modified":
            Z[batch // 2, c * d - 1] += 1.0
        return rc

    def bwd(self, ctx, z, ldz, g, ldg, zg, ldzg, batch, c, d, flags, s):
        f = self.fault
        if f == "beyond-grid-untouched":
            batch = min(batch, IH.GRID_PASS)
        if f in ("transposed-pair", "no-direct-path"):          # the library reads a private copy of the gradient with the fault in it
            gg = np.ascontiguousarray(_rows(g, batch, ldg, d + c * (c - 1) // 2))
            if f == "transposed-pair":
                gg[:, [d + 3, d + 4]] = gg[:, [d + 4, d + 3]]
            else:
                gg[:, :d] = 0.0
            g, ldg = gg.ctypes.data, gg.shape[1]
        if f == "ldz-for-z_grad":
            assert ldz < ldzg, "the faulty stride has to stay inside the allocation"
            ldzg = ldz
        rc = self.o.lib.ffh_dot_interaction_bwd(ctx, z, ldz, g, ldg, zg, ldzg, batch, c, d, flags, s)
        if f == "padding-written":
            _view(zg, ldzg + 1)[c * d] = 0.0
        elif f == "input-modified":
            _rows(g, batch, ldg, d + c * (c - 1) // 2)[batch // 2, d] += 1.0
        return rc


def _named(cus, entry, kind, dist, overwrite=None, pick=0):
    cases = [c for c in IH.edge_table(cus)[entry] if c.kind == kind and c.dist == dist and (overwrite is None or c.overwrite == overwrite)]
    return cases[pick]


FAULTS = [
    # fault, entry of the edge table, kind, distribution, what the report has to name
    ("drop-last-k", "k-tails-vec1", "fwd", "uniform", "out:"),
    ("drop-last-k", "strides-differ", "fwd", "integer", "out:"),
    ("transposed-pair", "strides-differ", "fwd", "uniform", "out:"),
    ("transposed-pair", "strides-differ", "bwd", "uniform", "z_grad:"),
    ("transposed-pair", "strides-differ", "bwd", "integer", "z_grad:"),
    ("no-direct-path", "strides-differ", "bwd", "uniform", "z_grad:"),
    ("no-direct-path", "c-range-d8", "bwd", "integer", "z_grad:"),
    ("ldz-for-z_grad", "strides-differ", "bwd", "uniform", "z_grad:"),
    ("beyond-grid-untouched", "grid-stride-5x10-G+7-uniform", "fwd", "uniform", "out:"),
    ("beyond-grid-untouched", "grid-stride-5x10-G+7-integer", "bwd", "integer", "z_grad:"),
    ("third-pass-stale", "lds-third-sample", "fwd", "uniform", "out:"),
    ("third-pass-stale", "lds-third-sample", "fwd", "integer", "out:"),
    ("padding-written", "strides-differ", "fwd", "uniform", "padding"),
    ("padding-written", "strides-differ", "bwd", "uniform", "padding"),
    ("input-modified", "strides-differ", "fwd", "uniform", "z: the input was modified"),
    ("input-modified", "strides-differ", "bwd", "uniform", "out_grad: the input was modified"),
]


@pytest.mark.parametrize("fault,entry,kind,dist,names", FAULTS, ids=[f"{f[0]}-{f[2]}-{f[3]}" for f in FAULTS])
def test_checker_reports_a_faulty_library(olib, fault, entry, kind, dist, names):
    be, cus = IH.HostBackend(), IH.num_cus(olib)
    case = _named(cus, entry, kind, dist, pick=-1 if entry == "strides-differ" else 0)
    if fault == "transposed-pair":
        assert case.c >= 4
    _, rep = IH.run_and_check(olib, be, case)
    assert rep.ok(), f"{case!r}\n{rep}"
    _, rep = IH.run_and_check(Faulty(olib, fault, cus), be, case)
    assert any(names in v for v in rep.violations), f"{fault} went unnoticed on {case!r}\n{rep}"


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_checker_reports_a_result_three_bounds_off(olib, kind):
    be, cus = IH.HostBackend(), IH.num_cus(olib)
    case = _named(cus, "strides-differ", kind, "uniform")
    res = IH.run_case(olib, be, case)
    rep = IH.check(res)
    assert rep.ok(), str(rep)
    name, buf = res.outputs[0]
    bound = rep.bound[name]
    b, e = np.unravel_index(int(np.argmax(bound)), bound.shape)
    assert bound[b, e] > 0
    at = IH.value_index(case, buf, b, e)
    for sign in (1.0, -1.0):
        keep = buf.host[at]
        buf.host[at] = np.float32(float(keep) + sign * 3.0 * bound[b, e])
        rep2 = IH.check(res)
        assert any(v.startswith(name + ":") and "beyond" in v for v in rep2.violations), f"a {name} element 3 bounds off went unnoticed\n{rep2}"
        buf.host[at] = keep
    assert IH.check(res).ok()


def test_checker_rejects_a_nan_and_a_nonzero_where_the_mass_is_zero(olib):
    be, cus = IH.HostBackend(), IH.num_cus(olib)
    case = _named(cus, "c-range-d8", "bwd", "integer", overwrite=True)       # c == 2: dz[1, k] = g(1, 0) z[0, k], nothing where z[0, k] == 0
    assert case.c == 2
    for dist in ("integer", "uniform"):
        case.dist = dist
        inp = IH.make_inputs(case)
        inp["z"][:, 0, ::3] = 0.0
        res = IH.run_case(olib, be, case, inp=inp)
        rep = IH.check(res)
        assert rep.ok(), str(rep)
        zg, mass = res.z_grad, rep.mass["z_grad"]
        zeros = np.argwhere(mass == 0)
        assert len(zeros), "no element without any term"
        b, e = zeros[0]
        at = IH.value_index(case, zg, b, e)
        for wrong in (1e-30, np.nan):
            zg.host[at] = wrong
            assert any(v.startswith("z_grad:") for v in IH.check(res).violations), f"{wrong} where the mass is zero went unnoticed ({dist})"
        zg.host[at] = 0.0
        assert IH.check(res).ok()


def test_a_refused_call_is_reported(olib):
    be = IH.HostBackend()
    case = IH.Case("refused", "fwd", 3, 4, 8)
    res = IH.run_case(olib, be, case, args=dict(nrows=33))
    assert res.rc == capi.FFH_ERR_BAD_ARG and not IH.check(res).ok()
    assert all(buf.untouched() for _, buf in res.buffers())
