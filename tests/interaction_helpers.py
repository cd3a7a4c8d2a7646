"""Generator, float64 reference and checker for ffh_dot_interaction_fwd / ffh_dot_interaction_bwd (include/ff_hip.h).

Used by tests/test_interaction_sweep_cpu.py (the oracle library, on a CPU: proves the harness) and tests/test_gpu_interaction_sweep.py (the four
MFMA kernels of csrc/interaction.hip).  Nothing here calls the oracle library: the reference is plain numpy in float64, written from the contract
in the header.  tests/dot_helpers.py is the model-level helper and has nothing to do with this file.

  forward    out[b, :d]                    =  z[b, 0, :]                                   (bit for bit)
             out[b, d + i (i - 1) / 2 + j] =  sum_k z[b, i, k] z[b, j, k]      i > j
  backward   dz[b, i, :]                   =  sum_j S[b, i, j] z[b, j, :]                  S = G + G^T, G strictly lower from g[b, d:]
             dz[b, 0, :]                  +=  g[b, :d]
             z_grad                        =  dz (FFH_DOT_BWD_OVERWRITE)  or  z_grad + dz

The bound is derived, not tuned:  |got - ref| <= (k + 2) * eps32 * mass + k * tiny32.  mass = the float64 sum of the absolute values of the terms
of that element (with |g| on row 0 and the old value when accumulating), k = the number of terms (d forward; c - 1 backward, one more each for the
direct path and the old value), tiny32 = float32's smallest normal (a product flushed to zero), eps32 = 2^-23 = twice the unit roundoff of
round-to-nearest -- so the bound holds for any summation order and for a truncating accumulator.  A dropped, doubled or misplaced term of order-one
inputs misses it by 1 / (k^2 eps32), about 500 at d = 128.  Where mass == 0 the result has to be exactly 0; a NaN anywhere fails.  With the
`integer` inputs every fp32 operation is exact, so the result has to EQUAL the float64 reference: a wrong index has no tolerance to hide in.

Every buffer is a chain_helpers.Buf: allocated with its leading dimension and offset, everything outside [batch][width] holds a NaN sentinel.  After
the call the outputs' padding holds the sentinel bit for bit and every input is bit-identical to what was uploaded.
"""
import numpy as np

from dlrm_flexflow_amd import capi
from chain_helpers import HostBackend, TorchBackend, Buf, num_cus, SENTINEL_BITS, EPS32       # noqa: F401  (re-exported to the two test files)

TINY32 = float(np.finfo(np.float32).tiny)
OVERWRITE = 1                         # FFH_DOT_BWD_OVERWRITE
MAX_C = 32                            # rows of z a sample may have
GRID_PASS = 4 * 4096                  # "G": samples per pass of the capped grids (4096 workgroups of 4 waves, one sample per wave)
CHUNK = 2048                          # samples per slice of the float64 reference
KEEP_ELEMS = 1 << 22                  # the report keeps mass and bound of outputs up to this size (the checker's own tests read them)
DISTS = ("uniform", "scaled", "integer")


def lds_pass(cus):
    """"A": samples per pass of the LDS forward's grid (one 4-wave workgroup per compute unit)."""
    return 4 * cus


def _up4(v):
    return (v + 3) & ~3


# ---------------------------------------------------------------------------------------------------------------------------
# a case
class Case:
    """One call.  Leading dimensions left None get a padded default that keeps 16-byte alignment where the width allows it, all four different."""

    def __init__(self, name, kind, batch, c, d, ldz=None, z_off=0, ldo=None, out_off=0, ldg=None, g_off=0, ldzg=None, zg_off=0, overwrite=False,
                 dist="uniform", seed=0):
        assert kind in ("fwd", "bwd") and dist in DISTS
        self.name, self.kind, self.batch, self.c, self.d = name, kind, int(batch), int(c), int(d)
        self.P = self.c * (self.c - 1) // 2
        self.wo = self.d + self.P                                   # floats of an output / gradient row
        self.ldz = c * d + 4 if ldz is None else int(ldz)
        self.ldzg = c * d + 8 if ldzg is None else int(ldzg)
        self.ldo = _up4(self.wo) + 4 if ldo is None else int(ldo)
        self.ldg = self.wo + 3 if ldg is None else int(ldg)
        self.z_off, self.out_off, self.g_off, self.zg_off = int(z_off), int(out_off), int(g_off), int(zg_off)
        self.overwrite, self.dist, self.seed = bool(overwrite), dist, int(seed)

    @property
    def flags(self):
        return OVERWRITE if self.overwrite else 0

    def __repr__(self):
        s = f"Case({self.name}: {self.kind} B={self.batch} c={self.c} d={self.d} {self.dist} seed={self.seed} ldz={self.ldz}+{self.z_off}"
        if self.kind == "fwd":
            return s + f" ldo={self.ldo}+{self.out_off} -> {kernel(self)})"
        return s + f" ldg={self.ldg}+{self.g_off} ldzg={self.ldzg}+{self.zg_off} overwrite={self.overwrite} -> {kernel(self)})"


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch rules of ffh_dot_interaction_fwd / _bwd (csrc/interaction.hip), recomputed from the case: allocations are 16-byte aligned, so a
# base is aligned exactly when its offset is a multiple of 4 floats
def predicates(case):
    if case.kind == "fwd":
        v4 = case.d % 4 == 0 and case.ldz % 4 == 0 and case.z_off % 4 == 0
        return {"v4": v4, "o4": v4 and case.ldo % 4 == 0 and case.out_off % 4 == 0, "d128": case.d == 128}
    v4 = case.d % 4 == 0 and case.ldz % 4 == 0 and case.ldzg % 4 == 0 and case.z_off % 4 == 0 and case.zg_off % 4 == 0
    return {"v4": v4, "d128": case.d == 128, "overwrite": case.overwrite}


def kernel(case):
    """The instantiation that serves the case."""
    p = predicates(case)
    if case.kind == "fwd":
        if p["v4"] and p["d128"]:
            return f"fwd_lds<OV={4 if p['o4'] else 1}>"
        return f"fwd<VEC={4 if p['v4'] else 1},OV={4 if p['o4'] else 1}>"
    acc = 0 if case.overwrite else 1
    if p["v4"] and p["d128"]:
        return f"bwd_d128<ACCUM={acc}>"
    return f"bwd<VEC={4 if p['v4'] else 1},ACCUM={acc}>"


ALL_KERNELS = (["fwd_lds<OV=4>", "fwd_lds<OV=1>", "fwd<VEC=4,OV=4>", "fwd<VEC=4,OV=1>", "fwd<VEC=1,OV=1>"]
               + [f"bwd_d128<ACCUM={a}>" for a in (0, 1)] + [f"bwd<VEC={v},ACCUM={a}>" for v in (4, 1) for a in (0, 1)])


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
def make_inputs(case):
    """z [B][c][d]; for the backward also g [B][d + P] and the old z_grad [B][c][d].  The same for a given case on every backend."""
    rng = np.random.default_rng([case.seed, case.batch, case.c, case.d, DISTS.index(case.dist), case.kind == "bwd"])
    B, c, d = case.batch, case.c, case.d
    inp = {}
    if case.dist == "integer":
        draw = lambda *shape: rng.integers(-4, 5, shape, dtype=np.int8).astype(np.float32)
    else:
        draw = lambda *shape: rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)
    inp["z"] = draw(B, c, d)
    if case.dist == "scaled":
        inp["z"] *= np.exp2(rng.integers(-8, 9, (B, c, 1))).astype(np.float32)
    if case.kind == "bwd":
        inp["g"] = draw(B, case.wo)
        if case.dist == "scaled":
            inp["g"] *= np.exp2(rng.integers(-8, 9, (B, 1))).astype(np.float32)
        inp["old"] = draw(B, c, d)
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# the call
class Result:
    def __init__(self, case, inp, rc, inputs, outputs):
        self.case, self.inp, self.rc, self.inputs, self.outputs = case, inp, rc, inputs, outputs
        self.__dict__.update(dict(inputs + outputs))

    def buffers(self):
        return self.inputs + self.outputs


def run_case(lib, be, case, args=None, null=(), inp=None):
    """Run one case.  `args` replaces arguments of the call (nrows, d, batch, ldz, ldo, ldg, ldzg, flags) and `null` names buffers passed as a null
    pointer, both without changing what is allocated: the refusals."""
    inp = inp or make_inputs(case)
    B, c, d = case.batch, case.c, case.d
    a = dict(nrows=c, d=d, batch=B, ldz=case.ldz, ldo=case.ldo, ldg=case.ldg, ldzg=case.ldzg, flags=case.flags)
    a.update(args or {})
    Z = Buf(be, B, c * d, case.ldz, case.z_off, inp["z"])
    at = lambda name, buf: None if name in null else buf.ptr
    if case.kind == "fwd":
        O = Buf(be, B, case.wo, case.ldo, case.out_off)
        inputs, outputs = [("z", Z)], [("out", O)]
        rc = lib.lib.ffh_dot_interaction_fwd(lib.ctx, at("z", Z), a["ldz"], at("out", O), a["ldo"], a["batch"], a["nrows"], a["d"], None)
    else:
        Gr = Buf(be, B, case.wo, case.ldg, case.g_off, inp["g"])
        ZG = Buf(be, B, c * d, case.ldzg, case.zg_off, inp["old"])
        inputs, outputs = [("z", Z), ("out_grad", Gr)], [("z_grad", ZG)]
        rc = lib.lib.ffh_dot_interaction_bwd(lib.ctx, at("z", Z), a["ldz"], at("out_grad", Gr), a["ldg"], at("z_grad", ZG), a["ldzg"], a["batch"],
                                             a["nrows"], a["d"], a["flags"], None)
    be.sync()
    for _, b in inputs + outputs:
        b.fetch()
    return Result(case, inp, rc, inputs, outputs)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker
class Report:
    def __init__(self):
        self.violations, self.mass, self.bound, self.worst = [], {}, {}, {}

    def ok(self):
        return not self.violations

    def __str__(self):
        return "\n".join(self.violations)


WORST = {}       # kernel instantiation -> worst |got - ref| / bound seen in this process (printed by the tests: a measurement, not a check)


def _rows(buf, lo, hi):
    """Rows [lo, hi) of the [rows][cols] block as the library left it: a view of the downloaded allocation."""
    return np.lib.stride_tricks.as_strided(buf.host[buf.off + lo * buf.ld:], shape=(hi - lo, buf.cols), strides=(4 * buf.ld, 4), writeable=False)


def reference(case, inp, lo, hi):
    """(ref, mass, k) of samples [lo, hi) in float64: [n][P] for the forward's triangle, [n][c][d] for the backward; k broadcasts against them."""
    c, d = case.c, case.d
    z = inp["z"][lo:hi].astype(np.float64)
    il, jl = np.tril_indices(c, -1)                               # row-major over i > j: position i (i - 1) / 2 + j
    if case.kind == "fwd":
        za = np.abs(z)
        return (z @ z.transpose(0, 2, 1))[:, il, jl], (za @ za.transpose(0, 2, 1))[:, il, jl], float(d)
    g = inp["g"][lo:hi].astype(np.float64)
    S = np.zeros((hi - lo, c, c))
    S[:, il, jl] = g[:, d:]
    S = S + S.transpose(0, 2, 1)
    ref, mass = S @ z, np.abs(S) @ np.abs(z)
    ref[:, 0, :] += g[:, :d]
    mass[:, 0, :] += np.abs(g[:, :d])
    k = np.full((1, c, 1), c - 1.0)
    k[0, 0, 0] += 1
    if not case.overwrite:
        old = inp["old"][lo:hi].astype(np.float64)
        ref, mass, k = ref + old, mass + np.abs(old), k + 1
    return ref, mass, k


def bound_of(case, mass, k):
    if case.dist == "integer":
        return np.zeros_like(mass)                                # every fp32 operation was exact
    return np.where(mass > 0, (k + 2) * EPS32 * mass + k * TINY32, 0.0)


def compare_slice(case, inp, got, lo, hi):
    """The compared values of samples [lo, hi) (the forward's triangle, the backward's z_grad) against the reference: the number of elements beyond
    the bound, where the worst of them is, the worst finite |got - ref| / bound, and the mass and the bound themselves."""
    ref, mass, k = reference(case, inp, lo, hi)
    got = np.asarray(got).astype(np.float64).reshape(ref.shape)
    bound = bound_of(case, mass, k)
    err = np.abs(got - ref)
    bad = ~(err <= bound)            # (a NaN is bad)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    finite = ratio[np.isfinite(ratio)]
    worst, where = (float(finite.max()) if finite.size else 0.0), None
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.nan_to_num(ratio, nan=np.inf, posinf=1e300), -1.0))), bad.shape)
        where = f"sample {lo + int(i[0])} element {tuple(int(v) for v in i[1:])}: got {got[i]!r} ref {ref[i]!r} mass {mass[i]:.3e} bound {bound[i]:.3e}"
    return int(bad.sum()), where, worst, mass, bound


def note_worst(case, worst):
    kern = kernel(case)
    WORST[kern] = max(WORST.get(kern, 0.0), worst)


def check(res):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    for name, buf in res.inputs:
        if not buf.untouched():
            at = np.flatnonzero(buf.host.view(np.uint32) != buf.before.view(np.uint32))
            rep.violations.append(f"{name}: the input was modified, {at.size} element(s), first at flat index {int(at[0])} (ld {buf.ld}, offset {buf.off})")
    for name, buf in res.outputs:
        if not buf.padding_intact():
            at = np.flatnonzero((buf.host.view(np.uint32) != SENTINEL_BITS) & ~buf.valid)
            rep.violations.append(f"{name}: {at.size} padding element(s) overwritten, first at flat index {int(at[0])} (ld {buf.ld}, offset {buf.off})")
    name, out = res.outputs[0]
    B, c, d = case.batch, case.c, case.d
    keep = B * out.cols <= KEEP_ELEMS
    masses, bounds, nbad, first, worst = [], [], 0, None, 0.0
    for lo in range(0, B, CHUNK):
        hi = min(B, lo + CHUNK)
        got = _rows(out, lo, hi)
        if case.kind == "fwd":
            zin = inp["z"][lo:hi, 0, :]
            same = got[:, :d].view(np.uint32) == zin.view(np.uint32)
            if not same.all() and not any("pass-through" in v for v in rep.violations):
                b, k = np.argwhere(~same)[0]
                rep.violations.append(f"{name}: pass-through column {int(k)} of sample {lo + int(b)} is {got[b, k]!r}, z holds {zin[b, k]!r}")
            got = got[:, d:]
        n, where, w, mass, bound = compare_slice(case, inp, got, lo, hi)
        nbad, first, worst = nbad + n, first or where, max(worst, w)
        if keep:
            masses.append(mass.reshape(hi - lo, -1))
            bounds.append(bound.reshape(hi - lo, -1))
    if keep and B:
        rep.mass[name], rep.bound[name] = np.concatenate(masses), np.concatenate(bounds)     # [B][P] forward, [B][c * d] backward
    rep.worst[name] = worst
    note_worst(case, worst)
    if nbad:
        what = "differ from the exact result" if case.dist == "integer" else "beyond (k + 2) eps32 mass + k tiny32"
        rep.violations.append(f"{name}: {nbad} element(s) {what}; worst in the first failing slice: {first}")
    return rep


def run_and_check(lib, be, case):
    res = run_case(lib, be, case)
    return res, check(res)


def value_index(case, buf, b, e):
    """Flat index in buf.host of element e of the compared part of sample b (the forward's triangle starts behind the d pass-through columns)."""
    return buf.flat_index(b, e + (case.d if case.kind == "fwd" else 0))


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed edge table
def _trio(name, batch, c, d, dists=("uniform",), kinds=("fwd", "bwd"), **kw):
    """The forward and the backward both ways (overwrite, accumulate) of one shape, for every distribution asked for."""
    out = []
    fwd_kw = {k: v for k, v in kw.items() if k in ("ldz", "z_off", "ldo", "out_off")}
    bwd_kw = {k: v for k, v in kw.items() if k in ("ldz", "z_off", "ldg", "g_off", "ldzg", "zg_off")}
    for dist in dists:
        tag = f"{name} B={batch} c={c} d={d} {dist}"
        seed = len(tag) + 31 * batch + 7 * c + d
        if "fwd" in kinds:
            out.append(Case(tag + " fwd", "fwd", batch, c, d, dist=dist, seed=seed, **fwd_kw))
        if "bwd" in kinds:
            out.append(Case(tag + " bwd overwrite", "bwd", batch, c, d, dist=dist, seed=seed, overwrite=True, **bwd_kw))
            out.append(Case(tag + " bwd accumulate", "bwd", batch, c, d, dist=dist, seed=seed + 1, overwrite=False, **bwd_kw))
    return out


GRID_STRIDE_SHAPES = ((9, 128), (5, 12), (5, 10))                # the d128 backward and the LDS forward; the general VEC 4 kernels; VEC 1
GRID_STRIDE_BATCHES = (("G+7", GRID_PASS + 7), ("2G+3", 2 * GRID_PASS + 3))


def edge_table(cus):
    """name -> list of cases; every entry is the smallest shape that reaches its branch (A = 4 * cus, G = 16384)."""
    A, UI = lds_pass(cus), ("uniform", "integer")
    t = {}
    # the LDS forward: a wave's third sample lands in image 0 while sample 1 is read from image 1; ragged last pass
    t["lds-third-sample"] = _trio("lds-third-sample", 2 * A + 5, 27, 128, UI)
    t["lds-four-passes"] = _trio("lds-four-passes", 3 * A + 1, 32, 128, UI) + _trio("lds-four-passes", 3 * A + 1, 2, 128, UI)      # npieces 16 and 1
    t["lds-odd-c"] = _trio("lds-odd-c", 2 * A + 2, 3, 128, UI) + _trio("lds-odd-c", 2 * A + 2, 31, 128, UI)
    wo = 128 + 17 * 16 // 2                                       # 264: o4 both ways, from the stride and from the base
    t["lds-ov1"] = (_trio("lds-ov1 stride", A + 3, 17, 128, UI, ldo=wo + 1, ldg=wo + 1)
                    + _trio("lds-ov1 base", A + 3, 17, 128, UI, ldo=wo + 4, out_off=1, ldg=wo + 4, g_off=1))
    t["lds-ov4"] = (_trio("lds-ov4 stride", A + 3, 17, 128, UI, ldo=wo + 4, ldg=wo + 4)
                    + _trio("lds-ov4 base", A + 3, 17, 128, UI, ldo=wo + 4, out_off=4, ldg=wo + 4, g_off=4))
    # d == 128 that must fall back to the VEC == 1 kernels
    t["d128-falls-back"] = (_trio("falls-back z_off", 67, 27, 128, z_off=1) + _trio("falls-back ldz", 67, 27, 128, ldz=27 * 128 + 2)
                            + _trio("falls-back zg_off", 67, 27, 128, kinds=("bwd",), zg_off=1))
    # the capped grids: a wave's second and third sample, S rewritten under wave barriers
    for c, d in GRID_STRIDE_SHAPES:
        for tag, batch in GRID_STRIDE_BATCHES:
            for dist in UI:                                       # (one entry per distribution: these are the large cases)
                t[f"grid-stride-{c}x{d}-{tag}-{dist}"] = _trio("grid-stride", batch, c, d, (dist,))
    # the general VEC == 4 backward with two and three 128-column chunks, the last one partial; both forward stores
    t["wide-vec4"] = [case for d in (132, 256, 260) for c in (2, 32)
                      for case in _trio("wide-vec4", 9, c, d) + _trio("wide-vec4 odd ldo", 9, c, d, kinds=("fwd",), ldo=d + c * (c - 1) // 2 + 1 | 1)]
    # every tail of the forward's 64-wide k loop
    t["k-tails-vec1"] = [case for d in (1, 3, 15, 17, 63, 65, 129) for case in _trio("k-tails", 6, 7, d, ("uniform", "scaled"))]
    t["k-tails-vec4"] = [case for d in (4, 60, 64, 68) for case in _trio("k-tails", 6, 7, d, ("uniform", "scaled"))
                         + _trio("k-tails odd ldo", 6, 7, d, ("uniform", "scaled"), kinds=("fwd",), ldo=(d + 21) | 1)]
    # every triangle size (s_pair)
    for d in (128, 8):
        t[f"c-range-d{d}"] = [case for c in range(2, MAX_C + 1) for case in _trio("c-range", 5, c, d, UI)]
    # four different strides and four different nonzero offsets, all multiples of 4
    t["strides-differ"] = [case for c, d in ((27, 128), (6, 12), (5, 10))
                           for case in _trio("strides-differ", 11, c, d, UI, ldz=_up4(c * d) + 8, z_off=4, ldo=_up4(d + c * (c - 1) // 2) + 4, out_off=8,
                                             ldg=_up4(d + c * (c - 1) // 2) + 12, g_off=12, ldzg=_up4(c * d) + 16, zg_off=16)]
    # idle waves, fewer workgroups than compute units
    t["tiny-batches"] = [case for B in (1, 2, 3, 4, 5) for case in _trio("tiny-batches", B, 27, 128)]
    return t


EDGE_NAMES = list(edge_table(1))


# ---------------------------------------------------------------------------------------------------------------------------
# the random generator
def draw_case(rng, cus, name="random"):
    A = lds_pass(cus)
    m = int(rng.integers(3))
    d = 128 if m == 0 else 4 * int(rng.integers(1, 76)) if m == 1 else int(rng.integers(1, 301))
    c = int(rng.integers(2, MAX_C + 1))
    m = int(rng.integers(3))
    batch = int(rng.integers(1, 10)) if m == 0 else m * A + int(rng.integers(-3, 4))
    kind = "fwd" if rng.random() < 0.5 else "bwd"
    wo = d + c * (c - 1) // 2
    if rng.random() < 0.6:       # strides and offsets that keep a 16-byte alignment the width allows
        pad, off = (lambda: 4 * int(rng.integers(0, 4))), (lambda: 4 * int(rng.integers(0, 3)))
        ldz, ldzg, ldo = _up4(c * d) + pad(), _up4(c * d) + pad(), _up4(wo) + pad()
    else:
        pad, off = (lambda: int(rng.choice([0, 0, 1, 2, 3, 4, 5, 8]))), (lambda: int(rng.integers(0, 6)))
        ldz, ldzg, ldo = c * d + pad(), c * d + pad(), wo + pad()
    return Case(name, kind, batch, c, d, ldz=ldz, z_off=off(), ldo=ldo, out_off=off(), ldg=wo + int(rng.choice([0, 1, 2, 3, 4, 7])),
                g_off=int(rng.integers(0, 6)), ldzg=ldzg, zg_off=off(), overwrite=bool(rng.random() < 0.5), dist=str(rng.choice(DISTS)),
                seed=int(rng.integers(1 << 30)))


def draw_cases(seed, cus, count=6):
    """The cases of one seed.  Batches come from {1..9, A +- 3, 2A +- 3}: nothing beyond the capped grids (the edge table has those)."""
    rng = np.random.default_rng(seed)
    return [draw_case(rng, cus, name=f"seed{seed}.{i}") for i in range(count)]
