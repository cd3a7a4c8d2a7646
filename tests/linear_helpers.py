"""Generator, float64 reference, checker and route model for ffh_linear_fwd / ffh_linear_bwd_ex (include/ff_hip.h).

Used by tests/test_linear_sweep_cpu.py (the oracle library, on a CPU: proves the harness) and tests/test_gpu_linear_sweep.py (the HIP kernels of
csrc/linear.hip and csrc/linear_sk.hip).  The reference is plain numpy in float64, written from the contract in the header: nothing here calls
the oracle library or restates a kernel's arithmetic.  Buf, the backends, act64, LIPSCHITZ and the sentinel scheme are tests/chain_helpers.py's.

What is compared.  Every quantity is held against the reference applied to the values the library itself left in the inputs it consumed, so
every bound is the bound of one sum and nothing compounds:

  forward    y        vs  act(x @ w.T + bias)
  backward   dy       bit-identical to before with PREMASKED, with act NONE, with ONLY_DX + ReLU, and with ONLY_DW + Sigmoid (the header: the
                      ONLY_DX call has transformed it); exactly where(y > 0, dy, 0) with a live ReLU; dy * y * (1 - y) with a live Sigmoid
             dw, db   vs  dw0 + dy'.T @ x, db0 + dy'.sum(0)          dy' = the library's final dy (ONLY_DX + ReLU: the masked view of it)
             dx       vs  [dx0 +] (dy' @ w) [x > 0]                   in the plain buffer, or in the column map's destinations
             colsum   vs  colsum0 + dx.sum(0)                         dx as the library stored it

The bound is the project's own, |got - ref| <= 1e-5 * mass * L + 8 * eps32 * |ref|: mass = the sum of the absolute values of the terms (the
initial contents of an accumulated buffer included), L = the activation's Lipschitz constant.  No absolute floor: where mass == 0 (masked
elements) the result has to be exactly 0; a case with integer-valued operands (Case.integer) has to match exactly everywhere.

Every buffer carries NaN sentinels around its [rows][cols] block (padding columns, offset, tail): outputs must keep them, inputs must be
bit-identical after the call, and what a flag or a declined request excludes (dw / db under ONLY_DX, dx under ONLY_DW, the plain dx when the
column map is taken, the destinations when it is declined, colsum when it is declined) must be untouched as a whole.  (The oracle library
stores dx and then copies it through the map; the distributed host tests lean on that, so there its plain dx is compared, not required
untouched.  The HIP library is held to the header: the map INSTEAD of dx.)

One deviation from the letter of "ONLY_DX leaves dw and db untouched": with a live Sigmoid the header gives db to the ONLY_DX call ("in-place
activation gradient + db first") and takes it from the ONLY_DW call; the checker follows the header.

Routes.  route_fwd / route_bwd restate the dispatch predicates of the HIP library (sk_plan, plan_glds, the launch_gemm tile choice, the skinny
and thin conditions) as a function of the CU count; the GPU test asserts ffh_linear_last_route against them, and every edge case names the
kernel family it is there for (Case.want), which the CPU test asserts of the model at 256 CUs.
"""
import ctypes as C
import re

import numpy as np

from dlrm_flexflow_amd import capi
from chain_helpers import Buf, HostBackend, TorchBackend, act64, LIPSCHITZ, num_cus, SENTINEL_BITS, EPS32, TOL, TAIL  # noqa: F401

NONE, RELU, SIG, GELU = capi.AC_MODE_NONE, capi.AC_MODE_RELU, capi.AC_MODE_SIGMOID, capi.AC_MODE_GELU
OVERWRITE, ONLY_DW, ONLY_DX, PREMASKED, MASK_BY_X = (capi.LINEAR_DX_OVERWRITE, capi.LINEAR_ONLY_DW, capi.LINEAR_ONLY_DX, capi.LINEAR_DY_PREMASKED,
                                                     capi.LINEAR_DX_MASK_BY_X)
MATH_SPLIT_ALL = 3          # FFH_MATH_FP32_SPLIT_BF16X3_ALL
TABLE_CUS = 256             # the CU count the edge table's shapes were derived for (MI355X)


def _f64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# a case
class Case:
    """One ffh_linear_fwd (kind "fwd") or ffh_linear_bwd_ex (kind "bwd") call."""

    def __init__(self, name, kind, in_dim, out_dim, batch, act=NONE, flags=0, seed=0, ldx=None, x_off=0, ldy=None, y_off=0, lddy=None, dy_off=0,
                 lddx=None, dx_off=0, w_off=0, bias=True, bias_off=0, db=True, dx=True, forked=False, det=False, cmap=False, cmap_ncols=None,
                 colsum=False, colsum_ncols=None, scratch=True, integer=False, want=()):
        assert kind in ("fwd", "bwd")
        self.name, self.kind, self.in_dim, self.out_dim, self.batch, self.act, self.flags, self.seed = name, kind, int(in_dim), int(out_dim), int(batch), act, flags, seed
        self.ldx, self.x_off = (in_dim if ldx is None else ldx), x_off
        self.ldy, self.y_off = (out_dim if ldy is None else ldy), y_off
        self.lddy, self.dy_off = (out_dim if lddy is None else lddy), dy_off
        self.lddx, self.dx_off = (in_dim if lddx is None else lddx), dx_off
        self.w_off, self.bias, self.bias_off, self.db, self.dx = w_off, bias, bias_off, db, dx
        self.forked, self.det, self.scratch, self.integer = forked, det, scratch, integer
        self.cmap, self.cmap_ncols = cmap, (in_dim if cmap_ncols is None else cmap_ncols)
        self.colsum, self.colsum_ncols = colsum, (in_dim if colsum_ncols is None else colsum_ncols)
        self.want = (want,) if isinstance(want, str) else tuple(want)

    def has(self, flag):
        return bool(self.flags & flag)

    def __repr__(self):
        return (f"Case({self.name}: {self.kind} B={self.batch} {self.in_dim}->{self.out_dim} act={self.act} flags={self.flags} ldx={self.ldx}+{self.x_off} "
                f"ldy={self.ldy}+{self.y_off} lddy={self.lddy}+{self.dy_off} lddx={self.lddx}+{self.dx_off} w+{self.w_off} bias={self.bias}+{self.bias_off} "
                f"db={self.db} dx={self.dx} forked={self.forked} det={self.det} cmap={self.cmap}/{self.cmap_ncols} colsum={self.colsum}/{self.colsum_ncols} "
                f"scratch={self.scratch} integer={self.integer})")


def make_inputs(case):
    """Operands of order one (or small integers), the same for a given case on every backend."""
    rng = np.random.default_rng([case.seed, case.in_dim, case.out_dim, case.batch, case.flags])
    B, i, o = case.batch, case.in_dim, case.out_dim
    if case.integer:
        assert case.act in (NONE, RELU)
        draw = lambda *shape: rng.integers(-2, 3, shape).astype(np.float64)
        w = draw(o, i)
    else:
        draw = lambda *shape: rng.uniform(-1, 1, shape)
        w = draw(o, i) * np.sqrt(3.0 / i)
    inp = {"w": w.astype(np.float32), "b": (draw(o) * (1.0 if case.integer else 0.5)).astype(np.float32)}
    x = draw(B, i)
    if case.kind == "bwd" and case.has(MASK_BY_X):
        x = np.maximum(x, 0)          # the output of a ReLU
    inp["x"] = x.astype(np.float32)
    if case.kind == "bwd":
        # the float64 forward rounded to float32: the masks are decided on values both sides share
        y = act64(_f64(inp["x"]) @ _f64(inp["w"]).T + _f64(inp["b"]), case.act).astype(np.float32)
        g = draw(B, o)
        if case.has(PREMASKED) and case.act == RELU:
            g = np.where(y > 0, g, 0.0)
        inp.update(y=y, g=g.astype(np.float32), dx0=draw(B, i).astype(np.float32), dw0=draw(o, i).astype(np.float32), db0=draw(o).astype(np.float32),
                   cs0=draw(case.colsum_ncols).astype(np.float32))
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# the column map: three destinations with different leading dimensions, columns out of order, boundaries not at multiples of 4
def cmap_layout(ncols):
    """(dest, col) of every dX column, and the (width, ld) of the three destinations."""
    c1, c2 = max(1, (ncols // 3) | 1), max(2, (2 * ncols // 3) | 1)
    if not c1 < c2 < ncols:
        c1, c2 = 1, 2
    slot = np.random.default_rng(ncols).permutation(ncols)
    start = np.array([0, c1, c2])
    dest = np.searchsorted(start, slot, side="right") - 1
    widths = [c1, c2 - c1, ncols - c2]
    return dest, slot - start[dest], [(widths[0], widths[0] + 3), (widths[1], widths[1]), (widths[2], widths[2] + 8)]


class ColDest(C.Structure):
    """struct ffh_col_dest"""
    _fields_ = [("base", C.c_void_p), ("ld", C.c_int64)]


# ---------------------------------------------------------------------------------------------------------------------------
# the calls
class Result:
    def __init__(self, case, inp, rc, route, **kw):
        self.case, self.inp, self.rc, self.route = case, inp, rc, route
        self.scatter_used = self.colsum_used = 0
        self.is_hip = False
        self.__dict__.update(kw)


_STREAMS = {}


def _stream(lib, which):
    """A stream of the library's, made once: "bare" never gets scratch reserved, "dw" is the second stream of the forked calls."""
    key = (id(lib), which)
    if key not in _STREAMS:
        s = C.c_void_p()
        lib.check(lib.lib.ffh_stream_create(lib.ctx, C.byref(s)), "ffh_stream_create")
        _STREAMS[key] = s
    return _STREAMS[key]


def _finish(lib, be, streams):
    for s in streams:
        if s is not None:
            lib.check(lib.lib.ffh_stream_sync(lib.ctx, s), "ffh_stream_sync")
    be.sync()


def run_fwd(lib, be, case, inp=None):
    inp = inp or make_inputs(case)
    B, i, o = case.batch, case.in_dim, case.out_dim
    X = Buf(be, B, i, case.ldx, case.x_off, inp["x"])
    W = Buf(be, o, i, i, case.w_off, inp["w"])
    Bi = Buf(be, 1, o, o, case.bias_off, inp["b"]) if case.bias else None
    Y = Buf(be, B, o, case.ldy, case.y_off)
    s = None if case.scratch else _stream(lib, "bare")
    be.sync()
    rc = lib.lib.ffh_linear_fwd(lib.ctx, X.ptr, case.ldx, Y.ptr, case.ldy, W.ptr, Bi.ptr if Bi else None, i, o, B, case.act, s)
    route = (lib.lib.ffh_linear_last_route(lib.ctx) or b"").decode()
    _finish(lib, be, [s])
    inputs = [("x", X), ("w", W)] + ([("bias", Bi)] if Bi else [])
    for _, b in inputs + [("y", Y)]:
        b.fetch()
    return Result(case, inp, rc, route, Y=Y, outputs=[("y", Y)], inputs=inputs)


def run_bwd(lib, be, case, inp=None):
    inp = inp or make_inputs(case)
    B, i, o = case.batch, case.in_dim, case.out_dim
    X = Buf(be, B, i, case.ldx, case.x_off, inp["x"])
    W = Buf(be, o, i, i, case.w_off, inp["w"])
    Y = Buf(be, B, o, case.ldy, case.y_off, inp["y"])
    DY = Buf(be, B, o, case.lddy, case.dy_off, inp["g"])
    DW = Buf(be, o, i, i, 0, inp["dw0"])
    DB = Buf(be, 1, o, o, 0, inp["db0"]) if case.db else None
    DX = Buf(be, B, i, case.lddx, case.dx_off, inp["dx0"]) if case.dx else None
    dests, cmap_h, CS = [], None, None
    if case.cmap:
        n = case.cmap_ncols
        dest, col, shapes = cmap_layout(n)
        dests = [Buf(be, B, wd, ld, 0) for wd, ld in shapes]
        table = np.zeros((n, 2), np.int64)
        for k in range(n):
            table[k] = (dests[dest[k]].ptr + 4 * int(col[k]), dests[dest[k]].ld)
        cmap_h = be.upload(table.ravel())
    if case.colsum:
        CS = Buf(be, 1, case.colsum_ncols, case.colsum_ncols, 0, inp["cs0"])
    s = None if case.scratch else _stream(lib, "bare")
    s_dw = _stream(lib, "dw") if case.forked else None
    be.sync()
    if case.det:
        lib.check(lib.lib.ffh_ctx_set_deterministic(lib.ctx, 1), "deterministic")
    try:
        if case.cmap:
            lib.check(lib.lib.ffh_linear_bwd_set_dx_scatter(lib.ctx, be.addr(cmap_h), case.cmap_ncols, None), "set_dx_scatter")
        if case.colsum:
            lib.check(lib.lib.ffh_linear_bwd_set_dx_colsum(lib.ctx, CS.ptr, case.colsum_ncols), "set_dx_colsum")
        rc = lib.lib.ffh_linear_bwd_ex(lib.ctx, X.ptr, case.ldx, DX.ptr if DX else None, case.lddx, Y.ptr, case.ldy, DY.ptr, case.lddy, W.ptr, DW.ptr,
                                       DB.ptr if DB else None, i, o, B, case.act, case.flags, s, s_dw)
        route = (lib.lib.ffh_linear_last_route(lib.ctx) or b"").decode()
        su, cu = lib.lib.ffh_linear_dx_scatter_used(lib.ctx), lib.lib.ffh_linear_dx_colsum_used(lib.ctx)
        _finish(lib, be, [s, s_dw])
    finally:
        if case.det:
            lib.check(lib.lib.ffh_ctx_set_deterministic(lib.ctx, 0), "deterministic")
    inputs = [("x", X), ("w", W), ("y", Y)]
    outs = [("dy", DY), ("dw", DW)] + ([("db", DB)] if DB else []) + ([("dx", DX)] if DX else [])
    outs += [(f"dest{k}", d) for k, d in enumerate(dests)] + ([("colsum", CS)] if CS else [])
    for _, b in inputs + outs:
        b.fetch()
    return Result(case, inp, rc, route, is_hip=be.is_hip, DY=DY, DW=DW, DB=DB, DX=DX, dests=dests, CS=CS, outputs=outs, inputs=inputs, scatter_used=su, colsum_used=cu,
                  keepalive=cmap_h)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker
class Report:
    def __init__(self):
        self.violations, self.mass, self.worst = [], {}, {}

    def ok(self):
        return not self.violations

    def __str__(self):
        return "\n".join(self.violations)


WORST = {}       # output kind -> worst |got - ref| / bound seen in this process (a measurement, not a check)


def _compare(rep, name, got, ref, mass, lip=1.0, exact=False):
    got, ref = _f64(got), _f64(ref)
    mass = _f64(mass) + np.zeros_like(ref)
    rep.mass[name] = mass
    bound = np.zeros_like(ref) if exact else TOL * mass * lip + 8 * EPS32 * np.abs(ref)
    err = np.abs(got - ref)
    bad = ~(err <= bound)            # (a NaN is bad)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    rep.worst[name] = worst
    kind = name.rstrip("0123456789")
    WORST[kind] = max(WORST.get(kind, 0.0), worst if np.isfinite(worst) else 0.0)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.nan_to_num(ratio, nan=np.inf, posinf=1e300), -1.0))), bad.shape)
        rep.violations.append(f"{name}: {int(bad.sum())} of {bad.size} beyond {'0 (exact)' if exact else f'{TOL} * mass * {lip} + 8 eps |ref|'}; worst at {i}: "
                              f"got {got[i]!r} ref {ref[i]!r} mass {mass[i]:.3e} bound {bound[i]:.3e}")


def _buffers(rep, res):
    for name, buf in res.outputs:
        if not buf.padding_intact():
            bad = np.flatnonzero((buf.host.view(np.uint32) != SENTINEL_BITS) & ~buf.valid)
            rep.violations.append(f"{name}: {bad.size} padding element(s) overwritten, first at flat index {int(bad[0])} (ld {buf.ld}, offset {buf.off})")
    for name, buf in res.inputs:
        if not buf.untouched():
            rep.violations.append(f"{name}: an input was modified")


def _untouched(rep, name, buf, why):
    if buf is not None and not buf.untouched():
        rep.violations.append(f"{name}: written although {why}")


def check_fwd(res):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    x, w = _f64(inp["x"]), _f64(inp["w"])
    b = _f64(inp["b"]) if case.bias else np.zeros(case.out_dim)
    _compare(rep, "y", res.Y.get(), act64(x @ w.T + b, case.act), np.abs(x) @ np.abs(w).T + np.abs(b), LIPSCHITZ[case.act], case.integer)
    _buffers(rep, res)
    return rep


def must_decline_scatter(case):
    """The contract's own exclusions (every library): an accumulating call, another width, no data gradient."""
    return not case.has(OVERWRITE) or case.cmap_ncols != case.in_dim or case.has(ONLY_DW) or not case.dx


def must_decline_colsum(case):
    return not case.has(OVERWRITE) or case.colsum_ncols != case.in_dim or case.has(ONLY_DW) or not case.dx or case.cmap


def check_bwd(res):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    x, w, y, g = _f64(inp["x"]), _f64(inp["w"]), _f64(inp["y"]), _f64(inp["g"])
    only_dx, only_dw, ex = case.has(ONLY_DX), case.has(ONLY_DW), case.integer
    act = NONE if case.has(PREMASKED) else case.act
    dy_after = res.DY.get()
    # dy
    if act == NONE or (act == RELU and only_dx) or (act == SIG and only_dw):
        if dy_after.tobytes() != inp["g"].tobytes():
            rep.violations.append("dy: modified although the call must leave it as it is")
        rep.mass["dy"] = np.abs(g)
        eff = np.where(y > 0, g, 0.0) if act == RELU else g
    elif act == RELU:
        _compare(rep, "dy", dy_after, np.where(y > 0, g, 0.0), np.where(y > 0, np.abs(g), 0.0), exact=True)
        eff = _f64(dy_after)
    else:
        _compare(rep, "dy", dy_after, g * y * (1.0 - y), np.abs(g), LIPSCHITZ[SIG])
        eff = _f64(dy_after)
    # dw, db
    if only_dx:
        _untouched(rep, "dw", res.DW, "ONLY_DX")
    else:
        _compare(rep, "dw", res.DW.get(), _f64(inp["dw0"]) + eff.T @ x, np.abs(_f64(inp["dw0"])) + np.abs(eff).T @ np.abs(x), exact=ex)
    if res.DB is not None:
        if (only_dw if act == SIG else only_dx):
            _untouched(rep, "db", res.DB, "this half of the split call does not own the bias gradient")
        else:
            _compare(rep, "db", res.DB.get()[0], _f64(inp["db0"]) + eff.sum(0), np.abs(_f64(inp["db0"])) + np.abs(eff).sum(0), exact=ex)
    # dx, in the plain buffer or in the destinations
    if case.cmap and must_decline_scatter(case) and res.scatter_used:
        rep.violations.append("column map: taken by a call the contract excludes")
    if case.colsum and must_decline_colsum(case) and res.colsum_used:
        rep.violations.append("column sums: taken by a call the contract excludes")
    if not case.cmap and res.scatter_used:
        rep.violations.append("column map: reported as used without a request")
    if not case.colsum and res.colsum_used:
        rep.violations.append("column sums: reported as used without a request")
    if res.DX is not None:
        if only_dw:
            _untouched(rep, "dx", res.DX, "ONLY_DW")
        else:
            ref, mass = eff @ w, np.abs(eff) @ np.abs(w)
            if case.has(MASK_BY_X):
                keep = x > 0
                ref, mass = np.where(keep, ref, 0.0), np.where(keep, mass, 0.0)
            if not case.has(OVERWRITE):
                ref, mass = ref + _f64(inp["dx0"]), mass + np.abs(_f64(inp["dx0"]))
            if res.scatter_used and case.cmap:
                if res.is_hip:
                    _untouched(rep, "dx", res.DX, "the column map was taken")
                else:       # the oracle library stores the gradient in dx AND copies it through the map (oracle/ffh_oracle.c): both are held to the bound
                    _compare(rep, "dx", res.DX.get(), ref, mass, exact=ex)
                dest, col, _ = cmap_layout(case.cmap_ncols)
                for k, d in enumerate(res.dests):
                    sel = np.flatnonzero(dest == k)
                    order = sel[np.argsort(col[sel])]
                    _compare(rep, f"dest{k}", d.get(), ref[:, order], mass[:, order], exact=ex)
            else:
                _compare(rep, "dx", res.DX.get(), ref, mass, exact=ex)
    if not (res.scatter_used and case.cmap):
        for k, d in enumerate(res.dests):
            _untouched(rep, f"dest{k}", d, "the column map was declined")
    if res.CS is not None:
        if res.colsum_used:
            stored = _f64(res.DX.get())
            _compare(rep, "colsum", res.CS.get()[0], _f64(inp["cs0"]) + stored.sum(0), np.abs(_f64(inp["cs0"])) + np.abs(stored).sum(0), exact=ex)
        else:
            _untouched(rep, "colsum", res.CS, "the column sums were declined")
    _buffers(rep, res)
    return rep


# ---------------------------------------------------------------------------------------------------------------------------
# the route the HIP library has to report: a restatement of its dispatch predicates (csrc/linear.hip, csrc/linear_sk.hip)
def _al(off, ld):
    return off % 4 == 0 and ld % 4 == 0


def _cdiv(a, b):
    return -(-a // b)


def sk_plan(cus, form, M, N, K, aligned, epi, colmap=False, mask=False, det=False):
    """The persistent kernel's plan (tile rows, stream-K or not), or None.  form "fwd" / "dx" / "dw"; epi "store" / "add" / "atomic"."""
    nw = M * N if form == "dw" else N * K
    if form != "fwd" and nw < 65536:
        return None
    if M % 128 or N % 128 or K % 64 or not aligned:
        return None
    if colmap and (form != "dx" or epi != "store" or mask):
        return None
    G = cus & ~7
    if G < 8:
        return None
    ntiles, nk = (M // 128) * (N // 128), K // 64
    whole = not (ntiles < G or ntiles * 100 < _cdiv(ntiles, G) * G * 80)
    if form == "dw":
        return None if det or ntiles * nk < 8 * G else dict(rows=128, split=False, whole=True)
    rounds = _cdiv(ntiles, G)
    idle_it = (rounds * G - ntiles) * nk // G
    if ntiles < G and M % 64 == 0 and nk >= 8:
        nt64 = (M // 64) * (N // 128)
        if nt64 <= G and nt64 * 100 >= G * 80:
            return dict(rows=64, split=False, whole=True)
    split = idle_it >= 2 and ntiles * nk >= 8 * G and epi == "store"
    if not split and not whole:
        return None
    return dict(rows=128, split=split, whole=whole)


def plan_glds(cus, M, N, K, a_al, b_al, a_extent, b_extent, atomic, det=False, min_work=1.5e8, min_k=128):
    """The LDS-DMA kernel's plan (tile rows, workgroups, splits), or None."""
    if det and atomic:
        return None
    if atomic and float(M) * N * K >= 1.0e9 and K <= 16384:
        return None
    if not a_al or not b_al or a_extent % 4 or b_extent % 4:
        return None
    if float(M) * N * K < min_work or M < 64 or N < 64 or K < min_k:
        return None
    tiles = _cdiv(M, 64) * _cdiv(N, 64)
    bm = 64
    if not atomic and tiles < (3 * cus) // 4:
        bm, tiles = 32, _cdiv(M, 32) * _cdiv(N, 64)
    if tiles > (3 * cus) // 2:
        return None
    splitk = 1
    if atomic:
        want = max(1, min(cus // tiles, (K + 255) // 256))
        kps = _cdiv(_cdiv(K, want), 64) * 64
        splitk = _cdiv(K, kps)
    return dict(bm=bm, wgs=_cdiv(M, bm) * _cdiv(N, 64) * splitk, splitk=splitk)


def gemm_cfg(cus, M, N, K, atomic, cmap=False):
    """launch_gemm's tile choice: 0 = 128 x 128, 1 = 64 x 64, 2 = 32 x 32 with the waves splitting K."""
    if atomic:
        work = float(M) * N * K
        cfg = 0 if work >= 3e9 and M >= 128 and N >= 128 else (1 if work >= 4e8 else 2)
    elif _cdiv(M, 128) * _cdiv(N, 128) >= 2 * cus and M >= 128 and N >= 128:
        cfg = 0
    elif _cdiv(M, 64) * _cdiv(N, 64) >= 2 * cus or K < 64:
        cfg = 1
    else:
        cfg = 2
    return 1 if cmap and cfg == 2 else cfg


def _gemm_tok(name, cfg):
    t = (128, 64, 32)[cfg]
    return f"{name}|f32_{t}x{t}_cfg{cfg}"


def _sk_tok(name, p, split, colmap=False, colsum=False):
    return f"{name}|sk_{p['rows']}x128x64" + ("|colmap" if colmap else "") + ("|streamk" if split else "") + ("|colsum" if colsum else "")


def route_fwd(c, cus):
    i, o, B = c.in_dim, c.out_dim, c.batch
    if o <= 4:
        return ["linear_fwd|skinny"]
    if i <= 16 and o >= 64 and B < 16384:
        return ["linear_fwd|thin"]
    toks = []
    al = _al(c.x_off, c.ldx) and c.w_off % 4 == 0 and i % 4 == 0 and _al(c.y_off, c.ldy) and (not c.bias or c.bias_off % 4 == 0)
    p = sk_plan(cus, "fwd", B, o, i, al, "store")
    if p:
        if p["split"] and not c.scratch:
            toks.append("linear_fwd gemm|no_scratch_on_this_stream")
            if p["whole"]:
                return toks + [_sk_tok("linear_fwd gemm", p, False)]
        else:
            return [_sk_tok("linear_fwd gemm", p, p["split"])]
    g = plan_glds(cus, B, o, i, _al(c.x_off, c.ldx), c.w_off % 4 == 0 and i % 4 == 0, i, i, False)
    if g:
        return toks + [f"linear_fwd gemm (lds-dma)|glds_{g['bm']}x64_s{2 if g['wgs'] > cus else 3}"]
    return toks + [_gemm_tok("linear_fwd gemm", gemm_cfg(cus, B, o, i, False))]


def route_bwd(c, cus):
    """(tokens, column map taken, column sums taken) of one ffh_linear_bwd_ex call."""
    st = dict(toks=[], scatter=0, colsum=0)
    _bwd_impl(st, c, cus, not c.has(ONLY_DX), not c.has(ONLY_DW), c.dx, c.forked)
    return st["toks"], st["scatter"], st["colsum"]


def _bwd_impl(st, c, cus, do_dw, do_dx, has_dx, forked):
    i, o, B, toks = c.in_dim, c.out_dim, c.batch, st["toks"]
    act = NONE if c.has(PREMASKED) else c.act
    mask, overwrite, separate, relu = c.has(MASK_BY_X), c.has(OVERWRITE), act == SIG, act == RELU
    x_al, dx_al, dy_al, w_al = _al(c.x_off, c.ldx), _al(c.dx_off, c.lddx), _al(c.dy_off, c.lddy), c.w_off % 4 == 0
    if ((o <= 4 and i <= 1024) or (o <= 16 and i <= 256)) and i % 4 == 0 and x_al and w_al and (not has_dx or dx_al) and not c.det:
        toks.append("linear_bwd|skinny")
        return
    want_dx = has_dx and do_dx
    epi = "store" if overwrite else "add"
    scatter_pending = c.cmap and c.cmap_ncols == i and overwrite
    scatter_sk = want_dx and scatter_pending and not c.det
    colsum_sk = want_dx and c.colsum and c.colsum_ncols == i and overwrite and not scatter_pending and not c.det
    ok = (do_dw or want_dx) and not (relu and not do_dw) and not (want_dx and scatter_pending and not scatter_sk)
    pw = sk_plan(cus, "dw", o, i, B, dy_al and x_al and i % 4 == 0, "atomic", det=c.det)
    px = sk_plan(cus, "dx", B, i, o, dy_al and w_al and i % 4 == 0 and (scatter_sk or dx_al) and (not mask or x_al), epi, colmap=scatter_sk, mask=mask) \
        if want_dx else None
    if ok and do_dw and want_dx and not relu and not separate and not scatter_pending and not pw and px:
        _bwd_impl(st, c, cus, False, True, True, False)
        _bwd_impl(st, c, cus, True, False, False, False)
        return
    if ok and (not do_dw or pw) and (not want_dx or px):
        if want_dx:
            launched = True
            if px["split"] and not c.scratch:
                toks.append("linear_bwd dx gemm|no_scratch_on_this_stream")
                launched = px["whole"]
            if launched:
                toks.append(_sk_tok("linear_bwd dx gemm", px, px["split"] and c.scratch, scatter_sk, colsum_sk and not scatter_sk))
                st["colsum"] = int(colsum_sk)
            else:
                toks.append(_gemm_tok("linear_bwd dx gemm (column map)" if scatter_sk else "linear_bwd dx gemm", gemm_cfg(cus, B, i, o, False, scatter_sk)))
            st["scatter"] = int(scatter_sk)
        if do_dw:
            toks.append(_sk_tok("linear_bwd dw gemm", pw, False))
        return
    if do_dw and do_dx and has_dx and not relu and not c.det:
        gx = plan_glds(cus, B, i, o, dy_al, w_al and i % 4 == 0, o, i, False, min_k=64)
        gw = plan_glds(cus, o, i, B, dy_al, x_al, o, i, True, c.det, min_k=64)
        if gx and gw:
            na8 = (gx["wgs"] + 7) & ~7
            toks.append(f"linear_bwd dx+dw|glds_dual_{gx['bm']}x64_s{2 if na8 + gw['wgs'] > cus else 3}")
            st["scatter"] = int(bool(scatter_pending))
            return
    forked_ = do_dw and do_dx and forked
    if do_dw:
        gw = None if relu else plan_glds(cus, o, i, B, dy_al, x_al, o, i, True, c.det)
        if gw:
            toks.append(f"linear_bwd dw gemm (lds-dma)|glds_64x64_s{2 if gw['wgs'] > cus else 3}")
        else:
            toks.append(_gemm_tok("linear_bwd dw gemm", gemm_cfg(cus, o, i, B, True)))
    if want_dx:
        if not relu:
            gx = plan_glds(cus, B, i, o, dy_al, w_al and i % 4 == 0, o, i, False)
            if gx:
                toks.append(f"linear_bwd dx gemm (lds-dma)|glds_{gx['bm']}x64_s{2 if gx['wgs'] > cus else 3}")
                return
        scatter = bool(scatter_pending and not c.det)
        masking = (forked_ or not do_dw) and relu
        name = "linear_bwd dx gemm" + {(0, 0): "", (0, 1): " (column map)", (1, 0): " (masking)", (1, 1): " (masking, column map)"}[(int(masking), int(scatter))]
        toks.append(_gemm_tok(name, gemm_cfg(cus, B, i, o, False, scatter)))
        st["scatter"] = int(scatter)


def normalize_route(route):
    """The library's tokens without their split and workgroup counts (route_fwd / route_bwd do not predict those)."""
    return [re.sub(r"\|(splitk|wgs)=\d+", "", t) for t in route.split(";") if t]


def expected_route(case, cus):
    return (route_fwd(case, cus), 0, 0) if case.kind == "fwd" else route_bwd(case, cus)


def check_route(res, cus):
    case, out = res.case, []
    toks, scatter, colsum = expected_route(case, cus)
    got = normalize_route(res.route)
    if got != toks:
        out.append(f"route {got}, expected {toks}")
    if case.kind == "bwd":
        if res.scatter_used != scatter:
            out.append(f"ffh_linear_dx_scatter_used = {res.scatter_used}, expected {scatter}")
        if res.colsum_used != colsum:
            out.append(f"ffh_linear_dx_colsum_used = {res.colsum_used}, expected {colsum}")
        if case.det:
            out += [f"deterministic mode: {t!r} is not an ordered route" for t in res.route.split(";")
                    if "skinny" in t or ("dw" in t.split("|")[0] and ("|sk_" in t or "glds" in t or not t.endswith("splitk=1")))]
    if cus == TABLE_CUS:
        joined = ";".join(got) + f";scatter_used={res.scatter_used};colsum_used={res.colsum_used}"
        out += [f"route {got} does not reach {w!r}, the kernel this case is in the table for" for w in case.want if w not in joined]
    return out


def model_reaches(case, cus=TABLE_CUS):
    """What check_route asserts of a 256-CU device, asked of the model alone: the tokens in Case.want that it does not predict."""
    toks, scatter, colsum = expected_route(case, cus)
    joined = ";".join(toks) + f";scatter_used={scatter};colsum_used={colsum}"
    return [w for w in case.want if w not in joined]


def run_and_check(lib, be, case, cus=None, routes=True):
    """Run one case, return (result, report); on the HIP library the route is part of the report."""
    res = run_fwd(lib, be, case) if case.kind == "fwd" else run_bwd(lib, be, case)
    rep = check_fwd(res) if case.kind == "fwd" else check_bwd(res)
    if be.is_hip and routes and res.rc == capi.FFH_OK and case.batch > 0:
        rep.violations += check_route(res, cus)
    return res, rep


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed edge table (shapes derived for 256 CUs)
ACTS_FWD = (NONE, RELU, SIG, GELU)
ACTS_BWD = (RELU, SIG, NONE)


def _fwd_table(t):
    k, cases = 0, []
    for o in (1, 2, 3, 4):
        for i in (1, 63, 64, 65, 1500):
            for B in (1, 5, 8197):
                odd = k % 3 == 1
                cases.append(Case(f"fwd-skinny-{B}x{i}->{o}", "fwd", i, o, B, ACTS_FWD[k % 4], bias=k % 5 != 0, ldx=i + (3 if odd else 0), ldy=o + (1 if odd else 0),
                                  x_off=1 if k % 4 == 2 else 0, y_off=k % 2, want="linear_fwd|skinny", integer=k % 7 == 3 and ACTS_FWD[k % 4] in (NONE, RELU)))
                k += 1
    t["fwd-skinny"] = cases
    cases = []
    for i in (1, 2, 3, 13, 15, 16):
        for o in (64, 65, 255, 257, 300):
            for B in (1, 31, 33):
                cases.append(Case(f"fwd-thin-{B}x{i}->{o}", "fwd", i, o, B, ACTS_FWD[k % 4], bias=k % 5 != 0, ldx=i + (k % 3), ldy=o + (k % 2) * 3, x_off=k % 2,
                                  integer=k % 7 == 3 and ACTS_FWD[k % 4] in (NONE, RELU), want="linear_fwd|thin"))
                k += 1
    cases.append(Case("fwd-not-thin-out63", "fwd", 13, 63, 33, RELU, want="linear_fwd gemm|f32_64x64_cfg1"))
    cases.append(Case("fwd-not-thin-batch16384", "fwd", 13, 64, 16384, RELU, want="linear_fwd gemm|f32_64x64_cfg1"))
    t["fwd-thin"] = cases
    t["fwd-persistent-whole-tiles"] = [Case("fwd-sk-128", "fwd", 64, 2048, 2048, RELU, ldx=68, ldy=2052, want="linear_fwd gemm|sk_128x128x64"),
                                       Case("fwd-sk-128-int", "fwd", 64, 2048, 2048, NONE, bias=False, integer=True, want="linear_fwd gemm|sk_128x128x64"),
                                       Case("fwd-sk-decline-bias-misaligned", "fwd", 64, 2048, 2048, SIG, bias_off=1, want="linear_fwd gemm|f32_64x64_cfg1"),
                                       Case("fwd-sk-decline-ldx", "fwd", 64, 2048, 2048, GELU, ldx=66, want="linear_fwd gemm|f32_64x64_cfg1")]
    t["fwd-persistent-64-row-tiles"] = [Case("fwd-sk-64", "fwd", 512, 2048, 1024, GELU, ldy=2056, want="linear_fwd gemm|sk_64x128x64")]
    t["fwd-persistent-stream-k"] = [Case("fwd-sk-streamk", "fwd", 1344, 1280, 1280, RELU, ldx=1348, want="sk_128x128x64|streamk"),
                                    Case("fwd-sk-streamk-no-scratch", "fwd", 1344, 1280, 1280, SIG, scratch=False,
                                         want=("linear_fwd gemm|no_scratch_on_this_stream", "linear_fwd gemm|f32_32x32_cfg2"))]
    glds = [(300, 1024, 512, "glds_32x64_s3"), (1024, 256, 832, "glds_64x64_s3"), (1280, 256, 1088, "glds_64x64_s2"), (2000, 256, 320, "glds_32x64_s2")]
    cases = []
    for n, (B, i, o, tok) in enumerate(glds):
        cases.append(Case(f"fwd-glds-{B}x{i}->{o}", "fwd", i, o, B, ACTS_FWD[n % 4], bias=n != 2, ldx=i + 4 * (n % 2), ldy=o + n, y_off=n % 2, want=tok))
        o2 = o + 3 if o != 320 else o - 1          # (a sixth tile column would move 2000 x 260 to the 64-row tiles)
        cases.append(Case(f"fwd-glds-{B}x{i + 4}->{o2}", "fwd", i + 4, o2, B, ACTS_FWD[(n + 1) % 4], ldy=o2 + n, want=tok))
    cases.append(Case("fwd-glds-1024x260->835", "fwd", 260, 835, 1024, RELU, want="glds_64x64_s3"))
    cases.append(Case("fwd-glds-int", "fwd", 260, 323, 2000, NONE, integer=True, want="glds_64x64_s3"))
    t["fwd-lds-dma"] = cases
    t["fwd-register-staged-cfg0"] = [Case(f"fwd-cfg0-{B}x{i}->{o}", "fwd", i, o, B, a, ldx=i + p, ldy=o + p, x_off=p, bias=p == 0, want="linear_fwd gemm|f32_128x128_cfg0")
                                     for (B, i, o, a, p) in ((4099, 70, 2049, RELU, 0), (4097, 65, 2047, GELU, 1), (4095, 63, 2049, NONE, 3))]
    t["fwd-register-staged-cfg1"] = [Case(f"fwd-cfg1-{B}x{i}->{o}", "fwd", i, o, B, a, ldx=i + p, ldy=o + p, y_off=p, bias=p != 1, integer=(a == NONE),
                                          want="linear_fwd gemm|f32_64x64_cfg1")
                                     for (B, i, o, a, p) in ((100, 20, 40, SIG, 0), (65, 33, 63, RELU, 1), (63, 31, 65, NONE, 2), (129, 30, 127, GELU, 0))]
    t["fwd-register-staged-cfg2"] = [Case(f"fwd-cfg2-{B}x{i}->{o}", "fwd", i, o, B, a, ldx=i + p, ldy=o + p, x_off=p, bias=p != 1, integer=(a == NONE),
                                          want="linear_fwd gemm|f32_32x32_cfg2")
                                     for (B, i, o, a, p) in ((100, 70, 40, RELU, 0), (33, 65, 31, SIG, 1), (31, 127, 33, NONE, 2), (97, 129, 65, GELU, 3), (32, 66, 32, NONE, 0))]


SKINNY_FLAGS = (0, OVERWRITE, ONLY_DX, ONLY_DW, PREMASKED, MASK_BY_X | OVERWRITE, ONLY_DX | OVERWRITE | MASK_BY_X, PREMASKED | ONLY_DW, MASK_BY_X)


def _bwd_table(t):
    k, cases = 0, []
    pairs = [(o, i) for o in (1, 3, 4) for i in (4, 256, 260, 512, 516, 1024)] + [(o, i) for o in (5, 16) for i in (64, 128, 192, 256)]
    for o, i in pairs:
        for B in (1, 17, 8200):
            fl, act = SKINNY_FLAGS[k % len(SKINNY_FLAGS)], ACTS_BWD[k % 3]
            cases.append(Case(f"bwd-skinny-{B}x{i}->{o}", "bwd", i, o, B, act, fl, ldx=i + 4 * (k % 2), lddx=i + 4 * (k % 3), ldy=o + k % 3, lddy=o + k % 2, y_off=k % 2,
                              dy_off=k % 3, db=k % 4 != 1, dx=k % 11 != 5, integer=(act != SIG and k % 5 == 2), want="linear_bwd|skinny"))
            k += 1
    for o, i in ((1, 1024), (4, 516), (16, 256), (5, 64), (3, 256)):
        cases.append(Case(f"bwd-skinny-last-arriver-16400x{i}->{o}", "bwd", i, o, 16400, ACTS_BWD[k % 3], (0, OVERWRITE)[k % 2], want="linear_bwd|skinny"))
        k += 1
    for o, i in ((1, 512), (4, 260), (16, 128)):          # the Sigmoid layer as its two halves
        cases.append(Case(f"bwd-skinny-sigmoid-only-dx-{i}->{o}", "bwd", i, o, 8200, SIG, ONLY_DX, want="linear_bwd|skinny"))
        cases.append(Case(f"bwd-skinny-sigmoid-only-dw-{i}->{o}", "bwd", i, o, 8200, SIG, ONLY_DW, want="linear_bwd|skinny"))
    t["bwd-skinny"] = cases
    t["bwd-just-outside-skinny"] = [
        Case("bwd-not-skinny-in1028", "bwd", 1028, 1, 300, RELU, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32")),
        Case("bwd-not-skinny-in1022", "bwd", 1022, 3, 77, SIG, OVERWRITE, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32")),
        Case("bwd-not-skinny-dx-misaligned", "bwd", 256, 4, 130, NONE, dx_off=1, lddx=257, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32")),
        Case("bwd-not-skinny-out17", "bwd", 256, 17, 200, RELU, MASK_BY_X, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32")),
        Case("bwd-not-skinny-out1-int", "bwd", 1028, 1, 65, RELU, OVERWRITE, integer=True, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32"))]
    SKX, SKW = "linear_bwd dx gemm|sk_128x128x64", "linear_bwd dw gemm|sk_128x128x64"
    t["bwd-persistent-dx-dw"] = [
        Case("bwd-sk-none-db", "bwd", 512, 512, 8192, NONE, ldx=516, lddy=520, want=(SKX, SKW)),
        Case("bwd-sk-live-relu", "bwd", 512, 512, 8192, RELU, OVERWRITE, forked=True, lddx=516, want=(SKX, SKW)),
        Case("bwd-sk-sigmoid", "bwd", 512, 512, 8192, SIG, db=False, want=(SKX, SKW)),
        Case("bwd-sk-premasked-maskx", "bwd", 512, 512, 8192, RELU, PREMASKED | MASK_BY_X, forked=True, want=(SKX, SKW)),
        Case("bwd-sk-int", "bwd", 512, 512, 8192, RELU, OVERWRITE | MASK_BY_X, integer=True, want=(SKX, SKW))]
    t["bwd-persistent-dx-only"] = [
        Case("bwd-sk64-dx-split-call", "bwd", 2048, 512, 1024, NONE, forked=True, want=("linear_bwd dx gemm|sk_64x128x64", "linear_bwd dw gemm|f32_64x64_cfg1")),
        Case("bwd-streamk-dx-split-call", "bwd", 1280, 1344, 1280, RELU, PREMASKED | OVERWRITE, want=("linear_bwd dx gemm|sk_128x128x64|streamk", "linear_bwd dw gemm")),
        Case("bwd-sk64-live-relu-falls-back", "bwd", 2048, 512, 1024, RELU, want=("linear_bwd dw gemm|f32_64x64_cfg1", "linear_bwd dx gemm|f32")),
        Case("bwd-streamk-live-relu-falls-back", "bwd", 1280, 1344, 1280, RELU, OVERWRITE, want=("linear_bwd dw gemm|f32", "linear_bwd dx gemm|f32"))]
    t["bwd-column-map"] = [
        Case("cmap-sk-whole", "bwd", 512, 512, 8192, NONE, OVERWRITE, cmap=True, want=(SKX + "|colmap", "scatter_used=1")),
        Case("cmap-sk-64", "bwd", 2048, 512, 1024, RELU, OVERWRITE | ONLY_DX | PREMASKED, cmap=True, want=("sk_64x128x64|colmap", "scatter_used=1")),
        Case("cmap-sk-streamk", "bwd", 1280, 1344, 1280, NONE, OVERWRITE | ONLY_DX, cmap=True, want=("sk_128x128x64|colmap|streamk", "scatter_used=1")),
        Case("cmap-glds-pair", "bwd", 512, 256, 2048, NONE, OVERWRITE | MASK_BY_X, cmap=True, want=("glds_dual_64x64_s2", "scatter_used=1")),
        Case("cmap-cfg0", "bwd", 2050, 70, 4099, NONE, OVERWRITE, cmap=True, want=("linear_bwd dx gemm (column map)|f32_128x128_cfg0", "scatter_used=1")),
        Case("cmap-cfg1", "bwd", 42, 20, 100, RELU, OVERWRITE, cmap=True, forked=True, want=("linear_bwd dx gemm (masking, column map)|f32_64x64_cfg1", "scatter_used=1")),
        Case("cmap-cfg2-promoted", "bwd", 42, 70, 100, SIG, OVERWRITE | MASK_BY_X, cmap=True, integer=False, want=("linear_bwd dx gemm (column map)|f32_64x64_cfg1", "scatter_used=1")),
        Case("cmap-int", "bwd", 42, 70, 100, NONE, OVERWRITE, cmap=True, integer=True, want=("(column map)", "scatter_used=1")),
        Case("cmap-declined-accumulating", "bwd", 42, 70, 100, NONE, 0, cmap=True, want="scatter_used=0"),
        Case("cmap-declined-ncols", "bwd", 42, 70, 100, NONE, OVERWRITE, cmap=True, cmap_ncols=41, want="scatter_used=0"),
        Case("cmap-declined-skinny", "bwd", 64, 16, 100, NONE, OVERWRITE, cmap=True, want=("linear_bwd|skinny", "scatter_used=0")),
        Case("cmap-declined-deterministic", "bwd", 42, 70, 100, NONE, OVERWRITE, cmap=True, det=True, want="scatter_used=0")]
    t["bwd-column-sums"] = [
        Case("colsum-taken", "bwd", 512, 512, 8192, NONE, OVERWRITE, colsum=True, want=(SKX + "|colsum", "colsum_used=1")),
        Case("colsum-taken-maskx", "bwd", 512, 512, 8192, RELU, OVERWRITE | MASK_BY_X, colsum=True, want=(SKX + "|colsum", "colsum_used=1")),
        Case("colsum-declined-accumulating", "bwd", 512, 512, 8192, NONE, 0, colsum=True, want=(SKX, "colsum_used=0")),
        Case("colsum-declined-map-pending", "bwd", 512, 512, 8192, NONE, OVERWRITE, colsum=True, cmap=True, want=(SKX + "|colmap", "colsum_used=0")),
        Case("colsum-declined-glds-pair", "bwd", 512, 256, 2048, NONE, OVERWRITE, colsum=True, want=("glds_dual", "colsum_used=0")),
        Case("colsum-declined-register-staged", "bwd", 42, 70, 100, NONE, OVERWRITE, colsum=True, want=("linear_bwd dx gemm|f32", "colsum_used=0"))]
    t["bwd-lds-dma"] = [
        Case("glds-pair", "bwd", 512, 256, 2048, SIG, ldx=516, lddy=260, lddx=520, want="linear_bwd dx+dw|glds_dual_64x64_s2"),
        Case("glds-pair-ragged-batch", "bwd", 512, 256, 2000, NONE, OVERWRITE, db=False, want="linear_bwd dx+dw|glds_dual_64x64"),
        Case("glds-pair-in516", "bwd", 516, 256, 2048, RELU, PREMASKED | MASK_BY_X, want="linear_bwd dx+dw|glds_dual_64x64"),
        Case("glds-pair-int", "bwd", 516, 256, 2000, NONE, OVERWRITE, integer=True, want="linear_bwd dx+dw|glds_dual_64x64"),
        Case("glds-only-dx", "bwd", 516, 256, 2000, NONE, ONLY_DX | OVERWRITE | MASK_BY_X, want="linear_bwd dx gemm (lds-dma)|glds_64x64"),
        Case("glds-only-dx-accumulate", "bwd", 512, 260, 2048, SIG, ONLY_DX, want="linear_bwd dx gemm (lds-dma)|glds_64x64"),
        Case("glds-only-dw-short-last-split", "bwd", 512, 256, 2000, NONE, ONLY_DW, want="linear_bwd dw gemm (lds-dma)|glds_64x64"),
        Case("glds-only-dw-in516", "bwd", 516, 260, 2100, SIG, ONLY_DW, db=False, want="linear_bwd dw gemm (lds-dma)|glds_64x64")]
    DWN, DXN = "linear_bwd dw gemm|f32_", "linear_bwd dx gemm"
    t["bwd-register-staged-fused-mask"] = [
        Case("fused-live-relu-forked", "bwd", 70, 40, 300, RELU, forked=True, want=(DWN + "32x32_cfg2", DXN + " (masking)|f32")),
        Case("fused-live-relu-unforked", "bwd", 70, 40, 300, RELU, OVERWRITE, want=(DWN + "32x32_cfg2", DXN + "|f32")),
        Case("fused-only-dx-relu", "bwd", 70, 72, 300, RELU, ONLY_DX | MASK_BY_X, want=DXN + " (masking)|f32_32x32_cfg2"),
        Case("fused-only-dw-relu", "bwd", 70, 40, 300, RELU, ONLY_DW, db=False, want=DWN + "32x32_cfg2"),
        Case("fused-empty-second-split", "bwd", 70, 40, 100, RELU, forked=True, lddy=44, ldy=41, want=DWN + "32x32_cfg2"),
        Case("fused-empty-second-split-int", "bwd", 66, 33, 128, RELU, OVERWRITE, integer=True, want=DWN + "32x32_cfg2"),
        Case("fused-dw-cfg1", "bwd", 70, 200, 30001, RELU, forked=True, want=DWN + "64x64_cfg1"),
        Case("fused-dw-cfg0", "bwd", 516, 512, 11401, RELU, OVERWRITE, forked=True, want=DWN + "128x128_cfg0")]
    k, cases = 0, []
    for o in (1, 5, 252, 256, 260, 1028):       # a live Sigmoid beside the general kernels: its own pass over dy
        for B, pad in ((77, 0), (2100, 0), (131, 1)):
            cases.append(Case(f"act-pass-{B}->{o}{'-scalar' if pad or o % 4 else ''}", "bwd", 30, o, B, SIG, (0, OVERWRITE)[k % 2], lddy=o + pad, ldy=o + (k % 2) * 4, db=k % 5 != 4,
                              want=("linear_bwd dw gemm|f32", DXN)))
            k += 1
    cases.append(Case("act-pass-live-relu-persistent", "bwd", 512, 512, 8192 + 0, RELU, OVERWRITE, lddy=516, want=(SKX, SKW)))
    t["bwd-act-bwd-bias"] = cases
    t["bwd-deterministic"] = [
        Case("det-skinny", "bwd", 256, 1, 8200, SIG, det=True, want=DWN),
        Case("det-skinny-16", "bwd", 64, 16, 2100, RELU, OVERWRITE, det=True, want=DWN),
        Case("det-persistent-dw", "bwd", 512, 512, 8192, NONE, OVERWRITE, det=True, want=(SKX, DWN)),
        Case("det-lds-dma-dw", "bwd", 512, 256, 2000, NONE, det=True, want=DWN),
        Case("det-atomic", "bwd", 70, 40, 300, RELU, forked=True, det=True, want=DWN)]


def edge_table(cus=TABLE_CUS):
    """name -> list of cases.  The shapes are those derived for 256 CUs; on another CU count the route model still says what each must take."""
    t = {}
    _fwd_table(t)
    _bwd_table(t)
    return t


EDGE_NAMES = list(edge_table())
SPLIT_MODE_GROUPS = [n for n in EDGE_NAMES if any(k in n for k in ("persistent", "lds-dma", "register-staged"))]


# ---------------------------------------------------------------------------------------------------------------------------
# the random generator
def _draw_width(rng):
    m = int(rng.integers(5))
    if m == 0:
        w = int(rng.integers(1, 18))
    elif m == 1:
        w = 4 * int(rng.integers(1, 276))
    elif m == 2:
        w = 64 * int(rng.integers(1, 18)) + int(rng.choice([-4, -1, 0, 1, 4]))
    elif m == 3:
        w = 128 * int(rng.integers(1, 9))
    else:
        w = int(rng.integers(1, 1101))
    return min(max(w, 1), 1100)


def _draw_batch(rng):
    m = int(rng.integers(4))
    if m == 0:
        return int(rng.integers(1, 130))
    if m == 1:
        return 128 * int(rng.integers(1, 33))
    if m == 2:
        return 64 * int(rng.integers(1, 64)) + int(rng.choice([-1, 1]))
    return int(rng.integers(1, 4101))


def draw_case(rng, name="random"):
    kind = "fwd" if rng.random() < 0.4 else "bwd"
    i, o, B = _draw_width(rng), _draw_width(rng), _draw_batch(rng)
    pad = lambda: int(rng.choice([0, 0, 0, 1, 3, 4, 8]))
    off = lambda: int(rng.choice([0, 0, 0, 1, 2, 4]))
    seed = int(rng.integers(1 << 30))
    if kind == "fwd":
        return Case(name, "fwd", i, o, B, int(rng.choice(ACTS_FWD)), seed=seed, ldx=i + pad(), x_off=off(), ldy=o + pad(), y_off=off(), w_off=off(),
                    bias=bool(rng.random() < 0.75), bias_off=off())
    flags = 0
    for f, p in ((OVERWRITE, 0.5), (PREMASKED, 0.3), (MASK_BY_X, 0.4)):
        if rng.random() < p:
            flags |= f
    flags |= int(rng.choice([0, 0, ONLY_DX, ONLY_DW]))
    return Case(name, "bwd", i, o, B, int(rng.choice(ACTS_BWD)), flags, seed=seed, ldx=i + pad(), x_off=off(), ldy=o + pad(), y_off=off(), lddy=o + pad(),
                dy_off=off(), lddx=i + pad(), dx_off=off(), w_off=off(), db=bool(rng.random() < 0.75), dx=bool(rng.random() < 0.8),
                forked=bool(rng.random() < 0.4), scratch=bool(rng.random() < 0.8))


def draw_cases(seed, count=6):
    rng = np.random.default_rng(1000 + seed)
    return [draw_case(rng, f"seed{seed}.{k}") for k in range(count)]
