"""Generator, float64 reference and checker for ffh_mlp_chain_fwd / ffh_mlp_chain_bwd (include/ff_hip.h).

Used by tests/test_chain_sweep_cpu.py (the oracle library, on a CPU: proves the harness) and tests/test_gpu_chain_sweep.py (the HIP kernels of
csrc/mlp_chain.hip).  Nothing here calls the oracle library: the reference is plain numpy in float64, written from the contract in the header.

What is compared.  Every layer's result is held against the reference applied to the inputs THAT LAYER consumed, read back from the library under
test as float32 and widened -- so every bound is the bound of one GEMM and nothing compounds over eight layers:

  forward    y_l            vs  act(y_(l-1) @ w_l.T + b_l)          y_(-1) = x, y_(l-1) as the library wrote it
  backward   top dy         vs  dy * act'(y)                          (premasked: unchanged bit for bit)
             dy_(l-1)       vs  (dy_l @ w_l) [y_(l-1) > 0 if ReLU]    dy_l as the library left it
             dx             vs  [dx0 +] (dy_0 @ w_0) [x > 0]
             dw_l, db_l     vs  dy_l.T @ x_l, dy_l.sum(0)             the library's final dy_l

The bound is the project's own, |got - ref| <= 1e-5 * mass * L + 8 * eps32 * |ref|: mass = the sum of the absolute values of the terms (float64;
an accumulating dx includes |dx0|), L = the activation's Lipschitz constant, the second term covers the device expf / tanhf.  There is no absolute
floor: the top gradient and dx0 are of order one, and where mass == 0 the result has to be exactly 0.

Every buffer is allocated with its leading dimension (and offset) and pre-filled with a NaN sentinel; after the call every element outside
[rows][width] of every output has to hold the sentinel bit for bit.  The inputs' padding holds the same NaN, so a kernel that reads padding into
its arithmetic poisons a result and fails the bound.
"""
import numpy as np

from dlrm_flexflow_amd import capi

NONE, RELU, SIG, GELU = capi.AC_MODE_NONE, capi.AC_MODE_RELU, capi.AC_MODE_SIGMOID, capi.AC_MODE_GELU
LIPSCHITZ = {NONE: 1.0, RELU: 1.0, SIG: 0.25, GELU: 1.13}
EPS32 = float(np.finfo(np.float32).eps)
TOL = 1e-5
SENTINEL_BITS = 0x7FC0BEEF            # a quiet NaN with a payload no arithmetic produces
MAX_LAYERS, MAX_WIDTH = 8, 512        # FFH_CHAIN_MAX_LAYERS, FFH_CHAIN_MAX_WIDTH
HOST_STAND_IN_CUS = 8                 # the oracle reports no compute units: the "32 * num_cus + r" batches still want a size on a CPU
TAIL = 3                              # sentinel floats behind the last row of every buffer


# ---------------------------------------------------------------------------------------------------------------------------
# where the buffers live
class HostBackend:
    """Buffers of the oracle library: numpy arrays."""
    is_hip = False

    def upload(self, flat):
        return flat.copy()

    def download(self, h):
        return h.copy()

    def addr(self, h):
        return h.ctypes.data

    def sync(self):
        pass


class TorchBackend:
    """Buffers of the HIP library: torch tensors on cuda:0 (the allocator's blocks are 256-byte aligned)."""
    is_hip = True

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device = torch, device

    def upload(self, flat):
        t = self.torch.from_numpy(flat).to(self.device)
        assert t.data_ptr() % 16 == 0
        return t

    def download(self, h):
        return h.cpu().numpy()

    def addr(self, h):
        return h.data_ptr()

    def sync(self):
        self.torch.cuda.synchronize()


def num_cus(lib):
    return int(lib.device_info().compute_units) or HOST_STAND_IN_CUS


class Buf:
    """[rows][cols] floats with leading dimension ld, `off` floats into an aligned allocation; everything else is the sentinel."""

    def __init__(self, be, rows, cols, ld, off=0, data=None):
        self.be, self.rows, self.cols, self.ld, self.off = be, int(rows), int(cols), int(ld), int(off)
        pitch = max(self.ld, self.cols)
        flat = np.full(self.off + self.rows * pitch + TAIL, 0, np.uint32)
        flat[:] = SENTINEL_BITS
        flat = flat.view(np.float32)
        self.valid = np.zeros(flat.size, bool)
        if self.rows:
            idx = (self.off + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]).ravel()
            self.valid[idx] = True
            self.idx = idx
            if data is not None:
                flat[idx] = np.asarray(data, np.float32).ravel()
        else:
            self.idx = np.zeros(0, np.int64)
        self.before = flat.copy()
        self.h = be.upload(flat)
        self.host = None

    @property
    def ptr(self):
        return self.be.addr(self.h) + 4 * self.off

    def fetch(self):
        self.host = self.be.download(self.h)
        return self

    def get(self):
        """The [rows][cols] block as the library left it (float32)."""
        return self.host[self.idx].reshape(self.rows, self.cols)

    def flat_index(self, r, c):
        return self.off + r * self.ld + c

    def padding_intact(self):
        return bool((self.host.view(np.uint32)[~self.valid] == SENTINEL_BITS).all())

    def untouched(self):
        return self.host.view(np.uint32).tobytes() == self.before.view(np.uint32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# a case
class Case:
    """One call.  kind "fwd" or "bwd"; per-layer lists may be None (dense, aligned, bias and db present)."""

    def __init__(self, name, kind, widths, acts, batch, seed=0, ldx=None, x_off=0, ldw=None, w_off=None, bias=None, ldy=None, y_off=None,
                 lddy=None, dy_off=None, db=None, want_dx=False, lddx=None, dx_off=0, overwrite=False, mask_by_x=False, premasked=False,
                 extra_flags=0):
        n = len(widths) - 1
        assert len(acts) == n and kind in ("fwd", "bwd")
        self.name, self.kind, self.widths, self.acts, self.batch, self.seed, self.n = name, kind, tuple(widths), tuple(acts), int(batch), seed, n
        self.ldx = widths[0] if ldx is None else ldx
        self.x_off = x_off
        self.ldw = list(ldw) if ldw is not None else list(widths[:-1])
        self.w_off = list(w_off) if w_off is not None else [0] * n
        self.bias = list(bias) if bias is not None else [True] * n
        self.ldy = list(ldy) if ldy is not None else list(widths[1:])
        self.y_off = list(y_off) if y_off is not None else [0] * n
        self.lddy = list(lddy) if lddy is not None else list(widths[1:])
        self.dy_off = list(dy_off) if dy_off is not None else [0] * n
        self.db = list(db) if db is not None else [True] * n
        self.want_dx, self.lddx, self.dx_off = want_dx, (widths[0] if lddx is None else lddx), dx_off
        self.overwrite, self.mask_by_x, self.premasked, self.extra_flags = overwrite, mask_by_x, premasked, extra_flags

    @property
    def flags(self):
        return ((capi.LINEAR_DX_OVERWRITE if self.overwrite else 0) | (capi.LINEAR_DX_MASK_BY_X if self.mask_by_x else 0)
                | (capi.LINEAR_DY_PREMASKED if self.premasked else 0) | self.extra_flags)

    def __repr__(self):
        return (f"Case({self.name}: {self.kind} {'-'.join(map(str, self.widths))} acts={self.acts} B={self.batch} ldx={self.ldx}+{self.x_off} "
                f"ldw={self.ldw}+{self.w_off} bias={self.bias} ldy={self.ldy}+{self.y_off} lddy={self.lddy}+{self.dy_off} db={self.db} "
                f"dx={self.want_dx} lddx={self.lddx}+{self.dx_off} flags={self.flags})")


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference
def act64(v, act):
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == SIG:
        return 1.0 / (1.0 + np.exp(-v))
    if act == GELU:        # the tanh form (tests/test_oracle_golden.py::test_linear_gelu_forward_matches_torch_tanh_form)
        return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))
    return v


def _f64(a):
    return np.asarray(a, np.float64)


def make_inputs(case):
    """Operands of order one, the same for a given case on every backend."""
    rng = np.random.default_rng([case.seed, len(case.widths), case.batch] + list(case.widths))
    B, wd = case.batch, case.widths
    inp = {}
    inp["w"] = [(rng.uniform(-1, 1, (o, i)) * np.sqrt(3.0 / i)).astype(np.float32) for i, o in zip(wd[:-1], wd[1:])]
    inp["b"] = [rng.uniform(-0.5, 0.5, o).astype(np.float32) for o in wd[1:]]
    x = rng.uniform(-1, 1, (B, wd[0]))
    if case.kind == "bwd" and case.mask_by_x:
        x = np.maximum(x, 0)          # the output of a ReLU
    inp["x"] = x.astype(np.float32)
    if case.kind == "bwd":
        ys, cur = [], _f64(inp["x"])
        for l in range(case.n):       # the float64 forward rounded to float32: the masks are decided on values both sides share
            z = cur @ _f64(inp["w"][l]).T + (_f64(inp["b"][l]) if case.bias[l] else 0.0)
            ys.append(act64(z, case.acts[l]).astype(np.float32))
            cur = _f64(ys[-1])
        inp["y"] = ys
        g = rng.uniform(-1, 1, (B, wd[-1]))
        if case.premasked and case.acts[-1] == RELU:
            g = np.where(ys[-1] > 0, g, 0.0)
        inp["g"] = g.astype(np.float32)
        inp["dx0"] = rng.uniform(-1, 1, (B, wd[0])).astype(np.float32)
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# the calls
class Result:
    def __init__(self, case, inp, rc, route, **bufs):
        self.case, self.inp, self.rc, self.route = case, inp, rc, route
        self.__dict__.update(bufs)


def _layers(lib, case, W, Bi, Y, DY=None, DW=None, DB=None):
    ent = []
    for l in range(case.n):
        ent.append(dict(w=W[l].ptr, bias=Bi[l].ptr if Bi and Bi[l] is not None else None, y=Y[l].ptr, ldy=case.ldy[l], ldw=case.ldw[l],
                        dy=DY[l].ptr if DY else None, lddy=case.lddy[l], dw=DW[l].ptr if DW else None,
                        db=DB[l].ptr if DB and DB[l] is not None else None,
                        in_dim=case.widths[l], out_dim=case.widths[l + 1], activation=case.acts[l]))
    return lib.chain_layers(ent)


def run_fwd(lib, be, case, inp=None):
    inp = inp or make_inputs(case)
    B, wd, n = case.batch, case.widths, case.n
    X = Buf(be, B, wd[0], case.ldx, case.x_off, inp["x"])
    W = [Buf(be, wd[l + 1], wd[l], case.ldw[l], case.w_off[l], inp["w"][l]) for l in range(n)]
    Bi = [Buf(be, 1, wd[l + 1], wd[l + 1], 0, inp["b"][l]) if case.bias[l] else None for l in range(n)]
    Y = [Buf(be, B, wd[l + 1], case.ldy[l], case.y_off[l]) for l in range(n)]
    rc = lib.lib.ffh_mlp_chain_fwd(lib.ctx, X.ptr, case.ldx, _layers(lib, case, W, Bi, Y), n, B, None)
    route = lib.lib.ffh_linear_last_route(lib.ctx).decode()
    be.sync()
    for y in Y:
        y.fetch()
    return Result(case, inp, rc, route, Y=Y, outputs=[(f"y{l}", Y[l]) for l in range(n)])


def run_bwd(lib, be, case, inp=None, stream=None):
    inp = inp or make_inputs(case)
    B, wd, n = case.batch, case.widths, case.n
    X = Buf(be, B, wd[0], case.ldx, case.x_off, inp["x"])
    W = [Buf(be, wd[l + 1], wd[l], case.ldw[l], case.w_off[l], inp["w"][l]) for l in range(n)]
    Y = [Buf(be, B, wd[l + 1], case.ldy[l], case.y_off[l], inp["y"][l]) for l in range(n)]
    DY = [Buf(be, B, wd[l + 1], case.lddy[l], case.dy_off[l], inp["g"] if l == n - 1 else None) for l in range(n)]
    DW = [Buf(be, wd[l + 1], wd[l], case.ldw[l], 0, np.zeros((wd[l + 1], wd[l]), np.float32)) for l in range(n)]      # (the caller zeroes dw / db)
    DB = [Buf(be, 1, wd[l + 1], wd[l + 1], 0, np.zeros(wd[l + 1], np.float32)) if case.db[l] else None for l in range(n)]
    DX = Buf(be, B, wd[0], case.lddx, case.dx_off, inp["dx0"]) if case.want_dx else None
    rc = lib.lib.ffh_mlp_chain_bwd(lib.ctx, X.ptr, case.ldx, DX.ptr if DX else None, case.lddx, _layers(lib, case, W, None, Y, DY, DW, DB), n, B,
                                   case.flags, stream)
    route = lib.lib.ffh_linear_last_route(lib.ctx).decode()
    be.sync()
    outs = [(f"dy{l}", DY[l]) for l in range(n)] + [(f"dw{l}", DW[l]) for l in range(n)] + [(f"db{l}", DB[l]) for l in range(n) if DB[l] is not None]
    if DX:
        outs.append(("dx", DX))
    for _, b in outs:
        b.fetch()
    return Result(case, inp, rc, route, DY=DY, DW=DW, DB=DB, DX=DX, outputs=outs)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker
class Report:
    def __init__(self):
        self.violations, self.mass, self.worst = [], {}, {}

    def ok(self):
        return not self.violations

    def __str__(self):
        return "\n".join(self.violations)


WORST = {}       # output kind -> worst |got - ref| / bound seen in this process (printed by the tests: a measurement, not a check)


def _compare(rep, name, got, ref, mass, lip=1.0):
    got, ref, mass = _f64(got), _f64(ref), _f64(mass) + np.zeros_like(_f64(ref))
    rep.mass[name] = mass
    bound = TOL * mass * lip + 8 * EPS32 * np.abs(ref)
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
        rep.violations.append(f"{name}: {int(bad.sum())} of {bad.size} beyond {TOL} * mass * {lip} + 8 eps |ref|; worst at {i}: got {got[i]!r} ref {ref[i]!r} "
                              f"mass {mass[i]:.3e} bound {bound[i]:.3e}")


def _padding(rep, res):
    for name, buf in res.outputs:
        if not buf.padding_intact():
            bad = np.flatnonzero((buf.host.view(np.uint32) != SENTINEL_BITS) & ~buf.valid)
            rep.violations.append(f"{name}: {bad.size} padding element(s) overwritten, first at flat index {int(bad[0])} (ld {buf.ld}, offset {buf.off})")


def check_fwd(res):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    cur = _f64(inp["x"])
    for l in range(case.n):
        w = _f64(inp["w"][l])
        b = _f64(inp["b"][l]) if case.bias[l] else np.zeros(case.widths[l + 1])
        ref = act64(cur @ w.T + b, case.acts[l])
        mass = np.abs(cur) @ np.abs(w).T + np.abs(b)
        got = res.Y[l].get()
        _compare(rep, f"y{l}", got, ref, mass, LIPSCHITZ[case.acts[l]])
        cur = _f64(got)               # what the next layer consumed
    _padding(rep, res)
    return rep


def check_bwd(res):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    n = case.n
    x, ys = _f64(inp["x"]), [_f64(y) for y in inp["y"]]
    g, top = _f64(inp["g"]), res.DY[n - 1].get()
    act = case.acts[n - 1]
    if case.premasked or act == NONE:
        if top.tobytes() != inp["g"].tobytes():
            rep.violations.append(f"dy{n - 1}: a final top gradient was modified")
        rep.mass[f"dy{n - 1}"] = np.abs(g)
    elif act == RELU:
        _compare(rep, f"dy{n - 1}", top, np.where(ys[-1] > 0, g, 0.0), np.where(ys[-1] > 0, np.abs(g), 0.0))
    else:
        _compare(rep, f"dy{n - 1}", top, g * ys[-1] * (1.0 - ys[-1]), np.abs(g), LIPSCHITZ[SIG])
    for l in range(n - 1, -1, -1):
        dy = _f64(res.DY[l].get())                     # the library's final dy_l
        w = _f64(inp["w"][l])
        xin = x if l == 0 else ys[l - 1]
        _compare(rep, f"dw{l}", res.DW[l].get(), dy.T @ xin, np.abs(dy).T @ np.abs(xin))
        if res.DB[l] is not None:
            _compare(rep, f"db{l}", res.DB[l].get()[0], dy.sum(0), np.abs(dy).sum(0))
        ref, mass = dy @ w, np.abs(dy) @ np.abs(w)
        if l > 0:
            if case.acts[l - 1] == RELU:
                keep = ys[l - 1] > 0
                ref, mass = np.where(keep, ref, 0.0), np.where(keep, mass, 0.0)
            _compare(rep, f"dy{l - 1}", res.DY[l - 1].get(), ref, mass)
        elif res.DX is not None:
            if case.mask_by_x:
                keep = x > 0
                ref, mass = np.where(keep, ref, 0.0), np.where(keep, mass, 0.0)
            if not case.overwrite:
                ref, mass = ref + _f64(inp["dx0"]), mass + np.abs(_f64(inp["dx0"]))
            _compare(rep, "dx", res.DX.get(), ref, mass)
    _padding(rep, res)
    return rep


# ---------------------------------------------------------------------------------------------------------------------------
# the route the HIP library has to report (csrc/mlp_chain.hip: 32-row blocks from 32 * num_cus samples on, where two blocks fit the LDS)
def _stride(w):
    return ((w + 15) & ~15) + 8


LDS_MAX, STAGE_FLOATS = 150 * 1024, 8 * 16 * 72


def rows_fwd(widths, batch, cus):
    w = [0, 0]
    for p, width in enumerate(widths):
        w[p & 1] = max(w[p & 1], _stride(width))
    return 32 if batch >= 32 * cus and (32 * (w[0] + w[1]) + STAGE_FLOATS) * 4 <= LDS_MAX else 16


def rows_bwd(widths, batch, cus):
    w = [0, 0]
    for j, width in enumerate(reversed(widths[1:])):
        w[j & 1] = max(w[j & 1], _stride(width))
    return 32 if batch >= 32 * cus and 32 * (w[0] + w[1]) * 4 <= LDS_MAX else 16


def check_route(res, cus, ordered=False):
    case, toks, out = res.case, res.route.split(";"), []
    if case.kind == "fwd":
        want = f"mlp_chain_fwd|layers={case.n}|rows={rows_fwd(case.widths, case.batch, cus)}"
        if toks != [want]:
            out.append(f"route {res.route!r}, expected {want!r}")
        return out
    top_live = not case.premasked and case.acts[-1] != NONE
    dx_launch = case.n > 1 or case.want_dx or top_live
    want = f"mlp_chain_dx|layers={case.n}|rows={rows_bwd(case.widths, case.batch, cus)}"
    if dx_launch != (want in toks) or dx_launch != any(t.startswith("mlp_chain_dx") for t in toks):
        out.append(f"route {res.route!r}: data-gradient token {want!r} {'missing' if dx_launch else 'present without a launch'}")
    items = sum(((o + 63) // 64) * ((i + 63) // 64) for i, o in zip(case.widths[:-1], case.widths[1:]))
    dw = [t for t in toks if t.startswith(f"mlp_chain_dw|blocks={items}|splits=")]
    if len(dw) != 1 or dw[0].endswith("|ordered") != ordered:
        out.append(f"route {res.route!r}: expected one mlp_chain_dw|blocks={items}|splits=S{'|ordered' if ordered else ''}")
    return out


def run_and_check(lib, be, case, cus=None, stream=None, ordered=False):
    """Run one case, return (result, report); the route is part of the report on the HIP library."""
    res = run_fwd(lib, be, case) if case.kind == "fwd" else run_bwd(lib, be, case, stream=stream)
    rep = check_fwd(res) if case.kind == "fwd" else check_bwd(res)
    if be.is_hip and res.rc == capi.FFH_OK and case.batch > 0:
        rep.violations += check_route(res, cus, ordered)
    return res, rep


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed edge table
def _up4(w):
    return (w + 3) & ~3


def _bwd_widths(widths):
    """The backward contract: every inner width and the top width a multiple of 4 (the input's only where dx is wanted)."""
    return (widths[0],) + tuple(_up4(w) for w in widths[1:])


def _pair(name, widths, acts, batch, fwd_kw=None, **bwd_kw):
    """The forward of a row of the table, and its backward on the widths the backward serves."""
    fwd_kw = dict(fwd_kw or {})
    shared = {k: bwd_kw[k] for k in ("ldx", "ldw", "ldy", "bias") if k in bwd_kw}
    shared.update(fwd_kw)
    bw = _bwd_widths(widths)
    return [Case(name + "/fwd", "fwd", widths, acts, batch, **shared), Case(name + "/bwd", "bwd", bw, acts, batch, **bwd_kw)]


def edge_table(cus):
    """name -> list of cases (forward, then backward where the backward contract serves the row)."""
    t = {}
    t["one-layer-dx-discarded-premasked"] = _pair("one-layer-premasked", (64, 32), (RELU,), 77, premasked=True)
    t["one-layer-live-sigmoid-dx-wanted"] = _pair("one-layer-sigmoid", (64, 32), (SIG,), 77, want_dx=True, overwrite=True)
    t["eight-layers"] = _pair("eight-layers", (40, 72, 136, 264, 392, 20, 12, 4, 8), (RELU, NONE, RELU, RELU, RELU, NONE, RELU, RELU), 100,
                              want_dx=True, overwrite=True, mask_by_x=True)
    t["stale-lds"] = _pair("stale-lds", (64, 500, 20, 300, 12, 260), (RELU, RELU, NONE, RELU, SIG), 50, want_dx=True)
    acts7 = (RELU, NONE, RELU, RELU, NONE, RELU, RELU)
    t["tile-boundaries"] = [Case("tile-boundaries/fwd", "fwd", (16, 128, 129, 256, 257, 384, 385, 512), acts7, 33),
                            Case("tile-boundaries/bwd", "bwd", (16, 128, 132, 256, 260, 384, 388, 512), acts7, 33, want_dx=True, overwrite=True)]
    t["forward-only-ragged"] = [Case("ragged/fwd", "fwd", (13, 7, 1, 3, 17, 65), (RELU, NONE, GELU, RELU, SIG), 19, bias=[True, False, True, True, True])]
    t["rows32-ragged-tail"] = _pair("rows32-tail", (13, 64, 16), (RELU, RELU), 32 * cus + 5)
    t["lds-fallback"] = _pair("lds-fallback", (512, 512, 512), (RELU, NONE), 32 * cus + 5, want_dx=True, overwrite=True)
    for B in (1, 15, 16, 17, 31, 63, 64, 65):
        t[f"tiny-batch-{B}"] = _pair(f"tiny-batch-{B}", (32, 48, 16), (RELU, RELU), B, want_dx=True)
    t["activations-gelu-sigmoid-gelu"] = [Case("activations-a/fwd", "fwd", (24, 40, 56, 8), (GELU, SIG, GELU), 130)]
    t["activations-none-gelu-sigmoid"] = [Case("activations-b/fwd", "fwd", (24, 40, 56, 8), (NONE, GELU, SIG), 130)]
    t["strides"] = _pair("strides", (32, 64, 16), (RELU, RELU), 200, ldx=44, ldw=[36, 68], ldy=[72, 24], lddy=[68, 20], lddx=36, want_dx=True,
                         mask_by_x=True)
    t["misaligned-forward"] = [Case("misaligned/fwd", "fwd", (32, 64, 16), (RELU, NONE), 70, x_off=1, ldx=33, y_off=[0, 1], ldy=[65, 17])]
    # (the row reads "32-64-16 with bias = NULL on layers 0 and 2, db = NULL on layer 1": three layers are meant, so a third, 8 wide, follows;
    #  the two-layer chain as written runs beside it)
    t["nulls"] = _pair("nulls", (32, 64, 16, 8), (RELU, RELU, NONE), 90, bias=[False, True, False], db=[True, False, True], want_dx=True)
    t["nulls-two-layers"] = _pair("nulls-two", (32, 64, 16), (RELU, NONE), 90, bias=[False, True], db=[True, False], want_dx=True)
    for ow in (True, False):
        for mk in (True, False):
            for top, (act, pm) in {"premasked": (RELU, True), "live-relu": (RELU, False), "live-sigmoid": (SIG, False), "none": (NONE, False)}.items():
                name = f"dx-{'overwrite' if ow else 'accumulate'}-{'maskx' if mk else 'nomask'}-{top}"
                t[name] = _pair(name, (32, 64, 16), (RELU, act), 45, want_dx=True, overwrite=ow, mask_by_x=mk, premasked=pm)
    return t


EDGE_NAMES = list(edge_table(1))


# ---------------------------------------------------------------------------------------------------------------------------
# the random generator
def _draw_width(rng, mult4=False):
    m = int(rng.integers(5))
    if m == 0:
        w = int(rng.integers(1, 17))
    elif m == 1:
        w = 4 * int(rng.integers(1, 129))
    elif m == 2:
        w = 16 * int(rng.integers(1, 33)) + int(rng.choice([-1, 1]))
    elif m == 3:
        w = 64 * int(rng.integers(1, 9)) + int(rng.choice([-4, -1, 0, 1, 4]))
    else:
        w = int(rng.integers(1, MAX_WIDTH + 1))
    w = min(max(w, 1), MAX_WIDTH)
    return _up4(w) if mult4 else w


def _draw_batch(rng):
    m = int(rng.integers(4))
    if m == 0:
        return int(rng.integers(1, 71))
    if m == 1:
        return 16 * int(rng.integers(1, 64)) + int(rng.choice([-1, 1]))
    if m == 2:
        return 32 * int(rng.integers(1, 64)) + int(rng.choice([-1, 1]))
    return int(rng.integers(1, 3001))


def draw_case(rng, kind=None, batch=None, max_width=MAX_WIDTH, name="random"):
    """One random case; backward cases are drawn inside the served contract, forward cases use any width and alignment."""
    kind = kind or ("fwd" if rng.random() < 0.5 else "bwd")
    n = int(rng.integers(1, MAX_LAYERS + 1))
    B = batch if batch is not None else _draw_batch(rng)
    pad = lambda q: int(rng.choice([0, 0, 1, 2, 3, 5, 8])) * q
    if kind == "fwd":
        widths = [min(_draw_width(rng), max_width) for _ in range(n + 1)]
        acts = [int(rng.choice([NONE, RELU, SIG, GELU])) for _ in range(n)]
        return Case(name, "fwd", widths, acts, B, seed=int(rng.integers(1 << 30)), ldx=widths[0] + pad(1), x_off=int(rng.integers(4)),
                    ldw=[w + pad(1) for w in widths[:-1]], w_off=[int(rng.integers(4)) for _ in range(n)], bias=[bool(rng.random() < 0.75) for _ in range(n)],
                    ldy=[w + pad(1) for w in widths[1:]], y_off=[int(rng.integers(4)) for _ in range(n)])
    want_dx = bool(rng.random() < 0.6)
    mask = want_dx and bool(rng.random() < 0.5)
    widths = [min(_draw_width(rng, mult4=want_dx), max_width)] + [min(_draw_width(rng, mult4=True), max_width) for _ in range(n)]
    acts = [int(rng.choice([NONE, RELU])) for _ in range(n - 1)] + [int(rng.choice([NONE, RELU, SIG]))]
    loose = not want_dx                       # layer 0 produces no data gradient: its w and x rows need no alignment
    ldw = [widths[0] + (pad(1) if loose else pad(4))] + [w + pad(4) for w in widths[1:-1]]
    w_off = [int(rng.integers(4)) if loose else 0] + [0] * (n - 1)
    return Case(name, "bwd", widths, acts, B, seed=int(rng.integers(1 << 30)),
                ldx=widths[0] + (pad(4) if mask or widths[0] % 4 == 0 and rng.random() < 0.5 else pad(1)), x_off=0 if mask else int(rng.integers(4)),
                ldw=ldw, w_off=w_off, ldy=[w + pad(4) for w in widths[1:]], lddy=[w + pad(4) for w in widths[1:]],
                db=[bool(rng.random() < 0.75) for _ in range(n)], want_dx=want_dx, lddx=widths[0] + pad(4), overwrite=bool(rng.random() < 0.5),
                mask_by_x=mask, premasked=bool(rng.random() < 0.4))


def draw_cases(seed, cus, count=6):
    """The cases of one seed: the first at 32 * num_cus + r rows with widths <= 128, the others free."""
    rng = np.random.default_rng(seed)
    out = [draw_case(rng, batch=32 * cus + int(rng.integers(0, 32)), max_width=128, name=f"seed{seed}.0")]
    for i in range(1, count):
        out.append(draw_case(rng, name=f"seed{seed}.{i}"))
    return out
