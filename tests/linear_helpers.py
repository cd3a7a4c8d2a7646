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

Tensor-op mode (Case.mode = 1, FFH_MATH_TENSOR_OP_BF16; tests/test_linear_bf16_sweep_cpu.py, tests/test_gpu_linear_bf16_sweep.py).  A layer with
in_dim >= 128 and out_dim >= 128 has both operands of each GEMM rounded to bfloat16, nearest even (rne_bf16: numpy on the bits, written from
include/ff_hip.h, not from the oracle or a kernel), widened to float64 and summed there: y vs act(rne(x) @ rne(w).T + b), dw vs dw0 + rne(dy').T @
rne(x), dx vs [dx0 +] (rne(dy') @ rne(w)) [x > 0]; db, the bias, the activations and the dy transform stay fp32 quantities of unrounded values;
the mass is taken on the rounded operands; the bound is the same one (the header: "against a twin that rounds the same operands the fp32
summation-order bound of the fp32 mode applies").  A narrower layer keeps the fp32 reference.  Case.twins names the buffers among x w y dy dx
that get a registered bfloat16 twin (TwinBuf: same layout at 2 bytes per element, SENTINEL16 in padding, offset and tail; an input's twin filled
by ffh_convert_f32_to_bf16, as a model's producers would): an output's twin is untouched as a whole or, over the whole block and nowhere else,
the nearest-even rounding of the floats the library stored -- written it must be where the route names the bf16 pipe; an input's twin is
bit-identical after the call (Case.stale: dy's twin holds NaN and must not be read).  run_fwd / run_bwd set the mode and register the twins, and
undo both in a finally.  Case.dist: "uniform", "integer" (exact), "ties" (every GEMM operand a bfloat16 plus half an ulp), "wide" (+-20 binades).

Routes.  route_fwd / route_bwd restate the dispatch predicates of the HIP library (sk_plan, plan_glds, the launch_gemm tile choice, the skinny
and thin conditions) as a function of the CU count; the GPU test asserts ffh_linear_last_route against them, and every edge case names the
kernel family it is there for (Case.want), which the CPU test asserts of the model at 256 CUs.  In tensor-op mode bf16_gemm restates
launch_gemm_bf16 (csrc/linear_bf16.hip: the tile, the split count, the twins' conditions) and launch_gemm_bf16_dma's serve conditions
(csrc/linear_bf16_dma.hip); the split count is part of the expected token except for the LDS-DMA weight gradient, whose cost search is only held
to its range.

Split mode (Case.mode = 3, FFH_MATH_FP32_SPLIT_BF16X3_ALL; tests/test_linear_x3_sweep_cpu.py, tests/test_gpu_linear_x3_sweep.py).  A layer with both
widths >= 128 computes each product as the six bfloat16 plane products a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1 of x1 = bf16(x), x2 = bf16(x - x1),
x3 = bf16(x - x1 - x2) (split3 / split_product: numpy, written from include/ff_hip.h).  On the distributions above the mode is held to the project's
bound against the float64 product of the UNSPLIT operands, which cannot tell six products from four; Case.dist = "planes" is the family on which
it can: every non-zero GEMM operand is s * (2^18 + t * 2^9 + r), s, t in {-1, +1}, r in {0, 1}, whose planes are exactly s 2^18, s t 2^9 and s r,
so the six kept products are multiples of 2^18 and the three dropped ones are not zero; zeros are placed so that no output of any GEMM of the
call has more than PLANES_MAX_TERMS = 48 reduction positions with both operands non-zero (asserted by the generator with a boolean product of
the masks), spread over the whole reduction range.  Every partial sum in any order is then a multiple of 2^18 below 2^42, exact in fp32: y, dx
and dw have to EQUAL the float64 sum of the six kept products, whatever the tile, split-K or atomics (db sums unsplit values and keeps the
bound).  (t = -1 puts x on or just above a rounding tie of the first plane and x - x1 on one of the second: with t = +1 alone every remainder
lies below half an ulp and a truncating split gives the same planes as nearest-even.)  Case.images names the buffers among x w y dy dx with a
registered three-plane image (ImageBuf / Images: the region is the Buf's whole allocation, 128-byte aligned; the image holds SENTINEL16
everywhere, an input's is filled by ffh_convert_f32_to_bf16x3 and compared with the numpy restatement before the call): after the call an input's
image is bit-identical, an output's is untouched as a whole or exactly the image of the stored floats over the block and the sentinel elsewhere,
and written it must be where the route names "bf16x3" or "x3_dma" for that GEMM.  x3_gemm restates the split branch of launch_gemm_bf16
(csrc/linear_bf16.hip) and the serve conditions of launch_gemm_x3_dma (csrc/linear_x3_dma.hip).  NumpySplitLib is the same entry points in numpy
with the arithmetic as a parameter: what the CPU test feeds the checker, right and wrong.
"""
import ctypes as C
import re

import numpy as np

from dlrm_flexflow_amd import capi
from chain_helpers import Buf, HostBackend, TorchBackend, act64, LIPSCHITZ, num_cus, SENTINEL_BITS, EPS32, TOL, TAIL  # noqa: F401

NONE, RELU, SIG, GELU = capi.AC_MODE_NONE, capi.AC_MODE_RELU, capi.AC_MODE_SIGMOID, capi.AC_MODE_GELU
OVERWRITE, ONLY_DW, ONLY_DX, PREMASKED, MASK_BY_X = (capi.LINEAR_DX_OVERWRITE, capi.LINEAR_ONLY_DW, capi.LINEAR_ONLY_DX, capi.LINEAR_DY_PREMASKED,
                                                     capi.LINEAR_DX_MASK_BY_X)
MATH_BF16 = 1               # FFH_MATH_TENSOR_OP_BF16
MATH_SPLIT_ALL = 3          # FFH_MATH_FP32_SPLIT_BF16X3_ALL
BF16_MIN_DIM = 128          # FFH_BF16_MIN_DIM
DISTS = ("uniform", "integer", "ties", "wide")
ALL_DISTS = DISTS + ("planes",)          # "planes": the split mode's own family
TWIN_NAMES = ("x", "w", "y", "dy", "dx")
IMAGE_NAMES = TWIN_NAMES
PLANES_MAX_TERMS = 48       # "planes": reduction positions with both operands non-zero, per output element: 48 * (2^18 + 2^9 + 1)^2 < 2^42
PLANE_UNIT = 2.0 ** 18
SENTINEL16 = 0x7FDE         # a bfloat16 NaN: a twin's padding read into a GEMM poisons the result
TABLE_CUS = 256             # the CU count the edge table's shapes were derived for (MI355X)


def _f64(a):
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# a case
class Case:
    """One ffh_linear_fwd (kind "fwd") or ffh_linear_bwd_ex (kind "bwd") call."""

    def __init__(self, name, kind, in_dim, out_dim, batch, act=NONE, flags=0, seed=0, ldx=None, x_off=0, ldy=None, y_off=0, lddy=None, dy_off=0,
                 lddx=None, dx_off=0, w_off=0, bias=True, bias_off=0, db=True, dx=True, forked=False, det=False, cmap=False, cmap_ncols=None,
                 colsum=False, colsum_ncols=None, scratch=True, integer=False, want=(), mode=0, twins=(), dist=None, stale=(), images=()):
        assert kind in ("fwd", "bwd")
        self._kw = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        dist = dist or ("integer" if integer else "uniform")
        assert dist in ALL_DISTS and mode in (0, MATH_BF16, MATH_SPLIT_ALL) and set(twins) <= set(TWIN_NAMES) and set(images) <= set(IMAGE_NAMES)
        assert set(stale) <= set(twins) | set(images) and not (twins and images)
        assert dist != "planes" or act in (NONE, RELU)
        integer = dist == "integer"
        self.mode, self.twins, self.dist, self.stale, self.images = mode, frozenset(twins), dist, frozenset(stale), frozenset(images)
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

    def replace(self, **kw):
        """The same case with some constructor arguments changed."""
        return Case(**{**self._kw, **kw})

    @property
    def bf16_layer(self):
        """The layer rule of FFH_MATH_TENSOR_OP_BF16 (include/ff_hip.h): both widths >= FFH_BF16_MIN_DIM."""
        return self.mode == MATH_BF16 and self.in_dim >= BF16_MIN_DIM and self.out_dim >= BF16_MIN_DIM

    @property
    def x3_layer(self):
        """The layer rule of FFH_MATH_FP32_SPLIT_BF16X3_ALL (include/ff_hip.h): both widths >= FFH_BF16_MIN_DIM, whatever the size."""
        return self.mode == MATH_SPLIT_ALL and self.in_dim >= BF16_MIN_DIM and self.out_dim >= BF16_MIN_DIM

    @property
    def planes_exact(self):
        """y, dx and dw have to equal the six-product sum: the "planes" family on a layer the split kernels take."""
        return self.dist == "planes" and self.x3_layer

    def __repr__(self):
        return (f"Case({self.name}: {self.kind} B={self.batch} {self.in_dim}->{self.out_dim} act={self.act} flags={self.flags} ldx={self.ldx}+{self.x_off} "
                f"ldy={self.ldy}+{self.y_off} lddy={self.lddy}+{self.dy_off} lddx={self.lddx}+{self.dx_off} w+{self.w_off} bias={self.bias}+{self.bias_off} "
                f"db={self.db} dx={self.dx} forked={self.forked} det={self.det} cmap={self.cmap}/{self.cmap_ncols} colsum={self.colsum}/{self.colsum_ncols} "
                f"scratch={self.scratch} dist={self.dist} mode={self.mode} twins={sorted(self.twins)} images={sorted(self.images)} stale={sorted(self.stale)})")


def make_inputs(case):
    """Operands of order one (or small integers), the same for a given case on every backend."""
    rng = np.random.default_rng([case.seed, case.in_dim, case.out_dim, case.batch, case.flags])
    B, i, o = case.batch, case.in_dim, case.out_dim
    if case.dist == "planes":
        return _make_planes(case, rng)
    if case.integer:
        assert case.act in (NONE, RELU)
        draw = lambda *shape: rng.integers(-2, 3, shape).astype(np.float64)
        w = draw(o, i)
    elif case.dist == "ties":
        # a bfloat16 value plus exactly half a bfloat16 ulp (low 16 bits 0x8000), random sign, exponent of order one: nearest-even, half-up
        # and truncation give three different roundings (even / odd kept mantissas come equally often)
        def draw(*shape, e0=126):
            bits = (rng.integers(0, 2, shape).astype(np.uint32) << 31) | (rng.integers(e0 - 2, e0 + 1, shape).astype(np.uint32) << 23) \
                | (rng.integers(0, 128, shape).astype(np.uint32) << 16) | np.uint32(0x8000)
            return bits.view(np.float32).astype(np.float64)
        w = draw(o, i, e0=126 - int(np.log2(i)) // 2)
    elif case.dist == "wide":
        assert case.act in (NONE, RELU)
        draw = lambda *shape: rng.uniform(-1, 1, shape) * 2.0 ** rng.integers(-20, 21, shape)       # a rounding that carries into the exponent occurs
        w = draw(o, i) * np.sqrt(3.0 / i)
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


def _band(rng, rows, cols, n):
    """bool [rows][cols]: n non-zeros in every row, one in each of n equal stretches of the columns, the pattern moved on from row to row by a
    step that takes the rows through a whole stretch (so every part of the range is used) and has no factor in common with cols: no column
    holds more than n * ceil(rows / cols)."""
    n = max(1, min(int(n), cols))
    edges = (np.arange(n + 1) * cols) // n
    pos = edges[:-1] + rng.integers(0, edges[1:] - edges[:-1])
    step = max(1, _cdiv(_cdiv(cols, n), rows))
    while np.gcd(step, cols) != 1:
        step += 1
    m = np.zeros((rows, cols), bool)
    m[np.arange(rows)[:, None], (pos[None, :] + step * np.arange(rows)[:, None]) % cols] = True
    return m


def _plane_values(rng, shape):
    """s * (2^18 + t * 2^9 + r): the planes are s 2^18, s t 2^9, s r exactly (t = -1: x1 by a tie to even or just above it, x2 = bf16(-511) a tie)."""
    s, t = (np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0) for _ in range(2))
    return s * (PLANE_UNIT + t * 2.0 ** 9 + rng.integers(0, 2, shape))


def planes_terms(case, inp):
    """GEMM name -> [M][N] count of the reduction positions at which both operands are non-zero, for every GEMM the call runs (a boolean product
    of the non-zero masks; dy counted before any mask: an upper bound)."""
    nz = lambda a: (np.asarray(a) != 0).astype(np.float32)
    if case.kind == "fwd":
        return {"fwd": nz(inp["x"]) @ nz(inp["w"]).T}
    out = {}
    if not case.has(ONLY_DX):
        out["dw"] = nz(inp["g"]).T @ nz(inp["x"])
    if case.dx and not case.has(ONLY_DW):
        out["dx"] = nz(inp["g"]) @ nz(inp["w"])
    return out


def _make_planes(case, rng):
    """The "planes" family (module docstring).  Forward: 48 non-zeros in every row of w, x dense.  Backward: x and w dense; with a weight gradient
    every column of dy has 48 non-zero rows spread over the batch (fewer where out_dim > batch, so that a row of dy keeps to 48 as well), with the
    data gradient alone every row of dy has 48 non-zeros spread over out_dim."""
    B, i, o = case.batch, case.in_dim, case.out_dim
    T = PLANES_MAX_TERMS
    small = lambda *shape: rng.integers(-2, 3, shape) * PLANE_UNIT
    w, x = _plane_values(rng, (o, i)), _plane_values(rng, (B, i))
    if case.kind == "fwd":
        w = np.where(_band(rng, o, i, T), w, 0.0)
    elif case.has(MASK_BY_X):
        x = np.maximum(x, 0)          # the output of a ReLU
    inp = {"w": w.astype(np.float32), "b": small(o).astype(np.float32), "x": x.astype(np.float32)}
    if case.kind == "bwd":
        y = act64(_f64(inp["x"]) @ _f64(inp["w"]).T + _f64(inp["b"]), case.act).astype(np.float32)
        g = _plane_values(rng, (B, o))
        if B:
            if not case.has(ONLY_DX):
                keep = _band(rng, o, B, T // _cdiv(o, B)).T
                if case.dx and not case.has(ONLY_DW) and keep.sum(1).max() > T:
                    keep &= _band(rng, B, o, T)
            else:
                keep = _band(rng, B, o, T)
            g = np.where(keep, g, 0.0)
        if case.has(PREMASKED) and case.act == RELU:
            g = np.where(y > 0, g, 0.0)
        inp.update(y=y, g=g.astype(np.float32), dx0=small(B, i).astype(np.float32), dw0=small(o, i).astype(np.float32), db0=small(o).astype(np.float32),
                   cs0=small(case.colsum_ncols).astype(np.float32))
    for name, terms in planes_terms(case, inp).items():          # a condition on the inputs, not a tolerance
        assert terms.size == 0 or terms.max() <= T, f"{case.name}: {name} has an output with {int(terms.max())} > {T} non-zero terms"
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
# bfloat16: the rounding of FFH_MATH_TENSOR_OP_BF16 (include/ff_hip.h: "round both operands to bfloat16 (nearest-even)") and the twins
def rne_bf16_bits(a):
    """float32 -> the 16 bits of the nearest bfloat16, ties to even, on the bits.  NaN stays NaN (quiet), what lies beyond the largest
    bfloat16 becomes +-inf (the carry runs into the exponent), denormals and the sign of zero are kept."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r.astype(np.uint32)).astype(np.uint16).reshape(np.shape(a))


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rne_bf16(a):
    """float32 -> bfloat16 (nearest even) -> float32."""
    return bf16_to_f32(rne_bf16_bits(a))


def trunc_bf16(a):
    """A WRONG rounding (the low 16 bits dropped): what the checker has to tell from rne_bf16."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(a))


def half_away_bf16(a):
    """A WRONG rounding (ties away from zero)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(np.shape(a))


# (float32 bits, bfloat16 bits) written by hand, and NaN patterns (quiet, signalling, payload in the low half only): what rne_bf16_bits and
# ffh_convert_f32_to_bf16 are pinned to
RNE_TABLE = [
    (0x3F800000, 0x3F80), (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81),
    (0x3F808000, 0x3F80),          # a tie, the kept mantissa even: down
    (0x3F818000, 0x3F82),          # a tie, the kept mantissa odd: up
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),
    (0x3FFF8000, 0x4000),          # a tie that carries into the exponent (1.99609375 + half an ulp -> 2.0)
    (0x3FFFFFFF, 0x4000), (0x007F8000, 0x0080),          # the largest denormals round up to the smallest normal
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80),          # the largest finite float: +-inf
    (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F),          # around the largest bfloat16
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    (0x00000001, 0x0000), (0x80000001, 0x8000),          # the smallest denormals: to zero, the sign kept
    (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002), (0x00010000, 0x0001),
    (0x00000000, 0x0000), (0x80000000, 0x8000)]
NAN_PATTERNS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FA00000, 0x7F80FFFF, 0xFF800001, 0x7FFFFFFF]


class TwinBuf:
    """The bfloat16 twin of a Buf (ffh_ctx_bf16_mirror_set): the same element layout at 2 bytes per element, so that the twin of the float at p is
    twin_base + (p - fp32_base) / 2, which is what the library computes from the registered region (the Buf's whole allocation).  Padding, offset
    and tail hold SENTINEL16; an input's twin is filled over the valid block by ffh_convert_f32_to_bf16 (fill()), an output's stays sentinel."""

    def __init__(self, be, buf):
        self.be, self.buf, self.valid, self.idx = be, buf, buf.valid, buf.idx
        flat = np.full(buf.valid.size, SENTINEL16, np.uint16)
        self.before = flat.copy()
        self.h = be.upload(flat.view(np.int16))
        self.host = None

    @property
    def base(self):
        return self.be.addr(self.h)

    def fill(self, lib):
        """What a model's producers leave in the twin of a buffer they wrote: the roundings of the valid block, row by row where it is strided."""
        b = self.buf
        runs = [(b.off, b.rows * b.cols)] if b.ld == b.cols or b.rows <= 1 else [(b.off + r * b.ld, b.cols) for r in range(b.rows)]
        for at, n in runs:
            if n:
                lib.check(lib.lib.ffh_convert_f32_to_bf16(lib.ctx, self.base + 2 * at, b.ptr + 4 * (at - b.off), n, None), "ffh_convert_f32_to_bf16")
        return self

    def poison(self, bits=0x7FC0):
        """A stale twin: the valid block replaced by bfloat16 NaN."""
        flat = self.be.download(self.h).view(np.uint16).copy()
        flat[self.idx] = bits
        self.h = None
        self.h = self.be.upload(flat.view(np.int16))
        return self

    def snapshot(self):
        self.before = self.be.download(self.h).view(np.uint16).copy()
        return self

    def fetch(self):
        self.host = self.be.download(self.h).view(np.uint16)
        return self

    def untouched(self):
        return self.host.tobytes() == self.before.tobytes()

    def problems(self, name, stored=None, must_write=False):
        """An output's twin after the call (stored: the [rows][cols] floats the library left in the fp32 buffer): untouched as a whole, or the
        nearest-even rounding of `stored` over the whole valid block and nothing else.  stored None: an input's twin, identical to before."""
        out = []
        if stored is None:
            if not self.untouched():
                out.append(f"{name} twin: an input's twin was modified ({int((self.host != self.before).sum())} elements)")
            return out
        if self.untouched():
            if must_write:
                out.append(f"{name} twin: not written by a launch on the bf16 pipe")
            return out
        pad = np.flatnonzero((self.host != SENTINEL16) & ~self.valid)
        if pad.size:
            out.append(f"{name} twin: {pad.size} padding element(s) overwritten, first at flat index {int(pad[0])} (ld {self.buf.ld}, offset {self.buf.off})")
        want = rne_bf16_bits(stored).ravel()
        got = self.host[self.idx]
        isnan = lambda v: (v & 0x7FFF) > 0x7F80
        bad = np.flatnonzero((got != want) & ~(isnan(got) & isnan(want)))
        if bad.size:
            r, c = divmod(int(bad[0]), self.buf.cols)
            out.append(f"{name} twin: {bad.size} of {got.size} elements are not the nearest-even rounding of the stored float; first at ({r}, {c}): "
                       f"0x{int(got[bad[0]]):04x}, expected 0x{int(want[bad[0]]):04x}")
        return out


class Twins:
    """The registrations of one call: made before it, undone whatever happens (the ctx is the whole session's)."""

    def __init__(self, lib, be, case, bufs, inputs):
        self.lib, self.t, self.inputs, self.regs = lib, {}, set(inputs), []
        try:
            for name in TWIN_NAMES:
                buf = bufs.get(name)
                if name not in case.twins or buf is None:
                    continue
                tw = self.t[name] = TwinBuf(be, buf)
                base = be.addr(buf.h)
                assert base % 16 == 0 and tw.base % 16 == 0, "ffh_ctx_bf16_mirror_set wants 16-byte aligned bases"
                lib.check(lib.lib.ffh_ctx_bf16_mirror_set(lib.ctx, base, 4 * buf.valid.size, tw.base), "ffh_ctx_bf16_mirror_set")
                self.regs.append(base)
                if name in self.inputs:
                    tw.fill(lib)
            be.sync()
            for name, tw in self.t.items():
                if name in case.stale:
                    old = tw.base
                    tw.poison()
                    assert tw.base % 16 == 0
                    if tw.base != old:
                        lib.check(lib.lib.ffh_ctx_bf16_mirror_set(lib.ctx, be.addr(tw.buf.h), 4 * tw.buf.valid.size, tw.base), "ffh_ctx_bf16_mirror_set")
                tw.snapshot()
        except BaseException:
            self.release()
            raise

    def release(self):
        for base in self.regs:
            self.lib.lib.ffh_ctx_bf16_mirror_set(self.lib.ctx, base, 4, None)
        self.regs = []


# ---------------------------------------------------------------------------------------------------------------------------
# the split of FFH_MATH_FP32_SPLIT_BF16X3 (include/ff_hip.h: x1 = bf16(x) nearest-even, x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), both
# differences exact in fp32; a * b = the fp32 sum of the six products a_i b_j with i + j <= 4) and the three-plane images
SIX = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))


def _rne_bf16_finite(a):
    """rne_bf16 for finite values below the largest bfloat16 (what a split meets), in 32-bit arithmetic: the same bits, a quarter of the time."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = (u >> np.uint32(16)) & np.uint32(1)
    r += np.uint32(0x7FFF)
    r += u
    r &= np.uint32(0xFFFF0000)
    return r.view(np.float32).reshape(np.shape(a))


def split3(a, rnd=None):
    """float32 -> its three bfloat16 terms, as float32 arrays.  rnd replaces nearest-even by a wrong rounding."""
    a = np.ascontiguousarray(a, np.float32)
    if rnd is None:
        rnd = _rne_bf16_finite if a.size == 0 or float(np.abs(a).max()) < 3.0e38 else rne_bf16          # (a NaN compares false: rne_bf16)
    x1 = rnd(a)
    r1 = a - x1
    x2 = rnd(r1)
    return x1, x2, rnd(r1 - x2)


def split_product(a, b, pairs=SIX, rnd=None):
    """a [M][K] @ b [K][N] as the float64 sum of the kept plane products a_i b_j, (i, j) in pairs."""
    pa, pb = split3(a, rnd), split3(b, rnd)
    out = np.zeros((np.shape(a)[0], np.shape(b)[1]))
    for i in (1, 2, 3):
        js = [j for ii, j in pairs if ii == i]
        if js:
            out += _f64(pa[i - 1]) @ sum(_f64(pb[j - 1]) for j in js)
    return out


def plane_bits(a, rnd=None):
    """float32 [n] -> uint16 [3][n]: the bits of the three terms."""
    return np.stack([(p.view(np.uint32) >> np.uint32(16)).astype(np.uint16) for p in split3(np.ravel(a), rnd)])


def image_at(e):
    """Element e of a region (counted from its 128-byte aligned base) -> the uint16 index of its term 0 in the image ("I32": 32 elements <-> 192
    bytes [x1 of the 32 | x2 of the 32 | x3 of the 32]); term p lies 32 * p further on."""
    e = np.asarray(e, np.int64)
    return (e // 32) * 96 + e % 32


def image_len(n):
    """uint16 elements of the image of a region of n floats: FFH_BF16X3_IMAGE_BYTES(4 n) / 2."""
    return (4 * n + 127) // 128 * 96


def _aligned(be, flat, align=128):
    """flat uploaded to an allocation whose base is `align`-byte aligned (over-allocated where the backend does not give that)."""
    h = be.upload(flat)
    if be.addr(h) % align == 0:
        return h
    assert isinstance(h, np.ndarray), "the device allocator is expected to give 128-byte aligned blocks"
    raw = np.empty(flat.nbytes + align, np.uint8)
    at = -raw.ctypes.data % align
    v = raw[at:at + flat.nbytes].view(flat.dtype)
    v[:] = flat
    return v


class ImageBuf:
    """The three-plane image of a Buf (ffh_ctx_bf16x3_mirror_set): the region is the Buf's whole allocation.  Every position holds SENTINEL16; an
    input's image is filled over the valid block by ffh_convert_f32_to_bf16x3 (fill()), an output's stays sentinel."""

    def __init__(self, be, buf):
        self.be, self.buf = be, buf
        if be.addr(buf.h) % 128:
            buf.h = _aligned(be, be.download(buf.h))
        self.before = np.full(image_len(buf.valid.size), SENTINEL16, np.uint16)
        self.at = image_at(buf.idx)[None, :] + 32 * np.arange(3)[:, None]          # [3][rows * cols]
        self.valid = np.zeros(self.before.size, bool)
        self.valid[self.at.ravel()] = True
        self.h = _aligned(be, self.before.view(np.int16))
        self.host = None

    @property
    def base(self):
        return self.be.addr(self.h)

    def register(self, lib):
        base = self.be.addr(self.buf.h)
        assert base % 128 == 0 and self.base % 128 == 0, "ffh_ctx_bf16x3_mirror_set wants 128-byte aligned bases"
        lib.check(lib.lib.ffh_ctx_bf16x3_mirror_set(lib.ctx, base, 4 * self.buf.valid.size, self.base), "ffh_ctx_bf16x3_mirror_set")
        return base

    def fill(self, lib):
        """What a model's producers leave in the image of a buffer they wrote: the planes of the valid block, row by row where it is strided."""
        b = self.buf
        runs = [(0, b.rows * b.cols)] if b.ld == b.cols or b.rows <= 1 else [(r * b.ld, b.cols) for r in range(b.rows)]
        for at, n in runs:
            if n:
                lib.check(lib.lib.ffh_convert_f32_to_bf16x3(lib.ctx, b.ptr + 4 * at, 1, n, n, None), "ffh_convert_f32_to_bf16x3")
        return self

    def poison(self, bits=0x7FC0):
        """A stale image: the three planes of the valid block replaced by bfloat16 NaN."""
        flat = self.be.download(self.h).view(np.uint16).copy()
        flat[self.valid] = bits
        self.h = None
        self.h = _aligned(self.be, flat.view(np.int16))
        return self

    def snapshot(self):
        self.before = self.be.download(self.h).view(np.uint16).copy()
        return self

    def fetch(self):
        self.host = self.be.download(self.h).view(np.uint16)
        return self

    def untouched(self):
        return self.host.tobytes() == self.before.tobytes()

    def problems(self, name, stored=None, must_write=False):
        """An output's image after the call (stored: the [rows][cols] floats the library left in the fp32 buffer): untouched as a whole, or the three
        terms of `stored` over the valid block and the sentinel everywhere else.  stored None: an input's image, identical to before."""
        out = []
        if stored is None:
            if not self.untouched():
                out.append(f"{name} image: an input's image was modified ({int((self.host != self.before).sum())} positions)")
            return out
        if self.untouched():
            if must_write:
                out.append(f"{name} image: not written by a launch of the split mode's kernels")
            return out
        pad = np.flatnonzero((self.host != SENTINEL16) & ~self.valid)
        if pad.size:
            out.append(f"{name} image: {pad.size} position(s) outside the valid block written, first at uint16 index {int(pad[0])} (group {int(pad[0]) // 96}, "
                       f"term {int(pad[0]) % 96 // 32}, element {int(pad[0]) % 32}; ld {self.buf.ld}, offset {self.buf.off})")
        want, got = plane_bits(stored), self.host[self.at]
        bad = np.argwhere(got != want)
        if bad.size:
            p, k = (int(v) for v in bad[0])
            r, c = divmod(k, self.buf.cols)
            out.append(f"{name} image: {bad.shape[0]} of {got.size} terms are not the split of the stored float; first: term {p + 1} of ({r}, {c}): "
                       f"0x{int(got[p, k]):04x}, expected 0x{int(want[p, k]):04x}")
        return out


class Images:
    """The image registrations of one call: made before it, undone whatever happens (the ctx is the whole session's).  An input's image, once
    filled, has to be what the numpy restatement says: ffh_convert_f32_to_bf16x3 is one of the passes under test."""

    def __init__(self, lib, be, case, bufs, inputs):
        self.lib, self.t, self.inputs, self.regs = lib, {}, set(inputs), []
        try:
            for name in IMAGE_NAMES:
                buf = bufs.get(name)
                if name not in case.images or buf is None:
                    continue
                im = self.t[name] = ImageBuf(be, buf)
                self.regs.append((im.register(lib), 4 * buf.valid.size))
                if name in self.inputs:
                    im.fill(lib)
            be.sync()
            for name, im in self.t.items():
                if name in self.inputs:
                    bad = im.fetch().problems(name, im.buf.before[im.buf.idx].reshape(im.buf.rows, im.buf.cols), must_write=im.buf.idx.size > 0)
                    assert not bad, f"{case.name}: ffh_convert_f32_to_bf16x3 left a wrong image: {bad}"
                if name in case.stale:
                    im.poison()
                    im.register(lib)
                im.snapshot()
        except BaseException:
            self.release()
            raise

    def release(self):
        for base, nbytes in self.regs:
            self.lib.lib.ffh_ctx_bf16x3_mirror_set(self.lib.ctx, base, nbytes, None)
        self.regs = []


class _Regs:
    """Twins and Images of one call behind one release()."""

    def __init__(self, lib, be, case, bufs, inputs):
        self.parts = []
        try:
            self.parts.append(Twins(lib, be, case, bufs, inputs))
            self.parts.append(Images(lib, be, case, bufs, inputs))
        except BaseException:
            self.release()
            raise
        self.t = {**self.parts[0].t, **self.parts[1].t}

    def release(self):
        for p in self.parts:
            p.release()


def _set_mode(lib, mode):
    lib.check(lib.lib.ffh_ctx_set_math_mode(lib.ctx, mode), "ffh_ctx_set_math_mode")


# ---------------------------------------------------------------------------------------------------------------------------
# the calls
class Result:
    def __init__(self, case, inp, rc, route, **kw):
        self.case, self.inp, self.rc, self.route = case, inp, rc, route
        self.scatter_used = self.colsum_used = 0
        self.is_hip = False
        self.twins, self.twin_inputs = {}, ()
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
    tw = None
    try:
        _set_mode(lib, case.mode)
        tw = _Regs(lib, be, case, dict(x=X, w=W, y=Y), ("x", "w"))
        rc = lib.lib.ffh_linear_fwd(lib.ctx, X.ptr, case.ldx, Y.ptr, case.ldy, W.ptr, Bi.ptr if Bi else None, i, o, B, case.act, s)
        route = (lib.lib.ffh_linear_last_route(lib.ctx) or b"").decode()
        _finish(lib, be, [s])
    finally:
        if tw:
            tw.release()
        _set_mode(lib, 0)
    inputs = [("x", X), ("w", W)] + ([("bias", Bi)] if Bi else [])
    for _, b in inputs + [("y", Y)] + list(tw.t.items()):
        b.fetch()
    return Result(case, inp, rc, route, is_hip=be.is_hip, Y=Y, outputs=[("y", Y)], inputs=inputs, twins=tw.t, twin_inputs=("x", "w"))


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
    tw = None
    try:
        _set_mode(lib, case.mode)
        if case.det:
            lib.check(lib.lib.ffh_ctx_set_deterministic(lib.ctx, 1), "deterministic")
        tw = _Regs(lib, be, case, dict(x=X, w=W, y=Y, dy=DY, dx=DX), ("x", "w", "y", "dy"))
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
        if tw:
            tw.release()
        if case.det:
            lib.check(lib.lib.ffh_ctx_set_deterministic(lib.ctx, 0), "deterministic")
        _set_mode(lib, 0)
    inputs = [("x", X), ("w", W), ("y", Y)]
    outs = [("dy", DY), ("dw", DW)] + ([("db", DB)] if DB else []) + ([("dx", DX)] if DX else [])
    outs += [(f"dest{k}", d) for k, d in enumerate(dests)] + ([("colsum", CS)] if CS else [])
    for _, b in inputs + outs + list(tw.t.items()):
        b.fetch()
    return Result(case, inp, rc, route, is_hip=be.is_hip, DY=DY, DW=DW, DB=DB, DX=DX, dests=dests, CS=CS, outputs=outs, inputs=inputs, scatter_used=su, colsum_used=cu,
                  keepalive=cmap_h, twins=tw.t, twin_inputs=("x", "w", "y", "dy"))


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


def _twins(rep, res, written):
    """written: output name -> (the floats the library stored, whether the route obliges the call to write the twin)."""
    for name, tw in res.twins.items():
        if name in written and res.is_hip:
            stored, must = written[name]
            rep.violations += tw.problems(name, stored, must)
        elif name in written:       # the oracle library's ffh_ctx_bf16_mirror_set is a no-op: untouched is the expected outcome
            rep.violations += tw.problems(name, written[name][0], False)
        else:
            rep.violations += tw.problems(name)


def _operand_rounding(case, rnd):
    """The rounding the GEMM operands of this case go through: the identity in fp32 mode and on a narrow layer, else nearest-even to bfloat16
    (include/ff_hip.h, FFH_MATH_TENSOR_OP_BF16); `rnd` replaces nearest-even by a wrong rounding (the discrimination tests)."""
    if not case.bf16_layer:
        return _f64
    return lambda a: _f64((rnd or rne_bf16)(np.asarray(a, np.float32)))


def _product(case):
    """a @ b as the reference of this case sums it: in float64 over the operands as they come, or, for the "planes" family on a layer of the split
    mode, the six kept plane products (exact in float64: integers below 2^53)."""
    if case.planes_exact:
        return lambda a, b: split_product(np.asarray(a, np.float32), np.asarray(b, np.float32))
    return lambda a, b: a @ b


def _on_pipe(tok):
    """The token names a launch that keeps the output's twin / image current (include/ff_hip.h)."""
    return "bf16" in tok or "x3_dma" in tok


def check_fwd(res, rnd=None):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    r = _operand_rounding(case, rnd)
    x, w = r(inp["x"]), r(inp["w"])
    b = _f64(inp["b"]) if case.bias else np.zeros(case.out_dim)
    _compare(rep, "y", res.Y.get(), act64(_product(case)(x, w.T) + b, case.act), np.abs(x) @ np.abs(w).T + np.abs(b), LIPSCHITZ[case.act],
             case.integer or case.planes_exact)
    _buffers(rep, res)
    _twins(rep, res, {"y": (res.Y.get(), _on_pipe(res.route))})
    return rep


def must_decline_scatter(case):
    """The contract's own exclusions (every library): an accumulating call, another width, no data gradient."""
    return not case.has(OVERWRITE) or case.cmap_ncols != case.in_dim or case.has(ONLY_DW) or not case.dx


def must_decline_colsum(case):
    return not case.has(OVERWRITE) or case.colsum_ncols != case.in_dim or case.has(ONLY_DW) or not case.dx or case.cmap


def check_bwd(res, rnd=None):
    case, inp, rep = res.case, res.inp, Report()
    if res.rc != capi.FFH_OK:
        rep.violations.append(f"rc = {res.rc}")
        return rep
    x, w, y, g = _f64(inp["x"]), _f64(inp["w"]), _f64(inp["y"]), _f64(inp["g"])
    r = _operand_rounding(case, rnd)
    xr, wr = r(inp["x"]), r(inp["w"])          # the GEMMs' operands; the masks, db and the dy transform stay on the unrounded values
    only_dx, only_dw, ex = case.has(ONLY_DX), case.has(ONLY_DW), case.integer
    prod, exg = _product(case), case.integer or case.planes_exact          # (db is a plain fp32 sum of unsplit values: exact on integers only)
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
        effr = r(eff)
        _compare(rep, "dw", res.DW.get(), _f64(inp["dw0"]) + prod(effr.T, xr), np.abs(_f64(inp["dw0"])) + np.abs(effr).T @ np.abs(xr), exact=exg)
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
            effr = r(eff)
            ref, mass = prod(effr, wr), np.abs(effr) @ np.abs(wr)
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
                _compare(rep, "dx", res.DX.get(), ref, mass, exact=exg)
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
    written = {}
    if res.DX is not None and not only_dw:
        written["dx"] = (res.DX.get(), any("dx" in t.split("|")[0] and _on_pipe(t) for t in res.route.split(";")) and not (res.scatter_used and case.cmap))
    _twins(rep, res, written)
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


# --- FFH_MATH_TENSOR_OP_BF16: launch_gemm_bf16 (csrc/linear_bf16.hip) and launch_gemm_bf16_dma (csrc/linear_bf16_dma.hip), restated
def bf16_dma_dw_split(cus, tiles, nk):
    """The LDS-DMA weight gradient's cost search over the number of k-slices (the same double arithmetic), or None: no candidate."""
    best, splitk = 1e30, None
    for sp in range(1, 65):
        if sp * 4 > nk:
            break
        nb = tiles * sp
        if nb * 2 < cus:
            continue
        t = float(_cdiv(nb, cus)) * float(_cdiv(nk, sp)) * 1.0 + float(nb) * (256.0 * 256 * 4) / 1.3e6
        if t < best:
            best, splitk = t, sp
    return splitk


def bf16_gemm(c, cus, name, form, M, N, K, epi, lda, ldb, ldc, a, b, a_off, b_off, c_off, masking=False, a_stale=False, bias_off=None, mask=None):
    """The token of one bf16-pipe GEMM.  form "fwd" / "dx" / "dw"; a, b: the operand buffers' names (their twins are looked up in c.twins) and
    offsets; a_stale: a live activation derivative rewrote dy in place; mask: (offset, leading dimension) of the mask-by-x operand.  (A bias
    gradient handed to the LDS-DMA weight gradient wants dy 16-byte aligned and out_dim % 4 == 0: both follow from the twins' own conditions.)"""
    tiles_big = _cdiv(N, 256) * _cdiv(M, 256)
    big = (form == "fwd" or (form == "dx" and K >= 1024)) and M >= 256 and N >= 256 and tiles_big >= cus
    if form == "dw" and epi == "atomic" and not c.det and tiles_big >= 32 and K >= 8192:
        big = True
    bt = 256 if big else 128
    tiles = _cdiv(N, bt) * _cdiv(M, bt)
    splitk, kps = 1, K
    if epi == "atomic" and c.det:
        epi = "add"
    if epi == "atomic":
        want = _cdiv((1 if big else 2) * cus, tiles)
        max_split = _cdiv(K, 256)                       # at least four k-tiles per workgroup
        if big:                                         # the split whose workgroups fill whole rounds of one per CU best
            best, best_u = want, 0.0
            for w2 in range(want, min(2 * want + 2, max_split) + 1):
                nb = tiles * w2
                u = float(nb) / float(_cdiv(nb, cus) * cus)
                if u > best_u + 1e-9:
                    best_u, best = u, w2
            want = best
        want = max(1, min(want, max_split))
        kps = _cdiv(_cdiv(K, want), 64) * 64
        splitk = max(2, _cdiv(K, kps))                  # a search that ends at 1 launches two splits, the second one empty
    twins = (not masking and not a_stale and M % 8 == 0 and N % 8 == 0 and M >= 8 and N >= 8 and K % 64 == 0 and kps % 64 == 0 and lda % 8 == 0
             and ldb % 8 == 0 and a in c.twins and b in c.twins and a_off % 8 == 0 and b_off % 8 == 0)
    if twins:
        ok = ldc % 4 == 0 and c_off % 4 == 0 and (bias_off is None or bias_off % 4 == 0) and (mask is None or (mask[0] % 4 == 0 and mask[1] % 4 == 0))
        t256 = _cdiv(M, 256) * _cdiv(N, 256)
        if ok and form == "dw":
            sp = bf16_dma_dw_split(cus, t256, K // 64) if epi == "atomic" and t256 >= 2 else None
            if sp:
                slots = sp > 1 and t256 * sp <= 512 and t256 * sp <= cus and c.scratch
                return f"{name}|bf16_dma_256x256_twins" + ("|slots" if slots else "")
        elif ok and (form == "dx" or epi == "store") and t256 * 100 >= cus * 50:
            return f"{name}|bf16_dma_256x256_twins"
    return f"{name}|bf16_{bt}x{bt}{'_twins' if twins else ''}|splitk={splitk}"


# --- FFH_MATH_FP32_SPLIT_BF16X3_ALL: the split branch of launch_gemm_bf16 (csrc/linear_bf16.hip) and launch_gemm_x3_dma (csrc/linear_x3_dma.hip), restated
def x3_dma_dw_split(cus, tiles, nk):
    """The LDS-DMA weight gradient's cost search over the number of k-slices (nk k-tiles of 32; at least eight a slice), or None: no candidate."""
    best, splitk = 1e30, None
    for sp in range(1, 65):
        if sp * 8 > nk:
            break
        nb = tiles * sp
        if nb * 2 < cus:
            continue
        t = float(_cdiv(nb, cus)) * float(_cdiv(nk, sp)) * 3.0 + float(nb) * (256.0 * 256 * 4) / 1.3e6
        if t < best:
            best, splitk = t, sp
    return splitk


def x3_gemm(c, cus, name, form, M, N, K, epi, lda, ldb, ldc, a, b, a_off, b_off, c_off, masking=False, a_stale=False, bias_off=None, mask=None, cname=None,
            db=False):
    """The token of one split-mode GEMM; the arguments of bf16_gemm, the images looked up in c.images; cname: the output's buffer (its image in
    place: "+image"); db: the bias gradient is handed to the weight-gradient GEMM.  The kernel behind bf16x3_128x128 is part of the token: v2w8 /
    v2w4 (gemm_bf16x3_v2_kernel on eight or four waves: forward and data gradient) or mfma32 (gemm_bf16x3_kernel: the weight gradient)."""
    tiles_big = _cdiv(N, 256) * _cdiv(M, 256)
    big = (form == "fwd" or (form == "dx" and K >= 1024)) and M >= 256 and N >= 256 and tiles_big >= cus
    if form == "dw" and epi == "atomic" and not c.det and tiles_big >= 32 and K >= 8192:
        big = True
    bt = 256 if big else 128
    tiles = _cdiv(N, bt) * _cdiv(M, bt)
    splitk = 1
    if epi == "atomic" and c.det:
        epi = "add"
    if epi == "atomic":
        want = _cdiv((1 if big else 2) * cus, tiles)
        max_split = _cdiv(K, 256)
        if big:
            best, best_u = want, 0.0
            for w2 in range(want, min(2 * want + 2, max_split) + 1):
                nb = tiles * w2
                u = float(nb) / float(_cdiv(nb, cus) * cus)
                if u > best_u + 1e-9:
                    best_u, best = u, w2
            want = best
        want = max(1, min(want, max_split))
        kps = _cdiv(_cdiv(K, want), 64) * 64
        splitk = max(2, _cdiv(K, kps))
    served = (not masking and not a_stale and K % 32 == 0 and N % 8 == 0 and lda % 32 == 0 and ldb % 32 == 0 and ldc % 4 == 0 and c_off % 4 == 0
              and (bias_off is None or bias_off % 4 == 0) and (mask is None or (mask[0] % 4 == 0 and mask[1] % 4 == 0))
              and not (form == "dw" and db and (a_off % 4 or M % 4)) and a in c.images and b in c.images and a_off % 32 == 0 and b_off % 32 == 0)
    if served:
        t256 = _cdiv(M, 256) * _cdiv(N, 256)
        if form == "dw":
            sp = x3_dma_dw_split(cus, t256, K // 32) if epi == "atomic" and t256 >= 2 else None
            if sp:
                slots = sp > 1 and t256 * sp <= 512 and t256 * sp <= cus and c.scratch
                return f"{name}|x3_dma_256x256_planes" + ("|slots" if slots else "")
        elif (form == "dx" or epi == "store") and t256 * 100 >= cus * 75:
            return f"{name}|x3_dma_256x256_planes" + ("+image" if ldc % 32 == 0 and c_off % 32 == 0 and cname in c.images else "")
    if big and epi == "atomic":
        return f"{name}|bf16x3_256x256|splitk={splitk}"
    if form in ("fwd", "dx") and epi != "atomic":
        return f"{name}|bf16x3_128x128|splitk={splitk}|" + ("v2w8" if _cdiv(N, 128) * _cdiv(M, 128) * 100 <= cus * 150 else "v2w4")
    return f"{name}|bf16x3_128x128|splitk={splitk}|mfma32"


def route_fwd_bf16(c, cus):
    gemm = x3_gemm if c.x3_layer else bf16_gemm
    return [gemm(c, cus, "linear_fwd gemm (bf16)", "fwd", c.batch, c.out_dim, c.in_dim, "store", c.ldx, c.in_dim, c.ldy, "x", "w", c.x_off, c.w_off,
                 c.y_off, bias_off=c.bias_off if c.bias else None, **(dict(cname="y") if c.x3_layer else {}))]


def _bwd_bf16(st, c, cus, do_dw, do_dx):
    """linear_bwd_impl's tensor-op branch (csrc/linear.hip): the activation gradient as its own pass (no token), the weight gradient, then the data
    gradient; a column map or a column-sum request is not looked at in this mode (declined: ffh_linear_bwd_ex drops it after the call)."""
    i, o, B, toks = c.in_dim, c.out_dim, c.batch, st["toks"]
    act = NONE if c.has(PREMASKED) else c.act
    relu = act == RELU
    relu_done = relu and do_dw and do_dx and c.dx           # the mask is written to dy in front of the fork: both GEMMs read a final dy
    if relu_done:
        relu = False
    forked = do_dw and do_dx and c.forked
    gemm, kw_dw, kw_dx = bf16_gemm, {}, {}
    if c.x3_layer:          # the same call sites in the split mode; the bias gradient rides on the weight-gradient GEMM where no activation pass runs
        gemm, kw_dw, kw_dx = x3_gemm, dict(db=c.db and act == NONE), dict(cname="dx")
    if do_dw:
        toks.append(gemm(c, cus, "linear_bwd dw gemm (bf16)", "dw", o, i, B, "atomic", c.lddy, c.ldx, i, "dy", "x", c.dy_off, c.x_off, 0, a_stale=act != NONE, **kw_dw))
    if c.dx and do_dx:
        masking = (forked or not do_dw) and relu
        toks.append(gemm(c, cus, "linear_bwd dx gemm (bf16, masking)" if masking else "linear_bwd dx gemm (bf16)", "dx", B, i, o,
                         "store" if c.has(OVERWRITE) else "add", c.lddy, i, c.lddx, "dy", "w", c.dy_off, c.w_off, c.dx_off, masking=masking,
                         a_stale=act != NONE, mask=(c.x_off, c.ldx) if c.has(MASK_BY_X) else None, **kw_dx))


def route_fwd(c, cus):
    i, o, B = c.in_dim, c.out_dim, c.batch
    if o <= 4:
        return ["linear_fwd|skinny"]
    if i <= 16 and o >= 64 and B < 16384:
        return ["linear_fwd|thin"]
    if c.bf16_layer or c.x3_layer:
        return route_fwd_bf16(c, cus)
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
    if c.bf16_layer or c.x3_layer:
        _bwd_bf16(st, c, cus, do_dw, do_dx)
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
    """The library's tokens without the split and workgroup counts that route_fwd / route_bwd do not predict: every one except the split count of
    the bf16-pipe kernels of csrc/linear_bf16.hip in tensor-op mode (the LDS-DMA kernel's comes from a cost search: dma_splits() checks its range)."""
    keep = re.compile(r"\|bf16(_(128x128|256x256)(_twins)?\|splitk=\d+|x3_(128x128|256x256)\|splitk=\d+(\|\w+)?)$")
    return [t if keep.search(t) else re.sub(r"\|(splitk|wgs)=\d+", "", t) for t in route.split(";") if t]


def dma_splits(route):
    """(token, splitk) of every LDS-DMA bf16 launch named in a route."""
    return [(t, int(m.group(1))) for t in route.split(";") for m in [re.search(r"bf16_dma_256x256_twins\|splitk=(\d+)(\|slots)?$", t)] if m]


def x3_dma_splits(route):
    """(token, splitk) of every launch of the split mode's LDS-DMA kernel named in a route."""
    return [(t, int(m.group(1))) for t in route.split(";") for m in [re.search(r"x3_dma_256x256_planes(?:\+image)?\|splitk=(\d+)(\|slots)?$", t)] if m]


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
                    if "skinny" in t or ("dw" in t.split("|")[0] and ("|sk_" in t or "glds" in t or not re.search(r"splitk=1(\|\w+)?$", t)))]
        for t, sp in dma_splits(res.route):
            if "dw" in t.split("|")[0]:
                if not (1 <= sp and 4 * sp <= case.batch // 64):
                    out.append(f"{t!r}: a split of {sp} slices does not leave four k-tiles each at batch {case.batch}")
            elif sp != 1:
                out.append(f"{t!r}: only the weight gradient splits K")
        for t, sp in x3_dma_splits(res.route):
            if "dw" in t.split("|")[0]:
                if not (1 <= sp and 8 * sp <= case.batch // 32):
                    out.append(f"{t!r}: a split of {sp} slices does not leave eight k-tiles of 32 each at batch {case.batch}")
            elif sp != 1:
                out.append(f"{t!r}: only the weight gradient splits K")
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


# ---------------------------------------------------------------------------------------------------------------------------
# FFH_MATH_TENSOR_OP_BF16: the edge table (shapes derived for 256 CUs from bf16_gemm above) and the random cases
def _bf16_table(t):
    M1 = dict(mode=MATH_BF16)
    F, DWT, DXT, DXM = "linear_fwd gemm (bf16)|", "linear_bwd dw gemm (bf16)|", "linear_bwd dx gemm (bf16)|", "linear_bwd dx gemm (bf16, masking)|"
    S, BIG, ST, BIGT, DMA = "bf16_128x128|splitk=", "bf16_256x256|splitk=", "bf16_128x128_twins|splitk=", "bf16_256x256_twins|splitk=", "bf16_dma_256x256_twins"
    # 128 x 128 tiles, fp32 operands rounded in the kernel: any wide layer below 256 tiles of 256 x 256.  Ragged in M, N and K (K neither a
    # multiple of 64 nor of 4: the guarded loader), every offset, padded rows, no bias, the four activations.
    t["bf16-128-fwd"] = [
        Case("b-fwd-129->130", "fwd", 129, 130, 70, RELU, ldx=133, x_off=1, ldy=131, y_off=2, w_off=1, want=F + S + "1", **M1),
        Case("b-fwd-136->257", "fwd", 136, 257, 300, SIG, bias=False, ldy=260, x_off=4, want=F + S + "1", **M1),
        Case("b-fwd-192->128", "fwd", 192, 128, 257, GELU, bias_off=1, w_off=4, y_off=4, want=F + S + "1", **M1),
        Case("b-fwd-130->192-int", "fwd", 130, 192, 129, NONE, integer=True, bias_off=2, want=F + S + "1", **M1),
        Case("b-fwd-192->136-ties", "fwd", 192, 136, 200, RELU, dist="ties", want=F + S + "1", **M1),
        Case("b-fwd-257->129-wide", "fwd", 257, 129, 130, NONE, dist="wide", w_off=2, ldx=260, want=F + S + "1", **M1)]
    # dX: accumulating (EPI_ADD), storing (EPI_STORE), masked by x; a live ReLU with both gradients is applied to dy in front of the fork (plain
    # form, forked or not), under ONLY_DX it is read through relu'(y) (the masking form).  The dW beside them splits K by atomics:
    # tiles = cdiv(out, 128) * cdiv(in, 128), want = cdiv(512, tiles) capped at cdiv(batch, 256).
    t["bf16-128-dx"] = [
        Case("b-dx-add", "bwd", 129, 130, 700, NONE, 0, lddy=133, dy_off=1, lddx=131, dx_off=2, want=(DXT + S + "1", DWT + S + "3"), **M1),
        Case("b-dx-store", "bwd", 136, 257, 300, SIG, OVERWRITE, w_off=1, ldx=137, x_off=4, db=False, want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-mask-by-x", "bwd", 192, 128, 257, RELU, OVERWRITE | MASK_BY_X | PREMASKED, ldx=195, x_off=1, want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-live-relu-forked", "bwd", 130, 192, 129, RELU, MASK_BY_X, forked=True, ldy=193, y_off=2, want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-live-relu", "bwd", 257, 129, 130, RELU, OVERWRITE, want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-masking-only-dx", "bwd", 129, 136, 200, RELU, ONLY_DX | OVERWRITE, lddy=137, ldy=139, dy_off=2, want=DXM + S + "1", **M1),
        Case("b-dx-masking-only-dx-add-maskx", "bwd", 192, 257, 77, RELU, ONLY_DX | MASK_BY_X, dx_off=1, want=DXM + S + "1", **M1),
        Case("b-dx-sigmoid-only-dx", "bwd", 130, 129, 131, SIG, ONLY_DX, want=DXT + S + "1", **M1),
        Case("b-dx-int", "bwd", 130, 192, 129, RELU, OVERWRITE, integer=True, want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-masking-int", "bwd", 136, 129, 70, RELU, ONLY_DX | OVERWRITE, integer=True, want=DXM + S + "1", **M1),
        Case("b-dx-ties", "bwd", 192, 136, 200, NONE, OVERWRITE, dist="ties", want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-masking-ties", "bwd", 192, 136, 200, RELU, ONLY_DX | OVERWRITE, dist="ties", want=DXM + S + "1", **M1),
        Case("b-dx-masking-wide", "bwd", 257, 130, 131, RELU, ONLY_DX, dist="wide", lddy=131, want=DXM + S + "1", **M1),
        Case("b-dx-wide", "bwd", 257, 129, 130, NONE, 0, dist="wide", want=(DXT + S + "1", DWT + S + "2"), **M1),
        Case("b-dx-column-map-declined", "bwd", 129, 130, 70, NONE, OVERWRITE, cmap=True, colsum=True, want=(DXT + S + "1", "scatter_used=0", "colsum_used=0"), **M1)]
    # dW alone: 700 x (130 -> 129): 4 tiles, want 128 capped at cdiv(700, 256) = 3 -> 256 samples per split, 3 splits; 1100 x (257 -> 136): 6 tiles,
    # want 86 capped at 5 -> 256 per split, 5 splits, the last one 76 deep (not a multiple of 4); no dx, no db, the three activations
    t["bf16-128-dw-splitk"] = [
        Case("b-dw-3-splits", "bwd", 130, 129, 700, RELU, ONLY_DW, lddy=131, dy_off=1, ldx=133, x_off=2, want=DWT + S + "3", **M1),
        Case("b-dw-5-splits-sigmoid", "bwd", 257, 136, 1100, SIG, ONLY_DW, db=False, want=DWT + S + "5", **M1),
        Case("b-dw-no-dx", "bwd", 136, 130, 513, NONE, 0, dx=False, want=DWT + S + "3", **M1),
        Case("b-dw-int", "bwd", 129, 192, 700, NONE, ONLY_DW, integer=True, want=DWT + S + "3", **M1),
        Case("b-dw-ties", "bwd", 192, 136, 700, NONE, ONLY_DW, dist="ties", want=DWT + S + "3", **M1),
        Case("b-dw-wide", "bwd", 130, 257, 700, RELU, ONLY_DW | PREMASKED, dist="wide", want=DWT + S + "3", **M1)]
    # batch <= 256: cdiv(batch, 256) = 1 caps the search at one split, and the launch runs with two, the second one empty
    t["bf16-128-dw-empty-second-split"] = [
        Case("b-dw-empty-70", "bwd", 129, 130, 70, RELU, ONLY_DW, want=DWT + S + "2", **M1),
        Case("b-dw-empty-256", "bwd", 192, 136, 256, NONE, OVERWRITE, want=DWT + S + "2", **M1),
        Case("b-dw-empty-255-int", "bwd", 130, 129, 255, NONE, ONLY_DW, integer=True, want=DWT + S + "2", **M1)]
    # deterministic mode: the same weight gradients as one ordered split adding into dw
    t["bf16-deterministic"] = [
        Case("b-det-700", "bwd", 130, 129, 700, RELU, ONLY_DW, det=True, lddy=131, dy_off=1, want=DWT + S + "1", **M1),
        Case("b-det-1100-sigmoid", "bwd", 257, 136, 1100, SIG, 0, det=True, want=(DWT + S + "1", DXT + S + "1"), **M1),
        Case("b-det-70", "bwd", 129, 130, 70, NONE, OVERWRITE, det=True, want=DWT + S + "1", **M1),
        Case("b-det-twins", "bwd", 192, 192, 192, NONE, OVERWRITE, det=True, twins=("x", "w", "dy", "dx"), want=(DWT + ST + "1", DXT + ST + "1"), **M1)]
    # 256 x 256 tiles: forward from 256 tiles on (both extents >= 256): 264 wide is 2 tile columns, so 128 tile rows: batch > 127 * 256 = 32512;
    # dX the same with a reduction depth (out_dim) >= 1024; dW from 32 tiles and batch 8192 on: 1030 x 1540 is 5 x 7 = 35 tiles, want cdiv(256, 35) = 8,
    # the search over 8 .. 18 splits takes the first fullest round
    t["bf16-256-fwd"] = [Case("b-big-fwd", "fwd", 136, 264, 32520, RELU, ldx=137, x_off=1, y_off=2, want=F + BIG + "1", **M1)]
    t["bf16-256-dx"] = [Case("b-big-dx", "bwd", 264, 1030, 32520, RELU, ONLY_DX | OVERWRITE | MASK_BY_X | PREMASKED, dx_off=1, want=DXT + BIG + "1", **M1)]
    # ... and the masking form (a live ReLU under ONLY_DX: dy read through relu'(y), y the third operand, its rows ldy apart) takes the same tile by the
    # same rule; the twins forms never serve it, so bf16_128x128 and bf16_256x256 are all it has.  Storing and accumulating, ragged in M, N and K
    t["bf16-256-dx-masking"] = [
        Case("b-big-dx-masking-store", "bwd", 264, 1030, 32520, RELU, ONLY_DX | OVERWRITE, lddy=1033, dy_off=1, ldy=1031, y_off=2, lddx=265, want=DXM + BIG + "1", **M1),
        Case("b-big-dx-masking-add-maskx", "bwd", 264, 1030, 32520, RELU, ONLY_DX | MASK_BY_X, ldy=1032, dx_off=1, ldx=267, x_off=1, want=DXM + BIG + "1", **M1)]
    t["bf16-256-dw"] = [Case("b-big-dw", "bwd", 1540, 1030, 8200, NONE, ONLY_DW, want=DWT + BIG, **M1)]
    # one tile fewer: 127 tile rows x 2 = 254 tiles; 5 x 6 = 30 tiles; the masking dX at 254 tiles
    t["bf16-256-tile-boundary"] = [
        Case("b-big-fwd-254-tiles", "fwd", 136, 264, 32504, RELU, want=F + S + "1", **M1),
        Case("b-big-dx-masking-254-tiles", "bwd", 264, 1030, 32504, RELU, ONLY_DX | OVERWRITE, ldy=1031, want=DXM + S + "1", **M1),
        Case("b-big-dw-30-tiles", "bwd", 1536, 1030, 8200, NONE, ONLY_DW, db=False, want=DWT + S, **M1)]
    # twins on both operands, whole 8-element pieces (M, N multiples of 8, K a multiple of 64, rows multiples of 8 apart, bases 16-byte aligned),
    # fewer than 128 tiles of 256 x 256: the SRC16 form of the 128 x 128 kernel
    XW, BW = ("x", "w", "y"), ("x", "w", "dy", "dx")
    t["bf16-128-twins"] = [
        Case("b-tw-fwd", "fwd", 192, 136, 200, RELU, ldx=200, x_off=8, ldy=137, y_off=1, twins=XW, want=F + ST + "1", **M1),
        Case("b-tw-fwd-ties", "fwd", 192, 136, 200, NONE, twins=XW, dist="ties", want=F + ST + "1", **M1),
        Case("b-tw-bwd", "bwd", 136, 192, 192, RELU, PREMASKED | OVERWRITE | MASK_BY_X, lddy=200, dy_off=8, twins=BW, want=(DWT + ST + "2", DXT + ST + "1"), **M1),
        Case("b-tw-bwd-add-int", "bwd", 136, 192, 320, NONE, 0, twins=BW, integer=True, want=(DWT + ST + "2", DXT + ST + "1"), **M1),
        Case("b-tw-bwd-wide", "bwd", 136, 192, 192, NONE, OVERWRITE, twins=BW, dist="wide", want=(DWT + ST + "2", DXT + ST + "1"), **M1)]
    # the LDS-DMA kernel: twins, from 128 tiles of 256 x 256 on (half the CUs): 8200 rows are 33 tile rows (ragged, a multiple of 8) x 4 tile columns = 132
    t["bf16-dma-fwd"] = [Case("b-dma-fwd", "fwd", 128, 1000, 8200, RELU, twins=XW, want=F + DMA, **M1),
                         Case("b-dma-fwd-ties", "fwd", 128, 1000, 8200, SIG, twins=("x", "w"), dist="ties", bias=False, ldy=1004, want=F + DMA, **M1)]
    t["bf16-dma-dx"] = [
        Case("b-dma-dx-store", "bwd", 1000, 128, 8200, NONE, ONLY_DX | OVERWRITE, twins=BW, want=DXT + DMA, **M1),
        Case("b-dma-dx-add", "bwd", 1000, 128, 8200, RELU, ONLY_DX | PREMASKED, twins=("w", "dy"), lddx=1004, want=DXT + DMA, **M1),
        Case("b-dma-dx-mask-twin", "bwd", 1000, 128, 8200, NONE, ONLY_DX | OVERWRITE | MASK_BY_X, twins=BW, want=DXT + DMA, **M1),
        Case("b-dma-dx-mask-fp32", "bwd", 1000, 128, 8200, NONE, ONLY_DX | OVERWRITE | MASK_BY_X, twins=("w", "dy", "dx"), want=DXT + DMA, **M1)]
    # dW: 2 tiles (264 x 192) need 64 slices for 128 workgroups (half the CUs) and four k-tiles each: batch 64 * 4 * 64 = 16384; 6 tiles (520 x 320)
    # need 22 slices: batch 22 * 4 * 64 = 5632.  128 and 132 workgroups fit one round: the slices meet in the stream's slots, without scratch by atomics
    DW2 = dict(twins=("x", "dy"), **M1)
    t["bf16-dma-dw"] = [
        Case("b-dma-dw-2-tiles-db", "bwd", 192, 264, 16384, NONE, ONLY_DW, want=DWT + DMA + "|slots", **DW2),
        Case("b-dma-dw-2-tiles-no-db", "bwd", 192, 264, 16384, RELU, ONLY_DW | PREMASKED, db=False, want=DWT + DMA + "|slots", **DW2),
        Case("b-dma-dw-2-tiles-atomics", "bwd", 192, 264, 16384, NONE, ONLY_DW, scratch=False, want=DWT + DMA, **DW2),
        Case("b-dma-dw-6-tiles", "bwd", 320, 520, 5632, NONE, ONLY_DW, want=DWT + DMA + "|slots", **DW2),
        Case("b-dma-dw-6-tiles-atomics-int", "bwd", 320, 520, 5632, NONE, ONLY_DW, scratch=False, db=False, integer=True, want=DWT + DMA, **DW2)]
    # one tile row fewer (31 x 4 = 124 tiles) stays on the 128 x 128 twins form; a batch one k-tile short of 16384 has no split with four k-tiles a slice
    t["bf16-dma-boundary"] = [
        Case("b-dma-fwd-124-tiles", "fwd", 128, 1000, 7936, RELU, twins=XW, want=F + ST + "1", **M1),
        Case("b-dma-dw-declined", "bwd", 192, 264, 16320, NONE, ONLY_DW, want=DWT + ST + "64", **DW2)]
    # 256 tiles and twins, but the LDS-DMA kernel declines: a bias, rows of y or a base of y that is not 16-byte aligned
    t["bf16-256-twins-fwd"] = [
        Case("b-bigtw-bias-off", "fwd", 128, 264, 32520, RELU, twins=XW, bias_off=1, want=F + BIGT + "1", **M1),
        Case("b-bigtw-ldy", "fwd", 128, 264, 32520, NONE, twins=XW, ldy=266, want=F + BIGT + "1", **M1),
        Case("b-bigtw-y-off", "fwd", 128, 264, 32520, GELU, twins=("x", "w"), y_off=2, want=F + BIGT + "1", **M1)]
    t["bf16-256-twins-dx"] = [Case("b-bigtw-dx", "bwd", 264, 1088, 32520, NONE, ONLY_DX | OVERWRITE, twins=BW, dx_off=2, want=DXT + BIGT + "1", **M1)]
    # twins registered and not usable: the fp32 operands are rounded in the kernel, the output's twin is written all the same
    t["bf16-twins-not-usable"] = [
        Case("b-nt-m", "fwd", 192, 136, 201, RELU, twins=XW, want=F + S + "1", **M1),
        Case("b-nt-n", "fwd", 192, 130, 200, RELU, twins=XW, want=F + S + "1", **M1),
        Case("b-nt-k", "fwd", 136, 192, 200, NONE, twins=XW, want=F + S + "1", **M1),
        Case("b-nt-ldx", "fwd", 192, 136, 200, SIG, twins=XW, ldx=196, want=F + S + "1", **M1),
        Case("b-nt-x-off", "fwd", 192, 136, 200, RELU, twins=XW, x_off=4, want=F + S + "1", **M1),
        Case("b-nt-one-operand", "fwd", 192, 136, 200, RELU, twins=("x", "y"), want=F + S + "1", **M1),
        Case("b-nt-bwd-k", "bwd", 192, 136, 200, NONE, OVERWRITE, twins=BW, want=(DWT + S + "2", DXT + S + "1"), **M1)]
    # a live activation derivative rewrites dy in place and leaves its twin stale (NaN here): the twin must not be read
    t["bf16-stale-twins"] = [
        Case("b-stale-relu", "bwd", 136, 192, 192, RELU, OVERWRITE, twins=BW, stale=("dy",), want=(DWT + S + "2", DXT + S + "1"), **M1),
        Case("b-stale-sigmoid", "bwd", 136, 192, 192, SIG, 0, twins=BW, stale=("dy",), want=(DWT + S + "2", DXT + S + "1"), **M1),
        Case("b-stale-masking", "bwd", 136, 192, 192, RELU, ONLY_DX | OVERWRITE, twins=BW, stale=("dy",), want=DXM + S + "1", **M1),
        Case("b-stale-sigmoid-only-dw", "bwd", 136, 192, 192, SIG, ONLY_DW, twins=BW, stale=("dy",), want=DWT + S + "2", **M1)]
    # narrow layers keep the fp32 kernels and the fp32 reference (unrounded: a rounding kernel cannot meet the bound on uniform data)
    t["bf16-narrow-layers"] = [
        Case("b-narrow-in127", "fwd", 127, 256, 300, RELU, twins=XW, want="linear_fwd gemm|f32_", **M1),
        Case("b-narrow-out127", "fwd", 256, 127, 300, SIG, twins=XW, want="linear_fwd gemm|f32_", **M1),
        Case("b-narrow-bwd-in127", "bwd", 127, 256, 300, RELU, OVERWRITE, twins=BW, want=("linear_bwd dw gemm|f32_", "linear_bwd dx gemm|f32_"), **M1),
        Case("b-narrow-bwd-out127", "bwd", 256, 127, 300, NONE, 0, twins=BW, want=("linear_bwd dw gemm|f32_", "linear_bwd dx gemm|f32_"), **M1),
        Case("b-narrow-skinny-fwd", "fwd", 256, 4, 300, SIG, twins=XW, want="linear_fwd|skinny", **M1),
        Case("b-narrow-thin-fwd", "fwd", 13, 512, 300, RELU, twins=XW, want="linear_fwd|thin", **M1),
        Case("b-narrow-skinny-bwd", "bwd", 256, 1, 4100, SIG, OVERWRITE | MASK_BY_X, twins=BW, want="linear_bwd|skinny", **M1)]


# calls that have to be refused before anything is written: name -> (case, the error)
REFUSALS = {
    "gelu-in-the-backward": (Case("r", "bwd", 70, 40, 33, GELU), capi.FFH_ERR_UNSUPPORTED),
    "only-dx-and-only-dw": (Case("r", "bwd", 70, 40, 33, RELU, ONLY_DX | ONLY_DW), capi.FFH_ERR_BAD_ARG),
    "ldx-below-in-dim": (Case("r", "bwd", 70, 40, 33, RELU, ldx=69), capi.FFH_ERR_BAD_ARG),
    "ldy-below-out-dim": (Case("r", "bwd", 70, 40, 33, RELU, ldy=39), capi.FFH_ERR_BAD_ARG),
    "lddy-below-out-dim": (Case("r", "bwd", 70, 40, 33, RELU, lddy=39), capi.FFH_ERR_BAD_ARG),
    "lddx-below-in-dim": (Case("r", "bwd", 70, 40, 33, RELU, lddx=69), capi.FFH_ERR_BAD_ARG),
    "fwd-ldx-below-in-dim": (Case("r", "fwd", 70, 40, 33, RELU, ldx=69), capi.FFH_ERR_BAD_ARG),
    "fwd-ldy-below-out-dim": (Case("r", "fwd", 70, 40, 33, RELU, ldy=39), capi.FFH_ERR_BAD_ARG),
    "fwd-tanh": (Case("r", "fwd", 70, 40, 33, capi.AC_MODE_TANH), capi.FFH_ERR_UNSUPPORTED),
}


def bf16_edge_table(cus=TABLE_CUS):
    t = {}
    _bf16_table(t)
    return t


BF16_EDGE_NAMES = list(bf16_edge_table())


def draw_case_bf16(rng, name="random-bf16"):
    """draw_case with each width raised to at least 128 with probability one half, in tensor-op mode, a random subset of twins, a random distribution."""
    c = draw_case(rng, name)
    i = max(c.in_dim, BF16_MIN_DIM) if rng.random() < 0.5 else c.in_dim
    o = max(c.out_dim, BF16_MIN_DIM) if rng.random() < 0.5 else c.out_dim
    twins = [n for n in TWIN_NAMES if rng.random() < 0.5]
    dist = str(rng.choice(DISTS))
    if dist in ("integer", "wide") and c.act not in (NONE, RELU):
        dist = "uniform"
    return c.replace(in_dim=i, out_dim=o, ldx=i + c.ldx - c.in_dim, lddx=i + c.lddx - c.in_dim, ldy=o + c.ldy - c.out_dim, lddy=o + c.lddy - c.out_dim,
                     mode=MATH_BF16, twins=twins, dist=dist)


def draw_cases_bf16(seed, count=6):
    rng = np.random.default_rng(7000 + seed)
    return [draw_case_bf16(rng, f"bf16-seed{seed}.{k}") for k in range(count)]


# ---------------------------------------------------------------------------------------------------------------------------
# FFH_MATH_FP32_SPLIT_BF16X3_ALL: the edge table (shapes derived for 256 CUs from x3_gemm above), the random cases, the run with and without images
def _x3_table(t):
    M3 = dict(mode=MATH_SPLIT_ALL)
    P, U, WD = dict(dist="planes", **M3), dict(dist="uniform", **M3), dict(dist="wide", **M3)
    F, DWT, DXT, DXM = "linear_fwd gemm (bf16)|", "linear_bwd dw gemm (bf16)|", "linear_bwd dx gemm (bf16)|", "linear_bwd dx gemm (bf16, masking)|"
    W8, W4, S = "bf16x3_128x128|splitk=1|v2w8", "bf16x3_128x128|splitk=1|v2w4", "bf16x3_128x128|splitk="
    DMA, DMAI = "x3_dma_256x256_planes", "x3_dma_256x256_planes+image"
    DXO = ONLY_DX | OVERWRITE
    # gemm_bf16x3_v2_kernel on eight waves: at most 384 tiles of 128 x 128 (150 % of the CUs); batch 200 is two tile rows.  K = 136 and 200 are no
    # multiples of 32 (the guarded k-tile), 192 is; ragged M and N, every offset, padded rows
    t["x3-v2w8-fwd"] = [
        Case("x-w8-fwd-136->192", "fwd", 136, 192, 200, NONE, ldx=137, x_off=1, bias_off=1, want=F + W8, **P),
        Case("x-w8-fwd-192->200-relu", "fwd", 192, 200, 200, RELU, w_off=4, ldy=203, y_off=2, want=F + W8, **P),
        Case("x-w8-fwd-200->136-no-bias", "fwd", 200, 136, 200, RELU, bias=False, ldy=139, y_off=1, w_off=1, want=F + W8, **U),
        Case("x-w8-fwd-136->200-wide", "fwd", 136, 200, 129, NONE, bias_off=2, ldx=140, want=F + W8, **WD),
        Case("x-w8-fwd-192->136-int", "fwd", 192, 136, 200, NONE, dist="integer", want=F + W8, **M3)]
    # the data gradient stored, accumulated, masked by x; the masking form (a live ReLU under ONLY_DX reads dy through relu'(y)); beside a
    # weight gradient of batch <= 256 the search ends at one split and the launch runs two, the second one empty
    t["x3-v2w8-dx"] = [
        Case("x-w8-dx-store", "bwd", 192, 136, 200, NONE, DXO, lddy=137, dy_off=1, want=DXT + W8, **P),
        Case("x-w8-dx-add", "bwd", 200, 192, 200, NONE, ONLY_DX, lddx=203, dx_off=1, w_off=1, want=DXT + W8, **P),
        Case("x-w8-dx-mask-by-x", "bwd", 136, 200, 200, RELU, DXO | MASK_BY_X | PREMASKED, ldx=139, x_off=2, want=DXT + W8, **P),
        Case("x-w8-dx-add-mask-by-x", "bwd", 192, 136, 129, NONE, ONLY_DX | MASK_BY_X, want=DXT + W8, **U),
        Case("x-w8-dx-masking", "bwd", 136, 192, 200, RELU, DXO, ldy=195, y_off=2, want=DXM + W8, **P),
        Case("x-w8-dx-masking-add-maskx", "bwd", 200, 136, 77, RELU, ONLY_DX | MASK_BY_X, dx_off=1, want=DXM + W8, **U),
        Case("x-w8-both", "bwd", 192, 200, 200, NONE, OVERWRITE, want=(DWT + S + "2|mfma32", DXT + W8), **P),
        Case("x-w8-both-live-relu-forked", "bwd", 136, 192, 200, RELU, MASK_BY_X, forked=True, want=(DWT + S + "2|mfma32", DXT + W8), **P),
        Case("x-w8-both-sigmoid", "bwd", 200, 136, 131, SIG, 0, db=False, want=(DWT + S + "2|mfma32", DXT + W8), **U),
        Case("x-w8-dx-wide", "bwd", 257, 129, 130, NONE, 0, want=(DWT + S + "2|mfma32", DXT + W8), **WD)]
    # ... on four waves: more than 384 tiles: 384 wide is three tile columns, 16400 rows are 129 tile rows = 387 tiles; 16256 rows are 127 = 381
    t["x3-v2w4"] = [
        Case("x-w4-fwd-128->384", "fwd", 128, 384, 16400, RELU, bias_off=1, want=F + W4, **P),
        Case("x-w4-fwd-136->380", "fwd", 136, 380, 16400, NONE, bias=False, ldy=381, y_off=1, x_off=1, want=F + W4, **U),
        Case("x-w4-dx-store", "bwd", 384, 136, 16400, NONE, DXO, want=DXT + W4, **P),
        Case("x-w4-dx-add-mask-by-x", "bwd", 380, 128, 16400, RELU, ONLY_DX | MASK_BY_X | PREMASKED, lddx=381, dx_off=1, want=DXT + W4, **P),
        Case("x-w4-dx-masking", "bwd", 384, 136, 16400, RELU, DXO, want=DXM + W4, **U),
        Case("x-w4-fwd-381-tiles", "fwd", 128, 384, 16256, RELU, want=F + W8, **P)]
    # gemm_bf16x3_kernel, 128 x 128: 700 x (130 -> 129): 4 tiles, want 128 capped at cdiv(700, 256) = 3 splits of 256; 1100 x (257 -> 136): 6 tiles, 5
    # splits, the last one 76 deep; batch <= 256: the forced empty second split; with and without db
    t["x3-dw-128"] = [
        Case("x-dw-3-splits-db", "bwd", 130, 129, 700, NONE, ONLY_DW, lddy=131, dy_off=1, ldx=133, x_off=2, want=DWT + S + "3|mfma32", **P),
        Case("x-dw-3-splits-no-db", "bwd", 130, 129, 700, RELU, ONLY_DW | PREMASKED, db=False, want=DWT + S + "3|mfma32", **P),
        Case("x-dw-5-splits", "bwd", 257, 136, 1100, RELU, ONLY_DW, want=DWT + S + "5|mfma32", **U),
        Case("x-dw-no-dx", "bwd", 136, 130, 513, NONE, 0, dx=False, want=DWT + S + "3|mfma32", **WD),
        Case("x-dw-empty-second-split", "bwd", 129, 130, 70, NONE, ONLY_DW, want=DWT + S + "2|mfma32", **P),
        Case("x-dw-empty-second-split-256", "bwd", 192, 136, 256, NONE, ONLY_DW, db=False, want=DWT + S + "2|mfma32", **U),
        Case("x-dw-int", "bwd", 129, 192, 700, NONE, ONLY_DW, dist="integer", want=DWT + S + "3|mfma32", **M3)]
    # deterministic mode: one ordered split adding into dw
    t["x3-deterministic"] = [
        Case("x-det-700", "bwd", 130, 129, 700, NONE, ONLY_DW, det=True, lddy=131, dy_off=1, want=DWT + S + "1|mfma32", **P),
        Case("x-det-1100", "bwd", 257, 136, 1100, RELU, 0, det=True, want=(DWT + S + "1|mfma32", DXT + W8), **U),
        Case("x-det-images", "bwd", 192, 256, 16416, NONE, ONLY_DW, det=True, lddy=256, images=("x", "dy"), want=DWT + S + "1|mfma32", **P)]
    # ... 256 x 256 from 32 tiles and batch 8192 on: 770 x 1800 is 4 x 8 = 32 tiles, 8 splits fill one round; 770 x 1792 is 28 tiles; batch 8190
    t["x3-dw-256"] = [
        Case("x-dw-big", "bwd", 1800, 770, 8200, NONE, ONLY_DW, want=DWT + "bf16x3_256x256|splitk=8", **P),
        Case("x-dw-big-uniform", "bwd", 1800, 770, 8200, RELU, ONLY_DW | PREMASKED, db=False, want=DWT + "bf16x3_256x256|splitk=8", **U),
        Case("x-dw-big-28-tiles", "bwd", 1792, 770, 8200, NONE, ONLY_DW, db=False, want=DWT + S + "6|mfma32", **U)]
    # gemm_x3_dma_kernel, forward: images on x and w, from 192 tiles of 256 x 256 on (75 % of the CUs): 1000 wide is 4 tile columns, 12200 rows
    # are 48 tile rows (ragged); the image of y in place where its rows are a multiple of 32 apart, else by the conversion pass
    XW = ("x", "w", "y")
    t["x3-dma-fwd"] = [
        Case("x-dma-fwd-image", "fwd", 128, 1000, 12200, RELU, ldy=1024, images=XW, want=F + DMAI, **P),
        Case("x-dma-fwd-convert-pass", "fwd", 128, 1000, 12200, NONE, bias_off=4, images=XW, want=F + DMA + ";", **U),
        Case("x-dma-fwd-no-bias-no-y-image", "fwd", 160, 1000, 12200, NONE, bias=False, ldx=192, x_off=32, images=("x", "w"), want=F + DMA + ";", **P),
        Case("x-dma-fwd-188-tiles", "fwd", 128, 1000, 12032, RELU, ldy=1024, images=XW, want=F + W4, **P)]
    # ... data gradient: dy and w from their images (w's rows are in_dim apart: a multiple of 32), stored and accumulated, masked by x from x's
    # image and from the fp32 x
    BW = ("w", "dy", "dx")
    t["x3-dma-dx"] = [
        Case("x-dma-dx-store", "bwd", 992, 128, 12200, NONE, DXO, images=BW, want=DXT + DMAI, **P),
        Case("x-dma-dx-add-convert-pass", "bwd", 992, 128, 12200, RELU, ONLY_DX | PREMASKED, lddx=996, images=BW, want=DXT + DMA + ";", **U),
        Case("x-dma-dx-188-tiles", "bwd", 992, 128, 12032, NONE, DXO, images=BW, want=DXT + W4, **U)]
    t["x3-dma-dx-masked"] = [
        Case("x-dma-dx-mask-image", "bwd", 992, 128, 12200, NONE, DXO | MASK_BY_X, images=("x",) + BW, want=DXT + DMAI, **P),
        Case("x-dma-dx-mask-fp32", "bwd", 992, 128, 12200, NONE, ONLY_DX | MASK_BY_X, ldx=996, images=BW, want=DXT + DMAI, **U)]
    # ... weight gradient: 2 tiles (264 x 192) need 64 slices for 128 workgroups (half the CUs) of eight k-tiles of 32: batch 16384 (16416: nine
    # in some); 6 tiles (520 x 320) need 22 slices: batch 5632.  One round: through the stream's slots; without scratch by atomics
    DW2 = dict(images=("x", "dy"))
    t["x3-dma-dw"] = [
        Case("x-dma-dw-2-tiles-db", "bwd", 192, 264, 16416, NONE, ONLY_DW, lddy=288, want=DWT + DMA + "|slots", **DW2, **P),
        Case("x-dma-dw-2-tiles-no-db", "bwd", 192, 264, 16384, RELU, ONLY_DW | PREMASKED, lddy=288, db=False, want=DWT + DMA + "|slots", **DW2, **U),
        Case("x-dma-dw-2-tiles-atomics", "bwd", 192, 264, 16416, NONE, ONLY_DW, lddy=288, scratch=False, want=DWT + DMA + ";", **DW2, **P),
        Case("x-dma-dw-6-tiles", "bwd", 320, 520, 5632, NONE, ONLY_DW, lddy=544, db=False, want=DWT + DMA + "|slots", **DW2, **P),
        Case("x-dma-dw-6-tiles-atomics", "bwd", 320, 520, 5632, NONE, ONLY_DW, lddy=544, scratch=False, want=DWT + DMA + ";", **DW2, **U),
        Case("x-dma-dw-no-split-fits", "bwd", 192, 264, 16352, NONE, ONLY_DW, lddy=288, want=DWT + S + "64|mfma32", **DW2, **P),
        Case("x-dma-dw-one-tile", "bwd", 192, 192, 16416, NONE, ONLY_DW, db=False, want=DWT + S, **DW2, **U)]
    # images registered, the LDS-DMA kernel declines (every shape is one it serves otherwise): the split-in-kernel form runs and the output's
    # image is written all the same; y off the group grid is served, its image written by the conversion pass
    t["x3-dma-declined-operands"] = [
        Case("x-nd-x-off", "fwd", 128, 1000, 12200, RELU, ldx=160, x_off=8, ldy=1024, images=XW, want=F + W4, **P),
        Case("x-nd-ldx", "fwd", 128, 1000, 12200, NONE, ldx=132, images=XW, want=F + W4, **U),
        Case("x-nd-one-operand", "fwd", 128, 1000, 12200, NONE, ldy=1024, images=("x", "y"), want=F + W4, **U)]
    t["x3-dma-declined-shape"] = [
        Case("x-nd-k", "fwd", 136, 1000, 12200, NONE, ldx=160, ldy=1024, images=XW, want=F + W4, **P),
        Case("x-nd-n", "fwd", 128, 1004, 12200, RELU, ldy=1024, images=XW, want=F + W4, **U)]
    t["x3-dma-image-by-the-conversion-pass"] = [
        Case("x-nd-y-off-grid", "fwd", 128, 1000, 12200, RELU, ldy=1024, y_off=4, images=XW, want=F + DMA + ";", **P),
        Case("x-nd-ldy", "fwd", 128, 1000, 12200, NONE, ldy=1004, y_off=32, images=XW, want=F + DMA + ";", **U)]
    t["x3-dma-declined-live-activation"] = [
        Case("x-nd-live-relu-masking", "bwd", 992, 128, 12200, RELU, DXO, images=BW, stale=("dy",), want=DXM + W4, **P),
        Case("x-nd-live-sigmoid", "bwd", 992, 128, 12200, SIG, DXO, images=BW, stale=("dy",), want=DXT + W4, **U),
        Case("x-nd-live-relu-dw", "bwd", 192, 264, 16416, RELU, OVERWRITE, lddy=288, images=("x", "w", "dy", "dx"), stale=("dy",), want=(DWT + S + "65|mfma32", DXT + W8), **P)]
    # narrow layers keep the fp32 kernels: no image is written (the one-launch backward of out_dim <= 16 refreshes dx's by the conversion pass:
    # allowed, not required), and "planes" is held to the bound against the unsplit product there
    t["x3-narrow-layers"] = [
        Case("x-narrow-in127", "fwd", 127, 256, 300, RELU, images=XW, want="linear_fwd gemm|f32_", **U),
        Case("x-narrow-out127", "fwd", 256, 127, 300, NONE, images=XW, want="linear_fwd gemm|f32_", **P),
        Case("x-narrow-bwd-in127", "bwd", 127, 256, 300, RELU, OVERWRITE, images=("x", "w", "dy", "dx"), want=("linear_bwd dw gemm|f32_", "linear_bwd dx gemm|f32_"), **U),
        Case("x-narrow-bwd-out127", "bwd", 256, 127, 300, NONE, 0, images=("x", "w", "dy", "dx"), want=("linear_bwd dw gemm|f32_", "linear_bwd dx gemm|f32_"), **WD),
        Case("x-narrow-skinny-fwd", "fwd", 256, 4, 300, SIG, images=XW, want="linear_fwd|skinny", **U),
        Case("x-narrow-skinny-bwd", "bwd", 256, 1, 4100, SIG, OVERWRITE | MASK_BY_X, images=("x", "w", "dy", "dx"), want="linear_bwd|skinny", **U)]


def x3_edge_table(cus=TABLE_CUS):
    t = {}
    _x3_table(t)
    return t


X3_EDGE_NAMES = list(x3_edge_table())
# kernel (as the issue lists them) -> a substring of the tokens that name it
X3_KERNELS = {"gemm_bf16x3_kernel 128 x 128": "|mfma32", "gemm_bf16x3_kernel 256 x 256": "bf16x3_256x256", "gemm_bf16x3_v2_kernel, four waves": "|v2w4",
              "gemm_bf16x3_v2_kernel, eight waves": "|v2w8", "gemm_x3_dma_kernel forward": "linear_fwd gemm (bf16)|x3_dma_256x256_planes",
              "gemm_x3_dma_kernel data gradient": "linear_bwd dx gemm (bf16)|x3_dma_256x256_planes",
              "gemm_x3_dma_kernel weight gradient": "linear_bwd dw gemm (bf16)|x3_dma_256x256_planes", "x3_dw_reduce_kernel": "x3_dma_256x256_planes|slots"}


def draw_case_x3(rng, name="random-x3"):
    """draw_case with each width raised to at least 128 with probability three quarters, in the split mode, a random subset of images, a random
    distribution."""
    c = draw_case(rng, name)
    i = max(c.in_dim, BF16_MIN_DIM) if rng.random() < 0.75 else c.in_dim
    o = max(c.out_dim, BF16_MIN_DIM) if rng.random() < 0.75 else c.out_dim
    images = [] if rng.random() < 0.2 else [n for n in IMAGE_NAMES if rng.random() < 0.5]
    dist = str(rng.choice(["uniform", "integer", "wide", "planes", "planes"]))
    if dist != "uniform" and c.act not in (NONE, RELU):
        dist = "uniform"
    return c.replace(in_dim=i, out_dim=o, ldx=i + c.ldx - c.in_dim, lddx=i + c.lddx - c.in_dim, ldy=o + c.ldy - c.out_dim, lddy=o + c.lddy - c.out_dim,
                     mode=MATH_SPLIT_ALL, images=images, dist=dist)


def draw_cases_x3(seed, count=6):
    rng = np.random.default_rng(9000 + seed)
    return [draw_case_x3(rng, f"x3-seed{seed}.{k}") for k in range(count)]


def run_and_check_x3(lib, be, case, cus=None, routes=True):
    """run_and_check; where the case has images and its y or dx came from a kernel of the split mode, the same case once more without images: the
    header promises the same bits in y and dx (the weight gradient is held to its bound, or to equality, in both runs)."""
    res, rep = run_and_check(lib, be, case, cus, routes)
    split_out = [n for n, tok in (("y", res.route if case.kind == "fwd" else ""),) + tuple(("dx", t) for t in res.route.split(";") if "dx" in t.split("|")[0])
                 if "bf16x3" in tok or "x3_dma" in tok]
    if case.images and rep.ok() and split_out:
        c2 = case.replace(images=(), stale=(), want=())
        bare = (run_fwd if case.kind == "fwd" else run_bwd)(lib, be, c2, res.inp)
        same = True
        for name in split_out:
            a, b = dict(res.outputs).get(name), dict(bare.outputs).get(name)
            if a is not None and a.host.tobytes() != b.host.tobytes():
                same = False
                rep.violations.append(f"{name}: differs between the run with images ({res.route}) and the run without ({bare.route})")
        # y and dx equal, whole buffers, to what was just checked: numbers and sentinels are checked with that; anything else the call writes
        # (a weight or bias gradient, dy and db under a live activation) is checked again, and so is the route
        final_dy = case.has(PREMASKED) or case.act == NONE
        if same and (case.kind == "fwd" or (case.has(ONLY_DX) and final_dy)) and bare.rc == capi.FFH_OK:
            rep2 = Report()
            _buffers(rep2, bare)
            if case.kind == "bwd" and not all(b.untouched() for n, b in bare.outputs if n in ("dw", "db")):
                rep2.violations.append("dw / db: written under ONLY_DX")
        else:
            rep2 = check_fwd(bare) if case.kind == "fwd" else check_bwd(bare)
        if be.is_hip and routes and bare.rc == capi.FFH_OK and case.batch > 0:
            rep2.violations += check_route(bare, cus)
        rep.violations += [f"without images: {v}" for v in rep2.violations]
    return res, rep


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points of the split mode in numpy, the arithmetic a parameter: what tests/test_linear_x3_sweep_cpu.py feeds the checker
class NumpySplitLib:
    """ffh_linear_fwd / ffh_linear_bwd_ex on host memory as include/ff_hip.h states them, a layer of the split mode summed by split_product(pairs,
    rnd) and rounded to fp32 once, every other layer in float64; images registered with ffh_ctx_bf16x3_mirror_set are kept as the header says
    (write_images False: an output's image is left alone).  Only what run_fwd / run_bwd call."""

    def __init__(self, pairs=SIX, rnd=None, write_images=True):
        self.lib, self.ctx, self.pairs, self.rnd, self.write_images = self, None, pairs, rnd, write_images
        self.mode, self.regions = 0, {}

    def check(self, rc, what=""):
        assert rc == capi.FFH_OK, what

    @staticmethod
    def _view(ptr, rows, cols, ld):
        if ptr is None or rows * cols == 0:
            return None
        flat = np.ctypeslib.as_array((C.c_float * ((rows - 1) * ld + cols)).from_address(int(ptr)))
        return np.lib.stride_tricks.as_strided(flat, (rows, cols), (4 * ld, 4))

    def _image(self, ptr, rows, cols, ld, rnd=None):
        """Write the planes of the [rows][cols] block at ptr into the image of the region that holds it; False: no such region."""
        ptr = int(ptr)
        for base, (nbytes, img) in self.regions.items():
            if base <= ptr and ptr + 4 * ((rows - 1) * ld + cols) <= base + nbytes:
                e = ((ptr - base) // 4 + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).ravel()
                planes = np.ctypeslib.as_array((C.c_uint16 * image_len(nbytes // 4)).from_address(img))
                planes[image_at(e)[None, :] + 32 * np.arange(3)[:, None]] = plane_bits(self._view(ptr, rows, cols, ld), rnd)
                return True
        return False

    def _prod(self, a, b, split):
        if split:
            return split_product(np.asarray(a, np.float32), np.asarray(b, np.float32), self.pairs, self.rnd)
        return _f64(a) @ _f64(b)

    def ffh_ctx_set_math_mode(self, ctx, mode):
        self.mode = mode
        return 0

    def ffh_ctx_set_deterministic(self, ctx, on):
        return 0

    def ffh_stream_create(self, ctx, ref):
        return 0

    def ffh_stream_sync(self, ctx, s):
        return 0

    def ffh_linear_last_route(self, ctx):
        return b""

    def ffh_linear_dx_scatter_used(self, ctx):
        return 0

    def ffh_linear_dx_colsum_used(self, ctx):
        return 0

    def ffh_ctx_bf16x3_mirror_set(self, ctx, base, nbytes, img):
        if img is None:
            self.regions.pop(int(base), None)
        else:
            self.regions[int(base)] = (int(nbytes), int(img))
        return 0

    def ffh_convert_f32_to_bf16x3(self, ctx, src, rows, cols, ld, s):
        return 0 if self._image(src, rows, cols, ld) else capi.FFH_ERR_BAD_ARG          # (the explicit conversion is not the mutant)

    def _split(self, i, o):
        return self.mode == MATH_SPLIT_ALL and i >= BF16_MIN_DIM and o >= BF16_MIN_DIM

    def ffh_linear_fwd(self, ctx, x, ldx, y, ldy, w, bias, i, o, B, act, s):
        if B == 0:
            return 0
        X, W, Y = self._view(x, B, i, ldx), self._view(w, o, i, i), self._view(y, B, o, ldy)
        b = _f64(self._view(bias, 1, o, o)[0]) if bias else 0.0
        Y[:] = act64(self._prod(X, W.T, self._split(i, o)) + b, act).astype(np.float32)
        if self._split(i, o) and self.write_images:
            self._image(y, B, o, ldy, self.rnd)
        return 0

    def ffh_linear_bwd_ex(self, ctx, x, ldx, dx, lddx, y, ldy, dy, lddy, w, dw, db, i, o, B, act, flags, s, s_dw):
        if B == 0:
            return 0
        X, W, Y, G = self._view(x, B, i, ldx), self._view(w, o, i, i), self._view(y, B, o, ldy), self._view(dy, B, o, lddy)
        only_dx, only_dw, split = bool(flags & ONLY_DX), bool(flags & ONLY_DW), self._split(i, o)
        act = NONE if flags & PREMASKED else act
        eff = G
        if act == RELU:
            eff = np.where(Y > 0, G, np.float32(0))
            if not only_dx:
                G[:] = eff
        elif act == SIG and not only_dw:
            eff = (_f64(G) * _f64(Y) * (1.0 - _f64(Y))).astype(np.float32)
            G[:] = eff
        if not only_dx:
            DW = self._view(dw, o, i, i)
            DW[:] = (_f64(DW) + self._prod(eff.T, X, split)).astype(np.float32)
        if db and not (only_dw if act == SIG else only_dx):
            DB = self._view(db, 1, o, o)
            DB[0] = (_f64(DB[0]) + _f64(eff).sum(0)).astype(np.float32)
        if dx and not only_dw:
            DX = self._view(dx, B, i, lddx)
            v = self._prod(eff, W, split)
            if flags & MASK_BY_X:
                v = np.where(X > 0, v, 0.0)
            if not flags & OVERWRITE:
                v = v + _f64(DX)
            DX[:] = v.astype(np.float32)
            if split and self.write_images:
                self._image(dx, B, i, lddx, self.rnd)
        return 0
