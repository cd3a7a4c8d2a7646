"""The grid-capped streaming kernels past their caps: the cap table, the trips model, the references and the checker.

Every memory-bound kernel of the library launches ffh_grid(work, per_block, cap) workgroups of 256 threads (csrc/ffh_common.h) and walks the
rest in a grid-stride loop.  TABLE restates, per entry point, the per_block and cap literals of that call and how `work` follows from the
arguments (the vector width the launcher picks included); trips() is ceil(work / (256 * blocks)).  CASES holds, per entry, shapes that make
exactly one full trip (`at`), a second trip (`past`) and three or more (`deep`).  tests/test_stream_cap_cpu.py compares the table with the
source text and proves the generators, references and the checker without a GPU; tests/test_gpu_stream_cap.py runs the cases on the device.

A case runs through a Backend: the product library on the GPU, or the CPU oracle (plus small numpy stand-ins for the entries the oracle
does not export).  Every output and in-place buffer sits inside an allocation with sentinels in front, behind and in pad columns; the
checker compares WHOLE allocations, so an element written twice (an accumulate done two times, a sentinel overwritten) and an element
never written both show, and it names the first bad index."""
import ctypes as C
import os
import re
from collections import namedtuple

import numpy as np
import torch

import bf16_helpers as BH
from dlrm_flexflow_amd import capi, ffmodel

THREADS = 256
G = THREADS * 2048          # threads of a default-cap grid
EPS32 = float(np.finfo(np.float32).eps)
CSRC = os.path.join(capi.REPO_ROOT, "dlrm_flexflow_amd", "csrc")
SENT32 = 0x7FC0BEEF          # a quiet NaN no arithmetic produces
SENT16 = 0xDEAD
SENT64 = -0x5EA75EA75EA75EA7
FRONT = BACK = 64            # elements of sentinel in front of / behind a payload (64 floats: the payload keeps a 256-byte alignment)


def ceil_div(a, b):
    return -(-a // b)


# =====================================================================================================================================
# 1. the cap table and the trips model
# =====================================================================================================================================
# file: under csrc/; func: the host function whose body holds the launch; kernel: a word on the line of the ffh_grid( call that tells it from
# the function's other launches (None: the function's only call); work(args): the first argument of ffh_grid for a case's arguments, which
# the source spells as one of WORK_EXPR[file, func].
# The two gathers size their grids in ROWS: per_block(args) rows per workgroup and trip, at most cap(args) workgroups per table (see GATHER_*).
Row = namedtuple("Row", "file func kernel per_block cap work")
GATHER_CAP, GATHER_U = 1024, 4          # FFH_EMB_FWD_CAP's default, over all tables; rows in flight per lane group (emb_fwd_launch)


def gather_block_rows(a):
    """RowLanes(D, vec).block_rows(U) of embedding_fwd.hip: 4 waves x rows per wave x U"""
    nvec = a["D"] // (4 if a["D"] % 4 == 0 else 1)
    return 4 * (64 // min(nvec, 64)) * GATHER_U


def _num(v, a):
    return v(a) if callable(v) else v


def _vec_n(a):          # the dense optimizers and sum_slices: n / 4 in the 16-byte form
    return a["n"] // 4 if a.get("vec", True) else a["n"]


def _cross_work(a):
    return a["batch"] * (a["dim"] if a.get("scalar") else a["dim"] // 4)


def _digest_work(a):
    return a["rows"] * (ceil_div(a["row_bytes"], 16) if a["lw"] == 16 else ceil_div(a["row_bytes"], 8))


def _x3_work(a):
    return a["rows"] * (a["cols"] if a.get("scalar") else a["cols"] // 4)


def _vol(a):
    return int(np.prod(a["dims"]))


def _tril_work(a):
    return a["batch"] * (a["n"] * (a["n"] - 1) // 2)


def _concat_work(a):
    return a["rows"] * ceil_div(max(a["widths"]), 4)


TABLE = {
    "ffh_cross_fwd": Row("cross.hip", "make_walk", None, 256, 2048, _cross_work),
    "ffh_cross_bwd": Row("cross.hip", "make_walk", None, 256, 2048, _cross_work),
    "ffh_sgd_update_ex": Row("elementwise.hip", "sgd_update_impl", "(sgd_kernel<{V}>)", 256, 2048, _vec_n),
    "ffh_sgd_update_ex_lr": Row("elementwise.hip", "sgd_update_impl", "(sgd_lr_kernel<{V}>)", 256, 2048, _vec_n),
    "ffh_adam_update": Row("elementwise.hip", "adam_update_impl", "(adam_kernel<{V}>)", 256, 2048, _vec_n),
    "ffh_adam_update_lr": Row("elementwise.hip", "adam_update_impl", "(adam_lr_kernel<{V}>)", 256, 2048, _vec_n),
    "ffh_adagrad_update": Row("elementwise.hip", "adagrad_update_impl", None, 256, 2048, _vec_n),
    "ffh_adagrad_update_lr": Row("elementwise.hip", "adagrad_update_impl", None, 256, 2048, _vec_n),
    "ffh_mse_bwd": Row("elementwise.hip", "ffh_mse_bwd", None, 256, 2048, lambda a: a["n"]),
    "ffh_add_scaled": Row("elementwise.hip", "ffh_add_scaled", None, 256, 2048, lambda a: a["n"]),
    "ffh_sum_slices_f32": Row("elementwise.hip", "ffh_sum_slices_f32", None, 256, 2048, _vec_n),
    "ffh_metrics_update": Row("elementwise.hip", "ffh_metrics_update", None, 256, 256, lambda a: a["ns"]),
    "ffh_mse_bwd_metrics": Row("elementwise.hip", "ffh_mse_bwd_metrics", None, 256, 256, lambda a: a["ns"]),
    "ffh_bce_bwd_metrics": Row("ctr.hip", "ffh_bce_bwd_metrics", None, 256, 256, lambda a: a["ns"]),
    "ffh_ctr_eval_update": Row("ctr.hip", "ffh_ctr_eval_update", None, 256, 256, lambda a: a["ns"]),
    "ffh_transpose_fwd": Row("elementwise.hip", "transpose_launch", "(transpose_generic_kernel<false>)", 256, 2048, _vol),
    "ffh_transpose_bwd": Row("elementwise.hip", "transpose_launch", "(transpose_generic_kernel<true>)", 256, 2048, _vol),
    "ffh_concat_fwd": Row("elementwise.hip", "concat_impl", None, 256, 1024, _concat_work),
    "ffh_concat_bwd": Row("elementwise.hip", "concat_impl", None, 256, 1024, _concat_work),
    "ffh_concat_bwd_ex": Row("elementwise.hip", "concat_impl", None, 256, 1024, _concat_work),
    "ffh_tril_fwd": Row("elementwise.hip", "ffh_tril_fwd", None, 1024, 4096, _tril_work),
    "ffh_tril_bwd": Row("elementwise.hip", "ffh_tril_bwd", None, 1024, 4096, _tril_work),
    "ffh_embedding_bwd_dense": Row("embedding.hip", "ffh_embedding_bwd_dense", None, 256, 4096, lambda a: a["batch"] * a["D"]),
    "ffh_embedding_localize_rows": Row("embedding.hip", "ffh_embedding_localize_rows", None, 256, 2048, lambda a: a["n"]),
    "ffh_convert_f32_to_bf16": Row("runtime.hip", "ffh_convert_f32_to_bf16", None, 256, 2048, lambda a: ceil_div(a["n"], 4)),
    "ffh_convert_f32_to_bf16x3": Row("runtime.hip", "ffh_convert_f32_to_bf16x3", None, 256, 2048, _x3_work),
    # an unaligned base takes the generator kernel, one element per thread
    "ffh_fill_f32": Row("runtime.hip", "ffh_fill_f32", "fill_f32_kernel", 256, 2048, lambda a: ceil_div(a["n"], 4)),
    "ffh_fill_f32/unaligned": Row("runtime.hip", "ffh_fill_f32", "(gen_f32_kernel<0>)", 256, 2048, lambda a: a["n"]),
    "ffh_init_uniform": Row("runtime.hip", "ffh_init_uniform", None, 256, 8192, lambda a: a["n"]),
    "ffh_init_uniform_bf16": Row("embedding.hip", "ffh_init_uniform_bf16", None, 256, 8192, lambda a: a["n"]),
    "ffh_embedding_fwd_multi": Row("embedding_fwd.hip", "emb_fwd_launch", None, gather_block_rows, lambda a: GATHER_CAP // a["nt"], lambda a: a["batch"]),
    "ffh_embedding_fwd_multi_bf16": Row("embedding_fwd.hip", "emb_fwd_launch", None, gather_block_rows, lambda a: GATHER_CAP // a["nt"], lambda a: a["batch"]),
    "ffh_gen_indices": Row("runtime.hip", "ffh_gen_indices", None, 256, 2048, lambda a: a["n"]),
    "ffh_gen_uniform01": Row("runtime.hip", "ffh_gen_uniform01", None, 256, 2048, lambda a: a["n"]),
    "ffh_gen_bernoulli": Row("runtime.hip", "ffh_gen_bernoulli", None, 256, 2048, lambda a: a["n"]),
    "ffh_state_digest": Row("digest.hip", "ffh_state_digest", None, 256, 2048, _digest_work),
}


# the first argument of the launchers' ffh_grid( calls as the source spells it (what Row.work restates)
WORK_EXPR = {
    ("cross.hip", "make_walk"): {"batch * w.groups"},
    ("digest.hip", "ffh_state_digest"): {"rows * w.groups"},
    ("elementwise.hip", "sgd_update_impl"): {"n / 4", "n"},
    ("elementwise.hip", "adam_update_impl"): {"n / 4", "n"},
    ("elementwise.hip", "adagrad_update_impl"): {"vec ? n / 4 : n"},
    ("elementwise.hip", "ffh_sum_slices_f32"): {"vec ? n / 4 : n"},
    ("elementwise.hip", "ffh_mse_bwd"): {"n"},
    ("elementwise.hip", "ffh_add_scaled"): {"n"},
    ("elementwise.hip", "ffh_metrics_update"): {"ns"},
    ("elementwise.hip", "ffh_mse_bwd_metrics"): {"ns"},
    ("ctr.hip", "ffh_bce_bwd_metrics"): {"ns"},
    ("ctr.hip", "ffh_ctr_eval_update"): {"ns"},
    ("elementwise.hip", "transpose_launch"): {"vol"},
    ("elementwise.hip", "concat_impl"): {"nblk * ((maxw + 3) / 4)"},
    ("elementwise.hip", "ffh_tril_fwd"): {"batch * ((int64_t)n * (n - 1) / 2)"},
    ("elementwise.hip", "ffh_tril_bwd"): {"batch * ((int64_t)n * (n - 1) / 2)"},
    ("embedding.hip", "ffh_embedding_bwd_dense"): {"batch * D"},
    ("embedding.hip", "ffh_embedding_localize_rows"): {"n"},
    ("embedding.hip", "ffh_init_uniform_bf16"): {"n"},
    ("runtime.hip", "ffh_convert_f32_to_bf16"): {"(n + 3) / 4"},
    ("runtime.hip", "ffh_convert_f32_to_bf16x3"): {"work"},          # vec ? rows * (cols / 4) : rows * cols, the line above the launch
    ("runtime.hip", "ffh_fill_f32"): {"(n + 3) / 4", "n"},
    ("runtime.hip", "ffh_init_uniform"): {"n"},
    ("runtime.hip", "ffh_gen_indices"): {"n"},
    ("runtime.hip", "ffh_gen_uniform01"): {"n"},
    ("runtime.hip", "ffh_gen_bernoulli"): {"n"},
}


def row_of(case):
    return TABLE[case.args.get("row", case.entry)]


def work_of(case):
    return int(row_of(case).work(case.args))


def per_block_of(case):
    return int(_num(row_of(case).per_block, case.args))


def cap_of(case):
    return int(_num(row_of(case).cap, case.args))


def unit_of(case):
    """work items of one workgroup in one trip: its 256 threads, or the gathers' rows per workgroup"""
    return per_block_of(case) if callable(row_of(case).per_block) else THREADS


def blocks_of(case):
    return max(1, min(ceil_div(work_of(case), per_block_of(case)), cap_of(case)))


def trips(entry, case):
    """ceil(work / (256 * blocks)): how often the busiest thread of `entry`'s kernel runs its loop body for `case`"""
    assert case.entry == entry
    return ceil_div(work_of(case), unit_of(case) * blocks_of(case))


def assert_trips(case):
    """Every case asserts the trip count it was written for before it launches.  `at`: the grid exactly at its cap and every trip full;
    `past`: one trip more, `deep`: two or more trips more.  With per_block = 256 (every entry but the tril pair, whose workgroups take
    1024 items, four trips, by design) that is 1, 2 and >= 3 trips."""
    t, w, b, pb, u = trips(case.entry, case), work_of(case), blocks_of(case), per_block_of(case), unit_of(case)
    base = pb // u
    assert b == cap_of(case), (case, b)
    if case.name == "at":
        assert t == base and w == pb * b, (case, t, w, b)
    elif case.name == "past":
        assert t == base + 1, (case, t)
    else:
        assert case.name == "deep" and t >= base + 2, (case, t)
    if case.name != "at" and case.args.get("ragged", True):
        assert w % (u * b) % u != 0, (case, "the last trip ends on a full workgroup")
    return t


def _balanced_args(text, at):
    """the arguments of the call whose opening parenthesis is text[at]"""
    assert text[at] == "("
    depth, args, cur = 0, [], ""
    for ch in text[at:]:
        if ch == "(":
            depth += 1
            if depth == 1:
                continue
        elif ch == ")":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args
        if ch == "," and depth == 1:
            args.append(cur.strip()); cur = ""
        else:
            cur += ch
    raise ValueError("unbalanced call")


def source_grid(row, vec_forms=("4", "1")):
    """[(work expression, per_block, cap)] of the ffh_grid( calls of row's launcher, read from the source text"""
    text = open(os.path.join(CSRC, row.file)).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (\w+) = (\d+);", text)}
    m = re.search(r"^[^\n/]*\b%s\s*\([^;{]*\)\s*\{" % re.escape(row.func), text, re.M)
    assert m, f"{row.func} not found in {row.file}"
    body = text[m.end():text.index("\n}", m.end())]
    wanted = [None] if row.kernel is None else sorted({row.kernel.replace("{V}", v) for v in vec_forms})
    out = []
    for word in wanted:
        lines = [ln for ln in body.split("\n") if "ffh_grid(" in ln and (word is None or word in ln)]
        assert lines, f"no ffh_grid( call with {word} in {row.func} ({row.file})"
        for ln in lines:
            a = _balanced_args(ln, ln.index("ffh_grid(") + len("ffh_grid"))
            per_block = consts[a[1]] if a[1] in consts else int(a[1])
            cap = int(a[2]) if len(a) > 2 else 2048
            out.append((a[0], per_block, cap))
    return out


# =====================================================================================================================================
# 2. the cases
# =====================================================================================================================================
Case = namedtuple("Case", "entry name args")
CASES = []


def case(entry, name, **args):
    CASES.append(Case(entry, name, args))


def case_id(c):
    return c.entry + "-" + c.name + "-" + "-".join(f"{k}{v}" for k, v in c.args.items() if k not in ("row", "ragged", "vec")).replace(" ", "")


for _e in ("ffh_cross_fwd", "ffh_cross_bwd"):
    case(_e, "at", batch=512, dim=4096)
    case(_e, "past", batch=607, dim=3456)                # 524,448 groups: step_r 606, step_c 704, the carry from column group 160 on
    # ... where the carry is taken only by threads that then leave the batch (row 607).  99 groups per row: step_r 5295, step_c 83, and the
    # second trip's 115 threads from 16 on carry INTO the last row: a carry that lands a row too far leaves that row's head unwritten, one
    # that stays a row behind revisits elements (which a store hides and the backward's ADD shows)
    case(_e, "past", batch=5297, dim=396)
    case(_e, "deep", batch=1300, dim=3456)
    case(_e, "deep", batch=2, dim=2097160)               # one row is longer than the whole grid: step_r 0
    case(_e, "deep", batch=607, dim=3456, scalar=True)   # the second operand based 4 bytes off
for _e in ("ffh_sgd_update_ex", "ffh_adam_update", "ffh_adagrad_update", "ffh_sgd_update_ex_lr", "ffh_adam_update_lr", "ffh_adagrad_update_lr"):
    case(_e, "at", n=4 * G)
    case(_e, "past", n=4 * G + 4 * 77)
    case(_e, "deep", n=3 * (4 * G) + 4 * 77)
    case(_e, "past", n=G + 301, vec=False)
for _e in ("ffh_sgd_update_ex", "ffh_adam_update", "ffh_adagrad_update"):
    case(_e, "past", n=4 * G + 4 * 77, mirror="twin")
    case(_e, "past", n=4 * G + 4 * 77, mirror="x3")
for _e in ("ffh_mse_bwd", "ffh_add_scaled", "ffh_embedding_localize_rows", "ffh_gen_indices", "ffh_gen_uniform01", "ffh_gen_bernoulli"):
    case(_e, "at", n=G)
    case(_e, "past", n=G + 301)
    case(_e, "deep", n=2 * G + 301)
case("ffh_sum_slices_f32", "at", n=4 * G)
case("ffh_sum_slices_f32", "past", n=4 * G + 4 * 77)
case("ffh_sum_slices_f32", "deep", n=2 * (4 * G) + 4 * 77)
case("ffh_sum_slices_f32", "past", n=G + 301, vec=False)
for _e in ("ffh_metrics_update", "ffh_mse_bwd_metrics", "ffh_bce_bwd_metrics", "ffh_ctr_eval_update"):
    case(_e, "at", ns=65536)
    case(_e, "past", ns=65536 + 301)
    case(_e, "deep", ns=200003)
for _e in ("ffh_transpose_fwd", "ffh_transpose_bwd"):
    case(_e, "at", dims=(2, 512, 512), perm=(2, 0, 1))
    case(_e, "past", dims=(3, 419, 421), perm=(2, 0, 1))
    case(_e, "past", dims=(65536, 3, 3), perm=(0, 2, 1), ragged=False)   # batch > 65,535: the tiled form declines
    case(_e, "deep", dims=(3, 701, 751), perm=(2, 0, 1))
for _e in ("ffh_concat_fwd", "ffh_concat_bwd", "ffh_concat_bwd_ex"):
    case(_e, "at", rows=2048, widths=(512, 8, 64, 5))
    case(_e, "past", rows=2049, widths=(513, 8, 64, 5))              # 129 groups, the last of one element: 264,321 items
    case(_e, "deep", rows=4100, widths=(513, 8, 64, 5))
for _e in ("ffh_tril_fwd", "ffh_tril_bwd"):
    case(_e, "at", n=2, batch=4096 * 1024)
    case(_e, "past", n=64, batch=2081)                              # 4,195,296 kept entries
    case(_e, "deep", n=64, batch=2601)
case("ffh_embedding_bwd_dense", "at", batch=8192, D=128)
case("ffh_embedding_bwd_dense", "past", batch=8257, D=127)
case("ffh_embedding_bwd_dense", "deep", batch=16400, D=128, ragged=False)   # the third trip is eight full workgroups
case("ffh_embedding_bwd_dense", "deep", batch=16515, D=127)
case("ffh_convert_f32_to_bf16", "at", n=4 * G)
case("ffh_convert_f32_to_bf16", "past", n=4 * G + 4 * 33 + 3)
case("ffh_convert_f32_to_bf16", "past", n=4 * G + 4 * 33 + 3, off=1)   # source and destination each one element off
case("ffh_convert_f32_to_bf16", "deep", n=2 * (4 * G) + 4 * 33 + 3)
case("ffh_convert_f32_to_bf16x3", "at", rows=1024, cols=2048, ld=2080)
case("ffh_convert_f32_to_bf16x3", "past", rows=1025, cols=2052, ld=2080)
case("ffh_convert_f32_to_bf16x3", "deep", rows=1025, cols=2052, ld=2080, scalar=True)   # the same sub-matrix from region element 5
case("ffh_convert_f32_to_bf16x3", "deep", rows=2500, cols=2052, ld=2080)
case("ffh_fill_f32", "at", n=4 * G)
case("ffh_fill_f32", "past", n=4 * G + 3)
case("ffh_fill_f32", "deep", n=2 * (4 * G) + 7)
case("ffh_fill_f32", "past", n=G + 301, off=1, row="ffh_fill_f32/unaligned")
case("ffh_init_uniform", "at", n=4 * G)
case("ffh_init_uniform", "past", n=4 * G + 301)
case("ffh_init_uniform", "deep", n=2 * (4 * G) + 301)
for _e in ("ffh_embedding_fwd_multi", "ffh_embedding_fwd_multi_bf16"):
    case(_e, "at", nt=64, D=128, batch=512)
    case(_e, "past", nt=64, D=128, batch=1000)          # 16 workgroups per table at 32 rows each: 2 trips with a ragged last block
    case(_e, "deep", nt=64, D=128, batch=1100)
    case(_e, "past", nt=64, D=3, batch=6000)            # the scalar form: 21 rows per wave and an idle lane
case("ffh_init_uniform_bf16", "at", n=4 * G)
case("ffh_init_uniform_bf16", "past", n=4 * G + 301)
case("ffh_init_uniform_bf16", "deep", n=2 * (4 * G) + 301)
case("ffh_state_digest", "at", rows=512, row_bytes=16 * 1024, lw=16)
case("ffh_state_digest", "past", rows=3, row_bytes=16 * 174863 - 6, lw=16)      # 3 x 174,863 = 524,288 + 301 groups
case("ffh_state_digest", "past", rows=3, row_bytes=8 * 174863 - 2, lw=4)
case("ffh_state_digest", "deep", rows=9, row_bytes=16 * 174863 - 6, lw=16)
case("ffh_state_digest", "deep", rows=9, row_bytes=8 * 174863 - 2, lw=4)


# =====================================================================================================================================
# 3. the checker
# =====================================================================================================================================
def sentinels(dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.full(n, SENT32, np.uint32).view(np.float32)
    if dtype.itemsize == 2:
        return np.full(n, SENT16, np.uint16).view(dtype)
    if dtype.itemsize == 8:
        return np.full(n, SENT64, np.int64).view(dtype)
    return np.full(n, 0xA5, np.uint8).view(dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check(what, got, exp):
    """Whole allocations, bit for bit.  Where the arithmetic itself makes a NaN the positions must agree and the payload is not compared
    (IEEE 754 leaves it to the implementation); a sentinel is compared in all its bits.  Names the first bad index."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.size == exp.size, f"{what}: {got.dtype}[{got.size}] against {exp.dtype}[{exp.size}]"
    gb, eb = _bits(got), _bits(exp)
    bad = gb != eb
    if got.dtype == np.float32:
        bad &= ~(np.isnan(got.reshape(-1)) & np.isnan(exp.reshape(-1)) & (eb != SENT32))
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first bad index {i}: got {got.reshape(-1)[i]!r} "
                             f"(bits {int(gb[i]):#x}), expected {exp.reshape(-1)[i]!r} (bits {int(eb[i]):#x})")
    return 0.0


def check_close(what, got, ref64, bound):
    """|got - ref64| <= bound element by element; returns the worst |got - ref| / bound.  Names the first bad index."""
    err = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(ref64, np.float64).reshape(-1))
    bound = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1), err.shape)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements past the bound, first bad index {i}: got {np.asarray(got).reshape(-1)[i]!r}, "
                             f"reference {np.asarray(ref64).reshape(-1)[i]!r}, bound {bound[i]:.3e}")
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(r.max()) if r.size else 0.0


# =====================================================================================================================================
# 4. backends and buffers
# =====================================================================================================================================
ALL_SIGS = {}
for _d in (capi._SIGS, capi._SIGS_CROSS, capi._SIGS_ADAGRAD, capi._SIGS_LR, capi._SIGS_CTR, capi._SIGS_DIGEST, capi._SIGS_BF16):
    ALL_SIGS.update(_d)


def hostmem(p, n, dtype):
    """a writable numpy view of n elements of host memory at address p (the stand-ins' face of a C pointer)"""
    dtype = np.dtype(dtype)
    return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(p), dtype)


class Backend:
    """`lib` under test (the product library on cuda:0, or the CPU oracle with STANDINS for what it does not export) and the oracle that
    supplies reference bits.  tamper: None, or a function (name, got, initial) -> got the CPU test uses to plant a wrong result."""

    def __init__(self, lib, oracle_lib):
        self.lib, self.oracle = lib, oracle_lib
        self.device = lib.backend != "oracle-cpu"
        self.tamper = None
        self.worst = 0.0

    def up(self, a, align=64):
        """a copy of `a` in the backend's memory, as a torch tensor (its data_ptr() at least `align`-byte aligned)"""
        a = np.ascontiguousarray(a)
        kind = a.dtype
        if a.dtype.kind == "u" and a.dtype.itemsize > 1:          # torch has no wide unsigned types: the signed one of the same size
            a = a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
        if self.device:
            t = torch.from_numpy(a).to("cuda:0")
        else:
            raw = torch.empty(a.nbytes + align, dtype=torch.uint8)
            skip = (-raw.data_ptr()) % align
            t = raw[skip:skip + a.nbytes].view(torch.from_numpy(a).dtype)
            t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % align == 0
        t.np_dtype = kind
        return t

    def fetch(self, name, t, initial=None):
        if self.device:
            torch.cuda.synchronize()
        got = t.cpu().numpy().copy()
        got = got.view(getattr(t, "np_dtype", got.dtype))
        if self.tamper is not None and initial is not None:
            got = self.tamper(name, got, initial)
        return got

    def call(self, name, *args):
        res, argtypes = ALL_SIGS[name]
        assert len(args) == len(argtypes) - 1, f"{name}: expected {len(argtypes) - 1} arguments, got {len(args)}"
        conv = [capi.ptr(a) if t is capi.P else a for a, t in zip(args, argtypes[1:])]
        fn = getattr(self.lib.lib, name, None)
        assert fn is not None or not self.device, f"{name} is missing from the product library"          # a missing kernel is an error
        if not self.device and name in STANDINS:
            rc = STANDINS[name](self, *conv) or 0
        else:
            fn.restype, fn.argtypes = res, argtypes
            rc = fn(self.lib.ctx, *conv)
        self.lib.check(rc, name)

    def note(self, ratio):
        self.worst = max(self.worst, float(ratio))

    # ---- the learning-rate block of the _lr entries: (handle, lr, alpha_t) -----------------------------------------------------------
    def lr_block(self, base, beta1, beta2):
        if not self.device:          # the stand-ins' block: two floats, the rate and Adam's alpha_t of the first step
            blk = torch.zeros(2, dtype=torch.float32)
            blk[0] = base
            blk[1] = float(base * np.sqrt(1 - beta2) / (1 - beta1)) if beta1 else base
            return blk, float(blk[0]), float(blk[1])
        lr = capi.lr_api(self.lib)
        blk = torch.zeros(lr.state_bytes(), dtype=torch.uint8, device="cuda:0")
        lr.init(blk, base, 0, 0, 0, beta1, beta2)
        v = lr.read(blk)
        return blk, float(np.float32(v.lr)), float(np.float32(v.alpha_t))


class Slab:
    """a flat payload inside an allocation of sentinels: FRONT (+ off) elements in front, BACK behind"""

    def __init__(self, be, name, payload, off=0):
        payload = np.ascontiguousarray(payload).reshape(-1)
        self.be, self.name, self.lo, self.n = be, name, FRONT + off, payload.size
        self.host = sentinels(payload.dtype, self.lo + self.n + BACK)
        self.host[self.lo:self.lo + self.n] = payload
        self.t = be.up(self.host)
        self.ptr = self.t.data_ptr() + self.lo * payload.dtype.itemsize

    def expect(self, payload=None):
        e = self.host.copy()
        if payload is not None:
            e[self.lo:self.lo + self.n] = np.ascontiguousarray(payload).reshape(-1)
        return e

    def got(self):
        return self.be.fetch(self.name, self.t, self.host)

    def around(self):
        """the sentinels around the payload kept their bits; returns the payload read back (for a check against a bound)"""
        g = self.got()
        inside = np.s_[self.lo:self.lo + self.n]
        check(self.name + " (the sentinels around it)", np.delete(g, inside), np.delete(self.host, inside))
        return g[inside]

    def check(self, payload=None):
        """the whole allocation afterwards: untouched (an input), or with the payload replaced; returns the payload read back"""
        g = self.got()
        check(self.name, g, self.expect(payload))
        return g[self.lo:self.lo + self.n]


def strided(rows, dim, ld, values, dtype=np.float32, behind=2):
    """[rows][dim] at row stride ld as a flat payload with sentinel pad columns and `behind` sentinel rows"""
    flat = sentinels(dtype, (rows + behind) * ld)
    np.lib.stride_tricks.as_strided(flat, (rows, dim), (flat.itemsize * ld, flat.itemsize))[:] = values
    return flat


def view2(flat, rows, dim, ld):
    return np.lib.stride_tricks.as_strided(flat, (rows, dim), (flat.itemsize * ld, flat.itemsize))


# =====================================================================================================================================
# 5. the runners: generator, launch, reference and check of one case
# =====================================================================================================================================
RUN = {}


def runner(*entries):
    def deco(f):
        for e in entries:
            RUN[e] = f
        return f
    return deco


def run_case(be, c):
    """asserts the case's trip count, runs it on `be`, prints and returns the worst |got - ref| / bound it saw (0: everything bit for bit)"""
    t = assert_trips(c)
    be.worst = 0.0
    RUN[c.entry](be, c)
    print(f"{case_id(c)}: {t} trips, worst |got - ref| / bound = {be.worst:.3f}")
    return be.worst


# ---- the cross combine ------------------------------------------------------------------------------------------------------------------
def _cross_buf(be, batch, dim, ld, off, vals):
    import test_gpu_cross as XC
    if be.device:
        return XC.Buf(batch, dim, ld, off, vals)
    b = XC.Buf.__new__(XC.Buf)
    b.batch, b.dim, b.ld, b.off = batch, dim, ld, off
    b.host = np.full(off + (batch + 2) * ld + 4, XC.SENTINEL, np.float32)
    b.view(b.host)[:] = vals
    b.dev = be.up(b.host)
    b.ptr = b.dev.data_ptr() + 4 * off
    return b


def _cross_check(be, name, buf, values=None):
    import test_gpu_cross as XC
    got = be.fetch(name, buf.dev, buf.host)
    check(name, got, buf.expect(values))
    XC.same_bits(got, buf.expect(values), name)


def _cross_layout(a):
    dim = a["dim"]
    ld = (dim + 31) // 32 * 32
    return ld, (lambda k: 1 if (a.get("scalar") and k == 1) else 0)


@runner("ffh_cross_fwd")
def run_cross_fwd(be, c):
    import test_gpu_cross as XC
    a = c.args
    batch, dim = a["batch"], a["dim"]
    ld, off = _cross_layout(a)
    x0 = _cross_buf(be, batch, dim, ld, off(0), XC.values(batch, dim, 1))
    v = _cross_buf(be, batch, dim, ld, off(1), XC.values(batch, dim, 2))
    xl = _cross_buf(be, batch, dim, ld, off(2), XC.values(batch, dim, 3))
    y = _cross_buf(be, batch, dim, ld, off(3), XC.SENTINEL)
    be.call("ffh_cross_fwd", y.ptr, ld, x0.ptr, ld, v.ptr, ld, xl.ptr, ld, batch, dim, None)
    _cross_check(be, "y", y, ffmodel.cross_reference(x0.view(x0.host), v.view(v.host), xl.view(xl.host)))
    for name, b in (("x0", x0), ("v", v), ("xl", xl)):
        _cross_check(be, name, b)


@runner("ffh_cross_bwd")
def run_cross_bwd(be, c):
    import test_gpu_cross as XC
    a = c.args
    batch, dim = a["batch"], a["dim"]
    ld, off = _cross_layout(a)
    dy = _cross_buf(be, batch, dim, ld, off(0), XC.values(batch, dim, 4))
    x0 = _cross_buf(be, batch, dim, ld, off(1), XC.values(batch, dim, 5))
    v = _cross_buf(be, batch, dim, ld, off(2), XC.values(batch, dim, 6))
    add0, addl = XC.values(batch, dim, 7), XC.values(batch, dim, 8)
    for aliased in (False, True):          # ADD / ADD on separate buffers, and layer 0's one accumulated write (dx0 == dxl)
        dv = _cross_buf(be, batch, dim, ld, off(3), XC.SENTINEL)
        dx0 = _cross_buf(be, batch, dim, ld, off(4), add0)
        dxl = dx0 if aliased else _cross_buf(be, batch, dim, ld, off(5), addl)
        be.call("ffh_cross_bwd", dy.ptr, ld, x0.ptr, ld, v.ptr, ld, dv.ptr, ld, dx0.ptr, ld, capi.CROSS_ADD, dxl.ptr, ld, capi.CROSS_ADD, batch, dim, None)
        g_dv, g0, gl = ffmodel.cross_reference_backward(dy.view(dy.host), x0.view(x0.host), v.view(v.host), aliased=aliased)
        with np.errstate(all="ignore"):
            _cross_check(be, "dv", dv, g_dv)
            _cross_check(be, "dx0", dx0, add0 + g0)
            if not aliased:
                _cross_check(be, "dxl", dxl, addl + gl)
        for name, b in (("dy", dy), ("x0", x0), ("v", v)):
            _cross_check(be, name, b)


# ---- the dense optimizers ---------------------------------------------------------------------------------------------------------------
HP = dict(lr=0.05, wd=1e-3, mom=0.9, alpha=0.001, b1=0.9, b2=0.999, eps=1e-8, ag_eps=1e-10)
# (hyper-parameters of the rule, FFH_OPT_ZERO_GRAD): SGD plain and with weight decay + Nesterov momentum; Adagrad without and with weight decay
OPT_CONFIGS = {"sgd": [(dict(wd=0.0, mom=0.0, nesterov=0), 0), (dict(wd=HP["wd"], mom=HP["mom"], nesterov=1), 1)],
               "adam": [(dict(wd=0.0), 0), (dict(wd=HP["wd"]), 1)],
               "adagrad": [(dict(wd=0.0), 1), (dict(wd=HP["wd"]), 0)]}


def f32(x):
    return float(np.float32(x))


def opt_reference(be, rule, w, g, s0, s1, rate, h):
    """(w, s0, s1 afterwards in float32 bits -- the oracle's for SGD and Adam, ffmodel.adagrad_reference for Adagrad --, float64 w, bound)"""
    n = w.size
    W, Gd, A, B_ = (None if x is None else x.astype(np.float64) for x in (w, g, s0, s1))
    rate32, wd32 = np.float64(np.float32(rate)), np.float64(np.float32(h["wd"]))
    if rule == "sgd":
        w1, g1 = w.copy(), g.copy()
        v1 = None if s0 is None else s0.copy()
        be.oracle.call("ffh_sgd_update_ex", w1, g1, v1, n, f32(rate), f32(h["wd"]), f32(h["mom"]), h["nesterov"], 0, None)
        mom = np.float64(np.float32(h["mom"]))
        gt, T = Gd + wd32 * W, np.abs(Gd) + wd32 * np.abs(W)
        if h["mom"] > 0:
            V1, Va = A * mom + gt, np.abs(A) * mom + T
            gt, T = (gt + mom * V1, T + mom * Va) if h["nesterov"] else (V1, Va)
        return w1, v1, None, W - rate32 * gt, 4 * EPS32 * (np.abs(W) + rate32 * T)          # the chain rounds four times
    if rule == "adam":
        w1, g1, m1, v1 = w.copy(), g.copy(), s0.copy(), s1.copy()
        be.oracle.call("ffh_adam_update", w1, g1, m1, v1, n, f32(rate), f32(HP["b1"]), f32(HP["b2"]), f32(h["wd"]), f32(HP["eps"]), 0, None)
        b1, b2 = np.float64(np.float32(HP["b1"])), np.float64(np.float32(HP["b2"]))
        omb1, omb2 = np.float64(np.float32(1) - np.float32(HP["b1"])), np.float64(np.float32(1) - np.float32(HP["b2"]))
        gt = Gd + wd32 * W
        M1, V1 = b1 * A + omb1 * gt, b2 * B_ + omb2 * gt * gt
        step = rate32 * M1 / (np.sqrt(V1) + np.float64(np.float32(HP["eps"])))
        return w1, m1, v1, W - step, 8 * EPS32 * (np.abs(W) + np.abs(step))                  # seven roundings
    w1, S1 = ffmodel.adagrad_reference(w, g, s0, f32(rate), f32(HP["ag_eps"]), f32(h["wd"]))
    gt, T = Gd + wd32 * W, np.abs(Gd) + wd32 * np.abs(W)
    d = np.sqrt(A + gt * gt) + np.float64(np.float32(HP["ag_eps"]))
    return w1, S1, None, W - rate32 * gt / d, 4 * EPS32 * (np.abs(W) + rate32 * T / d)


def opt_inputs(rule, n, h, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1, 1, n).astype(np.float32)
    g = rng.uniform(-1, 1, n).astype(np.float32)
    s0 = s1 = None
    if rule == "sgd" and h["mom"] > 0:
        s0 = rng.uniform(-1, 1, n).astype(np.float32)
    elif rule == "adam":
        s0 = (g * rng.uniform(0.1, 1, n)).astype(np.float32)          # a first moment of the gradient's sign: no cancellation in b1 m + (1 - b1) g
        s1 = rng.uniform(1e-3, 0.1, n).astype(np.float32)             # the square root is well conditioned
    elif rule == "adagrad":
        s0 = rng.uniform(1e-3, 0.1, n).astype(np.float32)
    return w, g, s0, s1


def opt_launch(be, entry, rule, wp, gp, s0p, s1p, n, h, zg):
    """launches `entry` at the rate the reference then uses; returns that rate"""
    lrf = entry.endswith("_lr")
    base = HP["alpha"] if rule == "adam" else HP["lr"]
    rate = base
    if lrf:
        blk, lr, alpha_t = be.lr_block(base, HP["b1"] if rule == "adam" else 0.0, HP["b2"] if rule == "adam" else 0.0)
        rate = alpha_t if rule == "adam" else lr
    if rule == "sgd":
        be.call(entry, wp, gp, s0p, n, blk if lrf else f32(rate), f32(h["wd"]), f32(h["mom"]), h["nesterov"], zg, None)
    elif rule == "adam":
        be.call(entry, wp, gp, s0p, s1p, n, blk if lrf else f32(rate), f32(HP["b1"]), f32(HP["b2"]), f32(h["wd"]), f32(HP["eps"]), zg, None)
    else:
        be.call(entry, wp, gp, s0p, n, blk if lrf else f32(rate), f32(HP["ag_eps"]), f32(h["wd"]), zg, None)
    return rate


@runner("ffh_sgd_update_ex", "ffh_adam_update", "ffh_adagrad_update", "ffh_sgd_update_ex_lr", "ffh_adam_update_lr", "ffh_adagrad_update_lr")
def run_opt(be, c):
    a, entry = c.args, c.entry
    rule = "sgd" if "sgd" in entry else "adam" if "adam" in entry else "adagrad"
    n = a["n"]
    assert (n % 4 == 0) == a.get("vec", True)          # n % 4 != 0 is what makes the launcher take the scalar form
    if a.get("mirror"):
        return run_opt_mirror(be, c, rule)
    for k, (h, zg) in enumerate(OPT_CONFIGS[rule]):
        w, g, s0, s1 = opt_inputs(rule, n, h, 1000 * k + n % 997)
        W, Gs = Slab(be, "w", w), Slab(be, "g", g)
        S0 = None if s0 is None else Slab(be, "state0", s0)
        S1 = None if s1 is None else Slab(be, "state1", s1)
        rate = opt_launch(be, entry, rule, W.ptr, Gs.ptr, S0 and S0.ptr, S1 and S1.ptr, n, h, zg)
        w1, a1, b1, w64, bound = opt_reference(be, rule, w, g, s0, s1, rate, h)
        gw = W.check(w1)
        Gs.check(np.zeros(n, np.float32) if zg else None)
        if S0 is not None:
            S0.check(a1)
        if S1 is not None:
            S1.check(b1)
        be.note(check_close("w against the float64 formula", gw, w64, bound))


def run_opt_mirror(be, c, rule):
    """the range inside a registered bf16 twin (tensor-op mode) / three-plane image (split mode): afterwards the mirror is the image of the
    stored floats over the WHOLE region"""
    from test_gpu_round6 import image_of
    assert be.device, "the mirrors of the product library"
    a, n = c.args, c.args["n"]
    twin = a["mirror"] == "twin"
    lo = 8 if twin else 32 * 7 + 4
    R = (lo + n + 40 + 31) // 32 * 32
    h, zg = OPT_CONFIGS[rule][1]
    rng = np.random.default_rng(5)
    region = rng.uniform(-1, 1, R).astype(np.float32)
    w, g, s0, s1 = opt_inputs(rule, n, h, 77)
    region[lo:lo + n] = w
    Wt = be.up(region, align=128)
    side = torch.zeros(R if twin else R // 32 * 96, dtype=torch.int16, device="cuda:0")
    Gs = Slab(be, "g", g)
    S0 = None if s0 is None else Slab(be, "state0", s0)
    S1 = None if s1 is None else Slab(be, "state1", s1)
    lib = be.lib
    reg = lib.lib.ffh_ctx_bf16_mirror_set if twin else lib.lib.ffh_ctx_bf16x3_mirror_set
    assert lib.lib.ffh_ctx_set_math_mode(lib.ctx, 1 if twin else 2) == 0
    try:
        assert reg(lib.ctx, Wt.data_ptr(), R * 4, side.data_ptr()) == 0
        if twin:
            be.call("ffh_convert_f32_to_bf16", side, Wt, R, None)
        else:
            be.call("ffh_convert_f32_to_bf16x3", Wt, 1, R, R, None)
        rate = opt_launch(be, c.entry, rule, Wt.data_ptr() + 4 * lo, Gs.ptr, S0 and S0.ptr, S1 and S1.ptr, n, h, zg)
        w1, a1, b1, w64, bound = opt_reference(be, rule, w, g, s0, s1, rate, h)
        exp = region.copy()
        exp[lo:lo + n] = w1
        got = be.fetch("w", Wt, region)
        check("w (the whole region)", got, exp)
        mirror = be.fetch("mirror", side).view(np.uint16)
        check("mirror", mirror, BH.rne(got) if twin else image_of(got).reshape(-1))
        Gs.check(np.zeros(n, np.float32) if zg else None)
        if S0 is not None:
            S0.check(a1)
        if S1 is not None:
            S1.check(b1)
        be.note(check_close("w against the float64 formula", got[lo:lo + n], w64, bound))
    finally:
        assert reg(lib.ctx, Wt.data_ptr(), R * 4, None) == 0
        assert lib.lib.ffh_ctx_set_math_mode(lib.ctx, 0) == 0


# ---- mse_bwd, add_scaled, sum_slices ------------------------------------------------------------------------------------------------------
def scaled_difference(x, y, scale):
    """the MSE gradient as the kernels and the oracle state it: fmaf(scale, x - y, +0) -- (x - y) * scale in float32, two roundings, where
    the + 0 of the fused form turns a product of -0 into +0 (the BCE entry multiplies plainly and keeps the sign)"""
    return (x - y) * np.float32(scale) + np.float32(0.0)


@runner("ffh_mse_bwd")
def run_mse_bwd(be, c):
    n = c.args["n"]
    rng = np.random.default_rng(n)
    logit, label = rng.uniform(-2, 2, n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)
    scale = np.float32(2.0 / 3.0)
    Lg, Lo, La = Slab(be, "lg", sentinels(np.float32, n)), Slab(be, "logit", logit), Slab(be, "label", label)
    be.call("ffh_mse_bwd", Lg.ptr, Lo.ptr, La.ptr, n, float(scale), None)
    Lg.check(scaled_difference(logit, label, scale))
    Lo.check(); La.check()


@runner("ffh_add_scaled")
def run_add_scaled(be, c):
    n = c.args["n"]
    rng = np.random.default_rng(n)
    d, src = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    scale = np.float32(-0.3)
    D, S = Slab(be, "dst", d), Slab(be, "src", src)
    be.call("ffh_add_scaled", D.ptr, S.ptr, n, float(scale), None)
    D.check((src.astype(np.float64) * np.float64(scale) + d.astype(np.float64)).astype(np.float32))      # one fma: the float64 value rounded once
    S.check()


@runner("ffh_sum_slices_f32")
def run_sum_slices(be, c):
    n = c.args["n"]
    stride, ns = n + (8 if n % 4 == 0 else 3), 3
    rng = np.random.default_rng(n)
    src = sentinels(np.float32, (ns - 1) * stride + n)
    sl = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(ns)]
    for q in range(ns):
        src[q * stride:q * stride + n] = sl[q]
    D, S = Slab(be, "dst", sentinels(np.float32, n)), Slab(be, "src", src)
    be.call("ffh_sum_slices_f32", D.ptr, S.ptr, ns, n, stride, None)
    D.check((sl[0] + sl[1]) + sl[2])
    S.check()


# ---- the metrics ----------------------------------------------------------------------------------------------------------------------------
ALL_FLAGS = capi.METRIC_ACCURACY | capi.METRIC_MSE | capi.METRIC_RMSE | capi.METRIC_MAE
SUM_RTOL = 1e-5          # of the sum of the absolute terms (tests/test_gpu_ctr.py)


def metrics_inputs(ns, nc, prob, seed):
    rng = np.random.default_rng(seed)
    if prob:
        x = rng.uniform(0.001, 0.999, (ns, nc)).astype(np.float32)
    else:
        x = rng.uniform(-2, 2, (ns, nc)).astype(np.float32)
    x[::3] = np.clip(np.round(x[::3] * 8) / 8, 0.125, 0.875) if prob else np.round(x[::3] * 4) / 4          # coarse values: ties of the maximum
    if nc == 1:
        y = rng.integers(0, 2, (ns, 1)).astype(np.float32)
    else:
        y = np.zeros((ns, nc), np.float32)
        y[np.arange(ns), rng.integers(0, nc, ns)] = 1.0
        y[5::11, 0] = 0.95          # two labels above 0.9 in some rows (the last one counts) ...
        y[7::13] = 0.0              # ... and none in others
    return x, y


def accuracy_rule(x, y):
    """the kernel's contract in numpy: the FIRST maximum of the row against the LAST label above 0.9"""
    ns, nc = x.shape
    if nc == 1:
        return 2 * ns, ns
    my = np.argmax(x, axis=1)
    m = y > np.float32(0.9)
    tr = np.where(m.any(axis=1), nc - 1 - np.argmax(m[:, ::-1], axis=1), -1)
    return ns, int((my == tr).sum())


def check_sum(be, what, got, terms):
    """a float32 sum of many terms against float64, within SUM_RTOL of the sum of the absolute terms"""
    t = np.asarray(terms, np.float64)
    be.note(check_close(what, np.float64(got), t.sum(), SUM_RTOL * np.abs(t).sum()))


def bce_terms(p, y):
    p, y = p.astype(np.float64), y.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(y * np.fmax(np.log(p), -100.0) + (1 - y) * np.fmax(np.log1p(-p), -100.0))          # fmaxf: a NaN logarithm (p > 1) gives -100


@runner("ffh_metrics_update", "ffh_mse_bwd_metrics", "ffh_bce_bwd_metrics")
def run_metrics(be, c):
    ns, entry = c.args["ns"], c.entry
    bce = entry == "ffh_bce_bwd_metrics"
    flags = ALL_FLAGS | (capi.METRIC_BCE if bce else 0)
    scale = np.float32(1.0 / 7.0)
    for nc in (1, 3):
        x, y = metrics_inputs(ns, nc, bce, ns + nc)
        X, Y = Slab(be, "logits", x), Slab(be, "labels", y)
        perf = be.up(np.zeros(C.sizeof(capi.PerfMetrics), np.uint8))
        Lg = Slab(be, "lg", sentinels(np.float32, ns * nc))
        Bs = Slab(be, "bce_sum", np.zeros(1, np.float32))
        if entry == "ffh_metrics_update":
            be.call(entry, X.ptr, Y.ptr, perf, ns, nc, flags, None)
        elif bce:
            be.call(entry, Lg.ptr, X.ptr, Y.ptr, perf, Bs.ptr, ns, nc, float(scale), flags, None)
        else:
            be.call(entry, Lg.ptr, X.ptr, Y.ptr, perf, ns, nc, float(scale), flags, None)
        pm = capi.PerfMetrics.from_buffer_copy(be.fetch("perf", perf).tobytes())
        all_, correct = accuracy_rule(x, y)
        assert (pm.train_all, pm.train_correct) == (all_, correct), f"counts nc={nc}: {(pm.train_all, pm.train_correct)} against {(all_, correct)}"
        d = x.astype(np.float64) - y.astype(np.float64)
        check_sum(be, f"mse nc={nc}", pm.mse_loss, d * d)
        check_sum(be, f"rmse nc={nc}", pm.rmse_loss, np.sqrt((d * d).sum(axis=1)))
        check_sum(be, f"mae nc={nc}", pm.mae_loss, np.abs(d))
        assert pm.cce_loss == 0 and pm.sparse_cce_loss == 0
        if entry == "ffh_metrics_update":
            Lg.check()
        else:
            Lg.check((x - y) * scale if bce else scaled_difference(x, y, scale))          # (p - y) * scale, two roundings
        if bce:
            check_sum(be, f"bce nc={nc}", Bs.around()[0], bce_terms(x, y))
        X.check(); Y.check()


def ctr_bins(p):
    t = np.nan_to_num(p * np.float32(capi.AUC_BINS), nan=0.0)
    return np.clip(t, 0, capi.AUC_BINS - 1).astype(np.int64)          # t <= 0 or NaN: bin 0; t >= the bins: the last one; else the integer part


@runner("ffh_ctr_eval_update")
def run_ctr_eval(be, c):
    ns = c.args["ns"]
    rng = np.random.default_rng(ns)
    p = rng.uniform(0, 1, ns).astype(np.float32)
    p[::101], p[3::103], p[5::107], p[7::109] = 0.0, 1.0, np.nan, 1.5
    y = rng.integers(0, 2, ns).astype(np.float32)
    P_, Y = Slab(be, "prob", p), Slab(be, "label", y)
    ev = be.up(np.zeros(C.sizeof(capi.CtrEval), np.uint8))
    be.call("ffh_ctr_eval_update", P_.ptr, Y.ptr, ev, ns, None)
    e = capi.CtrEval.from_buffer_copy(be.fetch("ev", ev).tobytes())
    ok = ~np.isnan(p)
    pos = (y >= 0.5) & ok
    assert e.samples == int(ok.sum()) and e.positives == int(pos.sum()) and e.nan_predictions == int((~ok).sum())
    assert e.correct == int((((p >= 0.5) == (y >= 0.5)) & ok).sum())
    bins = ctr_bins(p)
    check("hist_pos", np.ctypeslib.as_array(e.hist_pos).astype(np.uint64), np.bincount(bins[pos], minlength=capi.AUC_BINS).astype(np.uint64))
    check("hist_neg", np.ctypeslib.as_array(e.hist_neg).astype(np.uint64), np.bincount(bins[ok & ~pos], minlength=capi.AUC_BINS).astype(np.uint64))
    check_sum(be, "logloss", e.logloss_sum, bce_terms(p[ok], y[ok]))
    P_.check(); Y.check()


# ---- transpose, concat, tril ----------------------------------------------------------------------------------------------------------------
@runner("ffh_transpose_fwd", "ffh_transpose_bwd")
def run_transpose(be, c):
    dims, perm = c.args["dims"], c.args["perm"]
    vol = int(np.prod(dims))
    rng = np.random.default_rng(vol)
    if c.entry == "ffh_transpose_fwd":
        x = rng.uniform(-1, 1, dims).astype(np.float32)
        X, O = Slab(be, "in", x), Slab(be, "out", sentinels(np.float32, vol))
        be.lib.transpose("ffh_transpose_fwd", O.ptr, X.ptr, dims, perm)
        O.check(np.ascontiguousarray(x.transpose(perm)))
        X.check()
    else:
        og = rng.uniform(-1, 1, [dims[p] for p in perm]).astype(np.float32)
        ig0 = rng.uniform(-1, 1, dims).astype(np.float32)
        Og, Ig = Slab(be, "out_grad", og), Slab(be, "in_grad", ig0)
        be.lib.transpose("ffh_transpose_bwd", Ig.ptr, Og.ptr, dims, perm)
        Ig.check(ig0 + og.transpose(np.argsort(perm)))          # one float32 add per element
        Og.check()


@runner("ffh_concat_fwd", "ffh_concat_bwd", "ffh_concat_bwd_ex")
def run_concat(be, c):
    rows, widths = c.args["rows"], c.args["widths"]
    lds = [widths[0], widths[1], 80, widths[3]]
    lead, total = 3, sum(widths)          # 3 columns of something else in front: no 16-byte group of the wide row is aligned
    out_blk = lead + total + 5
    rng = np.random.default_rng(rows)
    cols = np.cumsum([0] + list(widths))
    parts0 = [rng.uniform(-1, 1, (rows, w)).astype(np.float32) for w in widths]
    big0 = rng.uniform(-1, 1, (rows, total)).astype(np.float32)
    fwd = c.entry == "ffh_concat_fwd"
    Ps = [Slab(be, f"part{k}", strided(rows, w, ld, p)) for k, (w, ld, p) in enumerate(zip(widths, lds, parts0))]
    bigflat = sentinels(np.float32, lead + (rows + 2) * out_blk)
    if not fwd:
        view2(bigflat[lead:], rows, total, out_blk)[:] = big0
    Bg = Slab(be, "big", bigflat)
    ptrs = [p.ptr for p in Ps]
    if fwd:
        be.lib.concat("ffh_concat_fwd", Bg.ptr + 4 * lead, out_blk, ptrs, widths, lds, rows)
        e = bigflat.copy()
        view2(e[lead:], rows, total, out_blk)[:] = np.concatenate(parts0, axis=1)
        Bg.check(e)
        for p in Ps:
            p.check()
        return
    overwrite = c.entry == "ffh_concat_bwd_ex"
    n = len(ptrs)
    pa, ba, la = (capi.P * n)(*ptrs), (capi.L * n)(*widths), (capi.L * n)(*lds)
    if overwrite:
        rc = be.lib.lib.ffh_concat_bwd_ex(be.lib.ctx, Bg.ptr + 4 * lead, out_blk, pa, ba, la, n, rows, capi.CONCAT_BWD_OVERWRITE, None)
    else:
        rc = be.lib.lib.ffh_concat_bwd(be.lib.ctx, Bg.ptr + 4 * lead, out_blk, pa, ba, la, n, rows, None)
    be.lib.check(rc, c.entry)
    for k, p in enumerate(Ps):
        gk = big0[:, cols[k]:cols[k + 1]]
        p.check(strided(rows, widths[k], lds[k], gk if overwrite else parts0[k] + gk))
    Bg.check()


@runner("ffh_tril_fwd", "ffh_tril_bwd")
def run_tril(be, c):
    n, batch = c.args["n"], c.args["batch"]
    P = n * (n - 1) // 2
    ld = P + 3
    rng = np.random.default_rng(batch)
    ii, jj = np.tril_indices(n, -1)
    if c.entry == "ffh_tril_fwd":
        z = rng.uniform(-1, 1, (batch, n, n)).astype(np.float32)
        Z, O = Slab(be, "in", z), Slab(be, "out", sentinels(np.float32, (batch + 2) * ld))
        be.call("ffh_tril_fwd", O.ptr, ld, Z.ptr, batch, n, None)
        ref = np.empty((batch, P), np.float32)
        be.oracle.call("ffh_tril_fwd", ref, P, z, batch, n, None)
        check("the oracle against numpy's tril_indices", ref, z[:, ii, jj])
        O.check(strided(batch, P, ld, ref))
        Z.check()
    else:
        g = rng.uniform(-1, 1, (batch, P)).astype(np.float32)
        ig0 = rng.uniform(-1, 1, (batch, n, n)).astype(np.float32)
        Gs, Ig = Slab(be, "out_grad", strided(batch, P, ld, g)), Slab(be, "in_grad", ig0)
        be.call("ffh_tril_bwd", Ig.ptr, Gs.ptr, ld, batch, n, None)
        ref = ig0.copy()
        be.oracle.call("ffh_tril_bwd", ref, np.ascontiguousarray(g), P, batch, n, None)
        e = ig0.copy()
        e[:, ii, jj] += g
        check("the oracle against numpy's tril_indices", ref, e)
        Ig.check(ref)
        Gs.check()


# ---- the embedding entries ------------------------------------------------------------------------------------------------------------------
@runner("ffh_embedding_bwd_dense")
def run_emb_bwd_dense(be, c):
    batch, D, R = c.args["batch"], c.args["D"], 1000
    rng = np.random.default_rng(batch)
    idx = rng.integers(0, R, (batch, 1)).astype(np.int64)
    g = rng.uniform(-1, 1, (batch, D)).astype(np.float32)
    wg0 = rng.uniform(-1, 1, (R, D)).astype(np.float32)
    I_, Gs, Wg = Slab(be, "idx", idx), Slab(be, "g", g), Slab(be, "wg", wg0)
    be.call("ffh_embedding_bwd_dense", I_.ptr, Gs.ptr, Wg.ptr, 1, D, batch, R, D, capi.AGGR_MODE_SUM, None)
    ref, mass = wg0.astype(np.float64), np.abs(wg0).astype(np.float64)
    np.add.at(ref, idx[:, 0], g.astype(np.float64))
    np.add.at(mass, idx[:, 0], np.abs(g).astype(np.float64))
    be.note(check_close("wg", Wg.around(), ref, 1e-5 * mass + 1e-6))          # test_embedding_backward_reference_fixture_on_gpu's bound
    I_.check(); Gs.check()


@runner("ffh_embedding_localize_rows")
def run_localize(be, c):
    n = c.args["n"]
    begin, local = 1000, 5000
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 8000, n).astype(np.int64)          # ids below, inside and above the slice
    idx[:6] = [0, begin - 1, begin, begin + local - 1, begin + local, 7999]
    I_, O = Slab(be, "idx", idx), Slab(be, "local", sentinels(np.int64, n))
    be.call("ffh_embedding_localize_rows", I_.ptr, O.ptr, n, begin, local, None)
    r = idx - begin
    O.check(np.where((r >= 0) & (r < local), r, local))
    I_.check()


# ---- conversions, fill, generators ----------------------------------------------------------------------------------------------------------
def wide_values(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    a[::97], a[5::101] = 0.0, -0.0
    return a


@runner("ffh_convert_f32_to_bf16")
def run_convert_bf16(be, c):
    n, off = c.args["n"], c.args.get("off", 0)
    a = wide_values(n, n)
    S, D = Slab(be, "src", a, off), Slab(be, "dst", sentinels(np.uint16, n), off)
    be.call("ffh_convert_f32_to_bf16", D.ptr, S.ptr, n, None)
    D.check(BH.rne(a))
    S.check()


@runner("ffh_convert_f32_to_bf16x3")
def run_convert_x3(be, c):
    from test_gpu_round6 import image_of
    a = c.args
    rows, cols, ld = a["rows"], a["cols"], a["ld"]
    e0 = 5 if a.get("scalar") else 0
    R = (e0 + (rows - 1) * ld + cols + 31) // 32 * 32
    region = wide_values(R, rows)
    Rt = be.up(region, align=128)
    img = be.up(np.zeros(R // 32 * 96, np.uint16), align=128)
    lib = be.lib
    assert lib.lib.ffh_ctx_bf16x3_mirror_set(lib.ctx, Rt.data_ptr(), R * 4, img.data_ptr()) == 0
    try:
        be.call("ffh_convert_f32_to_bf16x3", Rt.data_ptr() + 4 * e0, rows, cols, ld, None)
        mask = np.zeros(R, bool)
        view2(mask[e0:], rows, cols, ld)[:] = True
        exp = image_of(region)
        exp[~np.broadcast_to(mask.reshape(-1, 1, 32), exp.shape)] = 0          # elements outside the sub-matrix keep their zeros
        check("image", be.fetch("image", img, np.zeros(R // 32 * 96, np.uint16)), exp.reshape(-1))
        check("region", be.fetch("region", Rt), region)
    finally:
        assert lib.lib.ffh_ctx_bf16x3_mirror_set(lib.ctx, Rt.data_ptr(), R * 4, None) == 0


@runner("ffh_fill_f32")
def run_fill(be, c):
    n, off = c.args["n"], c.args.get("off", 0)
    D = Slab(be, "dst", sentinels(np.float32, n), off)
    be.call("ffh_fill_f32", D.ptr, n, 1.25, None)
    D.check(np.full(n, 1.25, np.float32))


@runner("ffh_init_uniform", "ffh_gen_indices", "ffh_gen_uniform01", "ffh_gen_bernoulli")
def run_gen(be, c):
    n, entry = c.args["n"], c.entry
    seed, first, R = 0x5EED1234, 2 ** 33, 39884407
    h = BH.hash64(np.uint64(seed), np.uint64(first) + np.arange(n, dtype=np.uint64))
    if entry == "ffh_gen_indices":
        D, ref = Slab(be, "dst", sentinels(np.int64, n)), np.empty(n, np.int64)
        be.call(entry, D.ptr, n, seed, first, R, None)
        be.oracle.call(entry, ref, n, seed, first, R, None)
        check("the oracle against the hash in numpy", ref, (h % np.uint64(R)).astype(np.int64))
    else:
        D, ref = Slab(be, "dst", sentinels(np.float32, n)), np.empty(n, np.float32)
        if entry == "ffh_init_uniform":
            be.call(entry, D.ptr, n, seed, -0.05, 0.07, None)
            be.oracle.call(entry, ref, n, seed, -0.05, 0.07, None)
        else:
            be.call(entry, D.ptr, n, seed, first, None)
            be.oracle.call(entry, ref, n, seed, first, None)
            num = ((h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)) if entry == "ffh_gen_uniform01" else \
                ((h >> np.uint64(33)) & np.uint64(1)).astype(np.float32)
            check("the oracle against the hash in numpy", ref, num)
    D.check(ref)


@runner("ffh_init_uniform_bf16")
def run_init_uniform_bf16(be, c):
    n, seed = c.args["n"], 0xB16B16
    D, ref = Slab(be, "dst", sentinels(np.uint16, n)), np.empty(n, np.float32)
    if be.device:
        be.call("ffh_init_uniform_bf16", D.ptr, n, seed, -0.05, 0.07, None)
    be.oracle.call("ffh_init_uniform", ref, n, seed, -0.05, 0.07, None)          # the float32 draw, rounded to nearest even
    if not be.device:          # (stand-in: the oracle has no bf16 tables)
        hostmem(D.ptr, n, np.uint16)[:] = BH.rne(ref)
    D.check(BH.rne(ref))


@runner("ffh_embedding_fwd_multi", "ffh_embedding_fwd_multi_bf16")
def run_gather(be, c):
    """tables of 23 + 17 t rows (tests/test_gpu_bags.py), side by side in one Concat-like destination; bits against the numpy sum in
    ascending j from +0"""
    a, bf16 = c.args, c.entry.endswith("_bf16")
    nt, D, batch, L = a["nt"], a["D"], a["batch"], 2
    col0 = 4 if D % 4 == 0 else 1
    ld = col0 + nt * D + 4
    rng = np.random.default_rng(batch + D)
    out = sentinels(np.float32, (batch + 2) * ld)
    exp = out.copy()
    Ws, Is = [], []
    for t in range(nt):
        R = 23 + 17 * t
        w = rng.standard_normal((R, D)).astype(np.float32)
        w[0, :] = -0.0          # (+0) + (-0) = +0
        if bf16:
            w = BH.widen(BH.rne(w))
        i = rng.integers(0, R, (batch, L)).astype(np.int64)
        i[2, :] = 0
        acc = np.zeros((batch, D), np.float32)
        for j in range(L):
            acc = acc + w[i[:, j]]
        view2(exp[col0 + t * D:], batch, D, ld)[:] = acc
        Ws.append(w); Is.append(i)
    O = Slab(be, "out", out)
    Wd = [Slab(be, f"w{t}", BH.rne(w) if (bf16 and be.device) else w) for t, w in enumerate(Ws)]
    Id = [Slab(be, f"idx{t}", i) for t, i in enumerate(Is)]
    entries = [(Id[t].ptr, Wd[t].ptr, O.ptr + 4 * (col0 + t * D), 23 + 17 * t, ld) for t in range(nt)]
    lib = be.lib
    if bf16 and be.device:
        arr = capi.Bf16Api.tables(entries)
        fn = lib.lib.ffh_embedding_fwd_multi_bf16
        fn.restype, fn.argtypes = capi._SIGS_BF16["ffh_embedding_fwd_multi_bf16"]
        lib.check(fn(lib.ctx, arr, nt, L, D, batch, capi.AGGR_MODE_SUM, None), c.entry)
    else:          # (host: the fp32 gather on the widened tables stands in for the bf16 one -- the same sums by contract)
        lib.check(lib.lib.ffh_embedding_fwd_multi(lib.ctx, lib.emb_tables(entries), nt, L, D, batch, capi.AGGR_MODE_SUM, None), c.entry)
    O.check(exp)
    for s_ in Wd + Id:
        s_.check()


# ---- the state digest -----------------------------------------------------------------------------------------------------------------------
@runner("ffh_state_digest")
def run_digest(be, c):
    a = c.args
    rows, rb, lw = a["rows"], a["row_bytes"], a["lw"]
    ld = (rb + 15) // 16 * 16 + 16
    off = 0 if lw == 16 else 2          # in uint16 elements: a base 4 bytes off a 16-byte boundary takes the 4-byte word form
    rng = np.random.default_rng(rows + lw)
    data = rng.integers(0, 65536, (rows, rb // 2)).astype(np.uint16)
    S = Slab(be, "state", strided(rows, rb // 2, ld // 2, data, np.uint16), off)
    assert S.ptr % 16 == (0 if lw == 16 else 4)
    seed, index_base, start = 0xD16E57, 12345, 0x0123456789ABCDEF
    acc = be.up(np.array([start], np.uint64))
    be.call("ffh_state_digest", S.ptr, rows, rb, ld, seed, index_base, acc, None)
    got = int(be.fetch("acc", acc)[0])
    exp = (start + ffmodel.state_digest_reference(data, seed, index_base)) % 2 ** 64
    assert got == exp, f"digest {got:#x} against {exp:#x}"
    S.check()


# =====================================================================================================================================
# 6. numpy stand-ins of the entries the CPU oracle does not export (the CPU test's checker proof; same signatures without the ctx)
# =====================================================================================================================================
def _s_cross_fwd(be, y, ldy, x0, ldx0, v, ldv, xl, ldxl, batch, dim, s):
    m = lambda p, ld: view2(hostmem(p, (batch - 1) * ld + dim, np.float32), batch, dim, ld)
    m(y, ldy)[:] = ffmodel.cross_reference(m(x0, ldx0), m(v, ldv), m(xl, ldxl))


def _s_cross_bwd(be, dy, lddy, x0, ldx0, v, ldv, dv, lddv, dx0, lddx0, m0, dxl, lddxl, ml, batch, dim, s):
    m = lambda p, ld: view2(hostmem(p, (batch - 1) * ld + dim, np.float32), batch, dim, ld)
    assert m0 == ml == capi.CROSS_ADD
    g_dv, g0, gl = ffmodel.cross_reference_backward(m(dy, lddy), m(x0, ldx0), m(v, ldv), aliased=dx0 == dxl)
    with np.errstate(all="ignore"):
        m(dv, lddv)[:] = g_dv
        m(dx0, lddx0)[:] += g0
        if dx0 != dxl:
            m(dxl, lddxl)[:] += gl


def _s_sgd_lr(be, w, g, v, n, blk, wd, mom, nesterov, flags, s):
    return be.lib.lib.ffh_sgd_update_ex(be.lib.ctx, w, g, v, n, float(hostmem(blk, 2, np.float32)[0]), wd, mom, nesterov, flags, s)


def _s_adam_lr(be, w, g, m, v, n, blk, b1, b2, wd, eps, flags, s):
    return be.lib.lib.ffh_adam_update(be.lib.ctx, w, g, m, v, n, float(hostmem(blk, 2, np.float32)[1]), b1, b2, wd, eps, flags, s)


def _s_adagrad(be, w, g, S, n, lr, eps, wd, flags, s):
    wv, gv, Sv = hostmem(w, n, np.float32), hostmem(g, n, np.float32), hostmem(S, n, np.float32)
    wv[:], Sv[:] = ffmodel.adagrad_reference(wv.copy(), gv.copy(), Sv.copy(), lr, eps, wd)
    if flags & capi.OPT_ZERO_GRAD:
        gv[:] = 0


def _s_adagrad_lr(be, w, g, S, n, blk, eps, wd, flags, s):
    return _s_adagrad(be, w, g, S, n, float(hostmem(blk, 2, np.float32)[0]), eps, wd, flags, s)


def _s_metrics(be, lg, x, label, perf, bce_sum, ns, nc, scale, flags):
    p, y = hostmem(x, ns * nc, np.float32).reshape(ns, nc), hostmem(label, ns * nc, np.float32).reshape(ns, nc)
    if lg and bce_sum:
        hostmem(lg, ns * nc, np.float32)[:] = ((p - y) * np.float32(scale)).reshape(-1)
    elif lg:          # the oracle's own gradient (its sums are what the stand-in replaces)
        be.lib.check(be.lib.lib.ffh_mse_bwd(be.lib.ctx, lg, x, label, ns * nc, scale, None), "ffh_mse_bwd")
    pm = capi.PerfMetrics.from_address(perf)
    all_, correct = accuracy_rule(p, y)
    pm.train_all += all_; pm.train_correct += correct
    d = p.astype(np.float64) - y
    pm.mse_loss += (d * d).sum(); pm.rmse_loss += np.sqrt((d * d).sum(axis=1)).sum(); pm.mae_loss += np.abs(d).sum()
    if bce_sum:
        hostmem(bce_sum, 1, np.float32)[0] += bce_terms(p, y).sum()


def _s_bce(be, lg, prob, label, perf, bce_sum, ns, nc, scale, flags, s):
    _s_metrics(be, lg, prob, label, perf, bce_sum, ns, nc, scale, flags)


def _s_metrics_update(be, logits, labels, perf, ns, nc, flags, s):
    _s_metrics(be, 0, logits, labels, perf, 0, ns, nc, 0.0, flags)


def _s_mse_bwd_metrics(be, lg, logit, label, perf, ns, nc, scale, flags, s):
    _s_metrics(be, lg, logit, label, perf, 0, ns, nc, scale, flags)


def _s_ctr_eval(be, prob, label, ev, ns, s):
    p, y = hostmem(prob, ns, np.float32), hostmem(label, ns, np.float32)
    e = capi.CtrEval.from_address(ev)
    ok = ~np.isnan(p)
    pos = (y >= 0.5) & ok
    e.samples += int(ok.sum()); e.positives += int(pos.sum()); e.nan_predictions += int((~ok).sum())
    e.correct += int((((p >= 0.5) == (y >= 0.5)) & ok).sum())
    e.logloss_sum += bce_terms(p[ok], y[ok]).sum()
    bins = ctr_bins(p)
    np.ctypeslib.as_array(e.hist_pos)[:] += np.bincount(bins[pos], minlength=capi.AUC_BINS).astype(np.uint64)
    np.ctypeslib.as_array(e.hist_neg)[:] += np.bincount(bins[ok & ~pos], minlength=capi.AUC_BINS).astype(np.uint64)


def _s_digest(be, base, rows, rb, ld, seed, index_base, acc, s):
    data = view2(hostmem(base, (rows - 1) * (ld // 2) + rb // 2, np.uint16), rows, rb // 2, ld // 2)
    a = hostmem(acc, 1, np.uint64)
    a[0] = np.uint64((int(a[0]) + ffmodel.state_digest_reference(np.ascontiguousarray(data), seed, index_base)) % 2 ** 64)


STANDINS = {"ffh_cross_fwd": _s_cross_fwd, "ffh_cross_bwd": _s_cross_bwd, "ffh_sgd_update_ex_lr": _s_sgd_lr, "ffh_adam_update_lr": _s_adam_lr,
            "ffh_adagrad_update": _s_adagrad, "ffh_adagrad_update_lr": _s_adagrad_lr, "ffh_bce_bwd_metrics": _s_bce,
            "ffh_ctr_eval_update": _s_ctr_eval, "ffh_state_digest": _s_digest,
            # the oracle exports these two, but adds every sample into ONE serial float32 chain: past 65,536 samples its own rounding error
            # (2.5e-5 of the sum in the rmse of the `at` case) is beyond the 1e-5 the GPU's tree of partial sums is held to
            "ffh_metrics_update": _s_metrics_update, "ffh_mse_bwd_metrics": _s_mse_bwd_metrics}


# =====================================================================================================================================
# 7. the two wrong results the cases exist for, planted into what a run read back (Backend.tamper)
# =====================================================================================================================================
class Tamper:
    """mode "stale": everything the call changed past the first `keep` changed elements is left at its old value (a loop that never made
    its second trip).  mode "twice": the second trip applied twice -- an accumulate done two times, or, where the call only stores, the
    sentinel behind the last stored element overwritten.  .first[name]: the index the checker has to name."""

    def __init__(self, mode, keep):
        self.mode, self.keep, self.first = mode, keep, {}

    def __call__(self, name, got, initial):
        if name in self.first or got.dtype != initial.dtype or got.size != initial.size:
            return got
        idx = np.flatnonzero(_bits(got) != _bits(initial))
        if idx.size <= self.keep:
            return got
        tail = idx[self.keep:]
        flat = got.reshape(-1)
        if self.mode == "stale":
            flat[tail] = initial.reshape(-1)[tail]
            self.first[name] = int(tail[0])
            return got
        old = initial.reshape(-1)[tail]
        stored = flat.dtype != np.float32 or bool(np.all(_bits(old) == SENT32)) or bool(np.all(old == old[0]))
        if stored:
            if idx[-1] + 1 >= flat.size:
                return got
            flat[idx[-1] + 1] = flat[idx[-1]]
            self.first[name] = int(idx[-1] + 1)
        else:
            with np.errstate(all="ignore"):
                twice = flat[tail] + (flat[tail] - old)
            moved = np.flatnonzero((_bits(twice) != _bits(flat[tail])) & ~(np.isnan(twice) & np.isnan(flat[tail])))
            if not moved.size:
                return got
            flat[tail] = twice
            self.first[name] = int(tail[moved[0]])
        return got
