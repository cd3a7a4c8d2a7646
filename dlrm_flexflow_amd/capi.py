"""ctypes binding of the operator C-ABI declared in include/ff_hip.h.

`FFHLib(path)` loads ANY library that exports that ABI and declares every
prototype; `load_hip()` loads the product library (libffhip.so, hand-written
gfx950 HIP) and raises loudly when it has not been built -- there is no
fallback of any kind.  Pointers cross as integers (`tensor.data_ptr()` or
`ndarray.ctypes.data`), sizes as int64, streams as `void*`.

The reference binds its operators to Python through python/flexflow_c.h
(opaque handles + cffi, [ref: python/flexflow_c.h:24-42]); this file is the
equivalent stub for the kernel tier.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
HIP_LIB_PATH = os.path.join(_HERE, "csrc", "libffhip.so")
HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip.h")

FFH_OK = 0
FFH_ERR_BAD_ARG, FFH_ERR_HIP, FFH_ERR_UNSUPPORTED, FFH_ERR_WORKSPACE, FFH_ERR_NOMEM = -1, -2, -3, -4, -5
AC_MODE_NONE, AC_MODE_RELU, AC_MODE_SIGMOID, AC_MODE_TANH, AC_MODE_GELU = 10, 11, 12, 13, 14
AGGR_MODE_NONE, AGGR_MODE_SUM, AGGR_MODE_AVG = 20, 21, 22
MAX_TABLES = 64
EMB_CHUNK, EMB_CHUNK1 = 32, 1024
OPT_ZERO_GRAD = 1
CONCAT_BWD_OVERWRITE = 1
LINEAR_DX_OVERWRITE, LINEAR_ONLY_DW, LINEAR_ONLY_DX, LINEAR_DY_PREMASKED, LINEAR_DX_MASK_BY_X = 1, 2, 4, 8, 16
METRIC_ACCURACY, METRIC_MSE, METRIC_RMSE, METRIC_MAE = 1, 2, 4, 8

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
U64 = C.c_uint64
SZ = C.c_size_t


class EmbTable(C.Structure):
    """struct ffh_emb_table"""
    _fields_ = [("idx", P), ("weight", P), ("io", P), ("num_entries", L), ("ld", L)]


class EmbState(C.Structure):
    """struct ffh_emb_state: per-table optimizer state of the sparse (touched-rows) optimizers"""
    _fields_ = [("s0", P), ("s1", P)]


class SparseOpt(C.Structure):
    """struct ffh_sparse_opt"""
    _fields_ = [("kind", C.c_int32), ("lr", F), ("weight_decay", F), ("momentum", F), ("nesterov", C.c_int32),
                ("beta1", F), ("beta2", F), ("epsilon", F)]


SPARSE_OPT_SGD, SPARSE_OPT_SGD_MOMENTUM, SPARSE_OPT_ADAM = 0, 1, 2
SPARSE_OPT_ADAGRAD = 3      # include/ff_hip_adagrad.h: accepted by a library with the Adagrad extension
SPARSE_OPT_ROWWISE_ADAGRAD = 8      # include/ff_hip_rowwise.h: accepted by a library with the row-wise Adagrad extension (s0 = one float per row)


class PerfMetrics(C.Structure):
    """struct ffh_perf_metrics"""
    _fields_ = [("train_all", C.c_int32), ("train_correct", C.c_int32), ("cce_loss", F),
                ("sparse_cce_loss", F), ("mse_loss", F), ("rmse_loss", F), ("mae_loss", F),
                ("pad_", C.c_int32)]


class ChainLayer(C.Structure):
    """struct ffh_chain_layer"""
    _fields_ = [("w", P), ("bias", P), ("y", P), ("dy", P), ("dw", P), ("db", P), ("ldy", L), ("lddy", L),
                ("ldw", C.c_int32), ("in_dim", C.c_int32), ("out_dim", C.c_int32), ("activation", C.c_int32)]


class DeviceInfo(C.Structure):
    """struct ffh_device_info"""
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 64), ("compute_units", C.c_int32),
                ("wavefront_size", C.c_int32), ("total_mem_bytes", L), ("lds_bytes_per_cu", C.c_int32),
                ("clock_khz", C.c_int32)]


# name -> (restype, argtypes); ctx is always the first argument where present
_SIGS = {
    "ffh_abi_version": (I, []),
    "ffh_backend_name": (C.c_char_p, []),
    "ffh_ctx_create": (I, [C.POINTER(P), I]),
    "ffh_ctx_destroy": (I, [P]),
    "ffh_ctx_default": (I, [C.POINTER(P)]),
    "ffh_linear_last_route": (C.c_char_p, [P]),
    "ffh_embedding_last_route": (C.c_char_p, [P]),
    "ffh_last_error_string": (C.c_char_p, [P]),
    "ffh_device_query": (I, [P, C.POINTER(DeviceInfo)]),
    "ffh_ctx_set_workspace": (I, [P, P, SZ]),
    "ffh_ctx_set_math_mode": (I, [P, I]),
    "ffh_ctx_set_deterministic": (I, [P, I]),
    "ffh_ctx_set_dw_cu_reserve": (I, [P, I]),
    "ffh_ctx_reserve_scratch": (I, [P, P]),
    "ffh_ctx_bf16_mirror_set": (I, [P, P, SZ, P]),
    "ffh_ctx_bf16x3_mirror_set": (I, [P, P, SZ, P]),
    "ffh_convert_f32_to_bf16x3": (I, [P, P, L, L, L, P]),
    "ffh_convert_f32_to_bf16": (I, [P, P, P, L, P]),
    "ffh_malloc": (I, [P, C.POINTER(P), SZ]),
    "ffh_free": (I, [P, P]),
    "ffh_memcpy_h2d": (I, [P, P, P, SZ, P]),
    "ffh_memcpy_d2h": (I, [P, P, P, SZ, P]),
    "ffh_memcpy_d2d": (I, [P, P, P, SZ, P]),
    "ffh_stream_create": (I, [P, C.POINTER(P)]),
    "ffh_stream_create_with_priority": (I, [P, C.POINTER(P), I]),
    "ffh_stream_destroy": (I, [P, P]),
    "ffh_stream_sync": (I, [P, P]),
    "ffh_device_sync": (I, [P]),
    "ffh_event_create": (I, [P, C.POINTER(P)]),
    "ffh_event_create_sync": (I, [P, C.POINTER(P)]),
    "ffh_event_destroy": (I, [P, P]),
    "ffh_event_record": (I, [P, P, P]),
    "ffh_event_sync": (I, [P, P]),
    "ffh_stream_wait_event": (I, [P, P, P]),
    "ffh_event_elapsed_ms": (I, [P, P, P, C.POINTER(F)]),
    "ffh_graph_begin_capture": (I, [P, P]),
    "ffh_graph_end_capture": (I, [P, P, C.POINTER(P)]),
    "ffh_graph_launch": (I, [P, P, P]),
    "ffh_graph_destroy": (I, [P, P]),
    "ffh_fill_f32": (I, [P, P, L, F, P]),
    "ffh_zero": (I, [P, P, SZ, P]),
    "ffh_init_uniform": (I, [P, P, L, U64, F, F, P]),
    "ffh_gen_indices": (I, [P, P, L, U64, L, L, P]),
    "ffh_gen_uniform01": (I, [P, P, L, U64, L, P]),
    "ffh_gen_bernoulli": (I, [P, P, L, U64, L, P]),
    "ffh_embedding_fwd": (I, [P, P, P, P, I, I, L, L, L, I, P]),
    "ffh_embedding_fwd_multi": (I, [P, C.POINTER(EmbTable), I, I, I, L, I, P]),
    "ffh_embedding_bwd_dense": (I, [P, P, P, P, I, I, L, L, L, I, P]),
    "ffh_embedding_bwd_sgd_fused": (I, [P, P, P, P, I, I, L, L, L, I, F, P]),
    "ffh_embedding_bwd_sgd_fused_multi": (I, [P, C.POINTER(EmbTable), I, I, I, L, I, F, P]),
    "ffh_embedding_bwd_sort_multi": (I, [P, C.POINTER(EmbTable), I, I, I, L, P]),
    "ffh_embedding_bwd_sgd_apply_multi": (I, [P, C.POINTER(EmbTable), I, I, I, L, I, F, P]),
    "ffh_embedding_bwd_opt_fused_multi": (I, [P, C.POINTER(EmbTable), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), P]),
    "ffh_embedding_bwd_opt_apply_multi": (I, [P, C.POINTER(EmbTable), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), P]),
    "ffh_embedding_bwd_workspace_bytes": (SZ, [I, I, I, L]),
    "ffh_embedding_localize_rows": (I, [P, P, P, L, L, L, P]),
    "ffh_linear_fwd": (I, [P, P, L, P, L, P, P, I, I, L, I, P]),
    "ffh_linear_fast_in_dim": (I, [I, I]),
    "ffh_linear_bwd": (I, [P, P, L, P, L, P, L, P, L, P, P, P, I, I, L, I, P]),
    "ffh_linear_bwd_ex": (I, [P, P, L, P, L, P, L, P, L, P, P, P, I, I, L, I, I, P, P]),
    "ffh_linear_bwd_mse": (I, [P, P, L, P, L, P, L, P, L, P, P, P, I, I, L, I, I, P, F, P, I, P]),
    "ffh_linear_pair_bwd": (I, [P, P, L, P, L, P, L, P, P, P, I, I, I, I, P, L, P, L, P, L, P, I, I, I, L, P]),
    "ffh_linear_pair_fwd": (I, [P, P, L, P, P, I, I, P, L, I, P, P, I, I, P, L, L, P]),
    "ffh_mlp_chain_fwd": (I, [P, P, L, C.POINTER(ChainLayer), I, L, P]),
    "ffh_mlp_chain_bwd": (I, [P, P, L, P, L, C.POINTER(ChainLayer), I, L, I, P]),
    "ffh_second_stream_used": (I, [P, I]),
    "ffh_event_record_with_next_linear_bwd": (I, [P, P]),
    "ffh_linear_bwd_set_dx_scatter": (I, [P, P, I, P]),
    "ffh_linear_dx_scatter_used": (I, [P]),
    "ffh_linear_bwd_set_dx_colsum": (I, [P, P, I]),
    "ffh_linear_dx_colsum_used": (I, [P]),
    "ffh_mse_bwd_metrics": (I, [P, P, P, P, P, L, I, F, I, P]),
    "ffh_concat_fwd": (I, [P, P, L, C.POINTER(P), C.POINTER(L), C.POINTER(L), I, L, P]),
    "ffh_concat_bwd": (I, [P, P, L, C.POINTER(P), C.POINTER(L), C.POINTER(L), I, L, P]),
    "ffh_concat_bwd_ex": (I, [P, P, L, C.POINTER(P), C.POINTER(L), C.POINTER(L), I, L, I, P]),
    "ffh_bmm_fwd": (I, [P, P, P, P, I, I, I, L, I, I, I, P]),
    "ffh_bmm_bwd": (I, [P, P, P, P, P, P, I, I, I, L, P]),
    "ffh_transpose_fwd": (I, [P, P, P, I, C.POINTER(L), C.POINTER(I), P]),
    "ffh_transpose_bwd": (I, [P, P, P, I, C.POINTER(L), C.POINTER(I), P]),
    "ffh_tril_fwd": (I, [P, P, L, P, L, I, P]),
    "ffh_tril_bwd": (I, [P, P, P, L, L, I, P]),
    "ffh_dot_interaction_fwd": (I, [P, P, L, P, L, L, I, I, P]),
    "ffh_dot_interaction_bwd": (I, [P, P, L, P, L, P, L, L, I, I, I, P]),
    "ffh_mse_bwd": (I, [P, P, P, P, L, F, P]),
    "ffh_metrics_update": (I, [P, P, P, P, L, I, I, P]),
    "ffh_sgd_update": (I, [P, P, P, P, L, F, F, F, I, P]),
    "ffh_sgd_update_ex": (I, [P, P, P, P, L, F, F, F, I, I, P]),
    "ffh_adam_update": (I, [P, P, P, P, P, L, F, F, F, F, F, I, P]),
    "ffh_add_scaled": (I, [P, P, P, L, F, P]),
    "ffh_sum_slices_f32": (I, [P, P, P, I, L, L, P]),
}


def _header_symbols(header_path: str, prefix: str) -> list[str]:
    """Every symbol of the <prefix>_API_LIST X-macro of a header: include/ff_hip.h (prefix FFH) or an extension's (FFH_<X>)."""
    m = re.search(r"#define %s_API_LIST\(X\)(.*?)\n\n" % prefix, open(header_path).read(), re.S)
    if not m:
        raise RuntimeError(prefix + "_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def _header_abi_version(header_path: str, prefix: str) -> int:
    """<prefix>_ABI_VERSION of a header."""
    m = re.search(r"#define\s+%s_ABI_VERSION\s+(\d+)" % prefix, open(header_path).read())
    if not m:
        raise RuntimeError(prefix + "_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def header_symbols(header_path: str = HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_API_LIST X-macro in include/ff_hip.h."""
    return _header_symbols(header_path, "FFH")


def header_abi_version(header_path: str = HEADER_PATH) -> int:
    """FFH_ABI_VERSION of include/ff_hip.h."""
    return _header_abi_version(header_path, "FFH")


class FFHError(RuntimeError):
    pass


def ptr(x) -> int:
    """Device/host address of a torch tensor, numpy array, int or None."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    raise TypeError(f"cannot take the address of {type(x)}")


def _ctx_args(sigs: dict, name: str, args) -> list:
    """`args` as `name(ctx, *args)` of `sigs` takes them: the count checked, void pointers taken from tensors/arrays/ints/None."""
    sig = sigs[name][1][1:]
    if len(args) != len(sig):
        raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
    return [ptr(a) if t is P else a for a, t in zip(args, sig)]


class FFHLib:
    """A loaded library exporting include/ff_hip.h, plus one ctx."""

    def __init__(self, path: str, device: int = 0):
        if not os.path.exists(path):
            raise FFHError(f"{path} not found: build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path = path
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.lib, name)          # AttributeError => symbol missing => loud
            fn.restype = res
            fn.argtypes = args
        if self.lib.ffh_abi_version() != header_abi_version():
            raise FFHError(f"{path}: ABI version {self.lib.ffh_abi_version()}, include/ff_hip.h says {header_abi_version()} (rebuild)")
        self.backend = self.lib.ffh_backend_name().decode()
        ctx = P()
        rc = self.lib.ffh_ctx_create(C.byref(ctx), device)
        if rc != FFH_OK:
            raise FFHError(f"ffh_ctx_create failed ({rc}) on {path}")
        self.ctx = ctx
        self._ws_keepalive = None
        # tests and tools launch on the null stream: its scratch (stream-K slots ...) is reserved here, by the caller -- the library's
        # compute entry points never allocate
        self.check(self.lib.ffh_ctx_reserve_scratch(self.ctx, None), "ffh_ctx_reserve_scratch")

    # -- plumbing -----------------------------------------------------------
    def check(self, rc: int, what: str = ""):
        if rc != FFH_OK:
            msg = self.lib.ffh_last_error_string(self.ctx)
            raise FFHError(f"{what} failed: rc={rc}: {msg.decode() if msg else ''}")

    def call(self, name: str, *args):
        """Call `name(ctx, *args)`; pointers may be tensors/arrays/ints/None."""
        self.check(getattr(self.lib, name)(self.ctx, *_ctx_args(_SIGS, name, args)), name)

    def set_workspace(self, buf, nbytes: int):
        self._ws_keepalive = buf
        self.check(self.lib.ffh_ctx_set_workspace(self.ctx, ptr(buf), nbytes), "ffh_ctx_set_workspace")

    def device_info(self) -> DeviceInfo:
        info = DeviceInfo()
        self.check(self.lib.ffh_device_query(self.ctx, C.byref(info)), "ffh_device_query")
        return info

    def close(self):
        if self.ctx:
            self.lib.ffh_ctx_destroy(self.ctx)
            self.ctx = None

    # -- helpers for the array-taking entry points --------------------------
    @staticmethod
    def emb_tables(entries) -> "C.Array":
        """entries: iterable of (idx, weight, io, num_entries, ld)."""
        entries = list(entries)
        arr = (EmbTable * len(entries))()
        for k, (idx, w, io, r, ld) in enumerate(entries):
            arr[k] = EmbTable(ptr(idx), ptr(w), ptr(io), int(r), int(ld))
        return arr

    @staticmethod
    def emb_states(entries) -> "C.Array":
        """entries: iterable of (s0, s1) buffers (None where the optimizer kind has no such state)."""
        entries = list(entries)
        arr = (EmbState * len(entries))()
        for k, (s0, s1) in enumerate(entries):
            arr[k] = EmbState(ptr(s0), ptr(s1))
        return arr

    @staticmethod
    def chain_layers(entries) -> "C.Array":
        """entries: iterable of dicts with w, bias, y, dy, dw, db, ldy, lddy, ldw, in_dim, out_dim, activation (missing: None / 0)."""
        entries = list(entries)
        arr = (ChainLayer * len(entries))()
        for k, e in enumerate(entries):
            arr[k] = ChainLayer(ptr(e.get("w")), ptr(e.get("bias")), ptr(e.get("y")), ptr(e.get("dy")), ptr(e.get("dw")), ptr(e.get("db")),
                                int(e.get("ldy", e["out_dim"])), int(e.get("lddy", e["out_dim"])), int(e.get("ldw", e["in_dim"])),
                                int(e["in_dim"]), int(e["out_dim"]), int(e["activation"]))
        return arr

    def transpose(self, name: str, dst, src, in_dims, perm, stream=None):
        n = len(in_dims)
        da = (L * n)(*[int(v) for v in in_dims])
        pa = (I * n)(*[int(v) for v in perm])
        self.check(getattr(self.lib, name)(self.ctx, ptr(dst), ptr(src), n, da, pa, ptr(stream)), name)

    def concat(self, name: str, big, out_blk: int, parts, in_blk, in_ld, num_blocks: int, stream=None):
        n = len(parts)
        pa = (P * n)(*[ptr(p) for p in parts])
        ba = (L * n)(*[int(v) for v in in_blk])
        la = (L * n)(*[int(v) for v in in_ld]) if in_ld is not None else None
        self.check(getattr(self.lib, name)(self.ctx, ptr(big), out_blk, pa, ba, la, n, num_blocks, ptr(stream)), name)


# ---- the optional extensions (include/ff_hip_<x>.h): each has a list and a version of its own; libffhip.so exports them, the oracle does not ----
class Extension:
    """What differs between the optional extensions: the header (and with it the macro prefix and the version symbol), the signatures, and the
    labels of the two messages.  The blocks below hold one each, in the order the host layer loads them (host/backend.h, FFH_EXTENSIONS)."""

    def __init__(self, key: str, sigs: dict, label: str, version_label: str | None = None):
        self.key = key                                        # bags_update: include/ff_hip_bags_update.h, FFH_BAGS_UPDATE_*, ffh_bags_update_abi_version
        self.header = f"include/ff_hip_{key}.h"
        self.header_path = os.path.join(REPO_ROOT, "include", f"ff_hip_{key}.h")
        self.prefix = "FFH_" + key.upper()
        self.version_symbol = f"ffh_{key}_abi_version"
        self.sigs = sigs
        self.label = label                                    # "no <label> extension"
        self.version_label = version_label or label           # "<label> ABI version ..."

    def header_symbols(self, header_path: str | None = None) -> list[str]:
        """Every symbol of the extension's FFH_<X>_API_LIST X-macro."""
        return _header_symbols(header_path or self.header_path, self.prefix)

    def header_abi_version(self, header_path: str | None = None) -> int:
        """The extension's FFH_<X>_ABI_VERSION."""
        return _header_abi_version(header_path or self.header_path, self.prefix)


EXTENSIONS: dict[str, Extension] = {}


def _extension(key: str, sigs: dict, label: str, version_label: str | None = None) -> Extension:
    EXTENSIONS[key] = Extension(key, sigs, label, version_label)
    return EXTENSIONS[key]


class ExtensionApi:
    """An extension of a loaded FFHLib, by the one rule: absent is an FFHError (e.g. on the CPU oracle); present means every symbol of the
    extension's signatures and the header's version.  A subclass names its extension (`ext`) and adds the helpers of its own; `<x>_api(lib)`
    builds it or raises."""
    ext: Extension

    def __init__(self, lib: FFHLib):
        e = self.ext
        self.base = lib
        for name, (res, args) in e.sigs.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no {e.label} extension ({name} missing; {e.header})")
            fn.restype = res
            fn.argtypes = args
        got, want = getattr(lib.lib, e.version_symbol)(), e.header_abi_version()
        if got != want:
            raise FFHError(f"{lib.path}: {e.version_label} ABI version {got}, {e.header} says {want} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def rc(self, name: str, *args) -> int:
        """`name(ctx, *args)` of the extension, returning its status code (FFH_OK, FFH_ERR_UNSUPPORTED, ...); pointers may be tensors / arrays /
        ints / None, struct arrays as the subclass builds them."""
        return getattr(self.lib, name)(self.ctx, *_ctx_args(self.ext.sigs, name, args))

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; FFHError unless it returns FFH_OK."""
        self.base.check(self.rc(name, *args), name)


# ---- the bf16-table extension (include/ff_hip_bf16.h) -------------------------------------------------------------------------------------
BF16_ROUND_STOCHASTIC, BF16_ROUND_NEAREST = 0, 1


class EmbTableBf16(C.Structure):
    """struct ffh_emb_table_bf16"""
    _fields_ = [("idx", P), ("weight", P), ("io", P), ("num_entries", L), ("ld", L), ("table", C.c_int32), ("col0", C.c_int32)]


class Bf16Rounding(C.Structure):
    """struct ffh_bf16_rounding"""
    _fields_ = [("mode", C.c_int32), ("reserved_", C.c_int32), ("seed", U64), ("counter", P)]


_SIGS_BF16 = {
    "ffh_bf16_abi_version": (I, []),
    "ffh_embedding_fwd_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), I, I, I, L, I, P]),
    "ffh_embedding_bwd_sgd_fused_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), I, I, I, L, I, F, C.POINTER(Bf16Rounding), P]),
    "ffh_embedding_bwd_sort_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), I, I, I, L, P]),
    "ffh_embedding_bwd_sgd_apply_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), I, I, I, L, I, F, C.POINTER(Bf16Rounding), P]),
    "ffh_init_uniform_bf16": (I, [P, P, L, U64, F, F, P]),
    "ffh_bf16_counter_advance": (I, [P, P, P]),
    "ffh_embedding_bwd_opt_fused_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), C.POINTER(Bf16Rounding), P]),
    "ffh_embedding_bwd_opt_apply_multi_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), C.POINTER(Bf16Rounding), P]),
}
BF16_EXT = _extension("bf16", _SIGS_BF16, "bf16-table", version_label="bf16")
BF16_HEADER_PATH, bf16_header_symbols, bf16_header_abi_version = BF16_EXT.header_path, BF16_EXT.header_symbols, BF16_EXT.header_abi_version


class Bf16Api(ExtensionApi):
    ext = BF16_EXT

    @staticmethod
    def tables(entries) -> "C.Array":
        """entries: iterable of (idx, weight, io, num_entries, ld[, table[, col0]]); `table` defaults to the entry's position."""
        entries = list(entries)
        arr = (EmbTableBf16 * len(entries))()
        for k, e in enumerate(entries):
            idx, w, io, r, ld = e[:5]
            table = int(e[5]) if len(e) > 5 else k
            col0 = int(e[6]) if len(e) > 6 else 0
            arr[k] = EmbTableBf16(ptr(idx), ptr(w), ptr(io), int(r), int(ld), table, col0)
        return arr

    @staticmethod
    def rounding(mode: int = BF16_ROUND_STOCHASTIC, seed: int = 0, counter=None) -> Bf16Rounding:
        return Bf16Rounding(int(mode), 0, int(seed) & (2**64 - 1), ptr(counter))


bf16_api = Bf16Api


# ---- the CTR extension (include/ff_hip_ctr.h): binary cross-entropy, evaluation histograms ------------------------------------------------
METRIC_BCE = 16
AUC_BINS = 65536


class CtrEval(C.Structure):
    """struct ffh_ctr_eval"""
    _fields_ = [("samples", U64), ("positives", U64), ("correct", U64), ("nan_predictions", U64), ("logloss_sum", F), ("pad_", F * 3),
                ("hist_pos", U64 * AUC_BINS), ("hist_neg", U64 * AUC_BINS)]


_SIGS_CTR = {
    "ffh_ctr_abi_version": (I, []),
    "ffh_bce_bwd_metrics": (I, [P, P, P, P, P, P, L, I, F, I, P]),
    "ffh_linear_bwd_bce": (I, [P, P, L, P, L, P, L, P, L, P, P, P, I, I, L, I, I, P, F, P, P, I, P]),
    "ffh_ctr_eval_update": (I, [P, P, P, P, L, P]),
}
CTR_EXT = _extension("ctr", _SIGS_CTR, "CTR")
CTR_HEADER_PATH, ctr_header_symbols, ctr_header_abi_version = CTR_EXT.header_path, CTR_EXT.header_symbols, CTR_EXT.header_abi_version


class CtrApi(ExtensionApi):
    ext = CTR_EXT


ctr_api = CtrApi


# ---- the learning-rate extension (include/ff_hip_lr.h): schedule state in device memory, optimizer entries that read it -------------------

class LrSchedule(C.Structure):
    """struct ffh_lr_schedule"""
    _fields_ = [("base", C.c_double), ("warmup_steps", L), ("decay_start", L), ("decay_steps", L), ("beta1", C.c_double), ("beta2", C.c_double)]


class LrValues(C.Structure):
    """struct ffh_lr_values"""
    _fields_ = [("k", L), ("lr", F), ("alpha_t", F), ("beta1_t", C.c_double), ("beta2_t", C.c_double)]


_SIGS_LR = {
    "ffh_lr_abi_version": (I, []),
    "ffh_lr_state_bytes": (SZ, []),
    "ffh_lr_state_init": (I, [P, P, C.POINTER(LrSchedule), L, P]),
    "ffh_lr_state_advance": (I, [P, P, P]),
    "ffh_lr_state_read": (I, [P, P, C.POINTER(LrValues), P]),
    "ffh_sgd_update_ex_lr": (I, [P, P, P, P, L, P, F, F, I, I, P]),
    "ffh_adam_update_lr": (I, [P, P, P, P, P, L, P, F, F, F, F, I, P]),
    "ffh_embedding_bwd_opt_fused_multi_lr": (I, [P, C.POINTER(EmbTable), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), P, P]),
    "ffh_embedding_bwd_opt_apply_multi_lr": (I, [P, C.POINTER(EmbTable), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), P, P]),
    "ffh_embedding_bwd_opt_fused_multi_bf16_lr": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), C.POINTER(Bf16Rounding), P, P]),
    "ffh_embedding_bwd_opt_apply_multi_bf16_lr": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(EmbState), I, I, I, L, I, C.POINTER(SparseOpt), C.POINTER(Bf16Rounding), P, P]),
}
LR_EXT = _extension("lr", _SIGS_LR, "learning-rate")
LR_HEADER_PATH, lr_header_symbols, lr_header_abi_version = LR_EXT.header_path, LR_EXT.header_symbols, LR_EXT.header_abi_version


class LrApi(ExtensionApi):
    ext = LR_EXT

    def state_bytes(self) -> int:
        return int(self.lib.ffh_lr_state_bytes())

    def init(self, block, base, W=0, S=0, N=0, beta1=0.0, beta2=0.0, first_step=0, stream=None):
        sc = LrSchedule(float(base), int(W), int(S), int(N), float(beta1), float(beta2))
        self.call("ffh_lr_state_init", block, C.byref(sc), int(first_step), stream)

    def read(self, block, stream=None) -> LrValues:
        v = LrValues()
        self.call("ffh_lr_state_read", block, C.byref(v), stream)
        return v


lr_api = LrApi


# ---- the data extension (include/ff_hip_data.h): one shuffled training batch gathered in one launch ----------------------------------------
GATHER_LOCAL_ROWS, GATHER_GLOBAL_ROWS = 0, 1
GATHER_MAX_SEGMENTS = 64


class GatherSegment(C.Structure):
    """struct ffh_gather_segment"""
    _fields_ = [("src", P), ("dst", P), ("row_bytes", C.c_int32), ("kind", C.c_int32)]


class BatchOrder(C.Structure):
    """struct ffh_batch_order"""
    _fields_ = [("seed", U64), ("epoch", L), ("step", L), ("local_batch", L), ("n_local", L), ("world", C.c_int32), ("rank", C.c_int32)]


_SIGS_DATA = {
    "ffh_data_abi_version": (I, []),
    "ffh_batch_gather": (I, [P, C.POINTER(GatherSegment), I, C.POINTER(BatchOrder), P]),
}
DATA_EXT = _extension("data", _SIGS_DATA, "data")
DATA_HEADER_PATH, data_header_symbols, data_header_abi_version = DATA_EXT.header_path, DATA_EXT.header_symbols, DATA_EXT.header_abi_version


class DataApi(ExtensionApi):
    ext = DATA_EXT

    def batch_gather_rc(self, segments, seed, epoch, step, local_batch, n_local, world=1, rank=0, stream=None) -> int:
        """ffh_batch_gather; `segments`: (src, dst, row_bytes, kind) tuples, pointers as tensors/arrays/ints/None.  Returns the status code."""
        arr = (GatherSegment * max(1, len(segments)))()
        for k, (src, dst, row_bytes, kind) in enumerate(segments):
            arr[k] = GatherSegment(ptr(src), ptr(dst), int(row_bytes), int(kind))
        order = BatchOrder(int(seed) & (2**64 - 1), int(epoch), int(step), int(local_batch), int(n_local), int(world), int(rank))
        return self.lib.ffh_batch_gather(self.ctx, arr, len(segments), C.byref(order), ptr(stream))

    def batch_gather(self, segments, seed, epoch, step, local_batch, n_local, world=1, rank=0, stream=None):
        self.base.check(self.batch_gather_rc(segments, seed, epoch, step, local_batch, n_local, world, rank, stream), "ffh_batch_gather")


data_api = DataApi


# ---- the cross extension (include/ff_hip_cross.h): the elementwise combine of a DCNv2 low-rank cross layer --------------------------------
CROSS_SKIP, CROSS_STORE, CROSS_ADD = 0, 1, 2

_SIGS_CROSS = {
    "ffh_cross_abi_version": (I, []),
    "ffh_cross_fwd": (I, [P, P, L, P, L, P, L, P, L, L, L, P]),
    "ffh_cross_bwd": (I, [P, P, L, P, L, P, L, P, L, P, L, I, P, L, I, L, L, P]),
}
CROSS_EXT = _extension("cross", _SIGS_CROSS, "cross")
CROSS_HEADER_PATH, cross_header_symbols, cross_header_abi_version = CROSS_EXT.header_path, CROSS_EXT.header_symbols, CROSS_EXT.header_abi_version


class CrossApi(ExtensionApi):
    ext = CROSS_EXT


cross_api = CrossApi


# ---- the digest extension (include/ff_hip_digest.h): a 64-bit digest of a strided device buffer -------------------------------------------
_SIGS_DIGEST = {
    "ffh_digest_abi_version": (I, []),
    "ffh_state_digest": (I, [P, P, L, L, L, C.c_uint64, C.c_uint64, P, P]),
}
DIGEST_EXT = _extension("digest", _SIGS_DIGEST, "digest")
DIGEST_HEADER_PATH, digest_header_symbols, digest_header_abi_version = DIGEST_EXT.header_path, DIGEST_EXT.header_symbols, DIGEST_EXT.header_abi_version


class DigestApi(ExtensionApi):
    ext = DIGEST_EXT

    def state_digest_rc(self, base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream=None) -> int:
        """ffh_state_digest, returning its status code (FFH_OK, FFH_ERR_BAD_ARG, ...): *acc += the digest."""
        m64 = 2 ** 64 - 1
        return self.lib.ffh_state_digest(self.ctx, ptr(base), int(rows), int(row_bytes), int(ld_bytes), int(seed) & m64, int(index_base) & m64, ptr(acc),
                                         ptr(stream))

    def state_digest(self, base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream=None):
        self.base.check(self.state_digest_rc(base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream), "ffh_state_digest")


digest_api = DigestApi


# ---- the Adagrad extension (include/ff_hip_adagrad.h): the dense launch; FFH_SPARSE_OPT_ADAGRAD in the table update -----------------------
_SIGS_ADAGRAD = {
    "ffh_adagrad_abi_version": (I, []),
    "ffh_adagrad_update": (I, [P, P, P, P, L, F, F, F, I, P]),
    "ffh_adagrad_update_lr": (I, [P, P, P, P, L, P, F, F, I, P]),
}
ADAGRAD_EXT = _extension("adagrad", _SIGS_ADAGRAD, "Adagrad")
ADAGRAD_HEADER_PATH, adagrad_header_symbols, adagrad_header_abi_version = ADAGRAD_EXT.header_path, ADAGRAD_EXT.header_symbols, ADAGRAD_EXT.header_abi_version


class AdagradApi(ExtensionApi):
    ext = ADAGRAD_EXT


adagrad_api = AdagradApi


# ---- the row-wise Adagrad extension (include/ff_hip_rowwise.h): FFH_SPARSE_OPT_ROWWISE_ADAGRAD in the table update; no launch of its own ----
_SIGS_ROWWISE = {
    "ffh_rowwise_abi_version": (I, []),
}
ROWWISE_EXT = _extension("rowwise", _SIGS_ROWWISE, "row-wise Adagrad")
ROWWISE_HEADER_PATH, rowwise_header_symbols, rowwise_header_abi_version = ROWWISE_EXT.header_path, ROWWISE_EXT.header_symbols, ROWWISE_EXT.header_abi_version


class RowwiseApi(ExtensionApi):
    """The rule itself is reached through the table update's entry points of `lib` with SparseOpt.kind = SPARSE_OPT_ROWWISE_ADAGRAD."""
    ext = ROWWISE_EXT


rowwise_api = RowwiseApi


# ---- the fold extension (include/ff_hip_fold.h): small embedding tables folded out of the first top layer's forward GEMM --------------------
class FoldGroup(C.Structure):
    """struct ffh_fold_group"""
    _fields_ = [("e", P), ("lde", L), ("col0", L), ("p", P), ("rows", L)]


class FoldSeg(C.Structure):
    """struct ffh_fold_seg"""
    _fields_ = [("k0", C.c_int32), ("len", C.c_int32)]


_SIGS_FOLD = {
    "ffh_fold_abi_version": (I, []),
    "ffh_fold_product": (I, [P, C.POINTER(FoldGroup), I, P, L, I, I, P]),
    "ffh_fold_gather_add": (I, [P, C.POINTER(EmbTable), I, I, I, L, I, P, L, P]),
    "ffh_fold_linear_fwd": (I, [P, P, L, P, L, P, P, I, I, L, I, C.POINTER(FoldSeg), I, P, L, P]),
    "ffh_fold_linear_fwd_plan": (I, [P, P, L, P, L, P, P, I, I, L, C.POINTER(FoldSeg), I, P, L]),
    "ffh_fold_segment_sum": (I, [P, C.POINTER(EmbTable), I, I, I, L, P]),
    "ffh_fold_dw_product": (I, [P, C.POINTER(FoldGroup), I, P, L, I, I, P]),
    "ffh_fold_linear_bwd_dw": (I, [P, P, L, P, L, P, P, I, I, L, C.POINTER(C.c_int32), I, P]),
    "ffh_fold_linear_bwd_dw_plan": (I, [P, P, L, P, L, P, P, I, I, L, C.POINTER(C.c_int32), I]),
    # ABI 3: the data gradient over kept column tiles (x, ldx, dx, lddx, dy, lddy, w, in, out, batch, flags, kept, nkept, colsum, event, stream)
    "ffh_fold_linear_bwd_dx": (I, [P, P, L, P, L, P, L, P, I, I, L, I, C.POINTER(C.c_int32), I, P, P, P]),
    "ffh_fold_linear_bwd_dx_plan": (I, [P, P, L, P, L, P, L, P, I, I, L, I, C.POINTER(C.c_int32), I, P]),
    "ffh_fold_table_update": (I, [P, C.POINTER(FoldGroup), I, P, L, I, I, C.c_float, P]),
    "ffh_fold_table_update_lr": (I, [P, C.POINTER(FoldGroup), I, P, L, I, I, P, P]),
}
FOLD_EXT = _extension("fold", _SIGS_FOLD, "fold")
FOLD_HEADER_PATH, fold_header_symbols, fold_header_abi_version = FOLD_EXT.header_path, FOLD_EXT.header_symbols, FOLD_EXT.header_abi_version


class FoldApi(ExtensionApi):
    ext = FOLD_EXT

    @staticmethod
    def groups(entries) -> "C.Array":
        """entries: iterable of (e, lde, col0, p, rows)."""
        entries = list(entries)
        arr = (FoldGroup * len(entries))()
        for k, (e, lde, col0, p, rows) in enumerate(entries):
            arr[k] = FoldGroup(ptr(e), int(lde), int(col0), ptr(p), int(rows))
        return arr

    @staticmethod
    def segs(entries) -> "C.Array":
        """entries: iterable of (k0, len); an empty list gives a one-element array nobody reads (pass nkeep = 0)."""
        entries = list(entries)
        arr = (FoldSeg * max(1, len(entries)))()
        for k, (k0, n) in enumerate(entries):
            arr[k] = FoldSeg(int(k0), int(n))
        return arr


fold_api = FoldApi


# ---- the bags extension (include/ff_hip_bags.h): the gather with a bag size per table, one launch ------------------------------------------
BAGS_MAX_IN_DIM = 65535

_SIGS_BAGS = {
    "ffh_bags_abi_version": (I, []),
    "ffh_bags_kernarg_bytes": (SZ, []),
    "ffh_embedding_fwd_multi_bags": (I, [P, C.POINTER(EmbTable), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(I), I, I, L, I, P]),
}
BAGS_EXT = _extension("bags", _SIGS_BAGS, "bags")
BAGS_HEADER_PATH, bags_header_symbols, bags_header_abi_version = BAGS_EXT.header_path, BAGS_EXT.header_symbols, BAGS_EXT.header_abi_version


class BagsApi(ExtensionApi):
    ext = BAGS_EXT

    @staticmethod
    def in_dims(sizes) -> "C.Array":
        """The `in_dims` argument: one C int per table."""
        sizes = [int(v) for v in sizes]
        return (I * max(1, len(sizes)))(*sizes)

    def rc(self, name: str, tables, in_dims, ntables: int, out_dim: int, batch: int, aggr: int, stream=None) -> int:
        """`name(ctx, tables, in_dims, ...)`, returning its status code; `tables` from FFHLib.emb_tables / Bf16Api.tables, `in_dims` from
        BagsApi.in_dims (or None: a null pointer)."""
        return getattr(self.lib, name)(self.ctx, tables, in_dims, int(ntables), int(out_dim), int(batch), int(aggr), ptr(stream))

    def call(self, name: str, *args, **kw):
        self.base.check(self.rc(name, *args, **kw), name)


bags_api = BagsApi


# ---- the bags-update extension (include/ff_hip_bags_update.h): the fused table update with a bag size per table, one call -----------------
BAGS_UPDATE_MAX_TABLES = MAX_TABLES


class BagsUpdate(C.Structure):
    """struct ffh_bags_update"""
    _fields_ = [("tables", C.POINTER(EmbTable)), ("tables_bf16", C.POINTER(EmbTableBf16)), ("in_dims", C.POINTER(I)),
                ("states", C.POINTER(EmbState)), ("ntables", I), ("out_dim", I), ("batch", L), ("aggr", I), ("lr", F),
                ("opt", C.POINTER(SparseOpt)), ("rounding", C.POINTER(Bf16Rounding)), ("lr_block", P)]


_SIGS_BAGS_UPDATE = {
    "ffh_bags_update_abi_version": (I, []),
    "ffh_bags_update_kernarg_bytes": (SZ, []),
    "ffh_embedding_bwd_bags_workspace_bytes": (SZ, [C.POINTER(I), I, I, L]),
    "ffh_embedding_bwd_fused_multi_bags": (I, [P, C.POINTER(BagsUpdate), P]),
}
BAGS_UPDATE_EXT = _extension("bags_update", _SIGS_BAGS_UPDATE, "bags-update")
BAGS_UPDATE_HEADER_PATH, bags_update_header_symbols, bags_update_header_abi_version = (
    BAGS_UPDATE_EXT.header_path, BAGS_UPDATE_EXT.header_symbols, BAGS_UPDATE_EXT.header_abi_version)


class BagsUpdateApi(ExtensionApi):
    ext = BAGS_UPDATE_EXT

    def kernarg_bytes(self) -> int:
        return int(self.lib.ffh_bags_update_kernarg_bytes())

    def workspace_bytes(self, in_dims, out_dim: int, batch: int, ntables: int | None = None) -> int:
        """ffh_embedding_bwd_bags_workspace_bytes (host arithmetic); `in_dims`: a list of bag sizes, or None for a null pointer."""
        arr = None if in_dims is None else BagsApi.in_dims(in_dims)
        nt = len(in_dims) if ntables is None else ntables
        return int(self.lib.ffh_embedding_bwd_bags_workspace_bytes(arr, int(nt), int(out_dim), int(batch)))

    @staticmethod
    def descriptor(*, in_dims, out_dim: int, batch: int, aggr: int, tables=None, tables_bf16=None, states=None, ntables: int | None = None,
                   lr: float = 0.0, opt: SparseOpt | None = None, rounding: Bf16Rounding | None = None, lr_block=None) -> BagsUpdate:
        """A struct ffh_bags_update.  `tables` from FFHLib.emb_tables, `tables_bf16` from Bf16Api.tables, `states` from FFHLib.emb_states,
        `in_dims` a list of bag sizes (or None: a null pointer), `lr_block` a device buffer.  The descriptor keeps its arrays alive."""
        u = BagsUpdate()
        keep = [tables, tables_bf16, states, opt, rounding, lr_block]
        if tables is not None:
            u.tables = C.cast(tables, C.POINTER(EmbTable))
        if tables_bf16 is not None:
            u.tables_bf16 = C.cast(tables_bf16, C.POINTER(EmbTableBf16))
        if in_dims is not None:
            arr = BagsApi.in_dims(in_dims)
            keep.append(arr)
            u.in_dims = C.cast(arr, C.POINTER(I))
        if states is not None:
            u.states = C.cast(states, C.POINTER(EmbState))
        u.ntables = int(len(in_dims) if ntables is None else ntables)
        u.out_dim, u.batch, u.aggr, u.lr = int(out_dim), int(batch), int(aggr), float(lr)
        if opt is not None:
            u.opt = C.pointer(opt)
        if rounding is not None:
            u.rounding = C.pointer(rounding)
        u.lr_block = ptr(lr_block)
        u._keep = keep
        return u

    def rc(self, u: BagsUpdate | None, stream=None) -> int:
        """ffh_embedding_bwd_fused_multi_bags, returning its status code."""
        return self.lib.ffh_embedding_bwd_fused_multi_bags(self.ctx, C.byref(u) if u is not None else None, ptr(stream))

    def call(self, u: BagsUpdate, stream=None):
        self.base.check(self.rc(u, stream), "ffh_embedding_bwd_fused_multi_bags")


bags_update_api = BagsUpdateApi


# ---- the bags-sort extension (include/ff_hip_bags_sort.h): the ragged update in two calls, sort (ids only) then apply ----------------------
_SIGS_BAGS_SORT = {
    "ffh_bags_sort_abi_version": (I, []),
    "ffh_embedding_bwd_sort_multi_bags": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_apply_multi_bags": (I, [P, C.POINTER(BagsUpdate), P]),
}
BAGS_SORT_EXT = _extension("bags_sort", _SIGS_BAGS_SORT, "bags-sort")
BAGS_SORT_HEADER_PATH, bags_sort_header_symbols, bags_sort_header_abi_version = (
    BAGS_SORT_EXT.header_path, BAGS_SORT_EXT.header_symbols, BAGS_SORT_EXT.header_abi_version)


class BagsSortApi(ExtensionApi):
    """Both calls take the descriptor of the fused ragged update (BagsUpdateApi.descriptor)."""
    ext = BAGS_SORT_EXT

    def sort_rc(self, u: BagsUpdate | None, stream=None) -> int:
        """ffh_embedding_bwd_sort_multi_bags, returning its status code."""
        return self.lib.ffh_embedding_bwd_sort_multi_bags(self.ctx, C.byref(u) if u is not None else None, ptr(stream))

    def apply_rc(self, u: BagsUpdate | None, stream=None) -> int:
        """ffh_embedding_bwd_apply_multi_bags, returning its status code."""
        return self.lib.ffh_embedding_bwd_apply_multi_bags(self.ctx, C.byref(u) if u is not None else None, ptr(stream))

    def sort(self, u: BagsUpdate, stream=None):
        self.base.check(self.sort_rc(u, stream), "ffh_embedding_bwd_sort_multi_bags")

    def apply(self, u: BagsUpdate, stream=None):
        self.base.check(self.apply_rc(u, stream), "ffh_embedding_bwd_apply_multi_bags")


bags_sort_api = BagsSortApi


# ---- the pad extension (include/ff_hip_pad.h): variable-length bags, the id EMB_PAD_ID being "no lookup" ---------------------------------
EMB_PAD_ID = -1

_SIGS_PAD = {
    "ffh_pad_abi_version": (I, []),
    "ffh_embedding_fwd_multi_bags_pad": (I, [P, C.POINTER(EmbTable), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_pad_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_bwd_fused_multi_bags_pad": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_sort_multi_bags_pad": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_apply_multi_bags_pad": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_pad_mask_indices": (I, [P, P, L, C.c_uint64, L, F, P]),
}
PAD_EXT = _extension("pad", _SIGS_PAD, "pad")
PAD_HEADER_PATH, pad_header_symbols, pad_header_abi_version = PAD_EXT.header_path, PAD_EXT.header_symbols, PAD_EXT.header_abi_version


class PadApi(ExtensionApi):
    """The gathers take the arguments of BagsApi.rc, the update entries the descriptor of the ragged update (BagsUpdateApi.descriptor)."""
    ext = PAD_EXT

    def fwd_rc(self, tables, in_dims, ntables: int, out_dim: int, batch: int, aggr: int, bf16: bool = False, stream=None) -> int:
        """ffh_embedding_fwd_multi_bags_pad[_bf16], returning its status code; `in_dims` from BagsApi.in_dims (or None: a null pointer)."""
        fn = self.lib.ffh_embedding_fwd_multi_bags_pad_bf16 if bf16 else self.lib.ffh_embedding_fwd_multi_bags_pad
        return fn(self.ctx, tables, in_dims, int(ntables), int(out_dim), int(batch), int(aggr), ptr(stream))

    def fwd(self, *args, **kw):
        self.base.check(self.fwd_rc(*args, **kw), "ffh_embedding_fwd_multi_bags_pad")

    def _u(self, name: str, u: BagsUpdate | None, stream) -> int:
        return getattr(self.lib, name)(self.ctx, C.byref(u) if u is not None else None, ptr(stream))

    def fused_rc(self, u: BagsUpdate | None, stream=None) -> int:
        return self._u("ffh_embedding_bwd_fused_multi_bags_pad", u, stream)

    def sort_rc(self, u: BagsUpdate | None, stream=None) -> int:
        return self._u("ffh_embedding_bwd_sort_multi_bags_pad", u, stream)

    def apply_rc(self, u: BagsUpdate | None, stream=None) -> int:
        return self._u("ffh_embedding_bwd_apply_multi_bags_pad", u, stream)

    def fused(self, u: BagsUpdate, stream=None):
        self.base.check(self.fused_rc(u, stream), "ffh_embedding_bwd_fused_multi_bags_pad")

    def sort(self, u: BagsUpdate, stream=None):
        self.base.check(self.sort_rc(u, stream), "ffh_embedding_bwd_sort_multi_bags_pad")

    def apply(self, u: BagsUpdate, stream=None):
        self.base.check(self.apply_rc(u, stream), "ffh_embedding_bwd_apply_multi_bags_pad")

    def mask_rc(self, idx, count: int, seed: int, first: int, fill: float, stream=None) -> int:
        """ffh_pad_mask_indices on a device buffer of int64 ids, returning its status code."""
        return self.lib.ffh_pad_mask_indices(self.ctx, ptr(idx), int(count), int(seed) & (2**64 - 1), int(first), float(fill), ptr(stream))

    def mask(self, *args, **kw):
        self.base.check(self.mask_rc(*args, **kw), "ffh_pad_mask_indices")


pad_api = PadApi


# ---- the pad-mean extension (include/ff_hip_pad_mean.h): the pad entries with a mean over the lookups that are there ---------------------
_SIGS_PAD_MEAN = {
    "ffh_pad_mean_abi_version": (I, []),
    "ffh_embedding_fwd_multi_bags_pad_mean": (I, [P, C.POINTER(EmbTable), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_pad_mean_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_bwd_bags_pad_mean_workspace_bytes": (SZ, [C.POINTER(I), I, I, L]),
    "ffh_embedding_bwd_fused_multi_bags_pad_mean": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_apply_multi_bags_pad_mean": (I, [P, C.POINTER(BagsUpdate), P]),
}
PAD_MEAN_EXT = _extension("pad_mean", _SIGS_PAD_MEAN, "pad-mean")
PAD_MEAN_HEADER_PATH, pad_mean_header_symbols, pad_mean_header_abi_version = (
    PAD_MEAN_EXT.header_path, PAD_MEAN_EXT.header_symbols, PAD_MEAN_EXT.header_abi_version)


class PadMeanApi(ExtensionApi):
    """PadApi's methods without the sort (the pad sort serves either apply), and the workspace query of the update."""
    ext = PAD_MEAN_EXT

    def fwd_rc(self, tables, in_dims, ntables: int, out_dim: int, batch: int, aggr: int, bf16: bool = False, stream=None) -> int:
        """ffh_embedding_fwd_multi_bags_pad_mean[_bf16], returning its status code; `in_dims` from BagsApi.in_dims (or None: a null pointer)."""
        fn = self.lib.ffh_embedding_fwd_multi_bags_pad_mean_bf16 if bf16 else self.lib.ffh_embedding_fwd_multi_bags_pad_mean
        return fn(self.ctx, tables, in_dims, int(ntables), int(out_dim), int(batch), int(aggr), ptr(stream))

    def fwd(self, *args, **kw):
        self.base.check(self.fwd_rc(*args, **kw), "ffh_embedding_fwd_multi_bags_pad_mean")

    def workspace_bytes(self, in_dims, out_dim: int, batch: int) -> int:
        """ffh_embedding_bwd_bags_pad_mean_workspace_bytes of a list of bag sizes (None: a null pointer with ntables 1); 0 on a bad argument."""
        if in_dims is None:
            return int(self.lib.ffh_embedding_bwd_bags_pad_mean_workspace_bytes(None, 1, int(out_dim), int(batch)))
        arr = (I * max(len(in_dims), 1))(*[int(v) for v in in_dims])
        return int(self.lib.ffh_embedding_bwd_bags_pad_mean_workspace_bytes(arr, len(in_dims), int(out_dim), int(batch)))

    def _u(self, name: str, u: BagsUpdate | None, stream) -> int:
        return getattr(self.lib, name)(self.ctx, C.byref(u) if u is not None else None, ptr(stream))

    def fused_rc(self, u: BagsUpdate | None, stream=None) -> int:
        return self._u("ffh_embedding_bwd_fused_multi_bags_pad_mean", u, stream)

    def apply_rc(self, u: BagsUpdate | None, stream=None) -> int:
        return self._u("ffh_embedding_bwd_apply_multi_bags_pad_mean", u, stream)

    def fused(self, u: BagsUpdate, stream=None):
        self.base.check(self.fused_rc(u, stream), "ffh_embedding_bwd_fused_multi_bags_pad_mean")

    def apply(self, u: BagsUpdate, stream=None):
        self.base.check(self.apply_rc(u, stream), "ffh_embedding_bwd_apply_multi_bags_pad_mean")


pad_mean_api = PadMeanApi


# ---- the q8 extension (include/ff_hip_q8.h): tables as 8-bit rows with a scale and a bias each; a quantizer and the gathers that read them ----
class EmbTableQ8(C.Structure):
    """struct ffh_emb_table_q8"""
    _fields_ = [("idx", P), ("rows", P), ("io", P), ("num_entries", L), ("ld", L), ("row_bytes", L)]


class Q8Source(C.Structure):
    """struct ffh_q8_source"""
    _fields_ = [("weight", P), ("rows", P), ("num_entries", L), ("row_bytes", L), ("bf16", C.c_int32), ("reserved_", C.c_int32)]


_SIGS_Q8 = {
    "ffh_q8_abi_version": (I, []),
    "ffh_q8_row_bytes": (SZ, [I]),
    "ffh_q8_quantize_max_workgroups": (I, []),
    "ffh_embedding_quantize_q8": (I, [P, C.POINTER(Q8Source), I, I, P]),
    "ffh_embedding_fwd_multi_q8": (I, [P, C.POINTER(EmbTableQ8), I, I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_q8": (I, [P, C.POINTER(EmbTableQ8), C.POINTER(I), I, I, L, I, P]),
}
Q8_EXT = _extension("q8", _SIGS_Q8, "q8")
Q8_HEADER_PATH, q8_header_symbols, q8_header_abi_version = Q8_EXT.header_path, Q8_EXT.header_symbols, Q8_EXT.header_abi_version


class Q8Api(ExtensionApi):
    ext = Q8_EXT

    def row_bytes(self, out_dim: int) -> int:
        return int(self.lib.ffh_q8_row_bytes(int(out_dim)))

    def quantize_max_workgroups(self) -> int:
        return int(self.lib.ffh_q8_quantize_max_workgroups())

    @staticmethod
    def quantize_rows_per_trip(out_dim: int) -> int:
        """Rows of one table that a quantizer workgroup takes per trip (include/ff_hip_q8.h, QUANTIZER)."""
        lanes = out_dim // 16 if out_dim % 16 == 0 else out_dim // 4
        p = 1
        while p < lanes and p < 64:
            p <<= 1
        return 4 * (64 // p)

    @staticmethod
    def tables(entries) -> "C.Array":
        """entries: iterable of (idx, rows, io, num_entries, ld, row_bytes)."""
        entries = list(entries)
        arr = (EmbTableQ8 * max(1, len(entries)))()
        for k, (idx, rows, io, n, ld, rb) in enumerate(entries):
            arr[k] = EmbTableQ8(ptr(idx), ptr(rows), ptr(io), int(n), int(ld), int(rb))
        return arr

    @staticmethod
    def sources(entries) -> "C.Array":
        """entries: iterable of (weight, rows, num_entries, row_bytes, bf16)."""
        entries = list(entries)
        arr = (Q8Source * max(1, len(entries)))()
        for k, (w, rows, n, rb, bf16) in enumerate(entries):
            arr[k] = Q8Source(ptr(w), ptr(rows), int(n), int(rb), int(bf16), 0)
        return arr

    def quantize_rc(self, sources, ntables: int, out_dim: int, stream=None) -> int:
        return self.lib.ffh_embedding_quantize_q8(self.ctx, sources, int(ntables), int(out_dim), ptr(stream))

    def quantize(self, sources, ntables: int, out_dim: int, stream=None):
        self.base.check(self.quantize_rc(sources, ntables, out_dim, stream), "ffh_embedding_quantize_q8")

    def fwd_rc(self, tables, ntables: int, in_dim: int, out_dim: int, batch: int, aggr: int, stream=None) -> int:
        return self.lib.ffh_embedding_fwd_multi_q8(self.ctx, tables, int(ntables), int(in_dim), int(out_dim), int(batch), int(aggr), ptr(stream))

    def fwd(self, *args, **kw):
        self.base.check(self.fwd_rc(*args, **kw), "ffh_embedding_fwd_multi_q8")

    def fwd_bags_rc(self, tables, in_dims, ntables: int, out_dim: int, batch: int, aggr: int, stream=None) -> int:
        """`in_dims` from BagsApi.in_dims (or None: a null pointer)."""
        return self.lib.ffh_embedding_fwd_multi_bags_q8(self.ctx, tables, in_dims, int(ntables), int(out_dim), int(batch), int(aggr), ptr(stream))

    def fwd_bags(self, *args, **kw):
        self.base.check(self.fwd_bags_rc(*args, **kw), "ffh_embedding_fwd_multi_bags_q8")


q8_api = Q8Api


_hip_singleton: FFHLib | None = None


def load_hip(device: int = 0) -> FFHLib:
    """The product library.  Fails loudly if the HIP extension is missing."""
    global _hip_singleton
    if _hip_singleton is None:
        import torch  # noqa: F401  (first: one HIP runtime per process, torch's libamdhip64.so.7)
        _hip_singleton = FFHLib(HIP_LIB_PATH, device)
        if not _hip_singleton.backend.startswith("hip"):
            raise FFHError(f"{HIP_LIB_PATH} is not the HIP backend ({_hip_singleton.backend})")
    return _hip_singleton
