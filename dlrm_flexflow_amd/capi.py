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


# include/ff_hip_bf16.h: the optional bf16-table extension (its own list and version; libffhip.so exports it, the oracle does not)
BF16_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_bf16.h")
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


# include/ff_hip_ctr.h: the optional CTR extension (binary cross-entropy, evaluation histograms); same rule as the bf16 extension
CTR_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_ctr.h")
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


# include/ff_hip_lr.h: the optional learning-rate extension (schedule state in device memory, optimizer entries that read it); same rule
LR_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_lr.h")


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


# include/ff_hip_data.h: the optional data extension (one shuffled training batch gathered in one launch); same rule
DATA_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_data.h")
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


# include/ff_hip_cross.h: the optional cross extension (the elementwise combine of a DCNv2 low-rank cross layer); same rule
CROSS_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_cross.h")
CROSS_SKIP, CROSS_STORE, CROSS_ADD = 0, 1, 2

_SIGS_CROSS = {
    "ffh_cross_abi_version": (I, []),
    "ffh_cross_fwd": (I, [P, P, L, P, L, P, L, P, L, L, L, P]),
    "ffh_cross_bwd": (I, [P, P, L, P, L, P, L, P, L, P, L, I, P, L, I, L, L, P]),
}


def cross_header_symbols(header_path: str = CROSS_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_CROSS_API_LIST X-macro in include/ff_hip_cross.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_CROSS_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_CROSS_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def cross_header_abi_version(header_path: str = CROSS_HEADER_PATH) -> int:
    """FFH_CROSS_ABI_VERSION of include/ff_hip_cross.h."""
    m = re.search(r"#define\s+FFH_CROSS_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_CROSS_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


# include/ff_hip_adagrad.h: the optional Adagrad extension (the dense launch; FFH_SPARSE_OPT_ADAGRAD in the table update); same rule
ADAGRAD_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_adagrad.h")

_SIGS_ADAGRAD = {
    "ffh_adagrad_abi_version": (I, []),
    "ffh_adagrad_update": (I, [P, P, P, P, L, F, F, F, I, P]),
    "ffh_adagrad_update_lr": (I, [P, P, P, P, L, P, F, F, I, P]),
}


def adagrad_header_symbols(header_path: str = ADAGRAD_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_ADAGRAD_API_LIST X-macro in include/ff_hip_adagrad.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_ADAGRAD_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_ADAGRAD_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def adagrad_header_abi_version(header_path: str = ADAGRAD_HEADER_PATH) -> int:
    """FFH_ADAGRAD_ABI_VERSION of include/ff_hip_adagrad.h."""
    m = re.search(r"#define\s+FFH_ADAGRAD_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_ADAGRAD_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


# include/ff_hip_rowwise.h: the optional row-wise Adagrad extension (FFH_SPARSE_OPT_ROWWISE_ADAGRAD in the table update; no launch of its own)
ROWWISE_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_rowwise.h")

_SIGS_ROWWISE = {
    "ffh_rowwise_abi_version": (I, []),
}


def rowwise_header_symbols(header_path: str = ROWWISE_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_ROWWISE_API_LIST X-macro in include/ff_hip_rowwise.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_ROWWISE_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_ROWWISE_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def rowwise_header_abi_version(header_path: str = ROWWISE_HEADER_PATH) -> int:
    """FFH_ROWWISE_ABI_VERSION of include/ff_hip_rowwise.h."""
    m = re.search(r"#define\s+FFH_ROWWISE_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_ROWWISE_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def data_header_symbols(header_path: str = DATA_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_DATA_API_LIST X-macro in include/ff_hip_data.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_DATA_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_DATA_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def data_header_abi_version(header_path: str = DATA_HEADER_PATH) -> int:
    """FFH_DATA_ABI_VERSION of include/ff_hip_data.h."""
    m = re.search(r"#define\s+FFH_DATA_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_DATA_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def lr_header_symbols(header_path: str = LR_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_LR_API_LIST X-macro in include/ff_hip_lr.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_LR_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_LR_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def lr_header_abi_version(header_path: str = LR_HEADER_PATH) -> int:
    """FFH_LR_ABI_VERSION of include/ff_hip_lr.h."""
    m = re.search(r"#define\s+FFH_LR_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_LR_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def ctr_header_symbols(header_path: str = CTR_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_CTR_API_LIST X-macro in include/ff_hip_ctr.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_CTR_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_CTR_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def ctr_header_abi_version(header_path: str = CTR_HEADER_PATH) -> int:
    """FFH_CTR_ABI_VERSION of include/ff_hip_ctr.h."""
    m = re.search(r"#define\s+FFH_CTR_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_CTR_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def bf16_header_symbols(header_path: str = BF16_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_BF16_API_LIST X-macro in include/ff_hip_bf16.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_BF16_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_BF16_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def bf16_header_abi_version(header_path: str = BF16_HEADER_PATH) -> int:
    """FFH_BF16_ABI_VERSION of include/ff_hip_bf16.h."""
    m = re.search(r"#define\s+FFH_BF16_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_BF16_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


def header_symbols(header_path: str = HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_API_LIST X-macro in include/ff_hip.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def header_abi_version(header_path: str = HEADER_PATH) -> int:
    """FFH_ABI_VERSION of include/ff_hip.h."""
    m = re.search(r"#define\s+FFH_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


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
        conv = []
        sig = _SIGS[name][1][1:]
        for a, t in zip(args, sig):
            conv.append(ptr(a) if t is P else a)
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        self.check(getattr(self.lib, name)(self.ctx, *conv), name)

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


class Bf16Api:
    """The bf16-table extension (include/ff_hip_bf16.h) of a loaded FFHLib; `bf16_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_BF16.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no bf16-table extension ({name} missing; include/ff_hip_bf16.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_bf16_abi_version()
        if got != bf16_header_abi_version():
            raise FFHError(f"{lib.path}: bf16 ABI version {got}, include/ff_hip_bf16.h says {bf16_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; pointers may be tensors/arrays/ints/None."""
        sig = _SIGS_BF16[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        self.base.check(getattr(self.lib, name)(self.ctx, *conv), name)

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


def bf16_api(lib: FFHLib) -> Bf16Api:
    """The bf16-table entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return Bf16Api(lib)


class CtrApi:
    """The CTR extension (include/ff_hip_ctr.h) of a loaded FFHLib; `ctr_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_CTR.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no CTR extension ({name} missing; include/ff_hip_ctr.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_ctr_abi_version()
        if got != ctr_header_abi_version():
            raise FFHError(f"{lib.path}: CTR ABI version {got}, include/ff_hip_ctr.h says {ctr_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def rc(self, name: str, *args) -> int:
        """`name(ctx, *args)` of the extension, returning its status code (FFH_OK, FFH_ERR_UNSUPPORTED, ...)."""
        sig = _SIGS_CTR[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        return getattr(self.lib, name)(self.ctx, *conv)

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; pointers may be tensors/arrays/ints/None."""
        self.base.check(self.rc(name, *args), name)


def ctr_api(lib: FFHLib) -> CtrApi:
    """The CTR entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return CtrApi(lib)


class LrApi:
    """The learning-rate extension (include/ff_hip_lr.h) of a loaded FFHLib; `lr_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_LR.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no learning-rate extension ({name} missing; include/ff_hip_lr.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_lr_abi_version()
        if got != lr_header_abi_version():
            raise FFHError(f"{lib.path}: learning-rate ABI version {got}, include/ff_hip_lr.h says {lr_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; pointers may be tensors/arrays/ints/None."""
        sig = _SIGS_LR[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        self.base.check(getattr(self.lib, name)(self.ctx, *conv), name)

    def state_bytes(self) -> int:
        return int(self.lib.ffh_lr_state_bytes())

    def init(self, block, base, W=0, S=0, N=0, beta1=0.0, beta2=0.0, first_step=0, stream=None):
        sc = LrSchedule(float(base), int(W), int(S), int(N), float(beta1), float(beta2))
        self.call("ffh_lr_state_init", block, C.byref(sc), int(first_step), stream)

    def read(self, block, stream=None) -> LrValues:
        v = LrValues()
        self.call("ffh_lr_state_read", block, C.byref(v), stream)
        return v


def lr_api(lib: FFHLib) -> LrApi:
    """The learning-rate entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return LrApi(lib)


class DataApi:
    """The data extension (include/ff_hip_data.h) of a loaded FFHLib; `data_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_DATA.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no data extension ({name} missing; include/ff_hip_data.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_data_abi_version()
        if got != data_header_abi_version():
            raise FFHError(f"{lib.path}: data ABI version {got}, include/ff_hip_data.h says {data_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def batch_gather_rc(self, segments, seed, epoch, step, local_batch, n_local, world=1, rank=0, stream=None) -> int:
        """ffh_batch_gather; `segments`: (src, dst, row_bytes, kind) tuples, pointers as tensors/arrays/ints/None.  Returns the status code."""
        arr = (GatherSegment * max(1, len(segments)))()
        for k, (src, dst, row_bytes, kind) in enumerate(segments):
            arr[k] = GatherSegment(ptr(src), ptr(dst), int(row_bytes), int(kind))
        order = BatchOrder(int(seed) & (2**64 - 1), int(epoch), int(step), int(local_batch), int(n_local), int(world), int(rank))
        return self.lib.ffh_batch_gather(self.ctx, arr, len(segments), C.byref(order), ptr(stream))

    def batch_gather(self, segments, seed, epoch, step, local_batch, n_local, world=1, rank=0, stream=None):
        self.base.check(self.batch_gather_rc(segments, seed, epoch, step, local_batch, n_local, world, rank, stream), "ffh_batch_gather")


def data_api(lib: FFHLib) -> DataApi:
    """The data entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return DataApi(lib)


# include/ff_hip_digest.h: the optional digest extension (a 64-bit digest of a strided device buffer); same rule
DIGEST_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_digest.h")

_SIGS_DIGEST = {
    "ffh_digest_abi_version": (I, []),
    "ffh_state_digest": (I, [P, P, L, L, L, C.c_uint64, C.c_uint64, P, P]),
}


def digest_header_symbols(header_path: str = DIGEST_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_DIGEST_API_LIST X-macro in include/ff_hip_digest.h."""
    text = open(header_path).read()
    m = re.search(r"#define FFH_DIGEST_API_LIST\(X\)(.*?)\n\n", text, re.S)
    if not m:
        raise RuntimeError("FFH_DIGEST_API_LIST not found in " + header_path)
    return re.findall(r"X\((ffh_[a-z0-9_]+)\)", m.group(1))


def digest_header_abi_version(header_path: str = DIGEST_HEADER_PATH) -> int:
    """FFH_DIGEST_ABI_VERSION of include/ff_hip_digest.h."""
    m = re.search(r"#define\s+FFH_DIGEST_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_DIGEST_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class DigestApi:
    """The digest extension (include/ff_hip_digest.h) of a loaded FFHLib; `digest_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_DIGEST.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no digest extension ({name} missing; include/ff_hip_digest.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_digest_abi_version()
        if got != digest_header_abi_version():
            raise FFHError(f"{lib.path}: digest ABI version {got}, include/ff_hip_digest.h says {digest_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def state_digest_rc(self, base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream=None) -> int:
        """ffh_state_digest, returning its status code (FFH_OK, FFH_ERR_BAD_ARG, ...): *acc += the digest."""
        m64 = 2 ** 64 - 1
        return self.lib.ffh_state_digest(self.ctx, ptr(base), int(rows), int(row_bytes), int(ld_bytes), int(seed) & m64, int(index_base) & m64, ptr(acc),
                                         ptr(stream))

    def state_digest(self, base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream=None):
        self.base.check(self.state_digest_rc(base, rows, row_bytes, ld_bytes, seed, index_base, acc, stream), "ffh_state_digest")


def digest_api(lib: FFHLib) -> DigestApi:
    """The digest entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return DigestApi(lib)


class CrossApi:
    """The cross extension (include/ff_hip_cross.h) of a loaded FFHLib; `cross_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_CROSS.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no cross extension ({name} missing; include/ff_hip_cross.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_cross_abi_version()
        if got != cross_header_abi_version():
            raise FFHError(f"{lib.path}: cross ABI version {got}, include/ff_hip_cross.h says {cross_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def rc(self, name: str, *args) -> int:
        """`name(ctx, *args)` of the extension, returning its status code (FFH_OK, FFH_ERR_BAD_ARG, ...)."""
        sig = _SIGS_CROSS[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        return getattr(self.lib, name)(self.ctx, *conv)

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; pointers may be tensors/arrays/ints/None."""
        self.base.check(self.rc(name, *args), name)


def cross_api(lib: FFHLib) -> CrossApi:
    """The cross entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return CrossApi(lib)


class AdagradApi:
    """The Adagrad extension (include/ff_hip_adagrad.h) of a loaded FFHLib; `adagrad_api(lib)` builds it or raises."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_ADAGRAD.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no Adagrad extension ({name} missing; include/ff_hip_adagrad.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_adagrad_abi_version()
        if got != adagrad_header_abi_version():
            raise FFHError(f"{lib.path}: Adagrad ABI version {got}, include/ff_hip_adagrad.h says {adagrad_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

    def rc(self, name: str, *args) -> int:
        """`name(ctx, *args)` of the extension, returning its status code (FFH_OK, FFH_ERR_BAD_ARG, ...)."""
        sig = _SIGS_ADAGRAD[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        return getattr(self.lib, name)(self.ctx, *conv)

    def call(self, name: str, *args):
        """Call `name(ctx, *args)` of the extension; pointers may be tensors/arrays/ints/None."""
        self.base.check(self.rc(name, *args), name)


def adagrad_api(lib: FFHLib) -> AdagradApi:
    """The Adagrad entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return AdagradApi(lib)


class RowwiseApi:
    """The row-wise Adagrad extension (include/ff_hip_rowwise.h) of a loaded FFHLib; `rowwise_api(lib)` builds it or raises.  The rule itself is
    reached through the table update's entry points of `lib` with SparseOpt.kind = SPARSE_OPT_ROWWISE_ADAGRAD."""

    def __init__(self, lib: FFHLib):
        self.base = lib
        for name, (res, args) in _SIGS_ROWWISE.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no row-wise Adagrad extension ({name} missing; include/ff_hip_rowwise.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_rowwise_abi_version()
        if got != rowwise_header_abi_version():
            raise FFHError(f"{lib.path}: row-wise Adagrad ABI version {got}, include/ff_hip_rowwise.h says {rowwise_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx


def rowwise_api(lib: FFHLib) -> RowwiseApi:
    """The row-wise Adagrad extension of `lib`; FFHError when the library does not export it (e.g. the CPU oracle)."""
    return RowwiseApi(lib)


# ---- the fold extension (include/ff_hip_fold.h): small embedding tables folded out of the first top layer's forward GEMM --------------------
FOLD_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_fold.h")


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


def fold_header_symbols(header_path: str = FOLD_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_FOLD_API_LIST X-macro in include/ff_hip_fold.h."""
    m = re.search(r"#define FFH_FOLD_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_FOLD_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def fold_header_abi_version(header_path: str = FOLD_HEADER_PATH) -> int:
    """FFH_FOLD_ABI_VERSION of include/ff_hip_fold.h."""
    m = re.search(r"#define\s+FFH_FOLD_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_FOLD_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class FoldApi:
    """The fold extension (include/ff_hip_fold.h) of a loaded FFHLib; `fold_api(lib)` builds it or raises."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_FOLD.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no fold extension ({name} missing; include/ff_hip_fold.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_fold_abi_version()
        if got != fold_header_abi_version():
            raise FFHError(f"{lib.path}: fold ABI version {got}, include/ff_hip_fold.h says {fold_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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

    def rc(self, name: str, *args) -> int:
        """`name(ctx, *args)` of the extension, returning its status code; pointers may be tensors / arrays / ints / None, struct arrays as built above."""
        sig = _SIGS_FOLD[name][1][1:]
        if len(args) != len(sig):
            raise TypeError(f"{name}: expected {len(sig)} args, got {len(args)}")
        conv = [ptr(a) if t is P else a for a, t in zip(args, sig)]
        return getattr(self.lib, name)(self.ctx, *conv)

    def call(self, name: str, *args):
        self.base.check(self.rc(name, *args), name)


def fold_api(lib: "FFHLib") -> FoldApi:
    """The fold entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return FoldApi(lib)


# ---- the bags extension (include/ff_hip_bags.h): the gather with a bag size per table, one launch ------------------------------------------
BAGS_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_bags.h")
BAGS_MAX_IN_DIM = 65535

_SIGS_BAGS = {
    "ffh_bags_abi_version": (I, []),
    "ffh_bags_kernarg_bytes": (SZ, []),
    "ffh_embedding_fwd_multi_bags": (I, [P, C.POINTER(EmbTable), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(I), I, I, L, I, P]),
}


def bags_header_symbols(header_path: str = BAGS_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_BAGS_API_LIST X-macro in include/ff_hip_bags.h."""
    m = re.search(r"#define FFH_BAGS_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_BAGS_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def bags_header_abi_version(header_path: str = BAGS_HEADER_PATH) -> int:
    """FFH_BAGS_ABI_VERSION of include/ff_hip_bags.h."""
    m = re.search(r"#define\s+FFH_BAGS_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_BAGS_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class BagsApi:
    """The bags extension (include/ff_hip_bags.h) of a loaded FFHLib; `bags_api(lib)` builds it or raises."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_BAGS.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no bags extension ({name} missing; include/ff_hip_bags.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_bags_abi_version()
        if got != bags_header_abi_version():
            raise FFHError(f"{lib.path}: bags ABI version {got}, include/ff_hip_bags.h says {bags_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def bags_api(lib: "FFHLib") -> BagsApi:
    """The ragged-gather entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return BagsApi(lib)


# ---- the bags-update extension (include/ff_hip_bags_update.h): the fused table update with a bag size per table, one call -----------------
BAGS_UPDATE_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_bags_update.h")
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


def bags_update_header_symbols(header_path: str = BAGS_UPDATE_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_BAGS_UPDATE_API_LIST X-macro in include/ff_hip_bags_update.h."""
    m = re.search(r"#define FFH_BAGS_UPDATE_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_BAGS_UPDATE_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def bags_update_header_abi_version(header_path: str = BAGS_UPDATE_HEADER_PATH) -> int:
    """FFH_BAGS_UPDATE_ABI_VERSION of include/ff_hip_bags_update.h."""
    m = re.search(r"#define\s+FFH_BAGS_UPDATE_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_BAGS_UPDATE_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class BagsUpdateApi:
    """The bags-update extension (include/ff_hip_bags_update.h) of a loaded FFHLib; `bags_update_api(lib)` builds it or raises."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_BAGS_UPDATE.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no bags-update extension ({name} missing; include/ff_hip_bags_update.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_bags_update_abi_version()
        if got != bags_update_header_abi_version():
            raise FFHError(f"{lib.path}: bags-update ABI version {got}, include/ff_hip_bags_update.h says {bags_update_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def bags_update_api(lib: "FFHLib") -> BagsUpdateApi:
    """The ragged-update entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return BagsUpdateApi(lib)


# ---- the bags-sort extension (include/ff_hip_bags_sort.h): the ragged update in two calls, sort (ids only) then apply ----------------------
BAGS_SORT_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_bags_sort.h")

_SIGS_BAGS_SORT = {
    "ffh_bags_sort_abi_version": (I, []),
    "ffh_embedding_bwd_sort_multi_bags": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_apply_multi_bags": (I, [P, C.POINTER(BagsUpdate), P]),
}


def bags_sort_header_symbols(header_path: str = BAGS_SORT_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_BAGS_SORT_API_LIST X-macro in include/ff_hip_bags_sort.h."""
    m = re.search(r"#define FFH_BAGS_SORT_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_BAGS_SORT_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def bags_sort_header_abi_version(header_path: str = BAGS_SORT_HEADER_PATH) -> int:
    """FFH_BAGS_SORT_ABI_VERSION of include/ff_hip_bags_sort.h."""
    m = re.search(r"#define\s+FFH_BAGS_SORT_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_BAGS_SORT_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class BagsSortApi:
    """The bags-sort extension (include/ff_hip_bags_sort.h) of a loaded FFHLib; `bags_sort_api(lib)` builds it or raises.  Both calls take
    the descriptor of the fused ragged update (BagsUpdateApi.descriptor)."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_BAGS_SORT.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no bags-sort extension ({name} missing; include/ff_hip_bags_sort.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_bags_sort_abi_version()
        if got != bags_sort_header_abi_version():
            raise FFHError(f"{lib.path}: bags-sort ABI version {got}, include/ff_hip_bags_sort.h says {bags_sort_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def bags_sort_api(lib: "FFHLib") -> BagsSortApi:
    """The ragged sort / apply entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return BagsSortApi(lib)


# ---- the pad extension (include/ff_hip_pad.h): variable-length bags, the id EMB_PAD_ID being "no lookup" ---------------------------------
PAD_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_pad.h")
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


def pad_header_symbols(header_path: str = PAD_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_PAD_API_LIST X-macro in include/ff_hip_pad.h."""
    m = re.search(r"#define FFH_PAD_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_PAD_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def pad_header_abi_version(header_path: str = PAD_HEADER_PATH) -> int:
    """FFH_PAD_ABI_VERSION of include/ff_hip_pad.h."""
    m = re.search(r"#define\s+FFH_PAD_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_PAD_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class PadApi:
    """The pad extension (include/ff_hip_pad.h) of a loaded FFHLib; `pad_api(lib)` builds it or raises.  The gathers take the arguments of
    BagsApi.rc, the update entries the descriptor of the ragged update (BagsUpdateApi.descriptor)."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_PAD.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no pad extension ({name} missing; include/ff_hip_pad.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_pad_abi_version()
        if got != pad_header_abi_version():
            raise FFHError(f"{lib.path}: pad ABI version {got}, include/ff_hip_pad.h says {pad_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def pad_api(lib: "FFHLib") -> PadApi:
    """The pad entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return PadApi(lib)


# ---- the pad-mean extension (include/ff_hip_pad_mean.h): the pad entries with a mean over the lookups that are there ---------------------
PAD_MEAN_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_pad_mean.h")

_SIGS_PAD_MEAN = {
    "ffh_pad_mean_abi_version": (I, []),
    "ffh_embedding_fwd_multi_bags_pad_mean": (I, [P, C.POINTER(EmbTable), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_fwd_multi_bags_pad_mean_bf16": (I, [P, C.POINTER(EmbTableBf16), C.POINTER(I), I, I, L, I, P]),
    "ffh_embedding_bwd_bags_pad_mean_workspace_bytes": (SZ, [C.POINTER(I), I, I, L]),
    "ffh_embedding_bwd_fused_multi_bags_pad_mean": (I, [P, C.POINTER(BagsUpdate), P]),
    "ffh_embedding_bwd_apply_multi_bags_pad_mean": (I, [P, C.POINTER(BagsUpdate), P]),
}


def pad_mean_header_symbols(header_path: str = PAD_MEAN_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_PAD_MEAN_API_LIST X-macro in include/ff_hip_pad_mean.h."""
    m = re.search(r"#define FFH_PAD_MEAN_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_PAD_MEAN_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def pad_mean_header_abi_version(header_path: str = PAD_MEAN_HEADER_PATH) -> int:
    """FFH_PAD_MEAN_ABI_VERSION of include/ff_hip_pad_mean.h."""
    m = re.search(r"#define\s+FFH_PAD_MEAN_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_PAD_MEAN_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class PadMeanApi:
    """The pad-mean extension (include/ff_hip_pad_mean.h) of a loaded FFHLib; `pad_mean_api(lib)` builds it or raises.  PadApi's methods without
    the sort (the pad sort serves either apply), and the workspace query of the update."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_PAD_MEAN.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no pad-mean extension ({name} missing; include/ff_hip_pad_mean.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_pad_mean_abi_version()
        if got != pad_mean_header_abi_version():
            raise FFHError(f"{lib.path}: pad-mean ABI version {got}, include/ff_hip_pad_mean.h says {pad_mean_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def pad_mean_api(lib: "FFHLib") -> PadMeanApi:
    """The pad-mean entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return PadMeanApi(lib)


# ---- the q8 extension (include/ff_hip_q8.h): tables as 8-bit rows with a scale and a bias each; a quantizer and the gathers that read them ----
Q8_HEADER_PATH = os.path.join(REPO_ROOT, "include", "ff_hip_q8.h")


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


def q8_header_symbols(header_path: str = Q8_HEADER_PATH) -> list[str]:
    """Every symbol of the FFH_Q8_API_LIST X-macro in include/ff_hip_q8.h."""
    m = re.search(r"#define FFH_Q8_API_LIST\(X\)(.*?)\n\n", open(header_path).read(), re.S)
    if not m:
        raise RuntimeError("FFH_Q8_API_LIST not found in " + header_path)
    return re.findall(r"X\((\w+)\)", m.group(1))


def q8_header_abi_version(header_path: str = Q8_HEADER_PATH) -> int:
    """FFH_Q8_ABI_VERSION of include/ff_hip_q8.h."""
    m = re.search(r"#define\s+FFH_Q8_ABI_VERSION\s+(\d+)", open(header_path).read())
    if not m:
        raise RuntimeError("FFH_Q8_ABI_VERSION not found in " + header_path)
    return int(m.group(1))


class Q8Api:
    """The q8 extension (include/ff_hip_q8.h) of a loaded FFHLib; `q8_api(lib)` builds it or raises."""

    def __init__(self, lib: "FFHLib"):
        self.base = lib
        for name, (res, args) in _SIGS_Q8.items():
            fn = getattr(lib.lib, name, None)
            if fn is None:
                raise FFHError(f"{lib.path}: no q8 extension ({name} missing; include/ff_hip_q8.h)")
            fn.restype = res
            fn.argtypes = args
        got = lib.lib.ffh_q8_abi_version()
        if got != q8_header_abi_version():
            raise FFHError(f"{lib.path}: q8 ABI version {got}, include/ff_hip_q8.h says {q8_header_abi_version()} (rebuild)")
        self.lib = lib.lib
        self.ctx = lib.ctx

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


def q8_api(lib: "FFHLib") -> Q8Api:
    """The 8-bit-row entry points of `lib`; FFHError when the library does not export them (e.g. the CPU oracle)."""
    return Q8Api(lib)


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
