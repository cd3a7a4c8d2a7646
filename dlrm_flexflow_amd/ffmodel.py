"""Python face of the C++ FFModel shim (dlrm_flexflow_amd/host/libffmodel.so), bound with ctypes
over host/ffmodel_c.h -- the counterpart of the reference's python/flexflow/core/flexflow_cffi.py
over python/flexflow_c.h.  Method names follow the reference's Python API
(`ffmodel.dense / embedding / concat / batch_matmul / compile / forward / backward / update`).

The operator kernels come from the library `FFConfig.backend` names; the default is the HIP
library and a missing build raises -- nothing here falls back to a CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "host", "libffmodel.so")

# enums [ref: include/ffconst.h:4-57]
DT_FLOAT, DT_INT64 = 40, 43
DT_BF16 = 140                  # this build: bf16 embedding tables (--embedding-dtype bf16); values are uint16 bit patterns
ROUND_STOCHASTIC, ROUND_NEAREST = 0, 1   # --embedding-rounding (include/ffh_bf16.h)
LOSS_MSE_AVG, LOSS_MSE_SUM = 52, 53
METRICS_ACCURACY, METRICS_MSE = 1001, 1008
COMP_MODE_TRAINING, COMP_MODE_INFERENCE = 70, 71
# this build: binary cross-entropy on the final sigmoid and held-out evaluation (include/ff_hip_ctr.h), outside the reference's values
LOSS_BCE = 150
METRICS_BCE, METRICS_AUC = 2001, 2002


class _H(C.Structure):
    _fields_ = [("impl", C.c_void_p)]


class PerfMetrics(C.Structure):
    _fields_ = [("train_all", C.c_int), ("train_correct", C.c_int), ("cce_loss", C.c_float),
                ("sparse_cce_loss", C.c_float), ("mse_loss", C.c_float), ("rmse_loss", C.c_float),
                ("mae_loss", C.c_float)]


class EvalMetricsC(C.Structure):
    """struct flexflow_eval_metrics_t"""
    _fields_ = [("samples", C.c_uint64), ("positives", C.c_uint64), ("correct", C.c_uint64), ("nan_predictions", C.c_uint64),
                ("logloss_sum", C.c_double), ("auc", C.c_double)]


ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
BARRIER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
REDUCE_SCATTER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class FFComm(C.Structure):
    """struct ffcomm (host/ffcomm.h)"""
    _fields_ = [("rank", C.c_int), ("world_size", C.c_int), ("user", C.c_void_p),
                ("alltoall_f32", ALLTOALL_FN), ("allreduce_sum_f32", ALLREDUCE_FN), ("barrier", BARRIER_FN), ("nonblocking", C.c_int),
                ("reduce_scatter_sum_f32", REDUCE_SCATTER_FN), ("allgather_f32", ALLGATHER_FN), ("allreduce_bucket_sum_f32", ALLREDUCE_FN), ("bucket_channel_own", C.c_int),
                ("alltoall_bucket_f32", ALLTOALL_FN), ("allgather_bucket_f32", ALLGATHER_FN)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HOST_LIB_PATH):
        raise capi.FFHError(f"{HOST_LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; g.build()')")
    import torch  # noqa: F401  one HIP runtime per process: torch's copy is loaded first
    L = C.CDLL(HOST_LIB_PATH, mode=C.RTLD_GLOBAL)
    H, I, P, B, F, D = _H, C.c_int, C.c_void_p, C.c_bool, C.c_float, C.c_double
    IP = C.POINTER(C.c_int)
    sigs = {
        "flexflow_config_create": (H, []), "flexflow_config_destroy": (None, [H]),
        "flexflow_config_parse_args": (None, [H, C.POINTER(C.c_char_p), I]),
        "flexflow_config_set_comm": (None, [H, C.POINTER(FFComm)]),
        "flexflow_rccl_available": (I, [C.c_char_p]), "flexflow_rccl_get_unique_id": (I, [C.POINTER(C.c_ubyte), C.c_char_p]),
        "flexflow_rccl_comm_create": (I, [C.POINTER(C.c_ubyte), I, I, C.c_char_p, C.POINTER(FFComm)]),
        "flexflow_rccl_comm_destroy": (None, [C.POINTER(FFComm)]), "flexflow_rccl_last_error": (C.c_char_p, []),
        "flexflow_rccl_comm_calls": (None, [C.POINTER(FFComm), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "flexflow_rccl_comm_calls2": (None, [C.POINTER(FFComm), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "flexflow_config_set_batch_size": (None, [H, I]), "flexflow_config_get_batch_size": (I, [H]),
        "flexflow_config_set_backend": (None, [H, C.c_char_p]), "flexflow_config_set_seed": (None, [H, C.c_uint64]),
        "flexflow_config_set_device": (None, [H, I]), "flexflow_config_set_enable_graph": (None, [H, B]),
        "flexflow_config_set_overlap_embedding": (None, [H, B]), "flexflow_config_set_dense_embedding_update": (None, [H, B]),
        "flexflow_config_set_ragged_update": (None, [H, B]), "flexflow_config_set_embedding_padding": (None, [H, B]),
        "flexflow_config_set_embedding_dtype": (None, [H, I]), "flexflow_config_set_embedding_rounding": (None, [H, I]),
        "flexflow_config_set_eval_embedding_dtype": (None, [H, I]),
        "flexflow_config_set_lr_schedule": (None, [H, C.c_int64, C.c_int64, C.c_int64, I]),
        "flexflow_lr_schedule_value": (D, [C.c_int64, D, C.c_int64, C.c_int64, C.c_int64]),
        "flexflow_model_get_current_lr": (D, [H]),
        "flexflow_shuffle_index": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
        "flexflow_shuffle_indices": (None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, P]),
        "flexflow_model_create": (H, [H]), "flexflow_model_destroy": (None, [H]),
        "flexflow_tensor_create": (H, [H, I, IP, I, B]),
        "flexflow_model_add_dense": (H, [H, H, I, I, B, H, H, C.c_char_p]),
        "flexflow_model_add_embedding": (H, [H, H, I, I, I, H, C.c_char_p]),
        "flexflow_model_add_concat": (H, [H, I, C.POINTER(H), I, C.c_char_p]),
        "flexflow_model_add_batch_matmul": (H, [H, H, H, I, I]),
        "flexflow_model_add_flat": (H, [H, H, C.c_char_p]),
        "flexflow_model_add_tril": (H, [H, H, C.c_char_p]),
        "flexflow_model_add_dot_interaction": (H, [H, H, I, C.c_char_p]),
        "flexflow_model_add_cross_combine": (H, [H, H, H, H, C.c_char_p]),
        "flexflow_model_add_cross_net": (H, [H, H, I, I, C.c_char_p]),
        "flexflow_model_add_transpose": (H, [H, H, I, IP, C.c_char_p]),
        "flexflow_model_add_reshape": (H, [H, H, I, IP, C.c_char_p]),
        "flexflow_zero_initializer_create": (H, []), "flexflow_uniform_initializer_create": (H, [I, F, F]),
        "flexflow_norm_initializer_create": (H, [I, F, F]), "flexflow_glorot_uniform_initializer_create": (H, [I]),
        "flexflow_sgd_optimizer_create": (H, [H, D, D, B, D]), "flexflow_model_set_sgd_optimizer": (None, [H, H]),
        "flexflow_adam_optimizer_create": (H, [H, D, D, D, D, D]), "flexflow_model_set_adam_optimizer": (None, [H, H]),
        "flexflow_adam_optimizer_set_lr": (None, [H, D]),
        "flexflow_config_set_adagrad": (None, [H, D, D]),
        "flexflow_model_weight_mirror_stale_bytes": (C.c_int64, [H]),
        "flexflow_adagrad_optimizer_create": (H, [H, D, D, D, D]), "flexflow_model_set_adagrad_optimizer": (None, [H, H]),
        "flexflow_config_set_adagrad_rowwise": (None, [H, I]), "flexflow_adagrad_optimizer_set_rowwise": (None, [H, I]),
        "flexflow_model_compile": (None, [H, I, IP, I, I]),
        "flexflow_model_init_layers": (None, [H]), "flexflow_model_reset_metrics": (None, [H]),
        "flexflow_model_forward": (None, [H, I]), "flexflow_model_zero_gradients": (None, [H]),
        "flexflow_model_backward": (None, [H, I]), "flexflow_model_update": (None, [H]),
        "flexflow_model_begin_trace": (None, [H, I]), "flexflow_model_end_trace": (None, [H, I]),
        "flexflow_model_sync": (None, [H]), "flexflow_model_get_perf_metrics": (None, [H, C.POINTER(PerfMetrics)]),
        "flexflow_model_get_label_tensor": (H, [H]), "flexflow_model_get_num_layers": (I, [H]),
        "flexflow_model_get_layer_name": (C.c_char_p, [H, I]), "flexflow_model_get_layer_num_weights": (I, [H, I]),
        "flexflow_model_get_parameter": (H, [H, I, I]), "flexflow_model_get_layer_output": (H, [H, I]),
        "flexflow_model_get_stream": (P, [H]), "flexflow_model_uses_graph": (I, [H]), "flexflow_model_set_trace_mode": (None, [H, I]), "flexflow_model_trace_replays": (I, [H, I]),
        "flexflow_model_get_counter": (C.c_int64, [H, C.c_char_p]),
        "flexflow_model_get_backend_name": (C.c_char_p, [H]), "flexflow_model_get_backend_path": (C.c_char_p, [H]),
        "flexflow_tensor_get_num_dims": (I, [H]), "flexflow_tensor_get_dims": (None, [H, IP]),
        "flexflow_tensor_get_local_rows": (C.c_int64, [H]), "flexflow_tensor_is_local": (B, [H]),
        "flexflow_tensor_get_device_ptr": (P, [H]), "flexflow_tensor_get_ld": (C.c_int64, [H]),
        "flexflow_tensor_set_float": (None, [H, H, IP, I, P]), "flexflow_tensor_set_int64": (None, [H, H, IP, I, P]),
        "flexflow_tensor_get_float": (None, [H, H, P]), "flexflow_tensor_get_int64": (None, [H, H, P]),
        "flexflow_tensor_get_grad_float": (None, [H, H, P]),
        "flexflow_tensor_get_data_type": (I, [H]),
        "flexflow_tensor_set_bf16": (None, [H, H, IP, I, P]), "flexflow_tensor_get_bf16": (None, [H, H, P]),
        "flexflow_dlrm_create": (H, [I, C.POINTER(C.c_char_p), C.POINTER(FFComm)]), "flexflow_dlrm_destroy": (None, [H]),
        "flexflow_dlrm_get_model": (H, [H]), "flexflow_dlrm_get_num_samples": (I, [H]), "flexflow_dlrm_get_num_tables": (I, [H]), "flexflow_dlrm_get_bag_size": (I, [H, I]), "flexflow_dlrm_get_bag_fill": (D, [H]), "flexflow_dlrm_get_embedding_pooling": (C.c_char_p, [H]), "flexflow_dlrm_get_start_epoch": (I, [H]),
        "flexflow_dlrm_get_sparse_input": (H, [H, I]), "flexflow_dlrm_get_dense_input": (H, [H]),
        "flexflow_dlrm_warmup": (None, [H]), "flexflow_dlrm_train_steps": (None, [H, I, B]),
        "flexflow_dlrm_run_epochs": (D, [H]), "flexflow_dlrm_time_kernel": (F, [H, I, I]),
        "flexflow_dlrm_probe_step": (None, [H, I, C.POINTER(F), I]),
        "flexflow_perf_metrics_get_bce_loss": (F, [H]), "flexflow_model_eval_batch": (None, [H]),
        "flexflow_model_reset_eval_metrics": (None, [H]),
        "flexflow_model_get_eval_metrics": (None, [H, C.POINTER(EvalMetricsC), P, P]),
        "flexflow_auc_bins": (I, []), "flexflow_auc_from_histograms": (D, [P, P, I]),
        "flexflow_dlrm_evaluate": (D, [H, I, C.POINTER(EvalMetricsC)]),
        "flexflow_model_save_checkpoint": (I, [H, C.c_char_p, C.c_int64]),
        "flexflow_model_load_checkpoint": (I, [H, C.c_char_p, C.POINTER(C.c_int64)]),
        "flexflow_model_state_digest": (C.c_uint64, [H]),
        "flexflow_state_digest_host": (C.c_uint64, [P, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64]),
        "flexflow_digest_record_seed": (C.c_uint64, [C.c_uint64]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _eval_dict(e: EvalMetricsC) -> dict:
    n = int(e.samples)
    return {"samples": n, "positives": int(e.positives), "correct": int(e.correct), "nan_predictions": int(e.nan_predictions),
            "logloss_sum": float(e.logloss_sum), "logloss": float(e.logloss_sum) / n if n else 0.0,
            "accuracy": int(e.correct) / n if n else 0.0, "auc": float(e.auc)}


def auc_from_histograms(hist_pos, hist_neg) -> float:
    """ffh_auc_from_histograms (include/ff_hip_ctr.h) on two uint64 numpy arrays of equal length; NaN without positives or negatives."""
    import numpy as np
    hp, hn = np.ascontiguousarray(hist_pos, dtype=np.uint64), np.ascontiguousarray(hist_neg, dtype=np.uint64)
    if hp.shape != hn.shape or hp.ndim != 1:
        raise ValueError("auc_from_histograms: two 1-D arrays of equal length")
    return float(lib().flexflow_auc_from_histograms(hp.ctypes.data, hn.ctypes.data, hp.shape[0]))


def lr_schedule_value(k: int, base: float, W: int = 0, S: int = 0, N: int = 0) -> float:
    """The learning-rate schedule of include/ff_hip_lr.h, a pure function: the rate of zero-based optimizer step k, computed in double and
    rounded to float once (linear warm-up over W steps, `base`, quadratic decay over N steps from step S, then held)."""
    return float(lib().flexflow_lr_schedule_value(int(k), float(base), int(W), int(S), int(N)))


def shuffle_index(seed: int, epoch: int, i: int, n: int) -> int:
    """The order of --data-randomize total, a pure function (ffh_perm_index of include/ffh_perm.h): the row of a stripe of n rows that
    position i of epoch `epoch` trains on.  For every (seed, epoch) a bijection of [0, n)."""
    if not 0 <= int(i) < max(int(n), 1):
        raise ValueError(f"shuffle_index: position {i} outside [0, {n})")
    return int(lib().flexflow_shuffle_index(int(seed) & (2**64 - 1), int(epoch), int(i), int(n)))


def shuffle_indices(seed: int, epoch: int, n: int, first: int = 0, count: int | None = None) -> np.ndarray:
    """shuffle_index for the positions first .. first + count - 1 (default: all n) as an int64 array."""
    count = int(n) - int(first) if count is None else int(count)
    if first < 0 or count < 0 or first + count > max(int(n), 1):
        raise ValueError(f"shuffle_indices: positions [{first}, {first + count}) outside [0, {n})")
    out = np.empty(count, np.uint64)
    lib().flexflow_shuffle_indices(int(seed) & (2**64 - 1), int(epoch), int(first), count, int(n), out.ctypes.data)
    return out.astype(np.int64)


def _mix64(z: np.ndarray) -> np.ndarray:
    """ffh_mix64 (include/ffh_rng.h) on a uint64 array; the arithmetic wraps as uint64 does"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pad_mask_reference(seed: int, first: int, count: int, fill: float) -> np.ndarray:
    """ffh_pad_mask_indices (include/ff_hip_pad.h) restated in numpy: a bool array, True where slot first + i KEEPS its id, that is where
    ffh_u24(ffh_hash(seed, first + i)) < fill in fp32 (False: the slot becomes the pad id -1)."""
    i = np.arange(int(first), int(first) + int(count), dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64(_mix64(np.array([int(seed) & (2 ** 64 - 1)], np.uint64)) + i)
    u = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)      # 24 bits: exact in fp32
    return u < np.float32(fill)


def padded_bag_counts(idx) -> np.ndarray:
    """count[b] of include/ff_hip_pad_mean.h: the ids >= 0 in bag b of `idx` [batch][L], as int64."""
    return (np.asarray(idx, np.int64) >= 0).sum(axis=1).astype(np.int64)


def padded_bag_reference(W, idx, mean: bool = False) -> np.ndarray:
    """The pad gather of include/ff_hip_pad.h in numpy: out[b] = sum of W[idx[b][j]] over the j, ascending, whose id is not negative, in
    fp32 starting from +0.  `W` is [rows][D] float32, `idx` [batch][L] integers; a bag of only pads gives a row of +0.
    `mean`: the mean gather of include/ff_hip_pad_mean.h -- that sum times float32(1) / float32(max(count, 1)), one fp32 reciprocal and one
    fp32 multiply per element."""
    W, idx = np.asarray(W, np.float32), np.asarray(idx, np.int64)
    out = np.zeros((idx.shape[0], W.shape[1]), np.float32)
    for j in range(idx.shape[1]):
        live = idx[:, j] >= 0
        out[live] = out[live] + W[idx[live, j]]
    if mean:
        inv = np.float32(1) / np.maximum(padded_bag_counts(idx), 1).astype(np.float32)
        out = out * inv[:, None]
    return out


def state_digest_reference(data, seed: int, index_base: int = 0, row_bytes: int | None = None) -> int:
    """The digest of include/ff_hip_digest.h restated in numpy: `data` is a 2-D array (its rows are the rows, row_bytes their length in bytes:
    whatever its strides are, only the elements count, so the result does not depend on a leading dimension), a 1-D array (one row), or
    bytes / bytearray (rows of row_bytes bytes each; default one row).  W = ceil(row_bytes / 8) little-endian words per row, bytes past
    row_bytes zero; word (r, w) has index i = index_base + r W + w; the result is sum ffh_mix64(ffh_hash(seed, i) ^ word) mod 2^64."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(bytes(data), np.uint8)
        rb = len(raw) if row_bytes is None else int(row_bytes)
        if rb <= 0 or len(raw) % rb:
            raise ValueError("state_digest_reference: the bytes are no whole number of rows")
        rows2 = raw.reshape(-1, rb)
    else:
        a = np.asarray(data)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2:
            raise ValueError("state_digest_reference: a 1-D or 2-D array")
        a = np.ascontiguousarray(a)
        rows2 = a.view(np.uint8).reshape(a.shape[0], a.shape[1] * a.dtype.itemsize)
        if row_bytes is not None and int(row_bytes) != rows2.shape[1]:
            raise ValueError("state_digest_reference: row_bytes does not match the array's rows")
        rb = rows2.shape[1]
    if rb < 2 or rb % 2:
        raise ValueError("state_digest_reference: row_bytes must be even and >= 2")
    n, W = rows2.shape[0], (rb + 7) // 8
    if n == 0:
        return 0
    total = 0
    block = max(1, (1 << 17) // W)          # rows per pass: the temporaries stay in cache
    with np.errstate(over="ignore"):
        key = _mix64(np.array([int(seed) & (2 ** 64 - 1)], np.uint64))[0]
        for r0 in range(0, n, block):
            part = rows2[r0:r0 + block]
            padded = np.zeros((part.shape[0], 8 * W), np.uint8)
            padded[:, :rb] = part
            words = padded.view("<u8").reshape(-1).astype(np.uint64)
            i = np.arange(words.size, dtype=np.uint64) + np.uint64((int(index_base) + r0 * W) & (2 ** 64 - 1))
            total += int(np.add.reduce(_mix64(_mix64(key + i) ^ words), dtype=np.uint64))
    return total & (2 ** 64 - 1)


def state_digest_host(data, seed: int, index_base: int = 0, row_bytes: int | None = None, ld_bytes: int | None = None) -> int:
    """ffh_state_digest_host of include/ff_hip_digest.h -- the header's own inline function as the host layer compiles it -- on a contiguous
    buffer of rows ld_bytes apart (default row_bytes)."""
    raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    rb = len(raw) if row_bytes is None else int(row_bytes)
    ld = rb if ld_bytes is None else int(ld_bytes)
    if rb < 2 or rb % 2 or ld < rb or ld % 2:
        raise ValueError("state_digest_host: row_bytes even and >= 2, ld_bytes even and >= row_bytes")
    rows = 0 if len(raw) < rb else (len(raw) - rb) // ld + 1
    raw = np.ascontiguousarray(raw)
    return int(lib().flexflow_state_digest_host(raw.ctypes.data, rows, rb, ld, int(seed) & (2 ** 64 - 1), int(index_base) & (2 ** 64 - 1)))


def digest_record_seed(ordinal: int) -> int:
    """ffh_digest_record_seed: the digest seed of record `ordinal` of a checkpoint."""
    return int(lib().flexflow_digest_record_seed(int(ordinal)))


CHECKPOINT_MAGIC = b"FFHCKPT\n"
_CK_DTYPES = {"f32": np.dtype("<f4"), "bf16": np.dtype("<u2"), "u64": np.dtype("<u8"), "raw": np.dtype("u1")}


def read_checkpoint(path: str) -> dict:
    """One rank's checkpoint file (DIR/rank-R-of-N.ffck; `path` may also be the directory of a one-rank checkpoint) as a dict: "meta" holds the
    manifest -- the run fields (epochs_done, steps, optimizer, table_optimizer, embedding_dtype, embedding_rounding, world_size, rank, lr_route,
    lr_host_steps; on the device learning-rate route also lr_schedule {base, warmup_steps, decay_start, decay_steps}), "tables" {operator: placement}, "digest" and "records" {name: {type, rows, cols, offset, digest, ordinal}} -- and every record
    name maps to its contents, memory-mapped read-only: [rows][cols] float32 / uint16 (bf16 bit patterns) / uint64 / uint8 (raw).  Raises ValueError on a
    file that is no checkpoint or is cut short; digests are NOT verified here (state_digest_reference(record, digest_record_seed(ordinal)) does that)."""
    if os.path.isdir(path):
        path = os.path.join(path, "rank-0-of-1.ffck")
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(24)
        if len(head) < 24 or head[:8] != CHECKPOINT_MAGIC:
            raise ValueError(f"{path}: not a checkpoint file")
        version, length = int.from_bytes(head[8:12], "little"), int.from_bytes(head[16:24], "little")
        if version != 1:
            raise ValueError(f"{path}: format version {version}")
        text = f.read(length)
    if len(text) != length:
        raise ValueError(f"{path}: truncated manifest")
    data_start = (24 + length + 4095) // 4096 * 4096
    meta = {"version": version, "tables": {}, "records": {}, "path": path}
    for line in text.decode().splitlines():
        k, *v = line.split()
        if k == "record":
            meta["records"][v[1]] = {"ordinal": int(v[0]), "type": v[2], "rows": int(v[3]), "cols": int(v[4]), "offset": int(v[5]), "digest": int(v[6], 16)}
        elif k == "table":
            meta["tables"][v[0]] = v[1]
        elif k == "digest":
            meta["digest"] = int(v[0], 16)
        elif k in ("epochs_done", "steps", "world_size", "rank", "lr_host_steps"):
            meta[k] = int(v[0])
        elif k == "lr_schedule":
            meta[k] = {"base": float(v[0]), "warmup_steps": int(v[1]), "decay_start": int(v[2]), "decay_steps": int(v[3])}
        elif k in ("optimizer", "table_optimizer", "embedding_dtype", "embedding_rounding", "lr_route"):
            meta[k] = v[0]
    out = {"meta": meta}
    for name, r in meta["records"].items():
        dt = _CK_DTYPES[r["type"]]
        nbytes = r["rows"] * r["cols"] * dt.itemsize
        if data_start + r["offset"] + nbytes > size:
            raise ValueError(f"{path}: truncated inside record {name}")
        out[name] = np.memmap(path, dtype=dt, mode="r", offset=data_start + r["offset"], shape=(r["rows"], r["cols"])) if nbytes else np.zeros((r["rows"], r["cols"]), dt)
    return out


def adagrad_reference(w, g, S, lr, eps, wd=0.0):
    """One Adagrad step as include/ff_hip_adagrad.h states it (torch.optim.Adagrad's element-wise rule, no lr_decay), restated with one numpy operation
    per rounded operation in the dtype of `w` (float32: the bits the kernels give; float64: the same statements for a comparison with torch).
    Returns (w_new, S_new); the inputs are left alone."""
    dt = np.asarray(w).dtype
    w, g, S = np.asarray(w, dt), np.asarray(g, dt), np.asarray(S, dt)
    lr, eps, wd = dt.type(lr), dt.type(eps), dt.type(wd)
    with np.errstate(all="ignore"):
        gt = g if wd == 0 else g + wd * w
        S = S + gt * gt
        d = np.sqrt(S) + eps
        q = gt / d
        w = w - lr * q
    return w, S


def rowwise_tree_sum(t):
    """TREE of include/ff_hip_rowwise.h over the last axis of the non-negative array `t`: zero-pad to the next power of two, then add neighbouring
    subtrees level by level (level k adds the elements whose indices differ in bit k), each addition rounded in t's dtype."""
    t = np.asarray(t)
    P = 1 << max(t.shape[-1] - 1, 0).bit_length()
    t = np.concatenate([t, np.zeros(t.shape[:-1] + (P - t.shape[-1],), t.dtype)], axis=-1)
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def rowwise_adagrad_reference(w, g, S, lr, eps, wd=0.0):
    """One row-wise Adagrad step as include/ff_hip_rowwise.h states it, restated with one numpy operation per rounded operation in the dtype of `w`
    (float32: the bits the kernels give; float64: the same statements for a comparison).  w, g: [rows][D]; S: [rows], one accumulator per row.
    Returns (w_new, S_new); the inputs are left alone."""
    dt = np.asarray(w).dtype
    w, g, S = np.asarray(w, dt), np.asarray(g, dt), np.asarray(S, dt)
    lr, eps, wd = dt.type(lr), dt.type(eps), dt.type(wd)
    with np.errstate(all="ignore"):
        gt = g if wd == 0 else g + wd * w
        t = gt * gt
        total = rowwise_tree_sum(t)
        ms = total / dt.type(w.shape[-1])
        S = S + ms
        d = np.sqrt(S) + eps
        q = gt / d[..., None]
        w = w - lr * q
    return w, S


def cross_reference(x0, v, xl) -> np.ndarray:
    """The combine of a DCNv2 low-rank cross layer as include/ff_hip_cross.h states it, in float32 numpy: fadd_rn(fmul_rn(x0, v), xl) -- two
    separately rounded float32 operations per element (numpy never contracts them), which ffh_cross_fwd equals bit for bit."""
    x0, v, xl = (np.asarray(a, dtype=np.float32) for a in (x0, v, xl))
    with np.errstate(all="ignore"):
        return (x0 * v).astype(np.float32) + xl


def cross_reference_backward(dy, x0, v, aliased=False):
    """Backward of cross_reference for the output gradient dy, as ffh_cross_bwd states it.  Returns (dv, g_x0, g_xl): dv = fmul_rn(dy, x0),
    g_x0 = fmul_rn(dy, v), g_xl = dy -- what a STORE leaves in the destination and what an ADD adds to it (fadd_rn(old, g)).
    aliased=True (layer 0: xl is x0, one gradient buffer): (dv, fadd_rn(fmul_rn(dy, v), dy), None)."""
    dy, x0, v = (np.asarray(a, dtype=np.float32) for a in (dy, x0, v))
    with np.errstate(all="ignore"):
        dv = (dy * x0).astype(np.float32)
        g0 = (dy * v).astype(np.float32)
        if aliased:
            return dv, g0 + dy, None
        return dv, g0, dy.copy()


def q8_quantize_reference(w):
    """Rows of a [rows][D] float32 table as 8-bit codes with a scale and a bias per row, as include/ff_hip_q8.h states the rule: float32
    throughout, every operation rounded on its own.  Returns (codes uint8 [rows][D], scale float32 [rows], bias float32 [rows])."""
    w = np.asarray(w, dtype=np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        mn = w.min(axis=-1) + f(0.0)             # a zero minimum is +0 whatever the order of the min
        mx = w.max(axis=-1)
        rng = (mx - mn).astype(f)
        scale = (rng / f(255.0)).astype(f)
        inv = (f(255.0) / (rng + f(1e-8)).astype(f)).astype(f)
        q = np.rint(((w - mn[..., None]).astype(f) * inv[..., None]).astype(f))      # round half to even
    return q.astype(np.uint8), scale, mn.astype(f)


def q8_dequantize_reference(codes, scale, bias) -> np.ndarray:
    """w[d] = (float)code[d] * scale + bias: a float32 multiply, then a float32 add (two roundings, not an fma)."""
    codes = np.asarray(codes, dtype=np.uint8)
    scale, bias = (np.asarray(a, dtype=np.float32) for a in (scale, bias))
    with np.errstate(all="ignore"):
        return (codes.astype(np.float32) * scale[..., None]).astype(np.float32) + bias[..., None]


def q8_pack_rows(codes, scale, bias, row_bytes: int | None = None) -> np.ndarray:
    """The byte layout of include/ff_hip_q8.h: uint8 [rows][row_bytes] = D codes, fp32 scale, fp32 bias, zeros.  row_bytes defaults to D + 8."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    rows, D = codes.shape
    row_bytes = D + 8 if row_bytes is None else int(row_bytes)
    if D % 4 or row_bytes < D + 8 or row_bytes % 4:
        raise ValueError(f"q8_pack_rows: D = {D} must be a multiple of 4 and row_bytes = {row_bytes} a multiple of 4 that is >= D + 8")
    out = np.zeros((rows, row_bytes), np.uint8)
    out[:, :D] = codes
    out[:, D:D + 4] = np.ascontiguousarray(scale, dtype="<f4").reshape(rows, 1).view(np.uint8)
    out[:, D + 4:D + 8] = np.ascontiguousarray(bias, dtype="<f4").reshape(rows, 1).view(np.uint8)
    return out


def q8_unpack_rows(rows, D: int):
    """(codes, scale, bias) of uint8 [rows][row_bytes] in the layout of q8_pack_rows."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim != 2 or rows.shape[1] < D + 8:
        raise ValueError("q8_unpack_rows: rows must be [rows][row_bytes >= D + 8]")
    scale = np.ascontiguousarray(rows[:, D:D + 4]).view("<f4").reshape(-1).astype(np.float32)
    bias = np.ascontiguousarray(rows[:, D + 4:D + 8]).view("<f4").reshape(-1).astype(np.float32)
    return rows[:, :D].copy(), scale, bias


def _argv(args):
    arr = (C.c_char_p * len(args))(*[a.encode() for a in args])
    return arr


class Tensor:
    def __init__(self, handle, model: "FFModel | None"):
        self.h = handle
        self.model = model

    @property
    def dims(self):
        n = lib().flexflow_tensor_get_num_dims(self.h)
        d = (C.c_int * n)()
        lib().flexflow_tensor_get_dims(self.h, d)
        return tuple(d)

    @property
    def local_rows(self) -> int:
        return lib().flexflow_tensor_get_local_rows(self.h)

    @property
    def is_local(self) -> bool:
        return bool(lib().flexflow_tensor_is_local(self.h))

    @property
    def device_ptr(self) -> int:
        """Address of element (0, 0) in the backend's memory (0: not held by this rank); tests / tools only."""
        return lib().flexflow_tensor_get_device_ptr(self.h) or 0

    @property
    def ld(self) -> int:
        return lib().flexflow_tensor_get_ld(self.h)

    @property
    def data_type(self) -> int:
        """DT_FLOAT, DT_INT64, ... or DT_BF16 (a bf16 embedding table)"""
        return lib().flexflow_tensor_get_data_type(self.h)

    def _local_shape(self):
        d = self.dims
        if len(d) == 1:
            return d
        if len(d) == 2:
            return (self.local_rows, d[1])
        return (self.local_rows // int(np.prod(d[1:-1])),) + d[1:]

    def set(self, arr: np.ndarray, raw_bf16: bool = False):
        """fp32 into a bf16 table is rounded to nearest even; raw_bf16=True: `arr` holds the uint16 bit patterns, copied as they are."""
        a = np.ascontiguousarray(arr)
        dims = (C.c_int * a.ndim)(*a.shape)
        if raw_bf16:
            if a.dtype != np.uint16:
                raise TypeError(f"raw_bf16 takes uint16 bit patterns, not {a.dtype}")
            lib().flexflow_tensor_set_bf16(self.h, self.model.h, dims, a.ndim, a.ctypes.data)
        elif a.dtype == np.float32:
            lib().flexflow_tensor_set_float(self.h, self.model.h, dims, a.ndim, a.ctypes.data)
        elif a.dtype == np.int64:
            lib().flexflow_tensor_set_int64(self.h, self.model.h, dims, a.ndim, a.ctypes.data)
        else:
            raise TypeError(a.dtype)

    def get(self, dtype=np.float32, raw_bf16: bool = False) -> np.ndarray:
        """A bf16 table comes out widened exactly to fp32; raw_bf16=True: its uint16 bit patterns."""
        if raw_bf16:
            out = np.empty(self._local_shape(), np.uint16)
            lib().flexflow_tensor_get_bf16(self.h, self.model.h, out.ctypes.data)
            return out
        out = np.empty(self._local_shape(), dtype)
        if dtype == np.float32:
            lib().flexflow_tensor_get_float(self.h, self.model.h, out.ctypes.data)
        else:
            lib().flexflow_tensor_get_int64(self.h, self.model.h, out.ctypes.data)
        return out

    def get_grad(self) -> np.ndarray:
        out = np.empty(self._local_shape(), np.float32)
        lib().flexflow_tensor_get_grad_float(self.h, self.model.h, out.ctypes.data)
        return out

    # reference names [ref: python/flexflow/core/flexflow_cffi.py Parameter.set_weights/get_weights]
    set_weights = set
    get_weights = get


class FFConfig:
    def __init__(self, argv=None, backend: str | None = None, comm: "FFComm | None" = None):
        self.h = lib().flexflow_config_create()
        self._comm = comm
        if argv:
            full = ["ffmodel"] + list(argv)
            lib().flexflow_config_parse_args(self.h, _argv(full), len(full))
        if backend:
            lib().flexflow_config_set_backend(self.h, backend.encode())
        if comm is not None:
            lib().flexflow_config_set_comm(self.h, C.byref(comm))

    batch_size = property(lambda s: lib().flexflow_config_get_batch_size(s.h),
                          lambda s, v: lib().flexflow_config_set_batch_size(s.h, v))

    def set(self, seed=None, device=None, enable_graph=None, overlap_embedding=None, dense_embedding_update=None,
            embedding_dtype=None, embedding_rounding=None, lr_warmup_steps=None, lr_decay_start_step=None, lr_num_decay_steps=None,
            device_lr=None, adagrad_eps=None, adagrad_initial_accumulator=None, adagrad_rowwise=None, ragged_update=None,
            eval_embedding_dtype=None, embedding_padding=None):
        """embedding_dtype: "fp32" | "bf16"; embedding_rounding: "stochastic" | "nearest" (the --embedding-* flags).
        lr_*: the schedule of --lr-num-warmup-steps / --lr-decay-start-step / --lr-num-decay-steps; device_lr: True = --device-lr,
        False = --host-lr-schedule, None = compile() chooses the route.
        adagrad_eps / adagrad_initial_accumulator: --adagrad-eps / --adagrad-initial-accumulator, what an AdagradOptimizer without its own takes.
        adagrad_rowwise: --adagrad-rowwise, the tables of an AdagradOptimizer keep one accumulator per row (include/ff_hip_rowwise.h).
        eval_embedding_dtype: "fp32" | "int8" (--eval-embedding-dtype): eval_batch() gathers from 8-bit row images of the tables (include/ff_hip_q8.h).
        embedding_padding: --embedding-padding, the id -1 in a sparse input is "no lookup" (variable-length bags; include/ff_hip_pad.h).
        FFModel(config) copies the config: call set() before the model is built (as for every other field)."""
        if embedding_padding is not None: lib().flexflow_config_set_embedding_padding(self.h, bool(embedding_padding))
        if adagrad_rowwise is not None:
            lib().flexflow_config_set_adagrad_rowwise(self.h, 1 if adagrad_rowwise else 0)
        if adagrad_eps is not None or adagrad_initial_accumulator is not None:
            self._adagrad = tuple(old if new is None else float(new) for old, new in zip(getattr(self, "_adagrad", (1e-10, 0.0)),
                                                                                       (adagrad_eps, adagrad_initial_accumulator)))
            lib().flexflow_config_set_adagrad(self.h, *self._adagrad)
        if any(v is not None for v in (lr_warmup_steps, lr_decay_start_step, lr_num_decay_steps, device_lr)):
            self._lr = tuple(old if new is None else int(new) for old, new in zip(getattr(self, "_lr", (0, 0, 0)),
                                                                               (lr_warmup_steps, lr_decay_start_step, lr_num_decay_steps)))
            if device_lr is not None:
                self._device_lr = 1 if device_lr else -1
            lib().flexflow_config_set_lr_schedule(self.h, *self._lr, getattr(self, "_device_lr", 0))
        if seed is not None: lib().flexflow_config_set_seed(self.h, seed)
        if device is not None: lib().flexflow_config_set_device(self.h, device)
        if enable_graph is not None: lib().flexflow_config_set_enable_graph(self.h, enable_graph)
        if overlap_embedding is not None: lib().flexflow_config_set_overlap_embedding(self.h, overlap_embedding)
        if dense_embedding_update is not None: lib().flexflow_config_set_dense_embedding_update(self.h, dense_embedding_update)
        if ragged_update is not None: lib().flexflow_config_set_ragged_update(self.h, bool(ragged_update))      # (--ragged-update / --no-ragged-update)
        if embedding_dtype is not None:
            dt = {"fp32": DT_FLOAT, "bf16": DT_BF16}.get(embedding_dtype)
            if dt is None:
                raise ValueError(f"embedding_dtype {embedding_dtype!r}: 'fp32' or 'bf16'")
            lib().flexflow_config_set_embedding_dtype(self.h, dt)
        if eval_embedding_dtype is not None:
            q = {"fp32": 0, "int8": 1}.get(eval_embedding_dtype)
            if q is None:
                raise ValueError(f"eval_embedding_dtype {eval_embedding_dtype!r}: 'fp32' or 'int8'")
            lib().flexflow_config_set_eval_embedding_dtype(self.h, q)
        if embedding_rounding is not None:
            mode = {"stochastic": ROUND_STOCHASTIC, "nearest": ROUND_NEAREST}.get(embedding_rounding)
            if mode is None:
                raise ValueError(f"embedding_rounding {embedding_rounding!r}: 'stochastic' or 'nearest'")
            lib().flexflow_config_set_embedding_rounding(self.h, mode)
        return self


_NULL = _H(None)


class FFModel:
    def __init__(self, config: FFConfig | None = None, _handle=None):
        self.config = config
        self.h = _handle if _handle is not None else lib().flexflow_model_create(config.h)
        self._owned = _handle is None

    # -- graph construction (reference names) -------------------------------------------------
    def create_tensor(self, dims, data_type=DT_FLOAT, create_grad=True) -> Tensor:
        d = (C.c_int * len(dims))(*dims)
        return Tensor(lib().flexflow_tensor_create(self.h, len(dims), d, data_type, create_grad), self)

    def dense(self, input: Tensor, out_dim, activation=capi.AC_MODE_NONE, use_bias=True, kernel_initializer=None,
              bias_initializer=None, name=None) -> Tensor:
        return Tensor(lib().flexflow_model_add_dense(self.h, input.h, out_dim, activation, use_bias,
                                                     kernel_initializer or _NULL, bias_initializer or _NULL,
                                                     name.encode() if name else None), self)

    def embedding(self, input: Tensor, num_entries, out_dim, aggr=capi.AGGR_MODE_SUM, kernel_initializer=None, name=None) -> Tensor:
        return Tensor(lib().flexflow_model_add_embedding(self.h, input.h, num_entries, out_dim, aggr,
                                                         kernel_initializer or _NULL, name.encode() if name else None), self)

    def concat(self, tensors, axis, name=None) -> Tensor:
        arr = (_H * len(tensors))(*[t.h for t in tensors])
        return Tensor(lib().flexflow_model_add_concat(self.h, len(tensors), arr, axis, name.encode() if name else None), self)

    def batch_matmul(self, a: Tensor, b: Tensor, a_seq_length_dim=-1, b_seq_length_dim=-1) -> Tensor:
        return Tensor(lib().flexflow_model_add_batch_matmul(self.h, a.h, b.h, a_seq_length_dim, b_seq_length_dim), self)

    def flat(self, input: Tensor, name=None) -> Tensor:
        return Tensor(lib().flexflow_model_add_flat(self.h, input.h, name.encode() if name else None), self)

    def dot_interaction(self, input: Tensor, d: int, name=None) -> Tensor:
        """[batch][c * d] (concat of the bottom-MLP output and the embedding outputs) -> [batch][d + c (c - 1) / 2]:
        row 0 passed through, then the pairwise dot products i > j -- the whole interaction in one launch each way."""
        return Tensor(lib().flexflow_model_add_dot_interaction(self.h, input.h, d, name.encode() if name else None), self)

    def cross_combine(self, x0: Tensor, v: Tensor, xl: Tensor, name=None) -> Tensor:
        """x0 (.) v + xl on three [batch][D] tensors: the third line of a DCNv2 low-rank cross layer (include/ff_hip_cross.h); in layer 0
        xl is x0.  Needs a kernel library with the cross extension: compile() refuses the model otherwise."""
        return Tensor(lib().flexflow_model_add_cross_combine(self.h, x0.h, v.h, xl.h, name.encode() if name else None), self)

    def save_checkpoint(self, dir: str, epochs_done: int = 0) -> None:
        """Writes this rank's file of a checkpoint, DIR/rank-R-of-N.ffck: every parameter this rank holds, the optimizer state, the
        learning-rate position and the bf16 rounding counter, each record with its digest.  Between steps; synchronises; aborts with the reason on failure."""
        lib().flexflow_model_save_checkpoint(self.h, os.fsencode(dir), int(epochs_done))

    def load_checkpoint(self, dir: str) -> dict:
        """Loads DIR/rank-R-of-N.ffck into this compiled model, verifying every record's digest after the copy; whatever does not fit (other shapes,
        optimizer, element type, world size, placement, a damaged file) aborts with "FATAL: --load-checkpoint DIR: <reason>".  Returns {"epochs_done"}."""
        e = C.c_int64(0)
        lib().flexflow_model_load_checkpoint(self.h, os.fsencode(dir), C.byref(e))
        return {"epochs_done": int(e.value)}

    def state_digest(self) -> int:
        """The fold (sum mod 2^64) of the digests of every record a checkpoint of this model would hold -- its "digest" line; on the device where the
        kernel library has the digest extension (include/ff_hip_digest.h), nothing but one word is copied out.  Synchronises."""
        return int(lib().flexflow_model_state_digest(self.h))

    def cross_net(self, x0: Tensor, num_layers: int = 3, low_rank: int = 512, name=None) -> Tensor:
        """torchrec's LowRankCrossNet on x0 [batch][D]: per layer u = dense(x_l, low_rank, no bias), v = dense(u, D), x_{l+1} =
        cross_combine(x0, v, x_l) -- 3 * num_layers operators; returns x_L."""
        return Tensor(lib().flexflow_model_add_cross_net(self.h, x0.h, int(num_layers), int(low_rank), name.encode() if name else None), self)

    def tril(self, input: Tensor, name=None) -> Tensor:
        """Strict lower triangle of [batch][n][n] -> [batch][n (n - 1) / 2] (MLPerf-DLRM's pick of the pairwise dots)."""
        return Tensor(lib().flexflow_model_add_tril(self.h, input.h, name.encode() if name else None), self)

    def transpose(self, input: Tensor, perm, name=None) -> Tensor:
        p = (C.c_int * len(perm))(*perm)
        return Tensor(lib().flexflow_model_add_transpose(self.h, input.h, len(perm), p, name.encode() if name else None), self)

    def reshape(self, input: Tensor, shape, name=None) -> Tensor:
        p = (C.c_int * len(shape))(*shape)
        return Tensor(lib().flexflow_model_add_reshape(self.h, input.h, len(shape), p, name.encode() if name else None), self)

    @staticmethod
    def uniform_initializer(seed, lo, hi): return lib().flexflow_uniform_initializer_create(seed, lo, hi)

    @staticmethod
    def norm_initializer(seed, mean, std): return lib().flexflow_norm_initializer_create(seed, mean, std)

    @staticmethod
    def zero_initializer(): return lib().flexflow_zero_initializer_create()

    @staticmethod
    def glorot_uniform_initializer(seed): return lib().flexflow_glorot_uniform_initializer_create(seed)

    def set_sgd_optimizer(self, lr=0.01, momentum=0.0, nesterov=False, weight_decay=0.0):
        self._opt = lib().flexflow_sgd_optimizer_create(self.h, lr, momentum, nesterov, weight_decay)
        lib().flexflow_model_set_sgd_optimizer(self.h, self._opt)

    def set_adam_optimizer(self, alpha=0.001, beta1=0.9, beta2=0.999, weight_decay=0.0, epsilon=1e-8):
        """AdamOptimizer [ref: python/flexflow/core/flexflow_cffi.py AdamOptimizer; include/optimizer.h:62-85]"""
        self._opt = lib().flexflow_adam_optimizer_create(self.h, alpha, beta1, beta2, weight_decay, epsilon)
        lib().flexflow_model_set_adam_optimizer(self.h, self._opt)

    def set_adagrad_optimizer(self, lr=0.01, weight_decay=0.0, epsilon=None, initial_accumulator=None, rowwise=False):
        """AdagradOptimizer(self, ...) as this model's optimizer."""
        AdagradOptimizer(self, lr, weight_decay, epsilon, initial_accumulator, rowwise)

    def compile(self, loss_type=LOSS_MSE_AVG, metrics=(METRICS_ACCURACY, METRICS_MSE), comp_mode=COMP_MODE_TRAINING):
        m = (C.c_int * len(metrics))(*metrics)
        lib().flexflow_model_compile(self.h, loss_type, m, len(metrics), comp_mode)

    # -- step ---------------------------------------------------------------------------------
    def init_layers(self): lib().flexflow_model_init_layers(self.h)
    def reset_metrics(self): lib().flexflow_model_reset_metrics(self.h)
    def forward(self, seq_length=-1): lib().flexflow_model_forward(self.h, seq_length)
    def zero_gradients(self): lib().flexflow_model_zero_gradients(self.h)
    def backward(self, seq_length=-1): lib().flexflow_model_backward(self.h, seq_length)
    def update(self): lib().flexflow_model_update(self.h)
    def begin_trace(self, trace_id): lib().flexflow_model_begin_trace(self.h, trace_id)
    def end_trace(self, trace_id): lib().flexflow_model_end_trace(self.h, trace_id)
    def sync(self): lib().flexflow_model_sync(self.h)

    def train_step(self):
        self.forward(); self.zero_gradients(); self.backward(); self.update()

    # -- inspection ---------------------------------------------------------------------------
    @property
    def label_tensor(self) -> Tensor: return Tensor(lib().flexflow_model_get_label_tensor(self.h), self)
    @property
    def num_layers(self) -> int: return lib().flexflow_model_get_num_layers(self.h)
    def layer_name(self, i) -> str: return lib().flexflow_model_get_layer_name(self.h, i).decode()
    def layer_num_weights(self, i) -> int: return lib().flexflow_model_get_layer_num_weights(self.h, i)
    def parameter(self, layer, index) -> Tensor: return Tensor(lib().flexflow_model_get_parameter(self.h, layer, index), self)
    def layer_output(self, layer) -> Tensor: return Tensor(lib().flexflow_model_get_layer_output(self.h, layer), self)
    @property
    def stream(self) -> int: return lib().flexflow_model_get_stream(self.h) or 0
    def weight_mirror_stale_bytes(self) -> int:
        """Bytes of the weight slab's bf16 twin (tensor-op mode) / three-plane image (--fp32-split-bf16x3) that differ from a fresh conversion of
        the fp32 weights: 0 where the optimizer kept it current; -1: the model keeps none; -2: a host write is pending.  Synchronises."""
        return int(lib().flexflow_model_weight_mirror_stale_bytes(self.h))

    def current_lr(self) -> float:
        """The scheduled rate of the next optimizer step (base: the optimizer's lr / alpha), as the float the kernels receive."""
        return float(lib().flexflow_model_get_current_lr(self.h))

    @property
    def uses_graph(self) -> bool: return bool(lib().flexflow_model_uses_graph(self.h))
    def set_trace_mode(self, mode: int): lib().flexflow_model_set_trace_mode(self.h, int(mode))
    def trace_replays(self, trace_id: int = 111) -> bool: return bool(lib().flexflow_model_trace_replays(self.h, trace_id))
    def counter(self, name: str) -> int: return int(lib().flexflow_model_get_counter(self.h, name.encode()))
    @property
    def backend(self) -> dict:
        """the kernel library this model loaded: {'name': ffh_backend_name(), 'path': file}"""
        return {"name": lib().flexflow_model_get_backend_name(self.h).decode(), "path": lib().flexflow_model_get_backend_path(self.h).decode()}

    def perf_metrics(self) -> PerfMetrics:
        p = PerfMetrics()
        lib().flexflow_model_get_perf_metrics(self.h, C.byref(p))
        return p

    def bce_loss(self) -> float:
        """log-loss sum of the training batches since reset_metrics() (LOSS_BCE)"""
        return float(lib().flexflow_perf_metrics_get_bce_loss(self.h))

    # -- held-out evaluation (include/ff_hip_ctr.h) -----------------------------------------------
    def eval_batch(self): lib().flexflow_model_eval_batch(self.h)
    def reset_eval_metrics(self): lib().flexflow_model_reset_eval_metrics(self.h)

    def eval_metrics(self, histograms=False) -> dict:
        """Global figures of the eval_batch() calls since reset_eval_metrics(): samples, positives, correct, nan_predictions, logloss_sum,
        logloss, accuracy, auc; with histograms=True also hist_pos / hist_neg (uint64 numpy arrays, flexflow_auc_bins() bins)."""
        e = EvalMetricsC()
        hp = hn = None
        if histograms:
            import numpy as np
            k = lib().flexflow_auc_bins()
            hp, hn = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
        lib().flexflow_model_get_eval_metrics(self.h, C.byref(e), hp.ctypes.data if histograms else None, hn.ctypes.data if histograms else None)
        out = _eval_dict(e)
        if histograms:
            out["hist_pos"], out["hist_neg"] = hp, hn
        return out

    def close(self):
        if self._owned and self.h is not None:
            lib().flexflow_model_destroy(self.h)
            self.h = None


class AdagradOptimizer:
    """Adagrad with torch.optim.Adagrad's element-wise rule (include/ff_hip_adagrad.h; adagrad_reference restates it) as the optimizer of `model`:
    MLPs, cross layers and replicated tables in one dense launch, the other tables on the fused sorted-segments update (weight_decay == 0) or the dense
    table path.  epsilon / initial_accumulator None: the config's (--adagrad-eps, default 1e-10; --adagrad-initial-accumulator, default 0).  Needs a
    kernel library with the Adagrad extension: compile() refuses the model otherwise.
    rowwise=True (or the config's adagrad_rowwise / --adagrad-rowwise): the tables keep ONE accumulator per row, the running sum of the row's mean
    squared gradient (include/ff_hip_rowwise.h; rowwise_adagrad_reference restates it), on the fused update only; the dense slab stays element-wise."""

    def __init__(self, model: "FFModel", lr=0.01, weight_decay=0.0, epsilon=None, initial_accumulator=None, rowwise=False):
        nan = float("nan")
        self.h = lib().flexflow_adagrad_optimizer_create(model.h, lr, weight_decay, nan if epsilon is None else float(epsilon),
                                                         nan if initial_accumulator is None else float(initial_accumulator))
        if rowwise:
            lib().flexflow_adagrad_optimizer_set_rowwise(self.h, 1)
        lib().flexflow_model_set_adagrad_optimizer(model.h, self.h)
        model._opt = self


class DLRM:
    """examples/cpp/DLRM as a library object: same flags as the reference driver."""

    def __init__(self, argv, comm: "FFComm | None" = None):
        full = ["dlrm"] + [str(a) for a in argv]
        self._comm = comm
        self.h = lib().flexflow_dlrm_create(len(full), _argv(full), C.byref(comm) if comm is not None else None)
        self.model = FFModel(_handle=lib().flexflow_dlrm_get_model(self.h))

    num_samples = property(lambda s: lib().flexflow_dlrm_get_num_samples(s.h))
    num_tables = property(lambda s: lib().flexflow_dlrm_get_num_tables(s.h))
    embedding_pooling = property(lambda s: lib().flexflow_dlrm_get_embedding_pooling(s.h).decode())      # --embedding-pooling: "sum" or "mean"
    bag_fill = property(lambda s: float(lib().flexflow_dlrm_get_bag_fill(s.h)))      # --synthetic-bag-fill: the share of a synthetic bag's slots that hold a lookup (1: every slot)
    bag_sizes = property(lambda s: [lib().flexflow_dlrm_get_bag_size(s.h, t) for t in range(s.num_tables)])      # ids per sample, per table (--embedding-bag-size / --embedding-bag-sizes)
    start_epoch = property(lambda s: lib().flexflow_dlrm_get_start_epoch(s.h))      # --load-checkpoint: the epochs the checkpoint had completed
    def sparse_input(self, t) -> Tensor: return Tensor(lib().flexflow_dlrm_get_sparse_input(self.h, t), self.model)
    def dense_input(self) -> Tensor: return Tensor(lib().flexflow_dlrm_get_dense_input(self.h), self.model)
    def label_input(self) -> Tensor:
        """the labels of the batch the latest step trained on (this rank's rows), beside sparse_input / dense_input"""
        return self.model.label_tensor
    def warmup(self): lib().flexflow_dlrm_warmup(self.h)
    def train_steps(self, n, trace=True): lib().flexflow_dlrm_train_steps(self.h, n, trace)
    def run_epochs(self) -> float: return lib().flexflow_dlrm_run_epochs(self.h)
    def evaluate(self, epoch=0) -> dict:
        """--eval-batches: the held-out batches through eval_batch(), as the driver does after an epoch (prints its EVAL line)"""
        e = EvalMetricsC()
        secs = lib().flexflow_dlrm_evaluate(self.h, epoch, C.byref(e))
        return dict(_eval_dict(e), seconds=float(secs))

    def time_kernel(self, which, iters) -> float: return lib().flexflow_dlrm_time_kernel(self.h, which, iters)

    PROBE_PAIRS = ("gather", "table_update", "alltoall_fwd", "alltoall_bwd", "allreduce", "join_wait", "allreduce_wait") + tuple(f"bucket{i}" for i in range(8))

    def probe_step(self, iters) -> dict:
        """In-step event intervals (milliseconds, averaged over `iters` real eager steps): the side-stream gather (+ forward exchange)
        and table update (+ backward exchange), each collective alone, and the compute stream's wait for the embedding branch -- the
        exposed part of gather + exchange.  COLLECTIVE: with more than one rank every rank must call it."""
        out = (C.c_float * len(self.PROBE_PAIRS))()
        lib().flexflow_dlrm_probe_step(self.h, iters, out, len(self.PROBE_PAIRS))
        return {k: float(out[i]) for i, k in enumerate(self.PROBE_PAIRS)}

    def close(self):
        if self.h is not None:
            lib().flexflow_dlrm_destroy(self.h)
            self.h = None
