"""Shared by the tests of 8-bit embedding rows (tests/test_q8_cpu.py, tests/test_gpu_q8.py): tables with the rows that try the rule of
include/ff_hip_q8.h, and their packed images by the numpy restatement in dlrm_flexflow_amd.ffmodel."""
import numpy as np

import bf16_helpers as B16
from dlrm_flexflow_amd import ffmodel


def row_bytes_for(D, padded):
    """D + 8 (the default, fbgemm's layout), or that rounded up to 16 (zero padding behind the bias)."""
    return (D + 8 + 15) // 16 * 16 if padded else D + 8


def special_rows(D, rng):
    """Rows that try the rule: all -0, constant, one outlier, a range below 1e-8, the minimum in the last column with the maximum in the
    first, magnitudes 1e30 and 1e-30, and a row of exact ties (k + 0.5 before rounding: half to even)."""
    f = np.float32
    rows = []
    rows.append(np.full(D, -0.0, f))
    rows.append(np.full(D, 0.3, f))
    r = (rng.standard_normal(D) * 0.01).astype(f); r[D // 2] = 50.0
    rows.append(r)
    rows.append((rng.random(D) * 5e-9).astype(f))
    r = rng.random(D).astype(f); r[0] = 3.0; r[-1] = -2.0
    rows.append(r)
    rows.append((rng.standard_normal(D) * 1e30).astype(f))
    rows.append((rng.standard_normal(D) * 1e-30).astype(f))
    r = (np.arange(D) % 256).astype(f) * f(0.5); r[0] = 0.0; r[-1] = 127.5      # range 127.5: x * 2 lands on whole codes and ties stay rare
    rows.append(r)
    return np.stack(rows)


def make_table(rng, rows, D, bf16=False, special=True):
    """A [rows][D] float32 table, the special rows first where they fit; bf16: values a bf16 holds (the widened table)."""
    w = rng.standard_normal((rows, D)).astype(np.float32)
    if special:
        s = special_rows(D, rng)
        n = min(rows, len(s))
        w[:n] = s[:n]
    if bf16:
        w = B16.widen(B16.rne(w)).astype(np.float32)
    return w


def pack(w, row_bytes=None):
    """uint8 [rows][row_bytes]: the image the quantizer must leave for table w."""
    return ffmodel.q8_pack_rows(*ffmodel.q8_quantize_reference(w), row_bytes=row_bytes)


def dequantized(w):
    return ffmodel.q8_dequantize_reference(*ffmodel.q8_quantize_reference(w))
