/* ffh_bf16.h -- the scalar rules of bf16 embedding tables (include/ff_hip_bf16.h).
 *
 * One statement of the rules for the HIP kernels, host code and tests:
 *   - a stored bf16 value widens to fp32 exactly (the 16 bits are the high half of the fp32 pattern);
 *   - initialisation and set_weights round to nearest even (ffh_bf16_rne); a NaN stays a NaN (its sign kept, quieted) --
 *     the bare integer trick (u + 0x7FFF + lsb) >> 16 would turn some NaNs into a zero or an infinity;
 *   - the table update computes w32 = fmaf(-lr, sum, (float)w16) exactly as the fp32 update does, then rounds once:
 *     nearest (ffh_bf16_rne) or stochastic (ffh_bf16_sr: add 16 random bits to the fp32 pattern and truncate; an infinity
 *     passes unchanged, a NaN as in ffh_bf16_rne).
 * The 16 random bits of element (table, row, col) at update number `iter` of stream `seed` (ffh_bf16_sr_bits) are a function
 * of those five numbers only -- global row and column, global table index -- so they do not depend on launch geometry, the form
 * the update takes, table placement or the number of ranks.  `iter` is read from device memory by the update kernels and
 * advanced by ffh_bf16_counter_advance, so a step replayed from a captured graph draws fresh bits.
 */
#ifndef FFH_BF16_H_
#define FFH_BF16_H_

#include <stdint.h>

#include "ffh_rng.h"

#define FFH_BF16_ROUND_STOCHASTIC 0
#define FFH_BF16_ROUND_NEAREST    1

FFH_HD uint32_t ffh_f32_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
#endif
}

FFH_HD float ffh_bits_f32(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}

/* exact widening */
FFH_HD float ffh_bf16_to_f32(uint16_t h) { return ffh_bits_f32((uint32_t)h << 16); }

/* NaN: sign and the top payload bits kept, quiet bit set */
FFH_HD uint16_t ffh_bf16_nan(uint32_t u) { return (uint16_t)((u >> 16) | 0x0040u); }

/* round to nearest even */
FFH_HD uint16_t ffh_bf16_rne(float f) {
  const uint32_t u = ffh_f32_bits(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return ffh_bf16_nan(u);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

/* stochastic: r (16 bits) added below the kept bits, then truncation; +-Inf unchanged, NaN as ffh_bf16_rne */
FFH_HD uint16_t ffh_bf16_sr(float f, uint32_t r) {
  const uint32_t u = ffh_f32_bits(f);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return ffh_bf16_nan(u);
  if (a == 0x7F800000u) return (uint16_t)(u >> 16);
  return (uint16_t)((u + (r & 0xFFFFu)) >> 16);
}

FFH_HD uint16_t ffh_bf16_round(float f, int mode, uint32_t r) {
  return mode == FFH_BF16_ROUND_NEAREST ? ffh_bf16_rne(f) : ffh_bf16_sr(f, r);
}

/* the key of one (update, table, row): three chained ffh_hash steps */
FFH_HD uint64_t ffh_bf16_sr_table_key(uint64_t seed, uint64_t iter, uint64_t table) {
  return ffh_hash(ffh_hash(seed, iter), table);
}
FFH_HD uint64_t ffh_bf16_sr_row_key(uint64_t table_key, uint64_t row) { return ffh_hash(table_key, row); }

/* 64 bits per group of four columns (4k .. 4k+3); column c takes the 16-bit field c & 3 */
FFH_HD uint64_t ffh_bf16_sr_group(uint64_t row_key, uint64_t col) { return ffh_mix64(row_key + (col >> 2)); }
FFH_HD uint32_t ffh_bf16_sr_field(uint64_t group, uint64_t col) { return (uint32_t)(group >> (16 * (col & 3))) & 0xFFFFu; }

FFH_HD uint32_t ffh_bf16_sr_bits(uint64_t seed, uint64_t iter, uint64_t table, uint64_t row, uint64_t col) {
  return ffh_bf16_sr_field(ffh_bf16_sr_group(ffh_bf16_sr_row_key(ffh_bf16_sr_table_key(seed, iter, table), row), col), col);
}

#endif /* FFH_BF16_H_ */
