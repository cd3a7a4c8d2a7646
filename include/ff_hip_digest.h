/* ff_hip_digest.h -- optional extension of the kernel C-ABI (include/ff_hip.h): a 64-bit digest of a strided device buffer.
 *
 * A library may export this list or not; include/ff_hip.h and its symbol list are unchanged by it.  libffhip.so exports it,
 * the CPU oracle does not.  Callers load it separately (host/backend: KernelApi::digest, null when absent; capi.digest_api(lib)).
 * A checkpoint carries one digest per record, loading verifies each one after the host-to-device copy, and two models compare their
 * whole state without copying it out.
 *
 * DEFINITION (stated once, below, as inline host/device functions; the kernel, the host layer and the Python binding compile these)
 *   rows rows of row_bytes bytes (even, >= 2), ld_bytes apart;  W = ceil(row_bytes / 8)
 *   word(r, w) = the little-endian 8 bytes at offset 8 w of row r, bytes past row_bytes read as zero
 *   i          = index_base + r W + w                                    (64-bit, wrapping)
 *   digest     = sum over r, w of ffh_mix64(ffh_hash(seed, i) ^ word(r, w))    mod 2^64
 *   The sum is a wrapping integer sum: every summation order gives the same bits.  Pad bytes between row_bytes and ld_bytes never enter.
 *   A swap of two unequal words and a flip of one bit both change it (the position is hashed into every term).
 *
 * CONTRACT of ffh_state_digest
 *   *acc += digest: the caller clears acc (one uint64 in device memory, 8-byte aligned) with ffh_zero.  Several tensors fold into one
 *   word with distinct seeds; index_base lets a caller digest a large tensor in pieces: rows [0, a) plus rows [a, n) with
 *   index_base = a W is the whole.
 *   Requires rows >= 0, row_bytes even and >= 2, ld_bytes even and >= row_bytes, base 2-byte aligned, acc 8-byte aligned; anything else is
 *   FFH_ERR_BAD_ARG with nothing launched.  rows == 0 launches nothing.  Nothing is written but *acc; nothing outside the row_bytes
 *   bytes of a row is read.
 *   One memory-bound grid-stride launch on the caller's stream with arguments that do not change from call to call (capturable), no
 *   allocation, no scratch, no environment variable.  A lane moves 16 bytes where base and ld_bytes are multiples of 16, 8 bytes where
 *   they are multiples of 8, and assembles the same words from 4- or 2-byte loads otherwise: one choice per launch, made on the host.
 *   The lanes' sums are reduced in the wave and the workgroup; one 64-bit integer atomic add per workgroup reaches *acc (integer: the
 *   result is the same bits on every run).
 */
#ifndef FF_HIP_DIGEST_H_
#define FF_HIP_DIGEST_H_

#include "ff_hip.h"
#include "ffh_rng.h"

#define FFH_DIGEST_ABI_VERSION 1

/* words per row */
FFH_HD int64_t ffh_digest_row_words(int64_t row_bytes) { return (row_bytes + 7) / 8; }

/* ffh_hash(seed, i) with the seed's half done once: key = ffh_digest_key(seed) */
FFH_HD uint64_t ffh_digest_key(uint64_t seed) { return ffh_mix64(seed); }

/* one term of the sum: word `word` at index i */
FFH_HD uint64_t ffh_digest_term(uint64_t key, uint64_t i, uint64_t word) { return ffh_mix64(ffh_mix64(key + i) ^ word); }

/* the seed of record `ordinal` of a checkpoint (host/checkpoint.cc, ffmodel.read_checkpoint) */
FFH_HD uint64_t ffh_digest_record_seed(uint64_t ordinal) { return ffh_hash(0x46464843484B5054ULL, ordinal); }

/* the definition on host memory: what ffh_state_digest adds to *acc */
static inline uint64_t ffh_state_digest_host(const void* base, int64_t rows, int64_t row_bytes, int64_t ld_bytes, uint64_t seed, uint64_t index_base) {
  const uint64_t key = ffh_digest_key(seed);
  const int64_t W = ffh_digest_row_words(row_bytes);
  uint64_t sum = 0;
  for (int64_t r = 0; r < rows; r++) {
    const unsigned char* row = (const unsigned char*)base + r * ld_bytes;
    for (int64_t w = 0; w < W; w++) {
      uint64_t word = 0;
      const int64_t n = row_bytes - 8 * w < 8 ? row_bytes - 8 * w : 8;
      for (int64_t b = 0; b < n; b++) word |= (uint64_t)row[8 * w + b] << (8 * b);
      sum += ffh_digest_term(key, index_base + (uint64_t)r * (uint64_t)W + (uint64_t)w, word);
    }
  }
  return sum;
}

#ifdef __cplusplus
extern "C" {
#endif

int ffh_digest_abi_version(void);

int ffh_state_digest(ffh_ctx* ctx, const void* base, int64_t rows, int64_t row_bytes, int64_t ld_bytes, uint64_t seed, uint64_t index_base,
                     uint64_t* acc, ffh_stream stream);

#ifdef __cplusplus
}
#endif

#define FFH_DIGEST_API_LIST(X) \
  X(ffh_digest_abi_version) X(ffh_state_digest)

#endif /* FF_HIP_DIGEST_H_ */
