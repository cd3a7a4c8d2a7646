// digest.hip -- include/ff_hip_digest.h: a 64-bit digest of a strided device buffer (checkpoint records, whole-model state comparison).
//
// One memory-bound pass: a grid-stride walk of at most 2048 workgroups over (row, column group) positions, as csrc/cross.hip walks its
// operands -- a lane keeps its position as (row, group) and advances it by the grid's stride split the same way, so the loop has no
// division and row * ld_bytes is 64-bit arithmetic.  A group is 16 bytes (two words of the definition) where base and ld_bytes are
// multiples of 16, and one word otherwise, read as one 8-byte load, two 4-byte loads or four 2-byte loads: the host picks the widest form
// the alignment allows, once per launch.  The last word of a row whose length is no multiple of 8 is assembled from 2-byte loads in every
// form (row_bytes is even), so no load ever touches a byte behind row_bytes.
// Each word costs two ffh_mix64 (four 64-bit multiplies: the seed's half of ffh_hash is done on the host).  The lanes' wrapping sums are
// reduced by shuffles in the wave, through LDS in the workgroup, and reach *acc as ONE 64-bit integer vector atomic add per workgroup: an
// integer sum, so the order in which the workgroups arrive does not show in the result.
#include "ffh_common.h"

#include "../../include/ff_hip_digest.h"

namespace {

constexpr int kThreads = 256;

struct Walk {
  int64_t rows, groups, step_r, step_c;
};

__device__ __forceinline__ uint64_t ld_u16(const unsigned char* p) { return (uint64_t)*reinterpret_cast<const uint16_t*>(p); }

// the last word of a row: rem = 2, 4 or 6 bytes of it exist
__device__ __forceinline__ uint64_t load_tail(const unsigned char* p, int64_t rem) {
  uint64_t w = ld_u16(p);
  if (rem >= 4) w |= ld_u16(p + 2) << 16;
  if (rem >= 6) w |= ld_u16(p + 4) << 32;
  return w;
}

// the word at p (rem > 0 bytes of the row left from p on), by loads of LW bytes
template <int LW>
__device__ __forceinline__ uint64_t load_word(const unsigned char* p, int64_t rem) {
  if (rem < 8) return load_tail(p, rem);
  if (LW >= 8) return *reinterpret_cast<const uint64_t*>(p);
  if (LW == 4) return (uint64_t)*reinterpret_cast<const uint32_t*>(p) | ((uint64_t)*reinterpret_cast<const uint32_t*>(p + 4) << 32);
  return ld_u16(p) | (ld_u16(p + 2) << 16) | (ld_u16(p + 4) << 32) | (ld_u16(p + 6) << 48);
}

template <int LW>
__global__ __launch_bounds__(kThreads) void state_digest_kernel(const unsigned char* base, int64_t row_bytes, int64_t ld_bytes, int64_t words, uint64_t key,
                                                                uint64_t index_base, unsigned long long* acc, const Walk w) {
  ffh_kernel_prio();
  constexpr int kGroupBytes = LW == 16 ? 16 : 8;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t r = t / w.groups, c = t - r * w.groups;
  uint64_t sum = 0;
  while (r < w.rows) {
    const int64_t off = c * kGroupBytes;
    const unsigned char* p = base + r * ld_bytes + off;
    const int64_t rem = row_bytes - off;                     // > 0: groups = ceil(row_bytes / kGroupBytes)
    const uint64_t i = index_base + (uint64_t)r * (uint64_t)words + (uint64_t)(off >> 3);
    if (LW == 16) {
      if (rem >= 16) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p);
        sum += ffh_digest_term(key, i, v.x) + ffh_digest_term(key, i + 1, v.y);
      } else {
        sum += ffh_digest_term(key, i, load_word<8>(p, rem));
        if (rem > 8) sum += ffh_digest_term(key, i + 1, load_tail(p + 8, rem - 8));
      }
    } else {
      sum += ffh_digest_term(key, i, load_word<LW>(p, rem));
    }
    r += w.step_r; c += w.step_c;
    if (c >= w.groups) { c -= w.groups; r++; }
  }
  // wave, then workgroup, then one atomic
  for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_down((unsigned long long)sum, d, kWave);
  __shared__ unsigned long long part[kThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < kThreads / kWave; k++) total += part[k];
    atomicAdd(acc, total);
  }
}

}  // namespace

extern "C" {

int ffh_digest_abi_version(void) { return FFH_DIGEST_ABI_VERSION; }

int ffh_state_digest(ffh_ctx* c, const void* base, int64_t rows, int64_t row_bytes, int64_t ld_bytes, uint64_t seed, uint64_t index_base, uint64_t* acc,
                     ffh_stream s) {
  FFH_REQUIRE(c, rows >= 0, "state_digest: rows must be >= 0");
  FFH_REQUIRE(c, row_bytes >= 2 && (row_bytes & 1) == 0, "state_digest: row_bytes must be even and >= 2");
  FFH_REQUIRE(c, ld_bytes >= row_bytes && (ld_bytes & 1) == 0, "state_digest: ld_bytes must be even and >= row_bytes");
  FFH_REQUIRE(c, acc && ((uintptr_t)acc & 7) == 0, "state_digest: acc must be an 8-byte aligned device word");
  FFH_REQUIRE(c, (base || rows == 0) && ((uintptr_t)base & 1) == 0, "state_digest: base must be a 2-byte aligned device address");
  FFH_REQUIRE(c, rows == 0 || ld_bytes <= INT64_MAX / rows, "state_digest: rows * ld_bytes overflows");
  if (rows == 0) return FFH_OK;
  const uintptr_t align = (uintptr_t)base | (uintptr_t)ld_bytes;
  const int lw = (align & 15) == 0 ? 16 : (align & 7) == 0 ? 8 : (align & 3) == 0 ? 4 : 2;
  const int64_t words = ffh_digest_row_words(row_bytes);
  Walk w;
  w.rows = rows;
  w.groups = lw == 16 ? (row_bytes + 15) / 16 : words;
  FFH_REQUIRE(c, w.groups <= INT64_MAX / rows, "state_digest: too many words");
  const unsigned grid = ffh_grid(rows * w.groups, kThreads);
  const int64_t stride = (int64_t)grid * kThreads;
  w.step_r = stride / w.groups;
  w.step_c = stride % w.groups;
  const uint64_t key = ffh_digest_key(seed);
  const unsigned char* b = (const unsigned char*)base;
  unsigned long long* a = (unsigned long long*)acc;
#define FFH_DIGEST_LAUNCH(LW) \
  hipLaunchKernelGGL((state_digest_kernel<LW>), dim3(grid), dim3(kThreads), 0, as_stream(s), b, row_bytes, ld_bytes, words, key, index_base, a, w)
  if (lw == 16) FFH_DIGEST_LAUNCH(16);
  else if (lw == 8) FFH_DIGEST_LAUNCH(8);
  else if (lw == 4) FFH_DIGEST_LAUNCH(4);
  else FFH_DIGEST_LAUNCH(2);
#undef FFH_DIGEST_LAUNCH
  FFH_LAUNCH_CHECK(c, "state_digest");
  return FFH_OK;
}

}  // extern "C"
