// emb_gather.h -- what the gathers from fp32 / bf16 tables (embedding_fwd.hip) and from 8-bit rows (embedding_q8.hip) share: the store
// epilogue (store_row: the fp32 row and, beside it, the destination's bf16 twin and three-plane image), the ragged kernels' workgroup map
// (bag_blocks, kBagLong) and the host's lookup of every destination's twin / image (gather_dests).
// Internal: no kernel, nothing exported.  kBagMaxL is emb_tables.h.  The lane geometry, RowLanes, stays in embedding_fwd.hip, where
// tests/test_stream_cap_cpu.py reads it; embedding_q8.hip carries the same struct.
#pragma once
#include "emb_tables.h"

namespace ffh_emb {

// The store epilogue: vector `c` of output row `b` from one row's sums -- the fp32 row, and beside it the bf16 twin (o16) and the
// three-plane image (o3, column o3c) where the destination has one.
template <int VEC>
__device__ __forceinline__ void store_row(const ffh_emb_table& tb, unsigned short* const o16, char* const o3, const int o3c,
                                          const int64_t b, const int c, const float (&acc)[VEC], const bool avg, const float inv) {
  constexpr int NQ = VEC / 4;                     // 16-B groups of output floats per lane-access (0: scalar)
  float f[VEC];
#pragma unroll
  for (int v = 0; v < VEC; v++) f[v] = avg ? acc[v] * inv : acc[v];
  if constexpr (NQ == 0) {
    tb.io[b * tb.ld + c] = f[0];
  } else {
#pragma unroll
    for (int h = 0; h < NQ; h++) {
      const int q = c * NQ + h;                 // float4 index in the output row
      const float* g = f + 4 * h;
      typedef float f4 __attribute__((ext_vector_type(4)));
      const f4 o = {g[0], g[1], g[2], g[3]};
      reinterpret_cast<f4*>(tb.io + b * tb.ld)[q] = o;
      if (o16) {      // the twin the first top-MLP GEMM reads its operand from (ffh_ctx_bf16_mirror_set)
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        const bf2 lo = {(__bf16)g[0], (__bf16)g[1]}, hi = {(__bf16)g[2], (__bf16)g[3]};
        reinterpret_cast<uint2*>(o16 + b * tb.ld)[q] = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
      }
      if (o3) {       // split mode: the three-plane image of the row piece (ffh_ctx_bf16x3_mirror_set; ld a multiple of 32)
        uint2 p1, p2, p3;
        ffh_split_bf16x3(make_float4(g[0], g[1], g[2], g[3]), p1, p2, p3);
        char* d = o3 + b * tb.ld * 6 + ffh_i32_off(o3c + 4 * q);
        *reinterpret_cast<uint2*>(d) = p1; *reinterpret_cast<uint2*>(d + 64) = p2; *reinterpret_cast<uint2*>(d + 128) = p3;
      }
    }
  }
}

constexpr int kBagLong = 4;        // bags of at least this many ids take the JU = 4 form

__host__ __device__ inline int64_t bag_blocks(int64_t batch, int L, int shift, int64_t nrb) {
  int64_t w = (batch * (int64_t)L) >> shift;
  w = w < 1 ? 1 : w;
  return w > nrb ? nrb : w;
}

// The tables into the kernel arguments (EmbArgs / BagArgs), each with the registered twin and image of its destination.
template <class Args>
void gather_dests(const ffh_ctx* c, const ffh_emb_table* tables, int nt, int D, int64_t batch, int vec, Args& a) {
  for (int i = 0; i < nt; i++) {
    a.t[i] = tables[i];
    const size_t span = (size_t)((batch - 1) * tables[i].ld + D) * 4;
    // tensor-op mode with a registered twin of the destination: the gather writes the bf16 roundings beside the fp32 rows
    a.out16[i] = (vec >= 4 && tables[i].ld % 4 == 0) ? ffh_mirror_of(c, tables[i].io, span) : nullptr;
    // split mode with a registered image of the destination (rows a whole number of 32-element groups apart): the three terms beside the fp32 rows
    int col0 = 0;
    a.out3[i] = (vec >= 4 && tables[i].ld % 32 == 0) ? ffh_planes_of(c, tables[i].io, span, &col0) : nullptr;
    a.out3c[i] = col0;      // (0 .. 31: BagArgs keeps it in 8 bits)
    if (a.out3[i] && (col0 & 3)) a.out3[i] = nullptr;
  }
}

}  // namespace ffh_emb
