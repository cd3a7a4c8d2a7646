// emb_row_rules.h -- what happens to a touched table row once its gradient sum is complete: the row rules of the fused table update
// (embedding.hip), their parameters, and the one spelling of each access to a weight or state row.  Device code shared by the update
// kernels (emb_reduce.h), compiled once per weight type (embedding_update_f32.hip, embedding_update_bf16.hip).
#pragma once

#include "ffh_common.h"
#include "../../include/ff_hip_bf16.h"
#include "../../include/ffh_bf16.h"
#include "../../include/ff_hip_adagrad.h"
#include "../../include/ff_hip_rowwise.h"

#include <stddef.h>
#include <type_traits>

namespace ffh_emb {

constexpr int kMaxChunks = 4;   // row chunks per lane: D <= 4*64*4 = 1024 (vector) / 256 (scalar)

// The update kernels take two independent template parameters (ffh_sparse_opt, include/ff_hip.h):
//   RowRule R  the rule.  Sgd: the fused update of SURVEY 8a-4, w = fmaf(-lr, sum, w), no state.  Momentum: sgd_update with weight decay /
//              momentum / nesterov, s0 = V.  Adam: adam_update, s0 = M, s1 = V.  Adagrad (include/ff_hip_adagrad.h): s0 = S.  The element
//              arithmetic is that of sgd_kernel / adam_kernel / adagrad_element (elementwise.hip) statement by statement, so a row hit by one
//              gradient row ends up with the bits the dense optimizer gives that row.  RowwiseAdagrad (include/ff_hip_rowwise.h): s0 = S, ONE
//              float per row; the rule needs the whole row before it can update any of it (apply_row_rowwise, not apply_row).
//   class WT   the weight type, as in emb_fwd_kernel.  float: fp32 rows.  uint16_t: bf16 rows (ff_hip_bf16.h): the rule runs on the widened
//              row w = (float)w16 with fp32 state, statement by statement as on an fp32 table, then ONE rounding (ffh_bf16.h) keyed by the
//              update counter, table, global row and column (sr_* / SrKey; sr_counter: the update number in device memory).
enum class RowRule { Sgd, Momentum, Adam, Adagrad, RowwiseAdagrad };
constexpr bool opt_plain(RowRule r) { return r == RowRule::Sgd; }                  // no optimizer state
constexpr bool opt_state(RowRule r) { return r != RowRule::Sgd; }
constexpr bool opt_rowwise(RowRule r) { return r == RowRule::RowwiseAdagrad; }     // the row is applied whole (apply_row_rowwise), its state is one float
template <class WT> constexpr bool is_bf16() { return std::is_same<WT, uint16_t>::value; }      // 16-bit weight rows
// ffh_sparse_opt.kind -> the rule; false: no such kind
inline bool row_rule_of(int kind, RowRule* r) {
  switch (kind) {
    case FFH_SPARSE_OPT_SGD: *r = RowRule::Sgd; return true;
    case FFH_SPARSE_OPT_SGD_MOMENTUM: *r = RowRule::Momentum; return true;
    case FFH_SPARSE_OPT_ADAM: *r = RowRule::Adam; return true;
    case FFH_SPARSE_OPT_ADAGRAD: *r = RowRule::Adagrad; return true;
    case FFH_SPARSE_OPT_ROWWISE_ADAGRAD: *r = RowRule::RowwiseAdagrad; return true;
  }
  return false;
}

// lr_src_lo / _hi (include/ff_hip_lr.h): the two halves of the address the LRP instantiations of the kernels read lr from, once per wave; zero and
// unread otherwise.  They sit in the two 4-byte holes the struct already had (behind nesterov and behind sr_mode), so no member moves and the
// kernel arguments do not grow: the instantiations the scalar entries launch read every argument where they always did.
struct OptP { float lr, wd, mom, b1, b2, eps, omb1, omb2; int nesterov; uint32_t lr_src_lo; int64_t nt_rows;   // nt_rows: tables of more rows have their rows read and written nontemporal (plain SGD, 16-byte form)
              int sr_mode; uint32_t lr_src_hi; uint64_t sr_seed; const uint64_t* sr_counter; };
static_assert(sizeof(OptP) == 72, "OptP: the rate address must fit in the padding it replaced");
static inline void opt_set_lr_src(OptP& o, const float* p) { o.lr_src_lo = (uint32_t)(uintptr_t)p; o.lr_src_hi = (uint32_t)((uintptr_t)p >> 32); }
__host__ __device__ __forceinline__ const float* opt_lr_src(const OptP& o) { return reinterpret_cast<const float*>(((uintptr_t)o.lr_src_hi << 32) | o.lr_src_lo); }
// the row rule as the kernel applies it: LRP = false: the kernel arguments' own (no copy, the instructions of before); LRP = true: a copy with
// lr loaded from that address -- a uniform address, so one scalar load per wave
#define FFH_OPT_OF(LRP, name, args_op)                                   \
  OptP name##_l;                                                          \
  if (LRP) { name##_l = (args_op); name##_l.lr = *opt_lr_src(args_op); }    \
  const OptP& name = LRP ? name##_l : (args_op)

struct Bf16Keys { int32_t table[FFH_MAX_TABLES]; int32_t col0[FFH_MAX_TABLES]; };   // bf16 rows, every rule but Adam: in place of the (unused) s1 pointers
// Adam on bf16 rows needs the s1 pointers AND the keys: at most FFH_BF16_MAX_STATEFUL_TABLES tables, both in the space of s1[FFH_MAX_TABLES]
struct Bf16AdamKeys { float* s1[FFH_BF16_MAX_STATEFUL_TABLES]; int32_t table[FFH_BF16_MAX_STATEFUL_TABLES]; int32_t col0[FFH_BF16_MAX_STATEFUL_TABLES]; };
static_assert(sizeof(Bf16AdamKeys) <= sizeof(float*) * FFH_MAX_TABLES && sizeof(Bf16Keys) <= sizeof(float*) * FFH_MAX_TABLES, "bf16 keys in the s1 space");
struct SrKey { uint64_t tkey; int64_t col0; };                                      // per table: ffh_bf16_sr_table_key, global column of column 0
namespace {      // device code: internal linkage, as in the one translation unit this was (the inliner treats it differently otherwise)

// a kernel's arguments (RedArgs, SmallArgs): the table's second state row pointer and its rounding key, wherever (R, WT) keeps them
template <RowRule R, class WT, class A>
__device__ __forceinline__ float* state1_of(const A& a, int tix) {
  if (R != RowRule::Adam) return nullptr;
  return is_bf16<WT>() ? a.b16a.s1[tix] : a.s1[tix];
}
template <RowRule R, class WT, class A>
__device__ __forceinline__ SrKey sr_key(const A& a, int tix) {
  SrKey r{0, 0};
  if (is_bf16<WT>()) {
    const int32_t table = R == RowRule::Adam ? a.b16a.table[tix] : a.b16.table[tix];
    r.col0 = R == RowRule::Adam ? a.b16a.col0[tix] : a.b16.col0[tix];
    if (a.op.sr_mode == FFH_BF16_ROUND_STOCHASTIC) r.tkey = ffh_bf16_sr_table_key(a.op.sr_seed, *a.op.sr_counter, (uint64_t)table);
  }
  return r;
}
// the row's first element: fp32 tables and bf16 tables alike come in as `float* weight` (ffh_emb_table; the bf16 entry points cast)
template <class WT>
__device__ __forceinline__ float* weight_row(float* w, uint32_t row, int D) {
  return reinterpret_cast<float*>(reinterpret_cast<WT*>(w) + (int64_t)row * D);
}
// the row's stochastic-rounding key (ffh_bf16_sr_row_key), once per row rather than per vector of it; 0 where unused
template <class WT>
__device__ __forceinline__ uint64_t sr_row_key(const OptP& o, const SrKey& sk, uint32_t row) {
  return (is_bf16<WT>() && o.sr_mode == FFH_BF16_ROUND_STOCHASTIC) ? ffh_bf16_sr_row_key(sk.tkey, row) : 0;
}

// vector c of a weight row, widened to fp32.  `nt`: a nontemporal access (plain SGD on the tables above OptP::nt_rows)

typedef float emb_f4 __attribute__((ext_vector_type(4)));
typedef unsigned emb_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void widen_bf16x4(float (&wv)[4], const uint2 v) {
  wv[0] = ffh_bf16_to_f32((uint16_t)v.x); wv[1] = ffh_bf16_to_f32((uint16_t)(v.x >> 16));
  wv[2] = ffh_bf16_to_f32((uint16_t)v.y); wv[3] = ffh_bf16_to_f32((uint16_t)(v.y >> 16));
}
template <int VEC, class WT>
__device__ __forceinline__ void load_weights(float (&wv)[VEC], const float* wrow, int c, const bool nt) {
  if constexpr (is_bf16<WT>()) {
    const uint16_t* const w16 = reinterpret_cast<const uint16_t*>(wrow);
    if constexpr (VEC == 4) {
      uint2 v;
      if (nt) { const emb_u2 t = __builtin_nontemporal_load(reinterpret_cast<const emb_u2*>(w16) + c); v = make_uint2(t.x, t.y); }
      else v = reinterpret_cast<const uint2*>(w16)[c];
      widen_bf16x4(wv, v);
    } else {
      wv[0] = ffh_bf16_to_f32(w16[c]);
    }
  } else if constexpr (VEC == 4) {
    if (nt) {
      const emb_f4 w = __builtin_nontemporal_load(reinterpret_cast<const emb_f4*>(wrow) + c);
      wv[0] = w.x; wv[1] = w.y; wv[2] = w.z; wv[3] = w.w;
    } else {
      const float4 w = reinterpret_cast<const float4*>(wrow)[c];
      wv[0] = w.x; wv[1] = w.y; wv[2] = w.z; wv[3] = w.w;
    }
  } else {
    wv[0] = wrow[c];
  }
}
// ... and back.  bf16 rows: the one rounding of w32 with its key (global table, row, column; the update counter), packed and stored
template <int VEC, class WT>
__device__ __forceinline__ void store_weights(const OptP& o, float* wrow, int c, const float (&wv)[VEC], const SrKey& sk, uint64_t rkey, const bool nt) {
  if constexpr (is_bf16<WT>()) {
    uint16_t* const w16 = reinterpret_cast<uint16_t*>(wrow);
    uint16_t h[VEC];
    const int64_t g0 = sk.col0 + (int64_t)c * VEC;                 // global column of element 0
    const bool sr = o.sr_mode == FFH_BF16_ROUND_STOCHASTIC;
    const uint64_t grp = (sr && VEC == 4 && (g0 & 3) == 0) ? ffh_bf16_sr_group(rkey, (uint64_t)g0) : 0;      // one hash serves the four columns
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      uint32_t r = 0;
      if (sr) {
        const uint64_t gc = (uint64_t)(g0 + k);
        r = ffh_bf16_sr_field((VEC == 4 && (g0 & 3) == 0) ? grp : ffh_bf16_sr_group(rkey, gc), gc);
      }
      h[k] = ffh_bf16_round(wv[k], o.sr_mode, r);
    }
    if constexpr (VEC == 4) {
      const uint2 v = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
      if (nt) { const emb_u2 t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<emb_u2*>(w16) + c); }
      else reinterpret_cast<uint2*>(w16)[c] = v;
    } else {
      w16[c] = h[0];
    }
  } else if constexpr (VEC == 4) {
    if (nt) { const emb_f4 w = {wv[0], wv[1], wv[2], wv[3]}; __builtin_nontemporal_store(w, reinterpret_cast<emb_f4*>(wrow) + c); }
    else reinterpret_cast<float4*>(wrow)[c] = make_float4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    wrow[c] = wv[0];
  }
}
// vector c of an fp32 state row
template <int VEC>
__device__ __forceinline__ void load_state(float (&v)[VEC], const float* srow, int c) { load_weights<VEC, float>(v, srow, c, false); }
template <int VEC>
__device__ __forceinline__ void store_state(float* srow, int c, const float (&v)[VEC]) {
  if constexpr (VEC == 4) reinterpret_cast<float4*>(srow)[c] = make_float4(v[0], v[1], v[2], v[3]);
  else srow[c] = v[0];
}

// The rules on one element in registers: gradient sum g, widened weight w, state a (s0) / b (s1)
__device__ __forceinline__ void rule_sgd(const OptP& o, const float g, float& w) { w = __fmaf_rn(-o.lr, g, w); }
// sgd_update [ref: src/runtime/optimizer_kernel.cu:23-41], as sgd_kernel spells it
__device__ __forceinline__ void rule_momentum(const OptP& o, const float g, float& w, float& a) {
  float gt = __fmaf_rn(o.wd, w, g);
  if (o.mom > 0.f) {
    a = __fmaf_rn(a, o.mom, gt);
    gt = o.nesterov ? __fmaf_rn(o.mom, a, gt) : a;
  }
  w = __fmaf_rn(-o.lr, gt, w);
}
// adam_update [ref: src/runtime/optimizer_kernel.cu:206-226], as adam_kernel spells it (lr = alpha_t)
__device__ __forceinline__ void rule_adam(const OptP& o, const float g, float& w, float& a, float& b) {
#pragma clang fp contract(off)
  const float gt = fmaf(o.wd, w, g);
  const float t1 = o.omb1 * gt;
  a = fmaf(o.b1, a, t1);
  const float t2 = o.omb2 * gt;
  const float t3 = t2 * gt;
  b = fmaf(o.b2, b, t3);
  const float num = o.lr * a;
  const float den = sqrtf(b) + o.eps;
  const float step = num / den;
  w = w - step;
}
// include/ff_hip_adagrad.h: the statements of adagrad_element (elementwise.hip), a = S; weight decay is a wave-uniform branch here, a template parameter there
__device__ __forceinline__ void rule_adagrad(const OptP& o, const float g, float& w, float& a) {
#pragma clang fp contract(off)
  float gt = g;
  if (o.wd != 0.f) { const float t0 = o.wd * w; gt = g + t0; }
  const float t1 = gt * gt;
  a = a + t1;
  const float den = sqrtf(a) + o.eps;
  const float q = gt / den;
  const float t2 = o.lr * q;
  w = w - t2;
}

// vector c of a row under a per-element rule: load, the rule on each element, store
template <int VEC, RowRule R, class WT>
__device__ __forceinline__ void apply_row(const OptP& o, float* wrow, float* s0row, float* s1row, int c, const float (&acc)[VEC], const bool nt,
                                          const SrKey& sk, uint64_t rkey) {
  static_assert(!opt_rowwise(R), "a row-wise rule takes the whole row: apply_row_rowwise");
  if constexpr (opt_plain(R) && !is_bf16<WT>()) {
    // plain SGD on fp32 rows, the update the benchmark runs, keeps the body it always had: written with load_weights / rule_sgd / store_weights
    // its kernels compiled to other instructions
    if (VEC == 4 && nt) {
      emb_f4 w = __builtin_nontemporal_load(reinterpret_cast<const emb_f4*>(wrow) + c);
      w.x = __fmaf_rn(-o.lr, acc[0], w.x); w.y = __fmaf_rn(-o.lr, acc[1], w.y);
      w.z = __fmaf_rn(-o.lr, acc[2], w.z); w.w = __fmaf_rn(-o.lr, acc[3], w.w);
      __builtin_nontemporal_store(w, reinterpret_cast<emb_f4*>(wrow) + c);
    } else if (VEC == 4) {
      float4 w = reinterpret_cast<float4*>(wrow)[c];
      w.x = __fmaf_rn(-o.lr, acc[0], w.x); w.y = __fmaf_rn(-o.lr, acc[1], w.y);
      w.z = __fmaf_rn(-o.lr, acc[2], w.z); w.w = __fmaf_rn(-o.lr, acc[3], w.w);
      reinterpret_cast<float4*>(wrow)[c] = w;
    } else {
      wrow[c] = __fmaf_rn(-o.lr, acc[0], wrow[c]);
    }
    return;
  }
  const bool ntw = opt_plain(R) && nt;
  const bool has0 = R == RowRule::Adam || R == RowRule::Adagrad || (R == RowRule::Momentum && o.mom > 0.f);
  float wv[VEC], av[VEC], bv[VEC];
  load_weights<VEC, WT>(wv, wrow, c, ntw);
  if (has0) load_state<VEC>(av, s0row, c);
  if (R == RowRule::Adam) load_state<VEC>(bv, s1row, c);
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    if constexpr (R == RowRule::Sgd) rule_sgd(o, acc[k], wv[k]);
    else if constexpr (R == RowRule::Momentum) rule_momentum(o, acc[k], wv[k], av[k]);
    else if constexpr (R == RowRule::Adam) rule_adam(o, acc[k], wv[k], av[k], bv[k]);
    else rule_adagrad(o, acc[k], wv[k], av[k]);
  }
  store_weights<VEC, WT>(o, wrow, c, wv, sk, rkey, ntw);
  if (has0) store_state<VEC>(s0row, c, av);
  if (R == RowRule::Adam) store_state<VEC>(s1row, c, bv);
}

// Row-wise Adagrad on one complete row (include/ff_hip_rowwise.h, statement by statement), by the row's lane group: `lpr` consecutive lanes of one
// wave, this lane the c0-th of them; vector c = c0 + t * lpr of the row (VEC columns) is this lane's in trip t.  `sum_of(c, g)` gives the canonical
// gradient sum of vector c.  Gradient and weights of up to kMaxChunks trips stay in registers between the sum and the update (the entry points refuse
// wider rows for this rule), so no row is read twice.
// TREE: level k adds the subtrees whose column indices differ in bit k -- the VEC columns of a vector in the lane; then, per trip, a butterfly over
// the group's lane index c0 (the low bits of the vector index): each lane holds the sum of its aligned subtree of `s` lanes and reads the sibling
// subtree's from that subtree's first lane (every lane of a subtree holds the same value), nothing where the sibling lies wholly at or past lpr
// (padding: x + (+0) = x for the x >= +0 that occur); then the trips (the high bits of the vector index; only a group of 64 lanes makes several).
// A trip's butterfly is walked by all lanes of the group, a vector that does not exist (c >= nvec: the last trip of D / VEC not a multiple of 64)
// counting as +0.  A lane only ever reads lanes of its own group: they took the same branches to get here (sub-run / slot, `single` / `complete`
// and nvec are the group's), so they are active together whatever iteration the wave's other groups are in.  __shfl is ds_bpermute_b32: groups are
// neither a power of two wide (D = 48: 12 lanes) nor aligned to one, which rules out the DPP row operations; six dependent LDS-crossbar hops at most.
// S: loaded by every lane of the group (one address: a broadcast), stored by the group's first lane behind the loads in program order.
template <int VEC, class WT, class F>
__device__ __forceinline__ void apply_row_rowwise(const OptP& o, float* wrow, float* Sp, int D, int nvec, int lpr, int c0, int lane, F&& sum_of,
                                                  const SrKey& sk, uint64_t rkey) {
#pragma clang fp contract(off)
  const float S = *Sp;
  float gt[kMaxChunks][VEC], wv[kMaxChunks][VEC], part[kMaxChunks];
  uint2 w2[kMaxChunks];      // bf16 rows, 16-byte form: the packed words are what lives across the sum; wv[t] is widened from them again for the update
#pragma unroll
  for (int t = 0; t < kMaxChunks; t++) {
    part[t] = 0.f;
    if (t * 64 < nvec) {                  // (uniform over the wave; t > 0: nvec > 64, the group is the wave)
      const int c = c0 + t * lpr;
      float p = 0.f;
      if (c < nvec) {
        sum_of(c, gt[t]);
        if constexpr (VEC == 4 && is_bf16<WT>()) { w2[t] = reinterpret_cast<const uint2*>(wrow)[c]; widen_bf16x4(wv[t], w2[t]); }
        else load_weights<VEC, WT>(wv[t], wrow, c, false);
        float sq[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          if (o.wd != 0.f) { const float t0 = o.wd * wv[t][k]; gt[t][k] = gt[t][k] + t0; }
          sq[k] = gt[t][k] * gt[t][k];
        }
        if (VEC == 4) { const float lo = sq[0] + sq[1], hi = sq[2] + sq[3]; p = lo + hi; }
        else p = sq[0];
      }
      for (int s = 1; s < lpr; s <<= 1) {
        const int sib = (c0 & ~(s - 1)) ^ s;                      // first lane (of the group) of the sibling subtree
        const float other = __shfl(p, sib < lpr ? lane - c0 + sib : lane);
        if (sib < lpr) p = p + other;
      }
      part[t] = p;
    }
  }
  // the trips: absent ones are +0, and x + (+0) = x, so the one expression is TREE's for every number of trips
  const float sum01 = part[0] + part[1], sum23 = part[2] + part[3];
  const float sum = sum01 + sum23;
  const float ms = sum / (float)D;
  const float Sn = S + ms;
  const float den = sqrtf(Sn) + o.eps;
#pragma unroll
  for (int t = 0; t < kMaxChunks; t++) {
    const int c = c0 + t * lpr;
    if (t * 64 < nvec && c < nvec) {
      if constexpr (VEC == 4 && is_bf16<WT>()) widen_bf16x4(wv[t], w2[t]);      // widened again from the two packed words: exact, and half the registers across the sum
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const float q = gt[t][k] / den;
        const float t2 = o.lr * q;
        wv[t][k] = wv[t][k] - t2;
      }
      store_weights<VEC, WT>(o, wrow, c, wv[t], sk, rkey, false);
    }
  }
  if (c0 == 0) *Sp = Sn;
}
static_assert(kMaxChunks == 4, "apply_row_rowwise: the tree over the trips is written for four");

}  // namespace

}  // namespace ffh_emb
