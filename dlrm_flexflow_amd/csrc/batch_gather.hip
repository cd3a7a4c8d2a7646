// batch_gather.hip -- include/ff_hip_data.h: one training batch of the device-resident data set, in shuffled order, in one launch.
//
// The batch is 8.7 MB at the Terabyte shape (32768 x (26 x 8 + 52 + 4) bytes) and its source rows are scattered 8-byte ids: a
// latency-bound gather.  A workgroup takes kSlots consecutive slots of the batch.  One wave's worth of lanes maps each slot through
// ffh_perm_index ONCE (the walk of include/ffh_perm.h is a few hundred integer instructions per step) and leaves the source rows in
// LDS; then every wave takes whole segments (its segment index is wave-uniform, so a segment's descriptor is a scalar load from the
// kernel arguments) and its lanes move that segment's kSlots rows, one unit of 16, 8 or 4 bytes per lane and trip.  Consecutive
// lanes write consecutive destination units (the destination rows of a workgroup are contiguous), so the stores coalesce; the loads are
// as scattered as the order makes them.
#include "ffh_common.h"

#include "../../include/ff_hip_data.h"

namespace {

constexpr int kSlots = kWave;          // slots per workgroup
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

struct GatherArgs {
  ffh_batch_order    o;
  int                nseg;
  ffh_gather_segment seg[FFH_GATHER_MAX_SEGMENTS];
};

// rows [0, ns) of one segment (for one destination stripe): dst row drow0 + slot <- src row srow[slot] + sadd
template <typename U>
__device__ __forceinline__ void move_rows(const char* __restrict__ src, char* __restrict__ dst, const int64_t* srow, int64_t sadd,
                                          int64_t drow0, int row_bytes, int ns, int lane) {
  const int upr = row_bytes / (int)sizeof(U);            // units per row
  U* d = reinterpret_cast<U*>(dst + drow0 * row_bytes);  // ns * upr contiguous units
  for (int j = lane; j < ns * upr; j += kWave) {
    const int slot = upr == 1 ? j : j / upr;
    const int k = j - slot * upr;
    d[j] = *reinterpret_cast<const U*>(src + (srow[slot] + sadd) * (int64_t)row_bytes + (int64_t)k * (int64_t)sizeof(U));
  }
}

__global__ __launch_bounds__(kThreads) void batch_gather_kernel(const GatherArgs a) {
  ffh_kernel_prio();
  __shared__ int64_t local_row[kSlots];    // p: the stripe row of a slot
  __shared__ int64_t global_row[kSlots];   // ffh_perm_global_sample(p, Bl, world, 0); rank r adds r * Bl
  const int64_t Bl = a.o.local_batch;
  const int64_t i0 = (int64_t)blockIdx.x * kSlots;
  const int ns = (int)(Bl - i0 < kSlots ? Bl - i0 : kSlots);
  const int tid = (int)threadIdx.x;
  if (tid < ns) {
    const int64_t p = (int64_t)ffh_perm_index(a.o.seed, (uint64_t)a.o.epoch, (uint64_t)(a.o.step * Bl + i0 + tid), (uint64_t)a.o.n_local);
    local_row[tid] = p;
    global_row[tid] = ffh_perm_global_sample(p, Bl, a.o.world, 0);
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave;
  for (int s = wave; s < a.nseg; s += kWaves) {
    const ffh_gather_segment g = a.seg[s];
    if (!g.dst) continue;
    const bool global = g.kind == FFH_GATHER_GLOBAL_ROWS;
    const int64_t* srow = global ? global_row : local_row;
    const int stripes = global ? a.o.world : 1;
    const uintptr_t align = (uintptr_t)g.src | (uintptr_t)g.dst | (uintptr_t)g.row_bytes;
    for (int r = 0; r < stripes; r++) {
      const int64_t sadd = (int64_t)r * Bl, drow0 = (int64_t)r * Bl + i0;
      if (align % 16 == 0) move_rows<uint4>((const char*)g.src, (char*)g.dst, srow, sadd, drow0, g.row_bytes, ns, lane);
      else if (align % 8 == 0) move_rows<uint2>((const char*)g.src, (char*)g.dst, srow, sadd, drow0, g.row_bytes, ns, lane);
      else move_rows<uint32_t>((const char*)g.src, (char*)g.dst, srow, sadd, drow0, g.row_bytes, ns, lane);
    }
  }
}

}  // namespace

extern "C" {

int ffh_data_abi_version(void) { return FFH_DATA_ABI_VERSION; }

int ffh_batch_gather(ffh_ctx* c, const ffh_gather_segment* segments, int nsegments, const ffh_batch_order* o, ffh_stream s) {
  FFH_REQUIRE(c, o != nullptr && nsegments >= 0 && (segments != nullptr || nsegments == 0), "batch_gather: null order or segments");
  FFH_REQUIRE(c, o->world >= 1 && o->rank >= 0 && o->rank < o->world, "batch_gather: rank outside [0, world)");
  FFH_REQUIRE(c, o->local_batch >= 1 && o->n_local >= o->local_batch && o->n_local % o->local_batch == 0,
              "batch_gather: n_local must be a positive multiple of local_batch");
  FFH_REQUIRE(c, o->epoch >= 0 && o->step >= 0 && o->step < o->n_local / o->local_batch, "batch_gather: step outside the epoch");
  FFH_REQUIRE(c, o->local_batch <= (int64_t)0x7fffffff * kSlots, "batch_gather: local_batch too large for one grid");
  for (int i = 0; i < nsegments; i++) {
    const ffh_gather_segment& g = segments[i];
    if (!g.dst) continue;
    FFH_REQUIRE(c, g.src != nullptr, "batch_gather: segment with a destination but no source");
    FFH_REQUIRE(c, g.kind == FFH_GATHER_LOCAL_ROWS || g.kind == FFH_GATHER_GLOBAL_ROWS, "batch_gather: unknown segment kind");
    FFH_REQUIRE(c, g.row_bytes > 0 && (((uintptr_t)g.src | (uintptr_t)g.dst | (uintptr_t)g.row_bytes) & 3) == 0,
                "batch_gather: row_bytes must be a positive multiple of 4 and both bases 4-byte aligned");
  }
  GatherArgs a;
  memset(&a, 0, sizeof a);
  a.o = *o;
  const unsigned grid = (unsigned)((o->local_batch + kSlots - 1) / kSlots);
  for (int first = 0; first < nsegments; first += FFH_GATHER_MAX_SEGMENTS) {
    a.nseg = nsegments - first < FFH_GATHER_MAX_SEGMENTS ? nsegments - first : FFH_GATHER_MAX_SEGMENTS;
    memcpy(a.seg, segments + first, (size_t)a.nseg * sizeof(ffh_gather_segment));
    hipLaunchKernelGGL(batch_gather_kernel, dim3(grid), dim3(kThreads), 0, as_stream(s), a);
    FFH_LAUNCH_CHECK(c, "batch_gather");
  }
  return FFH_OK;
}

}  // extern "C"
