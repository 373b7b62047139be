// Eccentricity bounding over the level matrix of a 64-source batch pass
// (gfx950, wave64; backend.hpp EccArgs; Takes and Kosters).
//
//   ecc_degrees  the owned rows' lengths (the first selection's key)
//   ecc_init     scope, bounds and state of every vertex
//   ecc_select   drop what the target no longer needs, then the next sources:
//                every workgroup's best keys into its slot, one workgroup
//                merges the slots (a launch of its own, as cc_sizes' finish:
//                the slots are read after the launch that wrote them ended)
//   ecc_update   a stream over the rows of the live vertices, 16 bytes per lane
//   ecc_totals   the scope's counts, max lo and min hi: slots, then one workgroup
//
// Integers only, no atomics on global memory, no workgroup reads what another
// wrote in the same launch.
#include <climits>

#include "kernel_common.hpp"

namespace dbfs {
namespace kern {
namespace {

constexpr int kEccBlock = 256;
constexpr int kEccWaves = kEccBlock / kWave;
constexpr int kEccGrid = 4096;  // workgroups at most of the streaming kernels (grid-stride loops)

__global__ __launch_bounds__(kEccBlock) void ecc_degrees_kernel(EccArgs a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEccBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kEccBlock + threadIdx.x; r < a.g.rows; r += stride) {
    const eid_t b = a.g.row_off[r], e = a.g.row_off[r + 1];
    DBFS_DCHECK(b >= 0 && b <= e && e <= a.g.nnz, 60, r);
    a.deg_own[r] = static_cast<uint32_t>(e - b);
  }
}

__global__ __launch_bounds__(kEccBlock) void ecc_init_kernel(EccArgs a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kEccBlock + threadIdx.x; v < a.g.n; v += stride) {
    const bool in = a.scope_all || a.comp[v] == a.label;
    const bool empty = a.deg[v] == 0u;
    a.lo[v] = in ? 0 : -1;
    a.hi[v] = in ? (empty ? 0 : INT_MAX) : -1;
    a.state[v] = in ? kEccScope | (empty ? kEccSettled : kEccLive) : 0u;
  }
}

// ---- selection ----------------------------------------------------------------

// (larger value first, the smaller id on a tie) as one ordered key; never 0
// for a live vertex: its degree, its hi and INT_MAX - lo are all >= 1.
__device__ __forceinline__ unsigned long long ecc_key(uint32_t value, vid_t id) {
  return (static_cast<unsigned long long>(value) << 32) | (0xFFFFFFFFu - id);
}
__device__ __forceinline__ vid_t ecc_key_id(unsigned long long key) {
  return 0xFFFFFFFFu - static_cast<uint32_t>(key);
}

// A workgroup's K largest keys so far, in LDS: best[] descending (0: empty),
// low = best[K - 1], the key a newcomer has to beat.
template <int K>
struct EccTop {
  unsigned long long best[K], next[K], stage[kEccBlock], low;
  unsigned staged;
};

template <int K>
__device__ __forceinline__ void ecc_top_clear(EccTop<K>& t) {
  for (int i = threadIdx.x; i < K; i += kEccBlock) t.best[i] = 0ull;
  if (threadIdx.x == 0) t.low = 0ull, t.staged = 0u;
  __syncthreads();
}

// Every thread of the workgroup offers one key (0: none); called by all
// kEccBlock threads together.  Keys above `low` are staged, and the K largest
// of best[] and the staged ones, each placed by its rank (the keys are
// distinct), are the new best[].  Once best[] is full most calls stage
// nothing and cost one barrier.
template <int K>
__device__ __forceinline__ void ecc_top_offer(EccTop<K>& t, unsigned long long key) {
  const bool cand = key > t.low;
  if (!__syncthreads_or(cand)) return;
  if (cand) t.stage[atomicAdd(&t.staged, 1u)] = key;
  for (int i = threadIdx.x; i < K; i += kEccBlock) t.next[i] = 0ull;
  __syncthreads();
  const int total = K + static_cast<int>(t.staged);
  DBFS_DCHECK(total <= K + kEccBlock, 61, total);
  for (int i = threadIdx.x; i < total; i += kEccBlock) {
    const unsigned long long x = i < K ? t.best[i] : t.stage[i - K];
    if (x == 0ull) continue;
    int rank = 0;
    for (int j = 0; j < total; ++j) rank += (j < K ? t.best[j] : t.stage[j - K]) > x ? 1 : 0;
    if (rank < K) t.next[rank] = x;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += kEccBlock) t.best[i] = t.next[i];
  if (threadIdx.x == 0) t.low = t.next[K - 1], t.staged = 0u;
  __syncthreads();
}

// Every workgroup writes its whole slot, live vertices found or not: the
// merge reads all of them.
__global__ __launch_bounds__(kEccBlock) void ecc_select_kernel(EccArgs a) {
  __shared__ EccTop<kEccSelHi> top_hi;
  __shared__ EccTop<kMsSources> top_lo;
  __shared__ unsigned long long s_live;
  if (threadIdx.x == 0) s_live = 0ull;  // (the clears below end in a barrier)
  ecc_top_clear(top_hi);
  ecc_top_clear(top_lo);
  const int64_t n = a.g.n;
  const int32_t max_lo = static_cast<int32_t>(a.totals[kEccMaxLo]), min_hi = static_cast<int32_t>(a.totals[kEccMinHi]);
  unsigned long long live = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEccBlock;
  // (the trip count is the workgroup's: every thread reaches every barrier)
  for (int64_t v0 = static_cast<int64_t>(blockIdx.x) * kEccBlock; v0 < n; v0 += stride) {
    const int64_t v = v0 + threadIdx.x;
    unsigned long long key_hi = 0ull, key_lo = 0ull;
    if (v < n) {
      const uint32_t st = a.state[v];
      if (st & kEccLive) {
        const int32_t lo = a.lo[v], hi = a.hi[v];
        const bool drop = (a.target == EccTarget::Diameter && hi <= max_lo) ||
                          (a.target == EccTarget::Radius && lo >= min_hi);
        if (drop) {
          a.state[v] = st & ~kEccLive;
        } else {
          ++live;
          if (a.first) {
            key_lo = ecc_key(a.deg[v], static_cast<vid_t>(v));
          } else {
            key_hi = ecc_key(static_cast<uint32_t>(hi), static_cast<vid_t>(v));
            key_lo = ecc_key(static_cast<uint32_t>(INT_MAX - lo), static_cast<vid_t>(v));
          }
        }
      }
    }
    ecc_top_offer(top_hi, key_hi);
    ecc_top_offer(top_lo, key_lo);
  }
  live = static_cast<unsigned long long>(wave_sum(static_cast<long long>(live)));
  if (lane_id() == 0) atomicAdd(&s_live, live);  // (LDS)
  __syncthreads();
  DBFS_DCHECK(blockIdx.x < static_cast<unsigned>(kEccSelGrid), 62, blockIdx.x);
  unsigned long long* slot = a.sel_slots + static_cast<int64_t>(blockIdx.x) * kEccSelSlot;
  for (int i = threadIdx.x; i < kEccSelHi; i += kEccBlock) slot[i] = top_hi.best[i];
  for (int i = threadIdx.x; i < kMsSources; i += kEccBlock) slot[kEccSelHi + i] = top_lo.best[i];
  if (threadIdx.x == 0) slot[kEccSelHi + kMsSources] = s_live;
}

// One workgroup: the kEccSelHi best hi keys of all slots, then the best lo (or
// degree) keys of the vertices not among them, kMsSources ids in all at most.
// A vertex of the second list is among its workgroup's kMsSources best by lo:
// whoever beats it there and is not chosen with it is one of the kEccSelHi.
__global__ __launch_bounds__(kEccBlock) void ecc_select_finish_kernel(EccArgs a, int nslots) {
  __shared__ EccTop<kEccSelHi> top_hi;
  __shared__ EccTop<kMsSources> top_lo;
  __shared__ unsigned long long s_live;
  if (threadIdx.x == 0) s_live = 0ull;  // (the clears below end in a barrier)
  ecc_top_clear(top_hi);
  ecc_top_clear(top_lo);
  for (int i0 = 0; i0 < nslots * kEccSelHi; i0 += kEccBlock) {
    const int i = i0 + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < nslots * kEccSelHi)
      key = a.sel_slots[static_cast<int64_t>(i / kEccSelHi) * kEccSelSlot + i % kEccSelHi];
    ecc_top_offer(top_hi, key);
  }
  for (int i0 = 0; i0 < nslots * kMsSources; i0 += kEccBlock) {
    const int i = i0 + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < nslots * kMsSources)
      key = a.sel_slots[static_cast<int64_t>(i / kMsSources) * kEccSelSlot + kEccSelHi + i % kMsSources];
    if (key != 0ull)
      for (int j = 0; j < kEccSelHi; ++j)
        if (top_hi.best[j] != 0ull && ecc_key_id(top_hi.best[j]) == ecc_key_id(key)) key = 0ull;
    ecc_top_offer(top_lo, key);
  }
  unsigned long long live = 0;
  for (int i = threadIdx.x; i < nslots; i += kEccBlock)
    live += a.sel_slots[static_cast<int64_t>(i) * kEccSelSlot + kEccSelHi + kMsSources];
  live = static_cast<unsigned long long>(wave_sum(static_cast<long long>(live)));
  if (lane_id() == 0) atomicAdd(&s_live, live);  // (LDS)
  __syncthreads();
  int n_hi = 0;
  for (int j = 0; j < kEccSelHi; ++j) n_hi += top_hi.best[j] != 0ull ? 1 : 0;
  const int t = threadIdx.x;
  if (t < kMsSources) {
    const unsigned long long key = t < n_hi ? top_hi.best[t] : top_lo.best[t - n_hi];
    const bool have = key != 0ull;
    const vid_t id = ecc_key_id(key);
    DBFS_DCHECK(!have || (static_cast<int64_t>(id) < a.g.n && (a.state[id] & kEccLive)), 63, id);
    a.sel_out[1 + t] = have && static_cast<int64_t>(id) < a.g.n ? static_cast<int64_t>(id) : -1;
    // (both lists descend: the chosen ones are a prefix)
    const unsigned long long mask = __ballot(have);
    if (t == 0) {
      a.sel_out[0] = __popcll(mask);
      a.sel_out[1 + kMsSources] = static_cast<int64_t>(s_live);
    }
  }
}

// ---- update -------------------------------------------------------------------

// Row v of the matrix is kMsSources levels of type L: kLanes lanes take 16
// bytes of it each, fold their sources' bounds in registers and combine them
// across the kLanes neighbouring lanes with shuffles.  A lane group shares v
// and so its state: the row of a vertex that is not live is never loaded.
template <class L>
__global__ __launch_bounds__(kEccBlock) void ecc_update_kernel(EccArgs a) {
  constexpr int kPer = 16 / static_cast<int>(sizeof(L));  // levels per 16-byte load
  constexpr int kLanes = kMsSources / kPer;               // lanes per row: 4 or 8
  constexpr int kRows = kEccBlock / kLanes;               // rows per workgroup and step
  constexpr int kBits = 8 * static_cast<int>(sizeof(L));
  constexpr uint32_t kNone = static_cast<uint32_t>(ms_unreached<L>());
  __shared__ int32_t s_ecc[kMsSources];
  if (threadIdx.x < kMsSources) s_ecc[threadIdx.x] = static_cast<int>(threadIdx.x) < a.m.k ? a.ecc[threadIdx.x] : -1;
  __syncthreads();
  const int64_t n = a.g.n;
  const int sub = threadIdx.x % kLanes;
  const unsigned char* const lvl = static_cast<const unsigned char*>(a.m.lvl);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRows;
  for (int64_t v0 = static_cast<int64_t>(blockIdx.x) * kRows; v0 < n; v0 += stride) {
    const int64_t v = v0 + threadIdx.x / kLanes;
    uint32_t st = 0u;
    if (v < n) st = a.state[v];
    const bool live = (st & kEccLive) != 0u;
    int32_t lo = 0, hi = INT_MAX;
    if (live) {
      DBFS_DCHECK(v < a.m.lvl_rows, 64, v);
      lo = a.lo[v];
      hi = a.hi[v];
      const uint4 q = *reinterpret_cast<const uint4*>(lvl + (static_cast<size_t>(v) * kMsSources + sub * kPer) * sizeof(L));
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const uint32_t d = (w[j * kBits / 32] >> (j * kBits % 32)) & kNone;
        const int32_t e = s_ecc[sub * kPer + j];
        if (d == kNone || e < 0) continue;
        DBFS_DCHECK(static_cast<int32_t>(d) <= e, 65, v);
        lo = max(lo, max(static_cast<int32_t>(d), e - static_cast<int32_t>(d)));
        hi = min(hi, e + static_cast<int32_t>(d));
      }
    }
    // (every lane of the wave takes part: a group that is not live carries the neutral bounds)
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
      lo = max(lo, __shfl_xor(lo, off, kWave));
      hi = min(hi, __shfl_xor(hi, off, kWave));
    }
    if (live && sub == 0) {
      DBFS_DCHECK(lo <= hi, 66, v);
      a.lo[v] = lo;
      a.hi[v] = hi;
      if (lo >= hi) a.state[v] = (st & ~kEccLive) | kEccSettled;
    }
  }
}

// ---- totals -------------------------------------------------------------------

struct EccSums {
  long long scope = 0, settled = 0, live = 0, at_hi = 0, at_lo = 0;
  int32_t max_lo = -1, min_hi = INT_MAX;
};

__device__ __forceinline__ int32_t wave_max_i32(int32_t x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x = max(x, __shfl_xor(x, off, kWave));
  return x;
}
__device__ __forceinline__ int32_t wave_min_i32(int32_t x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, kWave));
  return x;
}

// A workgroup's sums reduced into `out` (kEccTotals entries).
__device__ __forceinline__ void ecc_block_totals(EccSums t, int64_t* out) {
  __shared__ long long s_sum[kEccWaves][5];
  __shared__ int32_t s_max[kEccWaves], s_min[kEccWaves];
  t.scope = wave_sum(t.scope);
  t.settled = wave_sum(t.settled);
  t.live = wave_sum(t.live);
  t.at_hi = wave_sum(t.at_hi);
  t.at_lo = wave_sum(t.at_lo);
  t.max_lo = wave_max_i32(t.max_lo);
  t.min_hi = wave_min_i32(t.min_hi);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) {
    s_sum[wave][0] = t.scope, s_sum[wave][1] = t.settled, s_sum[wave][2] = t.live;
    s_sum[wave][3] = t.at_hi, s_sum[wave][4] = t.at_lo;
    s_max[wave] = t.max_lo, s_min[wave] = t.min_hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kEccWaves; ++w) {
      t.scope += s_sum[w][0], t.settled += s_sum[w][1], t.live += s_sum[w][2];
      t.at_hi += s_sum[w][3], t.at_lo += s_sum[w][4];
      t.max_lo = max(t.max_lo, s_max[w]), t.min_hi = min(t.min_hi, s_min[w]);
    }
    out[kEccScopeSize] = t.scope;
    out[kEccSettledN] = t.settled;
    out[kEccLiveN] = t.live;
    out[kEccMaxLo] = t.max_lo;
    out[kEccMinHi] = t.min_hi;
    out[kEccAtHi] = t.at_hi;
    out[kEccAtLo] = t.at_lo;
  }
}

__global__ __launch_bounds__(kEccBlock) void ecc_totals_kernel(EccArgs a) {
  EccSums t;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kEccBlock + threadIdx.x; v < a.g.n; v += stride) {
    const uint32_t st = a.state[v];
    if (!(st & kEccScope)) continue;
    const int32_t lo = a.lo[v], hi = a.hi[v];
    ++t.scope;
    t.live += (st & kEccLive) ? 1 : 0;
    if (st & kEccSettled) {
      ++t.settled;
      t.at_hi += lo == a.count_hi ? 1 : 0;
      t.at_lo += lo == a.count_lo ? 1 : 0;
    }
    t.max_lo = max(t.max_lo, lo);
    t.min_hi = min(t.min_hi, hi);
  }
  DBFS_DCHECK(blockIdx.x < static_cast<unsigned>(kEccTotalsGrid), 67, blockIdx.x);
  ecc_block_totals(t, a.slots + static_cast<int64_t>(blockIdx.x) * kEccTotals);
}

__global__ __launch_bounds__(kEccBlock) void ecc_totals_finish_kernel(EccArgs a, int nslots) {
  EccSums t;
  for (int i = threadIdx.x; i < nslots; i += kEccBlock) {
    const int64_t* s = a.slots + static_cast<int64_t>(i) * kEccTotals;
    t.scope += s[kEccScopeSize];
    t.settled += s[kEccSettledN];
    t.live += s[kEccLiveN];
    t.at_hi += s[kEccAtHi];
    t.at_lo += s[kEccAtLo];
    t.max_lo = max(t.max_lo, static_cast<int32_t>(s[kEccMaxLo]));
    t.min_hi = min(t.min_hi, static_cast<int32_t>(s[kEccMinHi]));
  }
  ecc_block_totals(t, a.totals);
}

}  // namespace

void ecc_degrees(const EccArgs& a, hipStream_t st) {
  if (a.g.rows <= 0) return;
  ecc_degrees_kernel<<<grid_for(a.g.rows, kEccBlock, kEccGrid), kEccBlock, 0, st>>>(a);
}

void ecc_init(const EccArgs& a, hipStream_t st) {
  if (a.g.n <= 0) return;
  DBFS_CHECK(a.scope_all || a.comp, "ecc_init: a component scope needs the labels");
  ecc_init_kernel<<<grid_for(a.g.n, kEccBlock, kEccGrid), kEccBlock, 0, st>>>(a);
}

void ecc_select(const EccArgs& a, hipStream_t st) {
  if (a.g.n <= 0) {
    (void)hipMemsetAsync(a.sel_out, 0, kEccSelOut * sizeof(int64_t), st);
    return;
  }
  const unsigned slots = grid_for(a.g.n, kEccBlock, kEccSelGrid);
  ecc_select_kernel<<<slots, kEccBlock, 0, st>>>(a);
  ecc_select_finish_kernel<<<1, kEccBlock, 0, st>>>(a, static_cast<int>(slots));
}

void ecc_update(const EccArgs& a, hipStream_t st) {
  if (a.g.n <= 0 || a.m.k <= 0) return;
  DBFS_CHECK(a.m.lvl && a.m.lvl_rows >= a.g.n, "ecc_update: the level matrix is shorter than the graph");
  DBFS_CHECK(a.m.k <= kMsSources, "ecc_update: more sources than a pass holds");
  ms_level_type(a.m.lvl_bytes, [&](auto l) {
    using L = decltype(l);
    constexpr int rows = kEccBlock / (kMsSources * static_cast<int>(sizeof(L)) / 16);
    ecc_update_kernel<L><<<grid_for(a.g.n, rows, kEccGrid), kEccBlock, 0, st>>>(a);
  });
}

void ecc_totals(const EccArgs& a, hipStream_t st) {
  static_assert(kEccTotalsGrid <= kEccGrid, "a slot per workgroup");
  const unsigned slots = grid_for(a.g.n, kEccBlock, kEccTotalsGrid);
  ecc_totals_kernel<<<slots, kEccBlock, 0, st>>>(a);
  ecc_totals_finish_kernel<<<1, kEccBlock, 0, st>>>(a, static_cast<int>(slots));
}

unsigned long long take_check_ecc() { return take_check_local(); }
void inject_check_ecc(hipStream_t st) { inject_check_local(st); }
const bool kCheckedEcc = kCheckedLocal;

}  // namespace kern
}  // namespace dbfs
