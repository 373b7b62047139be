// Connected components: a hook-and-compress forest over the adjacency shard
// (gfx950, wave64; backend.hpp CcArgs; Afforest / ECL-CC style).
//
//   cc_init        comp[v] = v
//   cc_link        one pass over the owned rows' entries [first, first + count):
//                  hook both ends' trees together (cc_hook)
//   cc_link_pairs  hook (v, other[v]): the several-rank merge
//   cc_compress    full pointer jumping: comp[v] = v's root
//   cc_sample      a few labels gathered for the host
//   cc_sizes       size[label] and the totals
//
// comp[v] <= v at all times, a hook only ever hangs a root under a smaller id
// and a find only points a vertex at one of its ancestors, so a tree's root
// is its smallest vertex and the compressed labels do not
// depend on the order in which the hooks ran: one pass over every entry plus
// one compress is complete, with no outer "until nothing changes" loop.
//
// Row tiers of cc_link, as ms_push has them: a range of up to kCcLane entries
// is walked by its lane, up to kCcWave by its wave (64 coalesced column ids
// per step), a longer one is queued and walked by the whole grid in a second
// launch (an RMAT hub's row on one lane: the 5-7x ms_push measured).
#include "kernel_common.hpp"

namespace dbfs {
namespace kern {
namespace {

constexpr int kCcBlock = 256;
constexpr int kCcGrid = 4096;      // workgroups at most (grid-stride loops)
constexpr int kCcLongGrid = 512;   // ... of the long rows' launch
constexpr int kCcLane = 32;
constexpr int kCcWave = 1024;

__device__ __forceinline__ vid_t cc_load(const vid_t* p) {
  return __hip_atomic_load(const_cast<vid_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void cc_store(vid_t* p, vid_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of v's tree as far as this lane can tell, halving the path on the
// way (ECL-CC's intermediate pointer jumping): a vertex found with a parent
// is pointed at its grandparent.  Only vertices that already have a parent
// are written, with one of their ancestors, so comp[x] <= x stays and no such
// store meets a compare-and-swap (those succeed on roots only, and a vertex
// with a parent never becomes a root again).  `cur` falls strictly: bounded.
__device__ __forceinline__ vid_t cc_find(vid_t* comp, vid_t v) {
  vid_t cur = cc_load(comp + v);
  if (cur == v) return v;
  vid_t prev = v, next;
  while ((next = cc_load(comp + cur)) < cur) {
    cc_store(comp + prev, next);
    prev = cur;
    cur = next;
  }
  return cur;
}

// Join the trees of u and w: find both roots, then hang the larger under the
// smaller id.
// Loop safety: every value the loops decide on is either what the
// compare-and-swap returned or an agent-scope relaxed load (served by the L2,
// never by this CU's L1, which no other CU's store refreshes).  Every value
// ever stored in comp[x] is <= x, and == x only while x is a root.  A failed
// swap returns comp[hi] != hi, so a value < hi, and the retry goes on from
// (that value, lo): max(p1, p2) falls strictly with every retry, and so does
// cc_find's cursor.  Both loops end after at most min(depth, n) steps whatever
// the other lanes do, stale values included (a stale comp[x] is an older one:
// x itself or another ancestor of x), and no step waits for another lane's
// store.
__device__ __forceinline__ void cc_hook(vid_t* comp, vid_t u, vid_t w, int64_t n) {
  DBFS_DCHECK(static_cast<int64_t>(w) < n, 40, w);
  vid_t p1 = cc_find(comp, u), p2 = cc_find(comp, w);
  [[maybe_unused]] int64_t steps = 0;
  while (p1 != p2) {
    const vid_t hi = max(p1, p2), lo = min(p1, p2);
    const vid_t old = atomicCAS(comp + hi, hi, lo);
    if (old == hi) break;  // hi was a root and hangs under lo now
    p1 = old;              // (hi has a parent: on from there)
    p2 = lo;
#ifdef DBFS_CHECKED
    if (++steps > n) {
      DBFS_DCHECK(false, 41, u);
      break;
    }
#endif
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(vid_t* comp, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kCcBlock + threadIdx.x; v < n; v += stride)
    comp[v] = static_cast<vid_t>(v);
}

// The entries of row r this launch walks: [first, first + count) of the row.
__device__ __forceinline__ void cc_row_range(const CcArgs& a, int64_t r, eid_t& rs, eid_t& re) {
  const eid_t b = a.g.row_off[r], e = a.g.row_off[r + 1];
  DBFS_DCHECK(b >= 0 && b <= e && e <= a.g.nnz, 29, r);
  rs = min(e, b + a.first);
  re = a.count < 0 ? e : min(e, rs + a.count);
}

__global__ __launch_bounds__(kCcBlock) void cc_link_kernel(CcArgs a) {
  const ShardView& g = a.g;
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kCcBlock + (threadIdx.x & ~(kWave - 1)); r0 < g.rows;
       r0 += stride) {
    const int64_t r = r0 + lane;
    const vid_t u = static_cast<vid_t>(g.lo + r);
    eid_t rs = 0, re = 0;
    if (r < g.rows) {
      cc_row_range(a, r, rs, re);
      // (an undirected shard stores an edge in both rows: one that leaves the
      // skipped component is taken from its other end)
      if (a.skip && rs < re && cc_load(a.comp + u) == a.skip_label) re = rs;
    }
    const bool huge = re - rs > kCcWave;
    const bool wide = re - rs > kCcLane && !huge;
    const eid_t lane_end = wide || huge ? rs : re;
    const unsigned long long hm = __ballot(huge);
    if (hm) {
      const int leader = __ffsll(static_cast<long long>(hm)) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(a.long_count, static_cast<unsigned long long>(__popcll(hm)));
      base = readlane64(base, leader);
      const unsigned long long at = base + mask_rank(hm);
      // (ranges this long are at most nnz / kCcWave: the queue's capacity)
      DBFS_DCHECK(!huge || at < static_cast<unsigned long long>(a.long_cap), 42, at);
      if (huge && at < static_cast<unsigned long long>(a.long_cap)) a.long_rows[at] = static_cast<vid_t>(r);
    }
    for (eid_t e = rs; e < lane_end; ++e) cc_hook(a.comp, u, g.col[e], g.n);
    unsigned long long lm = __ballot(wide);
    while (lm) {
      const int l = __ffsll(static_cast<long long>(lm)) - 1;
      lm &= lm - 1;
      const eid_t b = readlane_i64(rs, l), en = readlane_i64(re, l);
      const vid_t ul = static_cast<vid_t>(g.lo + r0 + l);
      for (eid_t e = b + lane; e < en; e += kWave) cc_hook(a.comp, ul, g.col[e], g.n);
    }
  }
}

// The rows cc_link_kernel queued: every workgroup walks its share of every
// queued row, 256 entries per step and workgroup.
__global__ __launch_bounds__(kCcBlock) void cc_link_long_kernel(CcArgs a) {
  const ShardView& g = a.g;
  const int64_t nq = min(static_cast<int64_t>(__hip_atomic_load(a.long_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)),
                         a.long_cap);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t r = a.long_rows[q];
    DBFS_DCHECK(r < g.rows, 43, r);
    eid_t rs, re;
    cc_row_range(a, r, rs, re);
    const vid_t u = static_cast<vid_t>(g.lo + r);
    // (row q's chunks start at another workgroup for every q, as ms_push_long_kernel's)
    const int64_t first = static_cast<int64_t>((blockIdx.x + gridDim.x - static_cast<unsigned>((q * 37) % gridDim.x)) % gridDim.x);
    for (eid_t e = rs + first * kCcBlock + threadIdx.x; e < re; e += stride) cc_hook(a.comp, u, g.col[e], g.n);
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_link_pairs_kernel(CcArgs a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCcBlock + threadIdx.x; i < a.pairs; i += stride)
    cc_hook(a.comp, static_cast<vid_t>(a.pair_lo + i), a.other[i], a.g.n);
}

// Runs after the link launches have ended, so plain loads are fine: no pointer
// moves but to an ancestor here, a root stays a root, and whatever ancestor a
// load returns the climb ends at the root.  Concurrent writes are monotone.
__global__ __launch_bounds__(kCcBlock) void cc_compress_kernel(vid_t* comp, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kCcBlock + threadIdx.x; v < n; v += stride) {
    vid_t p = comp[v];
    [[maybe_unused]] int64_t steps = 0;
    for (vid_t pp = comp[p]; pp != p; pp = comp[p]) {
      p = pp;
#ifdef DBFS_CHECKED
      if (++steps > n) {
        DBFS_DCHECK(false, 44, v);
        break;
      }
#endif
    }
    comp[v] = p;
  }
}

__global__ void cc_sample_kernel(CcArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.samples) {
    DBFS_DCHECK(static_cast<int64_t>(a.sample_idx[i]) < a.g.n, 45, i);
    a.sample_out[i] = a.comp[a.sample_idx[i]];
  }
}

// size[label] += 1 per vertex, aggregated in the wave first: the wave loops
// over its distinct labels (the first pending lane's label, the ballot of the
// lanes that share it, one atomic with the popcount), so a wave of 64 vertices
// of the giant component costs one atomic, not 64 on one address.
__global__ __launch_bounds__(kCcBlock) void cc_hist_kernel(CcArgs a) {
  const int lane = lane_id();
  const int64_t n = a.g.n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t v0 = static_cast<int64_t>(blockIdx.x) * kCcBlock + (threadIdx.x & ~(kWave - 1)); v0 < n; v0 += stride) {
    const bool in = v0 + lane < n;
    const vid_t label = in ? a.comp[v0 + lane] : 0u;
    DBFS_DCHECK(!in || static_cast<int64_t>(label) <= v0 + lane, 46, v0 + lane);
    unsigned long long left = __ballot(in);
    while (left) {
      const int leader = __ffsll(static_cast<long long>(left)) - 1;
      const vid_t l = static_cast<vid_t>(__builtin_amdgcn_readlane(static_cast<int>(label), leader));
      const unsigned long long same = __ballot(in && label == l);
      if (lane == leader) atomicAdd(a.size + l, static_cast<uint32_t>(__popcll(same)));
      left &= ~same;
    }
  }
}

// (largest size, smaller label on a tie) as one ordered key
__device__ __forceinline__ unsigned long long cc_key(uint32_t size, vid_t label) {
  return (static_cast<unsigned long long>(size) << 32) | (0xFFFFFFFFu - label);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long y = static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(x), off, kWave));
    x = y > x ? y : x;
  }
  return x;
}

// A workgroup's (roots, roots of size 1, best key) reduced into slot `out`.
__device__ __forceinline__ void cc_block_totals(long long roots, long long single, unsigned long long key,
                                                int64_t* out) {
  __shared__ long long s_r[kCcBlock / kWave], s_s[kCcBlock / kWave];
  __shared__ unsigned long long s_k[kCcBlock / kWave];
  roots = wave_sum(roots);
  single = wave_sum(single);
  key = wave_max_u64(key);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_r[wave] = roots, s_s[wave] = single, s_k[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCcBlock / kWave; ++w) {
      roots += s_r[w];
      single += s_s[w];
      key = s_k[w] > key ? s_k[w] : key;
    }
    out[0] = roots;
    out[1] = single;
    out[2] = static_cast<int64_t>(key >> 32);
    out[3] = static_cast<int64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key));
  }
}

// Per-workgroup partial totals into the workgroup's slot ...
__global__ __launch_bounds__(kCcBlock) void cc_totals_kernel(CcArgs a) {
  const int64_t n = a.g.n;
  long long roots = 0, single = 0;
  unsigned long long key = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCcBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kCcBlock + threadIdx.x; v < n; v += stride) {
    if (a.comp[v] != static_cast<vid_t>(v)) continue;
    const uint32_t s = a.size[v];
    ++roots;
    single += s == 1u ? 1 : 0;
    const unsigned long long k = cc_key(s, static_cast<vid_t>(v));
    key = k > key ? k : key;
  }
  cc_block_totals(roots, single, key, a.slots + static_cast<int64_t>(blockIdx.x) * kCcTotals);
}

// ... and the slots into the totals, one workgroup (a launch of its own: the
// slots are read after the launch that wrote them has ended).
__global__ __launch_bounds__(kCcBlock) void cc_totals_finish_kernel(CcArgs a, int nslots) {
  long long roots = 0, single = 0;
  unsigned long long key = 0;
  for (int i = threadIdx.x; i < nslots; i += kCcBlock) {
    const int64_t* s = a.slots + static_cast<int64_t>(i) * kCcTotals;
    roots += s[0];
    single += s[1];
    // (an empty slot's key is (0, label 0): below every real one, sizes are >= 1)
    const unsigned long long k = cc_key(static_cast<uint32_t>(s[2]), static_cast<vid_t>(s[3]));
    key = s[2] > 0 && k > key ? k : key;
  }
  cc_block_totals(roots, single, key, a.totals);
}

}  // namespace

void cc_init(const CcArgs& a, hipStream_t st) {
  if (a.g.n <= 0) return;
  cc_init_kernel<<<grid_for(a.g.n, kCcBlock, kCcGrid), kCcBlock, 0, st>>>(a.comp, a.g.n);
}

void cc_link(const CcArgs& a, hipStream_t st) {
  if (a.g.rows <= 0 || a.g.nnz <= 0) return;
  DBFS_CHECK(a.long_rows && a.long_count && a.long_cap >= a.g.nnz / kCcWave + 1, "cc_link: long-row queue too small");
  DBFS_CHECK(a.first >= 0, "cc_link: negative first entry");
  (void)hipMemsetAsync(a.long_count, 0, sizeof(unsigned long long), st);
  cc_link_kernel<<<grid_for(a.g.rows, kCcBlock, kCcGrid), kCcBlock, 0, st>>>(a);
  // (no range of a launch that takes at most kCcWave entries per row is queued)
  if (a.count < 0 || a.count > kCcWave) cc_link_long_kernel<<<kCcLongGrid, kCcBlock, 0, st>>>(a);
}

void cc_link_pairs(const CcArgs& a, hipStream_t st) {
  if (a.pairs <= 0) return;
  DBFS_CHECK(a.pair_lo >= 0 && a.pair_lo + a.pairs <= a.g.n, "cc_link_pairs: pairs outside the graph");
  cc_link_pairs_kernel<<<grid_for(a.pairs, kCcBlock, kCcGrid), kCcBlock, 0, st>>>(a);
}

void cc_compress(const CcArgs& a, hipStream_t st) {
  if (a.g.n <= 0) return;
  cc_compress_kernel<<<grid_for(a.g.n, kCcBlock, kCcGrid), kCcBlock, 0, st>>>(a.comp, a.g.n);
}

void cc_sample(const CcArgs& a, hipStream_t st) {
  if (a.samples <= 0) return;
  cc_sample_kernel<<<grid_for(a.samples, kCcBlock), kCcBlock, 0, st>>>(a);
}

void cc_sizes(const CcArgs& a, hipStream_t st) {
  static_assert(kCcSizeGrid <= kCcGrid, "a slot per workgroup");
  if (a.g.n <= 0) {
    (void)hipMemsetAsync(a.totals, 0, kCcTotals * sizeof(int64_t), st);
    return;
  }
  (void)hipMemsetAsync(a.size, 0, static_cast<size_t>(a.g.n) * sizeof(uint32_t), st);
  cc_hist_kernel<<<grid_for(a.g.n, kCcBlock, kCcGrid), kCcBlock, 0, st>>>(a);
  const unsigned slots = grid_for(a.g.n, kCcBlock, kCcSizeGrid);
  cc_totals_kernel<<<slots, kCcBlock, 0, st>>>(a);
  cc_totals_finish_kernel<<<1, kCcBlock, 0, st>>>(a, static_cast<int>(slots));
}

unsigned long long take_check_cc() { return take_check_local(); }
void inject_check_cc(hipStream_t st) { inject_check_local(st); }
const bool kCheckedCc = kCheckedLocal;

}  // namespace kern
}  // namespace dbfs
