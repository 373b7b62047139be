// Strongly connected components: trim, forward colouring and backward closure
// over the out-rows and the in-edge rows (gfx950, wave64; backend.hpp SccArgs;
// the colouring scheme of Orzan / Slota et al.'s Multistep, in pull form).
//
//   scc_init         scc = cls = colour = none
//   scc_trim         a live vertex without a counting out- or in-edge settles alone
//   scc_pivot        the live vertex with the largest in-degree x out-degree
//   scc_colour_init  colour[v] = v (or only the pivot's)
//   scc_forward      colour[v] = min over counting in-neighbours, one sweep (the
//                    pivot round: the pivot's colour from the first that has it)
//   scc_backward     v joins its colour's root through an out-neighbour that is in
//   scc_end_round    the coloured leftovers become the class of their colour
//   scc_relabel      the pivot's component gets its smallest id
//
// Every sweep kernel writes only the entry of its own vertex and reads the
// entries of its neighbours; no kernel waits for another lane or workgroup,
// and every device loop is a bounded row walk.  "Until nothing changes" is the
// host's loop over the changed counter.  A value another workgroup may store
// during the same launch (scc in trim and backward, colour in forward) is read
// with a relaxed agent-scope load and stored with a relaxed agent-scope store,
// as cc_kernels.hip's comp is: served by the L2, never by this CU's L1, which
// no other CU's store refreshes.  A stale value is only an older one (a vertex
// still live, a colour not yet fallen): the sweep then changes less, never
// something wrong, and a sweep that changes nothing has read only values from
// before its launch, which a kernel boundary makes visible -- so the host's
// fixed point is the real one.
//
// Row tiers, as cc_link has them: a row of up to kSccLane entries is walked by
// its lane, a longer one by its wave (64 coalesced column ids per step, a
// ballot for the early exit).  The walks that stop at the first hit (all but
// the general colouring's minimum) give a long row's first kSccLane entries to
// its lane first: directed RMAT-22's trim took 3.2 ms handing one long row after
// the other to the wave, 0.53 ms so.  No row is handed
// to the whole grid.
#include "kernel_common.hpp"

namespace dbfs {
namespace kern {
namespace {

constexpr int kSccBlock = 256;
constexpr int kSccGrid = 2048;  // workgroups at most (grid-stride loops)
constexpr int kSccLane = 32;

__device__ __forceinline__ vid_t scc_load(const vid_t* p) {
  return __hip_atomic_load(const_cast<vid_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void scc_store(vid_t* p, vid_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Row r of g, checked.
__device__ __forceinline__ void scc_row(const ShardView& g, int64_t r, eid_t& b, eid_t& e) {
  b = g.row_off[r];
  e = g.row_off[r + 1];
  DBFS_DCHECK(b >= 0 && b <= e && e <= g.nnz, 50, r);
  // (a row the check refuses is not walked)
  if (!(b >= 0 && b <= e && e <= g.nnz)) b = e = 0;
}

__device__ __forceinline__ vid_t scc_entry(const ShardView& g, eid_t i) {
  const vid_t w = g.col[i];
  DBFS_DCHECK(static_cast<int64_t>(w) < g.n, 51, i);
  return static_cast<int64_t>(w) < g.n ? w : kSccNone;
}

// For the wave's 64 rows r0 + lane of g: whether some entry w of this lane's
// row has pred(v, w), v the row's vertex; walked only where `want`.  Called by
// all 64 lanes together (r0 is the wave's).  Every lane walks the first
// kSccLane entries of its row itself -- most walks end at one of the first
// entries -- and what is left of a longer row that found nothing there is
// walked by the wave.
template <class Pred>
__device__ __forceinline__ bool scc_row_any(const ShardView& g, int64_t r0, bool want, Pred pred) {
  const int lane = lane_id();
  eid_t b = 0, e = 0;
  if (want) scc_row(g, r0 + lane, b, e);
  const eid_t mid = min(e, b + kSccLane);
  bool found = false;
  {
    const vid_t v = static_cast<vid_t>(g.lo + r0 + lane);
    for (eid_t i = b; i < mid && !found; ++i) {
      const vid_t w = scc_entry(g, i);
      found = w != kSccNone && pred(v, w);
    }
  }
  unsigned long long lm = __ballot(!found && mid < e);
  while (lm) {
    const int l = __ffsll(static_cast<long long>(lm)) - 1;
    lm &= lm - 1;
    const eid_t bl = readlane_i64(mid, l), el = readlane_i64(e, l);
    const vid_t vl = static_cast<vid_t>(g.lo + r0 + l);
    bool any = false;
    for (eid_t i = bl; i < el && !any; i += kWave) {
      bool hit = false;
      if (i + lane < el) {
        const vid_t w = scc_entry(g, i + lane);
        hit = w != kSccNone && pred(vl, w);
      }
      any = __ballot(hit) != 0ull;
    }
    if (lane == l) found = any;
  }
  return found;
}

__device__ __forceinline__ vid_t wave_min_u32(vid_t x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x = min(x, static_cast<vid_t>(__shfl_xor(static_cast<int>(x), off, kWave)));
  return x;
}

// ... the smallest val(v, w) over the entries of this lane's row (kSccNone: none).
template <class Val>
__device__ __forceinline__ vid_t scc_row_min(const ShardView& g, int64_t r0, bool want, Val val) {
  const int lane = lane_id();
  eid_t b = 0, e = 0;
  if (want) scc_row(g, r0 + lane, b, e);
  const bool wide = e - b > kSccLane;
  vid_t best = kSccNone;
  if (!wide) {
    const vid_t v = static_cast<vid_t>(g.lo + r0 + lane);
    for (eid_t i = b; i < e; ++i) {
      const vid_t w = scc_entry(g, i);
      if (w != kSccNone) best = min(best, val(v, w));
    }
  }
  unsigned long long lm = __ballot(wide);
  while (lm) {
    const int l = __ffsll(static_cast<long long>(lm)) - 1;
    lm &= lm - 1;
    const eid_t bl = readlane_i64(b, l), el = readlane_i64(e, l);
    const vid_t vl = static_cast<vid_t>(g.lo + r0 + l);
    vid_t m = kSccNone;
    for (eid_t i = bl + lane; i < el; i += kWave) {
      const vid_t w = scc_entry(g, i);
      if (w != kSccNone) m = min(m, val(vl, w));
    }
    m = wave_min_u32(m);
    if (lane == l) best = m;
  }
  return best;
}

// The sweep enqueued before this one changed nothing: the step is at its
// fixed point and this sweep has nothing to do.  (The value is from a launch
// that has ended; the same in every lane.)
__device__ __forceinline__ bool scc_surplus(const SccArgs& a) {
  return a.prev_changed &&
         __hip_atomic_load(const_cast<unsigned long long*>(a.prev_changed), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull;
}

// A wave's sum of `mine`, added to the counter by one lane.
__device__ __forceinline__ void scc_count(unsigned long long* counter, long long mine) {
  const long long total = wave_sum(mine);
  if (total && lane_id() == 0) atomicAdd(counter, static_cast<unsigned long long>(total));
}

__global__ __launch_bounds__(kSccBlock) void scc_init_kernel(SccArgs a) {
  const int64_t n = a.out.n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; v < n; v += stride) {
    a.scc[v] = kSccNone;
    a.cls[v] = kSccNone;
    a.colour[v] = kSccNone;
  }
}

// cls does not change during a trim; scc does (a neighbour settling in this
// launch no longer counts: seen now or by the next sweep).
__global__ __launch_bounds__(kSccBlock) void scc_trim_kernel(SccArgs a) {
  if (scc_surplus(a)) return;
  const int lane = lane_id();
  const int64_t rows = a.out.rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  long long settled = 0;
  auto counts = [&](vid_t v, vid_t w) {
    return w != v && a.cls[w] == a.cls[v] && scc_load(a.scc + w) == kSccNone;
  };
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSccBlock + (threadIdx.x & ~(kWave - 1)); r0 < rows;
       r0 += stride) {
    const int64_t r = r0 + lane;
    const vid_t v = static_cast<vid_t>(a.out.lo + r);
    const bool live = r < rows && a.scc[v] == kSccNone;
    const bool has_out = scc_row_any(a.out, r0, live, counts);
    const bool has_in = scc_row_any(a.in, r0, live && has_out, counts);
    if (live && !(has_out && has_in)) {
      scc_store(a.scc + v, v);
      ++settled;
    }
  }
  scc_count(a.changed, settled);
}

// (largest product, smaller id on a tie); id kSccNone with product 0: no vertex
__device__ __forceinline__ bool scc_pivot_better(unsigned long long p, vid_t i, unsigned long long q, vid_t j) {
  return p > q || (p == q && i < j);
}

// A workgroup's best (product, id) into out[0..1].
__device__ __forceinline__ void scc_block_pivot(unsigned long long prod, vid_t id, unsigned long long* out) {
  __shared__ unsigned long long s_p[kSccBlock / kWave];
  __shared__ vid_t s_i[kSccBlock / kWave];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long q = static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(prod), off, kWave));
    const vid_t j = static_cast<vid_t>(__shfl_xor(static_cast<int>(id), off, kWave));
    if (scc_pivot_better(q, j, prod, id)) prod = q, id = j;
  }
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_p[wave] = prod, s_i[wave] = id;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSccBlock / kWave; ++w)
      if (scc_pivot_better(s_p[w], s_i[w], prod, id)) prod = s_p[w], id = s_i[w];
    out[0] = prod;
    out[1] = id;
  }
}

__global__ __launch_bounds__(kSccBlock) void scc_pivot_kernel(SccArgs a) {
  const int64_t rows = a.out.rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  unsigned long long prod = 0;
  vid_t id = kSccNone;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; r < rows; r += stride) {
    const vid_t v = static_cast<vid_t>(a.out.lo + r);
    if (a.scc[v] != kSccNone) continue;
    eid_t ob, oe, ib, ie;
    scc_row(a.out, r, ob, oe);
    scc_row(a.in, r, ib, ie);
    const unsigned long long p = static_cast<unsigned long long>(oe - ob) * static_cast<unsigned long long>(ie - ib);
    if (scc_pivot_better(p, v, prod, id)) prod = p, id = v;
  }
  scc_block_pivot(prod, id, a.pivot_slots + static_cast<int64_t>(blockIdx.x) * 2);
}

// (a launch of its own: the slots are read after the launch that wrote them has ended)
__global__ __launch_bounds__(kSccBlock) void scc_pivot_finish_kernel(SccArgs a, int nslots) {
  unsigned long long prod = 0;
  vid_t id = kSccNone;
  for (int i = threadIdx.x; i < nslots; i += kSccBlock) {
    const unsigned long long p = a.pivot_slots[2 * i];
    const vid_t j = static_cast<vid_t>(a.pivot_slots[2 * i + 1]);
    if (scc_pivot_better(p, j, prod, id)) prod = p, id = j;
  }
  scc_block_pivot(prod, id, a.pivot_out);
}

__global__ __launch_bounds__(kSccBlock) void scc_colour_init_kernel(SccArgs a) {
  const int64_t n = a.out.n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; v < n; v += stride) {
    if (a.scc[v] != kSccNone) continue;
    const vid_t id = static_cast<vid_t>(v);
    a.colour[v] = !a.pivot_only || id == a.pivot ? id : kSccNone;
  }
}

// scc and cls do not change during the colouring; colour does.
__global__ __launch_bounds__(kSccBlock) void scc_forward_kernel(SccArgs a) {
  if (scc_surplus(a)) return;
  const int lane = lane_id();
  const int64_t rows = a.in.rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  long long changed = 0;
  auto colour_of = [&](vid_t v, vid_t u) {
    return u != v && a.cls[u] == a.cls[v] && a.scc[u] == kSccNone ? scc_load(a.colour + u) : kSccNone;
  };
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSccBlock + (threadIdx.x & ~(kWave - 1)); r0 < rows;
       r0 += stride) {
    const int64_t r = r0 + lane;
    const vid_t v = static_cast<vid_t>(a.in.lo + r);
    const bool live = r < rows && a.scc[v] == kSccNone;
    const vid_t m = scc_row_min(a.in, r0, live, colour_of);
    // (only this lane stores colour[v]: a plain load of it is its last value)
    if (live && m < a.colour[v]) {
      scc_store(a.colour + v, m);
      ++changed;
    }
  }
  scc_count(a.changed, changed);
}

// The pivot round's colouring: one colour, so a coloured vertex is done and an
// uncoloured one takes the pivot's from the first counting in-neighbour that
// has it -- a pull reach with the early exit, not a minimum over whole rows.
__global__ __launch_bounds__(kSccBlock) void scc_forward_pivot_kernel(SccArgs a) {
  if (scc_surplus(a)) return;
  const int lane = lane_id();
  const int64_t rows = a.in.rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  long long changed = 0;
  // (the first round: every class is equal and every colour is none but this
  // round's, so a vertex with the pivot's colour is live, of v's class and not v)
  auto coloured = [&](vid_t, vid_t u) { return scc_load(a.colour + u) == a.pivot; };
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSccBlock + (threadIdx.x & ~(kWave - 1)); r0 < rows;
       r0 += stride) {
    const int64_t r = r0 + lane;
    const vid_t v = static_cast<vid_t>(a.in.lo + r);
    const bool open = r < rows && a.scc[v] == kSccNone && a.colour[v] == kSccNone;
    if (scc_row_any(a.in, r0, open, coloured)) {
      scc_store(a.colour + v, a.pivot);
      ++changed;
    }
  }
  scc_count(a.changed, changed);
}

// colour and cls do not change during the closure; scc does.  A live v with
// colour c joins when it is the root (v == c) or has an out-neighbour with
// scc == c: no component settled earlier carries the label of a live root,
// so that neighbour has colour c and is in, and v lies on a cycle through c.
__global__ __launch_bounds__(kSccBlock) void scc_backward_kernel(SccArgs a) {
  if (scc_surplus(a)) return;
  const int lane = lane_id();
  const int64_t rows = a.out.rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  long long joined = 0;
  auto is_in = [&](vid_t v, vid_t w) { return scc_load(a.scc + w) == a.colour[v]; };
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSccBlock + (threadIdx.x & ~(kWave - 1)); r0 < rows;
       r0 += stride) {
    const int64_t r = r0 + lane;
    const vid_t v = static_cast<vid_t>(a.out.lo + r);
    const bool live = r < rows && a.scc[v] == kSccNone;
    const vid_t c = live ? a.colour[v] : kSccNone;
    const bool root = c == v;
    const bool reaches = scc_row_any(a.out, r0, c != kSccNone && !root, is_in);
    if (root || reaches) {
      scc_store(a.scc + v, c);
      ++joined;
    }
  }
  scc_count(a.changed, joined);
}

__global__ __launch_bounds__(kSccBlock) void scc_end_round_kernel(SccArgs a) {
  const int64_t n = a.out.n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; v < n; v += stride)
    if (a.scc[v] == kSccNone && a.colour[v] != kSccNone) a.cls[v] = a.colour[v];
}

// The smallest member of the pivot's component, one atomic per wave that holds one ...
__global__ __launch_bounds__(kSccBlock) void scc_relabel_min_kernel(SccArgs a) {
  const int64_t n = a.out.n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  vid_t m = kSccNone;
  // (ascending: a lane's first member is its smallest)
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; v < n && m == kSccNone; v += stride)
    if (a.scc[v] == a.pivot) m = static_cast<vid_t>(v);
  m = wave_min_u32(m);
  if (m != kSccNone && lane_id() == 0) atomicMin(a.relabel_min, m);
}

// ... and the gather (the next launch: the word is final).
__global__ __launch_bounds__(kSccBlock) void scc_relabel_apply_kernel(SccArgs a) {
  const int64_t n = a.out.n;
  const vid_t to = *a.relabel_min;
  DBFS_DCHECK(to <= a.pivot, 52, to);
  if (to > a.pivot) return;  // (the pivot itself is a member)
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSccBlock;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kSccBlock + threadIdx.x; v < n; v += stride)
    if (a.scc[v] == a.pivot) a.scc[v] = to;
}

void scc_check_views(const SccArgs& a) {
  DBFS_CHECK(a.out.lo == a.in.lo && a.out.rows == a.in.rows && a.out.n == a.in.n,
             "scc: the out- and in-views are not of the same rows");
}

}  // namespace

void scc_init(const SccArgs& a, hipStream_t st) {
  if (a.out.n <= 0) return;
  scc_init_kernel<<<grid_for(a.out.n, kSccBlock, kSccGrid), kSccBlock, 0, st>>>(a);
}

void scc_trim(const SccArgs& a, hipStream_t st) {
  scc_check_views(a);
  if (a.out.rows <= 0) return;
  scc_trim_kernel<<<grid_for(a.out.rows, kSccBlock, kSccGrid), kSccBlock, 0, st>>>(a);
}

void scc_pivot(const SccArgs& a, hipStream_t st) {
  static_assert(kSccPivotGrid <= kSccGrid, "a slot per workgroup");
  scc_check_views(a);
  int slots = 0;
  if (a.out.rows > 0) {
    slots = static_cast<int>(grid_for(a.out.rows, kSccBlock, kSccPivotGrid));
    scc_pivot_kernel<<<slots, kSccBlock, 0, st>>>(a);
  }
  // (a rank without rows: no slot, the answer is "none")
  scc_pivot_finish_kernel<<<1, kSccBlock, 0, st>>>(a, slots);
}

void scc_colour_init(const SccArgs& a, hipStream_t st) {
  if (a.out.n <= 0) return;
  scc_colour_init_kernel<<<grid_for(a.out.n, kSccBlock, kSccGrid), kSccBlock, 0, st>>>(a);
}

void scc_forward(const SccArgs& a, hipStream_t st) {
  scc_check_views(a);
  if (a.in.rows <= 0) return;
  const unsigned grid = grid_for(a.in.rows, kSccBlock, kSccGrid);
  if (a.pivot_only) scc_forward_pivot_kernel<<<grid, kSccBlock, 0, st>>>(a);
  else scc_forward_kernel<<<grid, kSccBlock, 0, st>>>(a);
}

void scc_backward(const SccArgs& a, hipStream_t st) {
  scc_check_views(a);
  if (a.out.rows <= 0) return;
  scc_backward_kernel<<<grid_for(a.out.rows, kSccBlock, kSccGrid), kSccBlock, 0, st>>>(a);
}

void scc_end_round(const SccArgs& a, hipStream_t st) {
  if (a.out.n <= 0) return;
  scc_end_round_kernel<<<grid_for(a.out.n, kSccBlock, kSccGrid), kSccBlock, 0, st>>>(a);
}

void scc_relabel(const SccArgs& a, hipStream_t st) {
  if (a.out.n <= 0) return;
  DBFS_CHECK(static_cast<int64_t>(a.pivot) < a.out.n, "scc_relabel: no pivot");
  (void)hipMemsetAsync(a.relabel_min, 0xFF, sizeof(vid_t), st);
  const unsigned grid = grid_for(a.out.n, kSccBlock, kSccGrid);
  scc_relabel_min_kernel<<<grid, kSccBlock, 0, st>>>(a);
  scc_relabel_apply_kernel<<<grid, kSccBlock, 0, st>>>(a);
}

unsigned long long take_check_scc() { return take_check_local(); }
void inject_check_scc(hipStream_t st) { inject_check_local(st); }
const bool kCheckedScc = kCheckedLocal;

}  // namespace kern
}  // namespace dbfs
