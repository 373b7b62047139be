// Shortest-path counts and Brandes dependencies over a finished batch pass's
// level matrix (gfx950, wave64; backend.hpp MsBcArgs).
//
//   ms_bc_init      the sources' 1.0 and the zeros
//   ms_bc_forward   one level of path counts: sigma[v] = sum of sigma[u] over
//                   v's predecessor entries one level closer
//   ms_bc_backward  one level of dependencies, the matrix turned in place from
//                   sigma into the coefficient (1 + delta) / sigma, and the
//                   vertex's share of the centrality vector
//
// Both sweeps walk as ms_check_kernel does (ms_kernels.hip): a wave per owned
// vertex, striding over the rows; lane s is source s; the row's level lines
// come from ms_walk_row (ms_walk.hpp), a group at a time.
// A value line (512 B per vertex) is touched only by the lanes whose level
// matches, and a vertex none of whose lanes sits on the launch's level is
// skipped after its own level line, before its row offsets are read.
// Every sum is pull-form and per lane in stored row order: no atomics on
// floating-point values, the same bits on every run.  A forward count past
// DBL_MAX sets its source's bit in MsBcArgs::overflow (an integer OR) and the
// engine fails the batch before the backward sweep.
#include <cfloat>

#include "ms_walk.hpp"

namespace dbfs {
namespace kern {
namespace {

constexpr int kMsBcBlock = 256;
// Workgroups at most: ms_check_kernel's value (its registers allow the same
// 8 waves per SIMD: profiles/ms_bfs_regs.txt).
constexpr int kMsBcGrid = 2048;

// Sum over the wave in a fixed order (lane i + lane i ^ 32, then ^ 16 .. ^ 1;
// every lane ends with the same bits).
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
  return x;
}

__global__ __launch_bounds__(kMsBcBlock) void ms_bc_init_kernel(MsBcArgs a) {
  const int lane = lane_id();
  const int64_t my_src = ((a.m.batch_mask >> lane) & 1ull) ? a.m.src[lane] : -1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (kMsBcBlock / kWave);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * (kMsBcBlock / kWave) + (threadIdx.x >> 6);
  for (int64_t v = first; v < a.m.lvl_rows; v += stride) a.val[v * kMsSources + lane] = v == my_src ? 1.0 : 0.0;
  for (int64_t r = first; r < a.g.rows; r += stride) a.own[r * kMsSources + lane] = a.g.lo + r == my_src ? 1.0 : 0.0;
}

// The sum, per lane, of val[w][lane] over the entries w of row [rs, re) whose
// level is `want` -- for the lanes with `at` set; the others load no value.
template <class L>
__device__ __forceinline__ double ms_bc_row_sum(const MsBcArgs& a, const L* __restrict__ lvl, eid_t rs, eid_t re,
                                                bool at, int want) {
  constexpr int kNone = ms_unreached<L>();
  const double* __restrict__ val = a.val;
  const int lane = lane_id();
  double sum = 0.0;
  ms_walk_row<L, kMsWalkAhead>(lvl, a.col, rs, re, a.m.lvl_rows, 28, [&](int valid, const vid_t* w, const int* lw) {
    double x[kMsWalkAhead];  // (the group's value loads: issued together, after its level lines)
#pragma unroll
    for (int i = 0; i < kMsWalkAhead; ++i) {
      // (&, not &&: a branch on the wave-uniform i < valid would take the entry's level load along)
      const bool take = (i < valid) & at & (lw[i] == want) & (lw[i] != kNone);
      x[i] = take ? val[static_cast<int64_t>(w[i]) * kMsSources + lane] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kMsWalkAhead; ++i) sum += x[i];  // (stored row order; + 0.0 changes no bit of a sum >= 0)
    return true;
  });
  return sum;
}

// A vertex's forward result: the path counts of the lanes on the level.
// Returns the lanes whose count left double's range, for MsBcArgs::overflow
// (the engine fails the batch on it).  The caller ORs them in a scalar and
// stores once, after its rows: an atomic inside the row loop would turn the
// loop's scalar row-offset loads into vector loads.  Wave-uniform call.
__device__ __forceinline__ unsigned long long ms_bc_store_forward(const MsBcArgs& a, int64_t r, bool at, double sum) {
  if (at) a.own[r * kMsSources + lane_id()] = sum;
  return __ballot(at && !(sum <= DBL_MAX));
}

// A vertex's backward result from acc, the sum of its successors'
// coefficients: delta, the vertex's own coefficient in place of sigma, and
// its share of dep.  Wave-uniform call.
__device__ __forceinline__ void ms_bc_store_backward(const MsBcArgs& a, int64_t r, bool at, bool counts, double acc) {
  const int lane = lane_id();
  double delta = 0.0;
  if (at) {  // (reached: sigma >= 1; no other lane divides)
    const double sigma = a.own[r * kMsSources + lane];
    delta = sigma * acc;
    a.own[r * kMsSources + lane] = (1.0 + delta) / sigma;
  }
  if (__ballot(counts) == 0ull) return;
  const double mine = wave_sum_f64(counts ? delta : 0.0);
  if (lane == 0) a.dep[r] += mine;  // (one wave per vertex and launch: a plain store)
}

template <class L>
__global__ __launch_bounds__(kMsBcBlock) void ms_bc_forward_kernel(MsBcArgs a) {
  const ShardView& g = a.g;
  const L* __restrict__ lvl = static_cast<const L*>(a.m.lvl);
  const int lane = lane_id();
  const bool on = (a.m.batch_mask >> lane) & 1ull;  // lanes past the pass's sources are idle
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  unsigned long long walked = 0, over = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (kMsBcBlock / kWave);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kMsBcBlock / kWave) + wave; r < g.rows; r += stride) {
    const int64_t v = g.lo + r;
    DBFS_DCHECK(v < a.m.lvl_rows, 27, v);
    const bool at = on && static_cast<int>(lvl[v * kMsSources + lane]) == a.level;
    if (__ballot(at) == 0ull) continue;
    const eid_t rs = a.row_off[r], re = a.row_off[r + 1];
    DBFS_DCHECK(rs >= 0 && rs <= re && re <= a.nnz, 29, r);
    if (a.n_long > 0 && re - rs > a.split_above) continue;  // (ms_bc_long_kernel's)
    ++walked;
    over |= ms_bc_store_forward(a, r, at, ms_bc_row_sum<L>(a, lvl, rs, re, at, a.level - 1));
  }
  if (a.walked && lane == 0 && walked) atomicAdd(a.walked, walked);
  if (lane == 0 && over) atomicOr(a.overflow, over);
}

template <class L>
__global__ __launch_bounds__(kMsBcBlock) void ms_bc_backward_kernel(MsBcArgs a) {
  const ShardView& g = a.g;
  const L* __restrict__ lvl = static_cast<const L*>(a.m.lvl);
  const int lane = lane_id();
  const bool on = (a.m.batch_mask >> lane) & 1ull;
  const int64_t my_src = on ? a.m.src[lane] : -1;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  unsigned long long walked = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (kMsBcBlock / kWave);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kMsBcBlock / kWave) + wave; r < g.rows; r += stride) {
    const int64_t v = g.lo + r;
    DBFS_DCHECK(v < a.m.lvl_rows, 27, v);
    const bool at = on && static_cast<int>(lvl[v * kMsSources + lane]) == a.level;
    if (__ballot(at) == 0ull) continue;
    double acc = 0.0;
    if (!a.leaf) {
      const eid_t rs = a.row_off[r], re = a.row_off[r + 1];
      DBFS_DCHECK(rs >= 0 && rs <= re && re <= a.nnz, 29, r);
      if (a.n_long > 0 && re - rs > a.split_above) continue;  // (ms_bc_long_kernel's)
      acc = ms_bc_row_sum<L>(a, lvl, rs, re, at, a.level + 1);
    }
    ++walked;
    ms_bc_store_backward(a, r, at, at && v != my_src, acc);
  }
  if (a.walked && lane == 0 && walked) atomicAdd(a.walked, walked);
}

// The rows of more than split_above entries (MsBcArgs::long_rows), a
// workgroup of 16 waves per row: wave w walks the w-th sixteenth of the row
// (whole 64-entry steps), the partial sums meet in LDS and wave 0 adds them in
// wave order, then finishes the vertex as the kernels above do -- a hub's row
// is 1/16 of one wave's walk, and the result is the same on every run.
constexpr int kMsBcLongBlock = 1024;
constexpr int kMsBcLongWaves = kMsBcLongBlock / kWave;

template <class L, bool kBackward>
__global__ __launch_bounds__(kMsBcLongBlock) void ms_bc_long_kernel(MsBcArgs a) {
  __shared__ double s_part[kMsBcLongWaves][kWave];
  const ShardView& g = a.g;
  const L* __restrict__ lvl = static_cast<const L*>(a.m.lvl);
  const int lane = lane_id();
  const bool on = (a.m.batch_mask >> lane) & 1ull;
  const int64_t my_src = on ? a.m.src[lane] : -1;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  unsigned long long walked = 0, over = 0;  // (wave 0's)
  for (int64_t i = blockIdx.x; i < a.n_long; i += gridDim.x) {
    const int64_t r = a.long_rows[i];
    const int64_t v = g.lo + r;
    DBFS_DCHECK(r < g.rows && v < a.m.lvl_rows, 30, r);
    // (every wave reads the same line: the skip is uniform over the workgroup)
    const bool at = on && static_cast<int>(lvl[v * kMsSources + lane]) == a.level;
    if (__ballot(at) == 0ull) continue;
    const eid_t rs = a.row_off[r], re = a.row_off[r + 1];
    DBFS_DCHECK(rs >= 0 && rs <= re && re <= a.nnz, 29, r);
    const eid_t chunk = (((re - rs + kMsBcLongWaves - 1) / kMsBcLongWaves) + kWave - 1) & ~static_cast<eid_t>(kWave - 1);
    const eid_t b = min(re, rs + wave * chunk), en = min(re, b + chunk);
    s_part[wave][lane] = ms_bc_row_sum<L>(a, lvl, b, en, at, kBackward ? a.level + 1 : a.level - 1);
    __syncthreads();
    if (wave == 0) {
      double sum = 0.0;
#pragma unroll
      for (int w = 0; w < kMsBcLongWaves; ++w) sum += s_part[w][lane];
      ++walked;
      if (kBackward) ms_bc_store_backward(a, r, at, at && v != my_src, sum);
      else over |= ms_bc_store_forward(a, r, at, sum);
    }
    __syncthreads();  // (s_part is the next row's)
  }
  if (a.walked && threadIdx.x == 0 && walked) atomicAdd(a.walked, walked);
  if (!kBackward && threadIdx.x == 0 && over) atomicOr(a.overflow, over);
}

__global__ __launch_bounds__(kMsBcBlock) void ms_bc_long_rows_kernel(const eid_t* row_off, int64_t rows, int64_t above,
                                                                      vid_t* list, int64_t cap,
                                                                      unsigned long long* count) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBcBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kMsBcBlock + threadIdx.x; r < rows; r += stride) {
    if (row_off[r + 1] - row_off[r] <= above) continue;
    const unsigned long long at = atomicAdd(count, 1ull);
    if (at < static_cast<unsigned long long>(cap)) list[at] = static_cast<vid_t>(r);
  }
}

// One level of a sweep: the rows by their wave, then the long ones.
template <bool kBackward>
void ms_bc_sweep(const MsBcArgs& a, hipStream_t st) {
  if (a.g.rows <= 0) return;
  const unsigned grid = grid_for(a.g.rows, kMsBcBlock / kWave, kMsBcGrid);
  ms_level_type(a.m.lvl_bytes, [&](auto l) {
    using L = decltype(l);
    if (kBackward) ms_bc_backward_kernel<L><<<grid, kMsBcBlock, 0, st>>>(a);
    else ms_bc_forward_kernel<L><<<grid, kMsBcBlock, 0, st>>>(a);
    if (a.n_long > 0)
      ms_bc_long_kernel<L, kBackward><<<grid_for(a.n_long, 1, kMsBcGrid), kMsBcLongBlock, 0, st>>>(a);
  });
}

}  // namespace

void ms_bc_init(const MsBcArgs& a, hipStream_t st) {
  if (a.m.lvl_rows <= 0) return;
  ms_bc_init_kernel<<<grid_for(a.m.lvl_rows, kMsBcBlock / kWave, kMsBcGrid), kMsBcBlock, 0, st>>>(a);
}

void ms_bc_forward(const MsBcArgs& a, hipStream_t st) {
  DBFS_CHECK(a.overflow, "ms_bc_forward: MsBcArgs::overflow missing");
  ms_bc_sweep<false>(a, st);
}
void ms_bc_backward(const MsBcArgs& a, hipStream_t st) { ms_bc_sweep<true>(a, st); }

void ms_bc_long_rows(const eid_t* row_off, int64_t rows, int64_t above, vid_t* list, int64_t cap,
                     unsigned long long* count, hipStream_t st) {
  if (rows <= 0) return;
  ms_bc_long_rows_kernel<<<grid_for(rows, kMsBcBlock, kMsBcGrid), kMsBcBlock, 0, st>>>(row_off, rows, above, list, cap,
                                                                                      count);
}

unsigned long long take_check_ms_bc() { return take_check_local(); }

}  // namespace kern
}  // namespace dbfs
