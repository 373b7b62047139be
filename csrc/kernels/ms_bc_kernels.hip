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
//
// Every kernel is templated on the value type next to the level type: MsBcF64
// (doubles, the 512-B line above) or MsBcWide (dbfs/wide.hpp: a mantissa and
// an exponent, a 768-B record per vertex -- 64 mantissas, then 64 exponents, so
// a lane's two loads hit adjacent lines).  The wide form has no overflow mask,
// its coefficients stay wide (they underflow a double exactly when counts
// overflow it), and delta = sigma * acc leaves it as a double.
#include <cfloat>

#include "dbfs/wide.hpp"
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

// The value types.  T: a stored value; Sum: a lane's running sum; val / own:
// MsBcArgs' matrices; load / store: lane's value of row v; finish: a forward
// sum as it is stored, in_range: whether it may be; turn: delta = sigma * acc
// and sigma's coefficient (1 + delta) / sigma; LDS: what the long rows' 16
// partial sums meet in.
struct MsBcF64 {
  using T = double;
  using Sum = double;
  using Mat = double;
  static __device__ __forceinline__ const Mat* val(const MsBcArgs& a) { return a.val; }
  static __device__ __forceinline__ Mat* own(const MsBcArgs& a) { return a.own; }
  static __device__ __forceinline__ T zero() { return 0.0; }
  static __device__ __forceinline__ T one() { return 1.0; }
  static __device__ __forceinline__ Sum sum_zero() { return 0.0; }
  static __device__ __forceinline__ T load(const Mat* m, int64_t v, int lane) { return m[v * kMsSources + lane]; }
  static __device__ __forceinline__ void store(Mat* m, int64_t v, int lane, T x) { m[v * kMsSources + lane] = x; }
  // (stored row order; + 0.0 changes no bit of a sum >= 0)
  static __device__ __forceinline__ void add(Sum& sum, T x) { sum += x; }
  static __device__ __forceinline__ T finish(Sum sum) { return sum; }
  static __device__ __forceinline__ bool in_range(Sum sum) { return sum <= DBL_MAX; }
  static __device__ __forceinline__ double turn(T sigma, Sum acc, T& coef) {
    const double delta = sigma * acc;
    coef = (1.0 + delta) / sigma;
    return delta;
  }
  struct LDS {
    double part[1024 / kWave][kWave];
    __device__ __forceinline__ void put(int w, int lane, Sum x) { part[w][lane] = x; }
    __device__ __forceinline__ Sum get(int w, int lane) const { return part[w][lane]; }
  };
};
struct MsBcWide {
  using T = Wide;
  using Sum = WideSum;
  using Mat = unsigned char;
  static __device__ __forceinline__ const Mat* val(const MsBcArgs& a) { return a.wval; }
  static __device__ __forceinline__ Mat* own(const MsBcArgs& a) { return a.wown; }
  static __device__ __forceinline__ T zero() { return wide_zero(); }
  static __device__ __forceinline__ T one() { return wide_one(); }
  static __device__ __forceinline__ Sum sum_zero() { return wide_sum_zero(); }
  static __device__ __forceinline__ T load(const Mat* m, int64_t v, int lane) { return wide_load(m, v, lane); }
  static __device__ __forceinline__ void store(Mat* m, int64_t v, int lane, T x) { wide_store(m, v, lane, x); }
  static __device__ __forceinline__ void add(Sum& sum, T x) { wide_add(sum, x); }
  static __device__ __forceinline__ T finish(Sum sum) { return wide_normalise(sum); }
  static __device__ __forceinline__ bool in_range(Sum) { return true; }  // (no overflow mask in this form)
  // (sigma, acc and the coefficient wide; delta, at most n, a double: 0 when below 2^-1074)
  static __device__ __forceinline__ double turn(T sigma, Sum acc, T& coef) {
    const double delta = wide_delta(sigma, acc);
    coef = wide_coefficient(delta, sigma);
    return delta;
  }
  struct LDS {
    double m[1024 / kWave][kWave];
    int32_t e[1024 / kWave][kWave];
    __device__ __forceinline__ void put(int w, int lane, Sum x) { m[w][lane] = x.m, e[w][lane] = x.e; }
    __device__ __forceinline__ Sum get(int w, int lane) const { return Sum{m[w][lane], e[w][lane]}; }
  };
};

template <class V>
__global__ __launch_bounds__(kMsBcBlock) void ms_bc_init_kernel(MsBcArgs a) {
  const int lane = lane_id();
  const int64_t my_src = ((a.m.batch_mask >> lane) & 1ull) ? a.m.src[lane] : -1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (kMsBcBlock / kWave);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * (kMsBcBlock / kWave) + (threadIdx.x >> 6);
  typename V::Mat* const val = const_cast<typename V::Mat*>(V::val(a));
  for (int64_t v = first; v < a.m.lvl_rows; v += stride) V::store(val, v, lane, v == my_src ? V::one() : V::zero());
  for (int64_t r = first; r < a.g.rows; r += stride)
    V::store(V::own(a), r, lane, a.g.lo + r == my_src ? V::one() : V::zero());
}

// The sum, per lane, of val[w][lane] over the entries w of row [rs, re) whose
// level is `want` -- for the lanes with `at` set; the others load no value.
template <class L, class V>
__device__ __forceinline__ typename V::Sum ms_bc_row_sum(const MsBcArgs& a, const L* __restrict__ lvl, eid_t rs,
                                                         eid_t re, bool at, int want) {
  constexpr int kNone = ms_unreached<L>();
  const typename V::Mat* __restrict__ val = V::val(a);
  const int lane = lane_id();
  typename V::Sum sum = V::sum_zero();
  ms_walk_row<L, kMsWalkAhead>(lvl, a.col, rs, re, a.m.lvl_rows, 28, [&](int valid, const vid_t* w, const int* lw) {
    typename V::T x[kMsWalkAhead];  // (the group's value loads: issued together, after its level lines)
#pragma unroll
    for (int i = 0; i < kMsWalkAhead; ++i) {
      // (&, not &&: a branch on the wave-uniform i < valid would take the entry's level load along)
      const bool take = (i < valid) & at & (lw[i] == want) & (lw[i] != kNone);
      x[i] = take ? V::load(val, static_cast<int64_t>(w[i]), lane) : V::zero();
    }
#pragma unroll
    for (int i = 0; i < kMsWalkAhead; ++i) V::add(sum, x[i]);  // (stored row order)
    return true;
  });
  return sum;
}

// A vertex's forward result: the path counts of the lanes on the level.
// Returns the lanes whose count left double's range, for MsBcArgs::overflow
// (the engine fails the batch on it).  The caller ORs them in a scalar and
// stores once, after its rows: an atomic inside the row loop would turn the
// loop's scalar row-offset loads into vector loads.  Wave-uniform call.
// The wide form stores the normalised sum and has no such lanes.
template <class V>
__device__ __forceinline__ unsigned long long ms_bc_store_forward(const MsBcArgs& a, int64_t r, bool at,
                                                                  typename V::Sum sum) {
  if (at) V::store(V::own(a), r, lane_id(), V::finish(sum));
  return __ballot(at && !V::in_range(sum));
}

// A vertex's backward result from acc, the sum of its successors'
// coefficients: delta, the vertex's own coefficient in place of sigma, and
// its share of dep.  Wave-uniform call.
template <class V>
__device__ __forceinline__ void ms_bc_store_backward(const MsBcArgs& a, int64_t r, bool at, bool counts,
                                                     typename V::Sum acc) {
  const int lane = lane_id();
  double delta = 0.0;
  if (at) {  // (reached: sigma >= 1; no other lane divides)
    typename V::T coef;
    delta = V::turn(V::load(V::own(a), r, lane), acc, coef);
    V::store(V::own(a), r, lane, coef);
  }
  if (__ballot(counts) == 0ull) return;
  const double mine = wave_sum_f64(counts ? delta : 0.0);
  if (lane == 0) a.dep[r] += mine;  // (one wave per vertex and launch: a plain store)
}

template <class L, class V>
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
    over |= ms_bc_store_forward<V>(a, r, at, ms_bc_row_sum<L, V>(a, lvl, rs, re, at, a.level - 1));
  }
  if (a.walked && lane == 0 && walked) atomicAdd(a.walked, walked);
  if (lane == 0 && over) atomicOr(a.overflow, over);  // (wide: never)
}

template <class L, class V>
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
    typename V::Sum acc = V::sum_zero();
    if (!a.leaf) {
      const eid_t rs = a.row_off[r], re = a.row_off[r + 1];
      DBFS_DCHECK(rs >= 0 && rs <= re && re <= a.nnz, 29, r);
      if (a.n_long > 0 && re - rs > a.split_above) continue;  // (ms_bc_long_kernel's)
      acc = ms_bc_row_sum<L, V>(a, lvl, rs, re, at, a.level + 1);
    }
    ++walked;
    ms_bc_store_backward<V>(a, r, at, at && v != my_src, acc);
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

template <class L, class V, bool kBackward>
__global__ __launch_bounds__(kMsBcLongBlock) void ms_bc_long_kernel(MsBcArgs a) {
  static_assert(kMsBcLongWaves == 1024 / kWave, "MsBcF64::LDS, MsBcWide::LDS");
  __shared__ typename V::LDS s_part;
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
    s_part.put(wave, lane, ms_bc_row_sum<L, V>(a, lvl, b, en, at, kBackward ? a.level + 1 : a.level - 1));
    __syncthreads();
    if (wave == 0) {
      typename V::Sum sum = V::sum_zero();
#pragma unroll
      for (int w = 0; w < kMsBcLongWaves; ++w) V::add(sum, s_part.get(w, lane));
      ++walked;
      if (kBackward) ms_bc_store_backward<V>(a, r, at, at && v != my_src, sum);
      else over |= ms_bc_store_forward<V>(a, r, at, sum);
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

// f(V{}) with the value type MsBcArgs::wide selects.
template <class F>
void ms_bc_value_type(const MsBcArgs& a, F&& f) {
  if (a.wide) {
    DBFS_CHECK(a.wval && a.wown, "MsBcArgs: wide without wval / wown");
    f(MsBcWide{});
  } else {
    f(MsBcF64{});
  }
}

// One level of a sweep: the rows by their wave, then the long ones.
template <bool kBackward>
void ms_bc_sweep(const MsBcArgs& a, hipStream_t st) {
  if (a.g.rows <= 0) return;
  const unsigned grid = grid_for(a.g.rows, kMsBcBlock / kWave, kMsBcGrid);
  ms_bc_value_type(a, [&](auto val) {
    using V = decltype(val);
    ms_level_type(a.m.lvl_bytes, [&](auto l) {
      using L = decltype(l);
      if (kBackward) ms_bc_backward_kernel<L, V><<<grid, kMsBcBlock, 0, st>>>(a);
      else ms_bc_forward_kernel<L, V><<<grid, kMsBcBlock, 0, st>>>(a);
      if (a.n_long > 0)
        ms_bc_long_kernel<L, V, kBackward><<<grid_for(a.n_long, 1, kMsBcGrid), kMsBcLongBlock, 0, st>>>(a);
    });
  });
}

}  // namespace

void ms_bc_init(const MsBcArgs& a, hipStream_t st) {
  if (a.m.lvl_rows <= 0) return;
  ms_bc_value_type(a, [&](auto val) {
    ms_bc_init_kernel<decltype(val)><<<grid_for(a.m.lvl_rows, kMsBcBlock / kWave, kMsBcGrid), kMsBcBlock, 0, st>>>(a);
  });
}

void ms_bc_forward(const MsBcArgs& a, hipStream_t st) {
  DBFS_CHECK(a.overflow || a.wide, "ms_bc_forward: MsBcArgs::overflow missing");
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
void inject_check_ms_bc(hipStream_t st) { inject_check_local(st); }
const bool kCheckedMsBc = kCheckedLocal;

}  // namespace kern
}  // namespace dbfs
