// Concurrent multi-source BFS kernels (gfx950, wave64): one 64-bit word per
// vertex carries up to 64 sources (bit s = source s; backend.hpp MsState).
//
//   ms_init    seeds a batch (the clears are fills enqueued before it)
//   ms_pull    dense level: every vertex that still misses sources ORs the
//              frontier words of its row, lane per vertex, long rows by the wave
//   ms_push    sparse level: the active vertices OR their frontier word into
//              their neighbours' `next` words (returning 64-bit atomic OR)
//   ms_settle  the touched vertices of a push level: new bits, bookkeeping
//   ms_check   after a pass: the level matrix against every edge, all sources
//              at once (violation counts, parent trees)
//
// Bookkeeping of a vertex with new bits (ms_record): the level bytes (lane s
// stores source s's level: one partial 64-B line per vertex), one
// wave-aggregated append to the next active list, per-source counts by
// ballots.  A level's totals leave the kernel as in the fused finishes
// (kernel_common.hpp last-arriver hand-offs): per-workgroup slots stored
// write-through, a ticket, the last workgroup sums them.
#include <algorithm>

#include "ms_walk.hpp"

namespace dbfs {
namespace kern {
namespace {

constexpr int kMsBlock = 256;
// rows of up to kMsPushLane entries are pushed by their lane, longer ones by
// the whole wave (64 entries per step), rows past kMsPushWave by the whole
// grid in a launch of their own (ms_push_long_kernel): a level whose few
// thousand active vertices are hubs would otherwise run on a few dozen waves
constexpr int kMsPushLane = 32;
constexpr int kMsPushWave = 1024;

__device__ __forceinline__ word_t wave_or(word_t x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) x |= __shfl_xor(x, off, kWave);
  return x;
}

__device__ __forceinline__ word_t uniform64(word_t x) {
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x));
  const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x >> 32));
  return (static_cast<word_t>(hi) << 32) | lo;
}

__device__ __forceinline__ void agent_store(int64_t* p, long long v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ long long agent_load(const int64_t* p) {
  return static_cast<long long>(__hip_atomic_load(reinterpret_cast<unsigned long long*>(const_cast<int64_t*>(p)),
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Per-lane accumulators of a wave over its steps: lane s counts source s.
struct MsAcc {
  long long src = 0;  // vertices source `lane` discovered
  long long deg = 0;  // degrees of this lane's vertices with new bits
};

// Wave-uniform call: lane `has` a vertex v (local row) with new bits nw and
// degree deg.  Level bytes, active-list append, per-source counts.
template <class L>
__device__ __forceinline__ void ms_record(const MsState& s, bool has, int64_t v, word_t nw, long long deg, MsAcc& acc) {
  const bool got = has && nw != 0;
  const unsigned long long found = __ballot(got);
  if (!found) return;
  const int lane = lane_id();
  const int leader = __ffsll(static_cast<long long>(found)) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(&s.cursor[0], static_cast<unsigned long long>(__popcll(found)));
  base = readlane64(base, leader);
  if (got) {
    DBFS_DCHECK(base + mask_rank(found) < static_cast<unsigned long long>(s.g.rows), 20, base);
    s.active_out[base + mask_rank(found)] = static_cast<vid_t>(v);
    acc.deg += deg;
  }
  // 64 x 64 bit transpose by ballots, only over the sources the wave found
  word_t uni = uniform64(wave_or(got ? nw : 0ull));
  while (uni) {
    const int src = __ffsll(static_cast<long long>(uni)) - 1;
    uni &= uni - 1;
    const int c = __popcll(__ballot(got && ((nw >> src) & 1ull)));
    if (lane == src) acc.src += c;
  }
  if (s.lvl) {
    L* lvl = static_cast<L*>(s.lvl);
    unsigned long long f = found;
    while (f) {
      const int l = __ffsll(static_cast<long long>(f)) - 1;
      f &= f - 1;
      const word_t nl = readlane64(nw, l);
      const int64_t vl = readlane_i64(v, l);
      if ((nl >> lane) & 1ull) lvl[vl * kMsSources + lane] = static_cast<L>(s.level);
    }
  }
}

// Every thread of the workgroup, once, after its last step: the workgroup's
// totals to its slot, the ticket, and in the last workgroup the level's totals
// to stats and the mailbox.  s_tot: kMsStats LDS words, zero before the steps.
__device__ __forceinline__ void ms_finish(const MsState& s, const MsAcc& acc, unsigned long long* s_tot,
                                          bool reset_touched) {
  __shared__ int s_last;
  const int t = threadIdx.x;
  const int lane = lane_id();
  if (acc.src) atomicAdd(&s_tot[2 + lane], static_cast<unsigned long long>(acc.src));
  const long long d = wave_sum(acc.deg);
  if (lane == 0 && d) atomicAdd(&s_tot[1], static_cast<unsigned long long>(d));
  __syncthreads();
  if (t < kMsStats) agent_store(s.tot + static_cast<int64_t>(blockIdx.x) * kMsStats + t, static_cast<long long>(s_tot[t]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    s_last = atomicAdd(s.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    if (s_last) last_arriver_acquire();
  }
  __syncthreads();
  if (!s_last) return;
  if (t < kMsStats) s_tot[t] = 0ull;
  __syncthreads();
  const int64_t n = static_cast<int64_t>(gridDim.x) * kMsStats;
  for (int64_t i = t; i < n; i += blockDim.x) {
    const long long x = agent_load(s.tot + i);
    if (x) atomicAdd(&s_tot[i % kMsStats], static_cast<unsigned long long>(x));
  }
  __syncthreads();
  if (t == 0) {
    s_tot[0] = __hip_atomic_load(&s.cursor[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s.cursor[0] = 0ull;
    if (reset_touched) s.cursor[1] = s.cursor[2] = 0ull;
    *s.ticket = 0u;  // the next launch is stream-ordered after this one
  }
  __syncthreads();
  if (t < kMsStats) {
    s.stats[t] = static_cast<int64_t>(s_tot[t]);
    if (s.mailbox)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(&s.mailbox->v[t]), s_tot[t], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0 && s.mailbox)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&s.mailbox->seq), static_cast<unsigned long long>(s.seq),
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Wave-uniform call: lane `has` an edge into w carrying the frontier word f.
__device__ __forceinline__ void ms_push_edge(const MsState& s, vid_t* touched, bool has, word_t f, vid_t w) {
  bool app = false;
  if (has) {
    DBFS_DCHECK(static_cast<int64_t>(w) < s.g.rows, 21, w);
    // (a load of next[w] first, to skip the atomic when the word already holds
    // the bits, measured no faster: profiles/ms_bfs_ab.txt)
    const word_t m = f & ~s.seen[w];
    if (m) app = atomicOr(&s.next[w], m) == 0ull;
  }
  const unsigned long long am = __ballot(app);
  if (!am) return;
  const int leader = __ffsll(static_cast<long long>(am)) - 1;
  unsigned long long base = 0;
  if (lane_id() == leader) base = atomicAdd(&s.cursor[1], static_cast<unsigned long long>(__popcll(am)));
  base = readlane64(base, leader);
  if (app) {
    DBFS_DCHECK(base + mask_rank(am) < static_cast<unsigned long long>(s.g.rows), 22, base);
    touched[base + mask_rank(am)] = w;
  }
}

}  // namespace

// One wave: the batch's sources (k <= 64), after the fills.
template <class L>
__global__ __launch_bounds__(kWave) void ms_init_kernel(MsInitArgs a) {
  const MsState& s = a.s;
  const int t = lane_id();
  const bool has = t < a.k;
  const int64_t v = has ? a.src[t] : 0;
  const bool owned = has && v >= s.g.lo && v < s.g.lo + s.g.rows;
  const int64_t r = v - s.g.lo;
  const word_t bit = 1ull << t;
  if (has) atomicOr(&s.front[v], bit);
  bool first = owned;
  if (owned) {
    atomicOr(&s.seen[r], bit);
    if (s.lvl) static_cast<L*>(s.lvl)[r * kMsSources + t] = static_cast<L>(0);
    // (two sources on one vertex: the vertex is listed once)
    for (int u = 0; u < t; ++u)
      if (a.src[u] == v) first = false;
  }
  const unsigned long long fm = __ballot(first);
  long long deg = 0;
  if (first) {
    s.active_out[mask_rank(fm)] = static_cast<vid_t>(r);
    deg = s.g.row_off[r + 1] - s.g.row_off[r];
  }
  deg = wave_sum(deg);
  const long long mine = t == 0 ? __popcll(fm) : (t == 1 ? deg : 0);
  if (t < 2) s.stats[t] = mine;
  s.stats[2 + t] = owned ? 1 : 0;
  if (s.mailbox) {
    if (t < 2)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(&s.mailbox->v[t]), static_cast<unsigned long long>(mine),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&s.mailbox->v[2 + t]), owned ? 1ull : 0ull,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(&s.mailbox->seq), static_cast<unsigned long long>(s.seq),
                         __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// kDirected: the rows searched are the in-edge shard's (MsState::in_row_off /
// in_col), and a vertex with new bits is recorded with its out-degree, read
// from g.row_off only then.  The undirected instantiation reads g's arrays
// alone, as before the flag existed.
template <class L, bool kDirected>
__global__ __launch_bounds__(kMsBlock) void ms_pull_kernel(MsPullArgs a) {
  __shared__ unsigned long long s_tot[kMsStats];
  const MsState& s = a.s;
  const ShardView& g = s.g;
  const eid_t* row_off = kDirected ? s.in_row_off : g.row_off;
  const vid_t* col = kDirected ? s.in_col : g.col;
  const int t = threadIdx.x;
  const int lane = lane_id();
  if (t < kMsStats) s_tot[t] = 0ull;
  __syncthreads();
  MsAcc acc;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t v0 = static_cast<int64_t>(blockIdx.x) * kMsBlock + (t & ~(kWave - 1)); v0 < g.rows; v0 += stride) {
    const int64_t v = v0 + lane;
    const bool in = v < g.rows;
    word_t sv = 0, need = 0;
    eid_t rs = 0, re = 0;
    if (in) {
      sv = s.seen[v];
      need = ~sv & s.batch_mask;
      if (need) {
        rs = row_off[v];
        re = row_off[v + 1];
        if (rs == re) need = 0ull;
      }
    }
    word_t got = 0;
    if (need) {
      const eid_t lim = min(re, rs + static_cast<eid_t>(a.lane_limit));
      for (eid_t e = rs; e < lim; ++e) {
        got |= s.front[col[e]];
        if ((got & need) == need) break;
      }
    }
    // rows past the per-lane limit: the wave reads 64 neighbours per step
    unsigned long long dm = __ballot(need != 0 && (got & need) != need && re - rs > a.lane_limit);
    while (dm) {
      const int l = __ffsll(static_cast<long long>(dm)) - 1;
      dm &= dm - 1;
      const eid_t b = readlane_i64(rs, l) + a.lane_limit, en = readlane_i64(re, l);
      const word_t nd = readlane64(need, l);
      word_t x = readlane64(got, l);
      for (eid_t e = b; e < en; e += kWave) {
        const word_t f = e + lane < en ? s.front[col[e + lane]] : 0ull;
        x |= wave_or(f);
        if ((x & nd) == nd) break;
      }
      if (lane == l) got = x;
    }
    const word_t nw = got & need;
    if (in) {
      if (nw) s.seen[v] = sv | nw;
      s.next[v] = nw;
    }
    long long deg = re - rs;
    if (kDirected) deg = nw ? g.row_off[v + 1] - g.row_off[v] : 0;  // (what the next push costs: out-entries)
    ms_record<L>(s, in, v, nw, deg, acc);
  }
  ms_finish(s, acc, s_tot, false);
}

__global__ __launch_bounds__(kMsBlock) void ms_clear_kernel(word_t* words, const vid_t* list, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kMsBlock + threadIdx.x; i < n; i += stride) words[list[i]] = 0ull;
}

__global__ __launch_bounds__(kMsBlock) void ms_push_kernel(MsPushArgs a) {
  const MsState& s = a.s;
  const ShardView& g = s.g;
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kMsBlock + (threadIdx.x & ~(kWave - 1)); i0 < a.n_active;
       i0 += stride) {
    const int64_t i = i0 + lane;
    const bool in = i < a.n_active;
    word_t f = 0;
    eid_t rs = 0, re = 0;
    if (in) {
      const vid_t v = a.active[i];
      DBFS_DCHECK(static_cast<int64_t>(v) < g.rows, 23, v);
      f = s.front[v];
      s.front[v] = 0ull;  // consumed: the buffer is the level after next's `next`
      rs = g.row_off[v];
      re = g.row_off[v + 1];
    }
    const bool huge = re - rs > kMsPushWave;
    const bool wide = re - rs > kMsPushLane && !huge;
    const eid_t lane_end = wide || huge ? rs : re;
    const unsigned long long hm = __ballot(huge);
    if (hm) {
      const int leader = __ffsll(static_cast<long long>(hm)) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(&s.cursor[2], static_cast<unsigned long long>(__popcll(hm)));
      base = readlane64(base, leader);
      const unsigned long long at = base + mask_rank(hm);
      // (rows this long are at most nnz / kMsPushWave: the queue's capacity)
      if (huge && at < static_cast<unsigned long long>(a.long_cap)) {
        a.long_v[at] = a.active[i];
        a.long_f[at] = f;
      }
    }
    for (eid_t e = rs; __ballot(e < lane_end) != 0ull; ++e) {
      const bool has = e < lane_end;
      ms_push_edge(s, a.touched, has, f, has ? g.col[e] : 0u);
    }
    unsigned long long lm = __ballot(wide);
    while (lm) {
      const int l = __ffsll(static_cast<long long>(lm)) - 1;
      lm &= lm - 1;
      const eid_t b = readlane_i64(rs, l), en = readlane_i64(re, l);
      const word_t fl = readlane64(f, l);
      for (eid_t e = b; e < en; e += kWave) {
        const bool has = e + lane < en;
        ms_push_edge(s, a.touched, has, fl, has ? g.col[e + lane] : 0u);
      }
    }
  }
}

// The rows ms_push_kernel queued: every workgroup walks every queued row, its
// share of each (256 entries per step and workgroup).  Meant for the levels
// the direction rule pushes: few active vertices, hubs among them.
__global__ __launch_bounds__(kMsBlock) void ms_push_long_kernel(MsPushArgs a) {
  const MsState& s = a.s;
  const ShardView& g = s.g;
  const int lane = lane_id();
  // (re-zeroed by the settle that follows)
  const int64_t nq = min(static_cast<int64_t>(__hip_atomic_load(&s.cursor[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)),
                         a.long_cap);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t q = 0; q < nq; ++q) {
    const vid_t v = a.long_v[q];
    const word_t f = a.long_f[q];
    const eid_t re = g.row_off[v + 1];
    // (row q's chunks start at another workgroup for every q: a row of a few
    // chunks keeps a few workgroups busy, and they are different ones per row)
    const int64_t first = static_cast<int64_t>((blockIdx.x + gridDim.x - static_cast<unsigned>((q * 37) % gridDim.x)) % gridDim.x);
    for (eid_t e0 = g.row_off[v] + first * kMsBlock + (threadIdx.x & ~(kWave - 1)); e0 < re; e0 += stride) {
      const bool has = e0 + lane < re;
      ms_push_edge(s, a.touched, has, f, has ? g.col[e0 + lane] : 0u);
    }
  }
}

template <class L>
__global__ __launch_bounds__(kMsBlock) void ms_settle_kernel(MsSettleArgs a) {
  __shared__ unsigned long long s_tot[kMsStats];
  const MsState& s = a.s;
  const ShardView& g = s.g;
  const int t = threadIdx.x;
  const int lane = lane_id();
  if (t < kMsStats) s_tot[t] = 0ull;
  __syncthreads();
  // (read by every workgroup before its ticket; re-zeroed by the last one)
  const int64_t n = min(static_cast<int64_t>(__hip_atomic_load(&s.cursor[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)),
                        a.max_touched);
  MsAcc acc;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kMsBlock + (t & ~(kWave - 1)); i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool in = i < n;
    int64_t w = 0;
    word_t nw = 0;
    long long deg = 0;
    if (in) {
      w = a.touched[i];
      const word_t sv = s.seen[w];
      nw = s.next[w] & ~sv;
      s.seen[w] = sv | nw;
      s.next[w] = nw;
      deg = g.row_off[w + 1] - g.row_off[w];
    }
    ms_record<L>(s, in, w, nw, deg, acc);
  }
  ms_finish(s, acc, s_tot, true);
}

__global__ __launch_bounds__(kMsBlock) void ms_degree_kernel(MsDegreeArgs a) {
  __shared__ unsigned long long s_sum[kMsSources];
  const ShardView& g = a.g;
  const int t = threadIdx.x;
  const int lane = lane_id();
  if (t < kMsSources) s_sum[t] = 0ull;
  __syncthreads();
  long long mine = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMsBlock;
  for (int64_t v0 = static_cast<int64_t>(blockIdx.x) * kMsBlock + (t & ~(kWave - 1)); v0 < g.rows; v0 += stride) {
    const int64_t v = v0 + lane;
    word_t sv = 0;
    long long deg = 0;
    if (v < g.rows) {
      deg = g.row_off[v + 1] - g.row_off[v];
      sv = deg ? a.seen[v] : 0ull;
    }
    word_t uni = uniform64(wave_or(sv));
    while (uni) {
      const int src = __ffsll(static_cast<long long>(uni)) - 1;
      uni &= uni - 1;
      const long long d = wave_sum(((sv >> src) & 1ull) ? deg : 0);
      if (lane == src) mine += d;
    }
  }
  if (mine) atomicAdd(&s_sum[lane], static_cast<unsigned long long>(mine));
  __syncthreads();
  if (t < kMsSources && s_sum[t])
    atomicAdd(reinterpret_cast<unsigned long long*>(a.deg_sum) + t, s_sum[t]);
}

// ms_check (backend.hpp MsCheckArgs): a wave per owned vertex u, striding over
// the rows; lane s is source s and holds lvl[u][s] (the vertex's line of the
// level matrix) against the lvl[w][s] of every entry w that ms_walk_row hands
// over, all sources at once.  Rows are walked in stored order, so the parent
// form's first parent is the host loops' first.
// Workgroups at most (they stride over the rows): 2048 x 4 waves = 8192 waves, the 256 CUs x 4 SIMDs
// x 8 waves the kernel's registers allow (profiles/ms_bfs_regs.txt) when the workgroups spread evenly
// over the CUs; not tuned against other sizes.
constexpr int kMsCheckGrid = 2048;

// kDirected: g is the in-edge view, lane s holds lvl[v][s] of the row's vertex
// v and every entry is a u with a stored u -> v: cross = u reached and v not,
// gap = both reached and lvl[v] > lvl[u] + 1 (MsCheckArgs).
template <class L, bool kCount, bool kParent, bool kDirected>
__global__ __launch_bounds__(kMsBlock) void ms_check_kernel(MsCheckArgs a) {
  __shared__ unsigned long long s_cnt[kMsSources * kMsCheckCounters];
  const ShardView& g = a.g;
  const L* __restrict__ lvl = static_cast<const L*>(a.m.lvl);
  constexpr int kNone = ms_unreached<L>();
  const int t = threadIdx.x;
  const int lane = lane_id();
  if (kCount) {
    if (t < kMsSources * kMsCheckCounters) s_cnt[t] = 0ull;
    __syncthreads();
  }
  const bool on = (a.m.batch_mask >> lane) & 1ull;  // lanes past the pass's sources count and store nothing
  const int64_t my_src = on ? a.m.src[lane] : -1;
  unsigned long long gap = 0, cross = 0, orphan = 0;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (kMsBlock / kWave);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kMsBlock / kWave) + wave; r < g.rows; r += stride) {
    const int64_t u = g.lo + r;
    const eid_t rs = g.row_off[r], re = g.row_off[r + 1];
    DBFS_DCHECK(rs >= 0 && rs <= re && re <= g.nnz, 24, r);
    DBFS_DCHECK(u < a.m.lvl_rows, 25, u);
    const int lu = lvl[u * kMsSources + lane];
    const bool ru = on && lu != kNone;
    const bool is_src = u == my_src;
    bool has_par = false;
    uint32_t par = kMsNoParent;
    // parents only: a row is walked while some lane still looks for its parent
    if (kCount || __ballot(ru && !is_src) != 0ull)
      ms_walk_row<L, kMsWalkAhead>(lvl, g.col, rs, re, a.m.lvl_rows, 26, [&](int valid, const vid_t* w, const int* lw) {
#pragma unroll
        for (int i = 0; i < kMsWalkAhead; ++i) {
          // (&, not &&: a branch on the wave-uniform `in` would take the entry's level load along)
          const bool in = i < valid;
          const bool rw = lw[i] != kNone;
          if (kCount) {
            const int d = lu - lw[i];
            if (kDirected) {
              cross += in & on & rw & !ru;
              gap += in & ru & rw & (d > 1);
            } else {
              cross += in & on & (ru != rw);
              gap += in & ru & rw & ((d > 1) | (d < -1));
            }
          }
          const bool found = in & ru & rw & (lw[i] + 1 == lu) & !has_par;
          par = found ? w[i] : par;
          has_par |= found;
        }
        return kCount || __ballot(ru && !is_src && !has_par) != 0ull;
      });
    if (kCount && (is_src ? lu != 0 : (ru && !has_par))) ++orphan;
    if (kParent && on) a.par[r * kMsSources + lane] = is_src ? static_cast<uint32_t>(u) : par;
  }
  if (kCount) {
    if (gap) atomicAdd(&s_cnt[kMsCheckCounters * lane + 0], gap);
    if (cross) atomicAdd(&s_cnt[kMsCheckCounters * lane + 1], cross);
    if (orphan) atomicAdd(&s_cnt[kMsCheckCounters * lane + 2], orphan);
    __syncthreads();
    if (t < kMsSources * kMsCheckCounters && s_cnt[t])
      atomicAdd(reinterpret_cast<unsigned long long*>(a.out) + t, s_cnt[t]);
  }
}

template <class L, bool kDirected>
void ms_check_launch(const MsCheckArgs& a, hipStream_t st) {
  const unsigned grid = grid_for(a.g.rows, kMsBlock / kWave, kMsCheckGrid);
  if (a.out && a.par) ms_check_kernel<L, true, true, kDirected><<<grid, kMsBlock, 0, st>>>(a);
  else if (a.out) ms_check_kernel<L, true, false, kDirected><<<grid, kMsBlock, 0, st>>>(a);
  else ms_check_kernel<L, false, true, kDirected><<<grid, kMsBlock, 0, st>>>(a);
}

void ms_check(const MsCheckArgs& a, hipStream_t st) {
  if (a.g.rows <= 0 || (!a.out && !a.par)) return;
  ms_level_type(a.m.lvl_bytes, [&](auto l) {
    using L = decltype(l);
    if (a.directed) ms_check_launch<L, true>(a, st);
    else ms_check_launch<L, false>(a, st);
  });
}

unsigned long long take_check_ms() { return take_check_local(); }
void inject_check_ms(hipStream_t st) { inject_check_local(st); }
const bool kCheckedMs = kCheckedLocal;

void ms_init(const MsInitArgs& a, hipStream_t st) {
  ms_level_type(a.s.lvl_bytes, [&](auto l) { ms_init_kernel<decltype(l)><<<1, kWave, 0, st>>>(a); });
}

void ms_pull(const MsPullArgs& a, hipStream_t st) {
  const unsigned grid = grid_for(a.s.g.rows, kMsBlock, kMsMaxGrid);
  ms_level_type(a.s.lvl_bytes, [&](auto l) {
    using L = decltype(l);
    if (a.s.directed) ms_pull_kernel<L, true><<<grid, kMsBlock, 0, st>>>(a);
    else ms_pull_kernel<L, false><<<grid, kMsBlock, 0, st>>>(a);
  });
}

void ms_push(const MsPushArgs& a, hipStream_t st) {
  if (a.clear_n > 0)
    ms_clear_kernel<<<grid_for(a.clear_n, kMsBlock, kMsMaxGrid), kMsBlock, 0, st>>>(a.s.next, a.clear_list, a.clear_n);
  ms_push_kernel<<<grid_for(a.n_active, kMsBlock, kMsMaxGrid), kMsBlock, 0, st>>>(a);
  // (no row of the level can be that long otherwise)
  if (a.active_edges > kMsPushWave)
    ms_push_long_kernel<<<grid_for(a.active_edges, 4 * kMsBlock, kMsMaxGrid), kMsBlock, 0, st>>>(a);
}

void ms_settle(const MsSettleArgs& a, hipStream_t st) {
  const unsigned grid = grid_for(a.max_touched, kMsBlock, kMsMaxGrid);
  ms_level_type(a.s.lvl_bytes, [&](auto l) { ms_settle_kernel<decltype(l)><<<grid, kMsBlock, 0, st>>>(a); });
}

void ms_degree_sums(const MsDegreeArgs& a, hipStream_t st) {
  ms_degree_kernel<<<grid_for(a.g.rows, kMsBlock, kMsMaxGrid), kMsBlock, 0, st>>>(a);
}

}  // namespace kern
}  // namespace dbfs
