// Device helpers shared by the kernels that settle a new frontier and finish
// its level in their last workgroup: the frontier update (bfs_kernels.hip) and
// the binned level's apply (td_kernels.hip).  A unit's new vertices (levels,
// unit statistics), the per-workgroup totals slots with the two-level ticket,
// and the folded unit scan.  Anonymous namespace: a copy per kernel file, as
// kernel_common.hpp.
#pragma once

#include "kernel_common.hpp"

namespace dbfs {
namespace kern {
namespace {

// A unit's statistics; write-through when the fused finish's last workgroup
// scans them (fold: read there with agent-scope loads).
__device__ __forceinline__ void store_unit_stats(int64_t* unit_cnt, int64_t* unit_deg, bool fold, int64_t unit,
                                                 long long c, long long d) {
  if (fold) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(unit_cnt + unit), static_cast<unsigned long long>(c),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(unit_deg + unit), static_cast<unsigned long long>(d),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    unit_cnt[unit] = c;
    unit_deg[unit] = d;
  }
}

// New vertices of a wave's words, 64 per step (one per lane, whatever word
// they sit in): a sparse level has about one new vertex per word, and one word
// per step would cost a dependent row_off round trip per new vertex.  Lane l
// holds the new bits `nb` of word l of the words that start at vertex v0;
// every new vertex's level is stored (store_level) and (cnt, deg) return the
// wave's count / degree sum of the new vertices with a non-empty row.
// Wave-uniform call.
// (Measured in the binned apply, whose 16 waves per CU each walk several
// units: 2 / 4 / 8 new vertices per lane and step, their row_off loads in
// flight together, change nothing -- the apply of RMAT-26's 28 M-edge level
// 177-180 us with each; the row_off lines, 8 bytes a vertex over most of the
// array once a level finds a sixth of the vertices, are what it waits for:
// profiles/binned_settle_apply.txt.)
__device__ __forceinline__ void settle_new_vertices(const eid_t* __restrict__ ro, const LevelOut& out,
                                                    bool store_level, int64_t v0, word_t nb, long long& cnt,
                                                    long long& deg) {
  const int lane = lane_id();
  cnt = 0;
  deg = 0;
  const int incl = static_cast<int>(wave_incl_scan(__popcll(nb)));
  const int total = __builtin_amdgcn_readlane(incl, kWave - 1);
  for (int base = 0; base < total; base += kWave) {
    const int idx = base + lane;
    const int pos = wave_set_position(nb, incl, idx);
    if (idx < total) {
      const int64_t v = v0 + pos;
      if (store_level) out.store(v);
      const eid_t d = ro[v + 1] - ro[v];
      if (d > 0) {
        cnt += 1;
        deg += d;
      }
    }
  }
  cnt = wave_sum(cnt);
  deg = wave_sum(deg);
}

// The fused finish's unit prefixes (fold_scan; every thread of the last
// workgroup of kThreads threads): unit_cnt / unit_deg become the exclusive
// prefixes over all units (at most kFoldScanUnits) and the chunk prefixes
// part_cnt / part_deg zero -- what scan_units_kernel leaves for the
// compaction.  The units are spread over all kThreads threads (a run of
// ceil(nunits / kThreads) each) and a run's agent-scope loads go out kFoldRun
// at a time: each batch is one round trip to memory (the stats were stored
// write-through by other XCDs' waves), so a run of up to kFoldRun units -- 2048
// units, a 2^23-vertex shard, on 256 threads -- costs one round trip, its
// values kept in registers for the second pass.  (The first version gave each
// thread a run of kFoldScanUnits / kBlock units, four loads in flight: on a
// 2048-unit shard one wave made 16 dependent round trips -- the P = 8
// post-bottom-up update 39.4 -> 33.8 us, RMAT-22 top-down only +2 %,
// profiles/r5_fold_scan_ab.txt.)
__device__ __forceinline__ long long agent_load_i64(const int64_t* p) {
  return static_cast<long long>(
      __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
constexpr int kFoldRun = 8;
template <int kThreads>
__device__ __forceinline__ void fold_unit_scan(const ScanArgs& a) {
  __shared__ long long s_fc[kThreads / kWave], s_fd[kThreads / kWave];
  const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
  const int64_t n = a.nunits;
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t u0 = min(static_cast<int64_t>(t) * per, n);
  const int64_t u1 = min(u0 + per, n);
  long long c[kFoldRun], d[kFoldRun];
  long long sc = 0, sd = 0;
  for (int64_t b = u0; b < u1; b += kFoldRun) {
#pragma unroll
    for (int k = 0; k < kFoldRun; ++k) {
      const bool in = b + k < u1;
      c[k] = in ? agent_load_i64(a.unit_cnt + b + k) : 0ll;
      d[k] = in ? agent_load_i64(a.unit_deg + b + k) : 0ll;
    }
#pragma unroll
    for (int k = 0; k < kFoldRun; ++k) {
      sc += c[k];
      sd += d[k];
    }
  }
  const long long ic = wave_incl_scan(sc), id = wave_incl_scan(sd);
  __syncthreads();  // (s_fc / s_fd: the caller's earlier LDS use is done)
  if (lane == kWave - 1) {
    s_fc[wv] = ic;
    s_fd[wv] = id;
  }
  __syncthreads();
  long long oc = ic - sc, od = id - sd;
  for (int k = 0; k < wv; ++k) {
    oc += s_fc[k];
    od += s_fd[k];
  }
  for (int64_t b = u0; b < u1; b += kFoldRun) {
    if (per > kFoldRun) {
      // (a longer run: the batch again -- the registers hold the last one)
#pragma unroll
      for (int k = 0; k < kFoldRun; ++k) {
        const bool in = b + k < u1;
        c[k] = in ? agent_load_i64(a.unit_cnt + b + k) : 0ll;
        d[k] = in ? agent_load_i64(a.unit_deg + b + k) : 0ll;
      }
    }
#pragma unroll
    for (int k = 0; k < kFoldRun; ++k) {
      if (b + k < u1) {
        a.unit_cnt[b + k] = oc;
        a.unit_deg[b + k] = od;
      }
      oc += c[k];
      od += d[k];
    }
  }
  for (int64_t p = t; p * kScanChunk < a.nunits; p += kThreads) {
    a.part_cnt[p] = 0;
    a.part_deg[p] = 0;
  }
}

// Fused finish of a level settled by a grid of kThreads-thread workgroups
// (every thread of every workgroup calls it once, after its last unit; the
// grid holds at most kMaxFusedGrid workgroups and none returns before it):
// the waves' totals (wc, wd) summed into the workgroup's slot of `tot`
// (write-through), a two-level ticket (group_ticket: kFusedGroup workgroups
// share one, its last arriver sums the group's slots into tot[2 kMaxFusedGrid
// + 2 g] and takes the level ticket scan.ticket), and the level's last
// workgroup sums the groups and runs scan_finish (totals, decision, stamp) and,
// with fold_scan, the unit prefixes.  True in that last workgroup, (tc, td)
// then hold the level's totals.
// (The unit statistics the last workgroup scans with fold_scan were stored by
// lane 0 of every wave, and a barrier does not wait for another wave's
// stores: each wave drains its own first.)
template <int kThreads>
__device__ __forceinline__ bool fused_finish(int64_t* tot, unsigned* group_ticket, const ScanArgs& scan,
                                             bool fold_scan, long long wc, long long wd, long long& tc,
                                             long long& td) {
  constexpr int kWaves = kThreads / kWave;
  __shared__ long long s_c[kWaves], s_d[kWaves];
  __shared__ int s_last, s_level_last;  // (separate: waves read s_last while wave 0 decides the level)
  const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));  // (wave-uniform)
  if (lane_id() == 0) {
    s_c[wv] = wc;
    s_d[wv] = wd;
  }
  if (fold_scan) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    long long c = 0, d = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      c += s_c[k];
      d += s_d[k];
    }
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(tot + 2 * blockIdx.x), static_cast<unsigned long long>(c),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(tot + 2 * blockIdx.x + 1),
                       static_cast<unsigned long long>(d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the group's last workgroup sums the group (below), then takes the
    // level ticket
    const unsigned grp = blockIdx.x / kFusedGroup;
    const unsigned gsz = min(static_cast<unsigned>(kFusedGroup), gridDim.x - grp * kFusedGroup);
    const unsigned prev = atomicAdd(group_ticket + grp * kBuQueueStride, 1u);
    s_last = prev == gsz - 1;
    if (s_last) {
      atomicExch(group_ticket + grp * kBuQueueStride, 0u);
      last_arriver_acquire();
    }
  }
  __syncthreads();
  if (!s_last) return false;
  auto slot_sum = [&](const int64_t* slots, unsigned first, unsigned n, long long& c, long long& d) {
    c = 0;
    d = 0;
    for (unsigned g = threadIdx.x; g < n; g += kThreads) {
      c += static_cast<long long>(__hip_atomic_load(reinterpret_cast<const unsigned long long*>(slots + 2 * (first + g)),
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      d += static_cast<long long>(__hip_atomic_load(
          reinterpret_cast<const unsigned long long*>(slots + 2 * (first + g) + 1), __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT));
    }
  };
  long long c = 0, d = 0;
  // group total (kFusedGroup slots: the first wave), then the level ticket
  const unsigned grp = blockIdx.x / kFusedGroup;
  const unsigned ngroups = (gridDim.x + kFusedGroup - 1) / kFusedGroup;
  if (wv == 0) {
    slot_sum(tot, grp * kFusedGroup, min(static_cast<unsigned>(kFusedGroup), gridDim.x - grp * kFusedGroup), c, d);
    c = wave_sum(c);
    d = wave_sum(d);
    if (lane_id() == 0) {
      int64_t* gt = tot + 2 * kMaxFusedGrid;
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(gt + 2 * grp), static_cast<unsigned long long>(c),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(gt + 2 * grp + 1), static_cast<unsigned long long>(d),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned prev = atomicAdd(scan.ticket, 1u);
      s_level_last = prev == ngroups - 1;
      if (s_level_last) last_arriver_acquire();
    }
  }
  __syncthreads();
  if (!s_level_last) return false;
  slot_sum(tot + 2 * kMaxFusedGrid, 0, ngroups, c, d);
  c = wave_sum(c);
  d = wave_sum(d);
  __syncthreads();  // (s_c / s_d reused)
  if (lane_id() == 0) {
    s_c[wv] = c;
    s_d[wv] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long sc = 0, sd = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      sc += s_c[k];
      sd += s_d[k];
    }
    scan_finish(scan, sc, sd);
    s_c[0] = sc;
    s_d[0] = sd;
  }
  if (fold_scan) fold_unit_scan<kThreads>(scan);
  __syncthreads();
  tc = s_c[0];
  td = s_d[0];
  return true;
}

}  // namespace
}  // namespace kern
}  // namespace dbfs
