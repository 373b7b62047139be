// The row walk of the kernels that read a finished pass's level matrix
// (backend.hpp MsPassMatrix): ms_check_kernel and the betweenness sweeps.
#pragma once

#include "kernel_common.hpp"

namespace dbfs {
namespace kern {
namespace {

// Level lines requested before the first is consumed.
constexpr int kMsWalkAhead = 8;

// One wave walks the entries [rs, re) of a row of `col`; lane s is source s.
// The row is read 64 column ids per step (lane i: col[e + i], coalesced), and
// for each of them, made wave-uniform by a readlane, lane s loads lvl[w][s]:
// one scattered 64-B line (128 B with 16-bit levels) per adjacency entry.  The
// walk is bound by the latency of those lines, so kAhead of them are requested
// before the first is consumed (the last group of a row repeats its last
// entry's line instead of branching around the loads).  Every group goes to
// visit(valid, w, lw): its first `valid` entries (1 .. kAhead, wave-uniform)
// are the row's next ones in stored order, w[i] the column id and lw[i] this
// lane's level of it; false ends the walk.  check_code: the checked build's
// code for a column id past lvl_rows.
template <class L, int kAhead, class Visit>
__device__ __forceinline__ void ms_walk_row(const L* __restrict__ lvl, const vid_t* __restrict__ col, eid_t rs,
                                            eid_t re, int64_t lvl_rows, int check_code, Visit&& visit) {
  const int lane = lane_id();
  for (eid_t e = rs; e < re; e += kWave) {
    const int cnt = static_cast<int>(min(static_cast<eid_t>(kWave), re - e));
    const vid_t mine = lane < cnt ? col[e + lane] : 0u;
    DBFS_DCHECK(static_cast<int64_t>(mine) < lvl_rows, check_code, mine);
    for (int j = 0; j < cnt; j += kAhead) {
      vid_t w[kAhead];
      int lw[kAhead];
#pragma unroll
      for (int i = 0; i < kAhead; ++i) {
        w[i] = static_cast<vid_t>(__builtin_amdgcn_readlane(static_cast<int>(mine), min(j + i, cnt - 1)));
        lw[i] = lvl[static_cast<int64_t>(w[i]) * kMsSources + lane];
      }
      if (!visit(min(kAhead, cnt - j), w, lw)) return;
    }
  }
}

}  // namespace
}  // namespace kern
}  // namespace dbfs
