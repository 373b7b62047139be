// Device abstraction the BFS engine is written against.
//
// Two implementations:
//   HipBackend  -- hand-written gfx950 HIP kernels on one HIP stream (the
//                  production path; csrc/backend/hip_backend.hip,
//                  csrc/kernels/*.hip).
//   CpuBackend  -- straightforward host loops with the identical semantics,
//                  used by the CPU test-suite (gloo multi-process tests) and
//                  the `--cpu` CLI path (csrc/backend/cpu_backend.cpp).
//
// Every primitive is asynchronous with respect to the host on the backend's
// stream (CpuBackend executes eagerly).  The reference has no such layer: its
// kernels take raw pointers pulled out of __managed__ tables (bfs.cu:252-269,
// 580-585).
#pragma once

#include <atomic>
#include <cstddef>
#include <functional>
#include <memory>
#include <string>
#include <utility>

#include "dbfs/common.hpp"
#include "dbfs/rmat.hpp"
#include "dbfs/wide.hpp"

namespace dbfs {

enum class DeviceKind { CPU, HIP };

// Device-checked build: the kernel files that record bounds violations, each
// in a word of its own (the codes of two files may coincide: a violation is
// reported with its file).
enum class CheckFile { Bfs, Td, Bu, Ms, MsBc, Cc, Graph, Scc, Ecc };
constexpr int kCheckFiles = 9;
inline const char* check_file_name(CheckFile f) {
  constexpr const char* names[kCheckFiles] = {"bfs_kernels", "td_kernels",  "bu_kernels",   "ms_kernels",
                                              "ms_bc_kernels", "cc_kernels", "graph_kernels", "scc_kernels",
                                              "ecc_kernels"};
  return names[static_cast<int>(f)];
}

// ---- kernel argument blocks -------------------------------------------------

// Local CSR shard: rows [lo, lo + rows) of an n-vertex graph, global column ids.
// Packed row record of the non-empty-row view (ShardView::nz_rec).
struct alignas(8) NzRec {
  uint32_t off;   // row start - unit_base[unit]
  vid_t head;     // the row's head (hub-encoded like ShardView::head)
};

struct ShardView {
  const eid_t* row_off = nullptr;  // rows + 1 (local)
  const vid_t* col = nullptr;      // row_off[rows]
  int64_t n = 0, lo = 0, rows = 0, nnz = 0;
  // Per-row copy of the first neighbour (col[row_off[r]]; any value for empty
  // rows), laid out per vertex so a wave's 64 first probes are one coalesced
  // 256-B load instead of 64 scattered col[] lines.  Every DeviceGraph builds
  // it; bu_step requires it.
  const vid_t* head = nullptr;
  // Hub-encoded heads (nhubs > 0): the nhubs highest-degree vertices of the
  // whole graph get compact indices; head[r] = kHubFlag | index when the row's
  // first neighbour is a hub (hub_vertex[index] = its vertex id), else the
  // vertex id.  Bottom-up keeps the hubs' frontier bits in LDS.
  const vid_t* hub_vertex = nullptr;
  int64_t nhubs = 0;
  // Hub-encoded copy of col (same layout; hub neighbours as kHubFlag | index),
  // read by bottom-up so that probes of hub neighbours hit LDS too.
  const vid_t* hub_col = nullptr;
  // Non-empty-row view, built with the heads and required by bu_step: the
  // bottom-up kernels take every row's bounds and head from it or from the
  // records below, never from row_off / col (Graph500 RMAT: about half the
  // vertices have no edges).  nz_pref[w] = number of non-empty rows before
  // bitmap word w, nz_row_off / nz_head = row_off / head of the non-empty rows
  // only (dense, so a bottom-up wave touches half the cache lines).  Row k of
  // the view is [nz_row_off[k], nz_row_off[k + 1]).
  const eid_t* nz_pref = nullptr;
  const eid_t* nz_row_off = nullptr;
  const vid_t* nz_head = nullptr;
  // Packed non-empty-row records (optional, with the view): nz_rec[k] = {row
  // start relative to unit_base[U], head} for row k of unit U (4096
  // vertices); row k ends where row k + 1 starts, or at unit_base[U + 1] for
  // the unit's last non-empty row.  8 bytes per row instead of the view's
  // 8-byte offset + 4-byte head; present when every unit spans < 2^32 edges.
  const struct NzRec* nz_rec = nullptr;
  // Way back from a record to its vertex (present exactly when nz_rec is):
  // nz_loc[k] = position (0..4095) of row k's vertex inside its unit, so row
  // k of unit U is vertex 4096 U + nz_loc[k].  2 bytes per non-empty row; a
  // static property of the graph.  The bottom-up kernels' record-order walk
  // reads a unit's records [nz_pref[64 U], nz_pref[64 U + 64]) in order with
  // it, instead of ranking each unvisited vertex among the unit's rows.
  const uint16_t* nz_loc = nullptr;
  const eid_t* unit_base = nullptr;  // ceil(rows / 4096) + 1 entries: row_off of each unit's first vertex
  // Top-down copy of col (same layout, neighbour-id order) with the
  // td_nhubs highest-degree vertices encoded as kHubFlag | index
  // (td_hub_vertex[index] = the vertex): a large top-down level tests them in
  // an LDS copy of their visited bits and reads no visited word for them.
  const vid_t* td_col = nullptr;
  const vid_t* td_hub_vertex = nullptr;
  int64_t td_nhubs = 0;
  // Hubs present: bit v set when global vertex v is a hub (the hubs are every
  // vertex of degree >= the hub threshold, so a hub-first row's hubs are a
  // prefix of it).  The array covers every rank's slice (global words: an
  // owned word w is read at cut_word_off + w).  Read by the hub-cut bottom-up
  // level (BuArgs::cut_edges), on one rank and on several.
  const word_t* hub_bits = nullptr;
  // Degree of every hub (nhubs entries; several ranks: a hub's row lives on
  // its owner, so the hub-cut decision sums these instead of row lengths).
  const uint32_t* hub_deg = nullptr;
};

// At most kTdMaxHubs top-down hubs (their visited bits, 8 KiB, sit in LDS
// next to the top-down owner map: five 256-thread workgroups per CU).
// Measured (RMAT-22 top-down only, hub marks on): 2^13 / 2^14 / 2^15 / 2^16
// / 2^17 / 2^18 hubs: 60 / 62 / 71 / 77 / 69 / 60 GTEPS.
#ifndef DBFS_TD_MAX_HUBS_LOG2
#define DBFS_TD_MAX_HUBS_LOG2 16
#endif
constexpr int64_t kTdMaxHubs = int64_t(1) << DBFS_TD_MAX_HUBS_LOG2;

// At most kMaxHubs hubs: their frontier bitmap (64 KiB) is staged in LDS by
// every bottom-up workgroup (two 1024-thread workgroups per CU fit in 160 KiB).
// (2^19 - 2^12: the 512 B below 64 KiB leave room for a 64-entry deferred-scan
// queue per wave next to the hub bits in two workgroups' LDS, see bu_hub_kernel)
#ifndef DBFS_MAX_HUBS
#define DBFS_MAX_HUBS ((int64_t(1) << 19) - (int64_t(1) << 12))
#endif
constexpr int64_t kMaxHubs = DBFS_MAX_HUBS;
constexpr vid_t kHubFlag = 0x80000000u;
// Rows of up to kSortedRowMax entries are sorted hub-first (neighbour degree
// descending, graph_sort); longer ones (a handful of hubs) keep their order.
constexpr int kSortedRowMax = 4096;
// Narrow (8-bit) level arrays: 0xFF = unreached, levels 0 .. 254.
constexpr uint8_t kNarrowUnreached = 0xFF;
// One-byte levels are stored as base + level, base = 64 x (run number mod
// kNarrowEpochs): a byte outside [base, base + kNarrowMaxLevel] reads as
// unreached, so the array is refilled with 0xFF only every kNarrowEpochs runs
// (base + 63 marks a level too deep for the narrow array: the traversal is
// repeated with 32-bit levels).
constexpr int kNarrowMaxLevel = 62;
constexpr int kNarrowEpochs = 4;

// Frontier bookkeeping is organised in "units" of 64 bitmap words (4096
// vertices): one 256-thread workgroup (4 waves) per unit, 16 consecutive words
// per wave64, in the HIP kernels.  (One wave per word would launch 1M waves for
// RMAT-26: dispatch alone then costs ~300 us per kernel on MI355X.)  Per-unit
// counts are scanned by a multi-block scan whose chunks hold kScanChunk units.
constexpr int kWaveWords = 16;
constexpr int kUnitWaves = 4;
constexpr int kUnitWords = kWaveWords * kUnitWaves;
constexpr int kUnitVertices = kUnitWords * kWordBits;
constexpr int kScanChunk = 1024;
// At most this many units are prefix-scanned by a fused finish's last
// workgroup (UpdateArgs::fold_scan): 32 per thread of a 256-thread workgroup.
constexpr int kFoldScanUnits = 8192;
// A shard of fewer units than this: the frontier update and the compaction
// run a unit per workgroup, 16 words per wave (update_unit_split,
// compact_split) -- 4x the waves, a quarter of the dependent row_off steps
// each; from this many units on, a unit per wave.
constexpr int64_t kUpdateSplitUnits = 4096;
// Top-down expansion handles kTdEdgesPerBlock frontier edges per workgroup.
constexpr int kTdThreads = 256;
constexpr int kTdItems = 8;
constexpr int kTdEdgesPerBlock = kTdThreads * kTdItems;

// ---- device-driven level loop (one rank) -------------------------------------
// The host enqueues level L+1 before level L has finished; every kernel of a
// level reads this block at entry and returns at once when the level is not
// its direction (or the traversal is done).  The scan's last workgroup turns
// the new frontier's totals into the next level's decision (level_ctrl_finish,
// the same Beamer switch as the host loop), so no per-level host round trip
// (~19 us of idle GPU on MI355X: D2H, host wake-up, next launch) remains.
struct LevelCtrl {
  // configuration (written once per run)
  int32_t mode = 2;             // 0 top-down only, 1 bottom-up only, 2 direction-optimising
  int32_t pad0 = 0;
  double alpha = 24.0, beta = 96.0;
  double n = 0.0, total_directed = 0.0;
  double td_byte_edges = 0.0, check_visited_min = 0.0;
  // state after the last finished level
  int32_t dir = 'T';            // direction of the next level
  int32_t bytes = 0;            // next top-down level writes the byte map
  int32_t check_visited = 1;    // ... with the visited pre-check
  int32_t done = 0;             // frontier empty: every later kernel returns
  int64_t n_f = 0, m_f = 0, prev_nf = 0, vis_deg = 0;
  int64_t reached = 0;          // vertices with degree > 0 reached so far (counts summed)
  // device wall clock (Backend::wall_clock_khz) when the running level's
  // first kernel started
  uint64_t t_start = 0;
  // Vertices with degree > 0 in the whole graph (configuration; 0: unknown --
  // directed graphs).  Once every one of them is reached no edge can discover
  // anything: the traversal is done without expanding its last frontier.
  int64_t n_active = 0;
};

// One record per finished level (device array; read after the run).
struct LevelRecDev {
  int32_t dir = 0, pad = 0;
  int64_t n_f = 0, m_f = 0, discovered = 0;
  uint64_t t0 = 0, t1 = 0;  // device wall clock: first kernel started, scan finished
};

// Host-visible mailbox slot (pinned, device-mapped), written by the scan's
// last workgroup of level L into slot L % kMailboxSlots.
struct LevelMailbox {
  int32_t level = -2;           // level that wrote this slot
  int32_t done = 0;
  int64_t vis_deg = 0;
  int32_t next_dir = 0;         // direction decided for the following level
  int32_t pad = 0;
  int64_t n_f = 0, m_f = 0;     // the following level's frontier (vertices, edges)
  int64_t reached = 0;          // LevelCtrl::reached
};
constexpr int kMailboxSlots = 8;

// Shared host/device decision logic (also used by the CPU backend).
DBFS_HD void level_ctrl_finish(LevelCtrl& c, int64_t count, int64_t degsum, bool seed, LevelRecDev* rec) {
  if (seed) {
    c.prev_nf = 0;
    c.vis_deg = degsum;
    c.reached = count;
  } else {
    rec->dir = c.dir;
    rec->n_f = c.n_f;
    rec->m_f = c.m_f;
    rec->discovered = count;
    c.prev_nf = c.n_f;
    c.vis_deg += degsum;
    c.reached += count;
  }
  c.n_f = count;
  c.m_f = degsum;
  c.done = count == 0 ? 1 : 0;
  if (!c.done && c.mode == 2) {
    const double m_u = c.total_directed - static_cast<double>(c.vis_deg);
    if (c.dir == 'T' && static_cast<double>(c.m_f) > m_u / c.alpha && c.n_f > c.prev_nf)
      c.dir = 'B';
    else if (c.dir == 'B' && static_cast<double>(c.n_f) < c.n / c.beta && c.n_f < c.prev_nf)
      c.dir = 'T';
  }
  // every vertex with an edge reached: the last frontier's edges can only
  // find visited vertices (levels, reached vertices and edges unchanged)
  if (c.n_active > 0 && c.reached >= c.n_active) c.done = 1;
  c.bytes = (c.dir == 'T' && static_cast<double>(c.m_f) >= c.td_byte_edges) ? 1 : 0;
  c.check_visited = static_cast<double>(c.vis_deg) >= c.check_visited_min * c.total_directed ? 1 : 0;
}

// A device-loop chain's kernels run only when the chain is live: the level is
// not done, its direction is the one the chain was enqueued for, and (sparse
// top-down chains) the global frontier edges are at most the chain's cap.
DBFS_HD bool chain_live(const LevelCtrl& c, int32_t dir, int64_t cap) {
  return !c.done && (dir == 0 || c.dir == dir) && (cap <= 0 || c.m_f <= cap);
}

// What every kernel of a chain tests at entry, built once per chain
// (DeviceLoop::enqueue_level).  No control block: the host loop, always live.
// (Kernels that carry a collective run its part on a no-op chain too.)
struct ChainGuard {
  const LevelCtrl* ctrl = nullptr;
  int32_t dir = 0;   // 'T' / 'B' (0: any)
  int64_t cap = 0;   // live while ctrl->m_f <= cap (0: no bound)
  DBFS_HD bool live() const { return !ctrl || chain_live(*ctrl, dir, cap); }
};

// Where a finished level is stamped (device loop): the control block the
// decision updates, the level's record (not for the seed) and its mailbox slot.
struct LevelStamp {
  LevelCtrl* ctrl = nullptr;
  LevelRecDev* rec = nullptr;
  LevelMailbox* mailbox = nullptr;  // device-mapped pinned slot
  int32_t level = 0;
  bool seed = false;
};

// Where new vertices' levels go (Engine::level_out): the narrow array (one
// byte per vertex, narrow_base + level; kNarrowUnreached = not reached) when
// the run uses one, else the 32-bit array.
struct LevelOut {
  lvl_t* level = nullptr;       // rows
  uint8_t* level8 = nullptr;    // rows, instead of `level` when set
  uint8_t narrow_base = 0;      // narrow level bytes of this run: base + level (kNarrowEpochs)
  lvl_t new_level = 0;
  // the byte of new_level (levels up to kNarrowMaxLevel)
  DBFS_HD uint8_t byte() const { return static_cast<uint8_t>(narrow_base + new_level); }
  // vertex i reached at new_level (uniform branch).  A level too deep for the
  // bytes stores base + kNarrowMaxLevel + 1: the engine reruns such a
  // traversal with wide levels.
  DBFS_HD void store(int64_t i) const {
    if (level8)
      level8[i] = static_cast<uint8_t>(narrow_base + (new_level <= kNarrowMaxLevel ? new_level : kNarrowMaxLevel + 1));
    else
      level[i] = new_level;
  }
};

// Load-balanced top-down work list of a frontier: qscan[i] = exclusive prefix
// of degrees (qscan[entries] = their sum), qbase[i] = row_off[v_i] - qscan[i],
// blk_vstart[b] = index of the entry covering edge b * kTdEdgesPerBlock,
// qv[i] = v_i (local row; optional).  WorkList for the kernels that write one,
// WorkListIn for those that read it.
struct WorkList {
  int64_t* qscan = nullptr;
  int64_t* qbase = nullptr;
  int32_t* blk_vstart = nullptr;
  vid_t* qv = nullptr;
};
struct WorkListIn {
  const int64_t* qscan = nullptr;
  const int64_t* qbase = nullptr;
  const int32_t* blk_vstart = nullptr;
  const vid_t* qv = nullptr;
  WorkListIn() = default;
  WorkListIn(const WorkList& w) : qscan(w.qscan), qbase(w.qbase), blk_vstart(w.blk_vstart), qv(w.qv) {}
};

// Per-run initialisation of the bitmap engine in one pass (replaces a level
// fill, a visited copy, the seed update and its scan: ~8 dependent launches):
//   level[r] = kUnreached (0 for the source), visited = zdeg (+ source bit),
//   frontier (owned slice) = source bit only, and the seed's totals --
//   stats[0..3] = (count, degree sum) of {source} counting degree > 0 only,
//   qscan[count] = degree sum, the source unit's scan offsets = 0 -- exactly
//   what update + scan leave for a one-vertex frontier.  With ctrl, the
//   device-loop state is *ctrl = level_ctrl_finish(ctrl_init, seed) and the
//   mailbox slot of level -1 is stamped.
struct InitRunArgs {
  ShardView g;
  LevelOut out;                    // (new_level 0: the source's)
  bool level8_filled = false;      // out.level8 already holds kNarrowUnreached (prefilled): only the source's byte
  const word_t* zdeg = nullptr;    // global
  word_t* visited = nullptr;       // global
  int64_t gwords = 0;
  word_t* frontier = nullptr;      // owned slice of the seed frontier
  int64_t words = 0;
  int64_t src_local = -1;          // source row on this rank, -1 if not owned
  int64_t vis_word_base = 0;       // global word index of the owned slice
  int64_t* unit_cnt = nullptr;
  int64_t* unit_deg = nullptr;
  int64_t* part_cnt = nullptr;
  int64_t* part_deg = nullptr;
  int64_t* stats = nullptr;
  // The seed's work list: its end marker in qscan always; device loop, with
  // qbase / blk_vstart / qv set: the seed's entry (source vertex, qbase, the
  // edge blocks it covers) so a sparse first level can run without a
  // compaction, and frontier_clear (the first level's output bitmap) zeroed.
  WorkList wl;
  word_t* frontier_clear = nullptr;
  // both owned frontier slices are known zero (the previous traversal ended
  // on a top-down level that found nothing: top-down levels clear their input
  // as they read it and set only new bits): only the seed's word is written
  // (the CPU backend checks the claim)
  bool frontier_clean = false;
  LevelCtrl* ctrl = nullptr;
  LevelCtrl ctrl_init;
  LevelMailbox* mailbox = nullptr;
  // Several ranks, seeded without a collective: every rank's replicated
  // degree array (deg_all, the global source id src_global) gives the seed's
  // global totals, so with ctrl / mailbox set each rank finishes the seed
  // itself -- the source's bit set in its replicated visited bitmap, and
  // (frontier_global, a bottom-up first level) the whole global seed
  // frontier written locally instead of all-gathered.
  const uint32_t* deg_all = nullptr;
  int64_t src_global = -1;
  word_t* frontier_global = nullptr;
};

// Multi-block exclusive scan of unit_cnt / unit_deg (in place, per chunk of
// kScanChunk units) plus chunk prefixes (part_cnt / part_deg, exclusive).  The
// last workgroup to finish (ticket, agent-scope release/acquire) scans the
// chunk totals and writes stats[0..1] = stats[2..3] = (count, degree sum) and
// the work-list end sentinel qscan[count] = degree sum.
struct ScanArgs {
  int64_t* unit_cnt = nullptr;
  int64_t* unit_deg = nullptr;
  int64_t nunits = 0;
  int64_t* part_cnt = nullptr;   // ceil(nunits / kScanChunk)
  int64_t* part_deg = nullptr;
  unsigned* ticket = nullptr;    // zero before the first launch; reset by the last block
  int64_t* stats = nullptr;
  int64_t* qscan = nullptr;
  // device loop: a no-op on a no-op chain; the last workgroup runs
  // level_ctrl_finish and stamps the level
  ChainGuard guard;
  LevelStamp stamp;
  // ... here (one rank); several ranks reduce the totals first and finish in
  // level_finish.
  bool finish = true;
};

// The fused finish of a kernel that settles a level's new frontier (the
// update, the binned apply), as DeviceLoop::fused_finish builds it: what
// UpdateArgs::fold_scan / scan / tot / group_ticket describe.
struct FusedFinishArgs {
  bool fold_scan = false;
  ScanArgs scan;
  int64_t* tot = nullptr;
  unsigned* group_ticket = nullptr;
};

// Device loop, several ranks: after the totals' all-reduce (stats[2..3] =
// global count / degree sum), one thread runs level_ctrl_finish (seed: from
// ctrl_init) and stamps rec / the mailbox, as the one-rank scan does.
struct LevelFinishArgs {
  const int64_t* stats = nullptr;
  LevelCtrl ctrl_init;
  ChainGuard guard;  // (not tested for the seed)
  LevelStamp stamp;
};

// Host-loop statistics mailbox (pinned, device-mapped).  After a level's
// totals are final (scan, plus the all-reduce on several ranks) one tiny
// kernel copies stats[0..3] here with system-scope stores and then writes
// `seq` with release semantics; the host spins on `seq`.  This replaces a
// D2H copy + stream synchronisation per level (a copy-engine round trip and a
// host wake-up) by a store the spinning host sees within a microsecond.
struct StatsMailbox {
  int64_t seq = 0;
  int64_t v[4] = {0, 0, 0, 0};
};

// Owned frontier bitmap -> load-balanced top-down work list (WorkList).
struct CompactArgs {
  ShardView g;
  const word_t* frontier = nullptr;
  int64_t words = 0;
  const int64_t* unit_cnt_off = nullptr;  // scanned (in-chunk) unit offsets
  const int64_t* unit_deg_off = nullptr;
  const int64_t* part_cnt = nullptr;      // chunk prefixes
  const int64_t* part_deg = nullptr;
  WorkList wl;                      // (qv optional)
  word_t* clear = nullptr;          // optional: zero the frontier words once read (== frontier)
  // optional: zero every word of this bitmap (a sparse level after a
  // bottom-up one writes its output into the bottom-up level's input)
  word_t* clear_all = nullptr;
  ChainGuard guard;
};

// Sparse top-down level (device loop, one rank): one kernel instead of
// compact + td_expand + update + scan.  Expands the work list (`in`, totals
// in dev_stats[0..1]) edge-balanced like td_expand,
// claims each new vertex with a fetch-or on `visited`, writes its level, sets
// its bit in frontier_out (clean on entry) and appends it -- wave-aggregated,
// one packed atomic (count << kSparseEdgeBits | edges) per wave, so entries
// stay ordered by edge offset -- to the output work list (`next`) the next
// level expands directly.  The input vertices' bits are
// cleared from frontier_in (keeps the bitmap the next sparse level writes
// clean).  The last workgroup publishes the totals (stats[0..3], next.qscan[q]),
// runs level_ctrl_finish and stamps rec / the mailbox like the scan.
constexpr int kSparseEdgeBits = 36;
// Direct exchanges (peer transport, Comm::direct_lists / direct_level_end):
// the kernels themselves move the data through the peers' windows, no
// exchange launch.  Every signal is a tagged cell of two 64-bit words in the
// receiver's window -- each word carries the exchange's sequence number next
// to its payload, so one write-through store publishes it and one poll both
// observes it and delivers the payload:
//   owner lists  word 0 = seq32 << 32 | count (the ids are in the slot,
//                stored and drained before the cell)
//   level end    word 0 = seq32 << 32 | new vertices (< 2^32 per rank),
//                word 1 = seq24 << 40 | their degree sum (< 2^40 per rank)
// The cells sit in the window's flag page, apart from every other
// collective's payload: a stale cell holds an older sequence number.
constexpr int kMaxDirectRanks = 16;
// Where the data goes and comes from, in device memory (the kernels index it
// with a wave-uniform rank): one table per window parity.
struct DirectTable {
  uint32_t* dst[kMaxDirectRanks];            // rank p's window slot for this rank (ids from word 1; [rank]: unused)
  uint64_t* cell_out[kMaxDirectRanks];       // rank p's cell for this rank ([rank]: unused)
  const uint32_t* src[kMaxDirectRanks];      // this rank's window slot of sender p
  const uint64_t* cell_in[kMaxDirectRanks];  // this rank's cell of sender p ([rank]: unused)
};
// Frontier slices pushed by the kernels that produce them (several ranks,
// peer transport, Comm::direct_frontier): each output word also goes,
// write-through, to every peer's window buffer for this rank's slice
// (dst[p]), and the next level's hub_gather copies the peers' slices from
// this rank's window (src[p]) into its global frontier -- the all-gather
// rides the producing kernel instead of a collective after it.  One table per
// buffer parity (the producing level's parity: a peer writes level L + 2's
// slice only after level L + 1's end, which this rank reaches after it has
// copied level L's); [rank] unused.
struct FrontierTable {
  uint64_t* dst[kMaxDirectRanks];
  const uint64_t* src[kMaxDirectRanks];
};

// A timed-out device wait's error word: the collective's sequence number
// (low 48 bits) and 1 + the peer it found missing (bits 48..55; 0: unknown).
constexpr uint64_t kWaitSeqMask = (uint64_t(1) << 48) - 1;

struct DirectExchange {
  int active = 0;  // 0: the exchange goes through a Comm collective instead
  int nranks = 1, rank = 0;
  uint64_t seq = 0;                     // this exchange's sequence number (the cells' tag)
  const DirectTable* table = nullptr;   // device memory
  uint64_t timeout_ticks = 0;           // a wait gives up after this many wall-clock ticks
  uint64_t* error = nullptr;            // ... and stores kWaitSeqMask & seq | (peer + 1) << 48 here (the host watches it)
  // a level end: the all-reduced totals as recorded (shadow replay) instead
  // of the peers' cells summed
  const int64_t* result = nullptr;
};

// new = (OR_r cand[r * cand_stride + w]) & ~visited[w] over the owned slice
// (force: new = cand, used to seed the source):  visited |= new;
// frontier = new; level[v] = new_level for v in new; unit_cnt[u] / unit_deg[u]
// = count / degree-sum of new vertices with degree > 0.  clear_cand zeroes the
// consumed cand words (single-chunk top-down: keeps `next` clean).
struct UpdateArgs {
  ShardView g;
  word_t* cand = nullptr;
  // Byte-map candidates (one byte per vertex, 0/1) instead of `cand`: used
  // after a byte-map top-down step on one rank; the bytes are cleared.
  uint8_t* cand_bytes = nullptr;
  int nchunks = 1;
  int64_t cand_stride = 0;       // words between chunks
  bool clear_cand = false;
  bool force = false;
  word_t* visited = nullptr;     // owned slice of the global visited bitmap
  word_t* frontier = nullptr;    // owned slice of the NEXT global frontier bitmap
  LevelOut out;
  int64_t words = 0;             // words of the owned slice
  int64_t* unit_cnt = nullptr;   // nunits
  int64_t* unit_deg = nullptr;   // nunits
  // Device loop: reads cand_bytes when guard.ctrl->bytes, else cand (both given).
  ChainGuard guard;
  // With the byte-map levels of TdArgs::level_direct: candidates are the
  // unvisited vertices whose level byte already reads out.byte() (level8,
  // padded to whole words); cand_bytes is not read.
  const uint8_t* level_direct = nullptr;
  // One rank, device loop (as BuArgs::fuse_scan): totals and finish in the
  // last-arriving workgroup, unit statistics left unscanned (a following
  // compaction scans them first); tot[0..1] zero, reset by the last one.
  bool fuse_scan = false;
  // ... and (graphs of at most kFoldScanUnits units) the unit prefixes the
  // next compaction reads, scanned by the same last workgroup -- no
  // scan_units launch between the levels (the unit statistics are stored
  // write-through and read with agent-scope loads, as the totals)
  bool fold_scan = false;
  ScanArgs scan;
  int64_t* tot = nullptr;
  // ... with the ticket two-level (required with fuse_scan): workgroups of
  // kFusedGroup consecutive ids share a group ticket (kBuQueueStride apart,
  // zero between launches; the group's last workgroup re-zeroes it, sums the
  // group's slots into tot[2 kMaxFusedGrid + 2 g] and takes the level ticket),
  // so the grid can be large without thousands of same-address atomics.
  // (Measured against one ticket and a grid of kMaxFusedGrid / 8:
  // profiles/r2_ab_td_group_ticket.txt.)
  unsigned* group_ticket = nullptr;
  // several ranks: the new frontier words also pushed to the peers (FrontierTable)
  const FrontierTable* push = nullptr;
  int push_rank = 0, push_nranks = 1;
  // several ranks: the send buffer of the candidates' all-to-all (zero_slices
  // slices of `words` words) zeroed here -- word w of every slice by the lane
  // of w -- instead of a memset launch after the exchange
  word_t* zero_next = nullptr;
  int zero_slices = 0;
  // several ranks, fused finish: the level's end in the last workgroup
  // (Comm::direct_level_end; no frontier gathered, or a pushed one); it runs
  // on a no-op chain too (a collective)
  DirectExchange end;
  LevelFinishArgs fin;
};

struct TdSparseArgs {
  ShardView g;
  WorkListIn in;                       // the level's work list
  const int64_t* dev_stats = nullptr;  // [0] entries, [1] edges of the input list
  word_t* frontier_in = nullptr;       // owned slice
  word_t* frontier_out = nullptr;      // owned slice, zero on entry
  word_t* visited = nullptr;           // global
  LevelOut out;
  WorkList next;                       // the next level's work list
  unsigned long long* counter = nullptr;  // zero on entry; reset by the last workgroup
  unsigned* ticket = nullptr;             // zero on entry; reset by the last workgroup
  int64_t* stats = nullptr;
  // (the cap: a sparse chain enqueued for a level that turns out large is a
  // no-op and is re-enqueued dense)
  ChainGuard guard;
  LevelStamp stamp;
  int64_t grid = 0;
  bool first = true;  // first kernel of the level (else a compaction ran before it)
  // from_bits (a level right after a bottom-up one): the input frontier is the
  // bitmap frontier_in itself (`words` owned words, zeroed as read), not a
  // work list -- no unit scan, no compaction; `in` and dev_stats are unused
  // and frontier_out must be zero on entry.  The kernel's
  // workgroups end on a two-level ticket (group_ticket: kFusedGroups tickets
  // kBuQueueStride apart, zero between launches).
  bool from_bits = false;
  int64_t words = 0;
  // Fault injection (DBFS_FAULT_INJECT=kind=late_wg): the workgroups that
  // take no ticket (blockIdx >= the level's active count) first wait this
  // many wall-clock ticks, so they start after the level's last workgroup has
  // finished it -- the dispatch order a busy or cold GPU can produce.  0: off.
  uint64_t late_ticks = 0;
  // Several ranks, direct exchange with a folded level end, a tiny level:
  // td_sparse's last workgroup publishes the lists and then runs the owner
  // side itself (td_sparse_apply's work on one workgroup: nranks, end, fin
  // set) -- one launch per level instead of two.
  bool fuse_apply = false;
  unsigned* group_ticket = nullptr;
  // Several ranks: every target is claimed in the replicated `visited`
  // (fetch-or); an owned one is finished here, a remote one appended to its
  // owner's list (lists + owner * list_stride: count, then the ids; wave-
  // aggregated) -- claiming the remote bit too sends each target at most once
  // per rank.  The lists then travel (Comm::alltoall_lists) and
  // td_sparse_apply claims the received ids on their owner.  Only the apply
  // kernel finishes the level (totals to stats, no decision: the totals are
  // all-reduced first); with lists == nullptr td_sparse finishes it (one rank).
  vid_t* lists = nullptr;
  int64_t list_stride = 0;   // 32-bit words per owner list (count included)
  int64_t part = 0;          // vertices per rank (owner = v / part)
  // td_sparse_apply: the received lists (same layout, nranks of them) and the
  // send lists whose counts it zeroes for the next list level
  const vid_t* recv_lists = nullptr;
  int nranks = 1;
  // direct.active: the lists go straight into the owners' windows (td_sparse)
  // and are read from this rank's window (td_sparse_apply, after the flags)
  DirectExchange direct;
  // end.active (td_sparse_apply, several ranks): the level's end folded into
  // its last workgroup -- the totals (stats[2..3]) pushed to every peer's
  // window, the peers' awaited and summed, then the decision (`fin`), as
  // Comm::level_end without a frontier gather; no collective launch after.
  DirectExchange end;
  LevelFinishArgs fin;
};

// Binned top-down level (one rank, large frontiers; propagation blocking):
// instead of a random probe and a random store per frontier edge, the edges'
// targets are first written into nbins contiguous bins by target range
// (count pass: per-workgroup bin counts; scan; fill pass: each workgroup puts
// a step's targets in bin order in LDS and copies every bin's run out
// contiguously at its scanned position), then one workgroup per bin
// holds the bin's slice of `visited` in LDS, claims the unvisited targets with
// LDS atomics and writes the bin's frontier / visited words, the new
// vertices' levels and its units' statistics -- every random access of the
// level lands in one bin's LDS / L2-resident range.  Replaces td_expand AND
// the update: a bin is a whole number of 4096-vertex units (shift >= 12), so
// the apply workgroup settles its units from the words it holds in LDS (as
// update_unit does from the candidate words) and the level ends in the
// apply's last workgroup (the update's fused finish: totals slots, two-level
// ticket, scan_finish, the folded unit scan).  No launch follows the apply.
// Correct for any frontier size.
struct BinArgs {
  ShardView g;
  WorkListIn in;
  const int64_t* dev_stats = nullptr;  // [0] work-list entries, [1] frontier edges
  // work list handed over by a sparse level (no compaction ran): zero its
  // vertices' (in.qv) words of clear_frontier
  word_t* clear_frontier = nullptr;
  ChainGuard guard;                    // (device loop only: ctrl required)
  int shift = 12;                      // bin = vertex >> shift (bins align with 4096-vertex units)
  int nbins = 0;
  int grid = 0;                        // workgroups of the count / fill passes
  // count pass: cnt[k * grid + g] = targets of bin k in workgroup g's edges;
  // the scan (one workgroup per bin) makes each bin's row exclusive and sets
  // bin_total[k]; the fill pass and the apply derive the bin starts from
  // bin_total themselves
  uint32_t* cnt = nullptr;             // nbins * grid
  int64_t* bin_total = nullptr;        // nbins
  vid_t* buf = nullptr;                // >= frontier edges
  word_t* visited = nullptr;
  word_t* frontier = nullptr;          // next frontier (every word written)
  int64_t words = 0;
  // the apply's settle (as UpdateArgs): the new vertices' levels, every
  // unit's statistics (count / degree sum of its new vertices with a
  // non-empty row) ...
  LevelOut out;
  int64_t* unit_cnt = nullptr;         // nunits
  int64_t* unit_deg = nullptr;
  // ... and the level's end in its last workgroup (UpdateArgs::fuse_scan /
  // fold_scan / tot / group_ticket: required; the apply's grid is nbins <=
  // kBinMaxBins <= kMaxFusedGrid workgroups and every one takes the ticket)
  FusedFinishArgs fin;
};
// Largest bin span (vertices) and bin count the kernels support.
constexpr int kBinMaxShift = 18;
constexpr int kBinMaxBins = 2048;

// For every edge (u, v) with u in the work list and v not visited: next[v] = 1.
struct TdArgs {
  ShardView g;
  WorkListIn in;
  int64_t q = 0;        // work-list entries
  int64_t m = 0;        // work-list edges (qscan[q])
  const word_t* visited = nullptr;  // global
  word_t* next = nullptr;           // global
  // Byte-map mode (large levels): next_bytes[v] = 1 with a plain byte store
  // instead of a scattered 64-bit atomicOr on next (the atomics bound the
  // top-down rate at ~40 G edges/s on MI355X).
  uint8_t* next_bytes = nullptr;
  // List mode (host loop; small levels, multi-rank): candidate v is appended to its
  // owner's list lists[o * (list_cap + 1) + 1 + k]; slot 0 of each list is its
  // count (wave-aggregated atomics, at most nranks per wave instruction).
  // list_cap >= global frontier edges guarantees no overflow.
  vid_t* lists = nullptr;
  int64_t list_cap = 0;
  int64_t part = 0;   // owner(v) = v / part
  // Byte mode only: skip the visited pre-check (few vertices visited yet).
  bool check_visited = true;
  // One rank, narrow levels, byte-map levels: instead of marking next_bytes,
  // store new_level straight into the level array of every unvisited
  // candidate (plain byte stores; the visited check is then always made) --
  // update_frontier(level_direct) derives the new frontier from it, nothing to
  // clear afterwards.
  uint8_t* level_direct = nullptr;
  LevelOut out;  // (level_direct stores out.byte())
  // Levels of at least td_hub_min_edges frontier edges read g.td_col and test
  // hub targets in an LDS copy of td_hub_vis (visited bits of the top-down
  // hubs, this level's snapshot: hub_visited); not with owner lists.
  const word_t* td_hub_vis = nullptr;
  int64_t td_hub_min_edges = 0;
  // ... and only once the visited vertices hold this fraction of all
  // adjacency entries (device loop: ctrl->vis_deg; earlier, most hub
  // targets are unvisited and decoding them costs a dependent load)
  double td_hub_vis_frac = 0.0;
  // With the filter and level_direct: a hub target unvisited at the level's
  // start is claimed by a byte store here (kTdMaxHubs bytes, L2-resident,
  // no decode of the hub id) instead of a level byte store scattered over
  // the whole level array; hub_apply turns the marks into level bytes.
  uint8_t* td_hub_mark = nullptr;
  // Unvisited filter (UnvisArgs, this level's snapshot): targets whose bit is
  // clear are visited without a `visited` probe (device loop, Dyn output; a
  // 1024-thread variant without the hub filter)
  const word_t* unvis = nullptr;
  uint64_t unvis_mult = 0;
  // ... its chunks' set bits (UnvisArgs::pop): the filter variant and the
  // plain one are both launched, and the level runs in the filter variant
  // iff at most unvis_max_density of the filter's bits are set
  const uint32_t* unvis_pop = nullptr;
  double unvis_max_density = 0.5;
  // Launch 1024-thread workgroups when the grid has fewer blocks than this.
  int64_t wide_below_blocks = 0;
  // Device loop: q / m come from dev_stats[0..1], bits vs bytes and the
  // visited pre-check from guard.ctrl; the fixed grid loops over the edge
  // blocks.  (Dense chains only: never with `lists`.)
  ChainGuard guard;
  const int64_t* dev_stats = nullptr;
  int64_t grid = 0;
  int64_t grid_filter = 0;  // ... for the hub-filter variant (0: grid)
  // Device loop, work list handed over by a sparse level (no compaction ran):
  // zero the input vertices' (in.qv) words of clear_frontier.
  word_t* clear_frontier = nullptr;
  // Split level (one rank, level_direct): this launch runs part split_i of
  // split_k equal runs of the level's edge blocks; between parts
  // refresh_visited ORs the vertices claimed so far into `visited`, so a
  // later part's probes skip them instead of storing their level byte again.
  int split_k = 1, split_i = 0;
};

// A split top-down level (TdArgs::split_k): visited |= the vertices whose level
// byte is out.byte() (claimed by the parts so far).  words: visited words
// (out.level8 holds 64 x words bytes).
struct RefreshArgs {
  LevelOut out;
  word_t* visited = nullptr;
  int64_t words = 0;
  ChainGuard guard;
};

// Received candidate lists (nranks lists of list_cap + 1 words, count first)
// -> bits in cand (owned slice), local index v - lo.
struct ListScatterArgs {
  const vid_t* lists = nullptr;
  int nranks = 1;
  int64_t list_cap = 0;
  int64_t lo = 0;
  word_t* cand = nullptr;
  int64_t words = 0;  // words of cand (bounds check of the checked build; 0: unchecked)
};

// next[w] |= bits of bytes[64 w .. 64 w + 63]; bytes cleared (multi-rank
// byte-map top-down: the exchange stays a bitmap all-to-all).
struct PackArgs {
  uint8_t* bytes = nullptr;
  word_t* next = nullptr;
  int64_t words = 0;
  // device loop: runs only on a live chain, and only on a byte-map top-down
  // level (guard.ctrl->bytes) -- or, with `flag`, when *flag is set (a
  // bottom-up chain: the several-rank hub cut's remote claims, BuArgs::cut_bytes)
  ChainGuard guard;
  const int* flag = nullptr;
  // words [skip_begin, skip_end) are left alone (the hub cut: this rank's own
  // slice, whose claims never go through the byte map)
  int64_t skip_begin = 0, skip_end = 0;
};

// Bottom-up step fused with the frontier update: for every owned unvisited v,
// if some neighbour u has frontier[u], v joins the new frontier: visited[v],
// new_frontier[v], level[v] = new_level, unit stats as in UpdateArgs.
// Slots of BuArgs::tot (one pair per workgroup of a fused bottom-up finish).
constexpr int kMaxFusedGrid = 4096;
// Group tickets kBuQueueStride uints apart (one 128-B line each: counters
// sharing a line serialise their atomics).
constexpr int kBuQueueStride = 32;
// Fused update finish, two-level ticket (UpdateArgs::group_ticket).
constexpr int kFusedGroup = 64;
constexpr int kFusedGroups = kMaxFusedGrid / kFusedGroup;
static_assert(kBinMaxBins <= kMaxFusedGrid, "the binned apply's workgroups each own a totals slot");

struct BuArgs {
  ShardView g;
  // Zero-degree / padding bits of the owned slice (required: a vertex's row in
  // the non-empty-row view is found by its rank among the non-zero-degree ones).
  const word_t* zdeg = nullptr;
  // Hub frontier bits (g.nhubs bits, from hub_gather), staged in LDS.
  const word_t* hub_front = nullptr;
  word_t* visited = nullptr;         // owned slice
  const word_t* frontier = nullptr;  // current frontier, global
  word_t* new_frontier = nullptr;    // owned slice of the next frontier (fully overwritten)
  LevelOut out;
  int64_t words = 0;
  int lane_limit = 32;               // neighbours scanned per lane before wave cooperation
  bool follow_up = false;            // the previous level was bottom-up too (launch shape)
  int whole_units = 0;               // hub kernel, compacted: 64 words per wave (1), 16 (-1), by shard size (0)
  int small_waves = 0;               // ... split units: 4 words per wave on a first level (1), never (-1), by shard size (0)
  // (follow_up, whole_units and small_waves shape shards with packed records; without them: 16 words per wave, queued scans)
  int64_t* unit_cnt = nullptr;
  int64_t* unit_deg = nullptr;
  ChainGuard guard;
  // One rank, device loop: the level's totals and finish (ScanArgs: stats,
  // direction decision, record, mailbox) run in the bottom-up kernel's
  // last-arriving workgroup instead of a scan launch: workgroup g stores its
  // totals in tot[2g], tot[2g + 1] (kMaxFusedGrid slots).  The per-unit
  // prefixes are left to a scan_units (finish off) in the next chain, only
  // when it compacts the frontier (a top-down level).  Kernels without the
  // epilogue launch scan_units after themselves.
  bool fuse_scan = false;
  ScanArgs scan;
  int64_t* tot = nullptr;
  // several ranks, fuse_scan: the level's end folded into the last
  // workgroup (Comm::direct_level_end; no frontier gather), as td_sparse_apply
  DirectExchange end;
  LevelFinishArgs fin;
  // Hub-cut level (one rank, narrow levels, hub kernels with packed records,
  // cut_edges > 0; bu_cut_prep before it): when the level's frontier edges
  // outside the hubs -- guard.ctrl->m_f minus the frontier hubs' degrees -- are at
  // most cut_edges, hub_gather sets *cut_flag and bu_cut_prep writes the level
  // byte of the non-hub frontier vertices' unvisited neighbours (top-down);
  // every row scan of the level then stops at its first non-hub neighbour (a
  // hub-first row's later neighbours cannot be in the frontier: rows with a
  // non-hub frontier neighbour were claimed).  Claimed vertices (unvisited,
  // level byte = this level) skip the scan and join the output with the
  // found ones.  *cut_flag = 0: a plain level.  Wide (32-bit) levels: the
  // claims are non-zero bytes of cut_claim (one per vertex, all zero between
  // levels), which the bottom-up kernel clears as it writes their levels.
  int64_t cut_edges = 0;
  int* cut_flag = nullptr;
  uint8_t* cut_claim = nullptr;
  // ... several ranks (bu_cut_prep): this rank's non-hub frontier is the
  // global frontier's words [cut_word_off, + words); a neighbour is skipped
  // when its bit in cut_vis (the replicated global visited bitmap) is set;
  // an owned one is claimed as above, a remote one gets its byte of
  // cut_bytes (the global byte map, packed per owner and all-to-all'ed).
  // bu_cut_merge then claims the received words (cut_recv: P slices of
  // `words`, this rank's own empty) and zeroes cut_next (the packed bitmap,
  // P slices) for the next user.
  uint8_t* cut_bytes = nullptr;
  const word_t* cut_vis = nullptr;
  int64_t cut_word_off = 0;
  const word_t* cut_recv = nullptr;
  word_t* cut_next = nullptr;
  int cut_rank = 0, cut_nranks = 1;
  // several ranks: the new frontier words also pushed to the peers (FrontierTable)
  const FrontierTable* push = nullptr;
  int push_rank = 0, push_nranks = 1;
};

// out bit h = visited bit of g.td_hub_vertex[h] (visited global): the
// snapshot a top-down level filters hub targets with; device loop: runs only
// on a live chain of a level of at least min_edges frontier edges.
struct HubVisitedArgs {
  ShardView g;
  const word_t* visited = nullptr;
  word_t* out = nullptr;
  ChainGuard guard;
  int64_t min_edges = 0;
  double vis_frac = 0.0;  // as TdArgs::td_hub_vis_frac
};

// A dense top-down level's unvisited filter (this level's snapshot): bit i
// is set iff some vertex v with unvis_index(v) == i is unvisited, where
// unvis_index(v) = (v * mult) >> 32 maps the n vertices onto kUnvisBits bits
// in contiguous runs (mult = unvis_mult(n): at most 2^32, identity for n <=
// kUnvisBits).  td_expand (TdArgs::unvis) stages it in LDS and probes
// `visited` only for targets whose filter bit is set: late levels, where most
// targets are visited, trade most scattered L2 requests for LDS reads.
// 7104 words: with td_expand's owner map of two edge blocks (kUnvisSpan,
// 16-bit entries) two 1024-thread workgroups fill a CU's 160 KiB of LDS.
// Built in chunks of 64 words (kUnvisChunks), each chunk's set bits counted
// (UnvisArgs::pop).
constexpr int64_t kUnvisWords = 7104;
constexpr int64_t kUnvisBits = kUnvisWords * 64;
constexpr int kUnvisChunks = static_cast<int>(kUnvisWords / 64);
constexpr int kUnvisSpan = 2;
DBFS_HD uint64_t unvis_mult(int64_t n) {
  if (n <= kUnvisBits) return uint64_t(1) << 32;
  return (static_cast<uint64_t>(kUnvisBits) << 32) / static_cast<uint64_t>(n);
}
DBFS_HD uint32_t unvis_index(uint64_t v, uint64_t mult) { return static_cast<uint32_t>((v * mult) >> 32); }
// the first vertex with unvis_index >= i
DBFS_HD uint64_t unvis_first(uint64_t i, uint64_t mult) { return ((i << 32) + mult - 1) / mult; }
struct UnvisArgs {
  const word_t* visited = nullptr;  // global (n bits)
  int64_t n = 0;
  uint64_t mult = 0;
  word_t* out = nullptr;            // kUnvisWords
  uint32_t* pop = nullptr;          // kUnvisChunks: set bits per 64-word chunk
  ChainGuard guard;
};

// out.level8[td_hub_vertex[h]] = out.byte() for every h with mark[h] != 0,
// which is cleared: td_expand's hub claims (TdArgs::td_hub_mark).  mark holds
// kTdMaxHubs bytes.
struct HubApplyArgs {
  ShardView g;
  uint8_t* mark = nullptr;
  LevelOut out;
  ChainGuard guard;
};

// hub_gather copies (visited merge, pushed slices) with at most this many
// workgroups (the hub-cut part sums are sized for it)
constexpr int kHgCopyGrid = 512;

// hub_front bit h = frontier bit of g.hub_vertex[h] (frontier global).
struct HubGatherArgs {
  ShardView g;
  const word_t* frontier = nullptr;
  word_t* hub_front = nullptr;  // ceil(nhubs / 64) words
  ChainGuard guard;
  // several ranks: visited[0, words) |= frontier (the all-gathered remote
  // slices into the replicated visited bitmap) in the same launch
  word_t* visited = nullptr;
  int64_t words = 0;
  // hub-cut levels (BuArgs::cut_edges): cut_part[b] = the summed degrees of
  // the frontier hubs of workgroup b (kBlock hubs each); the last workgroup
  // (cut_ticket, zero between levels) stores the decision in *cut_flag
  int64_t* cut_part = nullptr;
  int64_t cut_edges = 0;
  int* cut_flag = nullptr;
  unsigned* cut_ticket = nullptr;
  // several ranks, the previous level's slices pushed (FrontierTable): the
  // peers' slices copied from this rank's window into pull_out (the global
  // frontier; `words` per slice) -- and merged into visited with `visited` --
  // and the hubs' bits read from their owners' slices directly
  const FrontierTable* pull = nullptr;
  word_t* pull_out = nullptr;
  int pull_rank = 0, pull_nranks = 1;
  int64_t pull_words = 0;
};

// Bits of the owned slice for vertices with degree 0 or beyond the shard
// (padding): they can never be discovered, so they start out "visited".
struct ZeroDegArgs {
  ShardView g;
  word_t* out = nullptr;  // owned slice
  int64_t words = 0;
  bool padding_only = false;  // directed graphs: only the padding past the shard
};

// Vertex-centric ("status array") top-down: every owned v with level[v] == cur
// marks its unvisited neighbours in next.  (The reference's simple/multiBfs
// variant, bfs.cu:101-130, made race-free.)
struct StatusArgs {
  ShardView g;
  const lvl_t* level = nullptr;
  lvl_t cur = 0;
  const word_t* visited = nullptr;  // global
  word_t* next = nullptr;           // global
};

// Reference-algorithm mode (bfs.cu:134-165): thread per frontier vertex,
// atomicMin claim on a replicated distance array, one atomic counter per owner
// bucket.
struct RefExpandArgs {
  ShardView g;
  const vid_t* queue = nullptr;  // global ids of owned frontier vertices
  int64_t q = 0;
  lvl_t next_level = 0;
  lvl_t* dist = nullptr;         // replicated, n entries
  int64_t part = 0;              // owner(v) = v / part
  int64_t* bucket_cnt = nullptr; // nranks
  vid_t* buckets = nullptr;      // nranks * bucket_cap
  int64_t bucket_cap = 0;
};

// Received ids: entries in [self_begin, self_end) were claimed locally and are
// kept; the others are kept iff this rank's atomicMin claim succeeds.  Kept ids
// are appended to queue (counter *qcount).
struct RefAcceptArgs {
  const vid_t* recv = nullptr;
  int64_t total = 0;
  int64_t self_begin = 0, self_end = 0;
  lvl_t next_level = 0;
  lvl_t* dist = nullptr;
  vid_t* queue = nullptr;
  int64_t* qcount = nullptr;
};

// Scan-mode BFS (the reference's single-GPU "scan" pipeline nextLayer /
// countDegrees / scanDegrees / assignVerticesNextQueue, bfs.cu:706-781 and
// H16c in SURVEY.md): an atomic-free frontier build.  relax writes
// dist[v] = next_level and claim[v] = e (shard-local edge index, last writer
// wins) with plain stores; count gives every frontier vertex i, per owner o,
// the number of edges e it won (offs[o * q + i]); an exclusive scan turns the
// counts into an owner-major output layout; assign writes the children there.
struct ScanBfsArgs {
  ShardView g;
  const vid_t* queue = nullptr;  // global ids of owned frontier vertices
  int64_t q = 0;
  lvl_t next_level = 0;
  lvl_t* dist = nullptr;         // replicated, n entries
  eid_t* claim = nullptr;        // replicated, n entries (no reset needed)
  int64_t part = 0;              // owner(v) = v / part
  int nranks = 1;
  eid_t* offs = nullptr;         // nranks * q + 1 entries
  eid_t* bounds = nullptr;       // scan_bounds: offs[o * q] for o in [0, nranks]
  int64_t* counts = nullptr;     // scan_bounds: per-owner child counts
  vid_t* out = nullptr;          // children, owner-major
};

// Graph500-style validation of a full level array against a shard: counts
// violations of (a) |level[u] - level[v]| <= 1 over every edge with both ends
// reached, (b) reached-unreached edges, (c) reached v != src without a
// neighbour at level[v] - 1.  out[0..2] += counts.
// directed: g is the in-edge view (DeviceGraph::in_view: row v holds the u of
// every stored entry u -> v) and the rules are the directed ones -- (a) both
// ends reached and level[v] > level[u] + 1, (b) u reached and v unreached,
// (c) reached v != src without an entry u -> v at level[v] - 1; the reverse of
// (a) and (b) is legal.
struct ValidateArgs {
  ShardView g;
  const lvl_t* level_global = nullptr;  // n entries
  int64_t src = 0;
  int64_t* out = nullptr;               // 3 counters (device)
  bool directed = false;
};

// Graph500 parent tree from levels: parent[v] = first neighbour u with
// level[u] == level[v] - 1 (global vertex id), parent[src] = src, -1 if
// unreached.  Computed after a run from the all-gathered level array.
// A directed graph: the caller passes the in-edge view as g (the rule is the
// same, nothing branches); its rows are in ascending id order, so the parent is
// the smallest u with an entry u -> v one level closer.
struct ParentArgs {
  ShardView g;
  const lvl_t* level_global = nullptr;  // n entries
  int64_t src = 0;
  int64_t* parent = nullptr;            // rows (owned slice)
};

// ---- concurrent multi-source BFS (Engine::run_batch) -------------------------
// One batch is at most kMsSources sources; source s is bit s of a 64-bit word
// per vertex.  seen / next are indexed by owned row, front by global vertex
// (one rank: the same).  A level is either one ms_pull, or ms_push + ms_settle
// (one rank only); both leave the level's totals in stats[0..kMsStats) and,
// with a mailbox, stamp them there for the spinning host.
constexpr int kMsSources = 64;
// stats: [0] vertices with new bits (the next level's active list), [1] their
// degree sum, [2 + s] vertices source s discovered
constexpr int kMsStats = 2 + kMsSources;
// workgroups of an ms kernel at most (they stride over their work; one totals
// slot of kMsStats entries each)
constexpr int kMsMaxGrid = 1024;
// f(L{}) with the level type of lvl_bytes (2: uint16_t, else uint8_t): the one
// place that turns the width into a type, for the launchers and the host alike.
template <class F>
decltype(auto) ms_level_type(int lvl_bytes, F&& f) {
  if (lvl_bytes == 2) return f(uint16_t{});
  return f(uint8_t{});
}
// The level matrix entry that reads unreached: all ones.
template <class L>
DBFS_HD constexpr int ms_unreached() {
  return static_cast<int>(static_cast<L>(~static_cast<L>(0)));
}
inline int ms_unreached(int lvl_bytes) {
  return ms_level_type(lvl_bytes, [](auto l) { return ms_unreached<decltype(l)>(); });
}
// bit s set: s < k
DBFS_HD word_t ms_batch_mask(int k) { return k == kMsSources ? ~word_t(0) : (word_t(1) << k) - 1; }

// Host-mapped totals of a batch level (as StatsMailbox: values first, then seq).
struct MsMailbox {
  int64_t seq = 0;
  int64_t v[kMsStats] = {};
};

// What every ms kernel shares.
struct MsState {
  ShardView g;
  // The rows a pull searches: the in-edge shard of a directed graph
  // (DeviceGraph::in_view), g's own arrays otherwise.  Everything else (push,
  // settle, the degrees a level's totals sum) stays on g, the out-edges.
  const eid_t* in_row_off = nullptr;
  const vid_t* in_col = nullptr;
  bool directed = false;
  word_t* seen = nullptr;   // owned rows
  word_t* front = nullptr;  // this level's frontier words, by global vertex
  word_t* next = nullptr;   // owned rows: the new bits of this level
  // level matrix (optional): row v holds the kMsSources levels of owned vertex
  // v, lvl_bytes (1 or 2) each; 0: none kept
  void* lvl = nullptr;
  int lvl_bytes = 0;
  word_t batch_mask = 0;    // bit s set: source s is part of the batch
  int level = 0;            // the level new vertices get
  vid_t* active_out = nullptr;           // owned rows with new bits (local ids), unordered
  // [0] active_out entries, [1] touched entries, [2] queued long rows of a
  // push; zero between levels
  unsigned long long* cursor = nullptr;
  int64_t* tot = nullptr;                // kMsMaxGrid x kMsStats per-workgroup totals
  unsigned* ticket = nullptr;            // zero between launches
  int64_t* stats = nullptr;              // kMsStats
  MsMailbox* mailbox = nullptr;          // device pointer; nullptr: stats only
  int64_t seq = 0;
};

// Clears seen / next (next_words) / front (front_words) and the level matrix,
// then seeds the batch: bit s of seen / front of src[s], level 0, the distinct
// owned sources as the first active list, their totals in stats.
struct MsInitArgs {
  MsState s;
  int k = 0;
  int64_t src[kMsSources] = {};  // global vertex ids (duplicates allowed)
  int64_t next_words = 0, front_words = 0;
};

// Dense form: every owned vertex with need = ~seen & batch_mask != 0 ORs the
// front words of its row until need is covered; new = acc & need goes to
// seen, next (every owned word is written, zero included) and the level matrix.
struct MsPullArgs {
  MsState s;
  int lane_limit = 32;  // neighbours a lane reads itself before its row goes to the wave
};

// Sparse form (one rank): for every active vertex v and neighbour w,
// m = front[v] & ~seen[w] is ORed into next[w]; the first toucher of w appends
// it to `touched`.  front[v] is zeroed by the lane that read it.
struct MsPushArgs {
  MsState s;
  const vid_t* active = nullptr;
  int64_t n_active = 0;
  vid_t* touched = nullptr;
  // words of `next` to zero first (the level before was a pull, which read
  // this buffer as its frontier): that level's active list
  const vid_t* clear_list = nullptr;
  int64_t clear_n = 0;
  // degree sum of the active vertices, and (HIP) the queue of the rows too
  // long for one wave: vertex and frontier word, long_cap entries
  int64_t active_edges = 0;
  vid_t* long_v = nullptr;
  word_t* long_f = nullptr;
  int64_t long_cap = 0;
};

// Over the touched list of the push before it (cursor[1] entries, at most
// max_touched): new = next & ~seen, then the pull form's bookkeeping.
struct MsSettleArgs {
  MsState s;
  const vid_t* touched = nullptr;
  int64_t max_touched = 0;
};

// End pass of a batch: deg_sum[s] += degree of every owned vertex source s reached.
struct MsDegreeArgs {
  ShardView g;
  const word_t* seen = nullptr;
  int64_t* deg_sum = nullptr;  // kMsSources, zero on entry
};

// A finished pass's level matrix and its sources: what the check and the
// betweenness sweeps read (Engine::pass_matrix).  `lvl` is the full matrix:
// row v holds the kMsSources levels of global vertex v (one rank: the pass's
// own matrix; several: the all-gathered slices), all ones = unreached.
struct MsPassMatrix {
  const void* lvl = nullptr;
  int lvl_bytes = 1;
  int64_t lvl_rows = 0;          // rows of `lvl` (>= n: the checked build's bound on column ids)
  int k = 0;
  int64_t src[kMsSources] = {};  // global vertex ids
  word_t batch_mask = 0;         // ms_batch_mask(k)
};
// lvl[v][s] on the host (the CPU backend's loops).
inline int level_at(const MsPassMatrix& m, int64_t v, int s) {
  return ms_level_type(m.lvl_bytes, [&](auto l) -> int {
    return static_cast<const decltype(l)*>(m.lvl)[v * kMsSources + s];
  });
}

// Graph500-style check of a finished pass's level matrix, all sources at once
// (ValidateArgs' rules per source; Engine::run_batch validate / keep_parents).
// Over the directed adjacency entries (u, w) of the owned rows, for every
// source s < m.k:
//   count form (out):  out[3 s + 0] += entries with both ends reached and
//     |lvl[u][s] - lvl[w][s]| > 1 (gap), out[3 s + 1] += entries with exactly
//     one end reached (cross), out[3 s + 2] += reached u != src[s] without a
//     neighbour one level closer, and u == src[s] with a level other than 0
//     (orphan);
//   parent form (par): par[r * kMsSources + s] = the first neighbour of owned
//     row r, in stored row order, one level closer to source s (global id);
//     src[s] itself for u == src[s]; all ones when u is unreached (or has no
//     such neighbour).
// Entries of sources s >= k are neither counted nor stored.
// directed: g is the in-edge view (row v: the u of every stored entry u -> v,
// ascending) and the rules are ValidateArgs' directed ones -- gap: both reached
// and lvl[v] > lvl[u] + 1; cross: u reached, v unreached; orphan and parent as
// above over the in-row (the first parent is then the smallest id).
constexpr int kMsCheckCounters = 3;
constexpr uint32_t kMsNoParent = 0xFFFFFFFFu;
struct MsCheckArgs {
  ShardView g;
  MsPassMatrix m;
  int64_t* out = nullptr;        // kMsSources x kMsCheckCounters, accumulated; nullptr: no counts
  uint32_t* par = nullptr;       // owned rows x kMsSources; nullptr: no parents
  bool directed = false;
};

// Shortest-path counts and Brandes dependencies of a finished pass, all its
// sources at once (Engine::run_batch betweenness / keep_path_counts).  `m` is
// the pass's full level matrix (MsPassMatrix); `val` is a matrix of doubles
// of the same shape (row v: the kMsSources values of global vertex v) and
// `own` the lines of the owned rows, which a launch writes (one rank: val
// itself; several: a buffer of its own, all-gathered into every rank's val
// after each launch).  Entries are the stored adjacency entries, duplicates
// and self-loops included; lvl_s is source s's column of the matrix.
//   ms_bc_init      val[v][s] = own[..][s] = 1 for v == src[s], s < k; else 0.
//   ms_bc_forward   level L: for every owned v and s with lvl_s(v) == L,
//     own[v][s] = sum of val[u][s] over the entries u of v's row in
//     (row_off, col) -- the predecessor rows: the in-edge shard of a directed
//     graph, the shard's own rows otherwise -- with lvl_s(u) == L - 1, added in
//     stored row order.  After levels 1 .. depth - 1 the matrix holds sigma.
//   ms_bc_backward  level L, from the deepest down: for every owned v and s
//     with lvl_s(v) == L, acc = sum of val[w][s] over the entries w of v's
//     out-row (row_off, col = g's) with lvl_s(w) == L + 1 (leaf: the deepest
//     level, nothing is walked and acc = 0); delta = sigma * acc with sigma =
//     own[v][s], and own[v][s] becomes the coefficient (1 + delta) / sigma the
//     level above adds up -- a lane reads only entries of the adjacent level,
//     so counts and coefficients never mix.  dep[v] += the sum over the lanes
//     s with v != src[s] of delta, reduced in a fixed order (lane i + lane
//     i ^ 32, then ^ 16, ... ^ 1) and stored once per vertex: no atomics on
//     floating-point values anywhere, results are deterministic.
// No lane that is not at level L divides: an unreached vertex's 0 / 0 never
// reaches memory.  walked (optional): += the rows the launch walked (those
// with a lane at level L).
struct MsBcArgs {
  ShardView g;                      // the owned rows (lo, rows)
  const eid_t* row_off = nullptr;   // the rows this launch walks (local offsets, global column ids)
  const vid_t* col = nullptr;
  int64_t nnz = 0;                  // entries of `col` (the checked build's bound)
  MsPassMatrix m;                   // (val has m.lvl_rows rows too)
  double* val = nullptr;            // (written by ms_bc_init and the all-gathers only)
  double* own = nullptr;            // g.rows x kMsSources
  double* dep = nullptr;            // g.rows (backward)
  int level = 0;
  bool leaf = false;
  unsigned long long* walked = nullptr;
  // Forward: bit s is set (an integer atomic OR) when a count stored for
  // source s is not finite -- more than DBL_MAX shortest paths.  The engine
  // reads it after the forward sweep and fails the batch: the backward sweep
  // never sees such a count (with every sigma finite, delta <= n and every
  // coefficient are finite, so it needs no test of its own).
  unsigned long long* overflow = nullptr;
  // Long rows (HIP; optional): the n_long owned rows of more than split_above
  // entries in (row_off, col), in any order (Backend::ms_bc_long_rows).  They
  // are walked by a launch of their own, a workgroup of 16 waves per row, each
  // wave a sixteenth of the row, the partial sums added in wave order -- not
  // by the one wave the other rows get.  n_long = 0: every row by its wave.
  const vid_t* long_rows = nullptr;
  int64_t n_long = 0;
  int64_t split_above = 0;
  // Extended-range form (dbfs/wide.hpp): every value is a mantissa and an
  // exponent, wval / wown take the places of val / own (which are not read),
  // one 768-byte record per vertex -- its kMsSources mantissas, then their
  // exponents -- and the same rules hold with wide sums: forward stores the
  // normalised count and sets no overflow bit; backward keeps sigma, acc and
  // the coefficient wide and leaves delta = sigma * acc, at most n, as a
  // double (0 when below 2^-1074); the lanes' tree and dep are as above.
  // Each rounding is the double form's: where every count and coefficient is
  // a normal double, both forms give the same bits.
  bool wide = false;
  unsigned char* wval = nullptr;    // m.lvl_rows records
  unsigned char* wown = nullptr;    // g.rows records
};

// Connected components (Engine::components): a hook-and-compress forest over
// the adjacency shard.  comp has one entry per vertex of the whole graph
// (g.n; several ranks: every rank its own replica); comp[v] <= v always, a
// vertex with comp[v] == v is a root, and a tree's root is its smallest id.
//   cc_init        comp[v] = v for every v < g.n.
//   cc_link        for every owned row r and every stored entry w at positions
//     [first, first + count) of the row (count < 0: to the row's end), hook
//     (g.lo + r, w): while the two ends' trees have different roots, hang the
//     larger root under the smaller id (a 32-bit compare-and-swap), else climb
//     both trees.  Pointers only decrease, so the result after cc_compress
//     does not depend on the order of the hooks.  With `skip`, a row whose
//     comp[g.lo + r] == skip_label when the row is taken is not walked.
//   cc_link_pairs  hook (pair_lo + i, other[i]) for i < pairs.
//   cc_compress    comp[v] = the root of v's tree, for every v < g.n.
//   cc_sample      sample_out[i] = comp[sample_idx[i]] for i < samples.
//   cc_sizes       (compressed comp) size[l] = vertices with comp[v] == l, and
//     totals[0..3] = roots, roots of size 1, the largest size, its label (the
//     smaller label on a tie).
// Self-loops and duplicate entries change nothing.  g.col holds plain vertex
// ids; the hub-encoded copies are not read.
constexpr int kCcTotals = 4;
// HIP, cc_sizes: workgroups at most, each with a slot of kCcTotals partial totals.
constexpr int kCcSizeGrid = 1024;
struct CcArgs {
  ShardView g;                     // the owned rows (lo, rows, row_off, col, nnz) and n
  vid_t* comp = nullptr;           // g.n entries
  // cc_link
  int64_t first = 0, count = -1;
  bool skip = false;
  vid_t skip_label = 0;
  // Long rows (HIP): rows with more than 1024 entries to walk are queued
  // here by the first launch (long_count: one counter, zeroed by cc_link) and
  // walked by the whole grid in a second one; long_cap >= g.nnz / 1024 + 1
  // holds them all.
  vid_t* long_rows = nullptr;
  int64_t long_cap = 0;
  unsigned long long* long_count = nullptr;
  // cc_link_pairs
  const vid_t* other = nullptr;
  int64_t pair_lo = 0, pairs = 0;
  // cc_sample
  const vid_t* sample_idx = nullptr;
  vid_t* sample_out = nullptr;
  int samples = 0;
  // cc_sizes
  uint32_t* size = nullptr;        // g.n entries (zeroed by cc_sizes)
  int64_t* totals = nullptr;       // kCcTotals
  int64_t* slots = nullptr;        // HIP: kCcSizeGrid x kCcTotals
};

// Strongly connected components (Engine::strong_components): trim, forward
// colouring and backward closure over the out- and in-rows.  Every array has
// one entry per vertex of the whole graph (several ranks: every rank its own
// replica; a sweep writes only the entries of its owned rows, the engine
// all-gathers them).  scc[v] == kSccNone while v is live; an edge u -> w counts
// when u != w, both ends are live and cls[u] == cls[w].
//   scc_init         scc = cls = colour = kSccNone for every v < n.
//   scc_trim         one sweep over the owned rows: a live v with no counting
//     out-edge or no counting in-edge gets scc[v] = v; *changed += settled.
//   scc_pivot        pivot_out[0..1] = (in-degree x out-degree, id) of the live
//     owned vertex with the largest product (stored entries, duplicates and
//     self-loops included), the smaller id on a tie; id kSccNone when none.
//   scc_colour_init  live v (all n): colour[v] = v, or with pivot_only: v for
//     v == pivot and kSccNone otherwise.
//   scc_forward      one pull sweep over the owned in-rows: colour[v] = min(
//     colour[v], colour[u]) over counting in-neighbours u; *changed += changes.
//     With pivot_only the only colour is the pivot's: an uncoloured v takes it
//     from the first in-neighbour that has it, a coloured v is done.  (First
//     round only: all classes are equal and no colour of an earlier round is
//     left, so an in-neighbour with the pivot's colour counts.)
//   scc_backward     one pull sweep over the owned out-rows: a live v with
//     colour c joins (scc[v] = c) when v == c or some out-neighbour w has
//     scc[w] == c; *changed += joined.  (No other SCC ever has the label of a
//     live root, so scc[w] == c alone says "w has this colour and is in".)
//   scc_end_round    live v (all n) with a colour: cls[v] = colour[v].
//   scc_relabel      (all n) every v with scc[v] == pivot gets the smallest
//     such v (the pivot round's label is the pivot, not the minimum).
// Values only fall (colour) or settle once (scc), and each sweep's fixed point
// is unique: a sweep may read entries other rows stored during the same
// launch, in any order.  out.col / in.col hold plain vertex ids.
constexpr vid_t kSccNone = 0xFFFFFFFFu;
// HIP, scc_pivot: workgroups at most, each with a slot of two words.
constexpr int kSccPivotGrid = 1024;
struct SccArgs {
  ShardView out, in;               // the owned rows of the adjacency and of the in-edge shard (same lo, rows, n)
  vid_t* scc = nullptr;            // n entries each
  vid_t* cls = nullptr;
  vid_t* colour = nullptr;
  unsigned long long* changed = nullptr;  // this sweep's counter (the engine zeroes it)
  // The counter of the sweep enqueued before this one, of the same step
  // (nullptr: none): when it is zero that sweep was at the fixed point, and
  // this one returns at once -- a surplus sweep costs its launch only.
  const unsigned long long* prev_changed = nullptr;
  // scc_pivot
  unsigned long long* pivot_out = nullptr;    // 2 words
  unsigned long long* pivot_slots = nullptr;  // HIP: kSccPivotGrid x 2
  // scc_colour_init / scc_relabel
  vid_t pivot = kSccNone;
  bool pivot_only = false;
  vid_t* relabel_min = nullptr;    // HIP: one word
};

// Eccentricity bounding (Engine::eccentricities; Takes and Kosters): lower and
// upper bounds of every vertex's eccentricity, tightened from the level
// matrix of 64-source batch passes until they meet.  lo, hi and state have one
// entry per vertex of the whole graph (several ranks: every rank its own
// replica, updated in full from the all-gathered matrix, so all replicas stay
// equal); state is kEccScope (the call answers for v) | kEccLive (v may still
// be chosen as a source and is still updated) | kEccSettled (lo == hi is v's
// eccentricity).  Integers only.
//   ecc_degrees  deg_own[r] = stored entries of owned row r (the first pass's key).
//   ecc_init     every v < g.n: in scope (scope_all, or comp[v] == label) lo = 0,
//     hi = INT32_MAX and live -- a row without entries settled at 0 instead;
//     out of scope: state 0, lo = hi = -1.
//   ecc_select   first drops (clears kEccLive of) every live v the target no
//     longer needs, by the totals of the last ecc_totals: diameter hi[v] <=
//     totals[kEccMaxLo], radius lo[v] >= totals[kEccMinHi].  Then picks at
//     most kMsSources distinct live vertices.  first: those of largest deg, ties
//     to the smaller id.  Later: the kEccSelHi of largest hi (ties to the smaller
//     id), then among the rest those of smallest lo (ties to the smaller id)
//     until kMsSources are chosen.  Every key is (value << 32) | ~id, unique, so
//     the choice does not depend on the order vertices are looked at.
//     sel_out[0] = how many, sel_out[1 ..] their ids in that order,
//     sel_out[1 + kMsSources] = the live vertices left after the drop.
//   ecc_update   every live v and source s < m.k whose level d = lvl[v][s] is
//     reached: lo[v] = max(lo[v], d, ecc[s] - d), hi[v] = min(hi[v], ecc[s] + d);
//     bounds that meet settle v (live off, settled on).  Rows of vertices that
//     are not live are not read.
//   ecc_totals   over the scope: totals[kEccScopeSize], [kEccSettledN],
//     [kEccLiveN], [kEccMaxLo], [kEccMinHi], and the settled vertices with lo ==
//     count_hi ([kEccAtHi]: the periphery) and == count_lo ([kEccAtLo]: the centre).
constexpr uint32_t kEccScope = 1u, kEccLive = 2u, kEccSettled = 4u;
constexpr int kEccSelHi = 32;
enum EccTotal { kEccScopeSize = 0, kEccSettledN, kEccLiveN, kEccMaxLo, kEccMinHi, kEccAtHi, kEccAtLo, kEccTotals };
enum class EccTarget { All, Diameter, Radius };
// HIP: workgroups at most of ecc_totals (a slot of kEccTotals each) and of
// ecc_select (a slot of kEccSelSlot keys each: its kEccSelHi best by hi, its
// kMsSources best by lo or degree, its live count).
constexpr int kEccTotalsGrid = 1024;
constexpr int kEccSelGrid = 256;
constexpr int kEccSelSlot = kEccSelHi + kMsSources + 1;
constexpr int kEccSelOut = kMsSources + 2;
struct EccArgs {
  ShardView g;                     // the owned rows (lo, rows, row_off) and n
  int32_t* lo = nullptr;           // g.n entries each
  int32_t* hi = nullptr;
  uint32_t* state = nullptr;
  const uint32_t* deg = nullptr;   // every vertex's stored degree (several ranks: the all-gathered deg_own slices)
  uint32_t* deg_own = nullptr;     // ecc_degrees: g.rows entries
  // ecc_init
  const vid_t* comp = nullptr;     // components() labels (nullptr with scope_all)
  bool scope_all = false;
  vid_t label = 0;
  // ecc_select
  bool first = false;
  EccTarget target = EccTarget::All;
  unsigned long long* sel_slots = nullptr;  // HIP: kEccSelGrid x kEccSelSlot
  int64_t* sel_out = nullptr;               // kEccSelOut
  // ecc_update
  MsPassMatrix m;
  int32_t ecc[kMsSources] = {};    // the sources' eccentricities (depth - 1)
  // ecc_totals
  int32_t count_hi = -1, count_lo = -1;
  int64_t* totals = nullptr;       // kEccTotals
  int64_t* slots = nullptr;        // HIP: kEccTotalsGrid x kEccTotals
};

// ---- backend ----------------------------------------------------------------

class Backend {
 public:
  virtual ~Backend() = default;
  virtual DeviceKind kind() const = 0;
  virtual std::string name() const = 0;
  virtual int device_id() const { return -1; }
  // Compute units the launchers size their grids by (0: not a GPU).
  virtual int compute_units() { return 0; }
  virtual void* stream_handle() { return nullptr; }
  // Communication stream.  Collectives are enqueued on comm_stream_handle():
  // the compute stream itself, unless a side region is open.  fork_side()
  // makes the side stream wait for everything enqueued on the compute stream
  // so far and routes the following collectives to it, so kernels enqueued
  // meanwhile overlap them; join_side() makes the compute stream wait for the
  // side stream's work and routes collectives back.  (CPU: no-ops.)
  virtual void* comm_stream_handle() { return stream_handle(); }
  virtual void fork_side() {}
  virtual void join_side() {}
  // Rate of the device wall clock the kernels stamp level records with (ticks
  // per ms; 0: no device clock, records carry no times).
  virtual double wall_clock_khz() const { return 0.0; }

  // Host waits on the device (to_host, to_device, synchronize) call
  // watch(seconds waited) about every period_s while the stream is still busy;
  // the watch may throw to abandon the wait.  A communicator installs one to
  // turn a dead peer into an error instead of a hang.
  const std::function<void(double)>& wait_watch() const { return wait_watch_; }
  void set_wait_watch(std::function<void(double)> watch, double period_s = 0.05) {
    wait_watch_ = std::move(watch);
    wait_period_ = period_s;
  }

  // memory (alloc/free are synchronous; copies/memsets are stream-ordered)
  virtual void* alloc(size_t bytes) = 0;
  virtual void dealloc(void* p) = 0;
  // Device and mapped frees held until the backend is destroyed (HIP: several
  // ranks of one process sharing a device -- a free waits for every stream of
  // the device, a peer's spinning collective included); a no-op elsewhere.
  virtual void set_deferred_frees(bool on) { (void)on; }
  virtual bool deferred_frees() const { return false; }
  // Bytes held in DBufs of this backend now and at most so far: one rank's
  // device footprint (graph shard + traversal state; the peer transport's
  // windows are allocated outside DBufs and not counted).
  int64_t device_bytes() const { return live_bytes_.load(std::memory_order_relaxed); }
  int64_t peak_device_bytes() const { return peak_bytes_.load(std::memory_order_relaxed); }
  void note_device_bytes(int64_t delta) {
    const int64_t now = live_bytes_.fetch_add(delta, std::memory_order_relaxed) + delta;
    int64_t pk = peak_bytes_.load(std::memory_order_relaxed);
    while (now > pk && !peak_bytes_.compare_exchange_weak(pk, now, std::memory_order_relaxed)) {
    }
  }
  virtual void memset_async(void* p, int value, size_t bytes) = 0;
  virtual void copy_async(void* dst, const void* src, size_t bytes) = 0;
  // Several device-to-device copies as one launch (4-byte multiples; the
  // shadow rank's replayed collectives: ReplayComm).
  struct CopyPieces {
    static constexpr int kMax = 16;
    void* dst[kMax] = {};
    const void* src[kMax] = {};
    int64_t bytes[kMax] = {};
    int n = 0;
  };
  virtual void copy_pieces(const CopyPieces& c) {
    for (int i = 0; i < c.n; ++i) copy_async(c.dst[i], c.src[i], static_cast<size_t>(c.bytes[i]));
  }
  virtual void to_host(void* host_dst, const void* dev_src, size_t bytes) = 0;   // blocking
  virtual void to_device(void* dev_dst, const void* host_src, size_t bytes) = 0; // blocking
  virtual void synchronize() = 0;
  // Non-blocking: true when all enqueued work has completed (raises on a
  // device error).
  virtual bool stream_idle() {
    synchronize();
    return true;
  }

  // timing: ms between two recorded points (events on HIP)
  virtual int record_event() = 0;
  virtual double elapsed_ms(int ev_begin, int ev_end) = 0;
  virtual void reset_events() = 0;

  // BFS primitives
  virtual void fill_level(lvl_t* level, int64_t n, lvl_t value) = 0;
  virtual void set_bit(word_t* bitmap, int64_t bit) = 0;
  virtual void update_frontier(const UpdateArgs& a) = 0;
  virtual void scan_units(const ScanArgs& a) = 0;
  // *ctrl = init (stream-ordered)
  virtual void level_ctrl_init(LevelCtrl* ctrl, const LevelCtrl& init) = 0;
  virtual void init_run(const InitRunArgs& a) = 0;
  // mb->v[0..3] = stats[0..3], then mb->seq = seq (release); mb is the device
  // pointer of an alloc_mapped block.
  virtual void publish_stats(const int64_t* stats, StatsMailbox* mb, int64_t seq) = 0;
  // Give an installed wait watch a chance to inspect a host-side wait that does
  // not go through the stream (mailbox spins).
  void poll_wait_watch(double waited) {
    if (wait_watch_) wait_watch_(waited);
  }
  double wait_watch_period() const { return wait_period_; }
  // Pinned host memory the device can store to (nullptr-safe free).
  virtual void* alloc_mapped(size_t bytes, void** device_ptr) = 0;
  virtual void free_mapped(void* host_ptr) = 0;
  virtual void zero_degree_mask(const ZeroDegArgs& a) = 0;
  virtual void compact_frontier(const CompactArgs& a) = 0;
  virtual void td_sparse(const TdSparseArgs& a) = 0;
  virtual void td_sparse_apply(const TdSparseArgs& a) = 0;
  virtual void level_finish(const LevelFinishArgs& a) = 0;
  virtual void td_expand(const TdArgs& a) = 0;
  // the passes of a binned top-down level (BinArgs), stream-ordered
  virtual void td_binned(const BinArgs& a) = 0;
  virtual void pack_bytes(const PackArgs& a) = 0;
  virtual void list_scatter(const ListScatterArgs& a) = 0;
  virtual void bu_step(const BuArgs& a) = 0;
  virtual void hub_gather(const HubGatherArgs& a) = 0;
  // Hub-cut level's top-down part (BuArgs::cut_edges): the unvisited
  // neighbours of the frontier's non-hub vertices claimed into a.pre.
  virtual void bu_cut_prep(const BuArgs& a) = 0;
  // ... several ranks: the claims the peers sent (BuArgs::cut_recv) into the
  // owned claim bytes, the packed bitmap zeroed -- on a live cut level only
  virtual void bu_cut_merge(const BuArgs& a) = 0;
  // A direct exchange's wait as a launch of its own, one wave (ranks sharing
  // a GPU, Comm::split_waits): the consumer after it finds the cells tagged.
  virtual void direct_prewait(const DirectExchange& x) { (void)x; }
  virtual void hub_visited(const HubVisitedArgs& a) = 0;
  virtual void unvis_filter(const UnvisArgs& a) = 0;
  virtual void hub_apply(const HubApplyArgs& a) = 0;
  virtual void refresh_visited(const RefreshArgs& a) = 0;
  // Device-checked build (make checked): whether the kernels verify their
  // bounds, the first recorded violation (code << 48 | detail; 0: none;
  // synchronises, clears; *file: the kernel file whose word held it), and a
  // hook recording violation 99 in that file's word (fault tests).  Enabled
  // means every kernel file with check sites compiled them.
  virtual bool device_checks_enabled() const { return false; }
  virtual uint64_t take_device_check(CheckFile* file = nullptr) { (void)file; return 0; }
  virtual void inject_device_check(CheckFile file = CheckFile::Bfs) { (void)file; }
  virtual void status_expand(const StatusArgs& a) = 0;
  virtual void bitmap_or(word_t* dst, const word_t* src, int64_t words) = 0;
  virtual void ref_expand(const RefExpandArgs& a) = 0;
  virtual void ref_accept(const RefAcceptArgs& a) = 0;
  virtual void scan_relax(const ScanBfsArgs& a) = 0;
  virtual void scan_count(const ScanBfsArgs& a) = 0;   // then exclusive_scan(offs, nranks * q)
  virtual void scan_bounds(const ScanBfsArgs& a) = 0;
  virtual void scan_assign(const ScanBfsArgs& a) = 0;  // consumes offs
  virtual void validate_levels(const ValidateArgs& a) = 0;
  virtual void compute_parents(const ParentArgs& a) = 0;

  // Hub-first adjacency: out[r] = degree of local row r (saturated to uint32);
  // then sort every row by (key_deg[neighbour] descending, neighbour ascending).
  virtual void degrees_u32(const eid_t* row_off, int64_t rows, uint32_t* out) = 0;
  virtual void sort_neighbors(const eid_t* row_off, vid_t* col, int64_t rows, const uint32_t* key_deg) = 0;
  // Every row in neighbour-id order (n: vertex count; the device orders rows
  // of more than 4096 entries by 4096 id buckets only).
  // exact_long: those rows in exact id order too (the in-edge shard).
  virtual void sort_rows_by_id(const eid_t* row_off, vid_t* col, int64_t rows, int64_t n,
                               bool exact_long = false) = 0;
  // head[r] = col[row_off[r]] (0 for empty rows); with hub_idx (one entry per
  // vertex, UINT32_MAX for non-hubs) a hub head is stored as kHubFlag | index.
  virtual void row_heads(const eid_t* row_off, const vid_t* col, int64_t rows, vid_t* head,
                         const uint32_t* hub_idx = nullptr) = 0;
  // Non-empty-row view: counts[w] = non-empty rows of bitmap word w (words
  // entries), then (after an exclusive scan into nz_pref) the dense row_off /
  // head copies.
  virtual void nz_word_counts(const eid_t* row_off, int64_t rows, int64_t words, eid_t* counts) = 0;
  virtual void nz_fill(const eid_t* row_off, const vid_t* head, int64_t rows, const eid_t* nz_pref, eid_t* nz_row_off,
                       vid_t* nz_head) = 0;
  // Packed records of the view (ShardView::nz_rec), their vertices' positions
  // in their units (ShardView::nz_loc) and the unit bases (ceil(rows / 4096)
  // + 1 entries).
  virtual void nz_records(const eid_t* row_off, const vid_t* head, int64_t rows, const eid_t* nz_pref, NzRec* rec,
                          uint16_t* loc, eid_t* unit_base) = 0;
  // out[e] = kHubFlag | hub_idx[col[e]] for hub neighbours, else col[e].
  virtual void encode_hub_cols(const vid_t* col, int64_t nnz, const uint32_t* hub_idx, vid_t* out) = 0;
  // Hubs = vertices of degree >= min_deg (deg_all has n entries): hub_vertex
  // receives their ids (in some order), hub_idx[v] their index or UINT32_MAX;
  // returns the count (blocking).
  virtual int64_t select_hubs(const uint32_t* deg_all, int64_t n, uint32_t min_deg, vid_t* hub_vertex,
                              uint32_t* hub_idx) = 0;

  // graph construction on the device
  // deg[r] += number of edge endpoints owned in rows [lo, lo + rows) (deg zeroed by caller)
  virtual void gen_count_degrees(const GenParams& p, int64_t lo, int64_t rows, eid_t* deg) = 0;
  // in-place exclusive scan of n+1 entries (data[n] receives the total)
  virtual void exclusive_scan(eid_t* data, int64_t n) = 0;
  // col[cursor[u - lo]++] = v for every generated endpoint u owned
  virtual void gen_fill(const GenParams& p, int64_t lo, int64_t rows, eid_t* cursor, vid_t* col) = 0;
  // CSR build from a file's edges (DeviceGraph::from_edges): every edge
  // (u, v) gives the entries u -> v and v -> u, routed to rank x / part as
  // (row << 32 | neighbour).  counts[r] += entries for rank r; then the
  // entries scattered into per-rank segments (cursor[r] = segment start,
  // advanced); at the owner deg[row - lo] += 1 per entry (deg zeroed by the
  // caller) and, after the scan, col[cursor[row - lo]++] = neighbour.
  virtual void route_edges_count(const vid_t* u, const vid_t* v, int64_t m, int64_t part, int nranks,
                                 int64_t* counts) = 0;
  virtual void route_edges_fill(const vid_t* u, const vid_t* v, int64_t m, int64_t part, int nranks,
                                int64_t* cursor, uint64_t* out) = 0;
  // In-edge build (DeviceGraph::build_in_edges): every stored entry r -> c of
  // the shard g (rows [g.lo, g.lo + g.rows)) goes to rank c / part as
  // (c << 32 | g.lo + r).  counts[p] += entries for rank p; then the entries
  // scattered into per-rank segments (cursor[p] = segment start, advanced).
  virtual void in_route_count(const ShardView& g, int64_t part, int nranks, int64_t* counts) = 0;
  virtual void in_route_fill(const ShardView& g, int64_t part, int nranks, int64_t* cursor, uint64_t* out) = 0;
  virtual void entries_count(const uint64_t* e, int64_t k, int64_t lo, eid_t* deg) = 0;
  virtual void entries_fill(const uint64_t* e, int64_t k, int64_t lo, eid_t* cursor, vid_t* col) = 0;
  // sum of degrees of vertices with level != kUnreached (device scalar out)
  virtual void reached_degree_sum(const ShardView& g, const lvl_t* level, int64_t* out2) = 0;
  // over the shard's rows: out2[0] = sum of degree^2, out2[1] = rows with degree > 0
  virtual void degree_moments(const ShardView& g, int64_t* out2) = 0;
  // out[i] = in[i] (narrow levels; kNarrowUnreached -> kUnreached)
  virtual void widen_levels(const uint8_t* in, lvl_t* out, int64_t n, uint8_t base) = 0;
  // concurrent multi-source BFS (MsState)
  virtual void ms_init(const MsInitArgs& a) = 0;
  virtual void ms_pull(const MsPullArgs& a) = 0;
  virtual void ms_push(const MsPushArgs& a) = 0;
  virtual void ms_settle(const MsSettleArgs& a) = 0;
  virtual void ms_degree_sums(const MsDegreeArgs& a) = 0;
  virtual void ms_check(const MsCheckArgs& a) = 0;
  // path counts and dependencies of a finished pass (MsBcArgs)
  virtual void ms_bc_init(const MsBcArgs& a) = 0;
  virtual void ms_bc_forward(const MsBcArgs& a) = 0;
  virtual void ms_bc_backward(const MsBcArgs& a) = 0;
  // list[0 .. *count) = the rows r < rows with row_off[r + 1] - row_off[r] >
  // above, in some order (at most cap stored; *count zero on entry)
  virtual void ms_bc_long_rows(const eid_t* row_off, int64_t rows, int64_t above, vid_t* list, int64_t cap,
                               unsigned long long* count) = 0;
  // connected components (CcArgs)
  virtual void cc_init(const CcArgs& a) = 0;
  virtual void cc_link(const CcArgs& a) = 0;
  virtual void cc_link_pairs(const CcArgs& a) = 0;
  virtual void cc_compress(const CcArgs& a) = 0;
  virtual void cc_sample(const CcArgs& a) = 0;
  virtual void cc_sizes(const CcArgs& a) = 0;
  // strongly connected components (SccArgs)
  virtual void scc_init(const SccArgs& a) = 0;
  virtual void scc_trim(const SccArgs& a) = 0;
  virtual void scc_pivot(const SccArgs& a) = 0;
  virtual void scc_colour_init(const SccArgs& a) = 0;
  virtual void scc_forward(const SccArgs& a) = 0;
  virtual void scc_backward(const SccArgs& a) = 0;
  virtual void scc_end_round(const SccArgs& a) = 0;
  virtual void scc_relabel(const SccArgs& a) = 0;
  // eccentricity bounding (EccArgs)
  virtual void ecc_degrees(const EccArgs& a) = 0;
  virtual void ecc_init(const EccArgs& a) = 0;
  virtual void ecc_select(const EccArgs& a) = 0;
  virtual void ecc_update(const EccArgs& a) = 0;
  virtual void ecc_totals(const EccArgs& a) = 0;

 protected:
  std::function<void(double)> wait_watch_;
  double wait_period_ = 0.05;
  std::atomic<int64_t> live_bytes_{0}, peak_bytes_{0};
};

std::unique_ptr<Backend> make_cpu_backend();
std::unique_ptr<Backend> make_hip_backend(int device);
int hip_device_count();  // 0 when no GPU / runtime unavailable

// RAII device buffer.
template <class T>
class DBuf {
 public:
  DBuf() = default;
  DBuf(Backend& be, size_t n) : be_(&be), n_(n) {
    if (n_) {
      p_ = static_cast<T*>(be_->alloc(n_ * sizeof(T)));
      be_->note_device_bytes(static_cast<int64_t>(n_ * sizeof(T)));
    }
  }
  ~DBuf() { reset(); }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept { *this = std::move(o); }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) {
      reset();
      be_ = o.be_; p_ = o.p_; n_ = o.n_;
      o.be_ = nullptr; o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  void reset() {
    if (p_ && be_) {
      be_->dealloc(p_);
      be_->note_device_bytes(-static_cast<int64_t>(n_ * sizeof(T)));
    }
    p_ = nullptr; n_ = 0;
  }
  T* data() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }

 private:
  Backend* be_ = nullptr;
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace dbfs
