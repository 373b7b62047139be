// Distributed level-synchronous BFS engine.
//
// Reference: runCudaQueueBfs (bfs.cu:542-629, bfs_mpi.cu:549-643) -- a host
// loop that per level launches queueBfs on every device, synchronises, copies
// owner buckets peer-to-peer and reads managed counters.  This engine keeps the
// level-synchronous, owner-computes structure but:
//   * shards the CSR (owned rows only) instead of replicating it per device;
//   * represents frontier / visited as bitmaps (64 vertices per wave ballot);
//   * exchanges discoveries as equal-size bitmap slices (ncclAllToAll) and the
//     new frontier with one ncclAllGather, so no count exchange is needed;
//   * switches direction (Beamer alpha/beta) between top-down load-balanced
//     expansion and bottom-up parent search;
//   * keeps the reference algorithm as Mode::Ref (the measured baseline) and
//     the status-array variant as Mode::Simple.
#pragma once

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "dbfs/backend.hpp"
#include "dbfs/comm.hpp"
#include "dbfs/graph.hpp"
#include "dbfs/partition.hpp"

namespace dbfs {

enum class Mode { Ref, TopDown, BottomUp, DirOpt, Simple, Scan };
Mode parse_mode(const std::string& s);
const char* mode_name(Mode m);

// A CSR shard resident in backend memory.
class DeviceGraph {
 public:
  // `csr` is either the full graph (rows == n) or exactly this rank's shard.
  static std::unique_ptr<DeviceGraph> from_host(Backend& be, const HostCSR& csr, const Partition& part, int rank);
  // Generate this rank's shard of a synthetic graph directly on the device.
  static std::unique_ptr<DeviceGraph> generate(Backend& be, const GenParams& p, const Partition& part, int rank);
  // Build this rank's shard on the device from the edges this rank read (any
  // slice of the file, e.g. read_edge_shard): every edge's two entries are
  // routed to their owners (count -> all-to-all-v of (row, neighbour) pairs),
  // then count -> scan -> fill as generate().  Collective over `comm`.
  // input_edges: edges of the whole input (Graph500 TEPS numerator).
  static std::unique_ptr<DeviceGraph> from_edges(Backend& be, Comm& comm, const Partition& part, int rank,
                                                 int64_t input_edges, const vid_t* u, const vid_t* v,
                                                 int64_t m_local);
  // A file read in shards: edge list / MatrixMarket through read_edge_shard +
  // from_edges, a binary CSR cache through its rank's rows only.  Collective.
  static std::unique_ptr<DeviceGraph> from_file(Backend& be, Comm& comm, const std::string& path, int threads = 0);

  ShardView view() const;
  HostCSR to_host() const;  // the shard, copied back
  Backend& backend() const { return *be_; }
  const Partition& partition() const { return part_; }
  int rank() const { return rank_; }
  int64_t n() const { return part_.n; }
  int64_t lo() const { return lo_; }
  int64_t rows() const { return rows_; }
  int64_t nnz() const { return nnz_; }
  int64_t input_edges() const { return input_edges_; }
  std::vector<eid_t> degrees_of(const std::vector<int64_t>& local_rows) const;
  // Debug / tests: host copy of ShardView::nz_loc, one entry per non-empty
  // row (empty when the shard has no packed records).
  std::vector<uint16_t> debug_nz_loc() const;
  // Debug / tests: release the packed row records (nz_rec, nz_loc, unit_base)
  // as if a unit spanned 2^32 edges -- bottom-up then reads the non-empty-row
  // view and no level is hub-cut.  Call it on every rank, before the first run.
  void debug_drop_records();
  // Debug / tests: host copies of this rank's derived tables (ShardView), an
  // absent table empty: hub_vertex / hub_deg (nhubs entries), hub_bits
  // (Partition::global_words()), hub_col and td_col (nnz), td_hub_vertex
  // (td_nhubs entries), head (rows), nz_pref (words + 1), nz_row_off (non-empty
  // rows + 1), nz_head, nz_rec_off / nz_rec_head (NzRec's two fields), nz_loc,
  // unit_base (units + 1).  row_off and col: to_host().
  struct DebugTables {
    std::vector<vid_t> hub_vertex, hub_col, td_col, td_hub_vertex, head, nz_head, nz_rec_head;
    std::vector<uint32_t> hub_deg, nz_rec_off;
    std::vector<word_t> hub_bits;
    std::vector<eid_t> nz_pref, nz_row_off, unit_base;
    std::vector<uint16_t> nz_loc;
    int64_t td_nhubs = 0;
  };
  DebugTables debug_tables() const;
  // Reorder every row hub-first (neighbour degree descending); collective over
  // `comm` (all ranks need every vertex's degree).  One-time preprocessing.
  // With `hubs`, the (up to kMaxHubs) highest-degree vertices of the graph are
  // also indexed and every row head naming one is hub-encoded (ShardView).
  // With hubs and `id_order`, bottom-up keeps the hub-first order in its
  // hub-encoded copy and `col` is then put in neighbour-id order for the
  // top-down sweeps (neighbours of one row probe the bitmaps monotonically).
  // ... and with `td_hubs` also the hub-encoded top-down copy td_col (the
  // kTdMaxHubs highest-degree vertices encoded; one more nnz x 4 B).
  void sort_neighbors_by_degree(Comm& comm, bool hubs = true, int64_t max_hubs = kMaxHubs, bool id_order = true,
                                bool td_hubs = true);
  // The in-edge shard of a directed graph: for every owned vertex v the global
  // ids u of all stored entries u -> v of the whole graph, duplicates and
  // self-loops kept, every row in ascending u.  Built on the device from
  // `col` as it stands (any row order), collective over `comm`, one time: a
  // second call does nothing.  The owned out-entries are counted per owner of
  // their target, exchanged as (target << 32 | source) and built into rows by
  // count -> scan -> fill as from_edges, then sorted by id.  Transient: 16 B
  // per stored entry (send + receive), freed before return; resident: 4 B per
  // received entry + 8 B per row.  No heads, row records or hub encoding.
  void build_in_edges(Comm& comm);
  bool has_in_edges() const { return has_in_edges_; }
  // row_off, col, n, lo, rows and nnz of the in-edge shard; everything else unset
  ShardView in_view() const;
  HostCSR in_edges_to_host() const;  // the in-edge shard, copied back (tests)
  bool hub_sorted() const { return hub_sorted_; }
  // col is in id order (bottom-up must scan hub_col, whose order is hub-first)
  bool col_by_id() const { return col_by_id_; }
  // share of all adjacency entries held by the top-down hubs' rows (0 without
  // them): graphs whose hubs are only slightly above the mean degree (uniform
  // random graphs) gain nothing from the top-down hub filter
  double td_hub_share() const { return td_hub_share_; }
  // every rank's shard has the packed row records (agreed at the degree sort)
  bool rec_all() const { return rec_all_; }
  int64_t nhubs() const { return nhubs_; }
  // from_file: the byte range [begin, end) of the file this rank parsed and
  // the edges it read (a binary cache: rows, -1 bytes); -1 when not from a file
  struct IngestInfo {
    int64_t byte_begin = -1, byte_end = -1, edges = -1;
  };
  const IngestInfo& ingest() const { return ingest_; }

 private:
  IngestInfo ingest_;
  Backend* be_ = nullptr;
  Partition part_;
  int rank_ = 0;
  int64_t lo_ = 0, rows_ = 0, nnz_ = 0, input_edges_ = 0;
  bool hub_sorted_ = false;
  bool col_by_id_ = false;
  int64_t nhubs_ = 0;
  bool rec_all_ = false;  // every rank has the packed row records (rec_all())
  void build_heads(const uint32_t* hub_idx = nullptr);
  DBuf<vid_t> head_, hub_vertex_, nz_head_, hub_col_, td_col_, td_hub_vertex_;
  double td_hub_share_ = 0.0;
  DBuf<uint32_t> hub_deg_;  // ShardView::hub_deg
  DBuf<word_t> hub_bits_;  // global vertex bitmap of the hubs
  int64_t td_nhubs_ = 0;
  DBuf<eid_t> nz_pref_, nz_row_off_;
  DBuf<NzRec> nz_rec_;      // packed view records (empty when a unit spans >= 2^32 edges)
  DBuf<uint16_t> nz_loc_;   // ShardView::nz_loc (present exactly when nz_rec_ is)
  DBuf<eid_t> unit_base_;
  void build_nz_view();
  DBuf<eid_t> row_off_;
  DBuf<vid_t> col_;
  bool has_in_edges_ = false;
  int64_t in_nnz_ = 0;
  DBuf<eid_t> in_row_off_;
  DBuf<vid_t> in_col_;
};

struct EngineOptions {
  Mode mode = Mode::DirOpt;
  // Beamer's direction switch.  Defaults tuned on MI355X / RMAT-26 (sweeps in
  // profiles/): BU is cheap enough here that switching earlier than Beamer's
  // CPU value (14) pays.  alpha 40 (from 24, round 4): the same on the
  // bench's roots, +5 % on roots with a slower-growing frontier (a 64-root
  // tuning sample, seed 20261017; profiles/r4_final_alpha_sweep.txt), the
  // soc-LiveJournal1-sized graph unchanged.
  double alpha = 40.0;  // TD -> BU when m_f > m_u / alpha
  double beta = 384.0;  // BU -> TD when n_f < n / beta (and shrinking)
  // (384 since round 6, from 96: a shrinking frontier stays bottom-up
  // longer.  Asked to be a function of P -- a bottom-up level's cost per rank
  // shrinks with P, a sparse top-down level's does not -- the shadow replays
  // of RMAT-26 (ranks 0 and P - 1, four roots) found one value best at every
  // P: the late-switch roots' post-bottom-up level stays bottom-up (P = 8:
  // 103 -> 24 us), their traversals -12 % / -11 % / -19 % at P = 2 / 4 / 8,
  // early-switch ones unchanged, 768 and 1536 no better (profiles/
  // r6_policy_shadow_p*.txt); one GPU, 128 held-out roots, same box: 1498 /
  // 1494 -> 1506 / 1513 GTEPS (profiles/r6_beta_one_gpu_ab.txt).  alpha x 4
  // changed nothing at P = 8.)
  // neighbours a lane checks itself before rows go to wave-cooperative scans
  // (16: a first bottom-up level entered with a small frontier resolves more
  // rows per lane; RMAT-26 1240 -> 1259 GTEPS, 8 and 32 worse)
  int bu_lane_limit = 16;
  // Bottom-up waves take a whole 64-word unit (1), 16 words (-1), or by shard
  // size (0: whole units when they fill every resident wave slot).  Like
  // bu_small_waves, a shape choice of shards with packed row records: a shard
  // without them always runs 16 words per wave.
  int bu_whole_units = 0;
  // ... units split over waves (small shards): a first bottom-up level at 4
  // words per wave instead of 16 (1), never (-1), when 16 would leave wave
  // slots idle (0)
  int bu_small_waves = 0;
  // Top-down levels with at least this many local frontier edges mark
  // discoveries in a byte map (plain stores) instead of bitmap atomics.
  int64_t td_byte_edges = int64_t(1) << 22;
  // Device loop, one rank, narrow levels: top-down levels with at least
  // td_direct_edges frontier edges store the new level straight into the
  // one-byte level array of every unvisited candidate (no byte map, nothing
  // to clear; the update reads the level bytes back) -- cheaper than the
  // candidate bitmap's memory-side atomics from ~64 K edges (RMAT-26: a
  // 1.7 M-edge level 115 -> 68 us).  Replaces td_byte_edges there.
  static constexpr bool td_direct = true;
  int64_t td_direct_edges = int64_t(1) << 16;
  // Device loop, one rank: top-down levels predicted to have at least this
  // many frontier edges run binned (BinArgs: targets binned by vertex range,
  // claimed per bin in LDS, settled and the level ended by the same apply
  // kernel) instead of td_expand + update; 0 disables.  Only
  // on graphs of at least td_bin_min_rows vertices (level bytes and visited
  // bits far past the L2: a direct level's two random lines per edge go to
  // HBM; below, the direct level is faster -- RMAT-22 top-down) and only
  // before the run's first bottom-up level (the shrinking levels after it are
  // predicted from a falling frontier and are mostly far smaller).
  // Measured, RMAT-26 per root: a 28 M-edge second-level expansion 556 ->
  // 402 us; 1354 -> 1368 GTEPS with the bottom-up gate missing (post-bottom-up
  // levels of 200 K edges predicted at 2 M: 58 -> 80 us).
  // Not for levels the direct form does better since split top-down levels
  // (DeviceLoop::td_form): RMAT-26 top-down only 39.1 GTEPS binned against
  // 67.7 direct and split (its 0.5 B-edge level 5.6 -> 5.0 ms, the next one,
  // with the unvisited filter, 21.3 -> 10.8 ms; profiles/r5_td_binned_off_ab.txt).
  int64_t td_bin_edges = int64_t(1) << 21;
  // (2^26: RMAT-24, 2^24 vertices, measured 2 % slower binned -- 785 / 793
  // against 815 / 800 GTEPS; RMAT-26 +2-4 %; RMAT-27 flat)
  int64_t td_bin_min_rows = int64_t(1) << 26;
  // ... about 2^td_bin_log2_bins bins (of >= 4096 vertices, at most
  // kBinMaxBins; each bin's visited slice must fit LDS).  RMAT-26, the 28 M-edge
  // binned level: 256 / 512 / 1024 bins 407 / 417 / 441 us with the scatter
  // fill (more bins: more open lines); with the staged fill 256 / 512 bins
  // 340 / 357 us (profiles/binned_settle_fill_sweep.txt).
  static constexpr int64_t td_bin_log2_bins = 8;
  // Dense top-down levels predicted at >= td_unvis_edges frontier edges that
  // start with >= td_unvis_vis_frac of the adjacency visited test targets in
  // an LDS unvisited filter first (UnvisArgs, TdArgs::unvis): a clear bit
  // means visited, so only the rest cost a scattered `visited` probe.  0
  // disables.
  int64_t td_unvis_edges = int64_t(1) << 22;
  double td_unvis_vis_frac = 0.6;
  // ... such a level runs with the filter iff at most this fraction of the
  // filter's bits are set (decided on the device from the built filter)
  double td_unvis_max_density = 0.5;
  // One rank, level-byte (level_direct) top-down levels predicted at >=
  // td_split_edges frontier edges run in td_split_parts parts (twice as many
  // from 16 x td_split_edges on graphs of >= 2^25 vertices: a smaller graph's
  // predicted level overshoots, and RMAT-22 runs 3 % slower in 8), the claims of the parts so far ORed into
  // `visited` between them (refresh_visited): a target reached by many
  // frontier edges stores its level byte about once per part instead of once
  // per edge.  0 disables.  RMAT-22 top-down only 98.5 -> 105.7 GTEPS (8 parts:
  // 103); RMAT-26 top-down only 55.8 -> 67.7 (its 0.5 B-edge level 9.4 -> 5.0
  // ms; 8 parts 69.5): profiles/r5_td_split_levels_ab.txt.
  int64_t td_split_edges = int64_t(1) << 23;
  int td_split_parts = 4;
  // Dense top-down levels with at least this many frontier edges test hub
  // targets in an LDS copy of the hubs' visited bits (ShardView::td_col);
  // 0 disables.
  // (RMAT-22 top-down-only, per root: levels of 75-90 M edges 440-511 ->
  // 397-474 us, the 43-58 M-edge levels before the visited fraction is
  // reached unchanged; below ~16 M edges the hub snapshot and its LDS staging
  // cost what they save)
  int64_t td_hub_edges = int64_t(1) << 24;
  // ... once the visited vertices hold this fraction of the adjacency.
  // Without hub marks (TdArgs::td_hub_mark: direct-level top-down claims a
  // hub target as one byte of an L2-resident 128 KiB array, hub_apply turns
  // the marks into level bytes after the expansion) 0, i.e. also the earlier
  // big levels, was slower (58.9 against 63.5 GTEPS: decoding unvisited hubs
  // costs a dependent load); with them 0 is faster (69.0 against 65.9).
  double td_hub_vis_frac = 0.0;
  // ... only on graphs whose top-down hubs hold at least this share of the
  // adjacency entries (DeviceGraph::td_hub_share)
  static constexpr double td_hub_min_share = 0.0;
  // Byte-map levels skip the visited pre-check while the visited vertices
  // hold less than this fraction of all adjacency entries.
  double td_check_visited_min = 0.02;
  // Top-down grids of fewer workgroups than this use 1024-thread workgroups.
  int64_t td_wide_below_blocks = 2048;
  // Multi-rank top-down levels whose global frontier has at most this many
  // edges exchange owner lists instead of bitmap slices.
  int64_t sparse_max_edges = int64_t(1) << 17;
  // ... and only when the lists are smaller than half a bitmap slice (tests
  // switch this off to exercise the list path on small graphs).
  bool sparse_size_check = true;
  bool phase_timing = false;  // per-level device timing (adds events)
  // td/bu/do modes: device-driven level loop (LevelCtrl): the host enqueues
  // the next level before the current one finishes.  With several ranks each
  // level's chain carries its collectives (frontier all-gather, candidate
  // all-to-all, totals all-reduce), enqueued ahead like the kernels;
  // level_finish decides on the reduced totals.
  bool device_loop = true;
  // ... enqueueing each level with an extrapolated direction prediction (else:
  // the previous level's direction, one more level ahead).
  bool device_loop_predict = true;
  // Device loop: top-down levels whose frontier is predicted to have at most
  // this many edges run as one sparse kernel (TdSparseArgs: direct claims, work list
  // handed to the next level) instead of compact + td_expand + update + scan;
  // 0 disables.  td_sparse_grid: its workgroups (RMAT-26, 256 / 512 / 1024:
  // 1504-1509 / 1506-1509 / 1492-1503 GTEPS held-out, profiles/r6_sparse_grid_ab.txt).
  int64_t td_sparse_edges = int64_t(1) << 16;
  static constexpr int64_t td_sparse_grid = 256;
  // ... several ranks: the owners' side (td_sparse_apply) at most this many
  // workgroups (sized by the level's expected received ids, ~512 each; only
  // those with ids take part).  Shadow rank 0 of RMAT-26 at P = 2, the 1.3
  // M-edge sparse level: 128 workgroups 91 us, 512 81 us.
  static constexpr int64_t td_apply_grid = 512;
  // A sparse chain stays live up to td_sparse_cap_factor x td_sparse_edges
  // frontier edges (0: any size); a larger level is re-enqueued dense.
  static constexpr double td_sparse_cap_factor = 8.0;
  // Device loop: workgroups of the dense top-down expansion grid (at most;
  // they stride over the level's edge blocks; the launcher also caps the grid
  // at the kernel's residency), without and with the hub filter.  Measured:
  // RMAT-26 (no filter levels) 1024 workgroups 1354 / 1334 against 1323 /
  // 1318 GTEPS at 2048; RMAT-22 top-down only (filter levels) 1024 / 1280 /
  // 1536 (= residency) 77 / 81 / 83 GTEPS.
  static constexpr int64_t td_grid_max = 1024;
  static constexpr int64_t td_grid_filter_max = 2048;
  // The sparse threshold for the first top-down level after a bottom-up one
  // (the extrapolated prediction of a shrinking frontier overshoots), and
  // how far such a chain stays live.  RMAT-26: the late-switch roots' level
  // after three bottom-up levels (0.2-0.6 M edges, predicted 2-6 M) 52-58 ->
  // 19-28 us sparse; a shared cap (td_sparse_cap_factor) would also keep
  // mispredicted early chains sparse (measured: 112 -> 331 us).
  static constexpr int64_t td_sparse_bu_edges = int64_t(1) << 23;
  // ... and that level reads the bottom-up level's output bitmap itself
  // (TdSparseArgs::from_bits: one kernel after a clear of its output bitmap,
  // instead of scan_units + compact + td_sparse).
  bool td_sparse_bits = true;
  // Device loop, several ranks: sparse top-down levels (td_sparse with owner
  // lists, the lists exchanged count-sized, td_sparse_apply on the owners)
  // for levels predicted at <= xsparse_edges global frontier edges; such a
  // chain stays live up to list_form_edges (the owner lists' capacity: P x
  // that many ids per rank, twice) and a larger level is re-enqueued dense.
  // 0 disables (dense top-down chains only).
  int64_t list_form_edges = int64_t(1) << 21;
  int64_t xsparse_edges = int64_t(1) << 20;
  // ... levels predicted at <= xfuse_edges (a chain then live up to 4x that):
  // with a direct exchange and a folded level end, td_sparse's last workgroup
  // runs the owner side too (TdSparseArgs::fuse_apply: one launch per level);
  // 0 disables.  (Validated over the peer transport with 4 processes on one
  // GPU, tests/test_gpu_engine.py::test_peer_multirank_options; shadow rank 0
  // of RMAT-26 at P = 8: level 0 11-19 -> 6-10 us.)
  int64_t xfuse_edges = int64_t(1) << 12;
  // Several ranks, bottom-up levels: merge the gathered frontier into the
  // replicated visited bitmap (the remote slices; folded into hub_gather).
  // Only top-down levels read remote visited bits, as a filter: a stale one
  // sends an id its owner drops, so the levels stay exact without it -- but
  // the top-down level after the bottom-up ones then claims and sends every
  // remote target the bottom-up levels reached.  Shadow rank 0 of RMAT-26
  // (profiles/r5_shadow_ab_merge_apply_grid.txt): that level 51-67 -> 21-24
  // us at P = 2 for 3-5 us per bottom-up level; traversal -6.6 % at P = 2,
  // -3.6 % at P = 8.
  bool bu_merge_visited = true;
  // Device loop, hubs: a first bottom-up level whose frontier has at most
  // bu_cut_edges edges outside the hubs claims those vertices' neighbours
  // top-down (bu_cut_prep) and scans only the rows' hub prefixes
  // (BuArgs::cut_edges) -- the late-switch level, whose frontier is a few
  // thousand vertices, mostly hubs.  0 disables.
  int64_t bu_cut_edges = int64_t(1) << 22;
  // ... with several ranks too, up to this many: every rank claims its own
  // non-hub frontier's neighbours, the remote ones in the byte map, packed
  // and sent to their owners as one bitmap all-to-all (bu_cut_merge applies
  // them) -- the top-down part shrinks with P as the bottom-up share does.
  // (Round 4's form sent the remote claims as owner lists and measured
  // slower at P = 8.)  Shadow replays of RMAT-26's late-switch roots
  // (profiles/r6_xcut_shadow_ab.txt, traversal us per rank): P = 2
  // 602-766 -> 530-620, P = 4 393-508 -> 397-453, P = 8 270-334 ->
  // 298-345 -- the cut's fixed launches (decision, top-down part, 64 MB byte
  // map pack, all-to-all, merge) outweigh what it saves a rank's 1/8 share
  // of the bottom-up scan at P = 8, so it stops at 4.
  int64_t bu_cut_ranks = 4;
  // ... enqueued (its decision and top-down launches) only for levels
  // predicted at <= bu_cut_mf_frac of the graph's directed edges (RMAT-26:
  // the late-switch first bottom-up levels have 4-15 % of them, the others
  // 37 % and more)
  double bu_cut_mf_frac = 0.25;
  // ... on a transport that ships the lists' capacity (RCCL / TCP fallback;
  // the peer windows ship their lengths), a chain's lists hold
  // list_cap_factor x the predicted edges (a power of two >= 1024)
  double list_cap_factor = 4.0;
  // Several ranks, a level whose frontier is all-gathered for a bottom-up
  // level next (graphs with hubs): the producing kernels push their output
  // words straight into the peers' windows (Comm::direct_frontier) and the
  // bottom-up level's hub_gather copies them in -- the level end carries only
  // its totals (and may fold into the bottom-up kernel): the frontier
  // exchange overlaps the kernels that produce it instead of following them.
  bool direct_frontier = true;
  // Bitmap engine (td / bu / do): levels kept in a one-byte-per-vertex array
  // during the traversal (a quarter of the per-run initialisation traffic),
  // widened to 32 bits when read; a traversal deeper than kNarrowMaxLevel is
  // rerun with 32-bit levels (and later runs keep them).
  bool narrow_levels = true;
  // Take the multi-rank exchange path (alltoall / allgather / alltoallv) even
  // with one rank: lets a 1-rank RCCL communicator exercise every collective
  // call on a single GPU (tests).
  bool force_exchange = false;
  // Directed input (CSR holds out-edges only): top-down modes only for run();
  // vertices without out-edges are not pre-marked visited; traversed edges =
  // out-edges of the reached vertices.  run_batch, validate and the parent
  // trees build the graph's in-edge shard on their first call
  // (DeviceGraph::build_in_edges, or Engine::build_in_edges up front).
  bool directed = false;
  // run_batch(betweenness / keep_path_counts): rows of more than this many
  // entries are walked by a workgroup of 16 waves in a launch of their own
  // (MsBcArgs::long_rows) instead of by one wave; 0: never.
  int64_t bc_split_row = 512;
  // components(): one rank, undirected -- hook only the first
  // cc_sample_entries entries of every row, take the most frequent label of a
  // vertex sample, and skip that component's rows in the pass over the
  // remaining entries (Afforest's subgraph sampling; the rows are degree-
  // sorted, so the first entries are the hubs).  0: one pass over every entry,
  // which directed graphs and several ranks always run.
  int64_t cc_sample_entries = 2;
  // strong_components(): trim sweeps per round at most (-1: to the fixed
  // point; 0: no trim), and whether the first round colours only a pivot (the
  // live vertex with the largest in-degree x out-degree) instead of every vertex.
  int64_t scc_trim_rounds = -1;
  bool scc_pivot = true;
};

// Named access to the numeric tuning options (alpha, beta, bu_lane_limit,
// td_byte_edges, td_wide_below_blocks, td_check_visited_min, sparse_max_edges,
// sparse_size_check, force_exchange, phase_timing); throws on unknown names.
void set_engine_option(EngineOptions& o, const std::string& name, double value);
std::vector<std::pair<std::string, double>> engine_option_map(const EngineOptions& o);

struct LevelRecord {
  int level = 0;
  char direction = 'T';  // 'T' top-down, 'B' bottom-up, 'R' reference, 'S' simple, 'C' scan
  int64_t frontier = 0;       // global frontier vertices expanded at this level
  int64_t frontier_edges = 0; // global sum of their degrees
  int64_t discovered = 0;     // global new vertices
  double ms = 0.0;            // device time of the level (phase_timing only)
  double comm_ms = 0.0;       // ... of which in collectives (host loop, phase_timing only)
  // Device loop, device clock: idle time between the previous level's scan
  // and this level's first kernel (launch gaps; -1 when unknown).
  double gap_ms = -1.0;
};

// One level chain the device loop enqueued (mispredicted ones included):
// form 'T' dense top-down, 'S' sparse top-down (`cap`: the global frontier
// edges it stays live for; several ranks: its owner lists' capacity), 'X'
// binned top-down, 'B' bottom-up; `gather` (several ranks): the chain's
// collective also all-gathered its output frontier.
struct ChainRecord {
  int level = 0;
  char form = 'T';
  int64_t cap = 0;
  bool gather = false;
  // several ranks: its output frontier pushed by its kernels (no gather in
  // its level end; EngineOptions::direct_frontier)
  bool push = false;
  // a dense top-down chain with the unvisited filter (TdArgs::unvis)
  bool unvis = false;
  // ... run in this many parts (TdArgs::split_k; 1: whole)
  int split = 1;
  // a bottom-up chain with the hub cut's launches (decided on the device)
  bool cut = false;
};

struct RunResult {
  int64_t source = 0;
  double ms = 0.0;             // wall time of the traversal (max over ranks)
  int64_t reached = 0;         // vertices reached (global)
  int64_t edges = 0;           // traversed undirected edges (Graph500)
  // number of levels (max level + 1).  A directed graph: the levels expanded
  // -- one fewer when no vertex of the deepest level has an out-edge (the
  // frontier counts vertices with edges only); BatchResult::depth counts that
  // level too.
  int depth = 0;
  double gteps = 0.0;
  int mispredicts = 0;         // device loop: level chains enqueued for the wrong direction
  std::vector<LevelRecord> levels;
  std::vector<ChainRecord> chains;  // device loop: every chain enqueued, in order
};

// Concurrent multi-source BFS (Engine::run_batch): which form a level takes.
// Auto decides per level (one rank; several ranks: every level is a pull);
// Alternate is push on even levels and pull on odd ones (tests: both
// transitions on every graph).
enum class BatchDirection { Auto, Push, Pull, Alternate };
BatchDirection parse_batch_direction(const std::string& s);

// The number format of a batch's shortest-path counts (betweenness /
// keep_path_counts).  Double: doubles, a count past DBL_MAX fails the batch.
// Wide: dbfs/wide.hpp's mantissa and exponent in every pass, no range error.
// Auto: a pass runs in doubles and, if its forward sweep overflowed, its
// sweeps are redone wide.
enum class BatchCounts { Double, Wide, Auto };
BatchCounts parse_batch_counts(const std::string& s);

// What a batch does besides the traversal (Engine::run_batch describes each).
struct BatchOptions {
  BatchDirection direction = BatchDirection::Auto;
  bool keep_levels = true;
  bool validate = false, keep_parents = false;
  bool betweenness = false, keep_path_counts = false;
  BatchCounts counts = BatchCounts::Double;
};

// One level of one pass: form 'P' push, 'L' pull; the active vertices it
// expanded and the sum of their degrees (global).
struct BatchLevelRecord {
  int pass = 0, level = 0;
  char form = 'L';
  int64_t active = 0, edges = 0;
  double ms = 0.0;  // host wall time from the level's enqueue to its totals
};

struct BatchResult {
  std::vector<int64_t> sources;
  double ms = 0.0;     // wall time of all passes (max over ranks)
  double gteps = 0.0;  // sum of edges / ms
  int passes = 0;      // ceil(k / 64)
  // the level matrix is 16-bit: a pass (of this batch or an earlier one) was
  // deeper than one-byte levels hold and was rerun
  bool wide_levels = false;
  // per source, in the order given
  // edges: degree sum of the reached / 2; directed graphs: their out-degree
  // sum, not halved (RunResult::edges' convention)
  std::vector<int64_t> reached, edges, dist_sum;
  // levels (max level + 1), the deepest level counted on a directed graph too
  // (RunResult::depth there: the levels expanded)
  std::vector<int> depth;
  std::vector<std::vector<int64_t>> discovered;   // [source][level]
  std::vector<BatchLevelRecord> levels;
  // run_batch(validate): per source, in the order given, the device check's
  // (depth-gap, reached-unreached, orphan) counts, [k][3] row-major, summed
  // over ranks (all must be 0); empty when not asked for
  std::vector<int64_t> violations;
  // wall time of the per-pass checks (validate / keep_parents; max over
  // ranks): after each pass's timed window, never part of `ms`.  Several
  // ranks: the all-gather of the pass's level matrix is part of it (without a
  // check: of bc_ms and bc_forward_ms)
  double check_ms = 0.0;
  // run_batch(betweenness / keep_path_counts): wall time of the per-pass path
  // counts and dependency accumulation (max over ranks), after each pass's
  // timed window and its check: never part of `ms` or `check_ms`.  Its
  // forward (init and path counts, the counts' copy included) and backward
  // (dependencies) parts; the launches of all passes (one per level and
  // direction) and the rows they walked on this rank (those with a source on
  // the launch's level: launches x owned rows without that skip).
  double bc_ms = 0.0, bc_forward_ms = 0.0, bc_backward_ms = 0.0;
  int64_t bc_launches = 0, bc_rows_walked = 0;
  // the passes whose counts ran in the wide form (BatchCounts::Wide: all;
  // Auto: those redone -- their double sweeps' time, launches and rows are in
  // the figures above too)
  int wide_count_passes = 0;
};

// Engine::components.  sample_entries < 0: EngineOptions::cc_sample_entries.
struct ComponentsOptions {
  int64_t sample_entries = -1;
};

struct ComponentsResult {
  int64_t components = 0;      // connected components (weakly connected, on a directed graph)
  int64_t largest_label = -1;  // the largest one's label (its smallest vertex; the smaller label on a tie)
  int64_t largest_size = 0;
  int64_t singletons = 0;      // components of one vertex
  double ms = 0.0;             // wall time, max over ranks: link_ms + compress_ms + the sizes
  double link_ms = 0.0;        // the hook launches (several ranks: the label exchange too)
  double compress_ms = 0.0;    // the pointer-jumping launches
  bool sampled = false;        // the sample-and-skip form ran
};

// Engine::strong_components.  trim_rounds < -1 / pivot < 0: the engine options
// scc_trim_rounds / scc_pivot.
struct SccOptions {
  int64_t trim_rounds = -2;
  int pivot = -1;
};

struct SccResult {
  int64_t components = 0;      // strongly connected components
  int64_t largest_label = -1;  // the largest one's label (its smallest vertex; the smaller label on a tie)
  int64_t largest_size = 0;
  int64_t singletons = 0;      // components of one vertex
  int64_t trimmed = 0;         // vertices the trim settled (<= singletons)
  int64_t rounds = 0;          // colouring rounds (<= n)
  int64_t sweeps = 0;          // sweep launches of all three steps
  int64_t pivot = -1;          // the first round's pivot (-1: none)
  int64_t pivot_size = 0;      // ... and the size of its component
  double ms = 0.0;             // wall time, max over ranks
  double trim_ms = 0.0;        // the trim sweeps
  double colour_ms = 0.0;      // the colouring rounds (forward and backward sweeps)
};

// Engine::eccentricities.
struct EccOptions {
  EccTarget target = EccTarget::All;
  // the vertices the call answers for: kLargest the largest connected
  // component, kAll every vertex, a value >= 0 the component with that label
  static constexpr int64_t kLargest = -2, kAll = -1;
  int64_t component = kLargest;
  int64_t max_passes = -1;  // < 0: no cap
};
EccTarget parse_ecc_target(const std::string& s);

struct EccResult {
  // the largest lower bound / the smallest upper bound over the scope: with
  // target All and exact, the diameter and the radius; target Diameter
  // promises `diameter` only (radius is then an upper bound), Radius `radius`
  // only (diameter a lower bound)
  int64_t diameter = 0, radius = 0;
  int64_t centre = 0;      // settled vertices with eccentricity == radius
  int64_t periphery = 0;   // ... == diameter
  int64_t passes = 0;      // batch passes run
  int64_t sources = 0;     // traversals in them
  int64_t settled = 0;     // in-scope vertices whose bounds met
  int64_t scope_size = 0;
  bool exact = false;      // the loop ended by itself, not by max_passes
  bool wide_levels = false;
  double ms = 0.0;         // wall time, max over ranks: the three parts and the set-up
  double bfs_ms = 0.0;     // the batch passes (several ranks: the matrix all-gather too)
  double bound_ms = 0.0;   // ecc_update and ecc_totals
  double select_ms = 0.0;  // ecc_select and its copy to the host
};

// Fault injection for failure-detection tests (see Engine::inject_fault).
struct FaultSpec {
  int rank = -1, level = -1;
  std::string kind = "throw";  // FaultSpec::from_env lists the kinds
  int ms = 2000;  // kind=delay: how long the rank sleeps before enqueueing the level
  int us = 500;   // kind=late_wg: how long td_sparse's ticket-less workgroups wait (TdSparseArgs::late_ticks)
  CheckFile file = CheckFile::Bfs;  // kind=device: the kernel file whose word records it (file=td_kernels|bu_kernels)
  static FaultSpec from_env();
};

class DeviceLoop;  // the device-driven level loop (csrc/engine/device_loop.cpp)

class Engine {
 public:
  Engine(DeviceGraph& g, Comm& comm, const EngineOptions& opt = {});
  ~Engine();
  RunResult run(int64_t source);
  // Owned slice of the last run's levels.
  std::vector<lvl_t> levels_local() const;
  // Full level array (all ranks participate).
  std::vector<lvl_t> gather_levels();
  // Graph500-style device validation of the last run; returns violation counts
  // {depth-gap, reached-unreached, orphan} summed over ranks (all must be 0).
  std::vector<int64_t> validate(int64_t source);
  // Graph500 parent tree of the last run (global vertex ids; -1 unreached):
  // owned slice, and the full array (all ranks participate in both).
  std::vector<int64_t> parents_local(int64_t source);
  std::vector<int64_t> gather_parents(int64_t source);
  // Concurrent traversal from all `sources`, 64 per pass (one bit per source
  // in a 64-bit word per vertex); collective.  The single-source state (run)
  // is not touched.  keep_levels: the per-source levels are kept for
  // gather_batch_levels (64 bytes per vertex on the device).
  // validate: every pass's level matrix is checked on the device against
  // every edge, all its sources at once (Backend::ms_check; Graph500's level
  // rules as in validate()), after the pass's timed window: BatchResult::
  // violations, check_ms.  keep_parents: the same walk also leaves every
  // source's parent tree for gather_batch_parents (256 bytes per owned vertex
  // on the device during the check, k x 8 bytes per owned vertex on the host).
  // Both need keep_levels.  Several ranks: the owned slices of the matrix are
  // all-gathered for the check, as gather_batch_levels does.
  // betweenness: after each pass (and its check) the shortest-path counts and
  // Brandes' dependencies of its sources are computed on the device from the
  // level matrix (Backend::ms_bc_*, one launch per level and direction) and
  // summed into one vector for gather_betweenness (512 + 8 bytes per owned
  // vertex on the device).  keep_path_counts: the same forward sweep also
  // leaves every source's path counts for gather_batch_path_counts (k x n x 8
  // bytes on the host).  Both need keep_levels; BatchResult::bc_ms.  Several
  // ranks: the simple form -- the value matrix is replicated and the owned
  // lines are all-gathered after every launch.
  // Path counts are doubles: a batch in which a source has more than DBL_MAX
  // (~2^1024) shortest paths to some vertex throws after that pass's forward
  // sweep, on every rank, naming the first such source, and leaves no result
  // -- BatchOptions::counts = Double, the default.  Wide runs every pass with
  // extended-range counts and coefficients (a mantissa and an exponent,
  // MsBcArgs::wide: 768 + 8 bytes per owned vertex, allocated on first use)
  // and never fails for range; Auto runs a pass in doubles and redoes its
  // sweeps wide when the overflow mask, agreed across the ranks, is set.
  // BatchResult::wide_count_passes.  The dependency sums are doubles in every
  // form: a source's share below 2^-1074 counts as 0.  Kept path counts are
  // held as mantissa and exponent whenever counts is not Double.
  BatchResult run_batch(const std::vector<int64_t>& sources, const BatchOptions& o = {});
  // The last batch's dependency sums, one per vertex: dep(v) = the sum over the
  // source slots i with v != src_i of delta_{src_i}(v) -- raw: not halved on
  // an undirected graph, not rescaled, not normalised; collective.  Throws
  // when the batch ran without betweenness.
  std::vector<double> gather_betweenness();
  // The last batch's shortest-path counts, [k][n] row-major (0 where source k
  // does not reach; exact while below 2^53).  Throws when the batch ran
  // without keep_path_counts.
  // After a Wide or Auto batch: the same doubles when every count fits one,
  // an error naming gather_batch_path_counts_wide otherwise.
  std::vector<double> gather_batch_path_counts();
  // The same counts as mant * 2^exp, [k][n] each, in frexp's convention (mant
  // in [0.5, 1); (0.0, 0) for 0), after a batch of any counts form.
  void gather_batch_path_counts_wide(std::vector<double>& mant, std::vector<int32_t>& exp);
  int64_t batch_path_count_sources() const { return kept_.counts_k; }  // (-1: none)
  // The last batch's levels, [k][n] row-major, kUnreached where source k does
  // not reach; collective.  Throws when the batch ran without keep_levels.
  std::vector<lvl_t> gather_batch_levels();
  // Directed graphs: build the in-edge shard now (collective; a no-op when it
  // exists or the graph is undirected) instead of on the first call that
  // needs it.
  void build_in_edges();
  // The last batch's parent trees, [k][n] row-major, with gather_parents'
  // convention per source (parent[src] = src, -1 unreached); collective.
  // Throws when the batch ran without keep_parents.
  std::vector<int64_t> gather_batch_parents();
  int64_t batch_parent_sources() const { return kept_.parents_k; }  // of the last batch with parents (-1: none)
  // The count form of the check once more, on the level matrix still resident
  // from the last pass of the last batch, against `sources` (as many as that
  // pass had, at most 64): [k][3] as BatchResult::violations; collective.
  std::vector<int64_t> validate_batch_pass(const std::vector<int64_t>& sources);
  // Connected components of the whole graph on the device; collective.
  // label[v] = the smallest vertex id of v's component; a directed graph: the
  // weakly connected components (an entry u -> v joins u and v).  A hook-and-
  // compress forest over the owned rows (Backend::cc_*): one pass over the
  // entries and a pointer-jumping compress, not a traversal per component.
  // One rank, undirected, sample_entries > 0: the sample-and-skip form
  // (EngineOptions::cc_sample_entries).  Several ranks, the simple form: every
  // rank links its rows into its own full-length label array, the arrays are
  // all-gathered (in pieces) and each rank hooks every peer's (v, label[v])
  // pairs into its own -- every rank ends with the same array.  The labels do
  // not depend on the form, the rank count or the run.  Device state: 4 B per
  // vertex of the whole graph for the labels and 4 B for the sizes, allocated
  // by the first call and kept; apart from run / run_batch / validate state.
  ComponentsResult components(const ComponentsOptions& o = {});
  // The last components() call's labels, and every vertex's component size,
  // for all n vertices (this rank's replica: no communication).  Throw when
  // components() has not run.
  std::vector<int64_t> gather_components();
  std::vector<int64_t> gather_component_sizes();
  bool has_components() const { return cc_ && cc_->valid; }
  const ComponentsResult& last_components() const;
  // Strongly connected components of the whole graph on the device;
  // collective.  label[v] = the smallest vertex id of v's strongly connected
  // component (an undirected graph: its connected components).  Rounds of
  // trim, forward colouring over the in-edge rows and backward closure over
  // the out-rows (Backend::scc_*; csrc/engine/strong_components.cpp), every
  // "until nothing changes" loop on the host over a device counter, no
  // traversal per component.  A directed graph's in-edge shard is built by the
  // first call if it is not there.  Several ranks, the simple form: every rank
  // holds the state of all n vertices, a sweep writes its owned rows' entries
  // and the owned slices are all-gathered after every sweep -- correct, not
  // fast.  Device state: 12 B per vertex of the whole graph (label, class,
  // colour) and 4 B for the sizes, allocated by the first call and kept; apart
  // from run / run_batch / validate / components state.
  SccResult strong_components(const SccOptions& o = {});
  // The last strong_components() call's labels, and every vertex's component
  // size, for all n vertices (this rank's replica: no communication).  Throw
  // when strong_components() has not run.
  std::vector<int64_t> gather_strong_components();
  std::vector<int64_t> gather_strong_component_sizes();
  bool has_strong_components() const { return scc_ && scc_->valid; }
  const SccResult& last_strong_components() const;
  // Exact eccentricities by bounding (Takes and Kosters); collective,
  // undirected graphs only.  ecc(v) = the largest distance from v within its
  // connected component (0 for a vertex without neighbours; stored duplicates
  // and self-loops change nothing).  A loop of batch passes
  // (csrc/engine/eccentricity.cpp): select at most 64 live sources on the
  // device (Backend::ecc_select), traverse from all of them at once
  // (run_batch_pass, levels kept), tighten every live vertex's bounds from
  // the pass's level matrix (Backend::ecc_update: a source s with eccentricity
  // e at distance d gives max(d, e - d) <= ecc(v) <= e + d), until every
  // in-scope vertex is settled (target All) or the target's value is known.
  // Every pass settles at least its own sources, so the loop ends; max_passes
  // ends it early with exact = false and valid bounds.  components() runs
  // first if the scope needs its labels and it has not run.  Several ranks,
  // the simple form: pass_matrix all-gathers the level matrix, every rank
  // holds and updates the bounds of all n vertices and so selects the same
  // sources with no further exchange -- correct, not fast.  Device state: 16 B
  // per vertex of the whole graph (lo, hi, state, degree), allocated by the
  // first call and kept; apart from run / validate / components state.  The
  // call uses the batch buffers: it collects a pending batch's levels first,
  // and its passes replace the resident batch pass (validate_batch_pass then
  // needs a new run_batch).
  EccResult eccentricities(const EccOptions& o = {});
  // The last eccentricities() call's bounds for all n vertices (this rank's
  // replica: no communication): lo and hi, (-1, -1) out of scope, hi =
  // INT32_MAX where no source reached the vertex; and the eccentricities, -1
  // where out of scope or unsettled.  Throw when eccentricities() has not run.
  void gather_eccentricity_bounds(std::vector<int32_t>& lo, std::vector<int32_t>& hi);
  std::vector<int32_t> gather_eccentricities();
  bool has_eccentricities() const { return ecc_ && ecc_->valid; }
  const EccResult& last_eccentricities() const;
  // Test hook: overwrite source slot `slot`'s level of global `vertex` in the
  // resident level matrix (on its owner; level < 0: unreached), so a test can
  // plant a violation for validate_batch_pass to find.
  void debug_set_batch_level(int slot, int64_t vertex, int level);
  // Test hook: overwrite the last run's level of global `vertex` (on its
  // owner; level < 0: unreached), so a test can plant a violation for
  // validate() and parents_local() to find.
  void debug_set_level(int64_t vertex, int level);
  int64_t batch_sources() const { return kept_.k; }  // of the last batch with levels (-1: none)
  int64_t global_directed_edges() const { return total_directed_; }
  const EngineOptions& options() const { return opt_; }
  void set_options(const EngineOptions& o) {
    opt_ = o;
    frontier_clean_ = false;  // (the next traversal may take another path: it clears its frontier itself)
  }

 private:
  friend class DeviceLoop;
  RunResult run_bitmap(int64_t source);
  RunResult run_bitmap_device(int64_t source);
  bool use_device_loop() const;
  RunResult run_ref(int64_t source);
  void alloc_bitmap_state();
  void begin_run_scratch();
  InitRunArgs init_args(int64_t source, word_t* seed_frontier, LevelCtrl* ctrl, const LevelCtrl& ctrl_init,
                        LevelMailbox* mailbox);
  // Where a level's new vertices get new_level: the narrow array on a narrow
  // run (the one place that decides it), else the 32-bit one.
  LevelOut level_out(lvl_t new_level) const {
    return {level_.data(), run_narrow_ ? level8_.data() : nullptr, narrow_base_, new_level};
  }
  bool scratch_dirty_ = true;  // cand / next / byte map may hold stale bits
  bool frontier_clean_ = false;  // the owned frontier slices are zero (InitRunArgs::frontier_clean)
  void alloc_ref_state();
  void gather_levels_device(DBuf<lvl_t>& full);
  bool exchange() const { return part_.nranks > 1 || opt_.force_exchange; }
  void inject_fault(int level);
  void inject_batch_fault(int level);  // kind=batch_device, at level `level` of a batch pass
  void check_device();

  DeviceGraph& g_;
  Comm& comm_;
  Backend& be_;
  EngineOptions opt_;
  Partition part_;
  FaultSpec fault_;
  int64_t total_directed_ = 0;

  DBuf<lvl_t> level_;
  DBuf<uint8_t> level8_;
  DBuf<uint32_t> td_group_ticket_;  // UpdateArgs::group_ticket
  DBuf<int64_t> bu_tot_;  // fused bottom-up finish: per-workgroup totals (BuArgs::tot)
  DBuf<int64_t> td_tot_;  // fused top-down finish: the level's totals (UpdateArgs::tot)
  DBuf<uint8_t> td_hub_mark_;  // TdArgs::td_hub_mark (kTdMaxHubs bytes; zero between levels)
  bool level8_filled_ = false;        // level8_ reads unreached for the current run without a fill
  uint8_t narrow_base_ = 0;           // the current run's level byte base (kNarrowEpochs)
  int64_t narrow_run_ = 0;            // narrow runs since level8_ was allocated
  bool narrow_failed_ = false;        // a traversal overflowed the narrow levels
  bool run_narrow_ = false;           // the current run writes level8_
  mutable bool levels_narrow_ = false;  // level_ is stale: level8_ holds the last run's levels
  bool use_narrow() const;
  void ensure_wide_levels() const;
  // bitmap engine state
  bool bitmap_ready_ = false;
  DBuf<word_t> visited_, zdeg_, frontier_[2], next_, recv_, cand_, hub_front_, td_hub_vis_, unvis_;
  DBuf<uint32_t> unvis_pop_;
  DBuf<uint32_t> deg_all_;  // several ranks: every vertex's degree (InitRunArgs::deg_all)
  // hub-cut bottom-up levels: per-workgroup frontier hub degrees, the
  // decision and its ticket (zero between levels)
  DBuf<int64_t> cut_part_;
  DBuf<int> cut_flag_;
  DBuf<uint8_t> cut_claim_;  // wide-level runs' claims
  DBuf<unsigned> cut_ticket_;
  DBuf<uint8_t> next_bytes_;  // lazily allocated (GW * 64 bytes)
  DBuf<vid_t> send_lists_, recv_lists_;  // sparse exchange, lazily allocated
  DBuf<int64_t> unit_cnt_, unit_deg_, part_cnt_, part_deg_, qscan_, qbase_, stats_;
  // Several ranks (device loop): level L's totals go to
  // stats block (L + 1) % kStatsBlocks, so a mispredicted chain's
  // (unpredicated) reduction never touches the block the re-enqueued chain
  // reads.  One rank: level L's totals in block (L + 1) % kStatsBlocks1, so a
  // level's input totals stay put while its own kernels finish it (see
  // DeviceLoop::sblk).  stats_stride_: int64 entries per block.
  static constexpr int kStatsBlocks = 3;
  static constexpr int kStatsBlocks1 = 2;
  int64_t stats_stride_ = 8;
  DBuf<vid_t> dl_send_lists_, dl_recv_lists_;  // device loop list form, stride list_stride_ + 1
  // binned top-down levels (one rank): bin counts / positions, bin starts, targets
  DBuf<int64_t> bin_total_;
  DBuf<uint32_t> bin_cnt_;
  DBuf<vid_t> bin_buf_;
  int64_t list_stride_ = 0;
  DBuf<unsigned> ticket_;
  DBuf<int32_t> blk_vstart_;
  // device loop, sparse top-down levels: a second work-list set (level L
  // reads set L & 1), entry -> vertex maps, output counters, a ticket
  bool sparse_ready_ = false;
  double excess_degree_ = 0.0;  // sum deg^2 / sum deg (level-1 edge prediction)
  int64_t n_active_ = -1;       // vertices with degree > 0 (global; -1: not computed yet)
  DBuf<int64_t> qscan2_, qbase2_;
  DBuf<int32_t> blk_vstart2_;
  DBuf<vid_t> qv_[2];
  DBuf<unsigned long long> sparse_cnt_;
  DBuf<unsigned> sparse_ticket_;
  bool sparse_enabled() const;
  int64_t nunits_ = 0;
  // device-driven loop state
  DBuf<LevelCtrl> ctrl_;
  // per-level records in pinned, device-mapped segments of kRecSeg levels
  // (host pointer, device pointer): the host reads them after the last stamp
  // without a copy or a stream synchronisation
  static constexpr int kRecSeg = 1024;
  std::vector<std::pair<LevelRecDev*, LevelRecDev*>> rec_segs_;
  LevelRecDev* rec_at(int level);  // device pointer of level's record
  LevelMailbox* mailbox_host_ = nullptr;  // pinned, device-mapped
  LevelMailbox* mailbox_dev_ = nullptr;
  // host-loop statistics mailbox
  StatsMailbox* stats_mb_host_ = nullptr;
  StatsMailbox* stats_mb_dev_ = nullptr;
  int64_t stats_seq_ = 0;
  void read_level_stats(int64_t* host_stats);
  // concurrent multi-source state (csrc/engine/batch.cpp), allocated by the
  // first batch; separate from everything above
  struct MsBuffers {
    DBuf<word_t> seen, front, next;
    DBuf<uint8_t> lvl;
    int lvl_bytes = 0;  // of the allocated matrix (0: none)
    DBuf<vid_t> list[2], touched, long_v;
    DBuf<word_t> long_f;
    DBuf<unsigned long long> cursor;
    DBuf<int64_t> tot, stats, deg_sum;
    DBuf<unsigned> ticket;
    MsMailbox* mb_host = nullptr;
    MsMailbox* mb_dev = nullptr;
    int64_t seq = 0;
    bool wide = false;  // a batch overflowed the one-byte levels: 16-bit from then on
    DBuf<int64_t> check;   // MsCheckArgs::out
    DBuf<uint32_t> par;    // MsCheckArgs::par (allocated by the first batch that keeps parents)
    // MsBcArgs (allocated by the first batch that asks for betweenness or path
    // counts): the value matrix, several ranks' owned lines, the dependency
    // sums of the owned rows, the rows-walked counter followed by the overflow
    // mask (MsBcArgs::walked, ::overflow)
    DBuf<double> bc_val, bc_own, bc_dep;
    // the wide form's value matrix and owned records (MsBcArgs::wval, ::wown),
    // allocated by the first pass that runs wide
    DBuf<unsigned char> bc_wval, bc_wown;
    DBuf<unsigned long long> bc_walked;
    // MsBcArgs::long_rows of the predecessor rows [0] and the out-rows [1]
    // (an undirected graph: [0] for both), built on first use for
    // EngineOptions::bc_split_row = bc_long_above (-1 entries: not built)
    DBuf<vid_t> bc_long[2];
    int64_t bc_long_n[2] = {-1, -1};
    int64_t bc_long_above = 0;
  };
  std::unique_ptr<MsBuffers> ms_;
  // connected-components state (csrc/engine/components.cpp), allocated by the
  // first components() call; separate from everything above
  struct CcBuffers {
    DBuf<vid_t> comp;        // CcArgs::comp: n entries (several ranks: this rank's replica)
    DBuf<uint32_t> size;     // CcArgs::size
    DBuf<vid_t> long_rows;   // CcArgs::long_rows, with the counter
    DBuf<unsigned long long> long_count;
    DBuf<int64_t> totals, slots;
    DBuf<vid_t> sample_idx, sample_out;
    bool valid = false;      // comp and size hold the last call's result
    ComponentsResult last;
  };
  std::unique_ptr<CcBuffers> cc_;
  // strong-components state (csrc/engine/strong_components.cpp), allocated by
  // the first strong_components() call; separate from everything above
  struct SccBuffers {
    DBuf<vid_t> scc, cls, colour;  // SccArgs: nranks x part entries (an owned slice is all-gathered whole)
    DBuf<vid_t> xchg;              // several ranks: the all-gather's receive buffer
    DBuf<uint32_t> size;           // CcArgs::size (cc_sizes over the labels)
    DBuf<unsigned long long> words;  // changed, pivot_out[2], relabel_min
    DBuf<unsigned long long> pivot_slots, pivot_all;
    DBuf<int64_t> totals, slots;   // CcArgs::totals / slots
    bool valid = false;            // scc and size hold the last call's result
    SccResult last;
  };
  std::unique_ptr<SccBuffers> scc_;
  // eccentricity state (csrc/engine/eccentricity.cpp), allocated by the first
  // eccentricities() call; separate from everything above
  struct EccBuffers {
    DBuf<int32_t> lo, hi;        // EccArgs: n entries each
    DBuf<uint32_t> state;
    DBuf<uint32_t> deg, deg_own; // nranks x part entries; several ranks: the owned slice
    DBuf<unsigned long long> sel_slots;
    DBuf<int64_t> sel_out, totals, slots;
    bool valid = false;          // lo, hi and state hold the last call's result
    EccResult last;
  };
  std::unique_ptr<EccBuffers> ecc_;
  // 0: done; 1: deeper than the level type holds (rerun wider)
  int run_batch_pass(const int64_t* src, int k, int pass, BatchDirection dir, int lvl_bytes, BatchResult& out);
  void collect_batch_levels();
  // the view a level check walks: the in-edge shard of a directed graph
  // (built on first use), the shard itself otherwise
  ShardView check_view();
  // What the last batch left, and what of its last pass is still resident.
  struct BatchKept {
    int64_t k = -1;              // sources of the last batch (-1: none, or without levels)
    std::vector<lvl_t> levels;   // [k][n], passes collected so far
    int64_t pending_first = -1;  // last pass not collected yet: its first source ...
    int pending_k = 0;           // ... and size
    int last_k = 0;              // sources of the last pass whose level matrix is resident (0: none)
    // owned slices of the parent trees, [k][part] (-1: unreached or padding)
    std::vector<int64_t> parents;
    int64_t parents_k = -1;      // sources of the last batch with parents (-1: none)
    std::vector<double> counts;  // path counts, [k][n] (BatchCounts::Double) ...
    // ... or as mantissa and exponent (Wide, Auto)
    std::vector<double> counts_mant;
    std::vector<int32_t> counts_exp;
    bool counts_wide = false;
    int64_t counts_k = -1;       // sources of the last batch with path counts (-1: none)
    bool dep_valid = false;      // the last batch accumulated dependencies
  };
  BatchKept kept_;
  // The resident pass's level matrix with its sources src[0..k): the pass's
  // own (one rank), or the owned slices all-gathered into `gathered` (W
  // vertices each, so global vertex v is row v: the several-rank simple form).
  MsPassMatrix pass_matrix(const int64_t* src, int k, DBuf<uint8_t>& gathered);
  // The check of the pass m: counts into viol ([k][3], or nullptr), parents
  // into rows [first, first + k) of kept_.parents (parents set).  Blocking.
  void check_batch_pass(const MsPassMatrix& m, int64_t* viol, bool parents, int64_t first);
  // Path counts and dependencies of the pass m (the deepest of its sources
  // `depth` levels): dependencies into MsBuffers::bc_dep (accumulate), path
  // counts into rows [first, first + k) of kept_.counts (counts).  Blocking;
  // the forward and backward times are added to `out`.  form: Double throws
  // on an overflowed count, Wide runs the wide kernels, Auto redoes the pass
  // wide (init, forward, backward) instead of throwing.
  void bc_batch_pass(const MsPassMatrix& m, int depth, bool accumulate, bool counts, int64_t first, BatchCounts form,
                     BatchResult& out);
  // reference-mode state
  bool ref_ready_ = false;
  DBuf<lvl_t> dist_;
  DBuf<vid_t> queue_, buckets_, recvq_;
  DBuf<int64_t> bucket_cnt_, qcount_;
  DBuf<eid_t> claim_, scan_offs_;  // scan mode
};

}  // namespace dbfs
