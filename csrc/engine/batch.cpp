// Concurrent multi-source BFS (Engine::run_batch): up to 64 sources per pass,
// one bit per source in a 64-bit word per vertex ("The More the Merrier",
// Then et al., VLDB 2015).  A host loop: per level one kernel (pull) or two
// (push + settle) and one totals read -- through a host-mapped mailbox on one
// rank, after the all-gather / all-reduce on several.
//
// Buffers of a level (one rank): `front` holds the frontier words (non-zero
// exactly at the active list's vertices), `next` receives the new bits, then
// the two swap.  A push zeroes the front words it consumes, so the buffer
// comes back clean; a pull writes every word of `next` and leaves its
// frontier in place -- the push after a pull first zeroes those words through
// that level's active list (MsPushArgs::clear_list).  No level clears a whole
// array.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstring>
#include <utility>

#include "dbfs/engine.hpp"
#include "spin.hpp"

namespace dbfs {

namespace {

// Direction rule (Auto, one rank).  A push level costs a scattered `seen`
// probe and often a returning atomic per edge of the active vertices; a pull
// level reads the rows of every vertex that still misses a source, at most
// all directed edges E of the graph.  Push while the active vertices' degree
// sum is below E / kMsPullEnter; once pulling, stay until it is below
// E / kMsPushBack.  Chosen from the per-level push and pull times of the same
// levels on RMAT-20..26, a uniform graph and a road grid (one MI355X,
// profiles/ms_bfs_ab.txt): levels at E / 8.6 .. E / 33.7 run 1.5-4x faster
// pushed, one at E / 3.8 2x faster pulled; on the way back a pull stays ahead
// down to about E / 300 (16 was tried for kMsPushBack and pushed a level too
// early).
constexpr int64_t kMsPullEnter = 8;
constexpr int64_t kMsPushBack = 64;

// Vertex-major on the device, source-major on the host: the device matrix
// dev[rows][kMsSources] into the host rows host[t * stride + r], t < k, each
// entry through conv, copied and transposed kMsCopyRows rows at a time (a host
// temporary of 4 MB for one-byte levels, 32 MB for path counts).
constexpr int64_t kMsCopyRows = int64_t(1) << 16;
template <class TDev, class THost, class Conv>
void copy_transposed(Backend& be, const TDev* dev, int64_t rows, int k, THost* host, size_t stride, Conv conv) {
  std::vector<TDev> h(static_cast<size_t>(std::min(rows, kMsCopyRows)) * kMsSources);
  for (int64_t r0 = 0; r0 < rows; r0 += kMsCopyRows) {
    const int64_t nr = std::min(kMsCopyRows, rows - r0);
    be.to_host(h.data(), dev + static_cast<size_t>(r0) * kMsSources, static_cast<size_t>(nr) * kMsSources * sizeof(TDev));
    for (int64_t r = 0; r < nr; ++r) {
      const TDev* line = h.data() + static_cast<size_t>(r) * kMsSources;
      for (int t = 0; t < k; ++t) host[static_cast<size_t>(t) * stride + static_cast<size_t>(r0 + r)] = conv(line[t]);
    }
  }
}

// The same for a wide value matrix (dbfs/wide.hpp: a 768-byte record per
// vertex) into the host's mantissa and exponent rows.
void copy_transposed_wide(Backend& be, const unsigned char* dev, int64_t rows, int k, double* mant, int32_t* exp,
                          size_t stride) {
  std::vector<unsigned char> h(static_cast<size_t>(std::min(rows, kMsCopyRows)) * kWideRecord);
  for (int64_t r0 = 0; r0 < rows; r0 += kMsCopyRows) {
    const int64_t nr = std::min(kMsCopyRows, rows - r0);
    be.to_host(h.data(), dev + static_cast<size_t>(r0) * kWideRecord, static_cast<size_t>(nr) * kWideRecord);
    for (int64_t r = 0; r < nr; ++r)
      for (int t = 0; t < k; ++t) {
        const Wide x = wide_load(h.data(), r, t);
        mant[static_cast<size_t>(t) * stride + static_cast<size_t>(r0 + r)] = x.m;
        exp[static_cast<size_t>(t) * stride + static_cast<size_t>(r0 + r)] = x.e;
      }
  }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

BatchDirection parse_batch_direction(const std::string& s) {
  if (s == "auto") return BatchDirection::Auto;
  if (s == "push") return BatchDirection::Push;
  if (s == "pull") return BatchDirection::Pull;
  if (s == "alternate") return BatchDirection::Alternate;
  throw Error("batch direction must be auto, push, pull or alternate: '" + s + "'");
}

BatchCounts parse_batch_counts(const std::string& s) {
  if (s == "double") return BatchCounts::Double;
  if (s == "wide") return BatchCounts::Wide;
  if (s == "auto") return BatchCounts::Auto;
  throw Error("batch counts must be double, wide or auto: '" + s + "'");
}

int Engine::run_batch_pass(const int64_t* src, int k, int pass, BatchDirection dir, int lvl_bytes, BatchResult& out) {
  const int P = part_.nranks;
  const int64_t W = part_.part;  // owned vertices, padded: every rank's slice of `front`
  const int64_t front_words = P > 1 ? W * P : W;
  if (!ms_) ms_ = std::make_unique<MsBuffers>();
  MsBuffers& b = *ms_;
  if (b.seen.size() == 0) {
    b.seen = DBuf<word_t>(be_, static_cast<size_t>(W));
    b.next = DBuf<word_t>(be_, static_cast<size_t>(W));
    b.front = DBuf<word_t>(be_, static_cast<size_t>(front_words));
    b.list[0] = DBuf<vid_t>(be_, static_cast<size_t>(W));
    b.list[1] = DBuf<vid_t>(be_, static_cast<size_t>(W));
    b.touched = DBuf<vid_t>(be_, static_cast<size_t>(W));
    // (a push queues rows of more than 1024 entries: at most nnz / 1024 of them)
    b.long_v = DBuf<vid_t>(be_, static_cast<size_t>(g_.nnz() / 1024 + 1));
    b.long_f = DBuf<word_t>(be_, b.long_v.size());
    b.cursor = DBuf<unsigned long long>(be_, 3);
    b.tot = DBuf<int64_t>(be_, static_cast<size_t>(kMsMaxGrid) * kMsStats);
    b.stats = DBuf<int64_t>(be_, kMsStats);
    b.deg_sum = DBuf<int64_t>(be_, kMsSources);
    b.ticket = DBuf<unsigned>(be_, 1);
    be_.memset_async(b.cursor.data(), 0, b.cursor.bytes());
    be_.memset_async(b.ticket.data(), 0, b.ticket.bytes());
    if (P == 1) {
      void* dptr = nullptr;
      b.mb_host = static_cast<MsMailbox*>(be_.alloc_mapped(sizeof(MsMailbox), &dptr));
      b.mb_dev = static_cast<MsMailbox*>(dptr);
    }
  }
  if (lvl_bytes != b.lvl_bytes) {
    b.lvl.reset();
    b.lvl_bytes = 0;
    if (lvl_bytes) {
      b.lvl = DBuf<uint8_t>(be_, static_cast<size_t>(W) * kMsSources * lvl_bytes);
      b.lvl_bytes = lvl_bytes;
    }
  }
  // the deepest level an entry holds (without a matrix: as deep as 16-bit ones would)
  const int max_level = ms_unreached(lvl_bytes ? lvl_bytes : 2) - 1;

  MsState s;
  s.g = g_.view();
  s.in_row_off = s.g.row_off;
  s.in_col = s.g.col;
  if (opt_.directed) {  // (built by run_batch, before the timed window)
    const ShardView in = g_.in_view();
    s.in_row_off = in.row_off;
    s.in_col = in.col;
    s.directed = true;
  }
  s.seen = b.seen.data();
  s.front = b.front.data();
  s.next = b.next.data();
  s.lvl = lvl_bytes ? b.lvl.data() : nullptr;
  s.lvl_bytes = lvl_bytes;
  s.batch_mask = ms_batch_mask(k);
  s.cursor = b.cursor.data();
  s.tot = b.tot.data();
  s.ticket = b.ticket.data();
  s.stats = b.stats.data();
  s.mailbox = b.mb_dev;

  // the level's totals on the host (several ranks: global sums)
  int64_t h[kMsStats];
  auto read_totals = [&](bool reduce) {
    if (P == 1) {
      MsMailbox* mb = b.mb_host;
      const int64_t seq = b.seq;
      spin_until(be_, [&] { return __atomic_load_n(&mb->seq, __ATOMIC_ACQUIRE) == seq; },
                 "batch totals mailbox: stream drained without the stamp");
      for (int i = 0; i < kMsStats; ++i) h[i] = __atomic_load_n(&mb->v[i], __ATOMIC_RELAXED);
      return;
    }
    if (reduce) comm_.allreduce_sum_i64(b.stats.data(), kMsStats);
    be_.to_host(h, b.stats.data(), sizeof(h));
  };

  int cur = 0;  // list[cur]: the active vertices of the level about to run
  MsInitArgs ia;
  ia.k = k;
  std::copy(src, src + k, ia.src);
  ia.next_words = W;
  ia.front_words = front_words;
  s.level = 0;
  s.active_out = b.list[cur].data();
  s.seq = ++b.seq;
  ia.s = s;
  be_.ms_init(ia);
  read_totals(true);
  int64_t local_active = h[0];  // (several ranks: the global count; only one rank pushes)

  const size_t first = out.discovered.size() - static_cast<size_t>(k);  // this pass's sources in `out`
  const size_t first_level_rec = out.levels.size();
  auto note_discovered = [&](int level) {
    for (int t = 0; t < k; ++t) {
      auto& d = out.discovered[first + t];
      if (h[2 + t]) {
        d.resize(static_cast<size_t>(level) + 1, 0);
        d[level] = h[2 + t];
      }
    }
  };
  note_discovered(0);

  bool pulling = false, prev_pull = false;
  int64_t prev_local_active = 0;
  for (int level = 1; h[0] > 0; ++level) {
    if (level > max_level) {
      // (identical on every rank: the totals are global)
      DBFS_CHECK(lvl_bytes == 1, "run_batch: a traversal reached 65535 levels");
      for (int t = 0; t < k; ++t) out.discovered[first + t].clear();
      out.levels.resize(first_level_rec);
      return 1;
    }
    const int64_t n_a = h[0], m_a = h[1];
    bool pull = true;
    if (P == 1) {
      switch (dir) {
        case BatchDirection::Push: pull = false; break;
        case BatchDirection::Pull: pull = true; break;
        case BatchDirection::Alternate: pull = ((level - 1) & 1) != 0; break;
        case BatchDirection::Auto:
          pulling = pulling ? m_a * kMsPushBack >= total_directed_ : m_a * kMsPullEnter > total_directed_;
          pull = pulling;
          break;
      }
    }
    BatchLevelRecord rec;
    rec.pass = pass;
    rec.level = level - 1;
    rec.form = pull ? 'L' : 'P';
    rec.active = n_a;
    rec.edges = m_a;
    out.levels.push_back(rec);
    const auto lt0 = std::chrono::steady_clock::now();

    s.level = level;
    s.active_out = b.list[cur ^ 1].data();
    s.seq = ++b.seq;
    inject_batch_fault(level);
    if (pull) {
      MsPullArgs pa;
      pa.s = s;
      be_.ms_pull(pa);
      if (P > 1) {
        comm_.allgather_allreduce(s.next, s.front, static_cast<size_t>(W) * sizeof(word_t), b.stats.data(), kMsStats);
      } else {
        std::swap(s.front, s.next);
      }
    } else {
      MsPushArgs pa;
      pa.s = s;
      pa.active = b.list[cur].data();
      pa.n_active = local_active;
      pa.touched = b.touched.data();
      pa.active_edges = m_a;
      pa.long_v = b.long_v.data();
      pa.long_f = b.long_f.data();
      pa.long_cap = static_cast<int64_t>(b.long_v.size());
      if (prev_pull) {
        pa.clear_list = b.list[cur ^ 1].data();
        pa.clear_n = prev_local_active;
      }
      be_.ms_push(pa);
      MsSettleArgs sa;
      sa.s = s;
      sa.touched = b.touched.data();
      sa.max_touched = std::min<int64_t>(g_.rows(), m_a);
      be_.ms_settle(sa);
      std::swap(s.front, s.next);
    }
    prev_pull = pull;
    prev_local_active = local_active;
    cur ^= 1;
    read_totals(false);
    local_active = h[0];
    out.levels.back().ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - lt0).count();
    note_discovered(level);
  }

  // end pass: per-source degree sums of the reached
  be_.memset_async(b.deg_sum.data(), 0, b.deg_sum.bytes());
  MsDegreeArgs da;
  da.g = s.g;
  da.seen = s.seen;
  da.deg_sum = b.deg_sum.data();
  be_.ms_degree_sums(da);
  if (P > 1) comm_.allreduce_sum_i64(b.deg_sum.data(), kMsSources);
  int64_t deg[kMsSources];
  be_.to_host(deg, b.deg_sum.data(), sizeof(deg));
  for (int t = 0; t < k; ++t) {
    const auto& d = out.discovered[first + t];
    int64_t reached = 0, dist = 0;
    for (size_t l = 0; l < d.size(); ++l) {
      reached += d[l];
      dist += static_cast<int64_t>(l) * d[l];
    }
    out.reached[first + t] = reached;
    out.dist_sum[first + t] = dist;
    out.depth[first + t] = static_cast<int>(d.size());
    out.edges[first + t] = opt_.directed ? deg[t] : deg[t] / 2;
  }
  return 0;
}

BatchResult Engine::run_batch(const std::vector<int64_t>& sources, const BatchOptions& o) {
  const bool check = o.validate || o.keep_parents, bc = o.betweenness || o.keep_path_counts;
  DBFS_CHECK(o.keep_levels || !check, "run_batch: validate and keep_parents read the level matrix (keep_levels)");
  DBFS_CHECK(o.keep_levels || !bc,
             "run_batch: betweenness and keep_path_counts read the level matrix (keep_levels)");
  DBFS_CHECK(!sources.empty(), "run_batch: no sources");
  for (int64_t v : sources) DBFS_CHECK(v >= 0 && v < part_.n, "run_batch: source vertex out of range");
  DBFS_CHECK(part_.nranks == 1 || o.direction != BatchDirection::Push,
             "run_batch: the push form runs on one rank only (several ranks: every level is a pull)");
  build_in_edges();  // (a directed graph's first batch; outside the timed window)
  const int64_t k = static_cast<int64_t>(sources.size());
  BatchResult out;
  out.sources = sources;
  out.passes = static_cast<int>(div_up(k, kMsSources));
  kept_ = BatchKept{};
  kept_.counts_wide = o.counts != BatchCounts::Double;
  if (o.keep_path_counts) {
    const size_t cnt = static_cast<size_t>(k) * static_cast<size_t>(part_.n);
    if (kept_.counts_wide) {
      kept_.counts_mant.assign(cnt, 0.0);
      kept_.counts_exp.assign(cnt, 0);
    } else {
      kept_.counts.assign(cnt, 0.0);
    }
  }
  if (o.keep_levels) kept_.levels.assign(static_cast<size_t>(k) * static_cast<size_t>(part_.n), kUnreached);
  if (o.keep_parents) kept_.parents.assign(static_cast<size_t>(k) * static_cast<size_t>(part_.part), -1);
  if (o.validate) out.violations.assign(static_cast<size_t>(k) * kMsCheckCounters, 0);
  double ms = 0.0, check_ms = 0.0;
  bool dep_zeroed = false;
  for (int pass = 0; pass < out.passes; ++pass) {
    const int64_t first = static_cast<int64_t>(pass) * kMsSources;
    const int kp = static_cast<int>(std::min<int64_t>(kMsSources, k - first));
    const int64_t* src = sources.data() + first;
    collect_batch_levels();  // (the pass before: outside the timed window)
    out.discovered.resize(static_cast<size_t>(first + kp));
    out.reached.resize(static_cast<size_t>(first + kp), 0);
    out.edges.resize(static_cast<size_t>(first + kp), 0);
    out.dist_sum.resize(static_cast<size_t>(first + kp), 0);
    out.depth.resize(static_cast<size_t>(first + kp), 0);
    comm_.barrier();
    const auto t0 = std::chrono::steady_clock::now();
    const bool wide = ms_ && ms_->wide;
    int lvl_bytes = o.keep_levels ? (wide ? 2 : 1) : 0;
    if (run_batch_pass(src, kp, pass, o.direction, lvl_bytes, out) != 0) {
      // deeper than one-byte levels hold (or, without a level matrix, than
      // 16-bit ones would): once more with 16-bit levels, both runs timed
      ms_->wide = true;
      lvl_bytes = 2;
      const int again = run_batch_pass(src, kp, pass, o.direction, lvl_bytes, out);
      DBFS_CHECK(again == 0, "run_batch: the 16-bit rerun overflowed");
    }
    if (lvl_bytes > 1) out.wide_levels = true;
    be_.synchronize();
    const auto t1 = std::chrono::steady_clock::now();
    ms += ms_since(t0);
    check_device();  // (checked build: a violation a kernel of the pass recorded fails the batch)
    if (o.keep_levels) {
      kept_.pending_first = first;
      kept_.pending_k = kp;
      kept_.last_k = kp;
    }
    if (!check && !bc) continue;
    // After the timed window, before the next pass reuses the matrix (a rerun
    // pass: once, on the rerun's), resolved once (`gathered` ends with the
    // pass) for the check and then the betweenness sweep, each timed on its own.
    const auto tg = std::chrono::steady_clock::now();
    DBuf<uint8_t> gathered;
    const MsPassMatrix m = pass_matrix(src, kp, gathered);
    const double gather_ms = check ? 0.0 : ms_since(tg);  // (the all-gather: in check_ms when a check runs)
    if (check) {
      check_batch_pass(m, o.validate ? out.violations.data() + static_cast<size_t>(first) * kMsCheckCounters : nullptr,
                       o.keep_parents, first);
      check_ms += ms_since(t1);
    }
    if (bc) {
      out.bc_forward_ms += gather_ms;
      out.bc_ms += gather_ms;
      if (o.betweenness && !dep_zeroed) {
        if (ms_->bc_dep.size() == 0) ms_->bc_dep = DBuf<double>(be_, static_cast<size_t>(part_.part));
        be_.memset_async(ms_->bc_dep.data(), 0, ms_->bc_dep.bytes());
        dep_zeroed = true;
      }
      int depth = 0;
      for (int t = 0; t < kp; ++t) depth = std::max(depth, out.depth[static_cast<size_t>(first + t)]);
      bc_batch_pass(m, depth, o.betweenness, o.keep_path_counts, first, o.counts, out);
    }
  }
  out.ms = comm_.max_host(ms);
  if (check) out.check_ms = comm_.max_host(check_ms);
  if (bc) {
    out.bc_forward_ms = comm_.max_host(out.bc_forward_ms);
    out.bc_backward_ms = comm_.max_host(out.bc_backward_ms);
    out.bc_ms = comm_.max_host(out.bc_ms);
  }
  kept_.dep_valid = o.betweenness;
  if (o.keep_path_counts) kept_.counts_k = k;
  if (o.keep_parents) kept_.parents_k = k;
  int64_t edges = 0;
  for (int64_t e : out.edges) edges += e;
  out.gteps = out.ms > 0 ? static_cast<double>(edges) / (out.ms * 1e6) : 0.0;
  if (o.keep_levels) kept_.k = k;
  return out;
}

MsPassMatrix Engine::pass_matrix(const int64_t* src, int k, DBuf<uint8_t>& gathered) {
  const int P = part_.nranks;
  MsBuffers& b = *ms_;
  DBFS_CHECK(b.lvl_bytes != 0, "batch pass: no level matrix is resident");
  MsPassMatrix m;
  m.lvl = b.lvl.data();
  if (P > 1) {
    const size_t bytes = static_cast<size_t>(part_.part) * kMsSources * b.lvl_bytes;
    gathered = DBuf<uint8_t>(be_, bytes * P);
    comm_.allgather(b.lvl.data(), gathered.data(), bytes);
    m.lvl = gathered.data();
  }
  m.lvl_bytes = b.lvl_bytes;
  m.lvl_rows = part_.part * P;
  m.k = k;
  std::copy(src, src + k, m.src);
  m.batch_mask = ms_batch_mask(k);
  return m;
}

// The level matrix of the last pass, if not collected yet -> its rows of kept_.levels.
void Engine::collect_batch_levels() {
  if (kept_.pending_first < 0) return;
  const int64_t n = part_.n;
  DBuf<uint8_t> gathered;
  const MsPassMatrix m = pass_matrix(nullptr, 0, gathered);  // (the matrix alone; a gather of its own, deferred)
  lvl_t* const rows = kept_.levels.data() + static_cast<size_t>(kept_.pending_first) * static_cast<size_t>(n);
  ms_level_type(m.lvl_bytes, [&](auto l) {
    using L = decltype(l);
    copy_transposed(be_, static_cast<const L*>(m.lvl), n, kept_.pending_k, rows, static_cast<size_t>(n),
                    [](L x) { return x == ms_unreached<L>() ? kUnreached : static_cast<lvl_t>(x); });
  });
  kept_.pending_first = -1;
}

// Backend::ms_check on the pass's matrix.  A directed graph is checked by the
// directed rules in one walk over its in-edge shard, where every stored entry
// u -> v appears once, in v's row.
void Engine::check_batch_pass(const MsPassMatrix& m, int64_t* viol, bool parents, int64_t first) {
  const int P = part_.nranks;
  const int64_t W = part_.part;
  MsBuffers& b = *ms_;
  MsCheckArgs ca;
  ca.g = check_view();
  ca.directed = opt_.directed;
  ca.m = m;
  if (viol) {
    if (b.check.size() == 0) b.check = DBuf<int64_t>(be_, kMsSources * kMsCheckCounters);
    be_.memset_async(b.check.data(), 0, b.check.bytes());
    ca.out = b.check.data();
  }
  if (parents) {
    if (b.par.size() == 0) b.par = DBuf<uint32_t>(be_, static_cast<size_t>(W) * kMsSources);
    ca.par = b.par.data();
  }
  be_.ms_check(ca);
  if (viol) {
    if (P > 1) comm_.allreduce_sum_i64(b.check.data(), kMsSources * kMsCheckCounters);
    int64_t h[kMsSources * kMsCheckCounters];
    be_.to_host(h, b.check.data(), sizeof(h));
    std::copy(h, h + static_cast<size_t>(m.k) * kMsCheckCounters, viol);
  }
  if (parents)
    copy_transposed(be_, b.par.data(), g_.rows(), m.k,
                    kept_.parents.data() + static_cast<size_t>(first) * static_cast<size_t>(W), static_cast<size_t>(W),
                    [](uint32_t x) { return x == kMsNoParent ? int64_t(-1) : static_cast<int64_t>(x); });
  be_.synchronize();  // (a rank that copied nothing back: check_ms still ends with the work done)
  check_device();
}

// Backend::ms_bc_* on the pass's matrix: the sources' path counts level by
// level outwards, then (accumulate) the dependencies from the deepest level
// back, each level one launch.  Several ranks, the simple form: the value
// matrix replicated and the owned lines all-gathered into it after every
// launch.  A directed graph's forward sweep walks the in-edge shard, the
// backward one the out-edges.
void Engine::bc_batch_pass(const MsPassMatrix& m, int depth, bool accumulate, bool counts, int64_t first,
                           BatchCounts form, BatchResult& out) {
  static_assert(kWideLanes == kMsSources, "a wide record holds one value per source");
  const auto t0 = std::chrono::steady_clock::now();
  const int P = part_.nranks;
  const int64_t W = part_.part, n = part_.n;
  MsBuffers& b = *ms_;
  const size_t own_vals = static_cast<size_t>(W) * kMsSources;
  const size_t own_wide = static_cast<size_t>(W) * kWideRecord;
  if (b.bc_walked.size() == 0) b.bc_walked = DBuf<unsigned long long>(be_, 2);  // (rows walked; MsBcArgs::overflow)
  be_.memset_async(b.bc_walked.data(), 0, b.bc_walked.bytes());
  MsBcArgs a;
  a.g = g_.view();
  a.m = m;
  a.dep = accumulate ? b.bc_dep.data() : nullptr;
  a.walked = b.bc_walked.data();
  a.overflow = b.bc_walked.data() + 1;
  // the long rows of a view, listed once per engine and threshold
  auto long_rows = [&](int which, const ShardView& view) {
    a.long_rows = nullptr;
    a.n_long = 0;
    a.split_above = opt_.bc_split_row;
    if (opt_.bc_split_row <= 0) return;
    if (b.bc_long_above != opt_.bc_split_row) {
      b.bc_long_n[0] = b.bc_long_n[1] = -1;
      b.bc_long_above = opt_.bc_split_row;
    }
    if (b.bc_long_n[which] < 0) {
      const int64_t cap = view.nnz / opt_.bc_split_row + 1;
      b.bc_long[which] = DBuf<vid_t>(be_, static_cast<size_t>(cap));
      DBuf<unsigned long long> cnt(be_, 1);
      be_.memset_async(cnt.data(), 0, cnt.bytes());
      be_.ms_bc_long_rows(view.row_off, view.rows, opt_.bc_split_row, b.bc_long[which].data(), cap, cnt.data());
      unsigned long long h = 0;
      be_.to_host(&h, cnt.data(), sizeof(h));
      DBFS_CHECK(static_cast<int64_t>(h) <= cap, "batch betweenness: more long rows than the shard can hold");
      b.bc_long_n[which] = static_cast<int64_t>(h);
    }
    a.long_rows = b.bc_long[which].data();
    a.n_long = b.bc_long_n[which];
  };
  auto share = [&] {  // (several ranks: every rank's new lines into every rank's matrix)
    if (P == 1) return;
    if (a.wide) comm_.allgather(b.bc_wown.data(), b.bc_wval.data(), own_wide);
    else comm_.allgather(b.bc_own.data(), b.bc_val.data(), own_vals * sizeof(double));
  };
  const ShardView pred = check_view();
  // (Auto: once in doubles, and once more, wide, when that forward sweep overflowed)
  for (a.wide = form == BatchCounts::Wide;; a.wide = true) {
    if (a.wide) {
      if (b.bc_wval.size() == 0) {
        b.bc_wval = DBuf<unsigned char>(be_, own_wide * P);
        if (P > 1) b.bc_wown = DBuf<unsigned char>(be_, own_wide);
      }
      a.wval = b.bc_wval.data();
      a.wown = P > 1 ? b.bc_wown.data() : b.bc_wval.data();
    } else {
      if (b.bc_val.size() == 0) {
        b.bc_val = DBuf<double>(be_, own_vals * P);
        if (P > 1) b.bc_own = DBuf<double>(be_, own_vals);
      }
      a.val = b.bc_val.data();
      a.own = P > 1 ? b.bc_own.data() : b.bc_val.data();
    }
    be_.ms_bc_init(a);
    // forward: the predecessor rows
    a.row_off = pred.row_off;
    a.col = pred.col;
    a.nnz = pred.nnz;
    long_rows(0, pred);
    for (int level = 1; level < depth; ++level) {
      a.level = level;
      be_.ms_bc_forward(a);
      share();
      ++out.bc_launches;
    }
    if (a.wide) break;  // (no count leaves the wide range)
    if (fault_.kind == "bc_device" && fault_.rank == comm_.rank()) be_.inject_device_check(CheckFile::MsBc);
    // A count past DBL_MAX is inf, and the backward sweep's inf * 0 would be
    // NaN: the batch fails here, on every rank, before a count is copied out
    // (Auto: the pass starts again in the wide form, on every rank).
    unsigned long long over = 0;
    be_.to_host(&over, a.overflow, sizeof(over));
    if (P > 1)
      for (int64_t x : comm_.allgather_host_i64(static_cast<int64_t>(over))) over |= static_cast<unsigned long long>(x);
    if (over == 0ull) break;
    if (form != BatchCounts::Auto)
      throw Error("run_batch: the shortest-path counts from source " + std::to_string(m.src[__builtin_ctzll(over)]) +
                  " exceed the range of a double; betweenness and path counts are not available for this graph");
  }
  if (a.wide) {
    ++out.wide_count_passes;
    if (form == BatchCounts::Wide && fault_.kind == "bc_device" && fault_.rank == comm_.rank())
      be_.inject_device_check(CheckFile::MsBc);
  }
  if (counts) {
    const size_t at = static_cast<size_t>(first) * static_cast<size_t>(n);
    if (a.wide) {
      copy_transposed_wide(be_, b.bc_wval.data(), n, m.k, kept_.counts_mant.data() + at, kept_.counts_exp.data() + at,
                           static_cast<size_t>(n));
    } else if (kept_.counts_wide) {  // (Auto, a pass that stayed in doubles: frexp on the host)
      copy_transposed(be_, b.bc_val.data(), n, m.k, kept_.counts_mant.data() + at, static_cast<size_t>(n),
                      [](double x) { return x; });
      for (size_t i = at; i < at + static_cast<size_t>(m.k) * static_cast<size_t>(n); ++i) {
        const Wide x = wide_from_double(kept_.counts_mant[i]);
        kept_.counts_mant[i] = x.m;
        kept_.counts_exp[i] = x.e;
      }
    } else {
      copy_transposed(be_, b.bc_val.data(), n, m.k, kept_.counts.data() + at, static_cast<size_t>(n),
                      [](double x) { return x; });
    }
  }
  be_.synchronize();
  const auto t1 = std::chrono::steady_clock::now();
  if (accumulate) {
    // backward: the out-rows; level 0 holds the sources themselves, which
    // take no share of their own dependencies
    a.row_off = a.g.row_off;
    a.col = a.g.col;
    a.nnz = a.g.nnz;
    long_rows(opt_.directed ? 1 : 0, a.g);
    const int64_t n_long = a.n_long;
    for (int level = depth - 1; level >= 1; --level) {
      a.level = level;
      a.leaf = level == depth - 1;
      a.n_long = a.leaf ? 0 : n_long;  // (the deepest level walks no row: every vertex by its wave)
      be_.ms_bc_backward(a);
      share();
      ++out.bc_launches;
    }
  }
  unsigned long long walked = 0;
  be_.to_host(&walked, b.bc_walked.data(), sizeof(walked));
  out.bc_rows_walked += static_cast<int64_t>(walked);
  be_.synchronize();
  check_device();
  const auto t2 = std::chrono::steady_clock::now();
  out.bc_forward_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
  out.bc_backward_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
  out.bc_ms += std::chrono::duration<double, std::milli>(t2 - t0).count();
}

std::vector<double> Engine::gather_betweenness() {
  DBFS_CHECK(kept_.dep_valid && ms_, "gather_betweenness: no batch has run with betweenness");
  const int P = part_.nranks;
  const int64_t W = part_.part, n = part_.n;
  std::vector<double> h(static_cast<size_t>(W) * P);
  if (P > 1) {
    DBuf<double> allv(be_, h.size());
    comm_.allgather(ms_->bc_dep.data(), allv.data(), static_cast<size_t>(W) * sizeof(double));
    be_.to_host(h.data(), allv.data(), h.size() * sizeof(double));
  } else {
    be_.to_host(h.data(), ms_->bc_dep.data(), h.size() * sizeof(double));
  }
  h.resize(static_cast<size_t>(n));  // (slices are W vertices each: global vertex v is entry v)
  return h;
}

std::vector<double> Engine::gather_batch_path_counts() {
  DBFS_CHECK(kept_.counts_k > 0, "gather_batch_path_counts: no batch has run with keep_path_counts");
  if (!kept_.counts_wide) return kept_.counts;
  std::vector<double> out(kept_.counts_mant.size());
  for (size_t i = 0; i < out.size(); ++i) {
    out[i] = wide_to_double(Wide{kept_.counts_mant[i], kept_.counts_exp[i]});
    DBFS_CHECK(out[i] <= DBL_MAX,
               "gather_batch_path_counts: a shortest-path count exceeds the range of a double; "
               "gather_batch_path_counts_wide / batch_path_counts_wide return mantissas and exponents");
  }
  return out;
}

void Engine::gather_batch_path_counts_wide(std::vector<double>& mant, std::vector<int32_t>& exp) {
  DBFS_CHECK(kept_.counts_k > 0, "gather_batch_path_counts_wide: no batch has run with keep_path_counts");
  if (kept_.counts_wide) {
    mant = kept_.counts_mant;
    exp = kept_.counts_exp;
    return;
  }
  mant.resize(kept_.counts.size());
  exp.resize(kept_.counts.size());
  for (size_t i = 0; i < mant.size(); ++i) {
    const Wide x = wide_from_double(kept_.counts[i]);
    mant[i] = x.m;
    exp[i] = x.e;
  }
}

std::vector<int64_t> Engine::validate_batch_pass(const std::vector<int64_t>& sources) {
  DBFS_CHECK(ms_ && kept_.last_k > 0 && ms_->lvl_bytes != 0,
             "validate_batch_pass: no batch has run with keep_levels");
  DBFS_CHECK(static_cast<int>(sources.size()) == kept_.last_k,
             "validate_batch_pass: expected as many sources as the last pass had (" + std::to_string(kept_.last_k) +
                 "), got " + std::to_string(sources.size()));
  for (int64_t v : sources) DBFS_CHECK(v >= 0 && v < part_.n, "validate_batch_pass: source vertex out of range");
  std::vector<int64_t> viol(sources.size() * kMsCheckCounters, 0);
  DBuf<uint8_t> gathered;  // (resolved afresh: debug_set_batch_level may have changed the matrix)
  check_batch_pass(pass_matrix(sources.data(), kept_.last_k, gathered), viol.data(), false, 0);
  return viol;
}

void Engine::debug_set_batch_level(int slot, int64_t vertex, int level) {
  DBFS_CHECK(ms_ && kept_.last_k > 0 && ms_->lvl_bytes != 0,
             "debug_set_batch_level: no batch has run with keep_levels");
  DBFS_CHECK(slot >= 0 && slot < kMsSources && vertex >= 0 && vertex < part_.n,
             "debug_set_batch_level: slot or vertex out of range");
  MsBuffers& b = *ms_;
  const int none = ms_unreached(b.lvl_bytes);
  DBFS_CHECK(level < none, "debug_set_batch_level: the level does not fit the matrix");
  const int64_t r = vertex - g_.lo();
  if (r < 0 || r >= g_.rows()) return;  // another rank's
  const uint16_t x = static_cast<uint16_t>(level < 0 ? none : level);  // (little-endian: the low byte first)
  be_.to_device(b.lvl.data() + (static_cast<size_t>(r) * kMsSources + slot) * b.lvl_bytes, &x,
                static_cast<size_t>(b.lvl_bytes));
}

std::vector<int64_t> Engine::gather_batch_parents() {
  DBFS_CHECK(kept_.parents_k > 0, "gather_batch_parents: no batch has run with keep_parents");
  const int P = part_.nranks;
  const int64_t W = part_.part, n = part_.n, k = kept_.parents_k;
  std::vector<int64_t> out(static_cast<size_t>(k) * static_cast<size_t>(n));
  std::vector<int64_t> all;
  const int64_t* slices = kept_.parents.data();  // [rank][k][W]
  if (P > 1) {
    const size_t cnt = static_cast<size_t>(k) * static_cast<size_t>(W);
    DBuf<int64_t> send(be_, cnt), recv(be_, cnt * P);
    be_.to_device(send.data(), kept_.parents.data(), cnt * sizeof(int64_t));
    comm_.allgather(send.data(), recv.data(), cnt * sizeof(int64_t));
    all.resize(cnt * P);
    be_.to_host(all.data(), recv.data(), all.size() * sizeof(int64_t));
    slices = all.data();
  }
  for (int p = 0; p < P; ++p) {
    const int64_t lo = static_cast<int64_t>(p) * W, cnt = std::min(W, n - lo);
    for (int64_t t = 0; t < k && cnt > 0; ++t)
      std::copy_n(slices + (static_cast<size_t>(p) * k + t) * W, cnt, out.data() + static_cast<size_t>(t) * n + lo);
  }
  return out;
}

std::vector<lvl_t> Engine::gather_batch_levels() {
  DBFS_CHECK(kept_.k > 0, "gather_batch_levels: no batch has run with keep_levels");
  collect_batch_levels();
  return kept_.levels;
}

}  // namespace dbfs
