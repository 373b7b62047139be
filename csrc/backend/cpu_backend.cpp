// CPU implementation of the Backend primitives.
//
// Semantically identical to the HIP kernels (same work-list layout, same
// segment bookkeeping) so the engine's orchestration, partitioning and
// collectives are exercised by the CPU test-suite exactly as they run on the
// GPU.  Not a performance path.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "dbfs/backend.hpp"

namespace dbfs {
namespace {

// A level's decision from its totals and its stamp (HIP: finish_level); c:
// the control block the decision starts from.
inline void finish_level(const LevelStamp& s, LevelCtrl c, int64_t cnt, int64_t deg) {
  level_ctrl_finish(c, cnt, deg, s.seed, s.seed ? nullptr : s.rec);
  *s.ctrl = c;
  if (LevelMailbox* mb = s.mailbox) {
    mb->done = c.done;
    mb->vis_deg = c.vis_deg;
    mb->next_dir = c.dir;
    mb->n_f = c.n_f;
    mb->m_f = c.m_f;
    mb->reached = c.reached;
    mb->level = s.seed ? -1 : s.level;
  }
}

inline bool test_bit(const word_t* bm, uint64_t v) { return (bm[v >> 6] >> (v & 63)) & 1ull; }
inline word_t gather_bytes(uint8_t* p) {
  word_t bits = 0;
  for (int b = 0; b < 64; ++b)
    if (p[b]) bits |= 1ull << b;
  if (bits) std::memset(p, 0, 64);
  return bits;
}

class CpuBackend final : public Backend {
 public:
  DeviceKind kind() const override { return DeviceKind::CPU; }
  std::string name() const override { return "cpu"; }

  void* alloc(size_t bytes) override {
    void* p = std::aligned_alloc(64, round_up(std::max<size_t>(bytes, 64), 64));
    if (!p) raise_error(__FILE__, __LINE__, "host allocation failed");
    // DBFS_POISON_ALLOC=<byte>: as the HIP backend's (memory never written
    // reads as that byte instead of whatever the allocator hands back)
    static const int poison = [] {
      const char* e = std::getenv("DBFS_POISON_ALLOC");
      return e && *e ? static_cast<int>(std::strtol(e, nullptr, 0)) & 0xff : -1;
    }();
    if (poison >= 0) std::memset(p, poison, round_up(std::max<size_t>(bytes, 64), 64));
    return p;
  }
  void dealloc(void* p) override { std::free(p); }
  void memset_async(void* p, int v, size_t bytes) override { std::memset(p, v, bytes); }
  void copy_async(void* d, const void* s, size_t bytes) override {
    if (bytes) std::memmove(d, s, bytes);
  }
  void to_host(void* d, const void* s, size_t bytes) override { copy_async(d, s, bytes); }
  void to_device(void* d, const void* s, size_t bytes) override { copy_async(d, s, bytes); }
  void synchronize() override {}

  int record_event() override {
    events_.push_back(std::chrono::steady_clock::now());
    return static_cast<int>(events_.size() - 1);
  }
  double elapsed_ms(int a, int b) override {
    return std::chrono::duration<double, std::milli>(events_.at(b) - events_.at(a)).count();
  }
  void reset_events() override { events_.clear(); }

  void fill_level(lvl_t* level, int64_t n, lvl_t value) override { std::fill(level, level + n, value); }
  void set_bit(word_t* bm, int64_t bit) override { bm[bit >> 6] |= 1ull << (bit & 63); }

  void update_frontier(const UpdateArgs& a) override {
    if (a.fuse_scan) {
      // totals and finish right after the update, unit statistics unscanned
      UpdateArgs b = a;
      b.fuse_scan = false;
      update_frontier(b);
      const int64_t n = a.scan.nunits;
      std::vector<int64_t> c(a.scan.unit_cnt, a.scan.unit_cnt + n), d(a.scan.unit_deg, a.scan.unit_deg + n);
      scan_units(a.scan);
      if (a.fold_scan) return;  // (the prefixes stay: the next compaction reads them)
      std::copy(c.begin(), c.end(), a.scan.unit_cnt);
      std::copy(d.begin(), d.end(), a.scan.unit_deg);
      return;
    }
    bool use_bytes = a.cand_bytes != nullptr;
    if (!a.guard.live()) return;
    if (a.guard.ctrl) use_bytes = use_bytes && a.guard.ctrl->bytes != 0;
    const int64_t nunits = div_up(a.words, kUnitWords);
    for (int64_t u = 0; u < nunits; ++u) {
      int64_t cnt = 0, deg = 0;
      for (int64_t w = u * kUnitWords; w < std::min<int64_t>(a.words, (u + 1) * kUnitWords); ++w) {
        word_t c = 0;
        if (use_bytes && a.level_direct) {
          for (int b = 0; b < 64; ++b)
            if (a.level_direct[w * 64 + b] == a.out.byte()) c |= 1ull << b;
        } else if (use_bytes) {
          c = gather_bytes(a.cand_bytes + w * 64);
        } else {
          for (int r = 0; r < a.nchunks; ++r) c |= a.cand[r * a.cand_stride + w];
          if (a.clear_cand) a.cand[w] = 0;
        }
        const word_t nb = a.force ? c : (c & ~a.visited[w]);
        a.visited[w] |= nb;
        a.frontier[w] = nb;
        for (int p = 0; p < a.zero_slices; ++p) a.zero_next[p * a.words + w] = 0;
        word_t x = nb;
        while (x) {
          const int b = __builtin_ctzll(x);
          x &= x - 1;
          const int64_t v = w * 64 + b;
          // (padding bits are pre-set visited; a forced update takes its level bytes unmasked)
          DBFS_CHECK(v < a.g.rows, "update: a new vertex in the last word's padding");
          a.out.store(v);
          const eid_t d = a.g.row_off[v + 1] - a.g.row_off[v];
          if (d > 0) { ++cnt; deg += d; }
        }
      }
      a.unit_cnt[u] = cnt;
      a.unit_deg[u] = deg;
    }
  }

  void level_ctrl_init(LevelCtrl* c, const LevelCtrl& init) override { *c = init; }
  void init_run(const InitRunArgs& a) override {
    const int64_t src = a.src_local;
    if (a.out.level8 && a.level8_filled) {
      if (src >= 0) a.out.level8[src] = a.out.narrow_base;
    } else {
      for (int64_t i = 0; i < a.g.rows; ++i) {
        if (a.out.level8) a.out.level8[i] = i == src ? a.out.narrow_base : kNarrowUnreached;
        else a.out.level[i] = i == src ? 0 : kUnreached;
      }
      // (the last word's padding bytes too: a split level's forced update
      // takes every byte equal to its level as a new vertex, unmasked)
      if (a.out.level8)
        for (int64_t i = a.g.rows; i < a.words * kWordBits; ++i) a.out.level8[i] = kNarrowUnreached;
    }
    for (int64_t w = 0; w < a.gwords; ++w) a.visited[w] = a.zdeg[w];
    if (a.frontier_clean && !a.frontier_global) {
      // (the claim the device kernel relies on, checked: no stale bit left)
      for (int64_t w = 0; w < a.words; ++w)
        DBFS_CHECK(a.frontier[w] == 0 && (!a.frontier_clear || a.frontier_clear[w] == 0),
                   "init_run: a frontier claimed clean holds a stale bit");
    }
    for (int64_t w = 0; w < a.words; ++w) a.frontier[w] = 0;
    if (a.frontier_global)
      for (int64_t w = 0; w < a.gwords; ++w) a.frontier_global[w] = 0;
    if (a.src_global >= 0) {
      // (a seed without collective: the source's bits on every rank)
      const word_t gbit = 1ull << (a.src_global & 63);
      a.visited[a.src_global >> 6] |= gbit;
      if (a.frontier_global) a.frontier_global[a.src_global >> 6] = gbit;
    }
    int64_t cnt = 0, deg = 0;
    if (src >= 0) {
      const word_t bit = 1ull << (src & 63);
      a.visited[a.vis_word_base + (src >> 6)] |= bit;
      a.frontier[src >> 6] = bit;
      const eid_t d = a.g.row_off[src + 1] - a.g.row_off[src];
      if (d > 0) { cnt = 1; deg = d; }
      const int64_t unit = (src >> 6) / kUnitWords;
      a.unit_cnt[unit] = a.unit_deg[unit] = 0;
      a.part_cnt[unit / kScanChunk] = a.part_deg[unit / kScanChunk] = 0;
    }
    a.stats[0] = a.stats[2] = cnt;
    a.stats[1] = a.stats[3] = deg;
    a.wl.qscan[cnt] = deg;
    if (a.frontier_clear)
      for (int64_t w = 0; w < a.words; ++w) a.frontier_clear[w] = 0;
    if (cnt && a.wl.qbase) {
      a.wl.qscan[0] = 0;
      a.wl.qbase[0] = a.g.row_off[src];
      a.wl.qv[0] = static_cast<vid_t>(src);
      for (int64_t b = 0; b * kTdEdgesPerBlock < deg; ++b) a.wl.blk_vstart[b] = 0;
    }
    if (a.ctrl) {
      int64_t gc = cnt, gd = deg;
      if (a.deg_all) {
        gd = a.deg_all[a.src_global];
        gc = gd > 0 ? 1 : 0;
        a.stats[2] = gc;
        a.stats[3] = gd;
      }
      finish_level({a.ctrl, nullptr, a.mailbox, -1, true}, a.ctrl_init, gc, gd);
    }
  }
  void publish_stats(const int64_t* stats, StatsMailbox* mb, int64_t seq) override {
    for (int k = 0; k < 4; ++k) mb->v[k] = stats[k];
    __atomic_store_n(&mb->seq, seq, __ATOMIC_RELEASE);
  }
  // ---- concurrent multi-source BFS (backend.hpp MsState): plain loops ----
  static void ms_store_level(const MsState& s, int64_t row, int src, int level) {
    ms_level_type(s.lvl_bytes, [&](auto l) {
      static_cast<decltype(l)*>(s.lvl)[row * kMsSources + src] = static_cast<decltype(l)>(level);
    });
  }
  static void ms_publish(const MsState& s) {
    if (!s.mailbox) return;
    for (int k = 0; k < kMsStats; ++k) s.mailbox->v[k] = s.stats[k];
    __atomic_store_n(&s.mailbox->seq, s.seq, __ATOMIC_RELEASE);
  }
  // a vertex with new bits: levels, the next active list, the level's totals
  static void ms_record(const MsState& s, int64_t row, word_t nw) {
    if (!nw) return;
    s.active_out[s.cursor[0]++] = static_cast<vid_t>(row);
    s.stats[1] += s.g.row_off[row + 1] - s.g.row_off[row];
    for (int b = 0; b < kMsSources; ++b) {
      if (!((nw >> b) & 1ull)) continue;
      s.stats[2 + b] += 1;
      if (s.lvl) ms_store_level(s, row, b, s.level);
    }
  }
  static void ms_level_end(const MsState& s) {
    s.stats[0] = static_cast<int64_t>(s.cursor[0]);
    s.cursor[0] = 0;
    ms_publish(s);
  }
  void ms_init(const MsInitArgs& a) override {
    const MsState& s = a.s;
    std::fill(s.seen, s.seen + a.next_words, word_t(0));
    std::fill(s.next, s.next + a.next_words, word_t(0));
    std::fill(s.front, s.front + a.front_words, word_t(0));
    if (s.lvl) std::memset(s.lvl, 0xFF, static_cast<size_t>(a.next_words) * kMsSources * s.lvl_bytes);
    std::fill(s.stats, s.stats + kMsStats, int64_t(0));
    for (int t = 0; t < a.k; ++t) {
      const int64_t v = a.src[t];
      const word_t bit = word_t(1) << t;
      s.front[v] |= bit;
      if (v < s.g.lo || v >= s.g.lo + s.g.rows) continue;
      const int64_t r = v - s.g.lo;
      if (!s.seen[r]) {
        s.active_out[s.stats[0]++] = static_cast<vid_t>(r);
        s.stats[1] += s.g.row_off[r + 1] - s.g.row_off[r];
      }
      s.seen[r] |= bit;
      s.stats[2 + t] = 1;
      if (s.lvl) ms_store_level(s, r, t, 0);
    }
    ms_publish(s);
  }
  void ms_pull(const MsPullArgs& a) override {
    const MsState& s = a.s;
    const ShardView& g = s.g;
    // (a directed graph: the in-edge rows; ms_record sums out-degrees from s.g)
    const eid_t* row_off = s.directed ? s.in_row_off : g.row_off;
    const vid_t* col = s.directed ? s.in_col : g.col;
    std::fill(s.stats, s.stats + kMsStats, int64_t(0));
    for (int64_t v = 0; v < g.rows; ++v) {
      const word_t need = ~s.seen[v] & s.batch_mask;
      word_t got = 0;
      if (need)
        for (eid_t e = row_off[v]; e < row_off[v + 1]; ++e) {
          got |= s.front[col[e]];
          if ((got & need) == need) break;
        }
      const word_t nw = got & need;
      s.seen[v] |= nw;
      s.next[v] = nw;
      ms_record(s, v, nw);
    }
    ms_level_end(s);
  }
  void ms_push(const MsPushArgs& a) override {
    const MsState& s = a.s;
    const ShardView& g = s.g;
    for (int64_t i = 0; i < a.clear_n; ++i) s.next[a.clear_list[i]] = 0;
    for (int64_t i = 0; i < a.n_active; ++i) {
      const vid_t v = a.active[i];
      const word_t f = s.front[v];
      s.front[v] = 0;
      for (eid_t e = g.row_off[v]; e < g.row_off[v + 1]; ++e) {
        const vid_t w = g.col[e];
        const word_t m = f & ~s.seen[w];
        if (!m) continue;
        const word_t old = s.next[w];
        s.next[w] = old | m;
        if (!old) a.touched[s.cursor[1]++] = w;
      }
    }
  }
  void ms_settle(const MsSettleArgs& a) override {
    const MsState& s = a.s;
    std::fill(s.stats, s.stats + kMsStats, int64_t(0));
    const int64_t n = std::min<int64_t>(static_cast<int64_t>(s.cursor[1]), a.max_touched);
    for (int64_t i = 0; i < n; ++i) {
      const vid_t w = a.touched[i];
      const word_t nw = s.next[w] & ~s.seen[w];
      s.seen[w] |= nw;
      s.next[w] = nw;
      ms_record(s, w, nw);
    }
    s.cursor[1] = 0;
    ms_level_end(s);
  }
  void ms_degree_sums(const MsDegreeArgs& a) override {
    for (int64_t v = 0; v < a.g.rows; ++v) {
      const int64_t deg = a.g.row_off[v + 1] - a.g.row_off[v];
      word_t sv = deg ? a.seen[v] : 0;
      for (; sv; sv &= sv - 1) a.deg_sum[__builtin_ctzll(sv)] += deg;
    }
  }
  void ms_check(const MsCheckArgs& a) override {
    const ShardView& g = a.g;
    const int none = ms_unreached(a.m.lvl_bytes);
    for (int64_t r = 0; r < g.rows; ++r) {
      const int64_t u = g.lo + r;
      for (int s = 0; s < a.m.k; ++s) {
        const int lu = level_at(a.m, u, s);
        int64_t gap = 0, cross = 0;
        uint32_t par = kMsNoParent;
        bool has_parent = false;
        for (eid_t e = g.row_off[r]; e < g.row_off[r + 1]; ++e) {
          const vid_t w = g.col[e];
          const int lw = level_at(a.m, w, s);
          if (a.directed) {
            // (in-edge row of u: the entry is w -> u)
            if (lw == none) continue;
            if (lu == none) { ++cross; continue; }
            if (lu - lw > 1) ++gap;
          } else {
            if (lu == none && lw == none) continue;
            if ((lu == none) != (lw == none)) { ++cross; continue; }
            if (lu - lw > 1 || lw - lu > 1) ++gap;
          }
          if (lw == lu - 1 && !has_parent) {
            has_parent = true;
            par = w;
          }
        }
        const bool is_src = u == a.m.src[s];
        if (a.out) {
          a.out[kMsCheckCounters * s + 0] += gap;
          a.out[kMsCheckCounters * s + 1] += cross;
          if (is_src ? lu != 0 : (lu != none && !has_parent)) a.out[kMsCheckCounters * s + 2] += 1;
        }
        if (a.par) a.par[r * kMsSources + s] = is_src ? static_cast<uint32_t>(u) : par;
      }
    }
  }
  // ---- path counts and dependencies (backend.hpp MsBcArgs): plain loops, every
  // sum in the kernels' order (stored row order per source, the lanes' tree).
  // The two value forms: doubles, and dbfs/wide.hpp's mantissa and exponent ----
  struct BcF64 {
    using Sum = double;
    static Sum sum_zero() { return 0.0; }
    static void add(Sum& sum, const MsBcArgs& a, int64_t w, int s) { sum += a.val[w * kMsSources + s]; }
    static void init(const MsBcArgs& a, int s, int64_t src) {
      for (int64_t v = 0; v < a.m.lvl_rows; ++v) a.val[v * kMsSources + s] = v == src ? 1.0 : 0.0;
      for (int64_t r = 0; r < a.g.rows; ++r) a.own[r * kMsSources + s] = a.g.lo + r == src ? 1.0 : 0.0;
    }
    static void store_forward(const MsBcArgs& a, int64_t r, int s, Sum sum) {
      a.own[r * kMsSources + s] = sum;
      if (!(sum <= DBL_MAX)) *a.overflow |= 1ull << s;  // (out of double's range: the engine fails the batch)
    }
    // delta; own[r][s] turns from sigma into the coefficient
    static double store_backward(const MsBcArgs& a, int64_t r, int s, Sum acc) {
      const double sigma = a.own[r * kMsSources + s];
      const double delta = sigma * acc;
      a.own[r * kMsSources + s] = (1.0 + delta) / sigma;
      return delta;
    }
  };
  struct BcWide {
    using Sum = WideSum;
    static Sum sum_zero() { return wide_sum_zero(); }
    static void add(Sum& sum, const MsBcArgs& a, int64_t w, int s) { wide_add(sum, wide_load(a.wval, w, s)); }
    static void init(const MsBcArgs& a, int s, int64_t src) {
      for (int64_t v = 0; v < a.m.lvl_rows; ++v) wide_store(a.wval, v, s, v == src ? wide_one() : wide_zero());
      for (int64_t r = 0; r < a.g.rows; ++r) wide_store(a.wown, r, s, a.g.lo + r == src ? wide_one() : wide_zero());
    }
    static void store_forward(const MsBcArgs& a, int64_t r, int s, Sum sum) {
      wide_store(a.wown, r, s, wide_normalise(sum));
    }
    static double store_backward(const MsBcArgs& a, int64_t r, int s, Sum acc) {
      const Wide sigma = wide_load(a.wown, r, s);
      const double delta = wide_delta(sigma, acc);
      wide_store(a.wown, r, s, wide_coefficient(delta, sigma));
      return delta;
    }
  };
  template <class F>
  static void bc_value_type(const MsBcArgs& a, F&& f) {
    if (a.wide) {
      DBFS_CHECK(a.wval && a.wown, "MsBcArgs: wide without wval / wown");
      f(BcWide{});
    } else {
      f(BcF64{});
    }
  }
  template <class V>
  static typename V::Sum bc_row_sum(const MsBcArgs& a, int64_t r, int s, int want) {
    typename V::Sum sum = V::sum_zero();
    if (want == ms_unreached(a.m.lvl_bytes)) return sum;
    for (eid_t e = a.row_off[r]; e < a.row_off[r + 1]; ++e) {
      const vid_t w = a.col[e];
      if (level_at(a.m, w, s) == want) V::add(sum, a, static_cast<int64_t>(w), s);
    }
    return sum;
  }
  void ms_bc_init(const MsBcArgs& a) override {
    bc_value_type(a, [&](auto val) {
      for (int s = 0; s < kMsSources; ++s) decltype(val)::init(a, s, s < a.m.k ? a.m.src[s] : -1);
    });
  }
  // (the host loops walk every row themselves, the listed long ones included)
  void ms_bc_long_rows(const eid_t* row_off, int64_t rows, int64_t above, vid_t* list, int64_t cap,
                       unsigned long long* count) override {
    for (int64_t r = 0; r < rows; ++r) {
      if (row_off[r + 1] - row_off[r] <= above) continue;
      if (static_cast<int64_t>(*count) < cap) list[*count] = static_cast<vid_t>(r);
      ++*count;
    }
  }
  // connected components (CcArgs): the device's hook, one entry at a time
  static void cc_hook(vid_t* comp, vid_t u, vid_t w) {
    vid_t p1 = comp[u], p2 = comp[w];
    while (p1 != p2) {
      const vid_t hi = std::max(p1, p2), lo = std::min(p1, p2);
      if (comp[hi] == hi) {
        comp[hi] = lo;
        break;
      }
      p1 = comp[hi];
      p2 = comp[lo];
    }
  }
  void cc_init(const CcArgs& a) override {
    for (int64_t v = 0; v < a.g.n; ++v) a.comp[v] = static_cast<vid_t>(v);
  }
  void cc_link(const CcArgs& a) override {
    for (int64_t r = 0; r < a.g.rows; ++r) {
      const vid_t u = static_cast<vid_t>(a.g.lo + r);
      const eid_t rs = std::min<eid_t>(a.g.row_off[r + 1], a.g.row_off[r] + a.first);
      const eid_t re = a.count < 0 ? a.g.row_off[r + 1] : std::min<eid_t>(a.g.row_off[r + 1], rs + a.count);
      if (a.skip && a.comp[u] == a.skip_label) continue;
      for (eid_t e = rs; e < re; ++e) cc_hook(a.comp, u, a.g.col[e]);
    }
  }
  void cc_link_pairs(const CcArgs& a) override {
    for (int64_t i = 0; i < a.pairs; ++i) cc_hook(a.comp, static_cast<vid_t>(a.pair_lo + i), a.other[i]);
  }
  void cc_compress(const CcArgs& a) override {
    // (ascending: comp[v] <= v, so v's parent already holds its root)
    for (int64_t v = 0; v < a.g.n; ++v) a.comp[v] = a.comp[a.comp[v]];
  }
  void cc_sample(const CcArgs& a) override {
    for (int i = 0; i < a.samples; ++i) a.sample_out[i] = a.comp[a.sample_idx[i]];
  }
  void cc_sizes(const CcArgs& a) override {
    int64_t roots = 0, single = 0, best = 0, best_label = 0;
    for (int64_t v = 0; v < a.g.n; ++v) a.size[v] = 0;
    for (int64_t v = 0; v < a.g.n; ++v) ++a.size[a.comp[v]];
    for (int64_t v = 0; v < a.g.n; ++v) {
      if (a.comp[v] != static_cast<vid_t>(v)) continue;
      ++roots;
      single += a.size[v] == 1u ? 1 : 0;
      if (static_cast<int64_t>(a.size[v]) > best) best = a.size[v], best_label = v;  // (ascending: ties keep the smaller)
    }
    a.totals[0] = roots;
    a.totals[1] = single;
    a.totals[2] = best;
    a.totals[3] = best_label;
  }
  // strongly connected components (SccArgs): the device's sweeps as plain
  // loops, in place (a later row sees what an earlier one stored: the device's
  // "may read entries written earlier in the same launch")
  static bool scc_counts(const SccArgs& a, vid_t v, vid_t w) {
    return w != v && a.cls[w] == a.cls[v] && a.scc[w] == kSccNone;
  }
  void scc_init(const SccArgs& a) override {
    for (int64_t v = 0; v < a.out.n; ++v) a.scc[v] = a.cls[v] = a.colour[v] = kSccNone;
  }
  static bool scc_surplus(const SccArgs& a) { return a.prev_changed && *a.prev_changed == 0; }
  void scc_trim(const SccArgs& a) override {
    if (scc_surplus(a)) return;
    auto has = [&](const ShardView& g, int64_t r, vid_t v) {
      for (eid_t e = g.row_off[r]; e < g.row_off[r + 1]; ++e)
        if (scc_counts(a, v, g.col[e])) return true;
      return false;
    };
    for (int64_t r = 0; r < a.out.rows; ++r) {
      const vid_t v = static_cast<vid_t>(a.out.lo + r);
      if (a.scc[v] != kSccNone || (has(a.out, r, v) && has(a.in, r, v))) continue;
      a.scc[v] = v;
      ++*a.changed;
    }
  }
  void scc_pivot(const SccArgs& a) override {
    unsigned long long prod = 0;
    vid_t id = kSccNone;
    for (int64_t r = 0; r < a.out.rows; ++r) {
      const vid_t v = static_cast<vid_t>(a.out.lo + r);
      if (a.scc[v] != kSccNone) continue;
      const unsigned long long p = static_cast<unsigned long long>(a.out.row_off[r + 1] - a.out.row_off[r]) *
                                   static_cast<unsigned long long>(a.in.row_off[r + 1] - a.in.row_off[r]);
      if (id == kSccNone || p > prod) prod = p, id = v;  // (ascending: ties keep the smaller)
    }
    a.pivot_out[0] = prod;
    a.pivot_out[1] = id;
  }
  void scc_colour_init(const SccArgs& a) override {
    for (int64_t v = 0; v < a.out.n; ++v)
      if (a.scc[v] == kSccNone)
        a.colour[v] = !a.pivot_only || static_cast<vid_t>(v) == a.pivot ? static_cast<vid_t>(v) : kSccNone;
  }
  void scc_forward(const SccArgs& a) override {
    if (scc_surplus(a)) return;
    for (int64_t r = 0; r < a.in.rows; ++r) {
      const vid_t v = static_cast<vid_t>(a.in.lo + r);
      if (a.scc[v] != kSccNone) continue;
      vid_t m = a.colour[v];
      // (pivot_only: the one colour there is -- a coloured v is done, the walk ends at the first hit)
      // (... and, the first round, a neighbour with the pivot's colour counts: no class or liveness test)
      for (eid_t e = a.in.row_off[r]; e < a.in.row_off[r + 1] && !(a.pivot_only && m != kSccNone); ++e)
        if (a.pivot_only ? a.colour[a.in.col[e]] == a.pivot : scc_counts(a, v, a.in.col[e]))
          m = std::min(m, a.colour[a.in.col[e]]);
      if (m < a.colour[v]) {
        a.colour[v] = m;
        ++*a.changed;
      }
    }
  }
  void scc_backward(const SccArgs& a) override {
    if (scc_surplus(a)) return;
    for (int64_t r = 0; r < a.out.rows; ++r) {
      const vid_t v = static_cast<vid_t>(a.out.lo + r);
      const vid_t c = a.colour[v];
      if (a.scc[v] != kSccNone || c == kSccNone) continue;
      bool join = c == v;
      for (eid_t e = a.out.row_off[r]; e < a.out.row_off[r + 1] && !join; ++e) join = a.scc[a.out.col[e]] == c;
      if (join) {
        a.scc[v] = c;
        ++*a.changed;
      }
    }
  }
  void scc_end_round(const SccArgs& a) override {
    for (int64_t v = 0; v < a.out.n; ++v)
      if (a.scc[v] == kSccNone && a.colour[v] != kSccNone) a.cls[v] = a.colour[v];
  }
  void scc_relabel(const SccArgs& a) override {
    vid_t to = kSccNone;
    for (int64_t v = 0; v < a.out.n; ++v) {
      if (a.scc[v] != a.pivot) continue;
      if (to == kSccNone) to = static_cast<vid_t>(v);  // (ascending: the first member is the smallest)
      a.scc[v] = to;
    }
  }
  // eccentricity bounding (EccArgs): the device's stages as plain loops
  void ecc_degrees(const EccArgs& a) override {
    for (int64_t r = 0; r < a.g.rows; ++r) a.deg_own[r] = static_cast<uint32_t>(a.g.row_off[r + 1] - a.g.row_off[r]);
  }
  void ecc_init(const EccArgs& a) override {
    for (int64_t v = 0; v < a.g.n; ++v) {
      const bool in = a.scope_all || a.comp[v] == a.label;
      const bool empty = a.deg[v] == 0u;
      a.lo[v] = in ? 0 : -1;
      a.hi[v] = in ? (empty ? 0 : INT32_MAX) : -1;
      a.state[v] = in ? kEccScope | (empty ? kEccSettled : kEccLive) : 0u;
    }
  }
  void ecc_select(const EccArgs& a) override {
    auto key = [](uint32_t value, int64_t v) {
      return (static_cast<uint64_t>(value) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(v));
    };
    const int32_t max_lo = static_cast<int32_t>(a.totals[kEccMaxLo]), min_hi = static_cast<int32_t>(a.totals[kEccMinHi]);
    std::vector<uint64_t> by_hi, by_lo;
    for (int64_t v = 0; v < a.g.n; ++v) {
      if (!(a.state[v] & kEccLive)) continue;
      if ((a.target == EccTarget::Diameter && a.hi[v] <= max_lo) || (a.target == EccTarget::Radius && a.lo[v] >= min_hi)) {
        a.state[v] &= ~kEccLive;
        continue;
      }
      if (a.first) {
        by_lo.push_back(key(a.deg[v], v));
      } else {
        by_hi.push_back(key(static_cast<uint32_t>(a.hi[v]), v));
        by_lo.push_back(key(static_cast<uint32_t>(INT32_MAX - a.lo[v]), v));
      }
    }
    const int64_t live = static_cast<int64_t>(by_lo.size());
    auto best = [](std::vector<uint64_t>& keys, size_t k) {
      k = std::min(k, keys.size());
      std::partial_sort(keys.begin(), keys.begin() + static_cast<std::ptrdiff_t>(k), keys.end(), std::greater<uint64_t>());
      keys.resize(k);
    };
    best(by_hi, kEccSelHi);
    // (the second list skips the first's vertices: kEccSelHi more of them cover that)
    best(by_lo, static_cast<size_t>(kMsSources) + by_hi.size());
    int64_t k = 0;
    for (uint64_t x : by_hi) a.sel_out[1 + k++] = 0xFFFFFFFFu - static_cast<uint32_t>(x);
    const int64_t n_hi = k;
    for (uint64_t x : by_lo) {
      const int64_t v = 0xFFFFFFFFu - static_cast<uint32_t>(x);
      if (k == kMsSources) break;
      if (std::find(a.sel_out + 1, a.sel_out + 1 + n_hi, v) == a.sel_out + 1 + n_hi) a.sel_out[1 + k++] = v;
    }
    a.sel_out[0] = k;
    for (int64_t i = k; i < kMsSources; ++i) a.sel_out[1 + i] = -1;
    a.sel_out[1 + kMsSources] = live;
  }
  void ecc_update(const EccArgs& a) override {
    const int none = ms_unreached(a.m.lvl_bytes);
    for (int64_t v = 0; v < a.g.n; ++v) {
      if (!(a.state[v] & kEccLive)) continue;
      int32_t lo = a.lo[v], hi = a.hi[v];
      for (int s = 0; s < a.m.k; ++s) {
        const int d = level_at(a.m, v, s);
        if (d == none) continue;
        lo = std::max(lo, std::max(d, a.ecc[s] - d));
        hi = std::min(hi, a.ecc[s] + d);
      }
      a.lo[v] = lo;
      a.hi[v] = hi;
      if (lo >= hi) a.state[v] = (a.state[v] & ~kEccLive) | kEccSettled;
    }
  }
  void ecc_totals(const EccArgs& a) override {
    int64_t t[kEccTotals] = {};
    t[kEccMaxLo] = -1;
    t[kEccMinHi] = INT32_MAX;
    for (int64_t v = 0; v < a.g.n; ++v) {
      const uint32_t st = a.state[v];
      if (!(st & kEccScope)) continue;
      ++t[kEccScopeSize];
      t[kEccLiveN] += (st & kEccLive) ? 1 : 0;
      if (st & kEccSettled) {
        ++t[kEccSettledN];
        t[kEccAtHi] += a.lo[v] == a.count_hi ? 1 : 0;
        t[kEccAtLo] += a.lo[v] == a.count_lo ? 1 : 0;
      }
      t[kEccMaxLo] = std::max<int64_t>(t[kEccMaxLo], a.lo[v]);
      t[kEccMinHi] = std::min<int64_t>(t[kEccMinHi], a.hi[v]);
    }
    std::copy(t, t + kEccTotals, a.totals);
  }
  void ms_bc_forward(const MsBcArgs& a) override {
    bc_value_type(a, [&](auto val) {
      using V = decltype(val);
      for (int64_t r = 0; r < a.g.rows; ++r) {
        bool any = false;
        for (int s = 0; s < a.m.k; ++s) {
          if (level_at(a.m, a.g.lo + r, s) != a.level) continue;
          any = true;
          V::store_forward(a, r, s, bc_row_sum<V>(a, r, s, a.level - 1));
        }
        if (any && a.walked) ++*a.walked;
      }
    });
  }
  void ms_bc_backward(const MsBcArgs& a) override {
    bc_value_type(a, [&](auto val) {
      using V = decltype(val);
      for (int64_t r = 0; r < a.g.rows; ++r) {
        const int64_t v = a.g.lo + r;
        double lane[kMsSources] = {};
        bool any = false, counts = false;
        for (int s = 0; s < a.m.k; ++s) {
          if (level_at(a.m, v, s) != a.level) continue;
          any = true;
          const double delta = V::store_backward(a, r, s, a.leaf ? V::sum_zero() : bc_row_sum<V>(a, r, s, a.level + 1));
          if (v != a.m.src[s]) {
            lane[s] = delta;
            counts = true;
          }
        }
        if (any && a.walked) ++*a.walked;
        if (!counts) continue;
        for (int off = kMsSources / 2; off > 0; off >>= 1)
          for (int i = 0; i < off; ++i) lane[i] += lane[i + off];
        a.dep[r] += lane[0];
      }
    });
  }
  void* alloc_mapped(size_t bytes, void** dptr) override {
    void* h = std::calloc(1, std::max<size_t>(bytes, 1));
    DBFS_CHECK(h != nullptr, "host allocation failed");
    *dptr = h;
    return h;
  }
  void free_mapped(void* h) override { std::free(h); }

  void scan_units(const ScanArgs& a) override {
    if (!a.guard.live()) return;
    const int64_t nchunks = div_up(a.nunits, kScanChunk);
    int64_t c = 0, d = 0;
    for (int64_t k = 0; k < nchunks; ++k) {
      int64_t ic = 0, id = 0;
      for (int64_t u = k * kScanChunk; u < std::min<int64_t>(a.nunits, (k + 1) * kScanChunk); ++u) {
        const int64_t tc = a.unit_cnt[u], td = a.unit_deg[u];
        a.unit_cnt[u] = ic;
        a.unit_deg[u] = id;
        ic += tc;
        id += td;
      }
      a.part_cnt[k] = c;
      a.part_deg[k] = d;
      c += ic;
      d += id;
    }
    a.stats[0] = a.stats[2] = c;
    a.stats[1] = a.stats[3] = d;
    a.qscan[c] = d;
    if (a.stamp.ctrl && a.finish) finish_level(a.stamp, *a.stamp.ctrl, c, d);
  }

  void zero_degree_mask(const ZeroDegArgs& a) override {
    for (int64_t w = 0; w < a.words; ++w) {
      word_t m = 0;
      for (int b = 0; b < 64; ++b) {
        const int64_t v = w * 64 + b;
        if (v >= a.g.rows || (!a.padding_only && a.g.row_off[v + 1] == a.g.row_off[v])) m |= 1ull << b;
      }
      a.out[w] = m;
    }
  }

  void compact_frontier(const CompactArgs& a) override {
    if (!a.guard.live()) return;
    const int64_t nunits = div_up(a.words, kUnitWords);
    for (int64_t u = 0; u < nunits; ++u) {
      int64_t pos = a.unit_cnt_off[u] + a.part_cnt[u / kScanChunk];
      int64_t off = a.unit_deg_off[u] + a.part_deg[u / kScanChunk];
      for (int64_t w = u * kUnitWords; w < std::min<int64_t>(a.words, (u + 1) * kUnitWords); ++w) {
        word_t x = a.frontier[w];
        if (a.clear) a.clear[w] = 0;
        if (a.clear_all) a.clear_all[w] = 0;
        while (x) {
          const int b = __builtin_ctzll(x);
          x &= x - 1;
          const int64_t v = w * 64 + b;
          const eid_t rs = a.g.row_off[v], d = a.g.row_off[v + 1] - rs;
          if (d <= 0) continue;
          a.wl.qscan[pos] = off;
          a.wl.qbase[pos] = rs - off;
          if (a.wl.qv) a.wl.qv[pos] = static_cast<vid_t>(v);
          for (int64_t blk = div_up(off, kTdEdgesPerBlock); blk * kTdEdgesPerBlock < off + d; ++blk)
            a.wl.blk_vstart[blk] = static_cast<int32_t>(pos);
          ++pos;
          off += d;
        }
      }
    }
  }

  void td_expand(const TdArgs& a) override {
    int64_t q = a.q;
    bool bytes = a.next_bytes != nullptr;
    if (!a.guard.live()) return;
    if (a.guard.ctrl) {
      q = a.dev_stats[0];
      bytes = a.guard.ctrl->bytes != 0;
      if (a.clear_frontier)
        for (int64_t i = 0; i < q; ++i) a.clear_frontier[a.in.qv[i] >> 6] = 0;
    }
    // a split level's part (TdArgs::split_k): its run of the level's edges
    const int64_t m = a.guard.ctrl ? a.dev_stats[1] : a.m;
    const int64_t e_lo = a.split_k > 1 ? m * a.split_i / a.split_k : 0;
    const int64_t e_hi = a.split_k > 1 ? m * (a.split_i + 1) / a.split_k : m;
    for (int64_t i = 0; i < q; ++i) {
      const int64_t b = std::max(a.in.qscan[i], e_lo), e = std::min(a.in.qscan[i + 1], e_hi);
      for (int64_t k = b; k < e; ++k) {
        const vid_t v = a.g.col[k + a.in.qbase[i]];
        // (the filter's clear bits are visited vertices: skipping on them
        // changes nothing -- and catches a filter that drops an unvisited one)
        if (a.unvis && !test_bit(a.unvis, unvis_index(v, a.unvis_mult))) continue;
        if (test_bit(a.visited, v)) continue;
        if (a.lists) {
          vid_t* list = a.lists + static_cast<int64_t>(v / a.part) * (a.list_cap + 1);
          list[1 + list[0]++] = v;
        } else if (bytes && a.level_direct) {
          a.level_direct[v] = a.out.byte();
        } else if (bytes) {
          a.next_bytes[v] = 1;
        } else {
          a.next[v >> 6] |= 1ull << (v & 63);
        }
      }
    }
  }

  void td_binned(const BinArgs& a) override {
    if (!a.guard.live()) return;
    const int64_t q = a.dev_stats[0];
    if (a.clear_frontier)
      for (int64_t i = 0; i < q; ++i) a.clear_frontier[a.in.qv[i] >> 6] = 0;
    std::vector<word_t> nb(static_cast<size_t>(a.words), 0);
    for (int64_t i = 0; i < q; ++i)
      for (int64_t k = a.in.qscan[i]; k < a.in.qscan[i + 1]; ++k) {
        const vid_t v = a.g.col[k + a.in.qbase[i]];
        if (!test_bit(a.visited, v)) nb[v >> 6] |= 1ull << (v & 63);
      }
    for (int64_t w = 0; w < a.words; ++w) {
      a.frontier[w] = nb[w];
      a.visited[w] |= nb[w];
    }
    // the apply's settle and finish: the claimed words are the new frontier
    // (an update with force over them: levels, unit statistics, the fused
    // finish with its folded scan)
    UpdateArgs u;
    u.g = a.g;
    u.cand = a.frontier;
    u.force = true;
    u.visited = a.visited;
    u.frontier = a.frontier;
    u.out = a.out;
    u.words = a.words;
    u.unit_cnt = a.unit_cnt;
    u.unit_deg = a.unit_deg;
    u.guard = a.guard;
    u.fuse_scan = true;
    u.fold_scan = a.fin.fold_scan;
    u.scan = a.fin.scan;
    update_frontier(u);
  }

  void level_finish(const LevelFinishArgs& a) override {
    if (!a.stamp.seed && !a.guard.live()) return;
    finish_level(a.stamp, a.stamp.seed ? a.ctrl_init : *a.stamp.ctrl, a.stats[2], a.stats[3]);
  }

  // Sparse top-down level (see the HIP kernel): claims in the replicated
  // visited bitmap; owned claims settled into the next work list (the running
  // totals in sparse_cnt_ / sparse_deg_), remote ones (several ranks) appended
  // to their owners' lists; without lists the level is finished here.
  void sparse_settle(const TdSparseArgs& a, vid_t v) {
    const int64_t r = static_cast<int64_t>(v) - a.g.lo;
    DBFS_CHECK(r >= 0 && r < a.g.rows, "sparse level: settled vertex outside this shard");
    a.out.store(r);
    const eid_t rs = a.g.row_off[r], d = a.g.row_off[r + 1] - rs;
    if (d <= 0) return;
    a.frontier_out[r >> 6] |= 1ull << (r & 63);
    const int64_t cnt = sparse_cnt_, deg = sparse_deg_;
    a.next.qscan[cnt] = deg;
    a.next.qbase[cnt] = rs - deg;
    a.next.qv[cnt] = static_cast<vid_t>(r);
    for (int64_t blk = div_up(deg, kTdEdgesPerBlock); blk * kTdEdgesPerBlock < deg + d; ++blk)
      a.next.blk_vstart[blk] = static_cast<int32_t>(cnt);
    ++sparse_cnt_;
    sparse_deg_ += d;
  }
  void sparse_finish_totals(const TdSparseArgs& a) {
    a.stats[0] = a.stats[2] = sparse_cnt_;
    a.stats[1] = a.stats[3] = sparse_deg_;
    a.next.qscan[sparse_cnt_] = sparse_deg_;
  }
  void td_sparse(const TdSparseArgs& a) override {
    DBFS_CHECK(!a.direct.active, "CpuBackend: no direct list exchange (peer windows are GPU memory)");
    if (!a.guard.live()) return;
    // the input frontier's rows [col_begin, col_end), in work-list order (a
    // bitmap input: its set bits in (word, bit) order, as a compaction lists them)
    std::vector<std::pair<eid_t, eid_t>> rows;
    if (a.from_bits) {
      for (int64_t w = 0; w < a.words; ++w) {
        for (word_t m = a.frontier_in[w]; m; m &= m - 1) {
          const int64_t r = w * kWordBits + __builtin_ctzll(m);
          rows.emplace_back(a.g.row_off[r], a.g.row_off[r + 1]);
        }
        a.frontier_in[w] = 0;
      }
    } else {
      const int64_t q = a.dev_stats[0];
      for (int64_t i = 0; i < q; ++i) a.frontier_in[a.in.qv[i] >> 6] = 0;
      for (int64_t i = 0; i < q; ++i)
        rows.emplace_back(a.in.qscan[i] + a.in.qbase[i], a.in.qscan[i + 1] + a.in.qbase[i]);
    }
    sparse_cnt_ = sparse_deg_ = 0;
    for (const auto& [cb, ce] : rows) {
      for (eid_t k = cb; k < ce; ++k) {
        const vid_t v = a.g.col[k];
        if (test_bit(a.visited, v)) continue;
        a.visited[v >> 6] |= 1ull << (v & 63);
        const int64_t r = static_cast<int64_t>(v) - a.g.lo;
        if (a.lists && (r < 0 || r >= a.g.rows)) {
          vid_t* list = a.lists + (static_cast<int64_t>(v) / a.part) * a.list_stride;
          DBFS_CHECK(static_cast<int64_t>(list[0]) + 1 < a.list_stride, "owner list overflow");
          list[1 + list[0]++] = v;
          continue;
        }
        sparse_settle(a, v);
      }
    }
    if (a.lists) return;  // several ranks: td_sparse_apply finishes
    sparse_finish_totals(a);
    finish_level(a.stamp, *a.stamp.ctrl, sparse_cnt_, sparse_deg_);
  }
  void td_sparse_apply(const TdSparseArgs& a) override {
    DBFS_CHECK(!a.direct.active, "CpuBackend: no direct list exchange (peer windows are GPU memory)");
    if (!a.guard.live()) return;
    for (int r = 0; r < a.nranks; ++r) {
      const vid_t* list = a.recv_lists + static_cast<int64_t>(r) * a.list_stride;
      for (vid_t k = 0; k < list[0]; ++k) {
        const vid_t v = list[1 + k];
        if (test_bit(a.visited, v)) continue;
        a.visited[v >> 6] |= 1ull << (v & 63);
        sparse_settle(a, v);
      }
    }
    for (int r = 0; r < a.nranks; ++r) a.lists[static_cast<int64_t>(r) * a.list_stride] = 0;
    sparse_finish_totals(a);
  }
  int64_t sparse_cnt_ = 0, sparse_deg_ = 0;  // the current sparse level's settled entries / their edges

  // (no device checks in the CPU kernels; the injected violation exercises
  // the engine's failure path on the CPU: one word, reported with the file
  // the injection named)
  uint64_t take_device_check(CheckFile* file) override {
    if (file) *file = check_file_;
    return std::exchange(check_, 0);
  }
  void inject_device_check(CheckFile f) override {
    check_ = 99ull << 48;
    check_file_ = f;
  }
  uint64_t check_ = 0;
  CheckFile check_file_ = CheckFile::Bfs;

  void list_scatter(const ListScatterArgs& a) override {
    for (int r = 0; r < a.nranks; ++r) {
      const vid_t* list = a.lists + static_cast<int64_t>(r) * (a.list_cap + 1);
      for (vid_t k = 0; k < list[0]; ++k) {
        const int64_t v = static_cast<int64_t>(list[1 + k]) - a.lo;
        a.cand[v >> 6] |= 1ull << (v & 63);
      }
    }
  }

  void pack_bytes(const PackArgs& a) override {
    if (!a.guard.live() || (a.guard.ctrl && !(a.flag ? *a.flag : a.guard.ctrl->bytes))) return;
    for (int64_t w = 0; w < a.words; ++w)
      if (w < a.skip_begin || w >= a.skip_end) a.next[w] |= gather_bytes(a.bytes + w * 64);
  }

  void bu_step(const BuArgs& a) override {
    if (a.fuse_scan) {
      // totals and finish right after the step; the unit statistics stay
      // unscanned (as the HIP kernel's fused finish leaves them)
      BuArgs b = a;
      b.fuse_scan = false;
      bu_step(b);
      const int64_t n = a.scan.nunits;
      std::vector<int64_t> c(a.scan.unit_cnt, a.scan.unit_cnt + n), d(a.scan.unit_deg, a.scan.unit_deg + n);
      scan_units(a.scan);
      std::copy(c.begin(), c.end(), a.scan.unit_cnt);
      std::copy(d.begin(), d.end(), a.scan.unit_deg);
      return;
    }
    if (!a.guard.live()) return;
    // hub-cut level (as the HIP kernel): claimed vertices join the output
    // unscanned, the others find parents among the frontier hubs only
    const bool cut = a.cut_edges > 0 && *a.cut_flag;
    const int64_t nunits = div_up(a.words, kUnitWords);
    for (int64_t u = 0; u < nunits; ++u) {
      int64_t cnt = 0, deg = 0;
      for (int64_t w = u * kUnitWords; w < std::min<int64_t>(a.words, (u + 1) * kUnitWords); ++w) {
        // claimed: unvisited with this level's level byte already
        word_t pw = 0;
        if (cut)
          for (int b = 0; b < 64 && w * 64 + b < a.g.rows; ++b) {
            const int64_t v = w * 64 + b;
            const bool claimed =
                a.cut_claim ? a.cut_claim[v] != 0
                            : a.out.level8[v] == static_cast<uint8_t>(a.out.narrow_base +
                                                                      std::min<lvl_t>(a.out.new_level, kNarrowMaxLevel + 1));
            if (!((a.visited[w] >> b) & 1ull) && claimed) {
              pw |= 1ull << b;
              if (a.cut_claim) {
                a.cut_claim[v] = 0;
                a.out.level[v] = a.out.new_level;
              }
            }
          }
        word_t out = pw;
        const word_t vis = a.visited[w] | pw;
        for (word_t m = pw; m; m &= m - 1) {
          const int64_t v = w * 64 + __builtin_ctzll(m);
          ++cnt;
          deg += a.g.row_off[v + 1] - a.g.row_off[v];
        }
        for (int b = 0; b < 64; ++b) {
          const int64_t v = w * 64 + b;
          if (v >= a.g.rows || ((vis >> b) & 1ull)) continue;
          for (eid_t e = a.g.row_off[v]; e < a.g.row_off[v + 1]; ++e) {
            if (test_bit(a.frontier, a.g.col[e]) && (!cut || test_bit(a.g.hub_bits, a.g.col[e]))) {
              out |= 1ull << b;
              a.out.store(v);
              ++cnt;
              deg += a.g.row_off[v + 1] - a.g.row_off[v];
              break;
            }
          }
        }
        a.visited[w] = vis | out;
        a.new_frontier[w] = out;
      }
      a.unit_cnt[u] = cnt;
      a.unit_deg[u] = deg;
    }
  }

  void status_expand(const StatusArgs& a) override {
    for (int64_t v = 0; v < a.g.rows; ++v) {
      if (a.level[v] != a.cur) continue;
      for (eid_t e = a.g.row_off[v]; e < a.g.row_off[v + 1]; ++e) {
        const vid_t u = a.g.col[e];
        if (!test_bit(a.visited, u)) a.next[u >> 6] |= 1ull << (u & 63);
      }
    }
  }

  void bitmap_or(word_t* dst, const word_t* src, int64_t words) override {
    for (int64_t w = 0; w < words; ++w) dst[w] |= src[w];
  }

  void ref_expand(const RefExpandArgs& a) override {
    for (int64_t i = 0; i < a.q; ++i) {
      const int64_t u = static_cast<int64_t>(a.queue[i]) - a.g.lo;
      for (eid_t e = a.g.row_off[u]; e < a.g.row_off[u + 1]; ++e) {
        const vid_t v = a.g.col[e];
        if (a.dist[v] == kUnreached) {
          a.dist[v] = a.next_level;
          const int64_t owner = v / a.part;
          const int64_t pos = a.bucket_cnt[owner]++;
          a.buckets[owner * a.bucket_cap + pos] = v;
        }
      }
    }
  }

  void ref_accept(const RefAcceptArgs& a) override {
    for (int64_t i = 0; i < a.total; ++i) {
      const vid_t v = a.recv[i];
      bool keep;
      if (i >= a.self_begin && i < a.self_end) {
        keep = true;
      } else {
        keep = a.dist[v] == kUnreached;
        if (keep) a.dist[v] = a.next_level;
      }
      if (keep) a.queue[(*a.qcount)++] = v;
    }
  }

  // Scan mode: the same four passes as the HIP kernels (sequential, so the
  // claim is simply the first edge in queue order).
  void scan_relax(const ScanBfsArgs& a) override {
    for (int64_t i = 0; i < a.q; ++i) {
      const int64_t u = static_cast<int64_t>(a.queue[i]) - a.g.lo;
      for (eid_t e = a.g.row_off[u]; e < a.g.row_off[u + 1]; ++e) {
        const vid_t v = a.g.col[e];
        if (a.dist[v] == kUnreached) {
          a.dist[v] = a.next_level;
          a.claim[v] = e;
        }
      }
    }
  }
  void scan_count(const ScanBfsArgs& a) override {
    for (int64_t i = 0; i < a.q * a.nranks; ++i) a.offs[i] = 0;
    for (int64_t i = 0; i < a.q; ++i) {
      const int64_t u = static_cast<int64_t>(a.queue[i]) - a.g.lo;
      for (eid_t e = a.g.row_off[u]; e < a.g.row_off[u + 1]; ++e) {
        const vid_t v = a.g.col[e];
        if (a.dist[v] == a.next_level && a.claim[v] == e) ++a.offs[(v / a.part) * a.q + i];
      }
    }
  }
  void scan_bounds(const ScanBfsArgs& a) override {
    for (int o = 0; o <= a.nranks; ++o) a.bounds[o] = a.offs[o * a.q];
    for (int o = 0; o < a.nranks; ++o) a.counts[o] = a.bounds[o + 1] - a.bounds[o];
  }
  void scan_assign(const ScanBfsArgs& a) override {
    for (int64_t i = 0; i < a.q; ++i) {
      const int64_t u = static_cast<int64_t>(a.queue[i]) - a.g.lo;
      for (eid_t e = a.g.row_off[u]; e < a.g.row_off[u + 1]; ++e) {
        const vid_t v = a.g.col[e];
        if (a.dist[v] == a.next_level && a.claim[v] == e) a.out[a.offs[(v / a.part) * a.q + i]++] = v;
      }
    }
  }

  void validate_levels(const ValidateArgs& a) override {
    int64_t gap = 0, cross = 0, orphan = 0;
    for (int64_t r = 0; r < a.g.rows; ++r) {
      const int64_t u = a.g.lo + r;
      const lvl_t lu = a.level_global[u];
      bool has_parent = false;
      for (eid_t e = a.g.row_off[r]; e < a.g.row_off[r + 1]; ++e) {
        const lvl_t lv = a.level_global[a.g.col[e]];
        if (a.directed) {
          // (in-edge row of u: the entry is col[e] -> u)
          if (lv == kUnreached) continue;
          if (lu == kUnreached) { ++cross; continue; }
          if (lu - lv > 1) ++gap;
        } else {
          if (lu == kUnreached && lv == kUnreached) continue;
          if ((lu == kUnreached) != (lv == kUnreached)) { ++cross; continue; }
          if (lu - lv > 1 || lv - lu > 1) ++gap;
        }
        if (lv == lu - 1) has_parent = true;
      }
      if (lu != kUnreached && u != a.src && !has_parent) ++orphan;
      if (u == a.src && lu != 0) ++orphan;
    }
    a.out[0] += gap;
    a.out[1] += cross;
    a.out[2] += orphan;
  }

  void compute_parents(const ParentArgs& a) override {
    for (int64_t r = 0; r < a.g.rows; ++r) {
      const int64_t v = a.g.lo + r;
      const lvl_t lv = a.level_global[v];
      int64_t par = -1;
      if (v == a.src) {
        par = v;
      } else if (lv != kUnreached) {
        for (eid_t e = a.g.row_off[r]; e < a.g.row_off[r + 1]; ++e) {
          if (a.level_global[a.g.col[e]] == lv - 1) { par = a.g.col[e]; break; }
        }
      }
      a.parent[r] = par;
    }
  }

  void degrees_u32(const eid_t* ro, int64_t rows, uint32_t* out) override {
    for (int64_t r = 0; r < rows; ++r) {
      const eid_t d = ro[r + 1] - ro[r];
      out[r] = d > 0xFFFFFFFFll ? 0xFFFFFFFFu : static_cast<uint32_t>(d);
    }
  }

  void sort_neighbors(const eid_t* ro, vid_t* col, int64_t rows, const uint32_t* key_deg) override {
    // Same policy as the device: rows of 2..4096 entries, (degree desc, id asc).
    for (int64_t r = 0; r < rows; ++r) {
      const eid_t len = ro[r + 1] - ro[r];
      if (len < 2 || len > 4096) continue;
      std::sort(col + ro[r], col + ro[r + 1], [&](vid_t x, vid_t y) {
        return key_deg[x] != key_deg[y] ? key_deg[x] > key_deg[y] : x < y;
      });
    }
  }

  void sort_rows_by_id(const eid_t* ro, vid_t* col, int64_t rows, int64_t n, bool exact_long) override {
    (void)n;
    (void)exact_long;  // (every row is sorted exactly here)
    for (int64_t r = 0; r < rows; ++r) std::sort(col + ro[r], col + ro[r + 1]);
  }

  void encode_hub_cols(const vid_t* col, int64_t nnz, const uint32_t* hub_idx, vid_t* out) override {
    for (int64_t e = 0; e < nnz; ++e) out[e] = hub_idx[col[e]] != 0xFFFFFFFFu ? (kHubFlag | hub_idx[col[e]]) : col[e];
  }
  void nz_word_counts(const eid_t* ro, int64_t rows, int64_t words, eid_t* counts) override {
    for (int64_t w = 0; w < words; ++w) {
      eid_t c = 0;
      for (int64_t v = w * 64; v < std::min<int64_t>(rows, (w + 1) * 64); ++v) c += ro[v + 1] > ro[v] ? 1 : 0;
      counts[w] = c;
    }
  }
  void nz_fill(const eid_t* ro, const vid_t* head, int64_t rows, const eid_t* pref, eid_t* nz_ro,
               vid_t* nz_head) override {
    int64_t k = 0;
    for (int64_t v = 0; v < rows; ++v) {
      if (ro[v + 1] > ro[v]) {
        nz_ro[k] = ro[v];
        nz_head[k] = head[v];
        ++k;
      }
    }
    nz_ro[k] = rows > 0 ? ro[rows] : 0;
    (void)pref;
  }
  void nz_records(const eid_t* ro, const vid_t* head, int64_t rows, const eid_t* pref, NzRec* rec, uint16_t* loc,
                  eid_t* unit_base) override {
    const int64_t nunits = div_up(std::max<int64_t>(rows, 1), kUnitVertices);
    for (int64_t u = 0; u <= nunits; ++u) unit_base[u] = ro[std::min<int64_t>(u * kUnitVertices, rows)];
    int64_t k = 0;
    for (int64_t v = 0; v < rows; ++v) {
      if (ro[v + 1] > ro[v]) {
        rec[k].off = static_cast<uint32_t>(ro[v] - unit_base[v / kUnitVertices]);
        rec[k].head = head[v];
        loc[k] = static_cast<uint16_t>(v % kUnitVertices);
        ++k;
      }
    }
    (void)pref;
  }
  int64_t select_hubs(const uint32_t* deg, int64_t n, uint32_t min_deg, vid_t* hub_vertex,
                      uint32_t* hub_idx) override {
    int64_t k = 0;
    for (int64_t v = 0; v < n; ++v) {
      if (deg[v] >= min_deg) {
        hub_vertex[k] = static_cast<vid_t>(v);
        hub_idx[v] = static_cast<uint32_t>(k++);
      } else {
        hub_idx[v] = 0xFFFFFFFFu;
      }
    }
    return k;
  }
  void hub_gather(const HubGatherArgs& a) override {
    if (!a.guard.live()) return;
    for (int64_t w = 0; w < div_up(a.g.nhubs, 64); ++w) {
      word_t m = 0;
      int64_t d = 0;
      for (int b = 0; b < 64 && w * 64 + b < a.g.nhubs; ++b) {
        const vid_t hv = a.g.hub_vertex[w * 64 + b];
        if (test_bit(a.frontier, hv)) {
          m |= 1ull << b;
          if (a.cut_part) d += a.g.hub_deg ? a.g.hub_deg[w * 64 + b] : a.g.row_off[hv + 1] - a.g.row_off[hv];
        }
      }
      a.hub_front[w] = m;
      if (a.cut_part) a.cut_part[w] = d;
    }
    if (a.cut_part) {
      int64_t hub_edges = 0;
      for (int64_t w = 0; w < div_up(a.g.nhubs, 64); ++w) hub_edges += a.cut_part[w];
      *a.cut_flag = a.guard.ctrl->m_f - hub_edges <= a.cut_edges ? 1 : 0;
    }
    if (a.visited)
      for (int64_t i = 0; i < a.words; ++i) a.visited[i] |= a.frontier[i];
  }
  void bu_cut_prep(const BuArgs& a) override {
    if (!a.guard.live()) return;
    if (!*a.cut_flag) return;
    const bool x = a.cut_bytes != nullptr;
    DBFS_CHECK(x || a.g.lo == 0, "bu_cut_prep: a shard past vertex 0 needs the several-rank arguments");
    const int64_t lo = a.g.lo, off = x ? a.cut_word_off : 0;
    const word_t* vis = x ? a.cut_vis : a.visited;
    for (int64_t w = 0; w < a.words; ++w)
      for (word_t m = a.frontier[off + w] & ~a.g.hub_bits[off + w]; m; m &= m - 1) {
        const int64_t v = w * 64 + __builtin_ctzll(m);
        for (eid_t e = a.g.row_off[v]; e < a.g.row_off[v + 1]; ++e) {
          const vid_t t = a.g.col[e];
          if (test_bit(vis, t)) continue;
          const int64_t r = static_cast<int64_t>(t) - lo;
          if (r < 0 || r >= a.g.rows) {
            DBFS_CHECK(x, "bu_cut_prep: a remote neighbour without the several-rank arguments");
            a.cut_bytes[t] = 1;
            continue;
          }
          if (a.cut_claim) a.cut_claim[r] = 1;
          else a.out.store(r);
        }
      }
  }
  void bu_cut_merge(const BuArgs& a) override {
    DBFS_CHECK(a.cut_flag && a.cut_recv && a.cut_next && (a.out.level8 || a.cut_claim) && a.cut_nranks > 1,
               "bu_cut_merge: several ranks' hub-cut arguments missing");
    if (!a.guard.live()) return;
    if (!*a.cut_flag) return;
    for (int64_t w = 0; w < a.words; ++w) {
      word_t c = 0;
      for (int p = 0; p < a.cut_nranks; ++p) {
        if (p == a.cut_rank) continue;
        c |= a.cut_recv[p * a.words + w];
        a.cut_next[p * a.words + w] = 0;
      }
      for (c &= ~a.visited[w]; c; c &= c - 1) {
        const int64_t r = w * 64 + __builtin_ctzll(c);
        if (a.cut_claim) a.cut_claim[r] = 1;
        else a.out.store(r);
      }
    }
  }
  void hub_apply(const HubApplyArgs& a) override {
    if (!a.guard.live()) return;
    for (int64_t h = 0; h < a.g.td_nhubs; ++h) {
      if (!a.mark[h]) continue;
      const vid_t v = a.g.td_hub_vertex[h];
      a.out.level8[v] = a.out.byte();
      a.mark[h] = 0;
    }
  }
  void refresh_visited(const RefreshArgs& a) override {
    if (!a.guard.live()) return;
    const uint8_t lv = a.out.byte();
    for (int64_t w = 0; w < a.words; ++w) {
      word_t m = 0;
      for (int b = 0; b < 64; ++b)
        if (a.out.level8[w * 64 + b] == lv) m |= 1ull << b;
      a.visited[w] |= m;
    }
  }
  void hub_visited(const HubVisitedArgs& a) override {
    if (!a.guard.live()) return;
    for (int64_t w = 0; w < div_up(a.g.td_nhubs, 64); ++w) {
      word_t m = 0;
      for (int b = 0; b < 64 && w * 64 + b < a.g.td_nhubs; ++b)
        if (test_bit(a.visited, a.g.td_hub_vertex[w * 64 + b])) m |= 1ull << b;
      a.out[w] = m;
    }
  }
  void unvis_filter(const UnvisArgs& a) override {
    if (!a.guard.live()) return;
    std::fill(a.out, a.out + kUnvisWords, word_t(0));
    for (int64_t v = 0; v < a.n; ++v)
      if (!test_bit(a.visited, static_cast<vid_t>(v))) {
        const uint32_t i = unvis_index(static_cast<uint64_t>(v), a.mult);
        a.out[i >> 6] |= 1ull << (i & 63);
      }
  }
  void row_heads(const eid_t* ro, const vid_t* col, int64_t rows, vid_t* head, const uint32_t* hub_idx) override {
    for (int64_t r = 0; r < rows; ++r) {
      vid_t h = ro[r + 1] > ro[r] ? col[ro[r]] : 0u;
      if (hub_idx && ro[r + 1] > ro[r] && hub_idx[h] != 0xFFFFFFFFu) h = kHubFlag | hub_idx[h];
      head[r] = h;
    }
  }

  void gen_count_degrees(const GenParams& p, int64_t lo, int64_t rows, eid_t* deg) override {
    for (int64_t i = 0; i < p.m; ++i) {
      uint64_t u, v;
      gen_edge(p, static_cast<uint64_t>(i), u, v);
      if (static_cast<int64_t>(u) >= lo && static_cast<int64_t>(u) < lo + rows) ++deg[u - lo];
      if (static_cast<int64_t>(v) >= lo && static_cast<int64_t>(v) < lo + rows) ++deg[v - lo];
    }
  }

  void exclusive_scan(eid_t* data, int64_t n) override {
    eid_t acc = 0;
    for (int64_t i = 0; i < n; ++i) {
      const eid_t t = data[i];
      data[i] = acc;
      acc += t;
    }
    data[n] = acc;
  }

  void route_edges_count(const vid_t* u, const vid_t* v, int64_t m, int64_t part, int nranks,
                         int64_t* counts) override {
    for (int64_t i = 0; i < m; ++i) {
      ++counts[u[i] / part];
      ++counts[v[i] / part];
    }
    (void)nranks;
  }
  void route_edges_fill(const vid_t* u, const vid_t* v, int64_t m, int64_t part, int nranks, int64_t* cursor,
                        uint64_t* out) override {
    // edge order within every destination segment (the reference's adjacency
    // order survives the exchange: segments arrive in rank = file order)
    for (int64_t i = 0; i < m; ++i) {
      out[cursor[u[i] / part]++] = (static_cast<uint64_t>(u[i]) << 32) | v[i];
      out[cursor[v[i] / part]++] = (static_cast<uint64_t>(v[i]) << 32) | u[i];
    }
    (void)nranks;
  }
  void in_route_count(const ShardView& g, int64_t part, int nranks, int64_t* counts) override {
    for (eid_t e = 0; e < g.nnz; ++e) ++counts[g.col[e] / part];
    (void)nranks;
  }
  void in_route_fill(const ShardView& g, int64_t part, int nranks, int64_t* cursor, uint64_t* out) override {
    for (int64_t r = 0; r < g.rows; ++r)
      for (eid_t e = g.row_off[r]; e < g.row_off[r + 1]; ++e)
        out[cursor[g.col[e] / part]++] = (static_cast<uint64_t>(g.col[e]) << 32) | static_cast<uint64_t>(g.lo + r);
    (void)nranks;
  }
  void entries_count(const uint64_t* e, int64_t k, int64_t lo, eid_t* deg) override {
    for (int64_t i = 0; i < k; ++i) ++deg[static_cast<int64_t>(e[i] >> 32) - lo];
  }
  void entries_fill(const uint64_t* e, int64_t k, int64_t lo, eid_t* cursor, vid_t* col) override {
    for (int64_t i = 0; i < k; ++i)
      col[cursor[static_cast<int64_t>(e[i] >> 32) - lo]++] = static_cast<vid_t>(e[i] & 0xFFFFFFFFull);
  }
  void gen_fill(const GenParams& p, int64_t lo, int64_t rows, eid_t* cursor, vid_t* col) override {
    // Same order as build_csr (edge order, u-side then v-side).
    for (int64_t i = 0; i < p.m; ++i) {
      uint64_t u, v;
      gen_edge(p, static_cast<uint64_t>(i), u, v);
      if (static_cast<int64_t>(u) >= lo && static_cast<int64_t>(u) < lo + rows)
        col[cursor[u - lo]++] = static_cast<vid_t>(v);
      if (static_cast<int64_t>(v) >= lo && static_cast<int64_t>(v) < lo + rows)
        col[cursor[v - lo]++] = static_cast<vid_t>(u);
    }
  }

  void widen_levels(const uint8_t* in, lvl_t* out, int64_t n, uint8_t base) override {
    for (int64_t i = 0; i < n; ++i) {
      const uint8_t v = static_cast<uint8_t>(in[i] - base);
      out[i] = v > kNarrowMaxLevel ? kUnreached : static_cast<lvl_t>(v);
    }
  }
  void degree_moments(const ShardView& g, int64_t* out2) override {
    int64_t s = 0, c = 0;
    for (int64_t r = 0; r < g.rows; ++r) {
      const int64_t d = g.row_off[r + 1] - g.row_off[r];
      s += d * d;
      c += d > 0 ? 1 : 0;
    }
    out2[0] = s;
    out2[1] = c;
  }
  void reached_degree_sum(const ShardView& g, const lvl_t* level, int64_t* out2) override {
    int64_t c = 0, d = 0;
    for (int64_t r = 0; r < g.rows; ++r)
      if (level[r] != kUnreached) { ++c; d += g.row_off[r + 1] - g.row_off[r]; }
    out2[0] = c;
    out2[1] = d;
  }

 private:
  std::vector<std::chrono::steady_clock::time_point> events_;
};

}  // namespace

std::unique_ptr<Backend> make_cpu_backend() { return std::make_unique<CpuBackend>(); }

}  // namespace dbfs
