// Engine::strong_components: strongly connected components on the device
// (Backend::scc_*, backend.hpp SccArgs) -- rounds of trim, forward colouring
// over the in-edge rows and backward closure over the out-rows.  Every "until
// nothing changes" loop is here, over a device counter read after a few
// sweeps; each is bounded and refuses to go on past its bound.
#include <algorithm>
#include <chrono>

#include "dbfs/engine.hpp"

namespace dbfs {

namespace {

// One rank: sweeps enqueued between two reads of their changed counters, at
// most (2, 4, 8 while sweeps keep changing something).  Each sweep has a
// counter of its own and returns at once when the one before it changed
// nothing, so a surplus sweep costs a launch, not a pass.
constexpr int kSccBatch = 8;

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

}  // namespace

SccResult Engine::strong_components(const SccOptions& o) {
  const int P = part_.nranks;
  const int64_t n = part_.n;
  const int64_t trim_limit = o.trim_rounds < -1 ? opt_.scc_trim_rounds : o.trim_rounds;
  const bool use_pivot = o.pivot < 0 ? opt_.scc_pivot : o.pivot != 0;
  // every rank's slice padded to the partition's width: a slice is all-gathered whole
  const size_t len = static_cast<size_t>(std::max<int64_t>({n, static_cast<int64_t>(P) * part_.part, 1}));
  if (!scc_) {
    scc_ = std::make_unique<SccBuffers>();
    SccBuffers& b = *scc_;
    b.scc = DBuf<vid_t>(be_, len);
    b.cls = DBuf<vid_t>(be_, len);
    b.colour = DBuf<vid_t>(be_, len);
    if (P > 1) b.xchg = DBuf<vid_t>(be_, len);
    b.size = DBuf<uint32_t>(be_, static_cast<size_t>(std::max<int64_t>(n, 1)));
    b.words = DBuf<unsigned long long>(be_, kSccBatch + 3);
    b.pivot_slots = DBuf<unsigned long long>(be_, static_cast<size_t>(kSccPivotGrid) * 2);
    b.pivot_all = DBuf<unsigned long long>(be_, static_cast<size_t>(P) * 2);
    b.totals = DBuf<int64_t>(be_, kCcTotals);
    b.slots = DBuf<int64_t>(be_, static_cast<size_t>(kCcSizeGrid) * kCcTotals);
  }
  SccBuffers& b = *scc_;
  b.valid = false;
  SccArgs a;
  a.out = g_.view();
  a.in = check_view();  // (directed: the in-edge shard, built here when it is not there; else the graph's own rows)
  a.scc = b.scc.data();
  a.cls = b.cls.data();
  a.colour = b.colour.data();
  unsigned long long* const counters = b.words.data();  // kSccBatch of them
  a.pivot_out = b.words.data() + kSccBatch;
  a.relabel_min = reinterpret_cast<vid_t*>(b.words.data() + kSccBatch + 2);
  a.pivot_slots = b.pivot_slots.data();

  SccResult res;
  // Several ranks: every rank's owned slice of the array a sweep wrote, to every replica.
  auto exchange = [&](vid_t* arr) {
    if (P == 1) return;
    const size_t slice = static_cast<size_t>(part_.part) * sizeof(vid_t);
    comm_.allgather(arr + static_cast<int64_t>(comm_.rank()) * part_.part, b.xchg.data(), slice);
    be_.copy_async(arr, b.xchg.data(), slice * static_cast<size_t>(P));
  };
  // Sweeps of one step until one changes nothing (or `limit` of them have
  // run; < 0: none): what they changed in all, over every rank.
  auto sweep = [&](auto&& launch, vid_t* written, int64_t limit) {
    int64_t total = 0, done = 0;
    int batch = 2;
    while (limit < 0 || done < limit) {
      // (several ranks: a sweep's counter is only this rank's, so its successor cannot be told to skip)
      int64_t k = P > 1 ? 1 : batch;
      if (limit >= 0) k = std::min(k, limit - done);
      be_.memset_async(counters, 0, static_cast<size_t>(k) * sizeof(unsigned long long));
      for (int64_t i = 0; i < k; ++i) {
        a.changed = counters + i;
        a.prev_changed = i > 0 ? counters + i - 1 : nullptr;
        launch();
        exchange(written);
      }
      unsigned long long c[kSccBatch] = {};
      be_.to_host(c, counters, static_cast<size_t>(k) * sizeof(unsigned long long));
      int64_t changed = 0, ran = 0;
      while (ran < k && (ran == 0 || c[ran - 1] != 0)) changed += static_cast<int64_t>(c[ran++]);
      const bool fixed = c[ran - 1] == 0;
      if (P > 1) changed = comm_.sum_host(changed);
      done += ran;
      res.sweeps += ran;
      total += changed;
      if (P > 1 ? changed == 0 : fixed) break;
      // every changing sweep settles a vertex or lowers a colour along one more edge of a path
      DBFS_CHECK(done <= n + kSccBatch, "strong_components: a step's sweeps did not reach their fixed point within n");
      batch = std::min(batch * 2, kSccBatch);
    }
    return total;
  };

  comm_.barrier();
  be_.synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  be_.scc_init(a);
  int64_t live = n;
  while (live > 0) {
    DBFS_CHECK(res.rounds < n, "strong_components: more rounds than vertices");
    ++res.rounds;
    auto t = std::chrono::steady_clock::now();
    if (trim_limit != 0) {
      const int64_t settled = sweep([&] { be_.scc_trim(a); }, a.scc, trim_limit);
      res.trimmed += settled;
      live -= settled;
    }
    if (res.rounds == 1 && fault_.kind == "scc_device" && fault_.rank == comm_.rank())
      be_.inject_device_check(CheckFile::Scc);
    auto t1 = std::chrono::steady_clock::now();
    res.trim_ms += ms_between(t, t1);
    DBFS_CHECK(live >= 0, "strong_components: the trim settled more vertices than were live");
    if (live == 0) break;
    t = t1;
    a.pivot_only = false;
    // (the first round only: scc_forward's pivot form relies on equal classes and no older colours)
    if (res.rounds == 1 && use_pivot) {
      // the live vertex with the largest in-degree x out-degree, the smaller id on a tie
      unsigned long long best[2] = {0, kSccNone};
      be_.scc_pivot(a);
      if (P == 1) {
        be_.to_host(best, a.pivot_out, sizeof(best));
      } else {
        std::vector<unsigned long long> all(static_cast<size_t>(P) * 2);
        comm_.allgather(a.pivot_out, b.pivot_all.data(), sizeof(best));
        be_.to_host(all.data(), b.pivot_all.data(), all.size() * sizeof(unsigned long long));
        for (int q = 0; q < P; ++q)
          if (all[2 * q] > best[0] || (all[2 * q] == best[0] && all[2 * q + 1] < best[1]))
            best[0] = all[2 * q], best[1] = all[2 * q + 1];
      }
      DBFS_CHECK(static_cast<int64_t>(best[1]) < n, "strong_components: live vertices but no pivot");
      a.pivot = static_cast<vid_t>(best[1]);
      a.pivot_only = true;
      res.pivot = static_cast<int64_t>(best[1]);
    }
    be_.scc_colour_init(a);
    sweep([&] { be_.scc_forward(a); }, a.colour, -1);
    const int64_t joined = sweep([&] { be_.scc_backward(a); }, a.scc, -1);
    // (every class's smallest live vertex is a root and joins)
    DBFS_CHECK(joined > 0 && joined <= live, "strong_components: a round settled no component");
    live -= joined;
    if (a.pivot_only) res.pivot_size = joined;
    be_.scc_end_round(a);
    res.colour_ms += ms_between(t, std::chrono::steady_clock::now());
  }
  // the pivot round labelled its component with the pivot, every other with its smallest id
  if (res.pivot >= 0) {
    a.pivot = static_cast<vid_t>(res.pivot);
    be_.scc_relabel(a);
  }
  // sizes and totals: the labels are a compressed min-id forest (comp[l] == l)
  CcArgs c;
  c.g = a.out;
  c.comp = a.scc;
  c.size = b.size.data();
  c.totals = b.totals.data();
  c.slots = b.slots.data();
  int64_t tot[kCcTotals] = {0, 0, 0, 0};
  be_.cc_sizes(c);
  be_.to_host(tot, b.totals.data(), sizeof(tot));
  const double ms = ms_between(t0, std::chrono::steady_clock::now());
  check_device();
  res.components = n > 0 ? tot[0] : 0;
  res.singletons = n > 0 ? tot[1] : 0;
  res.largest_size = n > 0 ? tot[2] : 0;
  res.largest_label = n > 0 ? tot[3] : -1;
  res.ms = comm_.max_host(ms);
  res.trim_ms = comm_.max_host(res.trim_ms);
  res.colour_ms = comm_.max_host(res.colour_ms);
  b.last = res;
  b.valid = true;
  return res;
}

const SccResult& Engine::last_strong_components() const {
  DBFS_CHECK(scc_ && scc_->valid, "strong_components() has not run");
  return scc_->last;
}

std::vector<int64_t> Engine::gather_strong_components() {
  DBFS_CHECK(scc_ && scc_->valid, "strong_components() has not run");
  std::vector<vid_t> h(static_cast<size_t>(part_.n));
  if (!h.empty()) be_.to_host(h.data(), scc_->scc.data(), h.size() * sizeof(vid_t));
  return std::vector<int64_t>(h.begin(), h.end());
}

std::vector<int64_t> Engine::gather_strong_component_sizes() {
  DBFS_CHECK(scc_ && scc_->valid, "strong_components() has not run");
  const size_t n = static_cast<size_t>(part_.n);
  std::vector<vid_t> lab(n);
  std::vector<uint32_t> sz(n);
  if (n) {
    be_.to_host(lab.data(), scc_->scc.data(), n * sizeof(vid_t));
    be_.to_host(sz.data(), scc_->size.data(), n * sizeof(uint32_t));
  }
  std::vector<int64_t> out(n);
  for (size_t v = 0; v < n; ++v) out[v] = sz[lab[v]];
  return out;
}

}  // namespace dbfs
