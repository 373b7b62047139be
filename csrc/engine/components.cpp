// Engine::components: connected components on the device (Backend::cc_*,
// backend.hpp CcArgs) -- a hook-and-compress forest over the owned rows, the
// sample-and-skip form on one undirected rank, the all-gather merge on several.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <random>

#include "dbfs/engine.hpp"

namespace dbfs {

namespace {

constexpr int kCcSamples = 1024;
// Several ranks: the label replicas are exchanged in pieces of this many
// vertices per rank at most (the receive buffer holds P pieces).
// DBFS_CC_PIECE_VERTICES overrides (tests: several pieces on a small graph).
constexpr int64_t kCcPieceBytes = int64_t(64) << 20;

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

}  // namespace

ComponentsResult Engine::components(const ComponentsOptions& o) {
  const int P = part_.nranks;
  const int64_t n = part_.n;
  const int64_t sample = o.sample_entries < 0 ? opt_.cc_sample_entries : o.sample_entries;
  ComponentsResult res;
  // The skip is sound only where every edge is stored in both rows and one
  // rank sees both: a directed entry has no twin, and on several ranks the
  // two ends could each be skipped by their own rank's largest component.
  res.sampled = P == 1 && !opt_.directed && sample > 0 && n > 0;
  if (!cc_) {
    cc_ = std::make_unique<CcBuffers>();
    CcBuffers& b = *cc_;
    b.comp = DBuf<vid_t>(be_, static_cast<size_t>(std::max<int64_t>(n, 1)));
    b.size = DBuf<uint32_t>(be_, static_cast<size_t>(std::max<int64_t>(n, 1)));
    b.long_rows = DBuf<vid_t>(be_, static_cast<size_t>(g_.nnz() / 1024 + 1));
    b.long_count = DBuf<unsigned long long>(be_, 1);
    b.totals = DBuf<int64_t>(be_, kCcTotals);
    b.slots = DBuf<int64_t>(be_, static_cast<size_t>(kCcSizeGrid) * kCcTotals);
    b.sample_idx = DBuf<vid_t>(be_, kCcSamples);
    b.sample_out = DBuf<vid_t>(be_, kCcSamples);
    std::vector<vid_t> idx(kCcSamples, 0);
    std::mt19937_64 rng(0x9E3779B97F4A7C15ull);
    for (vid_t& x : idx) x = static_cast<vid_t>(rng() % static_cast<uint64_t>(std::max<int64_t>(n, 1)));
    be_.to_device(b.sample_idx.data(), idx.data(), idx.size() * sizeof(vid_t));
  }
  CcBuffers& b = *cc_;
  b.valid = false;
  CcArgs a;
  a.g = g_.view();
  a.comp = b.comp.data();
  a.long_rows = b.long_rows.data();
  a.long_cap = static_cast<int64_t>(b.long_rows.size());
  a.long_count = b.long_count.data();
  a.size = b.size.data();
  a.totals = b.totals.data();
  a.slots = b.slots.data();
  a.sample_idx = b.sample_idx.data();
  a.sample_out = b.sample_out.data();

  double link_ms = 0.0, compress_ms = 0.0;
  auto timed = [&](double& acc, auto&& work) {
    const auto t = std::chrono::steady_clock::now();
    work();
    be_.synchronize();
    acc += ms_between(t, std::chrono::steady_clock::now());
  };
  comm_.barrier();
  be_.synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  timed(link_ms, [&] {
    be_.cc_init(a);
    a.first = 0;
    a.count = res.sampled ? sample : -1;
    be_.cc_link(a);
    if (fault_.kind == "cc_device" && fault_.rank == comm_.rank()) be_.inject_device_check(CheckFile::Cc);
  });
  timed(compress_ms, [&] { be_.cc_compress(a); });
  if (res.sampled) {
    // the most frequent label among the sampled vertices (the smaller on a tie)
    std::vector<vid_t> lab(kCcSamples);
    timed(link_ms, [&] {
      a.samples = kCcSamples;
      be_.cc_sample(a);
      be_.to_host(lab.data(), b.sample_out.data(), lab.size() * sizeof(vid_t));
    });
    std::sort(lab.begin(), lab.end());
    vid_t best = lab[0];
    int best_n = 0;
    for (size_t i = 0; i < lab.size();) {
      size_t j = i;
      while (j < lab.size() && lab[j] == lab[i]) ++j;
      if (static_cast<int>(j - i) > best_n) best_n = static_cast<int>(j - i), best = lab[i];
      i = j;
    }
    timed(link_ms, [&] {
      a.first = sample;
      a.count = -1;
      a.skip = true;
      a.skip_label = best;
      be_.cc_link(a);
    });
    timed(compress_ms, [&] { be_.cc_compress(a); });
    a.skip = false;
  }
  if (P > 1 && n > 0) {
    // Every rank's labels are its entries' connectivity written as stars (v,
    // label[v]); the union of all ranks' stars is the graph's connectivity, so
    // hooking every peer's pairs into this replica, once, is complete.
    int64_t piece = std::max<int64_t>(int64_t(1) << 16, kCcPieceBytes / static_cast<int64_t>(sizeof(vid_t)) / P);
    if (const char* e = std::getenv("DBFS_CC_PIECE_VERTICES"))
      if (*e) piece = std::max<int64_t>(64, std::atoll(e) / 64 * 64);
    piece = std::min(piece, n);
    DBuf<vid_t> recv(be_, static_cast<size_t>(piece) * static_cast<size_t>(P));
    timed(link_ms, [&] {
      for (int64_t lo = 0; lo < n; lo += piece) {
        const int64_t len = std::min(piece, n - lo);
        comm_.allgather(b.comp.data() + lo, recv.data(), static_cast<size_t>(len) * sizeof(vid_t));
        for (int q = 0; q < P; ++q) {
          if (q == comm_.rank()) continue;
          a.other = recv.data() + static_cast<int64_t>(q) * len;
          a.pair_lo = lo;
          a.pairs = len;
          be_.cc_link_pairs(a);
        }
      }
    });
    timed(compress_ms, [&] { be_.cc_compress(a); });
  }
  int64_t tot[kCcTotals] = {0, 0, 0, 0};
  be_.cc_sizes(a);
  be_.to_host(tot, b.totals.data(), sizeof(tot));
  const double ms = ms_between(t0, std::chrono::steady_clock::now());
  check_device();
  res.components = n > 0 ? tot[0] : 0;
  res.singletons = n > 0 ? tot[1] : 0;
  res.largest_size = n > 0 ? tot[2] : 0;
  res.largest_label = n > 0 ? tot[3] : -1;
  res.ms = comm_.max_host(ms);
  res.link_ms = comm_.max_host(link_ms);
  res.compress_ms = comm_.max_host(compress_ms);
  b.last = res;
  b.valid = true;
  return res;
}

const ComponentsResult& Engine::last_components() const {
  DBFS_CHECK(cc_ && cc_->valid, "components() has not run");
  return cc_->last;
}

std::vector<int64_t> Engine::gather_components() {
  DBFS_CHECK(cc_ && cc_->valid, "components() has not run");
  std::vector<vid_t> h(static_cast<size_t>(part_.n));
  if (!h.empty()) be_.to_host(h.data(), cc_->comp.data(), h.size() * sizeof(vid_t));
  return std::vector<int64_t>(h.begin(), h.end());
}

std::vector<int64_t> Engine::gather_component_sizes() {
  DBFS_CHECK(cc_ && cc_->valid, "components() has not run");
  const size_t n = static_cast<size_t>(part_.n);
  std::vector<vid_t> lab(n);
  std::vector<uint32_t> sz(n);
  if (n) {
    be_.to_host(lab.data(), cc_->comp.data(), n * sizeof(vid_t));
    be_.to_host(sz.data(), cc_->size.data(), n * sizeof(uint32_t));
  }
  std::vector<int64_t> out(n);
  for (size_t v = 0; v < n; ++v) out[v] = sz[lab[v]];
  return out;
}

}  // namespace dbfs
