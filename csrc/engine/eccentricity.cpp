// Engine::eccentricities: exact eccentricities by bounding (Takes and
// Kosters; Backend::ecc_*, backend.hpp EccArgs) -- a loop of 64-source batch
// passes, each followed by one stream over its level matrix that tightens the
// bounds of the vertices still live.
#include <algorithm>
#include <chrono>
#include <climits>

#include "dbfs/engine.hpp"

namespace dbfs {

namespace {

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

}  // namespace

EccTarget parse_ecc_target(const std::string& s) {
  if (s == "all") return EccTarget::All;
  if (s == "diameter") return EccTarget::Diameter;
  if (s == "radius") return EccTarget::Radius;
  throw Error("eccentricity target must be all, diameter or radius: '" + s + "'");
}

EccResult Engine::eccentricities(const EccOptions& o) {
  DBFS_CHECK(!opt_.directed, "eccentricities: undirected graphs only");
  DBFS_CHECK(o.component >= EccOptions::kLargest && o.component < std::max<int64_t>(part_.n, 1),
             "eccentricities: no component with label " + std::to_string(o.component));
  const int P = part_.nranks;
  const int64_t n = part_.n, W = part_.part;
  const bool scope_all = o.component == EccOptions::kAll;
  int64_t label = o.component;
  if (!scope_all && n > 0) {
    if (!has_components()) components();
    if (label == EccOptions::kLargest) label = cc_->last.largest_label;
    vid_t root = 0;
    be_.to_host(&root, cc_->comp.data() + label, sizeof(root));
    DBFS_CHECK(static_cast<int64_t>(root) == label,
               "eccentricities: no component with label " + std::to_string(label) + " (a label is its component's smallest vertex)");
  }
  if (!ecc_) {
    ecc_ = std::make_unique<EccBuffers>();
    EccBuffers& b = *ecc_;
    const size_t all = static_cast<size_t>(std::max<int64_t>(W * P, 1));
    b.lo = DBuf<int32_t>(be_, all);
    b.hi = DBuf<int32_t>(be_, all);
    b.state = DBuf<uint32_t>(be_, all);
    b.deg = DBuf<uint32_t>(be_, all);
    if (P > 1) b.deg_own = DBuf<uint32_t>(be_, static_cast<size_t>(std::max<int64_t>(W, 1)));
    b.sel_slots = DBuf<unsigned long long>(be_, static_cast<size_t>(kEccSelGrid) * kEccSelSlot);
    b.sel_out = DBuf<int64_t>(be_, kEccSelOut);
    b.totals = DBuf<int64_t>(be_, kEccTotals);
    b.slots = DBuf<int64_t>(be_, static_cast<size_t>(kEccTotalsGrid) * kEccTotals);
  }
  EccBuffers& b = *ecc_;
  b.valid = false;
  EccResult res;
  if (n == 0) {
    res.exact = true;
    b.last = res;
    b.valid = true;
    return res;
  }
  // The passes below take over the batch buffers: a batch's last pass that is
  // still only on the device is copied out first, and no pass of it stays resident.
  collect_batch_levels();
  kept_.last_k = 0;

  EccArgs a;
  a.g = g_.view();
  a.lo = b.lo.data();
  a.hi = b.hi.data();
  a.state = b.state.data();
  a.deg = b.deg.data();
  a.deg_own = P > 1 ? b.deg_own.data() : b.deg.data();
  a.comp = scope_all ? nullptr : cc_->comp.data();
  a.scope_all = scope_all;
  a.label = static_cast<vid_t>(std::max<int64_t>(label, 0));
  a.target = o.target;
  a.sel_slots = b.sel_slots.data();
  a.sel_out = b.sel_out.data();
  a.totals = b.totals.data();
  a.slots = b.slots.data();

  comm_.barrier();
  be_.synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  be_.memset_async(b.deg.data(), 0, b.deg.bytes());  // (the padding behind a rank's last row)
  if (P > 1) be_.memset_async(b.deg_own.data(), 0, b.deg_own.bytes());
  be_.ecc_degrees(a);
  if (P > 1) comm_.allgather(b.deg_own.data(), b.deg.data(), static_cast<size_t>(W) * sizeof(uint32_t));
  be_.ecc_init(a);
  be_.ecc_totals(a);

  int64_t sel[kEccSelOut];
  for (a.first = true;; a.first = false) {
    if (o.max_passes >= 0 && res.passes >= o.max_passes) break;
    auto t = std::chrono::steady_clock::now();
    be_.ecc_select(a);
    be_.to_host(sel, b.sel_out.data(), sizeof(sel));
    res.select_ms += ms_between(t, std::chrono::steady_clock::now());
    const int k = static_cast<int>(sel[0]);
    if (k == 0) {
      res.exact = true;
      break;
    }
    DBFS_CHECK(k > 0 && k <= kMsSources, "eccentricities: the selection returned " + std::to_string(k) + " sources");
    for (int i = 0; i < k; ++i)
      DBFS_CHECK(sel[1 + i] >= 0 && sel[1 + i] < n, "eccentricities: selected vertex out of range");

    // the pass, as run_batch runs one: one-byte levels until a pass is too deep
    t = std::chrono::steady_clock::now();
    BatchResult out;
    auto size_out = [&] {
      out = BatchResult{};
      out.discovered.resize(static_cast<size_t>(k));
      out.reached.assign(static_cast<size_t>(k), 0);
      out.edges.assign(static_cast<size_t>(k), 0);
      out.dist_sum.assign(static_cast<size_t>(k), 0);
      out.depth.assign(static_cast<size_t>(k), 0);
    };
    size_out();
    int lvl_bytes = ms_ && ms_->wide ? 2 : 1;
    if (run_batch_pass(sel + 1, k, static_cast<int>(res.passes), BatchDirection::Auto, lvl_bytes, out) != 0) {
      ms_->wide = true;
      lvl_bytes = 2;
      size_out();
      const int again = run_batch_pass(sel + 1, k, static_cast<int>(res.passes), BatchDirection::Auto, lvl_bytes, out);
      DBFS_CHECK(again == 0, "eccentricities: the 16-bit rerun overflowed");
    }
    if (lvl_bytes > 1) res.wide_levels = true;
    DBuf<uint8_t> gathered;
    a.m = pass_matrix(sel + 1, k, gathered);
    be_.synchronize();
    res.bfs_ms += ms_between(t, std::chrono::steady_clock::now());
    check_device();

    t = std::chrono::steady_clock::now();
    for (int i = 0; i < k; ++i) a.ecc[i] = out.depth[static_cast<size_t>(i)] - 1;
    be_.ecc_update(a);
    if (res.passes == 0 && fault_.kind == "ecc_device" && fault_.rank == comm_.rank())
      be_.inject_device_check(CheckFile::Ecc);
    be_.ecc_totals(a);
    be_.synchronize();  // (`gathered` ends with the pass)
    res.bound_ms += ms_between(t, std::chrono::steady_clock::now());
    check_device();
    ++res.passes;
    res.sources += k;
  }
  if (!res.exact) {
    // the cap ended the loop: exact all the same when nothing is left to do
    // (the drop rule is the selection's: ask it, without running a pass)
    be_.ecc_select(a);
    be_.to_host(sel, b.sel_out.data(), sizeof(sel));
    res.exact = sel[0] == 0;
  }
  int64_t tot[kEccTotals];
  be_.to_host(tot, b.totals.data(), sizeof(tot));
  a.count_hi = static_cast<int32_t>(tot[kEccMaxLo]);
  a.count_lo = static_cast<int32_t>(tot[kEccMinHi]);
  be_.ecc_totals(a);
  be_.to_host(tot, b.totals.data(), sizeof(tot));
  const double ms = ms_between(t0, std::chrono::steady_clock::now());
  check_device();
  res.scope_size = tot[kEccScopeSize];
  res.settled = tot[kEccSettledN];
  res.diameter = tot[kEccMaxLo];
  res.radius = tot[kEccMinHi];
  res.periphery = tot[kEccAtHi];
  res.centre = tot[kEccAtLo];
  res.ms = comm_.max_host(ms);
  res.bfs_ms = comm_.max_host(res.bfs_ms);
  res.bound_ms = comm_.max_host(res.bound_ms);
  res.select_ms = comm_.max_host(res.select_ms);
  b.last = res;
  b.valid = true;
  return res;
}

const EccResult& Engine::last_eccentricities() const {
  DBFS_CHECK(ecc_ && ecc_->valid, "eccentricities() has not run");
  return ecc_->last;
}

void Engine::gather_eccentricity_bounds(std::vector<int32_t>& lo, std::vector<int32_t>& hi) {
  DBFS_CHECK(ecc_ && ecc_->valid, "eccentricities() has not run");
  const size_t n = static_cast<size_t>(part_.n);
  lo.resize(n);
  hi.resize(n);
  if (n == 0) return;
  be_.to_host(lo.data(), ecc_->lo.data(), n * sizeof(int32_t));
  be_.to_host(hi.data(), ecc_->hi.data(), n * sizeof(int32_t));
}

std::vector<int32_t> Engine::gather_eccentricities() {
  std::vector<int32_t> lo, hi;
  gather_eccentricity_bounds(lo, hi);
  std::vector<uint32_t> st(lo.size());
  if (!st.empty()) be_.to_host(st.data(), ecc_->state.data(), st.size() * sizeof(uint32_t));
  for (size_t v = 0; v < lo.size(); ++v)
    if (!(st[v] & kEccSettled)) lo[v] = -1;
  return lo;
}

}  // namespace dbfs
