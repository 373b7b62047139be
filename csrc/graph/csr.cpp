// Host CSR construction and the sequential BFS oracle.
//
// build_csr reproduces the reference's adjacency order (bfs.cu:851-872:
// adj[u] += v; adj[v] += u per input edge, flattened in vertex order) with a
// stable two-pass counting sort instead of vector<vector<int>>.
// cpu_bfs is the oracle of bfs.cu:923-945 (std::queue BFS).
#include <algorithm>
#include <cfloat>
#include <string>
#include <vector>

#include "dbfs/graph.hpp"

namespace dbfs {

HostCSR build_csr(const EdgeList& el, bool directed) {
  HostCSR g;
  g.n = el.n;
  g.row_lo = 0;
  g.rows = el.n;
  g.input_edges = el.m();
  g.row_off.assign(static_cast<size_t>(el.n + 1), 0);
  const int64_t m = el.m();
  for (int64_t i = 0; i < m; ++i) {
    ++g.row_off[el.u[i] + 1];
    if (!directed) ++g.row_off[el.v[i] + 1];
  }
  for (int64_t r = 0; r < el.n; ++r) g.row_off[r + 1] += g.row_off[r];
  g.col.resize(static_cast<size_t>(g.row_off[el.n]));
  std::vector<eid_t> cur(g.row_off.begin(), g.row_off.end() - 1);
  for (int64_t i = 0; i < m; ++i) {
    const vid_t a = el.u[i], b = el.v[i];
    g.col[cur[a]++] = b;
    if (!directed) g.col[cur[b]++] = a;
  }
  return g;
}

HostCSR slice_rows(const HostCSR& full, int64_t lo, int64_t hi) {
  DBFS_CHECK(full.row_lo == 0 && full.rows == full.n, "slice_rows expects a full CSR");
  DBFS_CHECK(0 <= lo && lo <= hi && hi <= full.n, "bad row range");
  HostCSR s;
  s.n = full.n;
  s.row_lo = lo;
  s.rows = hi - lo;
  s.input_edges = full.input_edges;
  s.row_off.resize(static_cast<size_t>(s.rows + 1));
  const eid_t base = full.row_off[lo];
  for (int64_t r = 0; r <= s.rows; ++r) s.row_off[r] = full.row_off[lo + r] - base;
  s.col.assign(full.col.begin() + base, full.col.begin() + full.row_off[hi]);
  return s;
}

CpuBfsResult cpu_bfs(const HostCSR& g, int64_t src) {
  DBFS_CHECK(g.row_lo == 0 && g.rows == g.n, "cpu_bfs expects a full CSR");
  DBFS_CHECK(src >= 0 && src < g.n, "source vertex out of range");
  CpuBfsResult r;
  r.level.assign(static_cast<size_t>(g.n), kUnreached);
  r.parent_edge.assign(static_cast<size_t>(g.n), -1);
  std::vector<vid_t> q;
  q.reserve(1024);
  q.push_back(static_cast<vid_t>(src));
  r.level[src] = 0;
  size_t head = 0;
  while (head < q.size()) {
    const vid_t u = q[head++];
    const lvl_t lu = r.level[u];
    for (eid_t e = g.row_off[u]; e < g.row_off[u + 1]; ++e) {
      const vid_t v = g.col[e];
      if (r.level[v] == kUnreached) {
        r.level[v] = lu + 1;
        r.parent_edge[v] = e;
        q.push_back(v);
      }
    }
  }
  return r;
}

// Sequential union-find (union by size, path halving), then every vertex
// gets the smallest id of its set.  Shares nothing with the backends' hooks.
std::vector<int64_t> cpu_components(const HostCSR& g) {
  DBFS_CHECK(g.row_lo == 0 && g.rows == g.n, "cpu_components expects a full CSR");
  const size_t n = static_cast<size_t>(g.n);
  std::vector<int64_t> parent(n), weight(n, 1);
  for (size_t v = 0; v < n; ++v) parent[v] = static_cast<int64_t>(v);
  auto find = [&](int64_t x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  };
  for (int64_t u = 0; u < g.n; ++u)
    for (eid_t e = g.row_off[u]; e < g.row_off[u + 1]; ++e) {
      int64_t a = find(u), b = find(g.col[e]);
      if (a == b) continue;
      if (weight[a] < weight[b]) std::swap(a, b);
      parent[b] = a;
      weight[a] += weight[b];
    }
  std::vector<int64_t> smallest(n, g.n), label(n);
  for (int64_t v = g.n - 1; v >= 0; --v) smallest[find(v)] = v;  // (descending: the last write is the smallest)
  for (int64_t v = 0; v < g.n; ++v) label[v] = smallest[find(v)];
  return label;
}

// One queue traversal per vertex, sequential and plain: the deepest level it
// reaches is the vertex's eccentricity within its component.  `mark` holds the
// traversal that last saw a vertex, so no array is cleared between two of them
// and a traversal costs its component only.  Test sizes.
std::vector<int32_t> cpu_eccentricities(const HostCSR& g) {
  DBFS_CHECK(g.row_lo == 0 && g.rows == g.n, "cpu_eccentricities expects a full CSR");
  const size_t n = static_cast<size_t>(g.n);
  std::vector<int32_t> ecc(n, 0), dist(n, 0);
  std::vector<int64_t> mark(n, -1);
  std::vector<vid_t> q;
  for (int64_t s = 0; s < g.n; ++s) {
    q.clear();
    q.push_back(static_cast<vid_t>(s));
    mark[s] = s;
    dist[s] = 0;
    int32_t deepest = 0;
    for (size_t head = 0; head < q.size(); ++head) {
      const vid_t u = q[head];
      for (eid_t e = g.row_off[u]; e < g.row_off[u + 1]; ++e) {
        const vid_t v = g.col[e];
        if (mark[v] == s) continue;
        mark[v] = s;
        dist[v] = dist[u] + 1;
        deepest = dist[v];  // (levels leave the queue in order: the last one set is the deepest)
        q.push_back(v);
      }
    }
    ecc[s] = deepest;
  }
  return ecc;
}

// Tarjan's algorithm with the recursion as an explicit stack of (vertex, next
// entry) frames; a component is popped when its root's frame ends, and gets
// the smallest id among the popped.  Shares nothing with the backends' sweeps.
std::vector<int64_t> cpu_strong_components(const HostCSR& g) {
  DBFS_CHECK(g.row_lo == 0 && g.rows == g.n, "cpu_strong_components expects a full CSR");
  const size_t n = static_cast<size_t>(g.n);
  constexpr int64_t kUnseen = -1;
  std::vector<int64_t> index(n, kUnseen), low(n, 0), label(n, kUnseen);
  std::vector<char> on_stack(n, 0);
  std::vector<int64_t> stack;
  std::vector<std::pair<int64_t, eid_t>> frames;
  int64_t next_index = 0;
  for (int64_t s = 0; s < g.n; ++s) {
    if (index[s] != kUnseen) continue;
    frames.emplace_back(s, g.row_off[s]);
    index[s] = low[s] = next_index++;
    stack.push_back(s);
    on_stack[s] = 1;
    while (!frames.empty()) {
      const int64_t v = frames.back().first;
      eid_t& e = frames.back().second;
      if (e < g.row_off[v + 1]) {
        const int64_t w = g.col[e++];
        if (index[w] == kUnseen) {
          index[w] = low[w] = next_index++;
          stack.push_back(w);
          on_stack[w] = 1;
          frames.emplace_back(w, g.row_off[w]);  // (invalidates e: the loop re-reads the frame)
        } else if (on_stack[w]) {
          low[v] = std::min(low[v], index[w]);
        }
        continue;
      }
      frames.pop_back();
      if (!frames.empty()) low[frames.back().first] = std::min(low[frames.back().first], low[v]);
      if (low[v] != index[v]) continue;
      // v is its component's root: the stack from v up is the component
      size_t first = stack.size();
      int64_t smallest = v;
      do {
        --first;
        smallest = std::min(smallest, stack[first]);
      } while (stack[first] != v);
      for (size_t i = first; i < stack.size(); ++i) {
        label[stack[i]] = smallest;
        on_stack[stack[i]] = 0;
      }
      stack.resize(first);
    }
  }
  return label;
}

namespace {

// cpu_betweenness' two count forms: a count, how it is added, tested, kept,
// and the ratio sigma[v] / sigma[w] of the backward pass (a double: at most 1).
struct OracleF64 {
  using T = double;
  static T zero() { return 0.0; }
  static T one() { return 1.0; }
  static void add(T& sum, T x) { sum += x; }
  static T finish(T sum) { return sum; }
  static bool in_range(T x) { return x <= DBL_MAX; }
  static double ratio(T v, T w) { return v / w; }
  static void keep(CpuBetweennessResult& r, const std::vector<T>& sigma, size_t at) {
    std::copy(sigma.begin(), sigma.end(), r.sigma.begin() + at);
  }
  static void reserve(CpuBetweennessResult& r, size_t cnt) { r.sigma.assign(cnt, 0.0); }
};
struct OracleWide {
  using T = Wide;  // (running sums between add and finish, the stored form otherwise)
  static T zero() { return wide_zero(); }
  static T one() { return wide_one(); }
  // (a sum that holds nothing is (0, 0) here, not wide_sum_zero(): wide_add takes a zero from either side)
  static void add(T& sum, T x) { wide_add(sum, x); }
  static T finish(T sum) { return wide_normalise(sum); }
  static bool in_range(T) { return true; }
  static double ratio(T v, T w) { return wide_div_to_double(v, w); }
  static void keep(CpuBetweennessResult& r, const std::vector<T>& sigma, size_t at) {
    for (size_t v = 0; v < sigma.size(); ++v) r.sigma_mant[at + v] = sigma[v].m, r.sigma_exp[at + v] = sigma[v].e;
  }
  static void reserve(CpuBetweennessResult& r, size_t cnt) {
    r.sigma_mant.assign(cnt, 0.0);
    r.sigma_exp.assign(cnt, 0);
  }
};

template <class V>
CpuBetweennessResult cpu_betweenness_as(const HostCSR& g, const std::vector<int64_t>& sources, bool directed,
                                        bool want_counts) {
  using T = typename V::T;
  const size_t n = static_cast<size_t>(g.n);
  CpuBetweennessResult r;
  r.dep.assign(n, 0.0);
  if (want_counts) V::reserve(r, sources.size() * n);
  std::vector<lvl_t> dist(n);
  std::vector<T> sigma(n);
  std::vector<double> delta(n);
  std::vector<vid_t> order;  // the queue; read backwards it is Brandes' stack
  order.reserve(n);
  // (a count past DBL_MAX is inf, and the dependencies above it NaN: as Engine::run_batch, an error)
  auto over = [](int64_t src) {
    return "cpu_betweenness: the shortest-path counts from source " + std::to_string(src) +
           " exceed the range of a double; betweenness and path counts are not available for this graph";
  };
  for (size_t i = 0; i < sources.size(); ++i) {
    const int64_t src = sources[i];
    DBFS_CHECK(src >= 0 && src < g.n, "source vertex out of range");
    std::fill(dist.begin(), dist.end(), kUnreached);
    std::fill(sigma.begin(), sigma.end(), V::zero());
    std::fill(delta.begin(), delta.end(), 0.0);
    order.clear();
    order.push_back(static_cast<vid_t>(src));
    dist[src] = 0;
    sigma[src] = V::one();
    for (size_t head = 0; head < order.size(); ++head) {
      const vid_t u = order[head];
      const lvl_t lu = dist[u];
      if (!directed && lu > 0) {
        // u's predecessors are in its own row, all dequeued before it
        T s = V::zero();
        for (eid_t e = g.row_off[u]; e < g.row_off[u + 1]; ++e)
          if (dist[g.col[e]] == lu - 1) V::add(s, sigma[g.col[e]]);
        sigma[u] = V::finish(s);
        DBFS_CHECK(V::in_range(sigma[u]), over(src));
      }
      for (eid_t e = g.row_off[u]; e < g.row_off[u + 1]; ++e) {
        const vid_t w = g.col[e];
        if (dist[w] == kUnreached) {
          dist[w] = lu + 1;
          order.push_back(w);
        }
        // (u's count is final: every vertex one level closer was dequeued before it)
        if (directed && dist[w] == lu + 1) {
          V::add(sigma[w], sigma[u]);
          sigma[w] = V::finish(sigma[w]);
          DBFS_CHECK(V::in_range(sigma[w]), over(src));
        }
      }
    }
    for (size_t at = order.size(); at-- > 0;) {
      const vid_t v = order[at];
      double d = 0.0;
      for (eid_t e = g.row_off[v]; e < g.row_off[v + 1]; ++e) {
        const vid_t w = g.col[e];
        if (dist[w] == dist[v] + 1) d += V::ratio(sigma[v], sigma[w]) * (1.0 + delta[w]);
      }
      delta[v] = d;
      if (static_cast<int64_t>(v) != src) r.dep[v] += d;
    }
    if (want_counts) V::keep(r, sigma, i * n);
  }
  return r;
}

}  // namespace

CpuBetweennessResult cpu_betweenness(const HostCSR& g, const std::vector<int64_t>& sources, bool directed,
                                     bool want_counts, bool wide) {
  DBFS_CHECK(g.row_lo == 0 && g.rows == g.n, "cpu_betweenness expects a full CSR");
  return wide ? cpu_betweenness_as<OracleWide>(g, sources, directed, want_counts)
              : cpu_betweenness_as<OracleF64>(g, sources, directed, want_counts);
}

int64_t traversed_edges(const HostCSR& g, const std::vector<lvl_t>& level) {
  int64_t s = 0;
  for (int64_t r = 0; r < g.rows; ++r)
    if (level[g.row_lo + r] != kUnreached) s += g.degree(r);
  return s / 2;
}

}  // namespace dbfs
