// Host-side graph containers, readers and CSR construction.
//
// Reference: struct Graph (bfs.cu:21-28) keeps three int32 vectors (adjacency,
// per-vertex offset, per-vertex degree).  Here the host CSR is the standard
// (n+1)-offset form with int64 offsets and uint32 column ids.  Adjacency order
// matches the reference reader exactly: for input edge (u, v) in file order, v
// is appended to adj(u) and u to adj(v) (bfs.cu:851-863); duplicates and
// self-loops are kept (a self-loop appears twice), numEdges = 2m (bfs.cu:875).
#pragma once

#include <string>
#include <vector>

#include "dbfs/common.hpp"
#include "dbfs/wide.hpp"

namespace dbfs {

// Undirected input edge list (u[i], v[i]) over vertices [0, n).
struct EdgeList {
  int64_t n = 0;
  std::vector<vid_t> u, v;
  int64_t m() const { return static_cast<int64_t>(u.size()); }
};

// Symmetrised CSR (rows [row_lo, row_lo + rows) of an n-vertex graph).
struct HostCSR {
  int64_t n = 0;          // global vertex count
  int64_t row_lo = 0;     // first row held (0 for a full graph)
  int64_t rows = 0;       // rows held
  std::vector<eid_t> row_off;  // rows + 1
  std::vector<vid_t> col;      // row_off[rows]
  int64_t input_edges = 0;     // undirected edges of the input (m)
  int64_t directed_edges() const { return static_cast<int64_t>(col.size()); }
  eid_t degree(int64_t local_row) const { return row_off[local_row + 1] - row_off[local_row]; }
};

enum class FileFormat { Auto, EdgeList, MatrixMarket, Binary };

struct ReadOptions {
  FileFormat format = FileFormat::Auto;
  bool verbose_reference_lines = false;  // print the reference's load lines
};

// Reference-format `n m` + m lines `u v` (0-based), or MatrixMarket
// (%%MatrixMarket header, % comments, 1-based, optional value column), or the
// binary CSR cache (see write_binary_csr).  Throws dbfs::Error on failure.
// path "-" reads the reference format (or MatrixMarket) from standard input.
EdgeList read_edge_list(const std::string& path, const ReadOptions& opt = {});
FileFormat detect_format(const std::string& path);

// Build a symmetrised CSR in reference adjacency order (stable counting sort).
// directed: u -> v entries only -- the reference's stdin reader `readGraph`
// (bfs.cu:882-920, dead there: main calls readGraphFromFile) reads the pairs as
// directed edges without symmetrising.
HostCSR build_csr(const EdgeList& el, bool directed = false);
// Rows [lo, hi) of a full CSR (shard extraction; column ids stay global).
HostCSR slice_rows(const HostCSR& full, int64_t lo, int64_t hi);

// Binary CSR cache: header {magic, version, n, rows, nnz, input_edges, checksum}
// then row_off (int64) and col (uint32).  SURVEY §5.4.
// Version 2 adds per-block checksums (row offsets and columns) so that a rank
// maps and verifies only its own rows; every read checks the header ranges,
// the offsets' monotonicity and span, and that column ids are < n.
void write_binary_csr(const std::string& path, const HostCSR& g);
HostCSR read_binary_csr(const std::string& path);
struct BinaryCsrInfo {
  int version = 0;
  int64_t n = 0, row_lo = 0, rows = 0, nnz = 0, input_edges = 0;
};
BinaryCsrInfo binary_csr_info(const std::string& path);
// Global rows [lo, hi) of the cache (a shard: row_lo = lo, rebased offsets).
HostCSR read_binary_csr_rows(const std::string& path, int64_t lo, int64_t hi);
bool is_binary_csr(const std::string& path);

// Reference-format edge list of a synthetic graph (generator edges in order),
// formatted by `threads` host threads (0: all cores).  Test / benchmark inputs
// for the file readers at scale (no dataset can be downloaded on the pool).
struct GenParams;
void write_generated_edge_list(const std::string& path, const GenParams& p, int threads = 0);

// Write per-vertex levels, one per line, 2147483647 for unreached.
void write_levels(const std::string& path, const std::vector<lvl_t>& levels);

// Sequential BFS oracle (bfs.cu:923-945): exact levels; parent[v] = index into
// col of the edge that discovered v (the reference's edge-index convention),
// parent[src] = -1.
struct CpuBfsResult {
  std::vector<lvl_t> level;
  std::vector<eid_t> parent_edge;
};
CpuBfsResult cpu_bfs(const HostCSR& g, int64_t src);

// Sequential connected-components oracle: label[v] = the smallest vertex id
// in v's component, every stored entry u -> w joining u and w (a directed
// CSR: the weakly connected components).  Self-loops and duplicates change
// nothing; a vertex without entries is its own component.
std::vector<int64_t> cpu_components(const HostCSR& g);

// Sequential eccentricity oracle: one queue traversal per vertex, ecc[v] = the
// largest distance from v to a vertex of its own component over the stored
// entries (0 for a vertex without neighbours; self-loops and duplicates
// change nothing).  O(sum over components of size x entries): test sizes.
std::vector<int32_t> cpu_eccentricities(const HostCSR& g);

// Sequential strongly-connected-components oracle (Tarjan 1972, an explicit
// stack instead of the recursion): label[v] = the smallest vertex id of v's
// strongly connected component over the stored entries u -> w.  Self-loops
// and duplicates change nothing; an undirected CSR (every edge stored in both
// rows) gives cpu_components' labels.
std::vector<int64_t> cpu_strong_components(const HostCSR& g);

// Sequential betweenness oracle (Brandes 2001: a queue, the visit order as a
// stack, a predecessor scan), one source at a time.  Entries are the stored
// adjacency entries, duplicates and self-loops kept: sigma_s(s) = 1, and for a
// reached v != s sigma_s(v) = the sum of sigma_s(u) over the entries u -> v
// with level(u) = level(v) - 1 (a duplicate counts again, a self-loop never);
// delta_s(v) = the sum over the entries v -> w with level(w) = level(v) + 1 of
// sigma_s(v) / sigma_s(w) (1 + delta_s(w)).  dep[v] = the sum over the source
// slots i with v != sources[i] of delta_{sources[i]}(v): raw, not halved, not
// rescaled.  directed: g holds out-entries only (the entries into v are found
// from their tails' rows); otherwise g is symmetric and v's own row lists them.
// sigma (want_counts): [k][n] row-major, 0 where unreached.  Throws, naming
// the source, when a count exceeds DBL_MAX (as Engine::run_batch does).
// wide: the counts are kept as dbfs/wide.hpp's mantissa and exponent, added
// in the same order, and nothing throws for range; sigma[v] / sigma[w] leaves
// the wide form as a double (0 when below 2^-1074), dep is doubles as before,
// and the counts (want_counts) come as sigma_mant * 2^sigma_exp in frexp's
// convention ((0.0, 0) where unreached) instead of sigma.
struct CpuBetweennessResult {
  std::vector<double> dep;
  std::vector<double> sigma;
  std::vector<double> sigma_mant;
  std::vector<int32_t> sigma_exp;
};
CpuBetweennessResult cpu_betweenness(const HostCSR& g, const std::vector<int64_t>& sources, bool directed,
                                     bool want_counts = false, bool wide = false);

// Traversed undirected edges (Graph500 convention): sum of degrees over
// reached vertices / 2.
int64_t traversed_edges(const HostCSR& g, const std::vector<lvl_t>& level);

}  // namespace dbfs
