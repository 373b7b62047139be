// `bfs` -- command-line driver, compatible with the reference's
// `./a.out <src> <file>` (README.md:4-14, bfs.cu:783-823) and its stdout lines
// (SURVEY Appendix A), plus the flags of SURVEY §5.6.
//
//   bfs <src> <edge-list|.mtx|.csr> [flags]
//   bfs --rmat SCALE[:EF] [src] [flags]
//
// Execution models:
//   default            1 GPU (HIP backend, device --device)
//   --gpus P           P GPUs in one process, one host thread per GPU: the
//                      peer-memory communicator (every rank's window shared
//                      as a device pointer, peer access enabled) over an
//                      in-process host communicator; one RCCL communicator
//                      per GPU (ncclCommInitAll) if the windows fail --
//                      replaces the reference's intra-node bfs.cu
//   --virtual-ranks P  P partitions on ONE device (threads + VirtualComm):
//                      exercises the distributed code path on one GPU
//   --cpu              CPU backend (no GPU needed)
//   WORLD_SIZE > 1     one process per GPU (torchrun / any launcher): TCP
//                      bootstrap on MASTER_ADDR:MASTER_PORT+1, the peer-memory
//                      communicator (IPC windows) over a TCP inner
//                      communicator -- replaces the reference's MPI build
//                      bfs_mpi.cu
// DBFS_COMM = peer | rccl | tcp selects the transport (default: peer with an
// agreed fallback to RCCL, then TCP), DBFS_DEVICE pins every process to one
// device (several ranks sharing a GPU: tests).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "dbfs/engine.hpp"

using namespace dbfs;

namespace {

struct Args {
  int64_t src = 0;
  bool src_given = false;
  std::string path;
  int gpus = 1;
  int virtual_ranks = 0;
  int device = 0;
  bool cpu = false;
  std::string mode = "do";
  double alpha = 40.0, beta = 384.0;
  int bu_lane_limit = 16;
  int rmat_scale = 0, rmat_ef = 16;
  int64_t uni_n = 0, uni_m = 0;
  uint64_t seed = 1;
  int roots = 0;
  bool batch = false;                 // --roots K: the K roots as one concurrent traversal (Engine::run_batch)
  std::string batch_dir = "auto";
  bool betweenness = false;           // --batch --betweenness: path counts and dependencies after every pass
  std::string betweenness_out;        // ... the raw dependency sums, one %.17g per vertex
  std::string betweenness_counts;     // ... the path counts' form: double | wide | auto (empty: not given, double)
  bool oracle = true;
  bool validate = false;
  std::string levels_out;
  std::string cache_out;
  bool json = false;
  std::string level_csv;
  bool quiet = false;
  bool phase_timing = false;
  bool hub_sort = true;
  bool directed = false;
  bool components = false;            // --components: connected components before the traversals (Engine::components)
  std::string components_out;         // ... the labels, one per line
  int64_t cc_sample_entries = -1;     // --cc-sample-entries N (EngineOptions::cc_sample_entries; -1: the default)
  bool strong_components = false;     // --strong-components: strongly connected components before the traversals
  std::string strong_components_out;  // ... the labels, one per line
  int64_t scc_trim_rounds = -2;       // --scc-trim-rounds N (EngineOptions::scc_trim_rounds; -2: the default)
  bool scc_pivot = true;              // --no-scc-pivot clears it (EngineOptions::scc_pivot)
  bool eccentricities = false;        // --eccentricities: eccentricity bounding before the traversals (Engine::eccentricities)
  std::string ecc_target = "all";     // --ecc-target all|diameter|radius
  std::string ecc_component = "largest";  // --ecc-component largest|all|LABEL
  int64_t ecc_max_passes = -1;        // --ecc-max-passes N (-1: no cap)
  std::string eccentricities_out;     // ... the eccentricities, one per line (-1: out of scope or unsettled)
  bool mode_given = false;            // --mode on the command line (--directed turns only the default into td)
  std::vector<std::pair<std::string, double>> opts;  // --opt name=value, in order (set_engine_option)
};

[[noreturn]] void usage(const char* msg = nullptr) {
  if (msg) std::fprintf(stderr, "error: %s\n\n", msg);
  std::fprintf(stderr,
               "usage: bfs <src> <edge-list|.mtx|.csr|-> [flags]   (- = standard input)\n"
               "       bfs --rmat SCALE[:EF] [<src>] [flags]\n"
               "flags: --gpus P | --virtual-ranks P | --cpu | --device D\n"
               "       --mode ref|td|bu|do|simple|scan  --alpha A --beta B --bu-lane-limit K\n"
               "       --rmat SCALE[:EF] | --uniform N:M   --seed S\n"
               "       --roots K (random sources, GTEPS summary)  --no-oracle  --validate\n"
               "       --batch (the K roots concurrently, 64 per pass)  --batch-direction auto|push|pull|alternate\n"
               "       --batch --validate (every pass's levels checked on the device, all its sources at once)\n"
               "       --batch --betweenness [--betweenness-out FILE] (betweenness centrality of the K roots on the device:\n"
               "                   the raw dependency sums, checked against the sequential oracle unless --no-oracle)\n"
               "       --betweenness-counts double|wide|auto (path counts as doubles: more than 2^1024 paths is an error;\n"
               "                   as a mantissa and an exponent; or wide only for the passes that overflow a double)\n"
               "       --components [--components-out FILE] (connected components on the device before the traversals: count,\n"
               "                   largest, singletons; the labels checked against the sequential oracle unless --no-oracle)\n"
               "       --cc-sample-entries N (entries per row hooked before the largest component is skipped; 0: one full pass)\n"
               "       --strong-components [--strong-components-out FILE] (strongly connected components on the device\n"
               "                   before the traversals, after --components: count, largest, singletons, trimmed, rounds;\n"
               "                   the labels checked against the sequential Tarjan oracle unless --no-oracle; an undirected\n"
               "                   graph: its connected components)\n"
               "       --scc-trim-rounds N (trim sweeps per round at most; -1: to the fixed point, the default; 0: no trim)\n"
               "       --no-scc-pivot (colour every vertex in the first round instead of one high-degree pivot)\n"
               "       --eccentricities [--eccentricities-out FILE] (exact eccentricities by bounding over 64-source batch\n"
               "                   passes, before the traversals, after --components: diameter, radius, centre, periphery;\n"
               "                   undirected graphs only; checked against one sequential traversal per vertex, or per\n"
               "                   sampled vertex on a large scope, unless --no-oracle)\n"
               "       --ecc-target all|diameter|radius (stop once every vertex is settled, or once that value is known)\n"
               "       --ecc-component largest|all|LABEL (the vertices answered for: the largest component, every vertex,\n"
               "                   or the component with that label)\n"
               "       --ecc-max-passes N (at most N passes: bounds as they stand, exact 0)\n"
               "       --levels-out FILE  --cache FILE (write binary CSR)  --json  --quiet  --phase-timing\n"
               "       --directed (edge list as directed u->v pairs, like the reference's stdin reader;\n"
               "                   top-down modes only; --batch and --validate work on the in-edge shard,\n"
               "                   built on the device on first use)\n"
               "       --level-csv FILE (per-level records of every run: root,level,dir,frontier,...,ms)\n"
               "       --opt NAME=VALUE (repeatable: an engine option by name, a number, applied after the flags above,\n"
               "                   e.g. td_bin_edges=1, device_loop=0; an unknown name or a value that is no number is an\n"
               "                   error)\n"
               "       --json lines of a run carry \"chains\": every level chain the device loop enqueued, in order, as\n"
               "                   {l, form (T dense, S sparse, X binned top-down; B bottom-up), unvis, split, cut};\n"
               "                   [] with the host loop\n");
  std::exit(2);
}

Args parse(int argc, char** argv) {
  Args a;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) usage(("missing value for " + s).c_str());
      return argv[++i];
    };
    if (s == "--gpus") a.gpus = std::stoi(next());
    else if (s == "--virtual-ranks") a.virtual_ranks = std::stoi(next());
    else if (s == "--device") a.device = std::stoi(next());
    else if (s == "--cpu") a.cpu = true;
    else if (s == "--mode") {
      a.mode = next();
      a.mode_given = true;
    }
    else if (s == "--alpha") a.alpha = std::stod(next());
    else if (s == "--beta") a.beta = std::stod(next());
    else if (s == "--bu-lane-limit") a.bu_lane_limit = std::stoi(next());
    else if (s == "--rmat") {
      std::string v = next();
      auto c = v.find(':');
      a.rmat_scale = std::stoi(v.substr(0, c));
      if (c != std::string::npos) a.rmat_ef = std::stoi(v.substr(c + 1));
    } else if (s == "--uniform") {
      std::string v = next();
      auto c = v.find(':');
      if (c == std::string::npos) usage("--uniform expects N:M");
      a.uni_n = std::stoll(v.substr(0, c));
      a.uni_m = std::stoll(v.substr(c + 1));
    } else if (s == "--seed") a.seed = std::stoull(next());
    else if (s == "--roots") a.roots = std::stoi(next());
    else if (s == "--batch") a.batch = true;
    else if (s == "--batch-direction") a.batch_dir = next();
    else if (s == "--betweenness") a.betweenness = true;
    else if (s == "--betweenness-out") a.betweenness_out = next();
    else if (s == "--betweenness-counts") a.betweenness_counts = next();
    else if (s == "--components") a.components = true;
    else if (s == "--components-out") a.components_out = next();
    else if (s == "--cc-sample-entries") a.cc_sample_entries = std::stoll(next());
    else if (s == "--strong-components") a.strong_components = true;
    else if (s == "--strong-components-out") a.strong_components_out = next();
    else if (s == "--scc-trim-rounds") a.scc_trim_rounds = std::stoll(next());
    else if (s == "--no-scc-pivot") a.scc_pivot = false;
    else if (s == "--eccentricities") a.eccentricities = true;
    else if (s == "--ecc-target") a.ecc_target = next();
    else if (s == "--ecc-component") a.ecc_component = next();
    else if (s == "--ecc-max-passes") a.ecc_max_passes = std::stoll(next());
    else if (s == "--eccentricities-out") a.eccentricities_out = next();
    else if (s == "--no-oracle") a.oracle = false;
    else if (s == "--validate") a.validate = true;
    else if (s == "--levels-out") a.levels_out = next();
    else if (s == "--cache") a.cache_out = next();
    else if (s == "--json") a.json = true;
    else if (s == "--level-csv") a.level_csv = next();
    else if (s == "--quiet") a.quiet = true;
    else if (s == "--phase-timing") a.phase_timing = true;
    else if (s == "--no-hub-sort") a.hub_sort = false;
    else if (s == "--directed") a.directed = true;
    else if (s == "--opt") {
      const std::string kv = next();
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || eq == 0 || eq + 1 == kv.size()) usage(("--opt expects NAME=VALUE, got " + kv).c_str());
      const std::string name = kv.substr(0, eq), val = kv.substr(eq + 1);
      char* end = nullptr;
      const double v = std::strtod(val.c_str(), &end);
      if (!end || *end || !std::isfinite(v)) usage(("--opt " + name + ": value is not a number: " + val).c_str());
      try {
        EngineOptions probe;
        set_engine_option(probe, name, v);
      } catch (const std::exception& e) {
        usage(("--opt: " + std::string(e.what())).c_str());
      }
      a.opts.emplace_back(name, v);
    }
    else if (s == "-h" || s == "--help") usage();
    else if (!s.empty() && s[0] == '-' && s.size() > 1 && !std::isdigit(static_cast<unsigned char>(s[1])))
      usage(("unknown flag " + s).c_str());
    else pos.push_back(s);
  }
  const bool synth = a.rmat_scale > 0 || a.uni_n > 0;
  if (!synth) {
    if (pos.size() != 2) usage("expected <src> <edge-list> (reference argument order)");
    a.path = pos[1];
  } else if (pos.size() > 1) {
    usage("synthetic graphs take at most one positional argument (<src>)");
  }
  if (!pos.empty()) {
    char* end = nullptr;
    a.src = std::strtoll(pos[0].c_str(), &end, 10);
    if (!end || *end) usage("source vertex must be an integer");
    a.src_given = true;
  }
  if (a.gpus < 1) usage("--gpus must be >= 1");
  if ((a.betweenness || !a.betweenness_out.empty()) && !(a.batch && a.roots > 0))
    usage("--betweenness needs --roots K --batch");
  if (!a.betweenness_out.empty() && !a.betweenness) usage("--betweenness-out needs --betweenness");
  if (!a.betweenness_counts.empty()) {
    if (!a.betweenness) usage("--betweenness-counts needs --betweenness");
    if (a.betweenness_counts != "double" && a.betweenness_counts != "wide" && a.betweenness_counts != "auto")
      usage("--betweenness-counts must be double, wide or auto");
  }
  if (!a.components_out.empty() && !a.components) usage("--components-out needs --components");
  if (a.cc_sample_entries < -1) usage("--cc-sample-entries must be >= 0");
  if (!a.strong_components_out.empty() && !a.strong_components)
    usage("--strong-components-out needs --strong-components");
  if (a.scc_trim_rounds < -2) usage("--scc-trim-rounds must be >= -1");
  if (!a.eccentricities_out.empty() && !a.eccentricities) usage("--eccentricities-out needs --eccentricities");
  if (a.eccentricities) {
    if (a.directed) usage("--eccentricities needs an undirected graph");
    if (a.ecc_target != "all" && a.ecc_target != "diameter" && a.ecc_target != "radius")
      usage("--ecc-target must be all, diameter or radius");
    if (a.ecc_component != "largest" && a.ecc_component != "all") {
      char* end = nullptr;
      const long long label = std::strtoll(a.ecc_component.c_str(), &end, 10);
      if (!end || *end || a.ecc_component.empty() || label < 0) usage("--ecc-component must be largest, all or a label");
    }
    if (a.ecc_max_passes < -1) usage("--ecc-max-passes must be >= 0");
  }
  if (a.directed) {
    // a single-source traversal is top-down only (the bottom-up kernels take
    // their degrees from their own rows); --batch pulls over the in-edge shard
    // and --validate checks the directed level rules on it
    if (synth) usage("--directed applies to edge-list input only");
    if (a.mode == "bu" || (a.mode == "do" && a.mode_given))
      usage("--directed needs a top-down mode (td, ref, simple, scan)");
    if (a.mode == "do") a.mode = "td";
  }
  return a;
}

int env_int(const char* k, int dflt) {
  const char* v = std::getenv(k);
  return v && *v ? std::atoi(v) : dflt;
}

// One rank's state.
struct RankCtx {
  std::unique_ptr<Backend> be;
  std::shared_ptr<Comm> comm;
  std::unique_ptr<DeviceGraph> graph;
  std::unique_ptr<Engine> engine;
};

// The peer-memory communicator over `inner` when every rank maps every window
// and its self-test passes (both agreed over the bootstrap / inner), else
// `inner` -- or an error when the peer transport was asked for.
std::shared_ptr<Comm> try_peer(std::shared_ptr<Bootstrap> boot, Backend& be, std::shared_ptr<Comm> inner,
                               bool required, bool report) {
  std::string why;
  try {
    // (DBFS_PEER_SLOT_KB, when set, overrides: small slots exercise the
    // slot-sized rounds of large collectives in tests)
    const size_t slot = std::getenv("DBFS_PEER_SLOT_KB") ? static_cast<size_t>(env_int("DBFS_PEER_SLOT_KB", 0)) << 10
                                                         : static_cast<size_t>(env_int("DBFS_PEER_SLOT_MB", 16)) << 20;
    auto pc = std::make_shared<PeerComm>(boot, be, inner, slot);
    if (pc->self_test(&why)) return pc;
  } catch (const std::exception& e) {
    why = e.what();
  }
  if (required) throw Error("DBFS_COMM=peer: peer communicator unavailable: " + why);
  if (report) std::fprintf(stderr, "[bfs] peer communicator unavailable (%s); using %s\n", why.c_str(), inner->name().c_str());
  return inner;
}

// One thread per local rank.  A rank that throws aborts the virtual group so
// its peers fail at their next collective instead of waiting forever.
void run_ranks(std::vector<RankCtx>& ranks, const std::function<void(int, RankCtx&)>& fn,
               VirtualGroup* group = nullptr) {
  if (ranks.size() == 1) {
    fn(0, ranks[0]);
    return;
  }
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> errs(ranks.size());
  for (size_t r = 0; r < ranks.size(); ++r)
    th.emplace_back([&, r] {
      try {
        fn(static_cast<int>(r), ranks[r]);
      } catch (const std::exception& e) {
        errs[r] = std::current_exception();
        if (group) group->abort("rank " + std::to_string(r) + ": " + e.what());
      } catch (...) {
        errs[r] = std::current_exception();
        if (group) group->abort("rank " + std::to_string(r) + " failed");
      }
    });
  for (auto& t : th) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
}

std::string json_run(const RunResult& r, const std::string& graph, int64_t n, int64_t m, int P, const char* mode,
                     const std::string& backend, const std::string& comm, const std::string& ingest = "") {
  std::string s = "{\"graph\":\"" + graph + "\",\"n\":" + std::to_string(n) + ",\"m\":" + std::to_string(m) +
                  ",\"ranks\":" + std::to_string(P) + ",\"mode\":\"" + mode + "\",\"backend\":\"" + backend +
                  "\",\"comm\":\"" + comm + "\",\"source\":" + std::to_string(r.source) + ",\"ms\":" + std::to_string(r.ms) +
                  ",\"reached\":" + std::to_string(r.reached) + ",\"edges\":" + std::to_string(r.edges) +
                  ",\"gteps\":" + std::to_string(r.gteps) + ",\"depth\":" + std::to_string(r.depth) +
                  (ingest.empty() ? std::string() : ",\"ingest\":" + ingest) + ",\"levels\":[";
  for (size_t i = 0; i < r.levels.size(); ++i) {
    const auto& l = r.levels[i];
    if (i) s += ",";
    s += "{\"l\":" + std::to_string(l.level) + ",\"dir\":\"" + std::string(1, l.direction) +
         "\",\"frontier\":" + std::to_string(l.frontier) + ",\"edges\":" + std::to_string(l.frontier_edges) +
         ",\"new\":" + std::to_string(l.discovered) + ",\"ms\":" + std::to_string(l.ms) + "}";
  }
  // every chain the device loop enqueued, in order (ChainRecord; none with the host loop)
  s += "],\"chains\":[";
  for (size_t i = 0; i < r.chains.size(); ++i) {
    const auto& c = r.chains[i];
    if (i) s += ",";
    s += "{\"l\":" + std::to_string(c.level) + ",\"form\":\"" + std::string(1, c.form) +
         "\",\"unvis\":" + (c.unvis ? "true" : "false") + ",\"split\":" + std::to_string(c.split) +
         ",\"cut\":" + (c.cut ? "true" : "false") + "}";
  }
  return s + "]}";
}

// Backends and communicators of this process's ranks (one for a process of
// a multi-process job): RCCL + peer windows, TCP, virtual ranks or local.
// Returns the virtual group when the ranks are virtual.
std::shared_ptr<VirtualGroup> make_ranks(const Args& a, int P, bool multiproc, int wrank, int world, bool leader,
                                         std::vector<RankCtx>& ranks) {
  const int nlocal = static_cast<int>(ranks.size());
  std::shared_ptr<VirtualGroup> vgroup;
  if (a.virtual_ranks > 0 && !multiproc) vgroup = std::make_shared<VirtualGroup>(P);
  const char* dev_pin = std::getenv("DBFS_DEVICE");  // several processes on one GPU (tests)
  const char* cm_env = std::getenv("DBFS_COMM");
  const std::string cm = cm_env ? cm_env : "";
  const bool want_peer = !a.cpu && (cm.empty() || cm == "peer");
  for (int i = 0; i < nlocal; ++i) {
    if (a.cpu) ranks[i].be = make_cpu_backend();
    else if (multiproc) ranks[i].be = make_hip_backend(dev_pin ? std::atoi(dev_pin) : env_int("LOCAL_RANK", 0));
    else if (a.virtual_ranks > 0) ranks[i].be = make_hip_backend(a.device);
    else ranks[i].be = make_hip_backend(P > 1 ? (dev_pin ? std::atoi(dev_pin) : i) : a.device);
  }
  // one process, P ranks pinned to one device (DBFS_DEVICE: the --gpus P
  // path rehearsed on one GPU): every free deferred to the end, so no rank's
  // hipFree waits for a peer's kernel spinning on that rank's next collective
  if (!multiproc && !a.cpu && a.virtual_ranks == 0 && P > 1 && dev_pin)
    for (auto& r : ranks) r.be->set_deferred_frees(true);
  if (multiproc) {
    const char* addr = std::getenv("MASTER_ADDR");
    const int port = env_int("DBFS_BOOTSTRAP_PORT", env_int("MASTER_PORT", 29500) + 1);
    auto boot = std::make_shared<TcpBootstrap>(addr ? addr : "127.0.0.1", port, wrank, world);
    auto make_rccl = [&]() -> std::shared_ptr<Comm> {
      // every rank takes part in the id broadcast before anything can fail
      // (an empty id: rank 0 could not make one), so the bootstrap's message
      // sequence stays aligned for the agreement after a failure
      std::string uid, why;
      if (wrank == 0) {
        try {
          uid = NcclComm::unique_id();
        } catch (const std::exception& e) {
          why = e.what();
        }
      }
      uid = boot->broadcast(uid);
      if (uid.empty()) throw Error(why.empty() ? "rank 0 could not create the RCCL id" : why);
      return std::make_shared<NcclComm>(uid, wrank, world, *ranks[0].be);
    };
    if (a.cpu || cm == "tcp") {
      // host transport (CPU ranks; debug)
      ranks[0].comm = std::make_shared<TcpComm>(boot, *ranks[0].be);
    } else if (cm == "rccl") {
      ranks[0].comm = make_rccl();
    } else {
      // the peer windows over a TCP inner communicator (setup agreements
      // only: every payload goes through the windows); RCCL (bounded setup,
      // agreed) only when the windows are unavailable on separate GPUs
      auto tcp = std::make_shared<TcpComm>(boot, *ranks[0].be);
      ranks[0].comm = try_peer(boot, *ranks[0].be, tcp, cm == "peer", leader);
      if (ranks[0].comm == tcp && !dev_pin) {
        std::shared_ptr<Comm> rc;
        std::string err;
        try {
          rc = make_rccl();
        } catch (const std::exception& e) {
          err = e.what();
        }
        std::string first;
        for (const auto& e : boot->allgather(err))
          if (first.empty()) first = e;
        if (first.empty()) ranks[0].comm = rc;
        else if (leader) std::fprintf(stderr, "[bfs] RCCL unavailable (%s); using tcp\n", first.c_str());
      }
    }
  } else if (vgroup) {
    for (int i = 0; i < P; ++i) ranks[i].comm = std::make_shared<VirtualComm>(vgroup, i, *ranks[i].be);
  } else if (P > 1) {
    // one process, P GPUs: the peer windows (device pointers, peer access)
    // over an in-process host communicator; ncclCommInitAll only when the
    // windows are unavailable (or DBFS_COMM=rccl)
    bool peer_ok = false;
    if (want_peer) {
      auto igroup = std::make_shared<VirtualGroup>(P);
      auto pgroup = std::make_shared<VirtualGroup>(P);
      std::vector<std::shared_ptr<Comm>> inner(static_cast<size_t>(P));
      for (int i = 0; i < P; ++i) inner[i] = std::make_shared<VirtualComm>(igroup, i, *ranks[i].be);
      run_ranks(ranks, [&](int i, RankCtx& rc) {
        rc.comm = try_peer(std::make_shared<GroupBootstrap>(pgroup, i), *rc.be, inner[i], cm == "peer", i == 0);
      }, pgroup.get());
      peer_ok = ranks[0].comm != inner[0];
    }
    if (!peer_ok) {
      std::vector<Backend*> bes;
      for (auto& r : ranks) bes.push_back(r.be.get());
      auto comms = NcclComm::init_all(bes);
      for (int i = 0; i < P; ++i) ranks[i].comm = std::move(comms[i]);
    }
  } else {
    ranks[0].comm = std::make_shared<LocalComm>(*ranks[0].be);
  }
  return vgroup;
}

// K random roots of degree >= 1 (the same sequence on every rank; a
// multi-process job asks each vertex's owner for its degree).
std::vector<int64_t> sample_roots(const Args& a, const Partition& part, std::vector<RankCtx>& ranks, bool multiproc,
                                  int wrank) {
  std::mt19937_64 rng(a.seed * 7919 + 17);
  std::vector<int64_t> roots;
  int tries = 0;
  while (static_cast<int>(roots.size()) < a.roots && tries < 100 * a.roots) {
    ++tries;
    const int64_t v = static_cast<int64_t>(rng() % static_cast<uint64_t>(part.n));
    const int own = part.owner(v);
    int64_t deg = 0;
    if (!multiproc) {
      deg = ranks[own].graph->degrees_of({v - part.lo(own)})[0];
    } else {
      const int64_t d = own == wrank ? ranks[0].graph->degrees_of({v - part.lo(own)})[0] : 0;
      deg = ranks[0].comm->sum_host(d);
    }
    if (deg > 0) roots.push_back(v);
  }
  return roots;
}

}  // namespace

int main(int argc, char** argv) {
  Args a = parse(argc, argv);
  const int world = env_int("WORLD_SIZE", 1);
  const int wrank = env_int("RANK", 0);
  const bool multiproc = world > 1;
  const bool leader = !multiproc || wrank == 0;
  const bool ref_lines = !a.quiet && leader;
  try {
    // ranks of this job (P) and of this process (nlocal)
    int P = 1;
    if (multiproc) P = world;
    else if (a.virtual_ranks > 0) P = a.virtual_ranks;
    else if (!a.cpu) P = a.gpus;
    const int nlocal = multiproc ? 1 : P;
    // Several ranks reading an edge-list / .mtx file / binary cache: every rank
    // parses only its byte range (or its rows) and builds its shard on its
    // device (DeviceGraph::from_file).  The reference reads and builds the
    // whole graph on every rank (bfs_mpi.cu:815); here only the leader reads
    // the whole file, and only for the CPU oracle (--no-oracle: not at all;
    // the device validator then checks the levels).
    const bool sharded = !a.path.empty() && a.path != "-" && !a.directed && P > 1;
    if (sharded && !a.oracle) a.validate = true;

    // ---- graph ingestion ----
    HostCSR full;
    bool have_host = false;
    std::string gname;
    GenParams gp;
    bool synth = false;
    if (!a.path.empty()) {
      gname = a.path;
      if (ref_lines) std::printf("%s\n", a.path.c_str());
      if (!sharded) {
        if (a.path != "-" && is_binary_csr(a.path)) {
          full = read_binary_csr(a.path);
        } else {
          ReadOptions ro;
          ro.verbose_reference_lines = ref_lines;
          EdgeList el = read_edge_list(a.path, ro);
          full = build_csr(el, a.directed);
        }
        have_host = true;
        if (ref_lines) std::printf("finish load graph\n");
      }
    } else {
      synth = true;
      if (a.rmat_scale > 0) {
        gp = rmat_params(a.rmat_scale, a.rmat_ef, a.seed);
        gname = "rmat" + std::to_string(a.rmat_scale) + "_ef" + std::to_string(a.rmat_ef);
      } else {
        gp = uniform_params(a.uni_n, a.uni_m, a.seed);
        gname = "uniform_n" + std::to_string(a.uni_n) + "_m" + std::to_string(a.uni_m);
      }
      // Host copy only when the CPU oracle / cache / CPU backend needs it.
      if ((a.oracle && leader) || !a.cache_out.empty()) {
        EdgeList el;
        el.n = gp.n;
        el.u.resize(static_cast<size_t>(gp.m));
        el.v.resize(static_cast<size_t>(gp.m));
        for (int64_t i = 0; i < gp.m; ++i) {
          uint64_t u, v;
          gen_edge(gp, static_cast<uint64_t>(i), u, v);
          el.u[i] = static_cast<vid_t>(u);
          el.v[i] = static_cast<vid_t>(v);
        }
        full = build_csr(el);
        have_host = true;
      }
    }
    // the reference's lines after the load, and the CPU oracle
    // (bfs.cu:789-802) on the leader
    std::vector<lvl_t> expected;
    auto print_graph_and_oracle = [&](int64_t n, int64_t directed_edges) {
      if (ref_lines) {
        std::printf("Number of vertices %lld\n", static_cast<long long>(n));
        std::printf("Number of edges %lld\n\n", static_cast<long long>(directed_edges));
      }
      if (!a.cache_out.empty() && leader && have_host) write_binary_csr(a.cache_out, full);
      if (a.src < 0 || a.src >= n)
        throw Error("source vertex " + std::to_string(a.src) + " out of range [0, " + std::to_string(n) + ")");
      if (a.oracle && leader) {
        if (sharded && !have_host) {
          // the whole graph on the leader only, for the oracle (not timed)
          if (is_binary_csr(a.path)) {
            full = read_binary_csr(a.path);
          } else {
            EdgeList el = read_edge_list(a.path, ReadOptions{});
            full = build_csr(el, false);
          }
          have_host = true;
        }
        if (ref_lines) std::printf("Starting sequential bfs.\n");
        auto c0 = std::chrono::steady_clock::now();
        expected = cpu_bfs(full, a.src).level;
        auto c1 = std::chrono::steady_clock::now();
        if (ref_lines)
          std::printf("Elapsed time in milliseconds : %li ms.\n\n",
                      static_cast<long>(std::chrono::duration_cast<std::chrono::milliseconds>(c1 - c0).count()));
      }
    };
    if (!sharded)
      print_graph_and_oracle(have_host ? full.n : gp.n, have_host ? full.directed_edges() : 2 * gp.m);

    // ---- ranks / devices ----
    std::vector<RankCtx> ranks(static_cast<size_t>(nlocal));
    if (!a.cpu && ref_lines && !sharded) std::printf("Enabling peer access between GPU0 and GPU1...\n");
    std::shared_ptr<VirtualGroup> vgroup = make_ranks(a, P, multiproc, wrank, world, leader, ranks);

    Partition part;
    if (sharded) {
      // every rank its byte range (host threads shared among this process's ranks)
      const int threads = std::max(1, static_cast<int>(std::thread::hardware_concurrency()) / nlocal);
      run_ranks(ranks, [&](int i, RankCtx& rc) {
        rc.graph = DeviceGraph::from_file(*rc.be, *rc.comm, a.path, std::min(threads, 16));
      }, vgroup.get());
      const DeviceGraph& g0 = *ranks[0].graph;
      part = g0.partition();
      if (ref_lines) {
        std::printf("nodes num: %lld\n", static_cast<long long>(g0.n()));
        std::printf("edge num: %lld\n", static_cast<long long>(g0.input_edges()));
        std::printf("finish load graph\n");
      }
      int64_t nnz = 0;
      if (multiproc) nnz = ranks[0].comm->sum_host(g0.nnz());
      else
        for (auto& r : ranks) nnz += r.graph->nnz();
      print_graph_and_oracle(g0.n(), nnz);
      if (!a.cpu && ref_lines) std::printf("Enabling peer access between GPU0 and GPU1...\n");
    } else {
      part = Partition::block(have_host ? full.n : gp.n, P);
    }
    const int64_t n = part.n;
    const int64_t m_in = sharded ? ranks[0].graph->input_edges() : have_host ? full.input_edges : gp.m;

    EngineOptions eo;
    eo.mode = parse_mode(a.mode);
    eo.alpha = a.alpha;
    eo.beta = a.beta;
    eo.bu_lane_limit = a.bu_lane_limit;
    eo.phase_timing = a.phase_timing;
    eo.directed = a.directed;
    if (a.cc_sample_entries >= 0) eo.cc_sample_entries = a.cc_sample_entries;
    if (a.scc_trim_rounds >= -1) eo.scc_trim_rounds = a.scc_trim_rounds;
    if (!a.scc_pivot) eo.scc_pivot = false;
    for (const auto& kv : a.opts) set_engine_option(eo, kv.first, kv.second);
    run_ranks(ranks, [&](int i, RankCtx& rc) {
      const int rk = multiproc ? wrank : i;
      if (synth) rc.graph = DeviceGraph::generate(*rc.be, gp, part, rk);
      else if (!sharded) rc.graph = DeviceGraph::from_host(*rc.be, full, part, rk);
      if (a.hub_sort) rc.graph->sort_neighbors_by_degree(*rc.comm);
      rc.engine = std::make_unique<Engine>(*rc.graph, *rc.comm, eo);
    }, vgroup.get());
    // what every rank parsed (sharded reads): [byte_begin, byte_end, edges] per rank
    std::string ingest_json;
    if (sharded) {
      std::vector<int64_t> b, e, m;
      if (multiproc) {
        const auto& gi = ranks[0].graph->ingest();
        b = ranks[0].comm->allgather_host_i64(gi.byte_begin);
        e = ranks[0].comm->allgather_host_i64(gi.byte_end);
        m = ranks[0].comm->allgather_host_i64(gi.edges);
      } else {
        for (auto& r : ranks) {
          b.push_back(r.graph->ingest().byte_begin);
          e.push_back(r.graph->ingest().byte_end);
          m.push_back(r.graph->ingest().edges);
        }
      }
      ingest_json = "[";
      for (size_t r = 0; r < b.size(); ++r)
        ingest_json += (r ? ",[" : "[") + std::to_string(b[r]) + "," + std::to_string(e[r]) + "," +
                       std::to_string(m[r]) + "]";
      ingest_json += "]";
    }

    // ---- connected components (--components), before the traversals ----
    if (a.components) {
      std::vector<ComponentsResult> cres(static_cast<size_t>(nlocal));
      std::vector<int64_t> labels;
      run_ranks(ranks, [&](int i, RankCtx& rc) {
        cres[i] = rc.engine->components();
        if (i == 0 && leader && ((a.oracle && have_host) || !a.components_out.empty()))
          labels = rc.engine->gather_components();
      }, vgroup.get());
      if (leader) {
        const ComponentsResult& c = cres[0];
        std::printf("components %lld largest label %lld size %lld singletons %lld ms %.3f\n",
                    static_cast<long long>(c.components), static_cast<long long>(c.largest_label),
                    static_cast<long long>(c.largest_size), static_cast<long long>(c.singletons), c.ms);
        if (a.oracle && have_host) {
          const std::vector<int64_t> exp = cpu_components(full);
          for (int64_t i = 0; i < n; ++i) {
            if (labels[i] != exp[i]) {
              std::printf("component %lld %lld %lld\n", static_cast<long long>(i), static_cast<long long>(labels[i]),
                          static_cast<long long>(exp[i]));
              std::printf("Wrong output!\n");
              return 1;
            }
          }
          if (!a.quiet) std::printf("Components OK!\n");
        }
        if (!a.components_out.empty()) {
          std::FILE* f = std::fopen(a.components_out.c_str(), "w");
          DBFS_CHECK(f != nullptr, "cannot write " + a.components_out);
          for (int64_t l : labels) std::fprintf(f, "%lld\n", static_cast<long long>(l));
          std::fclose(f);
        }
        if (a.json)
          std::printf("{\"graph\":\"%s\",\"n\":%lld,\"ranks\":%d,\"components\":%lld,\"largest_label\":%lld,"
                      "\"largest_size\":%lld,\"singletons\":%lld,\"ms\":%.6f,\"cc_link_ms\":%.6f,"
                      "\"cc_compress_ms\":%.6f,\"cc_sampled\":%s}\n",
                      gname.c_str(), static_cast<long long>(n), P, static_cast<long long>(c.components),
                      static_cast<long long>(c.largest_label), static_cast<long long>(c.largest_size),
                      static_cast<long long>(c.singletons), c.ms, c.link_ms, c.compress_ms, c.sampled ? "true" : "false");
      }
    }

    // ---- strongly connected components (--strong-components), before the traversals ----
    if (a.strong_components) {
      std::vector<SccResult> sres(static_cast<size_t>(nlocal));
      std::vector<int64_t> labels;
      run_ranks(ranks, [&](int i, RankCtx& rc) {
        sres[i] = rc.engine->strong_components();
        if (i == 0 && leader && ((a.oracle && have_host) || !a.strong_components_out.empty()))
          labels = rc.engine->gather_strong_components();
      }, vgroup.get());
      if (leader) {
        const SccResult& c = sres[0];
        std::printf("strong components %lld largest label %lld size %lld singletons %lld trimmed %lld rounds %lld ms %.3f\n",
                    static_cast<long long>(c.components), static_cast<long long>(c.largest_label),
                    static_cast<long long>(c.largest_size), static_cast<long long>(c.singletons),
                    static_cast<long long>(c.trimmed), static_cast<long long>(c.rounds), c.ms);
        if (a.oracle && have_host) {
          const std::vector<int64_t> exp = cpu_strong_components(full);
          for (int64_t i = 0; i < n; ++i) {
            if (labels[i] != exp[i]) {
              std::printf("strong component %lld %lld %lld\n", static_cast<long long>(i),
                          static_cast<long long>(labels[i]), static_cast<long long>(exp[i]));
              std::printf("Wrong output!\n");
              return 1;
            }
          }
          if (!a.quiet) std::printf("Strong components OK!\n");
        }
        if (!a.strong_components_out.empty()) {
          std::FILE* f = std::fopen(a.strong_components_out.c_str(), "w");
          DBFS_CHECK(f != nullptr, "cannot write " + a.strong_components_out);
          for (int64_t l : labels) std::fprintf(f, "%lld\n", static_cast<long long>(l));
          std::fclose(f);
        }
        if (a.json)
          std::printf("{\"graph\":\"%s\",\"n\":%lld,\"ranks\":%d,\"strong_components\":%lld,\"largest_label\":%lld,"
                      "\"largest_size\":%lld,\"singletons\":%lld,\"trimmed\":%lld,\"rounds\":%lld,\"ms\":%.6f,"
                      "\"scc_trim_ms\":%.6f,\"scc_colour_ms\":%.6f,\"scc_sweeps\":%lld,\"scc_pivot\":%lld}\n",
                      gname.c_str(), static_cast<long long>(n), P, static_cast<long long>(c.components),
                      static_cast<long long>(c.largest_label), static_cast<long long>(c.largest_size),
                      static_cast<long long>(c.singletons), static_cast<long long>(c.trimmed),
                      static_cast<long long>(c.rounds), c.ms, c.trim_ms, c.colour_ms, static_cast<long long>(c.sweeps),
                      static_cast<long long>(c.pivot));
      }
    }

    // ---- eccentricities (--eccentricities), before the traversals ----
    if (a.eccentricities) {
      EccOptions eo_ecc;
      eo_ecc.target = parse_ecc_target(a.ecc_target);
      eo_ecc.component = a.ecc_component == "largest" ? EccOptions::kLargest
                         : a.ecc_component == "all"   ? EccOptions::kAll
                                                      : std::stoll(a.ecc_component);
      eo_ecc.max_passes = a.ecc_max_passes;
      std::vector<EccResult> eres(static_cast<size_t>(nlocal));
      std::vector<int32_t> ecc, lo, hi;
      run_ranks(ranks, [&](int i, RankCtx& rc) {
        eres[i] = rc.engine->eccentricities(eo_ecc);
        if (i == 0 && leader && ((a.oracle && have_host) || !a.eccentricities_out.empty())) {
          ecc = rc.engine->gather_eccentricities();
          rc.engine->gather_eccentricity_bounds(lo, hi);
        }
      }, vgroup.get());
      if (leader) {
        const EccResult& c = eres[0];
        std::printf("eccentricities diameter %lld radius %lld centre %lld periphery %lld settled %lld of %lld passes %lld "
                    "sources %lld exact %d ms %.3f\n",
                    static_cast<long long>(c.diameter), static_cast<long long>(c.radius), static_cast<long long>(c.centre),
                    static_cast<long long>(c.periphery), static_cast<long long>(c.settled),
                    static_cast<long long>(c.scope_size), static_cast<long long>(c.passes),
                    static_cast<long long>(c.sources), c.exact ? 1 : 0, c.ms);
        if (a.oracle && have_host) {
          // One traversal per vertex while scope x entries is small; past that,
          // 16 settled vertices chosen by the seed, one traversal each.
          // (DBFS_ECC_ORACLE_LIMIT: the threshold, for the tests of the sampled branch)
          double limit = 4294967296.0;
          if (const char* e = std::getenv("DBFS_ECC_ORACLE_LIMIT"))
            if (*e) limit = std::atof(e);
          auto wrong = [&](int64_t v, long long got, long long exp) {
            std::printf("eccentricity %lld %lld %lld\n", static_cast<long long>(v), got, exp);
            std::printf("Wrong output!\n");
            return 1;
          };
          if (static_cast<double>(c.scope_size) * static_cast<double>(full.col.size()) <= limit) {
            const std::vector<int32_t> exp = cpu_eccentricities(full);
            int64_t dia = -1, rad = INT32_MAX;
            for (int64_t v = 0; v < n; ++v) {
              if (lo[v] < 0) continue;  // (out of scope)
              if (ecc[v] >= 0 && ecc[v] != exp[v]) return wrong(v, ecc[v], exp[v]);
              if (lo[v] > exp[v] || hi[v] < exp[v]) return wrong(v, lo[v], exp[v]);
              dia = std::max<int64_t>(dia, exp[v]);
              rad = std::min<int64_t>(rad, exp[v]);
            }
            if (c.exact && c.scope_size > 0) {
              if (eo_ecc.target != EccTarget::Radius && c.diameter != dia) return wrong(-1, c.diameter, dia);
              if (eo_ecc.target != EccTarget::Diameter && c.radius != rad) return wrong(-2, c.radius, rad);
            }
            if (!a.quiet) std::printf("Eccentricities OK!\n");
          } else {
            std::vector<int64_t> settled;
            for (int64_t v = 0; v < n; ++v)
              if (ecc[v] >= 0) settled.push_back(v);
            std::mt19937_64 pick(a.seed * 104729 + 5);
            for (int t = 0; t < 16 && !settled.empty(); ++t) {
              const int64_t v = settled[pick() % settled.size()];
              const CpuBfsResult r = cpu_bfs(full, v);
              int64_t deepest = 0;
              for (lvl_t l : r.level)
                if (l != kUnreached) deepest = std::max<int64_t>(deepest, l);
              if (ecc[v] != deepest) return wrong(v, ecc[v], deepest);
            }
            if (!a.quiet) std::printf("Eccentricities OK! (16 sampled)\n");
          }
        }
        if (!a.eccentricities_out.empty()) {
          std::FILE* f = std::fopen(a.eccentricities_out.c_str(), "w");
          DBFS_CHECK(f != nullptr, "cannot write " + a.eccentricities_out);
          for (int32_t e : ecc) std::fprintf(f, "%d\n", e);
          std::fclose(f);
        }
        if (a.json)
          std::printf("{\"graph\":\"%s\",\"n\":%lld,\"ranks\":%d,\"diameter\":%lld,\"radius\":%lld,\"centre\":%lld,"
                      "\"periphery\":%lld,\"settled\":%lld,\"scope_size\":%lld,\"passes\":%lld,\"sources\":%lld,"
                      "\"exact\":%s,\"wide_levels\":%s,\"ecc_target\":\"%s\",\"ms\":%.6f,\"bfs_ms\":%.6f,"
                      "\"bound_ms\":%.6f,\"select_ms\":%.6f}\n",
                      gname.c_str(), static_cast<long long>(n), P, static_cast<long long>(c.diameter),
                      static_cast<long long>(c.radius), static_cast<long long>(c.centre),
                      static_cast<long long>(c.periphery), static_cast<long long>(c.settled),
                      static_cast<long long>(c.scope_size), static_cast<long long>(c.passes),
                      static_cast<long long>(c.sources), c.exact ? "true" : "false", c.wide_levels ? "true" : "false",
                      a.ecc_target.c_str(), c.ms, c.bfs_ms, c.bound_ms, c.select_ms);
      }
    }

    // ---- the reference's single run from <src> ----
    std::vector<RunResult> res(static_cast<size_t>(nlocal));
    std::vector<lvl_t> got;
    std::vector<std::vector<int64_t>> viol(static_cast<size_t>(nlocal));
    if (ref_lines) std::printf("Starting queue parallel bfs.\n");
    run_ranks(ranks, [&](int i, RankCtx& rc) {
      res[i] = rc.engine->run(a.src);
      std::vector<lvl_t> lv = rc.engine->gather_levels();
      if (i == 0) got = std::move(lv);
      if (a.validate) viol[i] = rc.engine->validate(a.src);
    }, vgroup.get());
    if (ref_lines) std::printf("Elapsed time in milliseconds : %li ms.\n", static_cast<long>(res[0].ms));
    int rc_exit = 0;
    if (leader && !expected.empty()) {
      for (int64_t i = 0; i < n; ++i) {
        if (got[i] != expected[i]) {
          std::printf("%lld %d %d\n", static_cast<long long>(i), got[i], expected[i]);
          std::printf("Wrong output!\n");
          return 1;
        }
      }
      if (!a.quiet) std::printf("Output OK!\n\n");
    }
    if (a.validate && leader) {
      const auto& v = viol[0];
      if (v[0] || v[1] || v[2]) {
        std::printf("Validation FAILED: depth-gap %lld, reached-unreached %lld, orphan %lld\n",
                    static_cast<long long>(v[0]), static_cast<long long>(v[1]), static_cast<long long>(v[2]));
        rc_exit = 1;
      } else if (!a.quiet) {
        std::printf("Validation OK (Graph500 level checks)\n");
      }
    }
    if (!a.levels_out.empty() && leader) write_levels(a.levels_out, got);
    // Per-level profile CSV: one row per level of every run.
    std::FILE* csv = nullptr;
    if (!a.level_csv.empty() && leader) {
      csv = std::fopen(a.level_csv.c_str(), "w");
      DBFS_CHECK(csv != nullptr, "cannot write " + a.level_csv);
      std::fprintf(csv, "root,level,dir,frontier,frontier_edges,discovered,ms,run_ms\n");
    }
    auto csv_run = [&](const RunResult& r) {
      if (!csv) return;
      for (const auto& l : r.levels)
        std::fprintf(csv, "%lld,%d,%c,%lld,%lld,%lld,%.4f,%.4f\n", static_cast<long long>(r.source), l.level,
                     l.direction, static_cast<long long>(l.frontier), static_cast<long long>(l.frontier_edges),
                     static_cast<long long>(l.discovered), l.ms, r.ms);
    };
    csv_run(res[0]);
    const std::string bname = ranks[0].be->name() + (ranks[0].be->device_checks_enabled() ? "+checked" : "");
    if (a.json && leader)
      std::printf("%s\n", json_run(res[0], gname, n, m_in, P, a.mode.c_str(), bname, ranks[0].comm->name(), ingest_json).c_str());

    // ---- optional K random roots (Graph500-style GTEPS) ----
    if (a.roots > 0 && a.batch) {
      // ---- the K roots as one concurrent traversal ----
      const std::vector<int64_t> roots = sample_roots(a, part, ranks, multiproc, wrank);
      const bool check = a.oracle && have_host;  // (the same on every rank of this process)
      BatchOptions bopt;
      bopt.direction = parse_batch_direction(a.batch_dir);
      // (--validate, --betweenness: they read the level matrix, oracle or not)
      bopt.keep_levels = a.oracle || a.validate || a.betweenness;
      bopt.validate = a.validate;
      bopt.betweenness = a.betweenness;
      if (!a.betweenness_counts.empty()) bopt.counts = parse_batch_counts(a.betweenness_counts);
      const bool wide_counts = bopt.counts != BatchCounts::Double;
      std::vector<BatchResult> bres(static_cast<size_t>(nlocal));
      std::vector<lvl_t> blv;
      std::vector<double> bdep;
      if (!roots.empty())
        run_ranks(ranks, [&](int i, RankCtx& rc) {
          bres[i] = rc.engine->run_batch(roots, bopt);
          if (a.betweenness) {
            std::vector<double> d = rc.engine->gather_betweenness();
            if (i == 0) bdep = std::move(d);
          }
          if (!a.oracle) return;
          std::vector<lvl_t> lv = rc.engine->gather_batch_levels();
          if (i == 0) blv = std::move(lv);
        }, vgroup.get());
      if (leader && check && !roots.empty()) {
        for (size_t k = 0; k < roots.size(); ++k) {
          const std::vector<lvl_t> exp = cpu_bfs(full, roots[k]).level;
          const lvl_t* row = blv.data() + k * static_cast<size_t>(n);
          for (int64_t i = 0; i < n; ++i) {
            if (row[i] != exp[i]) {
              std::printf("root %lld: %lld %d %d\n", static_cast<long long>(roots[k]), static_cast<long long>(i), row[i],
                          exp[i]);
              std::printf("Wrong output!\n");
              return 1;
            }
          }
        }
        if (!a.quiet) std::printf("Output OK!\n\n");
      }
      if (leader && !roots.empty()) {
        const BatchResult& b = bres[0];
        std::printf("batch roots %zu passes %d ms %.3f aggregate GTEPS %.3f\n", roots.size(), b.passes, b.ms, b.gteps);
        // --validate: the device check's counts (global sums, the same on every rank)
        size_t clean = 0;
        long long viol[3] = {0, 0, 0};
        if (a.validate) {
          for (size_t k = 0; k < roots.size(); ++k) {
            const int64_t* v = b.violations.data() + 3 * k;
            if (!v[0] && !v[1] && !v[2]) ++clean;
            for (int c = 0; c < 3; ++c) viol[c] += v[c];
          }
          std::printf("batch validation %zu/%zu sources clean gap %lld cross %lld orphan %lld\n", clean, roots.size(),
                      viol[0], viol[1], viol[2]);
        }
        if (a.betweenness) {
          size_t top = 0;
          for (size_t v = 1; v < bdep.size(); ++v)
            if (bdep[v] > bdep[top]) top = v;
          std::printf("batch betweenness sources %zu bc_ms %.3f max vertex %zu score %.17g\n", roots.size(), b.bc_ms, top,
                      bdep.empty() ? 0.0 : bdep[top]);
          if (wide_counts) std::printf("batch betweenness wide passes %d of %d\n", b.wide_count_passes, b.passes);
          if (!a.betweenness_out.empty()) {
            std::FILE* f = std::fopen(a.betweenness_out.c_str(), "w");
            DBFS_CHECK(f != nullptr, "cannot write " + a.betweenness_out);
            for (double x : bdep) std::fprintf(f, "%.17g\n", x);
            std::fclose(f);
          }
          if (check) {
            // the sequential oracle: relative error 1e-9, an exact 0 where it has one
            // (wide or auto counts: the oracle's wide form)
            const std::vector<double> exp = cpu_betweenness(full, roots, a.directed, false, wide_counts).dep;
            for (size_t v = 0; v < exp.size(); ++v) {
              const double g = bdep[v], e = exp[v];
              const bool ok = std::isfinite(g) && (e == 0.0 ? g == 0.0 : std::fabs(g - e) <= 1e-9 * std::fabs(e));
              if (!ok) {
                std::printf("betweenness %zu %.17g %.17g\n", v, g, e);
                std::printf("Wrong output!\n");
                return 1;
              }
            }
            if (!a.quiet) std::printf("Betweenness OK!\n");
          }
        }
        if (a.json) {
          std::string extra;
          if (a.betweenness) {
            char ms[64];
            std::snprintf(ms, sizeof(ms), "%.6f", b.bc_ms);
            extra = std::string(",\"bc_ms\":") + ms;
            if (wide_counts) extra += ",\"wide_count_passes\":" + std::to_string(b.wide_count_passes);
          }
          if (a.validate) {
            char ms[64];
            std::snprintf(ms, sizeof(ms), "%.6f", b.check_ms);
            extra += ",\"validated_sources\":\"" + std::to_string(clean) + "/" + std::to_string(roots.size()) +
                    "\",\"check_ms\":" + ms;
          }
          std::printf("{\"graph\":\"%s\",\"n\":%lld,\"ranks\":%d,\"batch\":true,\"roots\":%zu,\"passes\":%d,\"ms\":%.6f,"
                      "\"gteps\":%.6f,\"wide_levels\":%s%s}\n",
                      gname.c_str(), static_cast<long long>(n), P, roots.size(), b.passes, b.ms, b.gteps,
                      b.wide_levels ? "true" : "false", extra.c_str());
        }
        if (a.validate && clean != roots.size()) {
          std::printf("Wrong output!\n");
          rc_exit = 1;
        }
      }
    } else if (a.roots > 0) {
      const std::vector<int64_t> roots = sample_roots(a, part, ranks, multiproc, wrank);
      double inv_sum = 0, ms_sum = 0;
      int64_t e_sum = 0;
      for (int64_t root : roots) {
        run_ranks(ranks, [&](int i, RankCtx& rc) { res[i] = rc.engine->run(root); }, vgroup.get());
        inv_sum += res[0].gteps > 0 ? 1.0 / res[0].gteps : 0;
        ms_sum += res[0].ms;
        e_sum += res[0].edges;
        if (a.json && leader) std::printf("%s\n", json_run(res[0], gname, n, m_in, P, a.mode.c_str(), bname, ranks[0].comm->name()).c_str());
        csv_run(res[0]);
      }
      if (leader && !roots.empty()) {
        const double hm = inv_sum > 0 ? roots.size() / inv_sum : 0.0;
        std::printf("roots %zu  mean ms %.3f  harmonic-mean GTEPS %.3f  aggregate GTEPS %.3f\n", roots.size(),
                    ms_sum / roots.size(), hm, ms_sum > 0 ? e_sum / (ms_sum * 1e6) : 0.0);
      }
    }
    if (csv) std::fclose(csv);
    return rc_exit;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "bfs: %s\n", e.what());
    return 1;
  }
}
