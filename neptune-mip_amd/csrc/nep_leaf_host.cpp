// nep_leaf_host.cpp — the host side of the fixed-placement evaluator (nep_leaf_eval, nep_leaf_routing_entries,
// nep_leaf_moves, nep_leaf_swaps, nep_leaf_search): argument checks, the device workspace, staging of a
// chunk of placements, the launches of nep_leaf.hip / nep_leaf_heur.hip / nep_leaf_moves.hip / nep_leaf_swaps.hip /
// nep_leaf_search.hip and the read-outs through nep_leaf_repair.cpp / nep_leaf_moves.cpp / nep_leaf_swaps.cpp /
// nep_leaf_search.cpp.
#include "nep_model.h"

using namespace nep;

// ---------------------------------------------------------------------------------------------
// fixed-placement evaluator (nep_leaf.hip, nep_leaf_repair.cpp)
// ---------------------------------------------------------------------------------------------
namespace nep {

const char *const kLeafRefusal =
    "the fixed-placement evaluator takes step-1 reference-relaxation models (NEP_STEP1, NEP_RELAX_REFERENCE)";

LeafInstance leaf_instance(const Model &m) {
  LeafInstance in{};
  in.N = m.N; in.F = m.F; in.R = m.R; in.has_n = m.has_n;
  in.eps = m.eps; in.kobj = m.kobj; in.cost_n = m.cost_n;
  in.D = m.Dh.data(); in.W = m.W.data(); in.cpr = m.cprh.data(); in.cores = m.capn.data() + m.N;
  in.row_f = m.row_f.data(); in.row_src = m.row_src.data(); in.frow = m.frow.data();
  return in;
}

// every c and n of z is 0 or 1; c_open [F*N] gets c, *nsum the open nodes
bool leaf_binary(const Model &m, const double *z, uint8_t *c_open, double *nsum) {
  const int FN = m.F * m.N;
  for (int k = 0; k < m.il.n_int; ++k)
    if (z[k] != 0.0 && z[k] != 1.0) return false;
  for (int k = 0; k < FN; ++k) c_open[k] = z[m.il.oc + k] != 0.0;
  double s = 0.0;
  for (int j = 0; j < m.N && m.has_n; ++j) s += z[m.il.on + j];
  *nsum = s;
  return true;
}

// a row without x rejects the placement: C3 memory, C6/C7 n against c, C8 budget, a function without a destination
bool leaf_rejects(const Model &m, const double *z, const uint8_t *c_open) {
  const int N = m.N, F = m.F;
  // (c is walked along its rows: a node's memory still sums over its functions in ascending order)
  std::vector<double> mem(N, 0.0);
  std::vector<uint8_t> any(N, 0);
  for (int f = 0; f < F; ++f) {
    const uint8_t *cf = c_open + (size_t)f * N;
    bool dest = false;
    for (int j = 0; j < N; ++j)
      if (cf[j]) { mem[j] += m.mem_f[f]; any[j] = 1; dest = true; }
    if (!dest) return true;
  }
  for (int j = 0; j < N; ++j) {
    if (mem[j] > m.capn[j] + 1e-9) return true;
    if (m.has_n) {
      const double nj = z[m.il.on + j];
      if ((any[j] != 0) != (nj != 0.0)) return true;
      if (m.node_cost[j] * nj > m.node_budget + 1e-9) return true;
    }
  }
  return false;
}

void leaf_point_out(const LeafPoint &pt, int32_t *row, int32_t *dst, double *val) {
  std::memcpy(row, pt.row.data(), pt.row.size() * sizeof(int32_t));
  std::memcpy(dst, pt.dst.data(), pt.dst.size() * sizeof(int32_t));
  std::memcpy(val, pt.val.data(), pt.val.size() * sizeof(double));
}

}  // namespace nep

// a failure part-way (rc != 0) gives back what the call allocated since `mark` (the next call starts over); returns rc
static int leaf_allocs_rollback(Model &m, size_t mark, int rc) {
  while (rc && m.allocs.size() > mark) {
    (void)hipFree(m.allocs.back());
    m.allocs.pop_back();
  }
  return rc;
}

// the evaluator's workspace, on first use: one chunk of `cap` placements (the shares, [cap][F][N] doubles, held to
// 64 MiB; at most 64 placements), the fp64 instance on the device and the pinned staging of a chunk
static int ensure_leaf_alloc(Model &m) {
  std::unique_ptr<Model::LeafWork> w(new Model::LeafWork());
  const size_t N = m.N, F = m.F, R = m.R;
  w->cap = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)64 << 20) / (F * N * sizeof(double))));
  int maxrf = 1;
  for (int f = 0; f < m.F; ++f) maxrf = std::max(maxrf, m.frow[f + 1] - m.frow[f]);
  // leaf_assign's workgroup: sized to the rows of a function while every function takes them a lane per row (N <=
  // kLeafLaneK: no open list is longer); else a function may take a wave per row, and gets all four waves
  w->threads = m.N > kLeafLaneK ? kLeafThreads : maxrf <= 64 ? 64 : maxrf <= 128 ? 128 : kLeafThreads;
  const size_t B = w->cap;
  LeafView &v = w->v;
  v.N = m.N; v.F = m.F; v.R = m.R; v.B = 0; v.kobj = m.kobj;
  v.frow = m.v.frow;
  int rc;
  std::vector<int32_t> src(m.row_src.begin(), m.row_src.end());
  std::vector<double> cores(m.capn.begin() + N, m.capn.end());
  if ((rc = upload(m, &v.row_src, src))) return rc;
  if ((rc = upload(m, &v.D, m.Dh))) return rc;
  if ((rc = upload(m, &v.W, m.W))) return rc;
  if ((rc = upload(m, &v.cpr, m.cprh))) return rc;
  if ((rc = upload(m, &v.cores, cores))) return rc;
  uint8_t *d_open = nullptr;
  if ((rc = dalloc(m, &d_open, B * F * N))) return rc;
  v.open = d_open;
  if ((rc = dalloc(m, &v.y, B * N))) return rc;
  if ((rc = dalloc(m, &v.ybest, B * N))) return rc;
  if ((rc = dalloc(m, &v.share, B * F * N))) return rc;
  if ((rc = dalloc(m, &v.fpart, B * F))) return rc;
  if ((rc = dalloc(m, &v.load, B * N))) return rc;
  if ((rc = dalloc(m, &v.g, B * N))) return rc;
  if ((rc = dalloc(m, &v.asg0, B * R))) return rc;
  if ((rc = dalloc(m, &v.asg, B * R))) return rc;
  if ((rc = dalloc(m, &v.ctrl, B))) return rc;
  // pinned: [ctrl | y | load | asg0 | open]
  const size_t bytes = B * (sizeof(LeafCtrl) + 2 * N * sizeof(double) + R * sizeof(int32_t) + F * N) + 64;
  if (hipHostMalloc(&w->pinned, bytes) != hipSuccess) return fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator)");
  char *p = static_cast<char *>(w->pinned);
  w->h_ctrl = reinterpret_cast<LeafCtrl *>(p); p += B * sizeof(LeafCtrl);
  w->h_y = reinterpret_cast<double *>(p); p += B * N * sizeof(double);
  w->h_load = reinterpret_cast<double *>(p); p += B * N * sizeof(double);
  w->h_asg0 = reinterpret_cast<int32_t *>(p); p += B * R * sizeof(int32_t);
  w->h_open = reinterpret_cast<uint8_t *>(p);
  m.leaf = std::move(w);
  return NEP_OK;
}
int nep::ensure_leaf(Model &m) {
  if (m.leaf) return NEP_OK;
  const size_t n0 = m.allocs.size();
  return leaf_allocs_rollback(m, n0, ensure_leaf_alloc(m));
}

// the per-round repair's workspace (nep_leaf_heur.hip), on the first call that asks for it: the open lists, the
// repair's state and the best round's copies for one chunk, and round_upper for `rounds` rounds
static int ensure_leaf_heur(Model &m, int rounds) {
  Model::LeafWork &w = *m.leaf;
  const size_t N = m.N, F = m.F, R = m.R, B = w.cap;
  if (!w.heur) {
    const size_t n0 = m.allocs.size();
    LeafHeurView h{};
    std::vector<int32_t> rf(m.row_f.begin(), m.row_f.end());
    int rc = upload(m, &h.row_f, rf);
    if (!rc) rc = dalloc(m, &h.opl, B * F * N);
    if (!rc) rc = dalloc(m, &h.opn, B * F);
    if (!rc) rc = dalloc(m, &h.flow, B * R);
    if (!rc) rc = dalloc(m, &h.room, B * F);
    if (!rc) rc = dalloc(m, &h.fcost, B * F);
    if (!rc) rc = dalloc(m, &h.nrows, B * R);
    if (!rc) rc = dalloc(m, &h.asgrep, B * R);
    if (!rc) rc = dalloc(m, &h.loadrep, B * N);
    if (!rc) rc = dalloc(m, &h.best, B);
    // pinned: [best | loadrep | asgrep]
    void *pin = nullptr;
    if (!rc && hipHostMalloc(&pin, B * (sizeof(LeafHeurBest) + N * sizeof(double) + R * sizeof(int32_t)) + 64) !=
                   hipSuccess)
      rc = fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, per-round repair)");
    if (rc) return leaf_allocs_rollback(m, n0, rc);
    h.floor_ = 1.0 - m.eps;
    w.hv = h;
    w.pinned_h = pin;
    char *p = static_cast<char *>(pin);
    w.h_best = reinterpret_cast<LeafHeurBest *>(p); p += B * sizeof(LeafHeurBest);
    w.h_loadrep = reinterpret_cast<double *>(p); p += B * N * sizeof(double);
    w.h_asgrep = reinterpret_cast<int32_t *>(p);
    w.heur = true;
  }
  if (rounds + 1 > w.ru_stride) {
    double *d = nullptr;
    void *pin = nullptr;
    const int rc = dalloc(m, &d, B * (size_t)(rounds + 1));
    if (rc) return rc;
    if (hipHostMalloc(&pin, B * (size_t)(rounds + 1) * sizeof(double)) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, round_upper)");
    if (w.pinned_ru) (void)hipHostFree(w.pinned_ru);
    w.pinned_ru = pin;
    w.h_ru = static_cast<double *>(pin);
    w.hv.round_upper = d;   // (an earlier, shorter one stays with the model's allocations)
    w.ru_stride = rounds + 1;
  }
  return NEP_OK;
}

// The argument checks nep_leaf_eval_ex, nep_leaf_moves and nep_leaf_swaps share, in the order both make them: the model's kind, n, the
// entry's own checks (own_checks, between the two), every entry of z_leaf 0 or 1, every price finite and >= 0
// (prices_name: the argument's name in the message).
template <typename OwnChecks>
static int leaf_check_args(const Model &m, int32_t n, const double *z_leaf, const double *prices,
                           const char *prices_name, OwnChecks own_checks) {
  if (m.step2 || m.fac) return fail(NEP_ERR_ARG, kLeafRefusal);
  if (n < 1) return fail(NEP_ERR_ARG, "n must be at least 1");
  if (const int rc = own_checks()) return rc;
  const size_t N = m.N, ni = m.il.n_int;
  for (size_t k = 0; k < (size_t)n * ni; ++k)
    if (z_leaf[k] != 0.0 && z_leaf[k] != 1.0)
      return fail(NEP_ERR_ARG, "placement " + std::to_string(k / ni) + ": entry " + std::to_string(k % ni) +
                                   " is not 0 or 1 (a leaf fixes every c and n)");
  for (size_t k = 0; prices && k < (size_t)n * N; ++k)
    if (!(prices[k] >= 0.0) || prices[k] == INF)
      return fail(NEP_ERR_ARG, std::string(prices_name) + " must be finite and >= 0");
  return NEP_OK;
}

// The first pass over a call's placements: those no row without x rejects reach the device, in order; for a rejected
// one the caller writes its outputs (rejected(b)).
template <typename Rejected>
static std::vector<int> leaf_first_pass(const Model &m, int32_t n, const double *z_leaf, Rejected rejected) {
  const size_t ni = m.il.n_int;
  std::vector<uint8_t> c_open((size_t)m.F * m.N);
  std::vector<int> todo;
  for (int b = 0; b < n; ++b) {
    double nsum = 0.0;
    leaf_binary(m, z_leaf + b * ni, c_open.data(), &nsum);
    if (leaf_rejects(m, z_leaf + b * ni, c_open.data())) rejected(b);
    else todo.push_back(b);
  }
  return todo;
}

// One chunk of B placements, todo[0 .. B), staged and on its way to the device: their c in h_open, their open nodes in
// nsums, their prices (or zeros) in h_y; the copies of open and y are enqueued on the auxiliary stream.
static int leaf_stage_chunk(Model &m, const LeafView &v, const int *todo, int B, const double *z_leaf,
                            const double *prices, std::vector<double> &nsums) {
  Model::LeafWork &w = *m.leaf;
  const size_t N = m.N, F = m.F, ni = m.il.n_int;
  nsums.resize(B);
  for (int q = 0; q < B; ++q) {
    const int b = todo[q];
    leaf_binary(m, z_leaf + b * ni, w.h_open + q * F * N, &nsums[q]);
    if (prices) std::memcpy(w.h_y + q * N, prices + b * N, N * sizeof(double));
    else std::fill(w.h_y + q * N, w.h_y + (q + 1) * N, 0.0);
  }
  HIPCHK(hipMemcpyAsync(const_cast<uint8_t *>(v.open), w.h_open, B * F * N, hipMemcpyHostToDevice, m.aux));
  HIPCHK(hipMemcpyAsync(v.y, w.h_y, B * N * sizeof(double), hipMemcpyHostToDevice, m.aux));
  return NEP_OK;
}

extern "C" {

int nep_leaf_eval(void *model, int32_t n, const double *z_leaf, const nep_leaf_opts *opts, const double *prices_in,
                  double *lower, double *upper, int32_t *status, double *prices_out, double *cpu) {
  return nep_leaf_eval_ex(model, n, z_leaf, opts, nullptr, prices_in, lower, upper, status, prices_out, cpu, nullptr,
                          nullptr, nullptr);
}

int nep_leaf_eval_ex(void *model, int32_t n, const double *z_leaf, const nep_leaf_opts *opts,
                     const nep_leaf_heur_opts *heur, const double *prices_in, double *lower, double *upper,
                     int32_t *status, double *prices_out, double *cpu, int32_t *upper_round, double *device_upper,
                     double *round_upper) {
  if (!model || !z_leaf || !lower || !upper || !status) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  const int every = heur ? heur->repair_every : 0;
  const int rounds = opts ? opts->rounds : 32;
  const double cutoff = opts ? opts->cutoff : INF;
  const double tol = opts && opts->tol > 0.0 ? opts->tol : 1e-6;
  int rc = leaf_check_args(m, n, z_leaf, prices_in, "prices_in", [&]() -> int {
    if (every < 0) return fail(NEP_ERR_ARG, "repair_every must be >= 0");
    if (rounds < 0 || cutoff != cutoff) return fail(NEP_ERR_ARG, "bad rounds or cutoff");
    return NEP_OK;
  });
  if (rc) return rc;
  const size_t N = m.N, F = m.F, R = m.R;
  if ((rc = ensure_leaf(m))) return rc;
  if (every && (rc = ensure_leaf_heur(m, rounds))) return rc;
  Model::LeafWork &w = *m.leaf;
  w.points.assign(n, LeafPoint());
  const LeafInstance in = leaf_instance(m);
  const size_t nr = (size_t)rounds + 1;
  for (int b = 0; b < n; ++b) {
    if (upper_round) upper_round[b] = -1;
    if (device_upper) device_upper[b] = INF;
    if (round_upper) std::fill(round_upper + b * nr, round_upper + (b + 1) * nr, INF);
    if (prices_out) std::fill(prices_out + b * N, prices_out + (b + 1) * N, 0.0);
    if (cpu) std::fill(cpu + b * N, cpu + (b + 1) * N, 0.0);
  }
  // the placements that reach the device
  const std::vector<int> todo = leaf_first_pass(m, n, z_leaf, [&](int b) {
    lower[b] = upper[b] = INF;
    status[b] = NEP_LEAF_INFEASIBLE;
  });
  std::vector<double> nsums;
  for (size_t t0 = 0; t0 < todo.size(); t0 += w.cap) {
    const int B = (int)std::min<size_t>(w.cap, todo.size() - t0);
    LeafView v = w.v;
    v.B = B;
    if ((rc = leaf_stage_chunk(m, v, todo.data() + t0, B, z_leaf, prices_in, nsums))) return rc;
    for (int q = 0; q < B; ++q) {
      LeafCtrl &c = w.h_ctrl[q];
      c = LeafCtrl{};
      c.base = m.has_n ? m.cost_n * nsums[q] : 0.0;
      c.best = -INF;
      c.lam = 1.0;
      c.cutoff = cutoff;
    }
    HIPCHK(hipMemcpyAsync(v.ctrl, w.h_ctrl, B * sizeof(LeafCtrl), hipMemcpyHostToDevice, m.aux));
    HIPCHK(hipMemcpyAsync(v.ybest, w.h_y, B * N * sizeof(double), hipMemcpyHostToDevice, m.aux));
    LeafHeurView hv = w.hv;
    hv.rounds = rounds;
    hv.every = every;
    HIPCHK(launch_leaf_rounds(v, rounds, w.threads, m.aux, every ? &hv : nullptr));
    // one read at the end: bounds and flags, the best prices, the last loads, the round-0 assignment
    HIPCHK(hipMemcpyAsync(w.h_ctrl, v.ctrl, B * sizeof(LeafCtrl), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_y, v.ybest, B * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_load, v.load, B * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_asg0, v.asg0, B * R * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
    if (every) {   // the best repaired round: its objective and number, its loads and assignment; the rounds' verdicts
      HIPCHK(hipMemcpyAsync(w.h_best, hv.best, B * sizeof(LeafHeurBest), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_loadrep, hv.loadrep, B * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_asgrep, hv.asgrep, B * R * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_ru, hv.round_upper, B * nr * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    }
    HIPCHK(hipStreamSynchronize(m.aux));
    for (int q = 0; q < B; ++q) {
      const int b = todo[t0 + q];
      const LeafCtrl &c = w.h_ctrl[q];
      if (every) {
        if (device_upper) device_upper[b] = w.h_best[q].obj;
        if (round_upper) std::memcpy(round_upper + b * nr, w.h_ru + q * nr, nr * sizeof(double));
      }
      lower[b] = c.best;
      upper[b] = INF;
      if (prices_out) std::memcpy(prices_out + b * N, w.h_y + q * N, N * sizeof(double));
      if (cpu) std::memcpy(cpu + b * N, w.h_load + q * N, N * sizeof(double));
      if (c.cut) {
        status[b] = NEP_LEAF_CUTOFF;
        continue;
      }
      LeafPoint &pt = w.points[b];
      leaf_repair(in, w.h_open + q * F * N, nsums[q], w.h_asg0 + q * R, pt);
      int from = pt.found ? 0 : -1;
      if (every && w.h_best[q].round >= 0) {
        // the device chose the round; its point is the host's, verified in fp64, from the loads the device started at
        LeafPoint alt;
        leaf_repair(in, w.h_open + q * F * N, nsums[q], w.h_asgrep + q * R, alt, w.h_loadrep + q * N);
        if (alt.found && (!pt.found || alt.obj < pt.obj)) {
          pt = std::move(alt);
          from = w.h_best[q].round;
        }
      }
      if (upper_round) upper_round[b] = from;
      if (!pt.found) {
        status[b] = NEP_LEAF_NO_POINT;
        continue;
      }
      upper[b] = pt.obj;
      if (cpu) std::memcpy(cpu + b * N, pt.cpu.data(), N * sizeof(double));
      status[b] = pt.obj - c.best <= tol * std::max(1.0, std::fabs(c.best)) ? NEP_LEAF_EXACT : NEP_LEAF_FEASIBLE;
    }
  }
  return NEP_OK;
}

int nep_leaf_routing_entries(void *model, int32_t k, int64_t capacity, int64_t *n_entries, int32_t *row, int32_t *dst,
                             double *val) {
  if (!model || !n_entries) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (m.step2 || m.fac) return fail(NEP_ERR_ARG, kLeafRefusal);
  if (!m.leaf || k < 0 || (size_t)k >= m.leaf->points.size())
    return fail(NEP_ERR_ARG, "no placement " + std::to_string(k) + " in the last nep_leaf_eval call");
  const LeafPoint &pt = m.leaf->points[k];
  if (!pt.found) return fail(NEP_ERR_STATE, "placement " + std::to_string(k) + " has no routing (upper = +inf)");
  const int64_t cnt = (int64_t)pt.row.size();
  *n_entries = cnt;
  if (capacity < cnt) return NEP_OK;   // size query
  if (!row || !dst || !val) return fail(NEP_ERR_ARG, "null argument");
  leaf_point_out(pt, row, dst, val);
  return NEP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// priced moves of a placement (nep_leaf_moves.hip, nep_leaf_moves.cpp; DESIGN.md §7 "Priced moves")
// ---------------------------------------------------------------------------------------------
namespace nep {

LeafLimits leaf_limits(const Model &m) {
  return LeafLimits{m.mem_f.data(), m.capn.data(), m.node_cost.data(), m.node_budget};
}

void leaf_moves_out(const std::vector<LeafMove> &mv, int max_moves, int32_t *n_moves, int32_t *kind, int32_t *fn,
                    int32_t *node, double *delta) {
  *n_moves = (int32_t)mv.size();
  for (int q = 0; q < max_moves; ++q) {
    const bool has = q < (int)mv.size();
    kind[q] = has ? mv[q].kind : -1;
    fn[q] = has ? mv[q].fn : -1;
    node[q] = has ? mv[q].node : -1;
    delta[q] = has ? mv[q].delta : INF;
  }
}

// L(C, y) = cost_n sum n + the functions' minima - y . cores, as leaf_step sums it per thread
static double leaf_lagr(const Model &m, const double *fpart, const double *y, const double *cores, double nsum) {
  double sf = 0.0, sy = 0.0;
  for (int f = 0; f < m.F; ++f) sf += fpart[f];
  for (int j = 0; j < m.N; ++j) sy += y[j] * cores[j];
  return (m.has_n ? m.cost_n * nsum : 0.0) + sf - sy;
}

// a pricing kernel keeps five doubles and four ints per destination / row in LDS and is held to the 64 KiB a launch
// gets without asking for more (the evaluator's own 36 bytes fit every admitted N)
static int leaf_check_lds(const Model &m, const char *entry, size_t (*lds)(int)) {
  if (lds(m.N) <= kLeafMovesLdsCap) return NEP_OK;
  int nmax = m.N;
  while (nmax > 1 && lds(nmax) > kLeafMovesLdsCap) --nmax;
  return fail(NEP_ERR_ARG, std::string(entry) + ": n_nodes " + std::to_string(m.N) + " needs " +
                               std::to_string(lds(m.N)) + " bytes of LDS per workgroup, above " +
                               std::to_string(kLeafMovesLdsCap) + " (largest supported n_nodes: " +
                               std::to_string(nmax) + ")");
}

}  // namespace nep

// the pinned staging of a chunk's [table | fpart], on the first call that reads a priced table
static int ensure_leaf_moves(Model &m) {
  Model::LeafWork &w = *m.leaf;
  if (w.pinned_m) return NEP_OK;
  const size_t N = m.N, F = m.F, B = w.cap;
  if (hipHostMalloc(&w.pinned_m, B * (F * N + F) * sizeof(double)) != hipSuccess) {
    w.pinned_m = nullptr;
    return fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, priced moves)");
  }
  w.h_table = static_cast<double *>(w.pinned_m);
  w.h_fpart = w.h_table + B * F * N;
  return NEP_OK;
}

extern "C" {

int nep_leaf_moves(void *model, int32_t n, const double *z_leaf, const double *prices, int32_t max_moves,
                   int32_t *n_moves, int32_t *kind, int32_t *fn, int32_t *node, double *delta, double *lagr,
                   double *table) {
  if (!model || !z_leaf || !n_moves) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  int rc = leaf_check_args(m, n, z_leaf, prices, "prices", [&]() -> int {
    if (max_moves < 0) return fail(NEP_ERR_ARG, "max_moves must be >= 0");
    if (max_moves > 0 && (!kind || !fn || !node || !delta)) return fail(NEP_ERR_ARG, "null argument");
    return leaf_check_lds(m, "nep_leaf_moves", leaf_moves_lds);
  });
  if (rc) return rc;
  const size_t N = m.N, F = m.F;
  if ((rc = ensure_leaf(m))) return rc;
  if ((rc = ensure_leaf_moves(m))) return rc;
  Model::LeafWork &w = *m.leaf;
  const LeafInstance in = leaf_instance(m);
  const LeafLimits lim = leaf_limits(m);
  std::vector<LeafMove> mv;
  // the placements that reach the device
  const std::vector<int> todo = leaf_first_pass(m, n, z_leaf, [&](int b) {
    mv.clear();
    leaf_moves_out(mv, max_moves, n_moves + b, kind + (size_t)b * max_moves, fn + (size_t)b * max_moves,
                   node + (size_t)b * max_moves, delta + (size_t)b * max_moves);
    if (lagr) lagr[b] = INF;
    if (table) std::fill(table + b * F * N, table + (b + 1) * F * N, INF);
  });
  std::vector<double> nsums;
  for (size_t t0 = 0; t0 < todo.size(); t0 += w.cap) {
    const int B = (int)std::min<size_t>(w.cap, todo.size() - t0);
    LeafView v = w.v;
    v.B = B;
    if ((rc = leaf_stage_chunk(m, v, todo.data() + t0, B, z_leaf, prices, nsums))) return rc;
    HIPCHK(launch_leaf_moves(v, w.threads, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_table, v.share, B * F * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_fpart, v.fpart, B * F * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipStreamSynchronize(m.aux));
    for (int q = 0; q < B; ++q) {
      const int b = todo[t0 + q];
      const double *tb = w.h_table + q * F * N;
      if (lagr) lagr[b] = leaf_lagr(m, w.h_fpart + q * F, w.h_y + q * N, in.cores, nsums[q]);
      if (table) std::memcpy(table + b * F * N, tb, F * N * sizeof(double));
      mv.clear();
      if (max_moves > 0) leaf_move_list(in, lim, w.h_open + q * F * N, tb, max_moves, mv);
      leaf_moves_out(mv, max_moves, n_moves + b, kind + (size_t)b * max_moves, fn + (size_t)b * max_moves,
                     node + (size_t)b * max_moves, delta + (size_t)b * max_moves);
    }
  }
  return NEP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// priced swaps of a placement (nep_leaf_swaps.hip, nep_leaf_swaps.cpp; DESIGN.md §7 "Priced swaps")
// ---------------------------------------------------------------------------------------------
namespace nep {

void leaf_swaps_out(const std::vector<LeafSwap> &sw, int max_moves, int32_t *n_moves, int32_t *fn, int32_t *from,
                    int32_t *to, double *delta) {
  *n_moves = (int32_t)sw.size();
  for (int q = 0; q < max_moves; ++q) {
    const bool has = q < (int)sw.size();
    fn[q] = has ? sw[q].fn : -1;
    from[q] = has ? sw[q].from : -1;
    to[q] = has ? sw[q].to : -1;
    delta[q] = has ? sw[q].delta : INF;
  }
}

}  // namespace nep

// the swaps' workspace, on the first call: the memory figures of the ADD screens, a chunk's node state and records
static int ensure_leaf_swaps(Model &m) {
  Model::LeafWork &w = *m.leaf;
  if (w.swaps) return NEP_OK;
  const size_t N = m.N, F = m.F, B = w.cap, n0 = m.allocs.size();
  LeafSwapView sv{};
  std::vector<double> fmem(m.mem_f.begin(), m.mem_f.begin() + F), nmem1(N);
  for (size_t j = 0; j < N; ++j) nmem1[j] = m.capn[j] + 1e-9;
  int32_t *ncnt = nullptr;
  double *mem = nullptr;
  int rc = upload(m, &sv.fmem, fmem);
  if (!rc) rc = upload(m, &sv.nmem1, nmem1);
  if (!rc) rc = dalloc(m, &ncnt, B * N);
  if (!rc) rc = dalloc(m, &mem, B * N);
  if (!rc) rc = dalloc(m, &sv.rec, B * F * kLeafSwapPerFn);
  // pinned: [rec | fpart | mem | ncnt]
  void *pin = nullptr;
  if (!rc && hipHostMalloc(&pin, B * (F * kLeafSwapPerFn * sizeof(LeafSwapRec) + F * sizeof(double) +
                                      N * (sizeof(double) + sizeof(int32_t))) + 64) != hipSuccess)
    rc = fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, priced swaps)");
  if (rc) return leaf_allocs_rollback(m, n0, rc);
  sv.ncnt = ncnt;
  sv.mem = mem;
  sv.cn = m.has_n ? m.cost_n : 0.0;
  w.sv = sv;
  w.pinned_s = pin;
  char *p = static_cast<char *>(pin);
  w.h_rec = reinterpret_cast<LeafSwapRec *>(p); p += B * F * kLeafSwapPerFn * sizeof(LeafSwapRec);
  w.h_sfpart = reinterpret_cast<double *>(p); p += B * F * sizeof(double);
  w.h_mem = reinterpret_cast<double *>(p); p += B * N * sizeof(double);
  w.h_ncnt = reinterpret_cast<int32_t *>(p);
  w.swaps = true;
  return NEP_OK;
}

// the tables' part of it, on the first call that asks for them
static int ensure_leaf_swap_tables(Model &m) {
  Model::LeafWork &w = *m.leaf;
  if (w.pinned_st) return NEP_OK;
  const size_t N = m.N, F = m.F, B = w.cap;
  if (!w.d_sfrom) {
    const int rc = dalloc(m, &w.d_sfrom, B * F * N);
    if (rc) return rc;
  }
  if (hipHostMalloc(&w.pinned_st, B * F * N * (sizeof(double) + sizeof(int32_t))) != hipSuccess) {
    w.pinned_st = nullptr;
    return fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, swap tables)");
  }
  w.h_sbest = static_cast<double *>(w.pinned_st);
  w.h_sfrom = reinterpret_cast<int32_t *>(w.h_sbest + B * F * N);
  return NEP_OK;
}

extern "C" {

int nep_leaf_swaps(void *model, int32_t n, const double *z_leaf, const double *prices, int32_t per_fn,
                   int32_t max_moves, int32_t *n_moves, int32_t *fn, int32_t *from, int32_t *to, double *delta,
                   double *lagr, double *best, int32_t *best_from) {
  if (!model || !z_leaf || !n_moves) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  int rc = leaf_check_args(m, n, z_leaf, prices, "prices", [&]() -> int {
    if (per_fn < 1 || per_fn > kLeafSwapPerFn)
      return fail(NEP_ERR_ARG, "per_fn must be 1 .. " + std::to_string(kLeafSwapPerFn));
    if (max_moves < 0) return fail(NEP_ERR_ARG, "max_moves must be >= 0");
    if (max_moves > 0 && (!fn || !from || !to || !delta)) return fail(NEP_ERR_ARG, "null argument");
    return leaf_check_lds(m, "nep_leaf_swaps", leaf_swaps_lds);
  });
  if (rc) return rc;
  const size_t N = m.N, F = m.F;
  const bool tables = best || best_from;
  if ((rc = ensure_leaf(m))) return rc;
  if ((rc = ensure_leaf_swaps(m))) return rc;
  if (tables && (rc = ensure_leaf_swap_tables(m))) return rc;
  Model::LeafWork &w = *m.leaf;
  const LeafInstance in = leaf_instance(m);
  const LeafLimits lim = leaf_limits(m);
  std::vector<LeafSwap> sw;
  const auto out = [&](int b) {
    leaf_swaps_out(sw, max_moves, n_moves + b, fn + (size_t)b * max_moves, from + (size_t)b * max_moves,
                   to + (size_t)b * max_moves, delta + (size_t)b * max_moves);
  };
  // the placements that reach the device
  const std::vector<int> todo = leaf_first_pass(m, n, z_leaf, [&](int b) {
    sw.clear();
    out(b);
    if (lagr) lagr[b] = INF;
    if (best) std::fill(best + b * F * N, best + (b + 1) * F * N, INF);
    if (best_from) std::fill(best_from + b * F * N, best_from + (b + 1) * F * N, -1);
  });
  std::vector<double> nsums;
  for (size_t t0 = 0; t0 < todo.size(); t0 += w.cap) {
    const int B = (int)std::min<size_t>(w.cap, todo.size() - t0);
    LeafView v = w.v;
    v.B = B;
    if ((rc = leaf_stage_chunk(m, v, todo.data() + t0, B, z_leaf, prices, nsums))) return rc;
    // the nodes' state behind the ADD screens: leaf_move_list's sums in its order (a node's memory over its functions
    // ascending), c walked along its rows
    for (int q = 0; q < B; ++q) {
      double *mem = w.h_mem + q * N;
      int32_t *cnt = w.h_ncnt + q * N;
      std::fill(mem, mem + N, 0.0);
      std::fill(cnt, cnt + N, 0);
      for (size_t f = 0; f < F; ++f) {
        const uint8_t *cf = w.h_open + (q * F + f) * N;
        for (size_t j = 0; j < N; ++j)
          if (cf[j]) { mem[j] += lim.fmem[f]; ++cnt[j]; }
      }
      for (size_t j = 0; j < N && in.has_n; ++j)
        if (cnt[j] == 0 && !(lim.cost[j] <= lim.budget + 1e-9)) cnt[j] = -1;
    }
    LeafSwapView sv = w.sv;
    sv.per_fn = per_fn;
    sv.best = tables ? v.share : nullptr;
    sv.best_from = tables ? w.d_sfrom : nullptr;
    HIPCHK(hipMemcpyAsync(const_cast<double *>(sv.mem), w.h_mem, B * N * sizeof(double), hipMemcpyHostToDevice, m.aux));
    HIPCHK(hipMemcpyAsync(const_cast<int32_t *>(sv.ncnt), w.h_ncnt, B * N * sizeof(int32_t), hipMemcpyHostToDevice,
                          m.aux));
    HIPCHK(launch_leaf_swaps(v, sv, w.threads, m.aux));
    // the read-out: per_fn records per (placement, function); the [F][N] tables only for a caller that asked
    HIPCHK(hipMemcpyAsync(w.h_rec, sv.rec, B * F * per_fn * sizeof(LeafSwapRec), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_sfpart, v.fpart, B * F * sizeof(double), hipMemcpyDeviceToHost, m.aux));
    if (tables) {
      HIPCHK(hipMemcpyAsync(w.h_sbest, sv.best, B * F * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_sfrom, sv.best_from, B * F * N * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
    }
    HIPCHK(hipStreamSynchronize(m.aux));
    for (int q = 0; q < B; ++q) {
      const int b = todo[t0 + q];
      if (lagr) lagr[b] = leaf_lagr(m, w.h_sfpart + q * F, w.h_y + q * N, in.cores, nsums[q]);
      if (best) std::memcpy(best + b * F * N, w.h_sbest + q * F * N, F * N * sizeof(double));
      if (best_from) std::memcpy(best_from + b * F * N, w.h_sfrom + q * F * N, F * N * sizeof(int32_t));
      sw.clear();
      for (size_t k = 0; max_moves > 0 && k < F * per_fn; ++k) {
        const LeafSwapRec &r = w.h_rec[q * F * per_fn + k];
        if (r.to >= 0) sw.push_back(LeafSwap{(int32_t)(k / per_fn), r.from, r.to, r.delta});
      }
      leaf_swap_merge(sw, max_moves);
      out(b);
    }
  }
  return NEP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// the native placement search (nep_leaf_search.hip, nep_leaf_search.cpp; DESIGN.md §7 "Native search")
// ---------------------------------------------------------------------------------------------

// the search's workspace, on the first call: a chunk's move records and the nodes that may not open
int nep::ensure_leaf_search(Model &m) {
  Model::LeafWork &w = *m.leaf;
  if (w.search) return NEP_OK;
  const size_t N = m.N, B = w.cap, n0 = m.allocs.size();
  std::vector<uint8_t> over(N, 0);
  for (size_t j = 0; j < N && m.has_n; ++j) over[j] = !(m.node_cost[j] <= m.node_budget + 1e-9);
  const uint8_t *d_over = nullptr;
  int rc = upload(m, &d_over, over);
  if (!rc) rc = dalloc(m, &w.d_mv, B);
  void *pin = nullptr;
  if (!rc && hipHostMalloc(&pin, B * sizeof(LeafSearchMove)) != hipSuccess)
    rc = fail(NEP_ERR_NOMEM, "hipHostMalloc (leaf evaluator, native search)");
  if (rc) {
    w.d_mv = nullptr;
    return leaf_allocs_rollback(m, n0, rc);
  }
  w.d_over = const_cast<uint8_t *>(d_over);
  w.pinned_q = pin;
  w.h_mv = static_cast<LeafSearchMove *>(pin);
  w.search = true;
  return NEP_OK;
}

// the view of the B slots from slot s on
LeafView nep::leaf_view_at(const LeafView &v, size_t s, int B) {
  const size_t N = v.N, F = v.F, R = v.R;
  LeafView o = v;
  o.B = B;
  o.open += s * F * N;
  o.y += s * N; o.ybest += s * N;
  o.share += s * F * N; o.fpart += s * F;
  o.load += s * N; o.g += s * N;
  o.asg0 += s * R; o.asg += s * R;
  o.ctrl += s;
  return o;
}
static LeafHeurView leaf_heur_view_at(const LeafHeurView &h, const LeafView &v, size_t s, int rounds, int every) {
  const size_t N = v.N, F = v.F, R = v.R;
  LeafHeurView o = h;
  o.rounds = rounds;
  o.every = every;
  o.opl += s * F * N; o.opn += s * F;
  o.flow += s * R; o.room += s * F; o.fcost += s * F;
  o.nrows += s * R; o.asgrep += s * R; o.loadrep += s * N;
  o.best += s;
  o.round_upper += s * ((size_t)rounds + 1);
  return o;
}

namespace {

// one pass's candidate moves and what the device and the host found for each
struct SearchPass {
  std::vector<LeafSearchMove> mv;
  std::vector<double> delta;
  std::vector<double> lower, dq;     // LeafCtrl::best; LeafHeurBest::obj (+inf: none)
  std::vector<uint8_t> live;         // reached the device and was not cut off
  std::vector<int> slot, chunk;      // where its rounds ran (-1: rejected on the host)
  void reset(size_t k) {
    lower.assign(k, INF); dq.assign(k, INF);
    live.assign(k, 0); slot.assign(k, -1); chunk.assign(k, -1);
  }
};

// the read-backs of the neighbours whose chunk a later chunk of the same pass overwrote (lazy passes with more
// neighbours than free slots)
struct SearchKept {
  std::vector<int32_t> asg0, asgrep;
  std::vector<double> loadrep, ybest;
};

}  // namespace

// the neighbour's point as nep_leaf_eval_ex verifies a placement's: the round-0 repair, the device round's repair from
// its loads, the cheaper of the two
static void search_verify(const LeafInstance &in, const uint8_t *c_open, double nsum, const int32_t *asg0,
                          const int32_t *asgrep, const double *loadrep, LeafPoint &pt) {
  pt = LeafPoint();
  leaf_repair(in, c_open, nsum, asg0, pt);
  if (!asgrep) return;
  LeafPoint alt;
  leaf_repair(in, c_open, nsum, asgrep, alt, loadrep);
  if (alt.found && (!pt.found || alt.obj < pt.obj)) pt = std::move(alt);
}

extern "C" {

int nep_leaf_search(void *model, const double *z0, const nep_leaf_search_opts *opts, double *z_out, double *upper,
                    double *lower, double *prices_out, double *start_upper, int32_t *passes, int64_t *evaluated,
                    int64_t *verified, int32_t *n_accepted, int32_t *kind, int32_t *fn, int32_t *node, int32_t *src,
                    double *delta, double *acc_upper) {
  if (!model || !z0 || !opts || !z_out || !upper || !lower || !start_upper || !passes || !evaluated || !verified ||
      !n_accepted)
    return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (m.step2 || m.fac) return fail(NEP_ERR_ARG, kLeafRefusal);
  const int rounds = opts->rounds <= 0 ? 32 : opts->rounds, every = opts->repair_every;
  const int width = opts->width, nswaps = opts->swaps, per_fn = opts->per_fn, max_passes = opts->max_passes;
  const bool lazy = opts->verify == 1, warm = opts->warm != 0;
  if (every < 0) return fail(NEP_ERR_ARG, "repair_every must be >= 0");
  if (width < 0) return fail(NEP_ERR_ARG, "width must be >= 0");
  if (nswaps < 0) return fail(NEP_ERR_ARG, "swaps must be >= 0");
  if (per_fn < 1 || per_fn > kLeafSwapPerFn)
    return fail(NEP_ERR_ARG, "per_fn must be 1 .. " + std::to_string(kLeafSwapPerFn));
  if (max_passes < 0) return fail(NEP_ERR_ARG, "max_passes must be >= 0");
  if (opts->verify != 0 && opts->verify != 1) return fail(NEP_ERR_ARG, "verify must be 0 (all) or 1 (lazy)");
  if (lazy && every < 1)
    return fail(NEP_ERR_ARG, "verify = 1 (lazy) needs the device objectives of repair_every >= 1");
  if (max_passes > 0 && (!kind || !fn || !node || !src || !delta || !acc_upper))
    return fail(NEP_ERR_ARG, "null argument");
  int rc = leaf_check_lds(m, "nep_leaf_search", leaf_moves_lds);
  if (rc) return rc;
  const size_t N = m.N, F = m.F, R = m.R, ni = m.il.n_int;
  for (size_t k = 0; k < ni; ++k)
    if (z0[k] != 0.0 && z0[k] != 1.0)
      return fail(NEP_ERR_ARG, "placement 0: entry " + std::to_string(k) + " is not 0 or 1 (a leaf fixes every c and n)");

  // the start: nep_leaf_eval_ex's cold evaluation without a cutoff; it leaves z0 in slot 0 with its best prices
  std::vector<double> z(z0, z0 + ni), prices(N, 0.0);
  double up = INF, lo = INF;
  {
    const nep_leaf_opts o{rounds, INF, 0.0};
    const nep_leaf_heur_opts h{every, 0};
    int32_t status = 0;
    if ((rc = nep_leaf_eval_ex(model, 1, z0, &o, every ? &h : nullptr, nullptr, &lo, &up, &status, prices.data(),
                               nullptr, nullptr, nullptr, nullptr)))
      return rc;
  }
  if ((rc = ensure_leaf_search(m))) return rc;
  if ((rc = ensure_leaf_moves(m))) return rc;
  if (nswaps > 0 && (rc = ensure_leaf_swaps(m))) return rc;
  Model::LeafWork &w = *m.leaf;
  if (w.cap < 2)
    return fail(NEP_ERR_ARG, "nep_leaf_search: the evaluator's workspace holds one placement of this model (it needs "
                             "the current one and a neighbour)");
  const size_t free_slots = (size_t)w.cap - 1;
  const LeafInstance in = leaf_instance(m);
  const LeafLimits lim = leaf_limits(m);
  LeafPoint cur = w.points.empty() ? LeafPoint() : std::move(w.points[0]);
  *start_upper = up;
  *passes = 0;
  *evaluated = 0;
  *verified = 0;
  *n_accepted = 0;

  LeafSearchBase base;
  {
    std::vector<uint8_t> c_open(F * N);
    double nsum = 0.0;
    leaf_binary(m, z.data(), c_open.data(), &nsum);
    base.set(m.F, m.N, c_open.data(), m.has_n ? z.data() + m.il.on : nullptr);
  }
  const LeafView bv = [&] {   // the base's slot; the pricing kernels read its best prices
    LeafView v = leaf_view_at(w.v, 0, 1);
    v.y = w.v.ybest;
    return v;
  }();
  const double cn = m.has_n ? m.cost_n : 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  SearchPass ps;
  SearchKept kept;
  std::vector<LeafMove> mvl;
  std::vector<LeafSwap> sw;
  std::vector<int> todo, order;
  std::vector<uint8_t> nb(F * N);
  std::vector<double> acc_prices(N);
  int npass = 0, nacc = 0;

  while (npass < max_passes && std::isfinite(lo)) {
    if (opts->time_limit > 0.0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= opts->time_limit)
      break;
    // the pass's moves at the base's best prices: nep_leaf_moves' table and host composition, nep_leaf_swaps' records
    ps.mv.clear();
    ps.delta.clear();
    if (width > 0) {
      HIPCHK(launch_leaf_moves(bv, w.threads, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_table, bv.share, F * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipStreamSynchronize(m.aux));
      leaf_move_list(in, lim, base.open.data(), w.h_table, width, mvl);
      for (const LeafMove &q : mvl) {
        ps.mv.push_back(base.record(q.kind, q.fn, q.node, -1));
        ps.delta.push_back(q.delta);
      }
    }
    if (nswaps > 0) {
      LeafSwapView sv = w.sv;
      sv.per_fn = per_fn;
      sv.best = nullptr;
      sv.best_from = nullptr;
      HIPCHK(launch_leaf_node_state(bv, sv.fmem, w.d_over, const_cast<int32_t *>(sv.ncnt),
                                    const_cast<double *>(sv.mem), m.aux));
      HIPCHK(launch_leaf_swaps(bv, sv, w.threads, m.aux));
      HIPCHK(hipMemcpyAsync(w.h_rec, sv.rec, F * per_fn * sizeof(LeafSwapRec), hipMemcpyDeviceToHost, m.aux));
      HIPCHK(hipStreamSynchronize(m.aux));
      sw.clear();
      for (size_t k = 0; k < F * per_fn; ++k) {
        const LeafSwapRec &r = w.h_rec[k];
        if (r.to >= 0) sw.push_back(LeafSwap{(int32_t)(k / per_fn), r.from, r.to, r.delta});
      }
      leaf_swap_merge(sw, nswaps);
      for (const LeafSwap &q : sw) {
        if (!base.in_range(3, q.fn, q.to, q.from)) return fail(NEP_ERR_STATE, "nep_leaf_search: a swap out of range");
        ps.mv.push_back(base.record(3, q.fn, q.to, q.from));
        ps.delta.push_back(q.delta);
      }
    }
    const size_t K = ps.mv.size();
    if (K == 0) break;
    ++npass;
    *evaluated += (int64_t)K;
    ps.reset(K);
    todo.clear();
    for (size_t q = 0; q < K; ++q)
      if (!base.rejects(lim, ps.mv[q])) todo.push_back((int)q);
    const int nchunks = (int)((todo.size() + free_slots - 1) / free_slots);
    if (lazy && nchunks > 1) {
      kept.asg0.resize(K * R); kept.asgrep.resize(K * R);
      kept.loadrep.resize(K * N); kept.ybest.resize(K * N);
    }
    // mode 0's running choice: the lowest-index minimum of the verified uppers (a start without a point: the first)
    int sel = -1;
    LeafPoint sel_pt;
    for (int ch = 0; ch < nchunks; ++ch) {
      const size_t c0 = (size_t)ch * free_slots;
      const int B = (int)std::min(free_slots, todo.size() - c0);
      const bool last = ch + 1 == nchunks;
      for (int q = 0; q < B; ++q) {
        const int t = todo[c0 + q];
        w.h_mv[q] = ps.mv[t];
        ps.slot[t] = 1 + q;
        ps.chunk[t] = ch;
      }
      const LeafView nv = leaf_view_at(w.v, 1, B);
      const LeafHeurView hv = every ? leaf_heur_view_at(w.hv, w.v, 1, rounds, every) : LeafHeurView{};
      const LeafSearchView xs{warm ? 1 : 0, cn, up, w.d_mv, bv.open, w.v.ybest};
      HIPCHK(hipMemcpyAsync(w.d_mv, w.h_mv, B * sizeof(LeafSearchMove), hipMemcpyHostToDevice, m.aux));
      HIPCHK(launch_leaf_search_expand(nv, xs, m.aux));
      HIPCHK(launch_leaf_rounds(nv, rounds, w.threads, m.aux, every ? &hv : nullptr));
      // the read-out: 48 bytes a neighbour on a lazy pass; what nep_leaf_eval_ex reads where every neighbour is
      // verified, or where a later chunk will overwrite these slots
      const bool bulk = !lazy || !last;
      HIPCHK(hipMemcpyAsync(w.h_ctrl + 1, nv.ctrl, B * sizeof(LeafCtrl), hipMemcpyDeviceToHost, m.aux));
      if (every) HIPCHK(hipMemcpyAsync(w.h_best + 1, hv.best, B * sizeof(LeafHeurBest), hipMemcpyDeviceToHost, m.aux));
      if (bulk) {
        HIPCHK(hipMemcpyAsync(w.h_y + N, nv.ybest, B * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
        HIPCHK(hipMemcpyAsync(w.h_asg0 + R, nv.asg0, B * R * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
        if (every) {
          HIPCHK(hipMemcpyAsync(w.h_loadrep + N, hv.loadrep, B * N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
          HIPCHK(hipMemcpyAsync(w.h_asgrep + R, hv.asgrep, B * R * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
        }
      }
      HIPCHK(hipStreamSynchronize(m.aux));
      for (int q = 0; q < B; ++q) {
        const int t = todo[c0 + q];
        const size_t s = 1 + (size_t)q;
        const LeafCtrl &c = w.h_ctrl[s];
        ps.lower[t] = c.best;
        ps.live[t] = c.cut ? 0 : 1;
        if (every) ps.dq[t] = w.h_best[s].obj;
        if (c.cut) continue;
        if (lazy) {
          if (!last) {
            std::memcpy(&kept.asg0[t * R], w.h_asg0 + s * R, R * sizeof(int32_t));
            std::memcpy(&kept.asgrep[t * R], w.h_asgrep + s * R, R * sizeof(int32_t));
            std::memcpy(&kept.loadrep[t * N], w.h_loadrep + s * N, N * sizeof(double));
            std::memcpy(&kept.ybest[t * N], w.h_y + s * N, N * sizeof(double));
          }
          continue;
        }
        ++*verified;
        LeafPoint pt;
        base.neighbour(ps.mv[t], nb.data());
        const bool rep = every && w.h_best[s].round >= 0;
        search_verify(in, nb.data(), m.has_n ? (double)ps.mv[t].nopen : 0.0, w.h_asg0 + s * R,
                      rep ? w.h_asgrep + s * R : nullptr, rep ? w.h_loadrep + s * N : nullptr, pt);
        if (!pt.found) continue;
        if (sel < 0 ? true : std::isfinite(up) && pt.obj < sel_pt.obj) {
          sel = t;
          sel_pt = std::move(pt);
          std::memcpy(acc_prices.data(), w.h_y + s * N, N * sizeof(double));
        }
      }
    }
    if (lazy) {
      // the candidates in ascending (device objective, index); the first whose verified point improves is taken
      leaf_search_order(ps.dq, ps.live, up, order);
      for (const int t : order) {
        const size_t s = (size_t)ps.slot[t];
        const int32_t *asg0, *asgrep;
        const double *loadrep;
        const bool here = ps.chunk[t] + 1 == nchunks;
        if (here) {   // still in its slot: this neighbour's assignments and loads cross now
          HIPCHK(hipMemcpyAsync(w.h_asg0 + s * R, w.v.asg0 + s * R, R * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
          HIPCHK(hipMemcpyAsync(w.h_asgrep + s * R, w.hv.asgrep + s * R, R * sizeof(int32_t), hipMemcpyDeviceToHost,
                                m.aux));
          HIPCHK(hipMemcpyAsync(w.h_loadrep + s * N, w.hv.loadrep + s * N, N * sizeof(double), hipMemcpyDeviceToHost,
                                m.aux));
          HIPCHK(hipStreamSynchronize(m.aux));
          asg0 = w.h_asg0 + s * R; asgrep = w.h_asgrep + s * R; loadrep = w.h_loadrep + s * N;
        } else {
          asg0 = &kept.asg0[t * R]; asgrep = &kept.asgrep[t * R]; loadrep = &kept.loadrep[t * N];
        }
        ++*verified;
        LeafPoint pt;
        base.neighbour(ps.mv[t], nb.data());
        search_verify(in, nb.data(), m.has_n ? (double)ps.mv[t].nopen : 0.0, asg0, asgrep, loadrep, pt);
        if (!pt.found || (std::isfinite(up) && !leaf_search_improves(pt.obj, up))) continue;
        sel = t;
        sel_pt = std::move(pt);
        if (here) {
          HIPCHK(hipMemcpyAsync(w.h_y + s * N, w.v.ybest + s * N, N * sizeof(double), hipMemcpyDeviceToHost, m.aux));
          HIPCHK(hipStreamSynchronize(m.aux));
          std::memcpy(acc_prices.data(), w.h_y + s * N, N * sizeof(double));
        } else {
          std::memcpy(acc_prices.data(), &kept.ybest[t * N], N * sizeof(double));
        }
        break;
      }
    } else if (sel >= 0 && std::isfinite(up) && !leaf_search_improves(sel_pt.obj, up)) {
      sel = -1;
    }
    if (sel < 0) break;
    // the accepted neighbour becomes the base, on the device and in the host's copy
    const LeafSearchMove &a = ps.mv[sel];
    int from = ps.slot[sel];
    if (ps.chunk[sel] + 1 != nchunks) {   // a later chunk took its slot: expanded once more, its prices from the host
      const LeafView nv = leaf_view_at(w.v, 1, 1);
      const LeafSearchView xs{0, cn, up, w.d_mv, bv.open, w.v.ybest};
      w.h_mv[0] = a;
      std::memcpy(w.h_y + N, acc_prices.data(), N * sizeof(double));
      HIPCHK(hipMemcpyAsync(w.d_mv, w.h_mv, sizeof(LeafSearchMove), hipMemcpyHostToDevice, m.aux));
      HIPCHK(launch_leaf_search_expand(nv, xs, m.aux));
      HIPCHK(hipMemcpyAsync(nv.ybest, w.h_y + N, N * sizeof(double), hipMemcpyHostToDevice, m.aux));
      from = 1;
    }
    HIPCHK(launch_leaf_search_adopt(w.v, from, m.aux));
    HIPCHK(hipStreamSynchronize(m.aux));
    kind[nacc] = a.kind;
    fn[nacc] = a.fn;
    node[nacc] = a.node;
    src[nacc] = a.src;
    delta[nacc] = ps.delta[sel];
    up = sel_pt.obj;
    lo = ps.lower[sel];
    acc_upper[nacc] = up;
    ++nacc;
    leaf_apply_move(m.F, m.N, m.has_n, z.data(), a.kind, a.fn, a.node, a.src, z.data());
    base.accept(a);
    cur = std::move(sel_pt);
    prices = acc_prices;
  }
  // the end placement's host-verified routing is nep_leaf_routing_entries' placement 0
  w.points.assign(1, LeafPoint());
  w.points[0] = std::move(cur);
  std::memcpy(z_out, z.data(), ni * sizeof(double));
  *upper = up;
  *lower = lo;
  if (prices_out) std::memcpy(prices_out, prices.data(), N * sizeof(double));
  *passes = npass;
  *n_accepted = nacc;
  return NEP_OK;
}

}  // extern "C"
