// nep_presolve.cpp — the per-node presolve of the NEPTUNE LP engine's host runtime (nep_lp_submit presolves every
// node on the host before it reaches the device).
#include "nep_model.h"

namespace nep {

// Node presolve: bounds, the C8 cap, n_ub = 0 => c_ub[:, j] = 0, destination masks, and a
// row-activity test over the node's box: the activity range of each dualised row, from the small
// variables' bounds and the x part's range (flow into (f, j) is in [0, ftot_f] when j is allowed for
// f, else 0; the CPU and score rows have non-negative x coefficients).  A row whose range misses
// [lo, hi] proves the node LP infeasible — e.g. step-2 delete mode with more fixed placements than
// the old allocation (constraints_step2.py:36-44), memory over-committed by fixed placements
// (constraints_step1.py:18-23), an open node with every placement closed (:69-78).
//
// presolve_full() evaluates all of it from scratch; it runs once per model on the natural bounds
// (the "base" box).  presolve_node() evaluates a node as a sparse change of that base: node bounds
// only tighten the base box, so a base-infeasible model makes every node infeasible, rows no
// changed variable touches keep their (feasible) base range, and the rows a change touches are
// re-tested from base range + delta (CSC of the non-x part of K).  Cost per node: one O(n_int) scan
// of the caller's bounds + O(changes x column length), instead of O(n_int + nnz(K) + F*N).
static void activity_ranges(const Model &m, const std::vector<double> &lb, const std::vector<double> &ub,
                            const std::vector<uint8_t> &mask, std::vector<double> &amin, std::vector<double> &amax) {
  const int N = m.N, F = m.F, NP = m.NP, o = m.dl.n_dual;
  amin.assign(o, 0.0);
  amax.assign(o, 0.0);
  for (int f = 0; f < F && m.dl.o1 >= 0; ++f)   // (C1/C2: not in the facility relaxation)
    for (int j = 0; j < N; ++j) {
      const double fx = mask[(size_t)f * NP + j] ? m.ftot[f] : 0.0;
      amax[m.dl.o1 + f * N + j] += fx;
      amax[m.dl.o2 + f * N + j] += fx;
    }
  for (int j = 0; j < N; ++j) {
    amax[m.dl.o5 + j] = INF;
    if (!m.x_coef_nonneg) amin[m.dl.o5 + j] = -INF;
  }
  if (m.step2) {
    amax[m.dl.oS] = INF;
    if (!m.x_coef_nonneg) amin[m.dl.oS] = -INF;
  }
  for (size_t e = 0; e < m.Kv.size(); ++e) {
    const double a = m.Kv[e] * lb[m.Kc[e]], b = m.Kv[e] * ub[m.Kc[e]];
    amin[m.Kr[e]] += std::min(a, b);
    amax[m.Kr[e]] += std::max(a, b);
  }
}

static inline bool row_range_ok(const Model &m, int k, double amin, double amax) {
  if (amin > m.hi[k] + 1e-9 * std::max(1.0, std::fabs(m.hi[k]))) return false;
  if (amax < m.lo[k] - 1e-9 * std::max(1.0, std::fabs(m.lo[k]))) return false;
  return true;
}

// the step-2 score / delay row's smallest activity over the routing simplexes: sum_r wsc[r] min over
// the allowed destinations j of f_r of D[src_r, j] (allow: [F][ld] nonzero = allowed)
static double score_row_xmin(const Model &m, const uint8_t *allow, int ld) {
  const int N = m.N;
  double xmin = 0.0;
  for (int r = 0; r < m.R; ++r) {
    const double w = m.row_wsc_d[r];   // fp64: a proof of infeasibility must not rest on fp32 rounding
    if (w == 0.0) continue;
    const double *Dr = &m.Dh[(size_t)m.row_src[r] * N];
    const uint8_t *al = allow + (size_t)m.row_f[r] * ld;
    double mn = INF;
    for (int j = 0; j < N; ++j)
      if (al[j]) mn = std::min(mn, Dr[j]);
    if (mn < INF) xmin += w * mn;
  }
  return xmin;
}

// CPU cover test over a box's allowed placements allow[f * ld + j] (c[f, j] not fixed to 0): every routing
// row of f sends its whole workload W[f, i] to allowed destinations (C4, constraints_step1.py:27-34), each
// unit costing cpr[f, j] cores at j (C5, :57-65), so (a) sum_f wsum_f min_{j allowed} cpr[f, j] cannot exceed
// the cores of the nodes any loaded function may use, and (b) a function with ONE allowed destination puts
// all of wsum_f cpr[f, j] on that node.  Either failing proves the box infeasible — e.g. a rounding leaf
// that opens too few nodes, whose LP PDHG can only stall on (a residual stuck at the overload).  Only for
// non-negative CPU coefficients (the generator's and the reference's inputs).
static bool cpu_cover_ok(const Model &m, const uint8_t *allow, int ld) {
  if (!m.x_coef_nonneg) return true;
  const int N = m.N, F = m.F;
  std::vector<uint8_t> usable(N, 0);
  std::vector<double> forced(N, 0.0);
  double demand = 0.0;
  for (int f = 0; f < F; ++f) {
    if (m.wsum[f] <= 0.0) continue;
    const uint8_t *al = allow + (size_t)f * ld;
    double mc = INF;
    int cnt = 0, only = -1;
    for (int j = 0; j < N; ++j)
      if (al[j]) {
        mc = std::min(mc, m.cprh[(size_t)f * N + j]);
        usable[j] = 1;
        ++cnt;
        only = j;
      }
    if (cnt == 0) return false;
    demand += m.wsum[f] * mc;
    if (cnt == 1) forced[only] += m.wsum[f] * m.cprh[(size_t)f * N + only];
  }
  double cap = 0.0;
  for (int j = 0; j < N; ++j) {
    const double cores = m.capn[N + j];
    if (forced[j] > cores + 1e-6 * std::max(1.0, cores)) return false;
    if (usable[j]) cap += cores;
  }
  return demand <= cap + 1e-6 * std::max(1.0, cap);
}

bool presolve_full(const Model &m, const double *lbi, const double *ubi, std::vector<double> &lb,
                   std::vector<double> &ub, std::vector<uint8_t> &mask) {
  const int n = m.il.n_int, N = m.N, F = m.F, NP = m.NP;
  lb = m.nat_lb;
  ub = m.nat_ub;
  if (lbi)
    for (int k = 0; k < n; ++k) lb[k] = std::max(lb[k], lbi[k]);
  if (ubi)
    for (int k = 0; k < n; ++k) ub[k] = std::min(ub[k], ubi[k]);
  if (m.step2)   // (see presolve_node: c within the box its moved_from / moved_to bounds imply)
    for (int k = 0; k < F * N; ++k) {
      const double old = -m.lo[m.dl.oD1 + k];
      ub[m.il.oc + k] = std::min(ub[m.il.oc + k], old + ub[m.il.omf + k]);
      lb[m.il.oc + k] = std::max(lb[m.il.oc + k], old - ub[m.il.omt + k]);
    }
  bool ok = true;
  if (m.has_n)
    for (int j = 0; j < N; ++j)
      if (ub[m.il.on + j] <= 0.0)
        for (int f = 0; f < F; ++f) ub[m.il.oc + f * N + j] = std::min(ub[m.il.oc + f * N + j], 0.0);
  for (int k = 0; k < n; ++k)
    if (lb[k] > ub[k] + 1e-12) ok = false;
  mask.assign((size_t)F * NP, 0);
  for (int f = 0; f < F; ++f) {
    int cnt = 0;
    for (int j = 0; j < N; ++j) {
      const bool a = ub[m.il.oc + f * N + j] > 0.0;
      mask[(size_t)f * NP + j] = a;
      cnt += a;
    }
    if (cnt == 0) ok = false;   // every routing row of f would be empty (C4 infeasible)
  }
  if (!ok) return false;
  std::vector<double> amin, amax;
  activity_ranges(m, lb, ub, mask, amin, amax);
  if (m.score_x) amin[m.dl.oS] += score_row_xmin(m, mask.data(), NP);   // (see presolve_node)
  for (int k = 0; k < m.dl.n_dual; ++k)
    if (!row_range_ok(m, k, amin[k], amax[k])) return false;
  return cpu_cover_ok(m, mask.data(), NP);
}

static void init_scratch(const Model &m, PresolveScratch &s) {
  s.pos.assign(m.il.n_int, -1);
  s.dmin.assign(m.dl.n_dual, 0.0);
  s.dmax.assign(m.dl.n_dual, 0.0);
  s.rowmark.assign(m.dl.n_dual, 0);
  s.fdelta.assign(m.F, 0);
  s.allow.assign((size_t)m.F * m.N, 0);
}

// once per model: the base box (natural bounds) and what presolve_node() needs
void presolve_setup(Model &m) {
  const int n = m.il.n_int, F = m.F, NP = m.NP;
  m.base_ok = presolve_full(m, nullptr, nullptr, m.base_lb, m.base_ub, m.base_mask);
  activity_ranges(m, m.base_lb, m.base_ub, m.base_mask, m.base_amin, m.base_amax);
  m.base_cnt.assign(F, 0);
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < m.N; ++j) m.base_cnt[f] += m.base_mask[(size_t)f * NP + j];
  m.Kcp.assign(n + 1, 0);
  for (int c : m.Kc) m.Kcp[c + 1]++;
  for (int k = 0; k < n; ++k) m.Kcp[k + 1] += m.Kcp[k];
  m.Kcr.resize(m.Kc.size());
  m.Kcv.resize(m.Kc.size());
  std::vector<int> fill(m.Kcp.begin(), m.Kcp.end() - 1);
  for (size_t e = 0; e < m.Kc.size(); ++e) {
    const int at = fill[m.Kc[e]]++;
    m.Kcr[at] = m.Kr[e];
    m.Kcv[at] = m.Kv[e];
  }
  m.psc.resize(1);
  init_scratch(m, m.psc[0]);
}

// One node as changes (index, lb, ub) of the base box, appended to ci/cl/cu.  Returns false (and
// appends nothing) if the node is infeasible.
static bool presolve_node(const Model &m, PresolveScratch &sc, const double *lbi, const double *ubi, std::vector<int32_t> &ci,
                   std::vector<double> &cl, std::vector<double> &cu) {
  const int n = m.il.n_int, N = m.N, F = m.F, NP = m.NP, oc = m.il.oc;
  if (!m.base_ok) return false;
  const size_t c0 = ci.size();
  for (int k = 0; k < n; ++k) {
    const double l = lbi ? std::max(m.base_lb[k], lbi[k]) : m.base_lb[k];
    const double u = ubi ? std::min(m.base_ub[k], ubi[k]) : m.base_ub[k];
    if (l != m.base_lb[k] || u != m.base_ub[k]) {
      sc.pos[k] = (int)(ci.size() - c0);
      ci.push_back(k);
      cl.push_back(l);
      cu.push_back(u);
    }
  }
  if (m.step2) {
    // bound propagation through the disruption rows D1 / D2 (constraints_step2.py:5-16): mf - c >= -old and
    // mt + c >= old give c <= old + ub(mf) and c >= old - ub(mt).  A node that fixes moved_from = 0 where
    // old = 0 closes the placement — so its routing column is masked, instead of PDHG having to find that its
    // flow must be 0 through the 1/M-priced big-M row (payload.json step 2: 1.4 units of flow left on such a
    // column after 200k iterations)
    const size_t nc = ci.size();
    for (size_t t = c0; t < nc; ++t) {
      const int k = ci[t];
      const bool isf = k >= m.il.omf && k < m.il.omf + F * N, ist = k >= m.il.omt && k < m.il.omt + F * N;
      if (!isf && !ist) continue;
      const int q = k - (isf ? m.il.omf : m.il.omt);
      const double old = -m.lo[m.dl.oD1 + q];
      const int kc = oc + q;
      double nl = -INF, nu = INF;
      if (isf) nu = old + cu[t];
      else nl = old - cu[t];
      if (sc.pos[kc] >= 0) {
        const size_t pc = c0 + sc.pos[kc];
        cu[pc] = std::min(cu[pc], nu);
        cl[pc] = std::max(cl[pc], nl);
      } else if (nu < m.base_ub[kc] || nl > m.base_lb[kc]) {
        sc.pos[kc] = (int)(ci.size() - c0);
        ci.push_back(kc);
        cl.push_back(std::max(m.base_lb[kc], nl));
        cu.push_back(std::min(m.base_ub[kc], nu));
      }
    }
  }
  if (m.has_n) {
    const size_t nc = ci.size();
    for (size_t t = c0; t < nc; ++t) {
      const int k = ci[t];
      if (k < m.il.on || k >= m.il.on + N || cu[t] > 0.0) continue;
      const int j = k - m.il.on;
      for (int f = 0; f < F; ++f) {
        const int kc = oc + f * N + j;
        if (sc.pos[kc] >= 0) {
          double &u = cu[c0 + sc.pos[kc]];
          u = std::min(u, 0.0);
        } else if (m.base_ub[kc] > 0.0) {
          sc.pos[kc] = (int)(ci.size() - c0);
          ci.push_back(kc);
          cl.push_back(m.base_lb[kc]);
          cu.push_back(0.0);
        }
      }
    }
  }
  bool ok = true;
  std::vector<int> &touched = sc.touched, &ftouched = sc.ftouched;
  touched.clear();
  ftouched.clear();
  // a node that changes many variables (a rounding leaf fixes every c and n) re-tests every row instead of
  // tracking the touched ones: the bookkeeping costs more than the test
  const bool dense = (ci.size() - c0) * 8 > (size_t)m.dl.n_dual;
  auto touch = [&](int r) {
    if (!dense && !sc.rowmark[r]) { sc.rowmark[r] = 1; touched.push_back(r); }
  };
  {
    // (raw pointers: the loop streams the CSC of K, ~7 row updates per change)
    const int *Kcp = m.Kcp.data(), *Kcr = m.Kcr.data();
    const double *Kcv = m.Kcv.data(), *blo = m.base_lb.data(), *bup = m.base_ub.data(), *ftot = m.ftot.data();
    const uint8_t *bmask = m.base_mask.data();
    double *dmin = sc.dmin.data(), *dmax = sc.dmax.data();
    int *fdelta = sc.fdelta.data();
    const int32_t *cip = ci.data();
    const double *clp = cl.data(), *cup = cu.data();
    const int o1 = m.dl.o1, o2 = m.dl.o2, FN = F * N;
    const size_t nchg = ci.size();
    for (size_t t = c0; t < nchg; ++t) {
      const int k = cip[t];
      const double l = clp[t], u = cup[t];
      if (l > u + 1e-12) ok = false;
      if (k >= oc && k < oc + FN) {
        const int q = k - oc, f = q / N, j = q - f * N;
        const int now = u > 0.0, was = bmask[(size_t)f * NP + j];
        if (now != was) {
          if (fdelta[f] == 0) ftouched.push_back(f);
          fdelta[f] += now - was;
          if (o1 >= 0) {   // (C1/C2: not in the facility relaxation)
            const double dfx = (now - was) * ftot[f];
            touch(o1 + q);
            touch(o2 + q);
            dmax[o1 + q] += dfx;
            dmax[o2 + q] += dfx;
          }
        }
      }
      const double bl = blo[k], bu = bup[k];
      for (int e = Kcp[k]; e < Kcp[k + 1]; ++e) {
        const int r = Kcr[e];
        const double a = Kcv[e];
        touch(r);
        dmin[r] += std::min(a * l, a * u) - std::min(a * bl, a * bu);
        dmax[r] += std::max(a * l, a * u) - std::max(a * bl, a * bu);
      }
    }
  }
  const bool cover = ok && !ftouched.empty();
  if (cover || (ok && m.score_x)) {
    // the node's allowed placements: the base mask with the node's c changes over it
    for (int f = 0; f < F; ++f)
      std::memcpy(&sc.allow[(size_t)f * N], &m.base_mask[(size_t)f * NP], (size_t)N);
    for (size_t t = c0; t < ci.size(); ++t) {
      const int k = ci[t];
      if (k >= oc && k < oc + F * N) sc.allow[k - oc] = cu[t] > 0.0;
    }
  }
  // the CPU cover test (cpu_cover_ok) over the node's allowed placements; a box that closes no placement
  // has the base box's (tested in presolve_full)
  if (cover) ok = cpu_cover_ok(m, sc.allow.data(), N);
  if (ok && m.score_x) {
    // The score / delay row (constraints_step2.py:57-88) over x: every routing row carries mass 1 on its
    // allowed destinations, so its activity is at least sum_r wsc[r] min_{j allowed} D[src_r, j].  Closed
    // placements can push that above the right-hand side (e.g. a step-1 delay of 0 admits only local
    // serving): such a node is infeasible, which PDHG cannot prove (DESIGN.md §4 "Infeasibility").
    const int rs = m.dl.oS;
    touch(rs);
    sc.dmin[rs] += score_row_xmin(m, sc.allow.data(), N);
  }
  for (int f : ftouched) {
    if (m.base_cnt[f] + sc.fdelta[f] == 0) ok = false;   // every routing row of f empty
    sc.fdelta[f] = 0;
  }
  if (dense) {
    for (int r = 0; r < m.dl.n_dual; ++r)
      if (ok && !row_range_ok(m, r, m.base_amin[r] + sc.dmin[r], m.base_amax[r] + sc.dmax[r])) ok = false;
    std::fill(sc.dmin.begin(), sc.dmin.end(), 0.0);
    std::fill(sc.dmax.begin(), sc.dmax.end(), 0.0);
  } else {
    for (int r : touched) {
      if (ok && !row_range_ok(m, r, m.base_amin[r] + sc.dmin[r], m.base_amax[r] + sc.dmax[r])) ok = false;
      sc.dmin[r] = sc.dmax[r] = 0.0;
      sc.rowmark[r] = 0;
    }
  }
  for (size_t t = c0; t < ci.size(); ++t) sc.pos[ci[t]] = -1;
  if (!ok) {
    ci.resize(c0);
    cl.resize(c0);
    cu.resize(c0);
  }
  return ok;
}

// presolve threads for a submit of n nodes: NEP_PRESOLVE_THREADS (default 8, 1 = serial), only for large
// models (below ~8k integer variables a node presolves in tens of microseconds, less than a thread start)
static int presolve_threads(const Model &m, int n) {
  static const int cap = [] {
    const char *e = std::getenv("NEP_PRESOLVE_THREADS");
    const int v = e ? std::atoi(e) : 8;
    const int hw = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(v, hw > 0 ? hw : 1));
  }();
  if (n < 2 || m.il.n_int < 8192) return 1;
  return std::min(cap, n);
}

// Presolve n nodes on the host — over the nodes in parallel when they are large (a rounding leaf at
// 256x128 changes ~33k bounds, ~1 ms of work; presolve_threads) — into box[0 .. n-1].
void presolve_batch(Model &m, int n, const double *lbi, const double *ubi, std::vector<NodeBox> &box) {
  const size_t ni = (size_t)m.il.n_int;
  box.assign(n, NodeBox{});
  auto one = [&](int b, int t) {
    PresolveScratch &sc = m.psc[t];
    NodeBox &nb = box[b];
    const double *L = lbi ? lbi + (size_t)b * ni : nullptr, *U = ubi ? ubi + (size_t)b * ni : nullptr;
    nb.t = t;
    nb.off = sc.ci.size();
    nb.ok = presolve_node(m, sc, L, U, sc.ci, sc.cl, sc.cu);
    nb.cnt = sc.ci.size() - nb.off;
    // the box fixes the objective when the routing carries no cost and every c and n is fixed (a
    // leaf): mf / mt / allocated / deallocated then follow from c at their cheapest (the repair)
    bool ex = nb.ok && m.x_cost_free && !m.fac;
    const int n_fix_end = m.has_n ? m.il.on + m.N : m.il.oc + m.F * m.N;
    for (int k = m.il.oc; ex && k < m.il.oc + m.F * m.N; ++k)
      ex = L && U && std::max(L[k], m.nat_lb[k]) == std::min(U[k], m.nat_ub[k]);
    for (int k = m.has_n ? m.il.on : n_fix_end; ex && k < n_fix_end; ++k)
      ex = L && U && std::max(L[k], m.nat_lb[k]) == std::min(U[k], m.nat_ub[k]);
    nb.ex = ex;
    if (nb.ok && m.dred) {
      // the reduced disruption block needs integral moved_from / moved_to bounds (binaries: every B&B box
      // has them) and a non-empty interval of T = sum c - sum old (dred_interval)
      const IntLayout &il = m.il;
      const int FN = m.F * m.N;
      double la = m.base_lb[il.oa], ua = m.base_ub[il.oa], ld = m.base_lb[il.od], ud = m.base_ub[il.od];
      for (size_t q = nb.off; q < nb.off + nb.cnt; ++q) {
        const int k = sc.ci[q];
        if (k >= il.omf && k < il.omt + FN) {
          if (std::floor(sc.cl[q]) != sc.cl[q] || std::floor(sc.cu[q]) != sc.cu[q]) nb.bad = true;
        } else if (k == il.oa) {
          la = sc.cl[q]; ua = sc.cu[q];
        } else if (k == il.od) {
          ld = sc.cl[q]; ud = sc.cu[q];
        }
      }
      double tlo, thi;
      dred_interval(m.sigma4, la, ua, ld, ud, tlo, thi);
      if (tlo > thi) nb.ok = false;
    }
  };
  const int nt = presolve_threads(m, n);
  while ((int)m.psc.size() < nt) {
    m.psc.emplace_back();
    init_scratch(m, m.psc.back());
  }
  for (int t = 0; t < nt; ++t) {
    m.psc[t].ci.clear();
    m.psc[t].cl.clear();
    m.psc[t].cu.clear();
  }
  if (nt <= 1) {
    for (int b = 0; b < n; ++b) one(b, 0);
  } else {
    std::atomic<int> next{0};
    auto work = [&](int t) {
      for (int b; (b = next.fetch_add(1)) < n;) one(b, t);
    };
    std::vector<std::thread> th;
    try {
      for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
    } catch (const std::system_error &) {   // (fewer threads: this one drains the rest)
    }
    work(0);
    for (auto &t : th) t.join();
  }
}

}  // namespace nep
