// nep_model_build.cpp — the model build of the NEPTUNE LP engine's host runtime: exact zero-workload aggregation,
// coefficients, diagonal scaling, step size (host or device power iteration) and the device set-up of a model.
#include "nep_model.h"

namespace nep {

// slot groups per block unless NEP_BLOCK_GROUPS says otherwise (launch_block; DESIGN.md §6 "Slot groups")
static constexpr int kBlockGroups = 2;

// ---------------------------------------------------------------------------------------------
// model build
// ---------------------------------------------------------------------------------------------
int build(Model &m, const nep_model_desc &d, bool host_power) {
  const int N = d.n_nodes, F = d.n_functions;
  if (N <= 0 || F <= 0) return fail(NEP_ERR_ARG, "n_nodes and n_functions must be positive");
  if (d.variant < 0 || d.variant > 2) return fail(NEP_ERR_ARG, "bad variant");
  if (d.step < 1 || d.step > 3) return fail(NEP_ERR_ARG, "bad step");
  if (!d.delay || !d.workload || !d.core_per_req || !d.function_memory || !d.node_memory || !d.node_cores ||
      !d.node_cost || !d.max_delay)
    return fail(NEP_ERR_ARG, "missing input array");
  if (d.step != NEP_STEP1 && !d.old_allocations) return fail(NEP_ERR_ARG, "step 2 needs old_allocations");
  m.N = N;
  m.F = F;
  m.variant = d.variant;
  m.step = d.step;
  m.step2 = d.step != NEP_STEP1;
  m.has_n = d.variant != NEP_MIN_DELAY;
  if (d.relaxation != NEP_RELAX_REFERENCE && d.relaxation != NEP_RELAX_FACILITY) return fail(NEP_ERR_ARG, "bad relaxation");
  m.fac = d.relaxation == NEP_RELAX_FACILITY;
  if (m.fac && (m.step2 || !m.has_n))
    return fail(NEP_ERR_ARG, "the facility relaxation is a step-1 MinUtilization / MinDelayAndUtilization model");
  m.alpha = d.alpha;
  m.M = d.big_m > 0 ? d.big_m : 1e6;
  m.eps = d.epsilon > 0 ? d.epsilon : 1e-6;
  m.sigma4 = d.step == NEP_STEP2_CREATE ? 1.0 : -1.0;
  m.NP = padded_width(N);
  // the widest rows whose certificate pass still fits a CU's LDS at the smallest tile (x_lds_bytes / fac_lds_bytes,
  // nep_internal.h — the launchers' own formula): a wider model could iterate but never launch a certificate
  if (const int np_max = max_padded_width(m.fac); m.NP > np_max)
    return fail(NEP_ERR_ARG, "n_nodes = " + std::to_string(N) + " not supported by this build: the " +
                                 (m.fac ? "facility" : "reference") + " relaxation's certificate pass holds rows of at most " +
                                 std::to_string(np_max) + " destinations in LDS (largest supported n_nodes: " +
                                 std::to_string(np_max) + ")");
  m.CPL = chunks_per_lane(m.NP);
  m.W.assign(d.workload, d.workload + (size_t)F * N);
  m.cprh.assign(d.core_per_req, d.core_per_req + (size_t)F * N);
  m.wsum.assign(F, 0.0);
  for (int f = 0; f < F; ++f)
    for (int i = 0; i < N; ++i) m.wsum[f] += m.W[(size_t)f * N + i];
  const double *D = d.delay;

  // exact aggregation of zero-workload sources: they enter only the column sums (C1/C2) and their
  // own C4 row, with zero objective / CPU / score coefficients, so one pooled row of weight
  // m_f = #zero sources carries them all (x[i,f,:] = pooled row for every such i).
  for (int f = 0; f < F; ++f) {
    int zeros = 0;
    for (int i = 0; i < N; ++i) {
      const double w = m.W[(size_t)f * N + i];
      if (w != 0.0) {
        m.row_f.push_back(f);
        m.row_src.push_back(i);
        m.row_m.push_back(1.f);
        m.row_w.push_back((float)w);
      } else {
        ++zeros;
      }
    }
    if (zeros > 0) {
      m.row_f.push_back(f);
      m.row_src.push_back(-1);
      m.row_m.push_back((float)zeros);
      m.row_w.push_back(0.f);
    }
  }
  m.R = (int)m.row_f.size();

  // objective / score coefficients (objectives.py:4-52, constraints_step2.py:57-88)
  double sumW = 0.0;
  for (double w : m.W) sumW += w;
  double kobj = 0.0;
  if (!m.step2) {
    if (d.variant == NEP_MIN_DELAY) {
      kobj = 1.0;
    } else if (d.variant == NEP_MIN_DELAY_AND_UTILIZATION && sumW != 0.0) {
      double mwd = 0.0;   // objectives.py:36-43
      for (int f = 0; f < F; ++f)
        for (int i = 0; i < N; ++i) {
          double best = -INF;
          for (int j = 0; j < N; ++j) {
            const double dl = D[(size_t)i * N + j];
            if (dl <= d.max_delay[f]) best = std::max(best, dl);
          }
          if (best == -INF) return fail(NEP_ERR_ARG, "max() of an empty delay set (objectives.py:41)");
          mwd += m.W[(size_t)f * N + i] * best;
        }
      if (mwd == 0.0) return fail(NEP_ERR_ARG, "max_workload_delay == 0: division by zero (objectives.py:50)");
      kobj = (1.0 - d.alpha) / mwd;
    }
    m.cost_n = d.variant == NEP_MIN_UTILIZATION ? 1.0 : d.variant == NEP_MIN_DELAY_AND_UTILIZATION ? d.alpha / N : 0.0;
  }
  m.kobj = kobj;
  double score_rhs = INF;
  std::vector<double> colmaxD(N, -INF);
  for (int k = 0; k < N; ++k)
    for (int i = 0; i < N; ++i) colmaxD[i] = std::max(colmaxD[i], D[(size_t)k * N + i]);
  m.row_wobj.resize(m.R);
  m.row_wsc.resize(m.R);
  m.row_wsc_d.assign(m.R, 0.0);
  for (int r = 0; r < m.R; ++r) {
    m.row_wobj[r] = (float)(kobj * m.row_w[r]);
    double wsc = 0.0;
    if (m.step2 && m.row_src[r] >= 0) {
      const int f = m.row_f[r], i = m.row_src[r];
      const double wd = m.W[(size_t)f * N + i];
      if (d.variant == NEP_MIN_DELAY) wsc = wd;
      else if (d.variant == NEP_MIN_DELAY_AND_UTILIZATION)
        wsc = (1.0 - d.alpha) * wd / std::max(d.max_delay[f], colmaxD[i]);
    }
    m.row_wsc[r] = (float)wsc;
    m.row_wsc_d[r] = wsc;
    if (wsc != 0.0) m.score_x = true;
  }
  // (step-1 reference models keep it too: the fixed-placement evaluator's fp64 delays, nep_leaf_eval)
  if (m.score_x || (!m.step2 && !m.fac)) m.Dh.assign(D, D + (size_t)N * N);
  if (m.step2) {
    if (d.variant == NEP_MIN_DELAY) {
      score_rhs = d.soften_step1_sol * d.prev_network_delay;
      m.score_n_coef = 0.0;
    } else {
      score_rhs = d.max_score * d.soften_step1_sol;
      m.score_n_coef = d.variant == NEP_MIN_UTILIZATION ? 1.0 : d.alpha / N;
    }
  }

  // rows of one function are consecutive: frow[f] .. frow[f+1] (one x-pass workgroup each)
  m.frow.assign(F + 1, 0);
  for (int r = 0; r < m.R; ++r) m.frow[m.row_f[r] + 1] += 1;
  for (int f = 0; f < F; ++f) m.frow[f + 1] += m.frow[f];
  m.rows.resize(m.R);
  for (int r = 0; r < m.R; ++r)
    m.rows[r] = RowInfo{m.row_m[r], m.row_w[r], m.row_wobj[r], m.row_wsc[r], m.row_src[r], m.row_f[r], 0, 0};
  m.JB = (N + kNodeJ - 1) / kNodeJ;   // node-pass workgroups per LP

  // integer-variable layout (variables.py order minus x)
  const int FN = F * N;
  IntLayout &il = m.il;
  il.oc = 0;
  if (!m.step2) {
    il.omf = il.omt = il.oa = il.od = -1;
    il.on = m.has_n ? FN : -1;
    il.n_int = FN + (m.has_n ? N : 0);
  } else {
    il.omf = FN;
    il.omt = 2 * FN;
    il.oa = 3 * FN;
    il.od = 3 * FN + 1;
    il.on = m.has_n ? 3 * FN + 2 : -1;
    il.n_int = 3 * FN + 2 + (m.has_n ? N : 0);
  }
  m.nat_lb.assign(il.n_int, 0.0);
  m.nat_ub.assign(il.n_int, 1.0);
  m.cost_int.assign(il.n_int, 0.0);
  if (m.has_n)
    for (int j = 0; j < N; ++j) {
      // C8 (constraints_step1.py:101-103): cost[j] * n[j] <= budget  ->  bound on n
      if (d.node_cost[j] > 0) m.nat_ub[il.on + j] = std::min(1.0, d.node_budget / d.node_cost[j]);
      else if (d.node_budget < 0) m.nat_ub[il.on + j] = -1.0;   // infeasible budget row
      m.cost_int[il.on + j] = m.cost_n;
    }
  double sum_old = 0.0;
  if (m.step2) {
    m.w_dis = (double)FN;   // objectives.py:56  w = np.ma.size(old)
    for (int k = 0; k < FN; ++k) {
      m.cost_int[il.omf + k] = m.w_dis;
      m.cost_int[il.omt + k] = m.w_dis;
      sum_old += d.old_allocations[k];
    }
    m.cost_int[il.oa] = m.w_dis - 1;
    m.cost_int[il.od] = m.w_dis + 1;
    m.nat_lb[il.oa] = m.nat_lb[il.od] = -(double)FN;
    m.nat_ub[il.oa] = m.nat_ub[il.od] = 0.0;
  }

  // dual layout + row bounds
  DualLayout &dl = m.dl;
  int o = 0;
  dl.o1 = dl.o2 = dl.oQ = -1;
  if (!m.fac) { dl.o1 = o; o += FN; dl.o2 = o; o += FN; }
  dl.o3 = o; o += N;
  dl.o5 = o; o += N;
  dl.o6 = dl.o7 = dl.oD1 = dl.oD2 = dl.oD3a = dl.oD3b = dl.oD4 = dl.oS = -1;
  if (m.fac) { dl.oQ = o; o += FN; }   // c[f, j] - n[j] <= 0
  else if (m.has_n) { dl.o6 = o; o += N; dl.o7 = o; o += N; }
  if (m.step2) {
    dl.oD1 = o; o += FN;
    dl.oD2 = o; o += FN;
    dl.oD3a = o++; dl.oD3b = o++; dl.oD4 = o++; dl.oS = o++;
  }
  dl.n_dual = o;
  m.lo.assign(o, -INF);
  m.hi.assign(o, INF);
  for (int k = 0; k < FN && !m.fac; ++k) {
    m.hi[dl.o1 + k] = 0.0;
    m.lo[dl.o2 + k] = -m.eps;
  }
  for (int k = 0; k < FN && m.fac; ++k) m.hi[dl.oQ + k] = 0.0;
  m.capn.resize(2 * (size_t)N);
  for (int j = 0; j < N; ++j) {
    m.capn[j] = d.node_memory[j];
    m.capn[N + j] = d.node_cores[j];
    // (fac: C3 / C5 carry n[j] on the right, mem c - Mem_j n <= 0 and CPU - cores_j n <= 0)
    m.hi[dl.o3 + j] = m.fac ? 0.0 : d.node_memory[j];
    m.hi[dl.o5 + j] = m.fac ? 0.0 : d.node_cores[j];
    if (m.has_n && !m.fac) { m.hi[dl.o6 + j] = 0.0; m.lo[dl.o7 + j] = -m.eps; }
  }
  if (m.step2) {
    for (int k = 0; k < FN; ++k) {
      m.lo[dl.oD1 + k] = -d.old_allocations[k];
      m.lo[dl.oD2 + k] = d.old_allocations[k];
    }
    m.lo[dl.oD3a] = -sum_old;
    m.lo[dl.oD3b] = sum_old;
    m.lo[dl.oD4] = m.sigma4 * sum_old;
    m.hi[dl.oS] = score_rhs;
  }
  // Step 2, reduced disruption block: with integral moved_from / moved_to bounds the LP optimum
  // has mf = max(lb_mf, c - old), mt = max(lb_mt, old - c) — a linear cost in c per (f, j) — and the rows
  // D3a/D3b/D4 force (create) d = 0, a = -T or (delete) a = 0, d = T for T = sum c - sum old, i.e. a cost
  // sT * T on an interval of T.  The iteration then carries c (and n, x) only; NEP_STEP2_FULL=1 keeps the
  // full rows (A/B).
  if (m.step2) {
    const char *e = std::getenv("NEP_STEP2_FULL");
    m.dred = !(e && std::atoi(e) != 0);
    for (int k = 0; k < FN && m.dred; ++k)   // (mf / mt are linear in c only for a binary old allocation)
      m.dred = d.old_allocations[k] == 0.0 || d.old_allocations[k] == 1.0;
    m.sT = m.sigma4 > 0 ? -(m.w_dis - 1.0) : (m.w_dis + 1.0);
    m.sum_old = sum_old;
  }
  m.mem_f.assign(d.function_memory, d.function_memory + F);
  m.node_cost.assign(d.node_cost, d.node_cost + N);
  m.node_budget = d.node_budget;

  // non-x entries of K (COO) and x-row norms (x columns are never rescaled)
  Coo K;
  std::vector<double> xmax(o, 0.0), xsum(o, 0.0);
  std::vector<double> mmax(F, 0.0), msum(F, 0.0);
  for (int r = 0; r < m.R; ++r) {
    mmax[m.row_f[r]] = std::max(mmax[m.row_f[r]], (double)m.row_m[r]);
    msum[m.row_f[r]] += m.row_m[r];
  }
  const double *cpr = d.core_per_req;
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < N; ++j) {
      const int k = f * N + j;
      if (m.fac) {   // C3 and c[f, j] - n[j] <= 0 (the x <= c rows are structured: rhoL, below)
        K.add(dl.o3 + j, il.oc + k, m.mem_f[f]);
        K.add(dl.oQ + k, il.oc + k, 1.0);
        K.add(dl.oQ + k, il.on + j, -1.0);
        continue;
      }
      K.add(dl.o1 + k, il.oc + k, -m.M);
      K.add(dl.o2 + k, il.oc + k, -1.0);
      K.add(dl.o3 + j, il.oc + k, m.mem_f[f]);
      xmax[dl.o1 + k] = xmax[dl.o2 + k] = mmax[f];
      xsum[dl.o1 + k] = xsum[dl.o2 + k] = msum[f];
      if (m.has_n) {
        K.add(dl.o6 + j, il.oc + k, 1.0);
        K.add(dl.o7 + j, il.oc + k, 1.0);
      }
      if (m.step2) {
        K.add(dl.oD1 + k, il.omf + k, 1.0);
        K.add(dl.oD1 + k, il.oc + k, -1.0);
        K.add(dl.oD2 + k, il.omt + k, 1.0);
        K.add(dl.oD2 + k, il.oc + k, 1.0);
        K.add(dl.oD3a, il.oc + k, -1.0);
        K.add(dl.oD3b, il.oc + k, 1.0);
        K.add(dl.oD4, il.oc + k, m.sigma4);
      }
    }
  if (m.fac)
    for (int j = 0; j < N; ++j) {
      K.add(dl.o3 + j, il.on + j, -m.capn[j]);
      K.add(dl.o5 + j, il.on + j, -m.capn[N + j]);
    }
  if (m.has_n && !m.fac)
    for (int j = 0; j < N; ++j) {
      K.add(dl.o6 + j, il.on + j, -m.M);
      K.add(dl.o7 + j, il.on + j, -1.0);
      if (m.step2 && m.score_n_coef != 0.0) K.add(dl.oS, il.on + j, m.score_n_coef);
    }
  if (m.step2) {
    K.add(dl.oD3a, il.oa, -1.0);
    K.add(dl.oD3b, il.od, -1.0);
    K.add(dl.oD4, il.od, 1.0);
    K.add(dl.oD4, il.oa, 1.0);
  }
  for (int r = 0; r < m.R; ++r) {
    const int f = m.row_f[r], src = m.row_src[r];
    for (int j = 0; j < N; ++j) {
      const double w = (double)m.row_w[r] * cpr[(size_t)f * N + j];
      xmax[dl.o5 + j] = std::max(xmax[dl.o5 + j], std::fabs(w));
      xsum[dl.o5 + j] += std::fabs(w);
      if (m.step2 && src >= 0 && m.row_wsc[r] != 0.f) {
        const double s = std::fabs((double)m.row_wsc[r] * D[(size_t)src * N + j]);
        xmax[dl.oS] = std::max(xmax[dl.oS], s);
        xsum[dl.oS] += s;
      }
    }
  }
  // row norms for the relative residual: max(1, |bounds|, max |coef|)
  m.rownorm.assign(o, 1.0);
  for (int k = 0; k < o; ++k) {
    double rn = std::max(1.0, xmax[k]);
    if (std::isfinite(m.lo[k])) rn = std::max(rn, std::fabs(m.lo[k]));
    if (std::isfinite(m.hi[k])) rn = std::max(rn, std::fabs(m.hi[k]));
    m.rownorm[k] = rn;
  }
  for (size_t e = 0; e < K.v.size(); ++e) m.rownorm[K.r[e]] = std::max(m.rownorm[K.r[e]], std::fabs(K.v[e]));
  m.Kr = K.r;
  m.Kc = K.c;
  m.Kv = K.v;
  for (int r = 0; r < m.R; ++r) m.x_cost_free = m.x_cost_free && m.row_wobj[r] == 0.f;
  m.ftot.assign(F, 0.0);
  for (int r = 0; r < m.R; ++r) m.ftot[m.row_f[r]] += m.row_m[r];
  for (size_t k = 0; k < (size_t)N * N && m.x_coef_nonneg; ++k) m.x_coef_nonneg = D[k] >= 0.0;
  for (size_t k = 0; k < (size_t)F * N && m.x_coef_nonneg; ++k)
    m.x_coef_nonneg = m.W[k] >= 0.0 && !(cpr[k] < 0.0);

  // the matrix the iteration runs on: K itself, or (step 2, reduced disruption block) K without the idle
  // rows D1/D2/D3a/D3b and with D4 as the row sum c (coefficient 1 on every c, no a / d): scaling and step
  // size are those of the reduced LP (presolve keeps the reference rows of K)
  Coo Kred;
  if (m.dred) {
    for (size_t e = 0; e < K.v.size(); ++e) {
      const int r = K.r[e], c = K.c[e];
      if ((r >= dl.oD1 && r < dl.oD1 + FN) || (r >= dl.oD2 && r < dl.oD2 + FN) || r == dl.oD3a || r == dl.oD3b) continue;
      if (r == dl.oD4) {
        if (c >= il.oc && c < il.oc + FN) Kred.add(r, c, 1.0);
        continue;
      }
      Kred.add(r, c, K.v[e]);
    }
  }
  const Coo &KS = m.dred ? Kred : K;
  // Ruiz equilibration (10 sweeps, inf-norm) + Pock-Chambolle (alpha = 1) on rows and the
  // non-x columns; x columns keep scale 1 so every routing row stays a plain simplex.
  // facility relaxation: the rows x[r, j] - c[f, j] <= 0 of every routing row r of f (x entry 1, unscaled;
  // c entry -gam_c): one scale per (f, j), and nrow_f entries in c[f, j]'s column
  std::vector<int> nrow_f(F, 0);
  for (int r = 0; r < m.R; ++r) nrow_f[m.row_f[r]] += 1;
  if (m.fac) m.rhoL.assign(FN, 1.0);
  auto ruiz = [&](const Coo &KK, std::vector<double> &rho, std::vector<double> &gam) {
    rho.assign(o, 1.0);
    gam.assign(il.n_int, 1.0);
    std::vector<double> rnL(m.fac ? FN : 0);
    std::vector<double> rn(o), cn(il.n_int);
    for (int sweep = 0; sweep < 11; ++sweep) {
      const bool pc = sweep == 10;
      for (int k = 0; k < o; ++k) rn[k] = pc ? rho[k] * xsum[k] : rho[k] * xmax[k];
      std::fill(cn.begin(), cn.end(), 0.0);
      for (size_t e = 0; e < KK.v.size(); ++e) {
        const double a = std::fabs(rho[KK.r[e]] * KK.v[e] * gam[KK.c[e]]);
        if (pc) { rn[KK.r[e]] += a; cn[KK.c[e]] += a; }
        else { rn[KK.r[e]] = std::max(rn[KK.r[e]], a); cn[KK.c[e]] = std::max(cn[KK.c[e]], a); }
      }
      for (int k = 0; k < (m.fac ? FN : 0); ++k) {
        const double gc = gam[il.oc + k], a = m.rhoL[k] * gc;
        rnL[k] = pc ? m.rhoL[k] * (1.0 + gc) : m.rhoL[k] * std::max(1.0, gc);
        const int f = k / N;
        if (pc) cn[il.oc + k] += nrow_f[f] * a;
        else cn[il.oc + k] = std::max(cn[il.oc + k], a);
      }
      for (int k = 0; k < o; ++k)
        if (rn[k] > 0) rho[k] /= std::sqrt(rn[k]);
      for (int k = 0; k < (m.fac ? FN : 0); ++k)
        if (rnL[k] > 0) m.rhoL[k] /= std::sqrt(rnL[k]);
      for (int k = 0; k < il.n_int; ++k)
        if (cn[k] > 0) gam[k] /= std::sqrt(cn[k]);
    }
  };
  ruiz(KS, m.rho, m.gam);

  m.Ks = KS;   // (the device power iteration, power_device, runs on it after setup_device)
  // ||K̃||_2 by power iteration on K̃ᵀK̃ (structured x part + COO part); nep_model_create runs the same passes on
  // the device (power_device, nep_build.hip) from the same start vector
  if (host_power) {
    std::vector<double> zx((size_t)m.R * N), zs(il.n_int), yv(o), gx((size_t)m.R * N), gs(il.n_int);
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> nd;
    for (auto &t : zx) t = nd(rng);
    for (auto &t : zs) t = nd(rng);
    double lam = 0.0;
    for (int it = 0; it < 60; ++it) {
      double nrm = 0.0;
      for (double t : zx) nrm += t * t;
      for (double t : zs) nrm += t * t;
      nrm = std::sqrt(nrm);
      for (auto &t : zx) t /= nrm;
      for (auto &t : zs) t /= nrm;
      // y = K̃ z
      std::fill(yv.begin(), yv.end(), 0.0);
      for (int r = 0; r < m.R; ++r) {
        const int f = m.row_f[r], src = m.row_src[r];
        const double mr = m.row_m[r], wr = m.row_w[r], sc = m.row_wsc[r];
        const double *xr = &zx[(size_t)r * N];
        double srow = 0.0;
        for (int j = 0; j < N; ++j) {
          if (!m.fac) {
            yv[dl.o1 + f * N + j] += mr * xr[j];
            yv[dl.o2 + f * N + j] += mr * xr[j];
          }
          yv[dl.o5 + j] += wr * cpr[(size_t)f * N + j] * xr[j];
          if (m.step2 && src >= 0 && sc != 0.0) srow += sc * D[(size_t)src * N + j] * xr[j];
        }
        if (m.step2) yv[dl.oS] += srow;
      }
      for (size_t e = 0; e < KS.v.size(); ++e) yv[KS.r[e]] += KS.v[e] * m.gam[KS.c[e]] * zs[KS.c[e]];
      for (int k = 0; k < o; ++k) yv[k] *= m.rho[k];
      // g = K̃ᵀ y
      for (int k = 0; k < o; ++k) yv[k] *= m.rho[k];   // now ρ y
      for (int r = 0; r < m.R; ++r) {
        const int f = m.row_f[r], src = m.row_src[r];
        const double mr = m.row_m[r], wr = m.row_w[r], sc = m.row_wsc[r];
        double *gr = &gx[(size_t)r * N];
        for (int j = 0; j < N; ++j) {
          double g = wr * cpr[(size_t)f * N + j] * yv[dl.o5 + j];
          if (!m.fac) g += mr * (yv[dl.o1 + f * N + j] + yv[dl.o2 + f * N + j]);
          if (m.step2 && src >= 0 && sc != 0.0) g += sc * D[(size_t)src * N + j] * yv[dl.oS];
          gr[j] = g;
        }
      }
      std::fill(gs.begin(), gs.end(), 0.0);
      if (m.fac)   // the x <= c rows, scaled: t = rhoL (x - gam_c z_c); x gets rhoL t, z_c gets -rhoL t (gam_c: below)
        for (int r = 0; r < m.R; ++r) {
          const int f = m.row_f[r];
          const double *xr = &zx[(size_t)r * N];
          double *gr = &gx[(size_t)r * N];
          for (int j = 0; j < N; ++j) {
            const int k = f * N + j;
            const double t = m.rhoL[k] * (xr[j] - m.gam[il.oc + k] * zs[il.oc + k]);
            gr[j] += m.rhoL[k] * t;
            gs[il.oc + k] -= m.rhoL[k] * t;
          }
        }
      for (size_t e = 0; e < KS.v.size(); ++e) gs[KS.c[e]] += KS.v[e] * yv[KS.r[e]];
      for (int k = 0; k < il.n_int; ++k) gs[k] *= m.gam[k];
      double dot = 0.0;
      for (size_t k = 0; k < zx.size(); ++k) dot += zx[k] * gx[k];
      for (int k = 0; k < il.n_int; ++k) dot += zs[k] * gs[k];
      lam = dot;
      zx.swap(gx);
      zs.swap(gs);
    }
    m.sigma_max = std::sqrt(std::max(lam, 1e-30));
    m.eta = 0.95 / m.sigma_max;
    m.power_host = true;
  }

  // initial primal weight (PDLP): ||c~||_2 / ||b~||_2 in the scaled space.  The NEPTUNE objectives
  // are tiny per unit of flow (e.g. (1-alpha) W D / MWD ~ 1e-4, objectives.py:30-52) while the row
  // bounds are node capacities ~1e2, so the balanced weight is far below 1; starting at 1 costs
  // tens of thousands of iterations before the restarts find it.
  {
    double cn2 = 0.0, bn2 = 0.0;
    for (int r = 0; r < m.R; ++r) {
      const int src = m.row_src[r];
      if (src < 0 || m.row_wobj[r] == 0.f) continue;
      for (int j = 0; j < N; ++j) {
        const double cx = (double)m.row_wobj[r] * D[(size_t)src * N + j];
        cn2 += m.row_m[r] * cx * cx;
      }
    }
    for (int k = 0; k < il.n_int; ++k) {
      double ck = m.cost_int[k];
      if (m.dred) {   // the reduced LP's costs at natural bounds: c carries mf / mt (w, -w) and sT; the rest 0
        ck = 0.0;
        if (k >= il.oc && k < il.oc + FN) ck = (d.old_allocations[k - il.oc] > 0.5 ? -m.w_dis : m.w_dis) + m.sT;
        else if (il.on >= 0 && k >= il.on) ck = m.cost_int[k];
      }
      cn2 += std::pow(m.gam[k] * ck, 2);
    }
    for (int k = 0; k < o; ++k) {
      if (m.dred && ((k >= dl.oD1 && k < dl.oD1 + FN) || (k >= dl.oD2 && k < dl.oD2 + FN) || k == dl.oD3a ||
                     k == dl.oD3b))
        continue;   // (idle rows of the reduced LP)
      double b = 0.0;
      if (std::isfinite(m.lo[k])) b = std::max(b, std::fabs(m.lo[k]));
      if (std::isfinite(m.hi[k])) b = std::max(b, std::fabs(m.hi[k]));
      if (m.fac && k >= dl.o3 && k < dl.o5 + N) b = m.capn[k < dl.o5 ? k - dl.o3 : N + k - dl.o5];   // (hi = 0)
      if (m.dred && k == dl.oD4) {   // the row sum c in [L, U] at the natural allocated / deallocated bounds
        double tlo, thi;
        dred_interval(m.sigma4, m.nat_lb[il.oa], m.nat_ub[il.oa], m.nat_lb[il.od], m.nat_ub[il.od], tlo, thi);
        b = std::max(std::fabs(m.sum_old + tlo), std::fabs(m.sum_old + thi));
      }
      bn2 += std::pow(m.rho[k] * b, 2);
    }
    m.omega0 = (cn2 > 0.0 && bn2 > 0.0) ? std::sqrt(cn2) / std::sqrt(bn2) : 1.0;
  }
  return NEP_OK;
}

int setup_device(Model &m, int max_batch, void *stream) {
  m.max_batch = max_batch;
  m.busy.assign(max_batch, 0);
  m.rc_stale.assign(max_batch, 0);
  if (stream) {
    m.stream = (hipStream_t)stream;
  } else {
    HIPCHK(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    m.own_stream = true;
  }
  HIPCHK(hipEventCreate(&m.ev0));
  HIPCHK(hipEventCreate(&m.ev1));
  // the auxiliary stream (host reads of finished slots, warm-start copies, submits) at the highest priority:
  // its small kernels and copies are dispatched between the workgroups of the block in flight instead of
  // queueing behind it (round-4 B&B profile: a flows read waited ~0.5 ms for a 64x32 block)
  // (NEP_AUX_PRIORITY=0: default priority — the rocprofv3 PMC passes of tools/traffic.py run that way)
  {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
    const char *e = std::getenv("NEP_AUX_PRIORITY");
    if (e && std::atoi(e) == 0) greatest = least;
    HIPCHK(hipStreamCreateWithPriority(&m.aux, hipStreamNonBlocking, greatest));
  }
  HIPCHK(hipEventCreateWithFlags(&m.ev_aux, hipEventDisableTiming));
  // the second slot group's stream (launch_block; NEP_BLOCK_GROUPS=1: one chain per block on `stream` alone, for A/B
  // — the results are the same bits).  More groups are not offered: each is one more stream on a process's few
  // hardware queues, of which `stream` and `aux` already take two.
  m.groups = kBlockGroups;
  if (const char *e = std::getenv("NEP_BLOCK_GROUPS")) m.groups = std::atoi(e) >= 2 ? 2 : 1;
  if (m.groups > 1) {
    HIPCHK(hipStreamCreateWithFlags(&m.grp, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&m.ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m.ev_join, hipEventDisableTiming));
  }
  DeviceView &v = m.v;
  v.N = m.N; v.NP = m.NP; v.F = m.F; v.R = m.R; v.JB = m.JB; v.CPL = m.CPL;
  v.has_n = m.has_n; v.step2 = m.step2; v.variant = m.variant; v.fac = m.fac;
  v.M = m.M; v.eps = m.eps; v.sigma4 = m.sigma4; v.cost_n = m.cost_n; v.score_n_coef = m.score_n_coef;
  v.w_dis = m.w_dis;
  v.dred = m.dred; v.sT = m.sT; v.sum_old = m.sum_old;
  v.dl = m.dl; v.il = m.il;
  v.rs_suff = 0.2; v.rs_nec = 0.9; v.rs_art = 0.36; v.omega_smooth = 0.5;   // necessary 0.9: DESIGN.md §4
  if (const char *e = std::getenv("NEP_RESTART")) std::sscanf(e, "%lf,%lf,%lf", &v.rs_suff, &v.rs_nec, &v.rs_art);
  if (const char *e = std::getenv("NEP_OMEGA_SMOOTH")) v.omega_smooth = std::atof(e);
  if (const char *e = std::getenv("NEP_PIPELINE_MAX_DONE")) m.pipe_max_done = std::atoi(e);
  v.polish_res = kPolishRes;
  v.polish_budget = kPolishBudget;
  if (const char *e = std::getenv("NEP_POLISH")) {   // "res,budget"
    long long b = v.polish_budget;
    std::sscanf(e, "%lf,%lld", &v.polish_res, &b);
    v.polish_budget = b;
  }
  v.xelide = 1;   // (0: the steady-state x_pass streams closed chunks too, for A/B; the results are the same bits)
  if (const char *e = std::getenv("NEP_XPASS_ELIDE")) v.xelide = std::atoi(e) != 0;
  int rc;
  if ((rc = upload(m, &v.rows, m.rows))) return rc;
  if ((rc = upload(m, &v.frow, m.frow))) return rc;
  if ((rc = upload(m, &v.gam, m.gam))) return rc;
  if ((rc = upload(m, &v.rho, m.rho))) return rc;
  if ((rc = upload(m, &v.lo, m.lo))) return rc;
  if ((rc = upload(m, &v.hi, m.hi))) return rc;
  if ((rc = upload(m, &v.rownorm, m.rownorm))) return rc;
  if ((rc = upload(m, &v.cost_int, m.cost_int))) return rc;
  if ((rc = upload(m, &v.mem_f, m.mem_f))) return rc;
  if ((rc = upload(m, &v.capn, m.capn))) return rc;
  return NEP_OK;
}

int setup_dense(Model &m, const nep_model_desc &d) {
  DeviceView &v = m.v;
  const int N = m.N, NP = m.NP, F = m.F;
  std::vector<float> Dp((size_t)N * NP, 0.f), cp((size_t)F * NP, 0.f);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) Dp[(size_t)i * NP + j] = (float)d.delay[(size_t)i * N + j];
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < N; ++j) {
      double c = d.core_per_req[(size_t)f * N + j];
      if (!std::isfinite(c)) c = std::numeric_limits<float>::max();
      cp[(size_t)f * NP + j] = (float)std::min(c, (double)std::numeric_limits<float>::max());
    }
  int rc;
  if ((rc = upload(m, &v.D, Dp))) return rc;
  if ((rc = upload(m, &v.cpr, cp))) return rc;
  // per-slot arrays
  const int B = m.max_batch;
  v.sx = (int64_t)m.R * NP;
  if (const char *e = std::getenv("NEP_SLOT_PAD")) v.sx += std::max(0, std::atoi(e)) / 64 * 64;   // (probe)
  v.smask = (int64_t)F * NP;
  v.sint = m.il.n_int;
  v.sdual = m.dl.n_dual;
  v.skty = (int64_t)F * NP + NP + 4;
  v.stpart = (int64_t)F * NTS;
  v.sbpart = (int64_t)(F + m.JB) * NBS;
  v.snpart = (int64_t)F * (m.fac ? 3 : 2) * NP;   // fac: c, CPU share, reflected c (2ĉ - c) per (f, j)
  v.srpart = (int64_t)F * 2 * NP;
  {   // (probe: NEP_SLOT_OVERALLOC=k allocates the routing state for k x the slots; only B are used)
    const char *e = std::getenv("NEP_SLOT_OVERALLOC");
    const size_t k = e ? (size_t)std::max(1, std::atoi(e)) : 1;
    if ((rc = dalloc(m, &v.x, k * B * v.sx))) return rc;
    if ((rc = dalloc(m, &v.xa, k * B * v.sx))) return rc;
  }
  if ((rc = dalloc(m, &v.acnt, (size_t)B * m.R))) return rc;
  if ((rc = dalloc(m, &v.aent, (size_t)B * m.R * kAnchorK))) return rc;
  if ((rc = dalloc(m, &v.theta, (size_t)B * m.R))) return rc;
  if ((rc = dalloc(m, &v.mask, (size_t)B * v.smask))) return rc;
  if ((rc = dalloc(m, &v.zi, (size_t)B * v.sint))) return rc;
  if ((rc = dalloc(m, &v.zia, (size_t)B * v.sint))) return rc;
  if ((rc = dalloc(m, &v.zr, (size_t)B * v.sint))) return rc;
  if ((rc = dalloc(m, &v.lb, (size_t)B * v.sint))) return rc;
  if ((rc = dalloc(m, &v.ub, (size_t)B * v.sint))) return rc;
  if ((rc = dalloc(m, &v.y, (size_t)B * v.sdual))) return rc;
  if ((rc = dalloc(m, &v.ya, (size_t)B * v.sdual))) return rc;
  if ((rc = dalloc(m, &v.ybak, (size_t)B * v.sdual))) return rc;
  if ((rc = dalloc(m, &v.kz, (size_t)B * v.sdual))) return rc;
  if ((rc = dalloc(m, &v.kza, (size_t)B * v.sdual))) return rc;
  if ((rc = dalloc(m, &v.kty, (size_t)B * v.skty))) return rc;
  if ((rc = dalloc(m, &v.tpart, (size_t)B * v.stpart))) return rc;
  if ((rc = dalloc(m, &v.bpart, (size_t)B * v.sbpart))) return rc;
  if ((rc = dalloc(m, &v.npart, (size_t)B * v.snpart))) return rc;
  if (m.fac) {
    v.slsum = (int64_t)F * NP;
    if ((rc = dalloc(m, &v.lam, (size_t)B * v.sx))) return rc;
    if ((rc = dalloc(m, &v.lama, (size_t)B * v.sx))) return rc;
    if ((rc = dalloc(m, &v.lsum, (size_t)B * v.slsum))) return rc;
    std::vector<float> rl((size_t)F * NP, 0.f);
    for (int f = 0; f < F; ++f)
      for (int j = 0; j < N; ++j) rl[(size_t)f * NP + j] = (float)m.rhoL[(size_t)f * N + j];
    if ((rc = upload(m, &v.rho_l, rl))) return rc;
    // the reduced costs the certificate launches keep (two buffers per slot; 2 MB per slot at 512x256)
    v.srcbuf = 2 * (int64_t)m.il.n_int;
    if ((rc = dalloc(m, &v.rcbuf, (size_t)B * v.srcbuf))) return rc;
    HIPCHK(hipMemsetAsync(v.rcbuf, 0, sizeof(double) * B * v.srcbuf, m.stream));
    HIPCHK(hipMemsetAsync(v.lam, 0, sizeof(float) * B * v.sx, m.stream));
    HIPCHK(hipMemsetAsync(v.lsum, 0, sizeof(float) * B * v.slsum, m.stream));
  }
  if ((rc = dalloc(m, &v.rpart, (size_t)B * v.srpart))) return rc;
  if ((rc = dalloc(m, &v.ctrl, (size_t)B))) return rc;
  {
    void *h = nullptr;
    if (hipHostMalloc(&h, sizeof(Ctrl) * B) != hipSuccess) return fail(NEP_ERR_NOMEM, "hipHostMalloc (Ctrl)");
    m.h_ctrl = static_cast<Ctrl *>(h);
    if (hipHostMalloc(&h, sizeof(int32_t) * B) != hipSuccess) return fail(NEP_ERR_NOMEM, "hipHostMalloc (act)");
    m.h_act = static_cast<int32_t *>(h);
  }
  if ((rc = dalloc(m, &m.d_prm, 3))) return rc;
  v.prm = m.d_prm;
  if ((rc = dalloc(m, &m.d_slots, (size_t)B))) return rc;
  if ((rc = dalloc(m, &m.d_new, (size_t)B))) return rc;
  {
    const double *p = nullptr;
    if ((rc = upload(m, &p, m.base_lb))) return rc;
    m.d_base_lb = const_cast<double *>(p);
    if ((rc = upload(m, &p, m.base_ub))) return rc;
    m.d_base_ub = const_cast<double *>(p);
    const uint8_t *q = nullptr;
    if ((rc = upload(m, &q, m.base_mask))) return rc;
    m.d_base_mask = const_cast<uint8_t *>(q);
  }
  if ((rc = dalloc(m, &m.d_sub_i, (size_t)3 * B + 1 + (size_t)B * v.sint))) return rc;
  // (a submit stages at most one bound change per integer variable and LP — presolve_node appends an index once —
  // i.e. 2 x nchg <= 2 B n_int doubles, and nep_lp_submit_ex two more per LP behind them: its budgets / bound stops)
  if ((rc = dalloc(m, &m.d_sub_d, (size_t)2 * B * (v.sint + 1)))) return rc;
  {   // every slot's Ctrl zeroed, with no reduced costs kept (rc_lagr = -inf)
    Ctrl c0;
    std::memset(&c0, 0, sizeof(Ctrl));
    c0.rc_lagr = -INF;
    const std::vector<Ctrl> init((size_t)B, c0);
    HIPCHK(hipMemcpy(v.ctrl, init.data(), sizeof(Ctrl) * B, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemsetAsync(v.x, 0, sizeof(float) * B * v.sx, m.stream));
  HIPCHK(hipMemsetAsync(v.xa, 0, sizeof(float) * B * v.sx, m.stream));
  HIPCHK(hipMemsetAsync(v.acnt, 0, sizeof(int32_t) * B * m.R, m.stream));
  HIPCHK(hipMemsetAsync(v.theta, 0xFF, sizeof(float) * B * m.R, m.stream));   // NaN: no hint
  HIPCHK(hipMemsetAsync(v.zi, 0, sizeof(double) * B * v.sint, m.stream));
  HIPCHK(hipMemsetAsync(v.y, 0, sizeof(double) * B * v.sdual, m.stream));
  HIPCHK(hipStreamSynchronize(m.stream));
  return NEP_OK;
}

// The step size on the device (nep_build.hip): the host build's 60 power-iteration passes on K̃ᵀK̃ from the same
// start vector (mt19937_64(12345) normals, routing entries first), in fp64 with fixed-order reductions, over the
// device copies of the rows, delay and core_per_req matrices (fp32, as the iteration reads them) and the CSR / CSC
// of the small-variable part.  Scratch is freed afterwards.
int power_device(Model &m) {
  const DeviceView &v = m.v;
  const int N = m.N, o = m.dl.n_dual, ni = m.il.n_int;
  const size_t nx = (size_t)m.R * N;
  std::vector<double> zx(nx), zs(ni);
  {
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> nd;
    for (auto &t : zx) t = nd(rng);
    for (auto &t : zs) t = nd(rng);
  }
  const Coo &K = m.Ks;
  const size_t ne = K.v.size();
  std::vector<int32_t> rp(o + 1, 0), ci(ne), cp(ni + 1, 0), ri(ne);
  std::vector<double> cv(ne), rv(ne);
  for (size_t e = 0; e < ne; ++e) { rp[K.r[e] + 1]++; cp[K.c[e] + 1]++; }
  for (int k = 0; k < o; ++k) rp[k + 1] += rp[k];
  for (int k = 0; k < ni; ++k) cp[k + 1] += cp[k];
  {
    std::vector<int32_t> fr(rp.begin(), rp.end() - 1), fc(cp.begin(), cp.end() - 1);
    for (size_t e = 0; e < ne; ++e) {
      const int a = fr[K.r[e]]++, b = fc[K.c[e]]++;
      ci[a] = K.c[e]; cv[a] = K.v[e];
      ri[b] = K.r[e]; rv[b] = K.v[e];
    }
  }
  constexpr int kIters = 60, kBlk = 512;
  std::vector<void *> tmp;
  auto alloc = [&](size_t bytes) -> void * {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr;
    tmp.push_back(p);
    return p;
  };
  auto release = [&]() { for (void *p : tmp) (void)hipFree(p); tmp.clear(); };
  double *dzx = (double *)alloc(nx * 8), *dgx = (double *)alloc(nx * 8), *dzs = (double *)alloc(ni * 8);
  double *dgs = (double *)alloc(ni * 8), *dy = (double *)alloc((size_t)o * 8);
  double *dup = (double *)alloc((size_t)m.F * N * 8), *dsp = (double *)alloc((size_t)m.F * 8);
  double *dgf = (double *)alloc((size_t)m.F * N * 8), *dpart = (double *)alloc(kBlk * 8);
  double *dout = (double *)alloc((kIters + 1) * 8);
  int32_t *drp = (int32_t *)alloc((o + 1) * 4), *dci = (int32_t *)alloc(ne * 4), *dcp = (int32_t *)alloc((ni + 1) * 4);
  int32_t *dri = (int32_t *)alloc(ne * 4);
  double *dcv = (double *)alloc(ne * 8), *drv = (double *)alloc(ne * 8);
  for (void *p : tmp)
    if (!p) { release(); return fail(NEP_ERR_NOMEM, "hipMalloc (device power iteration)"); }
  hipError_t e = hipSuccess;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  if (e == hipSuccess) e = hipMemcpyAsync(dzx, zx.data(), nx * 8, h2d, m.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dzs, zs.data(), (size_t)ni * 8, h2d, m.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(drp, rp.data(), rp.size() * 4, h2d, m.stream);
  if (e == hipSuccess && ne) e = hipMemcpyAsync(dci, ci.data(), ne * 4, h2d, m.stream);
  if (e == hipSuccess && ne) e = hipMemcpyAsync(dcv, cv.data(), ne * 8, h2d, m.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dcp, cp.data(), cp.size() * 4, h2d, m.stream);
  if (e == hipSuccess && ne) e = hipMemcpyAsync(dri, ri.data(), ne * 4, h2d, m.stream);
  if (e == hipSuccess && ne) e = hipMemcpyAsync(drv, rv.data(), ne * 8, h2d, m.stream);
  if (e == hipSuccess)
    e = launch_power_iteration(v, kIters, dzx, dzs, dgx, dgs, dy, dup, dsp, dgf, dpart, kBlk, dout, drp, dci, dcv, dcp,
                               dri, drv, m.stream);
  double lam = 0.0;
  if (e == hipSuccess) e = hipMemcpyAsync(&lam, dout + kIters, 8, hipMemcpyDeviceToHost, m.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m.stream);
  release();
  if (e != hipSuccess) return fail(NEP_ERR_HIP, std::string("device power iteration: ") + hipGetErrorString(e));
  m.sigma_max = std::sqrt(std::max(lam, 1e-30));
  m.eta = 0.95 / m.sigma_max;
  m.power_host = false;
  return NEP_OK;
}

}  // namespace nep
