// nep_leaf_repair.cpp — host repair of the fixed-placement evaluator (nep_leaf_eval; DESIGN.md §7 "Fixed-placement
// evaluator"): an assignment of every loaded routing row to one open destination becomes a routing that meets every
// reference step-1 row at the placement, or none is found.  Host only, fp64; tests/leaf_ref.py `repair` is its mirror,
// rule for rule and in the same order of operations.
//
//   1. overloaded nodes (CPU_j > cores_j) in ascending j; for each, while it is above its target
//      cores_j - 1e-12 max(1, |cores_j|) (core/engine/routing.py repair_cpu's), move flow of a loaded row from j to
//      another open destination of its function with CPU room: the least objective increase per unit of CPU relief,
//      ties by lowest row, then lowest destination; the move is cut to the row's flow at j, the destination's room, the
//      node's excess and what the column floor of (f, j) leaves (its loaded flow above 1 - eps plus the pooled mass
//      the function has left).  A destination is never filled past its target, so one pass over j suffices.
//   2. the pooled row of each function pays the column deficits 1 - eps - (loaded flow) of its open destinations; the
//      rest of its mass goes to the function's lowest open node.
//   3. every row is verified in fp64 (C1/C2, C4, C5 at CPU_j <= cores_j) on the entries as returned.
// No move left, or pooled mass short of the deficits: no point.  Chained moves are not tried.
#include <algorithm>
#include <cmath>
#include <utility>

#include "nep_leaf.h"

namespace nep {

namespace {
constexpr int64_t kMaxMoves = 100000;

struct Ent {
  int32_t j;
  double v;
};

inline int find(const std::vector<Ent> &e, int j) {
  for (size_t q = 0; q < e.size(); ++q)
    if (e[q].j == j) return (int)q;
  return -1;
}
}  // namespace

void leaf_repair(const LeafInstance &in, const uint8_t *c_open, double nsum, const int32_t *asg, LeafPoint &out,
                 const double *load) {
  const int N = in.N, F = in.F, R = in.R;
  const double floor_ = 1.0 - in.eps;
  out = LeafPoint();
  std::vector<double> lim(N), cpu(N, 0.0), col((size_t)F * N, 0.0), room(F), mf(F);
  for (int j = 0; j < N; ++j) lim[j] = in.cores[j] - 1e-12 * std::max(1.0, std::fabs(in.cores[j]));
  std::vector<std::vector<Ent>> ent(R);
  std::vector<std::vector<int>> node_rows(N), opens(F);
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < N; ++j)
      if (c_open[(size_t)f * N + j]) opens[f].push_back(j);
  bool ok = true;
  for (int r = 0; r < R; ++r) {
    const int f = in.row_f[r], i = in.row_src[r];
    if (i < 0) continue;
    const int j = asg[r];
    if (j < 0 || j >= N || !c_open[(size_t)f * N + j]) {   // (not an assignment of this placement)
      out.cpu.assign(N, 0.0);
      return;
    }
    ent[r].push_back(Ent{j, 1.0});
    if (!load) cpu[j] += in.W[(size_t)f * N + i] * in.cpr[(size_t)f * N + j];
    col[(size_t)f * N + j] += 1.0;
    node_rows[j].push_back(r);
  }
  // (the device rounds' loads, summed per function and then over the functions: the moves then see the bits the
  // device repair saw; the returned point's loads are recomputed from its entries either way)
  if (load) std::copy(load, load + N, cpu.begin());
  for (int f = 0; f < F; ++f) {
    const int rl = in.frow[f + 1] - 1;
    const bool pooled = in.frow[f + 1] > in.frow[f] && in.row_src[rl] < 0;
    mf[f] = pooled ? (double)(N - (in.frow[f + 1] - in.frow[f] - 1)) : 0.0;
    double def = 0.0;
    for (int j : opens[f]) def += std::max(0.0, floor_ - col[(size_t)f * N + j]);
    room[f] = mf[f] - def;
  }
  int64_t moves = 0;
  for (int j = 0; j < N && ok; ++j) {
    if (!(cpu[j] > in.cores[j])) continue;
    while (cpu[j] > lim[j]) {
      bool have = false, tie = false;
      double bs = 0.0, bt = 0.0, bld = 0.0, brelief = 0.0;
      int br = -1, bjd = -1, bf = -1;
      for (int r : node_rows[j]) {
        const int qv = find(ent[r], j);
        if (qv < 0 || ent[r][qv].v <= 0.0) continue;
        const double v = ent[r][qv].v;
        const int f = in.row_f[r], i = in.row_src[r];
        const double w = in.W[(size_t)f * N + i];
        const double relief = w * in.cpr[(size_t)f * N + j];
        if (!(relief > 0.0)) continue;
        const double tsrc = std::min(v, std::max(0.0, col[(size_t)f * N + j] - floor_) + std::max(0.0, room[f]));
        const double need = (cpu[j] - lim[j]) / relief;
        const double oc = in.kobj * w;
        for (int jd : opens[f]) {
          if (jd == j) continue;
          const double ld = w * in.cpr[(size_t)f * N + jd];
          double t = std::min(tsrc, need);
          if (ld > 0.0) {
            const double rm = lim[jd] - cpu[jd];
            if (!(rm > 0.0)) continue;
            t = std::min(t, rm / ld);
          }
          if (!(t > 1e-15)) continue;
          const double s = oc * (in.D[(size_t)i * N + jd] - in.D[(size_t)i * N + j]) / relief;
          bool take = false;
          if (!have || s < bs) {
            take = true;
            tie = false;
          } else if (s == bs) {
            tie = true;
            take = r < br || (r == br && jd < bjd);
          }
          if (take) {
            have = true;
            bs = s; bt = t; bld = ld; brelief = relief; br = r; bjd = jd; bf = f;
          }
        }
      }
      if (!have || moves >= kMaxMoves) {
        ok = false;
        break;
      }
      out.ties += tie ? 1 : 0;
      double &cj = col[(size_t)bf * N + j], &cd = col[(size_t)bf * N + bjd];
      const double d0 = std::max(0.0, floor_ - cj) + std::max(0.0, floor_ - cd);
      std::vector<Ent> &e = ent[br];
      const int qj = find(e, j);
      if (bt >= e[qj].v) e.erase(e.begin() + qj);
      else e[qj].v -= bt;
      if (const int qd = find(e, bjd); qd >= 0) {
        e[qd].v += bt;
      } else {
        node_rows[bjd].push_back(br);
        e.push_back(Ent{bjd, bt});
      }
      cpu[j] -= bt * brelief;
      cpu[bjd] += bt * bld;
      cj -= bt;
      cd += bt;
      room[bf] -= std::max(0.0, floor_ - cj) + std::max(0.0, floor_ - cd) - d0;
      ++moves;
    }
  }
  if (ok) {
    for (int f = 0; f < F; ++f) {
      const int r = in.frow[f + 1] - 1;
      const std::vector<int> &op = opens[f];
      if (op.empty()) { ok = false; continue; }
      if (in.row_src[r] >= 0) {   // no pooled row: the loaded flow alone must meet the floors
        for (int j : op)
          if (std::max(0.0, floor_ - col[(size_t)f * N + j]) > 1e-12) ok = false;
        continue;
      }
      const double m = mf[f];
      double rest = 1.0;
      for (size_t q = 1; q < op.size(); ++q) {
        const double d = std::max(0.0, floor_ - col[(size_t)f * N + op[q]]);
        if (d > 0.0) {
          ent[r].push_back(Ent{op[q], d / m});
          rest -= d / m;
        }
      }
      if (rest * m < std::max(0.0, floor_ - col[(size_t)f * N + op[0]])) ok = false;
      else ent[r].push_back(Ent{op[0], rest});
    }
  }
  // the point in output order (row-major, ascending destination), its CPU loads and objective, verified in fp64
  out.cpu.assign(N, 0.0);
  double obj = in.has_n ? in.cost_n * nsum : 0.0;
  std::vector<double> colt((size_t)F * N, 0.0);
  for (int r = 0; r < R; ++r) {
    std::vector<Ent> &e = ent[r];
    std::sort(e.begin(), e.end(), [](const Ent &a, const Ent &b) { return a.j < b.j; });
    const int f = in.row_f[r], i = in.row_src[r];
    double rsum = 0.0;
    for (const Ent &q : e) {
      if (!(q.v > 0.0)) continue;
      out.row.push_back(r);
      out.dst.push_back(q.j);
      out.val.push_back(q.v);
      rsum += q.v;
      if (i >= 0) {
        out.cpu[q.j] += q.v * (in.W[(size_t)f * N + i] * in.cpr[(size_t)f * N + q.j]);
        obj += (in.kobj * in.W[(size_t)f * N + i]) * in.D[(size_t)i * N + q.j] * q.v;
        colt[(size_t)f * N + q.j] += q.v;
      } else {
        colt[(size_t)f * N + q.j] += q.v * mf[f];
      }
    }
    if (!(std::fabs(rsum - 1.0) <= 1e-12)) ok = false;
  }
  for (int j = 0; j < N; ++j)
    if (!(out.cpu[j] <= in.cores[j])) ok = false;
  for (size_t k = 0; k < colt.size(); ++k) {
    if (c_open[k] ? !(colt[k] >= floor_ - 1e-12) : colt[k] > 0.0) ok = false;
  }
  out.obj = obj;
  out.found = ok;
}

}  // namespace nep
