// nep_leaf_search.cpp — the host's state of the native placement search (nep_leaf_search, nep_debug_leaf_apply_move;
// DESIGN.md §7 "Native search").  Host only and without HIP: the move application that rebuilds z and the verified
// neighbours' bytes, the current placement's counts, the neighbours' screens and the lazy pass's order.
// core/engine/heuristics.py `apply_move` is the mirror of leaf_apply_move.
#include "nep_leaf_search.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace nep {

static bool move_in_range(int F, int N, int kind, int fn, int node, int src) {
  if (kind < 0 || kind > 3 || node < 0 || node >= N) return false;
  if (kind != 2 && (fn < 0 || fn >= F)) return false;
  if (kind == 3 && (src < 0 || src >= N)) return false;
  return true;
}

bool leaf_apply_move(int F, int N, int has_n, const double *z_in, int kind, int fn, int node, int src, double *z_out) {
  if (!move_in_range(F, N, kind, fn, node, src)) return false;
  const size_t FN = (size_t)F * N, ni = FN + (has_n ? N : 0);
  if (z_out != z_in) std::memmove(z_out, z_in, ni * sizeof(double));
  double *C = z_out;
  const auto any = [&](int j) {
    for (int f = 0; f < F; ++f)
      if (C[(size_t)f * N + j] != 0.0) return true;
    return false;
  };
  double opened = 1.0;
  if (kind == 0) {
    C[(size_t)fn * N + node] = 1.0;
  } else if (kind == 1) {
    C[(size_t)fn * N + node] = 0.0;
    opened = any(node) ? 1.0 : 0.0;
  } else if (kind == 2) {
    for (int f = 0; f < F; ++f) C[(size_t)f * N + node] = 0.0;
    opened = 0.0;
  } else {
    C[(size_t)fn * N + src] = 0.0;
    C[(size_t)fn * N + node] = 1.0;
    if (has_n) z_out[FN + src] = any(src) ? 1.0 : 0.0;
  }
  if (has_n) z_out[FN + node] = opened;
  return true;
}

bool leaf_search_improves(double obj, double upper) {
  const double tol = 1e-9 * std::max(1.0, std::fabs(upper));
  return obj < upper - tol;
}

void LeafSearchBase::set(int F_, int N_, const uint8_t *c_open, const double *n) {
  F = F_; N = N_; has_n = n ? 1 : 0;
  open.assign(c_open, c_open + (size_t)F * N);
  ncnt.assign(N, 0);
  fcnt.assign(F, 0);
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < N; ++j)
      if (open[(size_t)f * N + j]) { ++ncnt[j]; ++fcnt[f]; }
  nval.assign(N, 0);
  nsum = 0;
  for (int j = 0; j < N; ++j) {
    nval[j] = n ? n[j] != 0.0 : ncnt[j] > 0;
    nsum += nval[j];
  }
}

bool LeafSearchBase::in_range(int kind, int fn, int node, int src) const {
  return move_in_range(F, N, kind, fn, node, src);
}

// the n of a node after the move, as apply_move writes it (`touched`: the move writes this node's n)
static int n_after(const LeafSearchBase &b, const LeafSearchMove &mv, int j, bool *touched) {
  const size_t N = b.N;
  *touched = true;
  if (mv.kind == 0 && j == mv.node) return 1;
  if (mv.kind == 1 && j == mv.node) return b.ncnt[j] - (b.open[mv.fn * N + j] ? 1 : 0) > 0;
  if (mv.kind == 2 && j == mv.node) return 0;
  if (mv.kind == 3 && j == mv.node) return 1;   // (apply_move writes the destination last)
  if (mv.kind == 3 && j == mv.src) return b.ncnt[j] - (b.open[mv.fn * N + j] ? 1 : 0) > 0;
  *touched = false;
  return b.nval[j];
}

LeafSearchMove LeafSearchBase::record(int kind, int fn, int node, int src) const {
  LeafSearchMove mv{kind, kind == 2 ? -1 : fn, node, kind == 3 ? src : -1, 0, 0};
  int64_t s = nsum;
  bool touched;
  s += n_after(*this, mv, node, &touched) - (int)nval[node];
  if (kind == 3 && src != node) s += n_after(*this, mv, src, &touched) - (int)nval[src];
  mv.nopen = (int32_t)s;
  return mv;
}

bool LeafSearchBase::rejects(const LeafLimits &lim, const LeafSearchMove &mv) const {
  const size_t Ns = N;
  // every function keeps a destination
  if (mv.kind == 2) {
    for (int f = 0; f < F; ++f)
      if (open[f * Ns + mv.node] && fcnt[f] <= 1) return true;
  } else {
    int cnt = fcnt[mv.fn];
    const uint8_t was = open[mv.fn * Ns + mv.node];
    cnt += (int)leaf_search_cell(mv, mv.fn, mv.node, was) - (int)was;
    if (mv.kind == 3 && mv.src != mv.node) cnt -= (int)open[mv.fn * Ns + mv.src];
    if (cnt <= 0) return true;
  }
  // a node that gains a placement: its memory, over its functions in ascending order (the others' sums lose terms)
  if (mv.kind == 0 || mv.kind == 3) {
    double mem = 0.0;
    for (int f = 0; f < F; ++f)
      if (leaf_search_cell(mv, f, mv.node, open[f * Ns + mv.node])) mem += lim.fmem[f];
    if (mem > lim.nmem[mv.node] + 1e-9) return true;
  }
  // a node whose n the move writes: the budget
  for (int k = 0; k < 2 && has_n; ++k) {
    if (k == 1 && (mv.kind != 3 || mv.src == mv.node)) continue;
    const int j = k == 0 ? mv.node : mv.src;
    bool touched;
    const double nj = n_after(*this, mv, j, &touched);
    if (touched && lim.cost[j] * nj > lim.budget + 1e-9) return true;
  }
  return false;
}

void LeafSearchBase::neighbour(const LeafSearchMove &mv, uint8_t *out) const {
  const size_t Ns = N;
  std::memcpy(out, open.data(), (size_t)F * Ns);
  if (mv.kind == 2) {
    for (int f = 0; f < F; ++f) out[f * Ns + mv.node] = 0;
    return;
  }
  for (int j : {mv.src, mv.node})
    if (j >= 0) out[mv.fn * Ns + j] = leaf_search_cell(mv, mv.fn, j, out[mv.fn * Ns + j]);
}

void LeafSearchBase::accept(const LeafSearchMove &mv) {
  const size_t Ns = N;
  bool touched;
  const int n_node = n_after(*this, mv, mv.node, &touched);
  const int n_src = mv.kind == 3 ? n_after(*this, mv, mv.src, &touched) : 0;
  const auto put = [&](int f, int j) {
    const uint8_t was = open[f * Ns + j], now = leaf_search_cell(mv, f, j, was);
    open[f * Ns + j] = now;
    ncnt[j] += (int)now - (int)was;
    fcnt[f] += (int)now - (int)was;
  };
  if (mv.kind == 2) {
    for (int f = 0; f < F; ++f) put(f, mv.node);
  } else {
    if (mv.kind == 3) put(mv.fn, mv.src);
    put(mv.fn, mv.node);
  }
  if (mv.kind == 3 && mv.src != mv.node) {
    nsum += n_src - (int)nval[mv.src];
    nval[mv.src] = (uint8_t)n_src;
  }
  nsum += n_node - (int)nval[mv.node];
  nval[mv.node] = (uint8_t)n_node;
}

void leaf_search_order(const std::vector<double> &dq, const std::vector<uint8_t> &live, double upper,
                       std::vector<int> &out) {
  out.clear();
  for (size_t q = 0; q < dq.size(); ++q) {
    if (!live[q] || !std::isfinite(dq[q])) continue;
    if (std::isfinite(upper) && !leaf_search_improves(dq[q], upper)) continue;
    out.push_back((int)q);
  }
  std::sort(out.begin(), out.end(), [&dq](int a, int b) { return dq[a] != dq[b] ? dq[a] < dq[b] : a < b; });
}

}  // namespace nep
