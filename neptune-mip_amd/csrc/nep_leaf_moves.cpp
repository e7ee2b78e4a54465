// nep_leaf_moves.cpp — the move list of a placement from its priced table (nep_leaf_moves, nep_debug_leaf_move_list;
// DESIGN.md §7 "Priced moves").  Host only, fp64; tests/leaf_moves_ref.py `move_list` is its mirror, rule for rule and
// in the same order of operations.  A node counts as open when its column of c has a 1.
//
//   ADD (f, j) closed    delta = table[f][j] + cost_n [node j closed, the variant has n]; kept while the node's memory
//                        holds f as well and, where the node opens, its cost is within the budget (the evaluator's
//                        INFEASIBLE rules: every placement a move leads to is one the evaluator takes)
//   DROP (f, j) open     with a finite entry (f keeps another destination):
//                        delta = table[f][j] - cost_n [the node's only placement, the variant has n]
//   CLOSE node j         with at least two placements, all with finite entries: delta = sum_f table[f][j] over its
//                        open f ascending, minus cost_n; fn = -1 (a node with one placement is its DROP)
#include <algorithm>
#include <cmath>

#include "nep_leaf.h"

namespace nep {

void leaf_move_list(const LeafInstance &in, const LeafLimits &lim, const uint8_t *c_open, const double *table,
                    int max_moves, std::vector<LeafMove> &out) {
  const int N = in.N, F = in.F;
  const double cn = in.has_n ? in.cost_n : 0.0;
  out.clear();
  for (int j = 0; j < N; ++j) {
    double mem = 0.0, closing = 0.0;
    int cnt = 0;
    bool finite = true;
    for (int f = 0; f < F; ++f) {
      if (!c_open[(size_t)f * N + j]) continue;
      const double t = table[(size_t)f * N + j];
      mem += lim.fmem[f];
      ++cnt;
      if (std::isfinite(t)) closing += t;
      else finite = false;
    }
    const bool opens = cnt == 0;
    for (int f = 0; f < F; ++f) {
      const double t = table[(size_t)f * N + j];
      if (!c_open[(size_t)f * N + j]) {
        if (!(mem + lim.fmem[f] <= lim.nmem[j] + 1e-9)) continue;
        if (opens && in.has_n && !(lim.cost[j] <= lim.budget + 1e-9)) continue;
        out.push_back(LeafMove{0, f, j, t + (opens ? cn : 0.0)});
      } else if (std::isfinite(t)) {
        out.push_back(LeafMove{1, f, j, t - (cnt == 1 ? cn : 0.0)});
      }
    }
    if (cnt >= 2 && finite) out.push_back(LeafMove{2, -1, j, closing - cn});
  }
  // (delta, kind, node, fn) is a strict total order — no two moves share kind, node and fn — so the head of a partial
  // sort is the head of the full one; a search asks for tens of the ~F N moves
  const auto less = [](const LeafMove &a, const LeafMove &b) {
    if (a.delta != b.delta) return a.delta < b.delta;
    if (a.kind != b.kind) return a.kind < b.kind;
    if (a.node != b.node) return a.node < b.node;
    return a.fn < b.fn;
  };
  const size_t keep = std::min(out.size(), (size_t)std::max(0, max_moves));
  std::partial_sort(out.begin(), out.begin() + keep, out.end(), less);
  out.resize(keep);
}

}  // namespace nep
