// nep_leaf_swaps.cpp — the swap list of a placement (nep_leaf_swaps, nep_debug_leaf_swap_list; DESIGN.md §7 "Priced
// swaps").  Host only; tests/leaf_swaps_ref.py `swap_list` is its mirror.  The kernel (nep_leaf_swaps.hip) prices every
// swap and keeps the per_fn cheapest (delta, to) of each function; leaf_swap_select is that selection on given tables,
// leaf_swap_merge orders what either selected.
#include <algorithm>
#include <cmath>

#include "nep_leaf.h"

namespace nep {

void leaf_swap_select(int F, int N, const double *best, const int32_t *best_from, int per_fn,
                      std::vector<LeafSwap> &out) {
  std::vector<int32_t> to;
  for (int f = 0; f < F; ++f) {
    const double *bf = best + (size_t)f * N;
    to.clear();
    for (int j = 0; j < N; ++j)
      if (std::isfinite(bf[j])) to.push_back(j);
    const size_t keep = std::min(to.size(), (size_t)per_fn);
    // (delta, to) is a strict total order: the head of a partial sort is the head of the full one
    std::partial_sort(to.begin(), to.begin() + keep, to.end(),
                      [bf](int32_t a, int32_t b) { return bf[a] != bf[b] ? bf[a] < bf[b] : a < b; });
    for (size_t q = 0; q < keep; ++q) out.push_back(LeafSwap{f, best_from[(size_t)f * N + to[q]], to[q], bf[to[q]]});
  }
}

void leaf_swap_merge(std::vector<LeafSwap> &out, int max_moves) {
  // (delta, fn, to, from) is a strict total order: a function has one record per destination
  const auto less = [](const LeafSwap &a, const LeafSwap &b) {
    if (a.delta != b.delta) return a.delta < b.delta;
    if (a.fn != b.fn) return a.fn < b.fn;
    if (a.to != b.to) return a.to < b.to;
    return a.from < b.from;
  };
  const size_t keep = std::min(out.size(), (size_t)std::max(0, max_moves));
  std::partial_sort(out.begin(), out.begin() + keep, out.end(), less);
  out.resize(keep);
}

}  // namespace nep
