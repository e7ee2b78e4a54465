// leaf_search_main.cpp — a stand-alone check of the native placement search's host state (csrc/nep_leaf_search.cpp) for a
// sanitizer build: no HIP, no Python.  Built with nep_leaf_search.cpp, nep_leaf_repair.cpp, nep_leaf_moves.cpp and
// nep_leaf_swaps.cpp (tests/test_leaf_search_host_sanitized.py: the host's address and undefined-behaviour sanitizers)
// and run on a text file:
//
//   F N has_n budget
//   fmem [F]   nmem [N]   cost [N]   z [F N (+ N)]
//   n_moves, then per move: kind fn node src
//
// For the file's moves and for every single move leaf_move_list composes from a zero table it checks, against a full
// O(F N) recomputation from leaf_apply_move's z': the neighbour's bytes, its open-node count, the incremental screen
// against the evaluator's INFEASIBLE rules, and the counts after accept().  Prints "ok <moves>" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../neptune-mip_amd/csrc/nep_leaf_search.h"

using namespace nep;

namespace {

struct Inst {
  int F = 0, N = 0, has_n = 0;
  double budget = 0.0;
  std::vector<double> fmem, nmem, cost, z;
};

// the evaluator's INFEASIBLE rules on a whole z (nep_leaf_host.cpp leaf_rejects), written out
bool rejects_full(const Inst &in, const std::vector<double> &z) {
  const int F = in.F, N = in.N;
  std::vector<double> mem(N, 0.0);
  std::vector<int> any(N, 0);
  for (int f = 0; f < F; ++f) {
    bool dest = false;
    for (int j = 0; j < N; ++j)
      if (z[(size_t)f * N + j] != 0.0) { mem[j] += in.fmem[f]; any[j] = 1; dest = true; }
    if (!dest) return true;
  }
  for (int j = 0; j < N; ++j) {
    if (mem[j] > in.nmem[j] + 1e-9) return true;
    if (in.has_n) {
      const double nj = z[(size_t)F * N + j];
      if ((any[j] != 0) != (nj != 0.0)) return true;
      if (in.cost[j] * nj > in.budget + 1e-9) return true;
    }
  }
  return false;
}

void base_of(const Inst &in, const std::vector<double> &z, LeafSearchBase &b) {
  std::vector<uint8_t> c((size_t)in.F * in.N);
  for (size_t k = 0; k < c.size(); ++k) c[k] = z[k] != 0.0;
  b.set(in.F, in.N, c.data(), in.has_n ? z.data() + c.size() : nullptr);
}

int fail_at(const char *what, int kind, int fn, int node, int src) {
  std::fprintf(stderr, "mismatch: %s at move (%d, %d, %d, %d)\n", what, kind, fn, node, src);
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <case file>\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  Inst in;
  if (!(f >> in.F >> in.N >> in.has_n >> in.budget) || in.F < 1 || in.N < 1) return 2;
  const size_t FN = (size_t)in.F * in.N, ni = FN + (in.has_n ? in.N : 0);
  in.fmem.resize(in.F); in.nmem.resize(in.N); in.cost.resize(in.N); in.z.resize(ni);
  for (double &v : in.fmem) f >> v;
  for (double &v : in.nmem) f >> v;
  for (double &v : in.cost) f >> v;
  for (double &v : in.z) f >> v;
  size_t nm = 0;
  f >> nm;
  std::vector<LeafSearchMove> moves(nm);
  for (LeafSearchMove &m : moves) f >> m.kind >> m.fn >> m.node >> m.src;
  if (!f) return 2;

  LeafSearchBase base;
  base_of(in, in.z, base);
  const bool base_rejected = rejects_full(in, in.z);
  // every single move the list composes from a zero table, besides the file's
  {
    LeafInstance li{};
    li.N = in.N; li.F = in.F; li.has_n = in.has_n;
    const LeafLimits lim{in.fmem.data(), in.nmem.data(), in.cost.data(), in.budget};
    std::vector<double> table(FN, 0.0);
    std::vector<LeafMove> mv;
    leaf_move_list(li, lim, base.open.data(), table.data(), (int)(2 * FN + in.N), mv);
    for (const LeafMove &m : mv) moves.push_back(LeafSearchMove{m.kind, m.fn, m.node, -1, 0, 0});
    std::vector<LeafSwap> sw{{0, 0, 0, 1.0}, {0, 0, 0, 0.5}};
    leaf_swap_merge(sw, 1);
    if (sw.size() != 1 || sw[0].delta != 0.5) return fail_at("leaf_swap_merge", 3, 0, 0, 0);
  }
  const LeafLimits lim{in.fmem.data(), in.nmem.data(), in.cost.data(), in.budget};
  std::vector<double> z2(ni);
  std::vector<uint8_t> nb(FN);
  std::vector<int> order;
  size_t done = 0;
  for (const LeafSearchMove &m : moves) {
    if (!base.in_range(m.kind, m.fn, m.node, m.src)) {
      if (leaf_apply_move(in.F, in.N, in.has_n, in.z.data(), m.kind, m.fn, m.node, m.src, z2.data()))
        return fail_at("a record out of range was applied", m.kind, m.fn, m.node, m.src);
      continue;
    }
    if (!leaf_apply_move(in.F, in.N, in.has_n, in.z.data(), m.kind, m.fn, m.node, m.src, z2.data()))
      return fail_at("a record in range was refused", m.kind, m.fn, m.node, m.src);
    const LeafSearchMove r = base.record(m.kind, m.fn, m.node, m.src);
    base.neighbour(r, nb.data());
    for (size_t k = 0; k < FN; ++k)
      if (nb[k] != (z2[k] != 0.0)) return fail_at("neighbour bytes", m.kind, m.fn, m.node, m.src);
    for (int ff = 0; ff < in.F; ++ff)
      for (int j = 0; j < in.N; ++j)
        if (leaf_search_cell(r, ff, j, base.open[(size_t)ff * in.N + j]) != nb[(size_t)ff * in.N + j])
          return fail_at("leaf_search_cell", m.kind, m.fn, m.node, m.src);
    LeafSearchBase want;
    base_of(in, z2, want);
    if (r.nopen != want.nsum) return fail_at("open-node count", m.kind, m.fn, m.node, m.src);
    if (!base_rejected && base.rejects(lim, r) != rejects_full(in, z2))
      return fail_at("the incremental screen", m.kind, m.fn, m.node, m.src);
    LeafSearchBase got = base;
    got.accept(r);
    if (got.open != want.open || got.ncnt != want.ncnt || got.fcnt != want.fcnt || got.nval != want.nval ||
        got.nsum != want.nsum)
      return fail_at("accept", m.kind, m.fn, m.node, m.src);
    ++done;
  }
  // the lazy pass's order on a small vector with ties, infinities and cut-off entries
  {
    const std::vector<double> dq{0.5, INFINITY, 0.25, 0.25, 0.9, 0.1};
    const std::vector<uint8_t> live{1, 1, 1, 1, 1, 0};
    leaf_search_order(dq, live, 0.8, order);
    if (order != std::vector<int>{2, 3, 0}) return fail_at("leaf_search_order", -1, -1, -1, -1);
    leaf_search_order(dq, live, INFINITY, order);
    if (order != std::vector<int>{2, 3, 0, 4}) return fail_at("leaf_search_order (no incumbent)", -1, -1, -1, -1);
  }
  std::printf("ok %zu\n", done);
  return 0;
}
