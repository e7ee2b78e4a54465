// nep_leaf.h — the fixed-placement evaluator (nep_leaf_eval; DESIGN.md §7 "Fixed-placement evaluator"):
// what its device rounds (nep_leaf.hip), its host repair (nep_leaf_repair.cpp) and the ABI (nep_leaf_host.cpp) share.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nep {

// The step rule of the price rounds (leaf_step, nep_leaf.hip; tests/leaf_ref.py carries the same constants): a Polyak
// step theta = lam (target - L) / |g|^2 toward the cutoff when it is finite, else toward
// best + kLeafMargin max(|best - base|, kLeafMarginFloor max(1, |best|)), where base = cost_n sum n is constant at a leaf
// (the margin scales with the routing part of the bound; measured on the fixture's congested leaves against a margin
// on |best|: the same bound after 64 rounds, a faster start where the node costs dominate); lam starts at 1 and halves
// after kLeafStall rounds in a row that did not raise the best bound.
constexpr double kLeafMargin = 0.05;
constexpr double kLeafMarginFloor = 1e-3;
constexpr int kLeafStall = 4;
// rows of a function are taken a lane per row while it has at most this many open destinations, else a wave per row
constexpr int kLeafLaneK = 16;
constexpr int kLeafThreads = 256;

// per-placement state of the rounds (device, one per placement of a chunk)
struct LeafCtrl {
  double base;      // cost_n sum n
  double best;      // best Lagrangian value so far (-inf before round 0)
  double lam;       // step scale
  double cutoff;
  int32_t stall;    // rounds in a row without a better bound
  int32_t done;     // 1: the placement's rounds have stopped (cut off, or a zero subgradient)
  int32_t cut;      // best >= cutoff
  int32_t pad_;
};

// device arrays of one chunk of placements
struct LeafView {
  int N, F, R, B;
  double kobj;
  const int32_t *frow, *row_src;   // [F + 1], [R]
  const double *D, *W, *cpr, *cores;   // fp64 instance: [N][N], [F][N], [F][N], [N]
  const uint8_t *open;   // [B][F][N] the placements' c
  double *y, *ybest;     // [B][N] prices: current, behind the best bound
  double *share;         // [B][F][N] CPU load of function f on node j
  double *fpart;         // [B][F] the functions' summed row minima
  double *load, *g;      // [B][N] CPU load, subgradient
  int32_t *asg0, *asg;   // [B][R] round-0 / current assignment (-1: pooled row)
  LeafCtrl *ctrl;        // [B]
};

// The per-round repair on the device (nep_leaf_heur.hip; nep_leaf_eval_ex with repair_every >= 1): moves of one round's
// repair at most, far below the host repair's 100000 — a round that needs more has no point.  The kernel's loops are
// bounded by this, N, F and R only.
constexpr int kLeafDevMoves = 4096;

// per-placement result of the device repairs
struct LeafHeurBest {
  double obj;       // the smallest objective a round's repair ended with (+inf: none)
  int32_t round;    // that round (-1: none); ties keep the earlier round
  int32_t pad_;
};

// device arrays of the per-round repair, one chunk of placements; the per-(f, j) column counts live in LeafView::share,
// dead between leaf_node and the next round's leaf_assign
struct LeafHeurView {
  int rounds;                // the call's rounds: round_upper's stride is rounds + 1
  int every;                 // repair rounds every, 2 every, ... and the last one
  double floor_;             // the column floor 1 - eps
  const int32_t *row_f;      // [R]
  uint16_t *opl;             // [B][F][N] the placements' open destinations per function, ascending
  int32_t *opn;              // [B][F] their counts
  double *flow;              // [B][R] flow left per row at its assigned node
  double *room, *fcost;      // [B][F] pooled mass left after the column deficits; the assignment's cost by function
  int32_t *nrows;            // [B][R] rows by overloaded node
  int32_t *asgrep;           // [B][R] the assignment of the best round
  double *loadrep;           // [B][N] its loads
  LeafHeurBest *best;        // [B]
  double *round_upper;       // [B][rounds + 1] objective per repaired round (+inf: not repaired, or no point)
};

// the host's fp64 view of a step-1 instance
struct LeafInstance {
  int N, F, R, has_n;
  double eps, kobj, cost_n;
  const double *D, *W, *cpr, *cores;
  const int *row_f, *row_src, *frow;
};

struct LeafPoint {
  bool found = false;
  double obj = 0.0;
  int64_t ties = 0;      // moves whose best score another candidate shared (the fixture generator asserts none)
  std::vector<int32_t> row, dst;
  std::vector<double> val, cpu;
};

// host repair of an assignment asg [R] (destination per loaded row) at the placement c_open [F][N] with nsum open nodes;
// load [N] (or nullptr: summed here from asg in row order) are the CPU loads of asg the moves start from
void leaf_repair(const LeafInstance &in, const uint8_t *c_open, double nsum, const int32_t *asg, LeafPoint &out,
                 const double *load = nullptr);

// Priced moves of a placement (nep_leaf_moves; nep_leaf_moves.hip prices, nep_leaf_moves.cpp composes): table [F][N]
// holds, per (f, j), the routing part of the change of the Lagrangian bound when a closed placement opens (<= 0) or
// an open one closes (>= 0, +inf: the function's only destination).
struct LeafMove {
  int32_t kind, fn, node;   // NEP_MOVE_ADD / DROP / CLOSE; the function (-1: CLOSE); the node
  double delta;             // L(C', y) - L(C, y)
};

// leaf_moves' and leaf_swaps' dynamic LDS (56 (N + 1) + 16 bytes each) is held to this: N <= 1169 (nep_leaf_moves and
// nep_leaf_swaps refuse a wider model)
constexpr size_t kLeafMovesLdsCap = 64 * 1024;

// what the move screens need beyond LeafInstance: the evaluator's INFEASIBLE rules on memory and budget
struct LeafLimits {
  const double *fmem, *nmem, *cost;   // [F], [N], [N]
  double budget;
};

// the moves of the placement c_open [F][N] from its table, screened (an ADD keeps the node's memory and, where it
// opens the node, the budget; a DROP or CLOSE leaves every function a destination) and in ascending (delta, kind,
// node, fn) order, at most max_moves of them
void leaf_move_list(const LeafInstance &in, const LeafLimits &lim, const uint8_t *c_open, const double *table,
                    int max_moves, std::vector<LeafMove> &out);

// Priced swaps of a placement (nep_leaf_swaps; nep_leaf_swaps.hip prices and selects, nep_leaf_swaps.cpp merges): a
// swap moves function fn from its open destination `from` to a closed one `to`.  At most kLeafSwapPerFn per function
// leave the device.
constexpr int kLeafSwapPerFn = 8;

// one selected swap of a (placement, function) on the device (+inf, -1, -1: none)
struct LeafSwapRec {
  double delta;
  int32_t from, to;
};

struct LeafSwap {
  int32_t fn, from, to;
  double delta;   // L(C', y) - L(C, y)
};

// device arrays of the swap pricing of one chunk of placements, beside its LeafView
struct LeafSwapView {
  int per_fn;             // records kept per function, 1 .. kLeafSwapPerFn
  double cn;              // cost_n (0: the variant has no n)
  const double *fmem;     // [F] the functions' memory
  const double *nmem1;    // [N] the nodes' memory + 1e-9 (the ADD screen's right-hand side)
  const int32_t *ncnt;    // [B][N] placements per node; -1: an empty node whose cost is beyond the budget
  const double *mem;      // [B][N] memory used per node, summed over its functions in ascending order
  LeafSwapRec *rec;       // [B][F][per_fn] the cheapest swaps per function, ascending (delta, to)
  double *best;           // [B][F][N] or nullptr: the cheapest swap of f into j' (+inf: open, or screened)
  int32_t *best_from;     // [B][F][N] or nullptr: its source node (-1: none)
};

// the per_fn cheapest (delta, to) per function of the tables best / best_from [F][N], appended to out in the kernel's
// order (functions ascending, then ascending (delta, to))
void leaf_swap_select(int F, int N, const double *best, const int32_t *best_from, int per_fn,
                      std::vector<LeafSwap> &out);
// out in ascending (delta, fn, to, from) order, cut to max_moves
void leaf_swap_merge(std::vector<LeafSwap> &out, int max_moves);

}  // namespace nep
