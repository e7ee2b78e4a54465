// nep_leaf_search.h — the native placement search (nep_leaf_search; DESIGN.md §7 "Native search"): the move records its
// kernels (nep_leaf_search.hip) expand on the device and the host's own state of the current placement
// (nep_leaf_search.cpp).  No HIP here: the host part builds and runs without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "nep_leaf.h"

namespace nep {

// one neighbour of the current placement on its way to the device
struct LeafSearchMove {
  int32_t kind;    // NEP_MOVE_ADD / DROP / CLOSE / SWAP
  int32_t fn;      // the function (-1: CLOSE)
  int32_t node;    // the node; a swap's destination
  int32_t src;     // a swap's source node (-1 otherwise)
  int32_t nopen;   // the neighbour's open nodes (the n of heuristics.apply_move's z', summed)
  int32_t pad_;
};

// device arrays and scalars of one expansion, beside the LeafView of the neighbours' slots
struct LeafSearchView {
  int warm;                    // the neighbours start from the base's best prices (0: from zeros)
  double cn;                   // cost_n (0: the variant has no n)
  double cutoff;
  const LeafSearchMove *mv;    // [B]
  const uint8_t *base_open;    // [F][N] the current placement's c
  const double *base_y;        // [N] its best prices
};

// the cell (f, j) of the neighbour `mv` of a placement whose cell is `was` (host and device: one rule)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint8_t leaf_search_cell(const LeafSearchMove &mv, int f, int j, uint8_t was) {
  uint8_t c = was;
  switch (mv.kind) {
    case 0: if (f == mv.fn && j == mv.node) c = 1; break;
    case 1: if (f == mv.fn && j == mv.node) c = 0; break;
    case 2: if (j == mv.node) c = 0; break;
    case 3:
      if (f == mv.fn && j == mv.src) c = 0;
      if (f == mv.fn && j == mv.node) c = 1;
      break;
    default: break;
  }
  return c;
}

// z' = z after one move, as core/engine/heuristics.py apply_move writes it (c f-major [F N], then n [N] where the variant
// has n); z_out may be z_in.  false: a record out of range (nothing written)
bool leaf_apply_move(int F, int N, int has_n, const double *z_in, int kind, int fn, int node, int src, double *z_out);

// an incumbent improves on upper by more than 1e-9 max(1, |upper|) (placement_search's acceptance, rounded as numpy's)
bool leaf_search_improves(double obj, double upper);

// The search's own copy of the current placement: its bytes, the placements per node and per function and its n.  A
// neighbour's open nodes and its screens against the evaluator's INFEASIBLE rules come from these in O(1) (O(F) for the
// memory of a node that gains a placement, and for a CLOSE); its bytes are built only where the host verifies it.
struct LeafSearchBase {
  int F = 0, N = 0, has_n = 0;
  std::vector<uint8_t> open;    // [F][N]
  std::vector<uint8_t> nval;    // [N] n (the variant without n: the node has a placement)
  std::vector<int32_t> ncnt;    // [N] placements per node
  std::vector<int32_t> fcnt;    // [F] destinations per function
  int64_t nsum = 0;             // sum of nval

  // c_open [F][N]; n [N] doubles of the placement's z (nullptr: the variant has no n)
  void set(int F_, int N_, const uint8_t *c_open, const double *n);
  bool in_range(int kind, int fn, int node, int src) const;
  // the record of a move in range, nopen filled
  LeafSearchMove record(int kind, int fn, int node, int src) const;
  // the neighbour is one the evaluator rejects (leaf_rejects on its z'), given that it does not reject the base
  bool rejects(const LeafLimits &lim, const LeafSearchMove &mv) const;
  // the neighbour's bytes, out [F][N]
  void neighbour(const LeafSearchMove &mv, uint8_t *out) const;
  // the neighbour becomes the base
  void accept(const LeafSearchMove &mv);
};

// the candidates of a lazy pass in the order they are verified: ascending (device objective, index) of the
// neighbours with live[q] != 0, a finite dq[q] and, for a finite upper, dq[q] improving on it
void leaf_search_order(const std::vector<double> &dq, const std::vector<uint8_t> &live, double upper,
                       std::vector<int> &out);

}  // namespace nep
