// nep_leaf_moves.hip — priced add / drop moves of a fixed placement (nep_leaf_moves; DESIGN.md §7 "Priced moves") for
// gfx950.  At prices y >= 0 a loaded row r = (f, i) costs rho_r(j) = oc_r D[i, j] + w_r (y_j cpr[f, j]) at destination
// j (leaf_assign's expression and rounding).  With m1_r / j1_r the minimum and argmin over the open destinations of f
// (ties to the lowest j) and m2_r the minimum over the others (+inf: none), the routing part of the change of
//
//   L(y) = cost_n sum n + sum_rows m1_r - sum_j y_j cores_j
//
// is, for every (f, j) at once,
//   (f, j) closed: - sum_r max(0, m1_r - rho_r(j))       opening it: rows that are cheaper there move
//   (f, j) open:     sum_{r : j1_r = j} (m2_r - m1_r)    closing it: its rows fall back to their second choice
//                    (+inf when f has no other destination)
// both summed over the rows of f in ascending order.  One launch per chunk of placements, grid (F, B) as leaf_assign:
//   phase 1  the open list and y_j cpr[f, j] to LDS; per loaded row m1, j1, m2 (a lane per row while K <= kLeafLaneK,
//            else a wave per row and a butterfly over (value, index, second value)), kept in LDS with the row's
//            source, workload and objective scale
//   phase 2  a thread per destination j, strided over N, walks the rows: reads of D[src_r, j] are coalesced along j
// fp64, no contraction, no atomics, every sum in a fixed order: two calls return the same bits.  The table goes to the
// chunk's `share` buffer and the functions' summed minima to `fpart` (both dead outside an evaluator round); nothing
// of LeafCtrl is read or written.
#include <hip/hip_runtime.h>

#include "nep_launch.h"
#include "nep_leaf.h"
#include "nep_leaf_device.h"

namespace nep {

// dynamic LDS of leaf_moves: leaf_assign's arrays plus three over the rows (second minima, objective scales, sources)
size_t leaf_moves_lds(int N) {
  return (size_t)(N + 1) * (5 * sizeof(double) + 4 * sizeof(int32_t)) + 16;
}

__global__ void leaf_moves(LeafView v) {
#pragma clang fp contract(off)   // (rho rounds as in leaf_assign and the fp64 mirror)
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, tid = threadIdx.x, lane = tid & 63;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int N1 = N + 1;
  double *yc = reinterpret_cast<double *>(lds_raw);   // [K] y_j cpr[f, j] of the open destinations
  double *m1 = yc + N1;                               // [rows] the rows' minima
  double *m2 = m1 + N1;                               // [rows] their second minima (+inf: one destination)
  double *wl = m2 + N1;                               // [rows] the rows' workloads
  double *ocs = wl + N1;                              // [rows] kobj w
  int32_t *oj = reinterpret_cast<int32_t *>(ocs + N1);   // [K] open destinations, ascending
  int32_t *kof = oj + N1;                             // [N] j -> its place in oj, -1 closed
  int32_t *kk = kof + N1;                             // [rows] the rows' argmin (place in oj)
  int32_t *srcs = kk + N1;                            // [rows] the rows' sources
  int32_t *ksh = srcs + N1;                           // K
  const uint8_t *open = v.open + ((size_t)b * v.F + f) * N;
  const double *y = v.y + (size_t)b * N, *cprf = v.cpr + (size_t)f * N;
  if (tid < 64) {   // the open list, in chunks of 64 destinations
    const int cnt = leaf_open_list(open, y, cprf, N, lane, oj, yc, kof);
    if (lane == 0) *ksh = cnt;
  }
  __syncthreads();
  const int K = *ksh;
  const int r0 = v.frow[f], r1 = v.frow[f + 1];
  const bool pooled = r1 > r0 && v.row_src[r1 - 1] < 0;
  const int nl = K > 0 ? r1 - r0 - (pooled ? 1 : 0) : 0;   // loaded rows; at most N
  leaf_row_minima(v, f, K, r0, nl, oj, yc, m1, m2, wl, ocs, kk, srcs);
  __syncthreads();
  double *table = v.share + ((size_t)b * v.F + f) * N;
  for (int j = tid; j < N; j += blockDim.x) {
    const int k = kof[j];
    double s = 0.0;
    if (k < 0) {   // closed: the rows that are cheaper at j
      const double ycj = y[j] * cprf[j];
      const double *Dj = v.D + j;
      for (int row = 0; row < nl; ++row) {
        const double c = ocs[row] * Dj[(size_t)srcs[row] * N] + wl[row] * ycj;
        const double d = m1[row] - c;
        s += d > 0.0 ? d : 0.0;
      }
      s = 0.0 - s;
    } else if (K == 1) {
      s = INFINITY;
    } else {       // open: its rows fall back to their second choice
      for (int row = 0; row < nl; ++row) s += kk[row] == k ? m2[row] - m1[row] : 0.0;
    }
    table[j] = s;
  }
  if (tid < 64) {   // the function's part of L(y), in leaf_assign's order
    const double s = leaf_rows_sum(m1, nl, lane);
    if (lane == 0) v.fpart[(size_t)b * v.F + f] = s;
  }
}

// the priced table of a chunk of v.B placements on s: v.open and v.y hold the placements and prices; v.share gets
// table [B][F][N], v.fpart the functions' summed minima.  `threads`: leaf_assign's workgroup
hipError_t launch_leaf_moves(const LeafView &v, int threads, hipStream_t s) {
  hipLaunchKernelGGL(leaf_moves, dim3(v.F, v.B), dim3(threads), leaf_moves_lds(v.N), s, v);
  return hipGetLastError();
}

}  // namespace nep
