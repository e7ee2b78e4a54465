// nep_leaf_swaps.hip — priced swap moves of a fixed placement, selected on the device (nep_leaf_swaps; DESIGN.md §7
// "Priced swaps") for gfx950.  SWAP (f, j -> j') moves function f from an open destination j to a closed one j'.  With
// rho_r, m1_r, k1_r (the place of the minimum in the open list oj) and m2_r as in nep_leaf_moves.hip, and bucket k the
// loaded rows of f with k1_r = k in ascending row order,
//
//   A_k(j') = sum_{r in bucket k} (min(m1_r, rho_r(j')) - m1_r)     the rows that j' takes while oj[k] stays open
//   S_k(j') = sum_{r in bucket k} (min(m2_r, rho_r(j')) - m1_r)     the same once oj[k] has closed
//   A_tot   = sum_k A_k, ascending k
//   g_k     = (S_k - A_k) - cost_n [node oj[k] holds only this placement]
//   delta(f, k, j') = (A_tot + g_k) + cost_n [node j' holds none]
//
// finite even for a function with one destination.  Per (f, j') the best source is the k of the smallest g_k (ties to
// the lowest k).  j' is admissible under leaf_move_list's ADD screens (the node's memory holds f as well; a node that
// opens is within the budget); every other entry is +inf.  One launch per chunk of placements, grid (F, B):
//   phase 1  leaf_moves' (nep_leaf_device.h): the open list, then m1 / k1 / m2 / workload / source per loaded row in LDS
//   sort     a thread per bucket scans k1 in ascending row order: the permutation and the bucket starts go where the
//            open list's priced CPU terms were (dead after phase 1)
//   phase 2  a thread per closed destination j', strided over N (reads of D[src_r, j'] are coalesced along j'), walks
//            the rows once in bucket order and keeps A_tot and the running best g_k; (delta, source) go to LDS
//   phase 3  per_fn block argmins over (delta, j') pick the function's cheapest swaps: per_fn records per (placement,
//            function) are all a caller without the tables reads back
// fp64, no contraction, no atomics, every sum in a fixed order: two calls return the same bits.  The functions' summed
// minima go to `fpart` as in leaf_moves and, when asked for, the [F][N] tables to `share` and a buffer of the call's
// own; nothing of LeafCtrl is read or written.
#include <hip/hip_runtime.h>

#include "nep_launch.h"
#include "nep_leaf.h"
#include "nep_leaf_device.h"

namespace nep {

// dynamic LDS of leaf_swaps: leaf_moves' size, array for array (the objective scales' place holds the deltas)
size_t leaf_swaps_lds(int N) {
  return (size_t)(N + 1) * (5 * sizeof(double) + 4 * sizeof(int32_t)) + 16;
}

__global__ void leaf_swaps(LeafView v, LeafSwapView sv) {
#pragma clang fp contract(off)   // (rho rounds as in leaf_assign and the fp64 mirror)
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, tid = threadIdx.x, lane = tid & 63;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int N1 = N + 1;
  double *yc = reinterpret_cast<double *>(lds_raw);   // [K] y_j cpr[f, j] of the open destinations (phase 1)
  double *m1 = yc + N1;                               // [rows] the rows' minima
  double *m2 = m1 + N1;                               // [rows] their second minima (+inf: one destination)
  double *wl = m2 + N1;                               // [rows] the rows' workloads
  double *dl = wl + N1;                               // [N] delta of the best swap into j' (+inf: none)
  int32_t *oj = reinterpret_cast<int32_t *>(dl + N1);   // [K] open destinations, ascending
  int32_t *kof = oj + N1;                             // [N] j -> its place in oj (phase 1), then:
  int32_t *kk = kof + N1;                             // [rows] the rows' argmin (place in oj), then:
  int32_t *srcs = kk + N1;                            // [rows] the rows' sources
  int32_t *ksh = srcs + N1;                           // K
  int32_t *perm = reinterpret_cast<int32_t *>(yc);    // [rows] after phase 1: the rows in bucket order
  int32_t *bst = perm + N;                            // [K + 1] the buckets' starts in perm
  int32_t *sgl = kof;                                 // [K] after phase 1: node oj[k] holds one placement
  int32_t *dk = kk;                                   // [N] after the sort: the best source of j' (place in oj)
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
  leaf_row_minima(v, f, K, r0, nl, oj, yc, m1, m2, wl, nullptr, kk, srcs);
  __syncthreads();
  // the bucket sort: bucket k starts after the rows of the buckets before it; its rows in ascending order
  const int32_t *ncnt = sv.ncnt + (size_t)b * N;
  for (int k = tid; k <= K; k += blockDim.x) {
    int at = 0;
    for (int row = 0; row < nl; ++row) at += kk[row] < k ? 1 : 0;
    bst[k] = at;
    if (k < K) {
      for (int row = 0; row < nl; ++row)
        if (kk[row] == k) perm[at++] = row;
      sgl[k] = ncnt[oj[k]] == 1 ? 1 : 0;
    }
  }
  __syncthreads();
  const double *mem = sv.mem + (size_t)b * N;
  const double fm = sv.fmem[f];
  double *tab = sv.best ? sv.best + ((size_t)b * v.F + f) * N : nullptr;
  int32_t *tabk = sv.best_from ? sv.best_from + ((size_t)b * v.F + f) * N : nullptr;
  for (int j = tid; j < N; j += blockDim.x) {
    const int c = ncnt[j];
    double d = INFINITY;
    int kb = -1;
    if (K > 0 && open[j] == 0 && c >= 0 && mem[j] + fm <= sv.nmem1[j]) {
      const double ycj = y[j] * cprf[j];
      const double *Dj = v.D + j;
      double atot = 0.0, g = INFINITY;
      for (int k = 0; k < K; ++k) {
        double ak = 0.0, sk = 0.0;
        const int q1 = bst[k + 1];
        for (int q = bst[k]; q < q1; ++q) {
          const int row = perm[q];
          const double w = wl[row], a = m1[row], s = m2[row];
          const double rho = (v.kobj * w) * Dj[(size_t)srcs[row] * N] + w * ycj;
          ak += (rho < a ? rho : a) - a;
          sk += (rho < s ? rho : s) - a;
        }
        atot += ak;
        const double gk = (sk - ak) - (sgl[k] ? sv.cn : 0.0);
        if (gk < g) {
          g = gk;
          kb = k;
        }
      }
      d = (atot + g) + (c == 0 ? sv.cn : 0.0);
    }
    dl[j] = d;
    dk[j] = kb;
    if (tab) tab[j] = d;
    if (tabk) tabk[j] = kb >= 0 ? oj[kb] : -1;
  }
  if (tid < 64) {   // the function's part of L(y), in leaf_assign's order
    const double s = leaf_rows_sum(m1, nl, lane);
    if (lane == 0) v.fpart[(size_t)b * v.F + f] = s;
  }
  __syncthreads();
  // the per_fn cheapest (delta, j'): a block argmin per pick; the waves' candidates meet where m1 / m2 were
  double *wd = m1;
  int32_t *wj = reinterpret_cast<int32_t *>(m2);
  const int wave = tid >> 6, nw = blockDim.x >> 6;
  LeafSwapRec *rec = sv.rec + ((size_t)b * v.F + f) * sv.per_fn;
  for (int p = 0; p < sv.per_fn; ++p) {
    double d = INFINITY;
    int jb = 0x7fffffff;
    for (int j = tid; j < N; j += blockDim.x) {   // (ascending j per thread: a tie keeps the lower j)
      const double t = dl[j];
      if (t < d) {
        d = t;
        jb = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(d, o, 64);
      const int ojb = __shfl_xor(jb, o, 64);
      if (od < d || (od == d && ojb < jb)) {
        d = od;
        jb = ojb;
      }
    }
    if (lane == 0) {
      wd[wave] = d;
      wj[wave] = jb;
    }
    __syncthreads();
    d = wd[0];
    jb = wj[0];
    for (int q = 1; q < nw; ++q) {
      const double od = wd[q];
      const int ojb = wj[q];
      if (od < d || (od == d && ojb < jb)) {
        d = od;
        jb = ojb;
      }
    }
    if (tid == 0) {
      const bool has = d < INFINITY;
      rec[p].delta = has ? d : INFINITY;
      rec[p].from = has ? oj[dk[jb]] : -1;
      rec[p].to = has ? jb : -1;
      if (has) dl[jb] = INFINITY;
    }
    __syncthreads();
  }
}

// the priced swaps of a chunk of v.B placements on s: v.open and v.y hold the placements and prices, sv.ncnt and sv.mem
// the nodes' state; sv.rec gets the records, v.fpart the functions' summed minima.  `threads`: leaf_assign's workgroup
hipError_t launch_leaf_swaps(const LeafView &v, const LeafSwapView &sv, int threads, hipStream_t s) {
  hipLaunchKernelGGL(leaf_swaps, dim3(v.F, v.B), dim3(threads), leaf_swaps_lds(v.N), s, v, sv);
  return hipGetLastError();
}

}  // namespace nep
