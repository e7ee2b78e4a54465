// nep_leaf_device.h — device helpers shared by the fixed-placement evaluator's kernels (nep_leaf.hip) and the priced
// moves and swaps (nep_leaf_moves.hip, nep_leaf_swaps.hip): all build the same open list and sum a function's row minima
// in the same order, which is what makes nep_leaf_moves' lagr the evaluator's round-0 lower; the two pricing kernels
// share their first phase, the rows' first and second minima.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nep_leaf.h"

namespace nep {

__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The open list of one function, built by one full wave (lane = its lane) in chunks of 64 destinations: oj [K] the open
// destinations in ascending order, yc [K] their priced CPU terms y_j cpr[f, j], kof [N] j -> its place in oj (-1:
// closed).  Returns K (in every lane).
__device__ __forceinline__ int leaf_open_list(const uint8_t *open, const double *y, const double *cprf, int N, int lane,
                                              int32_t *oj, double *yc, int32_t *kof) {
#pragma clang fp contract(off)
  int cnt = 0;
  for (int base = 0; base < N; base += 64) {
    const int j = base + lane;
    const bool o = j < N && open[j] != 0;
    const unsigned long long m = __ballot(o);
    const int k = cnt + __popcll(m & ((1ull << lane) - 1ull));
    if (o) {
      oj[k] = j;
      yc[k] = y[j] * cprf[j];
    }
    if (j < N) kof[j] = o ? k : -1;
    cnt += __popcll(m);
  }
  return cnt;
}

// a function's summed row minima in leaf_assign's order: 64 strided partials, then the butterfly (one full wave)
__device__ __forceinline__ double leaf_rows_sum(const double *vmin, int nl, int lane) {
  double s = 0.0;
  for (int row = lane; row < nl; row += 64) s += vmin[row];
  return wave_sum_fixed(s);
}

// Phase 1 of the pricing kernels, by the whole workgroup: per loaded row of f (row = 0 .. nl) its minimum m1 over the K
// open destinations oj (yc: their priced CPU terms), the minimum's place kk in oj (ties to the lowest), the second
// minimum m2 (+inf: K = 1), its workload wl, objective scale ocs = kobj w (nullptr: not kept) and source srcs.  A lane
// per row while K <= kLeafLaneK, else a wave per row and a butterfly over (value, index, second value).
__device__ __forceinline__ void leaf_row_minima(const LeafView &v, int f, int K, int r0, int nl, const int32_t *oj,
                                                const double *yc, double *m1, double *m2, double *wl, double *ocs,
                                                int32_t *kk, int32_t *srcs) {
#pragma clang fp contract(off)   // (rho rounds as in leaf_assign and the fp64 mirror)
  const int N = v.N, tid = threadIdx.x, lane = tid & 63;
  if (K <= kLeafLaneK) {
    for (int row = tid; row < nl; row += blockDim.x) {
      const int src = v.row_src[r0 + row];
      const double w = v.W[(size_t)f * N + src], oc = v.kobj * w;
      const double *Dr = v.D + (size_t)src * N;
      double best = oc * Dr[oj[0]] + w * yc[0], second = INFINITY;
      int kb = 0;
      for (int k = 1; k < K; ++k) {
        const double c = oc * Dr[oj[k]] + w * yc[k];
        if (c < best) {
          second = best;
          best = c;
          kb = k;
        } else if (c < second) {
          second = c;
        }
      }
      m1[row] = best;
      m2[row] = second;
      wl[row] = w;
      if (ocs) ocs[row] = oc;
      kk[row] = kb;
      srcs[row] = src;
    }
  } else {
    const int wave = tid >> 6, nw = blockDim.x >> 6;
    for (int row = wave; row < nl; row += nw) {
      const int src = v.row_src[r0 + row];
      const double w = v.W[(size_t)f * N + src], oc = v.kobj * w;
      const double *Dr = v.D + (size_t)src * N;
      double best = INFINITY, second = INFINITY;
      int kb = 0x7fffffff;
      for (int k = lane; k < K; k += 64) {
        const double c = oc * Dr[oj[k]] + w * yc[k];
        if (c < best) {
          second = best;
          best = c;
          kb = k;
        } else if (c < second) {
          second = c;
        }
      }
      // (value, index, second) butterfly: the loser's best is a candidate for the second minimum; minima are exact,
      // so the result does not depend on the order of the merges
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64), os = __shfl_xor(second, o, 64);
        const int ok = __shfl_xor(kb, o, 64);
        if (ov < best || (ov == best && ok < kb)) {
          second = fmin(best, os);
          best = ov;
          kb = ok;
        } else {
          second = fmin(second, ov);
        }
      }
      if (lane == 0) {
        m1[row] = best;
        m2[row] = second;
        wl[row] = w;
        if (ocs) ocs[row] = oc;
        kk[row] = kb;
        srcs[row] = src;
      }
    }
  }
}

}  // namespace nep
