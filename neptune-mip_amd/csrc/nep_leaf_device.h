// nep_leaf_device.h — device helpers shared by the fixed-placement evaluator's kernels (nep_leaf.hip) and the priced
// moves (nep_leaf_moves.hip): both build the same open list and sum a function's row minima in the same order, which is
// what makes nep_leaf_moves' lagr the evaluator's round-0 lower.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace nep
