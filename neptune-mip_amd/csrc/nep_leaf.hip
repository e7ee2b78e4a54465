// nep_leaf.hip — device rounds of the fixed-placement evaluator (nep_leaf_eval; DESIGN.md §7 "Fixed-placement
// evaluator") for gfx950.  A leaf fixes every c and n; with the CPU rows C5 priced by y >= 0 (and the column floors C2
// dropped) every loaded routing row goes to its cheapest open destination:
//
//   L(y) = cost_n sum n + sum_rows min_{j open for f} (oc_r D[src_r, j] + w_r (y_j cpr[f, j])) - sum_j y_j cores_j
//
// One round is three launches over a chunk of B placements, fp64 throughout, reading the instance's fp64 D / W / cpr:
//   leaf_assign  grid (F, B): the function's open list (ascending j) and its priced CPU terms y_j cpr[f, j] in LDS; the
//                rows of f a lane per row looping the K open destinations (K <= kLeafLaneK) or a wave per row; argmin
//                ties to the lowest j; then the load share of every (f, open j) summed over the rows in row order and
//                the rows' minima summed in a fixed order
//   leaf_node    per node: the functions' shares summed in ascending f, the subgradient g_j = load_j - cores_j (0 where
//                y_j = 0 and g_j < 0)
//   leaf_step    per placement: L, the best bound and its prices, the cutoff test, the step (nep_leaf.h) and
//                y <- max(0, y + theta g)
// (nep_leaf_eval_ex with repair_every >= 1 adds, between leaf_node and leaf_step of the selected rounds, the repair of
// the round's assignment: nep_leaf_heur.hip.)
// The rounds of a call are enqueued back to back; a placement that is cut off, or whose subgradient vanished (its
// prices are optimal), sets `done` and its blocks return at once in later rounds.  No atomics: every sum has a fixed
// order, so two calls on the same input return the same bits.  The working set (D, W, cpr, a chunk's shares) is L2
// resident; the kernels are bound by gather latency, so the workgroup is sized to the rows of a function (64 to 256
// threads) and many workgroups share a CU.
#include <hip/hip_runtime.h>

#include "nep_launch.h"
#include "nep_leaf.h"
#include "nep_leaf_device.h"

namespace nep {

namespace {

// block sum in a fixed order: per-thread strided partials (the caller's), a butterfly per wave, the waves in order
__device__ __forceinline__ double block_sum_fixed(double v, double *red /* [4] LDS */) {
  v = wave_sum_fixed(v);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

}  // namespace

// dynamic LDS of leaf_assign for rows of N destinations (a function has at most N + 1 rows)
size_t leaf_assign_lds(int N) { return (size_t)(N + 1) * (3 * sizeof(double) + 3 * sizeof(int32_t)) + 16; }

__global__ void leaf_assign(LeafView v, int32_t *asg_out) {
#pragma clang fp contract(off)   // (the argmin compares the same roundings as the fp64 mirror)
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, tid = threadIdx.x, lane = tid & 63;
  if (v.ctrl[b].done) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int N1 = N + 1;
  double *yc = reinterpret_cast<double *>(lds_raw);   // [K] y_j cpr[f, j] of the open destinations
  double *vmin = yc + N1;                             // [rows] the rows' minima
  double *wl = vmin + N1;                             // [rows] the rows' workloads
  int32_t *oj = reinterpret_cast<int32_t *>(wl + N1);   // [K] open destinations, ascending
  int32_t *kof = oj + N1;                             // [N] j -> its place in oj, -1 closed
  int32_t *kk = kof + N1;                             // [rows] the rows' argmin (place in oj)
  int32_t *ksh = kk + N1;                             // K
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
  const int nl = K > 0 ? r1 - r0 - (pooled ? 1 : 0) : 0;   // loaded rows (a function without a destination: none)
  int32_t *asg = asg_out + (size_t)b * v.R + r0;
  if (K <= kLeafLaneK) {
    for (int row = tid; row < nl; row += blockDim.x) {
      const int src = v.row_src[r0 + row];
      const double w = v.W[(size_t)f * N + src], oc = v.kobj * w;
      const double *Dr = v.D + (size_t)src * N;
      double best = oc * Dr[oj[0]] + w * yc[0];
      int kb = 0;
      for (int k = 1; k < K; ++k) {
        const double c = oc * Dr[oj[k]] + w * yc[k];
        if (c < best) { best = c; kb = k; }
      }
      vmin[row] = best;
      wl[row] = w;
      kk[row] = kb;
      asg[row] = oj[kb];
    }
  } else {
    const int wave = tid >> 6, nw = blockDim.x >> 6;
    for (int row = wave; row < nl; row += nw) {
      const int src = v.row_src[r0 + row];
      const double w = v.W[(size_t)f * N + src], oc = v.kobj * w;
      const double *Dr = v.D + (size_t)src * N;
      double best = INFINITY;
      int kb = 0x7fffffff;
      for (int k = lane; k < K; k += 64) {
        const double c = oc * Dr[oj[k]] + w * yc[k];
        if (c < best) { best = c; kb = k; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(kb, o, 64);
        if (ov < best || (ov == best && ok < kb)) { best = ov; kb = ok; }
      }
      if (lane == 0) {
        vmin[row] = best;
        wl[row] = w;
        kk[row] = kb;
        asg[row] = oj[kb];
      }
    }
  }
  if (tid == 0 && pooled) asg_out[(size_t)b * v.R + r1 - 1] = -1;
  __syncthreads();
  // the load share of (f, j): the workloads of the rows sent to j, in row order, times cpr[f, j]
  double *share = v.share + ((size_t)b * v.F + f) * N;
  for (int j = tid; j < N; j += blockDim.x) {
    const int k = kof[j];
    double s = 0.0;
    if (k >= 0)
      for (int row = 0; row < nl; ++row) s += kk[row] == k ? wl[row] : 0.0;
    share[j] = s * cprf[j];
  }
  if (tid < 64) {
    const double s = leaf_rows_sum(vmin, nl, lane);
    if (lane == 0) v.fpart[(size_t)b * v.F + f] = s;
  }
}

__global__ void leaf_node(LeafView v) {
  const int b = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (v.ctrl[b].done || j >= v.N) return;
  const double *share = v.share + (size_t)b * v.F * v.N + j;
  double load = 0.0;
  for (int f = 0; f < v.F; ++f) load += share[(size_t)f * v.N];
  double g = load - v.cores[j];
  if (v.y[(size_t)b * v.N + j] == 0.0 && g < 0.0) g = 0.0;
  v.load[(size_t)b * v.N + j] = load;
  v.g[(size_t)b * v.N + j] = g;
}

__global__ void leaf_step(LeafView v, int last) {
  const int b = blockIdx.x, N = v.N, tid = threadIdx.x;
  LeafCtrl &c = v.ctrl[b];
  if (c.done) return;
  __shared__ double red[4];
  __shared__ double sh_theta;
  __shared__ int sh_better, sh_move;
  double *y = v.y + (size_t)b * N;
  const double *g = v.g + (size_t)b * N;
  double sf = 0.0, sy = 0.0, gg = 0.0;
  for (int f = tid; f < v.F; f += blockDim.x) sf += v.fpart[(size_t)b * v.F + f];
  for (int j = tid; j < N; j += blockDim.x) {
    sy += y[j] * v.cores[j];
    gg += g[j] * g[j];
  }
  sf = block_sum_fixed(sf, red);
  sy = block_sum_fixed(sy, red);
  gg = block_sum_fixed(gg, red);
  if (tid == 0) {
    const double L = c.base + sf - sy;
    int better = 0, move = 0;
    if (L > c.best) {
      c.best = L;
      c.stall = 0;
      better = 1;
    } else if (++c.stall >= kLeafStall) {
      c.lam *= 0.5;
      c.stall = 0;
    }
    double theta = 0.0;
    if (c.best >= c.cutoff) {
      c.cut = 1;
      c.done = 1;
    } else if (gg == 0.0) {
      c.done = 1;
    } else if (!last) {
      const double target =
          c.cutoff < INFINITY
              ? c.cutoff
              : c.best + kLeafMargin * fmax(fabs(c.best - c.base), kLeafMarginFloor * fmax(1.0, fabs(c.best)));
      theta = c.lam * (target - L) / gg;
      move = 1;
    }
    sh_theta = theta;
    sh_better = better;
    sh_move = move;
  }
  __syncthreads();
  const double theta = sh_theta;
  const bool better = sh_better != 0, move = sh_move != 0;
  double *yb = v.ybest + (size_t)b * N;
  for (int j = tid; j < N; j += blockDim.x) {
    const double yj = y[j];
    if (better) yb[j] = yj;
    if (move) y[j] = fmax(0.0, yj + theta * g[j]);
  }
}

// the rounds 0 .. rounds of a chunk, back to back on s; `threads`: leaf_assign's workgroup (64, 128 or 256); heur (or
// nullptr): the per-round repair of nep_leaf_heur.hip, serial in the round between leaf_node and leaf_step
hipError_t launch_leaf_rounds(const LeafView &v, int rounds, int threads, hipStream_t s, const LeafHeurView *heur) {
  const size_t lds = leaf_assign_lds(v.N);
  if (heur) {
    const hipError_t e = launch_leaf_heur_init(v, *heur, s);
    if (e != hipSuccess) return e;
  }
  for (int rd = 0; rd <= rounds; ++rd) {
    hipLaunchKernelGGL(leaf_assign, dim3(v.F, v.B), dim3(threads), lds, s, v, rd == 0 ? v.asg0 : v.asg);
    hipLaunchKernelGGL(leaf_node, dim3((v.N + 255) / 256, v.B), dim3(256), 0, s, v);
    if (heur && ((rd > 0 && rd % heur->every == 0) || rd == rounds)) {
      const hipError_t e = launch_leaf_repair(v, *heur, rd, s);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(leaf_step, dim3(v.B), dim3(kLeafThreads), 0, s, v, rd == rounds ? 1 : 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace nep
