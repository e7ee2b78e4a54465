// nep_leaf_heur.hip — the per-round repair of the fixed-placement evaluator on the device (nep_leaf_eval_ex with
// repair_every >= 1; DESIGN.md §7 "Fixed-placement evaluator") for gfx950.  Every price round ends in an assignment that
// pushes load off congested nodes; repairing those as well as round 0's and keeping the cheapest point is the upper-bound
// half of a Lagrangian heuristic.  The device decides only WHICH round's assignment is worth a host repair: per
// placement it keeps the smallest objective a round's repair ended with, that round's number and copies of its
// assignment and loads; the host then runs its fp64-verified repair (nep_leaf_repair.cpp) from those.
//
// The rules are nep_leaf_repair.cpp's steps 1 and 2 (tests/leaf_heur_ref.py is the mirror), with the host's
// expressions in the host's order and fp contraction off, so both make the same moves.  A row only ever gives flow away
// from its own assigned node, and a destination is never filled past its target, so a node that received flow is never
// processed as overloaded; the state of a repair is therefore the flow left per row at asg[r], the per-(f, j) column
// counts (in the chunk's `share` buffer, dead between leaf_node and the next leaf_assign), room[f] and cpu[j] (from the
// bits leaf_node wrote).  No entries are produced: a verdict and the objective (the assignment's cost plus
// t oc (D[i, jd] - D[i, j]) per move).
//
//   leaf_open_lists    grid (F, B), once per chunk: the open destinations per function, ascending; the per-placement
//                      results reset
//   leaf_repair_count  grid (F, B), per repaired round: the column counts of f, flow = 1 on its loaded rows, room[f]
//                      (the deficits summed in ascending j, as the host does) and the assignment's cost over f's rows
//   leaf_repair_dev    one workgroup per placement: the overloaded nodes in ascending j, their row lists from one
//                      counting pass over asg, the move loop, the pooled rows' test, the selection
// A move's search runs over (row on node j) x (open destination of its function): rows take 64 lanes each while the
// node has few, down to a lane per row; the argmin of the key (score, row, destination) is the host's tie rule, so the
// order of the reduction (and of the row lists, filled with integer atomics) does not show in the result.
// Every loop is bounded by N, F, R or kLeafDevMoves: a round that needs more moves, or a move that does not shrink its
// node's excess, ends as "no point this round".
#include <hip/hip_runtime.h>

#include <climits>

#include "nep_launch.h"
#include "nep_leaf.h"

namespace nep {

namespace {

__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block sum in a fixed order (as nep_leaf.hip's): strided partials, a butterfly per wave, the waves in order
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

__device__ __forceinline__ bool key_less(double s, int r, int jd, double bs, int br, int bjd) {
  return s < bs || (s == bs && (r < br || (r == br && jd < bjd)));
}

}  // namespace

__global__ void leaf_open_lists(LeafView v, LeafHeurView h) {
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, lane = threadIdx.x;
  const uint8_t *open = v.open + ((size_t)b * v.F + f) * N;
  uint16_t *opl = h.opl + ((size_t)b * v.F + f) * N;
  int cnt = 0;
  for (int base = 0; base < N; base += 64) {
    const int j = base + lane;
    const bool o = j < N && open[j] != 0;
    const unsigned long long m = __ballot(o);
    if (o) opl[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)j;
    cnt += __popcll(m);
  }
  if (lane == 0) h.opn[(size_t)b * v.F + f] = cnt;
  if (f == 0) {
    for (int rd = lane; rd <= h.rounds; rd += 64) h.round_upper[(size_t)b * (h.rounds + 1) + rd] = INFINITY;
    if (lane == 0) h.best[b] = LeafHeurBest{INFINITY, -1, 0};
  }
}

__global__ void leaf_repair_count(LeafView v, LeafHeurView h, const int32_t *asg_in) {
#pragma clang fp contract(off)
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, tid = threadIdx.x;
  if (v.ctrl[b].done) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  __shared__ double red[4];
  int32_t *cnt = reinterpret_cast<int32_t *>(lds_raw);   // [N] rows of f by destination
  for (int j = tid; j < N; j += blockDim.x) cnt[j] = 0;
  __syncthreads();
  const int K = h.opn[(size_t)b * v.F + f];
  const int r0 = v.frow[f], r1 = v.frow[f + 1];
  const bool pooled = r1 > r0 && v.row_src[r1 - 1] < 0;
  const int nl = K > 0 ? r1 - r0 - (pooled ? 1 : 0) : 0;
  const int32_t *asg = asg_in + (size_t)b * v.R + r0;
  double *flow = h.flow + (size_t)b * v.R + r0;
  double c = 0.0;
  for (int row = tid; row < nl; row += blockDim.x) {
    const int j = asg[row], src = v.row_src[r0 + row];
    flow[row] = 1.0;
    if ((unsigned)j < (unsigned)N) {
      atomicAdd(&cnt[j], 1);
      c += (v.kobj * v.W[(size_t)f * N + src]) * v.D[(size_t)src * N + j];
    }
  }
  c = block_sum_fixed(c, red);
  double *col = v.share + ((size_t)b * v.F + f) * N;
  for (int j = tid; j < N; j += blockDim.x) col[j] = (double)cnt[j];
  if (tid == 0) {
    const uint16_t *opl = h.opl + ((size_t)b * v.F + f) * N;
    double def = 0.0;
    for (int k = 0; k < K; ++k) def += fmax(0.0, h.floor_ - (double)cnt[opl[k]]);
    const double mf = pooled ? (double)(N - (r1 - r0 - 1)) : 0.0;
    h.room[(size_t)b * v.F + f] = mf - def;
    h.fcost[(size_t)b * v.F + f] = c;
  }
}

// dynamic LDS of leaf_repair_dev
size_t leaf_repair_lds(int N) { return (size_t)N * (sizeof(double) + 4 * sizeof(int32_t)) + 16; }

__global__ __launch_bounds__(kLeafThreads) void leaf_repair_dev(LeafView v, LeafHeurView h, const int32_t *asg_in,
                                                                int rd) {
#pragma clang fp contract(off)   // (the moves compare the same roundings as the host repair and the fp64 mirror)
  const int b = blockIdx.x, N = v.N, F = v.F, R = v.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (v.ctrl[b].done) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double *cpu = reinterpret_cast<double *>(lds_raw);     // [N] CPU load by node
  int32_t *ovl = reinterpret_cast<int32_t *>(cpu + N);   // [nov] the overloaded nodes, ascending
  int32_t *ovpos = ovl + N;                              // [N] j -> its place in ovl, -1 not overloaded
  int32_t *cur = ovpos + N;                              // [nov] rows per overloaded node / fill cursor
  int32_t *ooff = cur + N;                               // [nov + 1] row list offsets
  __shared__ double red[4], sh_s[4];
  __shared__ int sh_r[4], sh_jd[4], sh_nov, sh_state;
  const int32_t *asg = asg_in + (size_t)b * R;
  const double *load = v.load + (size_t)b * N;
  double *col = v.share + (size_t)b * F * N, *room = h.room + (size_t)b * F, *flow = h.flow + (size_t)b * R;
  int32_t *nrows = h.nrows + (size_t)b * R;
  const uint16_t *opl = h.opl + (size_t)b * F * N;
  const int32_t *opn = h.opn + (size_t)b * F;
  const double floor_ = h.floor_;
  for (int j = tid; j < N; j += kLeafThreads) {
    cpu[j] = load[j];
    ovpos[j] = -1;
    cur[j] = 0;
  }
  __syncthreads();
  if (tid < 64) {
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
      const int j = base + lane;
      const bool o = j < N && cpu[j] > v.cores[j];
      const unsigned long long m = __ballot(o);
      if (o) {
        const int k = cnt + __popcll(m & ((1ull << lane) - 1ull));
        ovl[k] = j;
        ovpos[j] = k;
      }
      cnt += __popcll(m);
    }
    if (lane == 0) sh_nov = cnt;
  }
  double c = 0.0;
  for (int f = tid; f < F; f += kLeafThreads) c += h.fcost[(size_t)b * F + f];
  c = block_sum_fixed(c, red);   // (its barriers also publish ovl / ovpos / sh_nov)
  const int nov = sh_nov;
  double delta = 0.0;   // thread 0: the moves' cost
  int fail = 0;
  if (nov > 0) {
    // the rows of every overloaded node: count, offsets, fill
    for (int r = tid; r < R; r += kLeafThreads) {
      const int j = asg[r];
      if (v.row_src[r] >= 0 && (unsigned)j < (unsigned)N && ovpos[j] >= 0) atomicAdd(&cur[ovpos[j]], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int p = 0; p < nov; ++p) {
        ooff[p] = s;
        s += cur[p];
        cur[p] = 0;
      }
      ooff[nov] = s;
    }
    __syncthreads();
    for (int r = tid; r < R; r += kLeafThreads) {
      const int j = asg[r];
      if (v.row_src[r] >= 0 && (unsigned)j < (unsigned)N && ovpos[j] >= 0) {
        const int p = ovpos[j];
        nrows[ooff[p] + atomicAdd(&cur[p], 1)] = r;
      }
    }
    __syncthreads();
    int moves = 0;
    for (int q = 0; q < nov && !fail; ++q) {
      const int j = ovl[q], a = ooff[q], cnt = ooff[q + 1] - a;
      const double cores_j = v.cores[j];
      const double limj = cores_j - 1e-12 * fmax(1.0, fabs(cores_j));
      int lpr = 64;   // lanes per row
      while (lpr > 1 && cnt * lpr > kLeafThreads) lpr >>= 1;
      const int rp = kLeafThreads / lpr, slot = tid / lpr, k0 = tid % lpr;
      for (; moves < kLeafDevMoves; ++moves) {
        const double cj = cpu[j];
        if (!(cj > limj)) break;
        double bs = INFINITY;
        int br = INT_MAX, bjd = INT_MAX;
        for (int base = 0; base < cnt; base += rp) {
          const int idx = base + slot;
          if (idx >= cnt) continue;
          const int r = nrows[a + idx];
          const double vv = flow[r];
          if (!(vv > 0.0)) continue;
          const int f = h.row_f[r], i = v.row_src[r];
          const double w = v.W[(size_t)f * N + i];
          const double *cprf = v.cpr + (size_t)f * N, *Di = v.D + (size_t)i * N;
          const double relief = w * cprf[j];
          if (!(relief > 0.0)) continue;
          const double tsrc = fmin(vv, fmax(0.0, col[(size_t)f * N + j] - floor_) + fmax(0.0, room[f]));
          const double need = (cj - limj) / relief;
          const double oc = v.kobj * w, Dij = Di[j];
          const int K = opn[f];
          for (int k = k0; k < K; k += lpr) {
            const int jd = opl[(size_t)f * N + k];
            if (jd == j) continue;
            const double ld = w * cprf[jd];
            double t = fmin(tsrc, need);
            if (ld > 0.0) {
              const double cd = v.cores[jd];
              const double rm = (cd - 1e-12 * fmax(1.0, fabs(cd))) - cpu[jd];
              if (!(rm > 0.0)) continue;
              t = fmin(t, rm / ld);
            }
            if (!(t > 1e-15)) continue;
            const double s = oc * (Di[jd] - Dij) / relief;
            if (key_less(s, r, jd, bs, br, bjd)) { bs = s; br = r; bjd = jd; }
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double os = __shfl_xor(bs, o, 64);
          const int orr = __shfl_xor(br, o, 64), oj = __shfl_xor(bjd, o, 64);
          if (key_less(os, orr, oj, bs, br, bjd)) { bs = os; br = orr; bjd = oj; }
        }
        if (lane == 0) {
          sh_s[wave] = bs;
          sh_r[wave] = br;
          sh_jd[wave] = bjd;
        }
        __syncthreads();
        if (tid == 0) {
          for (int w = 1; w < kLeafThreads / 64; ++w)
            if (key_less(sh_s[w], sh_r[w], sh_jd[w], bs, br, bjd)) { bs = sh_s[w]; br = sh_r[w]; bjd = sh_jd[w]; }
          int state = 0;
          if (br == INT_MAX) {
            state = 1;   // no move left
          } else {
            const int r = br, jd = bjd, f = h.row_f[r], i = v.row_src[r];
            const double w = v.W[(size_t)f * N + i];
            const double *cprf = v.cpr + (size_t)f * N, *Di = v.D + (size_t)i * N;
            const double relief = w * cprf[j], vv = flow[r];
            double cjc = col[(size_t)f * N + j], cdc = col[(size_t)f * N + jd];
            const double tsrc = fmin(vv, fmax(0.0, cjc - floor_) + fmax(0.0, room[f]));
            const double need = (cj - limj) / relief;
            const double oc = v.kobj * w, ld = w * cprf[jd];
            double t = fmin(tsrc, need);
            if (ld > 0.0) {
              const double cd = v.cores[jd];
              const double rm = (cd - 1e-12 * fmax(1.0, fabs(cd))) - cpu[jd];
              t = fmin(t, rm / ld);
            }
            const double d0 = fmax(0.0, floor_ - cjc) + fmax(0.0, floor_ - cdc);
            flow[r] = t >= vv ? 0.0 : vv - t;
            const double cnew = cj - t * relief;
            cpu[j] = cnew;
            cpu[jd] += t * ld;
            cjc -= t;
            cdc += t;
            col[(size_t)f * N + j] = cjc;
            col[(size_t)f * N + jd] = cdc;
            room[f] -= fmax(0.0, floor_ - cjc) + fmax(0.0, floor_ - cdc) - d0;
            delta += t * (oc * (Di[jd] - Di[j]));
            if (!(cnew < cj)) state = 1;   // the excess did not shrink
          }
          sh_state = state;
        }
        __syncthreads();
        if (sh_state) {
          fail = 1;
          break;
        }
      }
      if (!fail && cpu[j] > limj) fail = 1;   // the move cap
    }
  }
  // the pooled rows pay the column deficits (ascending destination, as the host)
  int bad = fail;
  if (!fail) {
    for (int f = tid; f < F; f += kLeafThreads) {
      const int K = opn[f], r0 = v.frow[f], r1 = v.frow[f + 1];
      const bool pooled = r1 > r0 && v.row_src[r1 - 1] < 0;
      const uint16_t *op = opl + (size_t)f * N;
      const double *cf = col + (size_t)f * N;
      if (K == 0) {
        bad = 1;
      } else if (!pooled) {
        for (int k = 0; k < K; ++k)
          if (fmax(0.0, floor_ - cf[op[k]]) > 1e-12) bad = 1;
      } else {
        const double m = (double)(N - (r1 - r0 - 1));
        double rest = 1.0;
        for (int k = 1; k < K; ++k) {
          const double d = fmax(0.0, floor_ - cf[op[k]]);
          if (d > 0.0) rest -= d / m;
        }
        if (rest * m < fmax(0.0, floor_ - cf[op[0]])) bad = 1;
      }
    }
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    const double obj = v.ctrl[b].base + c + delta;
    LeafHeurBest &best = h.best[b];
    int better = 0;
    if (!bad) {
      h.round_upper[(size_t)b * (h.rounds + 1) + rd] = obj;
      if (obj < best.obj) {   // (strict: the earliest round wins)
        best.obj = obj;
        best.round = rd;
        better = 1;
      }
    }
    sh_state = better;
  }
  __syncthreads();
  if (sh_state) {
    for (int r = tid; r < R; r += kLeafThreads) h.asgrep[(size_t)b * R + r] = asg[r];
    for (int j = tid; j < N; j += kLeafThreads) h.loadrep[(size_t)b * N + j] = load[j];
  }
}

// once per chunk, before the rounds
hipError_t launch_leaf_heur_init(const LeafView &v, const LeafHeurView &h, hipStream_t s) {
  hipLaunchKernelGGL(leaf_open_lists, dim3(v.F, v.B), dim3(64), 0, s, v, h);
  return hipGetLastError();
}

// the repair of round rd's assignment, after leaf_node and before leaf_step
hipError_t launch_leaf_repair(const LeafView &v, const LeafHeurView &h, int rd, hipStream_t s) {
  const int32_t *asg = rd == 0 ? v.asg0 : v.asg;
  hipLaunchKernelGGL(leaf_repair_count, dim3(v.F, v.B), dim3(kLeafThreads), (size_t)v.N * sizeof(int32_t), s, v, h,
                     asg);
  hipLaunchKernelGGL(leaf_repair_dev, dim3(v.B), dim3(kLeafThreads), leaf_repair_lds(v.N), s, v, h, asg, rd);
  return hipGetLastError();
}

}  // namespace nep
