// nep_leaf_search.hip — the device side of the native placement search (nep_leaf_search; DESIGN.md §7 "Native search")
// for gfx950.  The current placement (the base) lives in slot 0 of the evaluator's chunk; its neighbours are written
// beside it from move records, so no placement crosses to the device as z after the start.
//   leaf_search_expand  grid (F, B): row f of the base's c into neighbour b's slot with the move applied; the block of
//                       f = 0 also writes the neighbour's LeafCtrl and its starting prices
//   leaf_node_state     a thread per node: the base's placements per node and memory per node (LeafSwapView::ncnt / mem),
//                       summed over the functions in ascending order as nep_leaf_swaps' host staging sums them
//   leaf_search_adopt   grid (F + 1): the accepted neighbour's c and best prices into slot 0
// Copies and counts only: the one product (cost_n x open nodes) and the memory sums are single operations in a fixed
// order, no atomics, nothing that depends on scheduling: two calls return the same bits.
#include <hip/hip_runtime.h>

#include "nep_launch.h"
#include "nep_leaf.h"
#include "nep_leaf_search.h"

namespace nep {

constexpr int kLeafSearchThreads = 256;

// n bytes from src to dst by the whole workgroup.  Rows start at multiples of N bytes, so neither is aligned in general:
// 16-byte accesses where both addresses are 16-byte aligned at the same byte, single bytes before, after and otherwise
__device__ __forceinline__ void leaf_copy_bytes(uint8_t *dst, const uint8_t *src, int n) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
  const bool together = ((reinterpret_cast<uintptr_t>(src) + head) & 15u) == 0;
  if (!together || n < head + 16) {
    for (int k = tid; k < n; k += nt) dst[k] = src[k];
    return;
  }
  const int nv = (n - head) >> 4, tail = head + (nv << 4);
  for (int k = tid; k < head; k += nt) dst[k] = src[k];
  const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
  uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
  for (int k = tid; k < nv; k += nt) d4[k] = s4[k];
  for (int k = tail + tid; k < n; k += nt) dst[k] = src[k];
}

__global__ void leaf_search_expand(LeafView v, LeafSearchView s) {
  const int f = blockIdx.x, b = blockIdx.y, N = v.N, tid = threadIdx.x;
  const LeafSearchMove mv = s.mv[b];
  const uint8_t *src = s.base_open + (size_t)f * N;
  uint8_t *dst = const_cast<uint8_t *>(v.open) + ((size_t)b * v.F + f) * N;
  leaf_copy_bytes(dst, src, N);
  __syncthreads();   // (the row is in place before the move's one or two cells of it are rewritten)
  if (tid == 0 && (mv.kind == 2 || f == mv.fn)) {
    if (mv.kind == 3) dst[mv.src] = leaf_search_cell(mv, f, mv.src, src[mv.src]);
    dst[mv.node] = leaf_search_cell(mv, f, mv.node, src[mv.node]);
  }
  if (f != 0) return;
  double *y = v.y + (size_t)b * N, *yb = v.ybest + (size_t)b * N;
  for (int j = tid; j < N; j += blockDim.x) {
    const double p = s.warm ? s.base_y[j] : 0.0;
    y[j] = p;
    yb[j] = p;
  }
  if (tid == 0) {
    LeafCtrl c;
    c.base = s.cn * (double)mv.nopen;
    c.best = -INFINITY;
    c.lam = 1.0;
    c.cutoff = s.cutoff;
    c.stall = 0;
    c.done = 0;
    c.cut = 0;
    c.pad_ = 0;
    v.ctrl[b] = c;
  }
}

// over [N]: 1 where an empty node may not open (a variant with n whose node cost is beyond the budget)
__global__ void leaf_node_state(LeafView v, const double *fmem, const uint8_t *over, int32_t *ncnt, double *mem) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, N = v.N;
  if (j >= N) return;
  double m = 0.0;
  int cnt = 0;
  for (int f = 0; f < v.F; ++f)
    if (v.open[(size_t)f * N + j]) {
      m += fmem[f];
      ++cnt;
    }
  mem[j] = m;
  ncnt[j] = cnt == 0 && over[j] ? -1 : cnt;
}

__global__ void leaf_search_adopt(LeafView v, int from) {
  const int f = blockIdx.x, N = v.N;
  if (f < v.F) {
    leaf_copy_bytes(const_cast<uint8_t *>(v.open) + (size_t)f * N, v.open + ((size_t)from * v.F + f) * N, N);
    return;
  }
  const double *yb = v.ybest + (size_t)from * N;
  for (int j = threadIdx.x; j < N; j += blockDim.x) v.ybest[j] = yb[j];
}

// v: the view of the v.B neighbours' slots; s.mv their records; s.base_open / s.base_y the base's slot
hipError_t launch_leaf_search_expand(const LeafView &v, const LeafSearchView &s, hipStream_t st) {
  hipLaunchKernelGGL(leaf_search_expand, dim3(v.F, v.B), dim3(kLeafSearchThreads), 0, st, v, s);
  return hipGetLastError();
}

// v: the view of the base's slot; ncnt / mem [N] get its node state
hipError_t launch_leaf_node_state(const LeafView &v, const double *fmem, const uint8_t *over, int32_t *ncnt, double *mem,
                                  hipStream_t st) {
  hipLaunchKernelGGL(leaf_node_state, dim3((v.N + 255) / 256), dim3(256), 0, st, v, fmem, over, ncnt, mem);
  return hipGetLastError();
}

// v: the view of the whole chunk (the base in slot 0); from: the slot of the accepted neighbour (>= 1)
hipError_t launch_leaf_search_adopt(const LeafView &v, int from, hipStream_t st) {
  hipLaunchKernelGGL(leaf_search_adopt, dim3(v.F + 1), dim3(kLeafSearchThreads), 0, st, v, from);
  return hipGetLastError();
}

}  // namespace nep
