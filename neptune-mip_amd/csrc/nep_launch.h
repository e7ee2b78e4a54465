// nep_launch.h — the one declaration of every host-callable function a .hip file defines: the kernel launchers and
// the launch-shape queries the host runtime shares with them.  Included by the file that defines each function and
// by every caller, so a changed signature fails to compile instead of failing to link.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "nep_internal.h"
#include "nep_leaf.h"
#include "nep_leaf_search.h"

namespace nep {

// nep_kernels.hip — the PDHG iteration (either relaxation: a facility model goes on to nep_fac.hip)
hipError_t launch_x_pass(const DeviceView &v, const int32_t *slots, int nslots, bool check, bool init, bool first,
                         bool plain, int it, hipStream_t s, int policy_slots = 0);
int block_tile_waves(const DeviceView &v, int nslots, bool check);
int block_split(const DeviceView &v, int na);
hipError_t launch_node_pass(const DeviceView &v, const int32_t *slots, int nslots, bool check, bool init, bool first,
                            bool plain, int it, hipStream_t s);
hipError_t launch_scalar_pass(const DeviceView &v, const int32_t *slots, int nslots, bool check, bool init,
                              bool first, bool plain, int it, int block_len, hipStream_t s);
hipError_t launch_node_bounds(const DeviceView &v, const int32_t *slots, int nslots, const double *base_lb,
                              const double *base_ub, const uint8_t *base_mask, const int32_t *off, const int32_t *idx,
                              const double *cl, const double *cu, int max_chg, hipStream_t s);
hipError_t launch_init_slot(const DeviceView &v, const int32_t *slots, const int32_t *exact, int nslots, bool warm,
                            double eta, double omega0, const double *per, hipStream_t s);

// nep_fac.hip — the facility relaxation's passes (called by launch_x_pass / launch_node_pass / block_tile_waves)
int fac_block_tile_waves(const DeviceView &v, int nslots, bool check);   // (fac_tile_waves)
hipError_t launch_fac_x_pass(const DeviceView &v, const int32_t *slots, int nslots, bool check, bool init, bool first,
                             bool plain, int it, hipStream_t s, int policy_slots);
hipError_t launch_fac_node_pass(const DeviceView &v, const int32_t *slots, int nslots, bool check, bool init, bool first,
                                bool plain, int it, hipStream_t s);

// nep_aux.hip — work on finished slots
hipError_t launch_node_flows(const DeviceView &v, const int32_t *slots, int n, float *out, float *wout,
                             hipStream_t s);
hipError_t launch_compact_f32(const float *vals, int rows, int cols, int64_t ld, double thr, int round3,
                              int32_t *cnt, int32_t *off, int32_t *orow, int32_t *ocol, double *oval, bool count_only,
                              hipStream_t s);
hipError_t launch_compact_f64(const double *vals, int rows, int cols, int64_t ld, double thr, int round3,
                              int32_t *cnt, int32_t *off, int32_t *orow, int32_t *ocol, double *oval, bool count_only,
                              hipStream_t s);
hipError_t launch_copy_segments(const SlotCopy &c, hipStream_t s);
hipError_t launch_copy_slots(const SlotCopyN &c, hipStream_t s);
hipError_t launch_gather_reduced_costs(const DeviceView &v, const int32_t *slots, int n, int ni, double *out,
                                       double *bound, hipStream_t s);
hipError_t launch_rc_fixings(const DeviceView &v, int slot, double cutoff, int ni, int32_t *cnt, int32_t *off,
                             int32_t *oidx, double *oval, bool count_only, hipStream_t s);
hipError_t launch_gather_solutions(const DeviceView &v, const int32_t *slots, int n, int ni, double *out,
                                   hipStream_t s);
hipError_t launch_score_check(const DeviceView &v, int slot, const double *zi, double *cpu_fj, double *fpart,
                              double *jpart, const double *node_cost, double budget, double *out, hipStream_t s);

// nep_build.hip — the step size's power iteration
hipError_t launch_power_iteration(const DeviceView &v, int iters, double *zx, double *zs, double *gx, double *gs,
                                  double *y, double *upart, double *spart, double *gfac, double *part, int nblk,
                                  double *out, const int32_t *rp, const int32_t *ci, const double *cv,
                                  const int32_t *cp, const int32_t *ri, const double *rv, hipStream_t s);

// nep_leaf.hip, nep_leaf_heur.hip, nep_leaf_moves.hip, nep_leaf_swaps.hip — the fixed-placement evaluator; *_lds: a
// kernel's dynamic LDS
size_t leaf_assign_lds(int N);
hipError_t launch_leaf_rounds(const LeafView &v, int rounds, int threads, hipStream_t s, const LeafHeurView *heur);
size_t leaf_repair_lds(int N);
hipError_t launch_leaf_heur_init(const LeafView &v, const LeafHeurView &h, hipStream_t s);
hipError_t launch_leaf_repair(const LeafView &v, const LeafHeurView &h, int rd, hipStream_t s);
size_t leaf_moves_lds(int N);
hipError_t launch_leaf_moves(const LeafView &v, int threads, hipStream_t s);
size_t leaf_swaps_lds(int N);
hipError_t launch_leaf_swaps(const LeafView &v, const LeafSwapView &sv, int threads, hipStream_t s);

// nep_leaf_search.hip — the native placement search: the neighbours of the base (slot 0) from move records, the base's
// node state for the swap screens, the accepted neighbour into slot 0
hipError_t launch_leaf_search_expand(const LeafView &v, const LeafSearchView &s, hipStream_t st);
hipError_t launch_leaf_node_state(const LeafView &v, const double *fmem, const uint8_t *over, int32_t *ncnt, double *mem,
                                  hipStream_t st);
hipError_t launch_leaf_search_adopt(const LeafView &v, int from, hipStream_t st);

}  // namespace nep
