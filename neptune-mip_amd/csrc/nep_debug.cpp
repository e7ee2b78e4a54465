// nep_debug.cpp — the nep_debug_* entries of include/neptune_lp.h: device state read-outs and the host paths of the
// build, the presolve and the fixed-placement evaluator on a scratch model (the tests' windows into the engine).
#include "nep_model.h"

using namespace nep;

// The preamble of the entries that run a host path on a scratch model: host arrays only (who: the entry's name in the
// refusal), the build, and for the evaluator's entries (leaf) its model kinds only.
static int scratch_model(Model &m, const nep_model_desc &desc, const char *who, bool leaf = false) {
  if (desc.device_inputs) return fail(NEP_ERR_ARG, std::string(who) + " takes host arrays (device_inputs = 0)");
  const int rc = build(m, desc);
  if (rc) return rc;
  if (leaf && (m.step2 || m.fac)) return fail(NEP_ERR_ARG, kLeafRefusal);
  return NEP_OK;
}

extern "C" {

int nep_debug_state(void *model, int32_t slot, double *y, double *kz, float *kty, double *lb, double *ub) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  const DeviceView &v = m.v;
  // (stream-ordered behind the submits / copies on the auxiliary stream, as nep_lp_get_diag)
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (y) HIPCHK(hipMemcpyAsync(y, v.y + slot * v.sdual, v.sdual * sizeof(double), d2h, m.aux));
  if (kz) HIPCHK(hipMemcpyAsync(kz, v.kz + slot * v.sdual, v.sdual * sizeof(double), d2h, m.aux));
  if (kty) HIPCHK(hipMemcpyAsync(kty, v.kty + slot * v.skty, v.skty * sizeof(float), d2h, m.aux));
  if (lb) HIPCHK(hipMemcpyAsync(lb, v.lb + slot * v.sint, v.sint * sizeof(double), d2h, m.aux));
  if (ub) HIPCHK(hipMemcpyAsync(ub, v.ub + slot * v.sint, v.sint * sizeof(double), d2h, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int nep_debug_sparse_rows(void *model, int32_t slot, int32_t *anchor_cnt, float *lambda_nnz) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (lambda_nnz && !m.fac) return fail(NEP_ERR_ARG, "not a facility-relaxation model");
  const DeviceView &v = m.v;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (anchor_cnt) HIPCHK(hipMemcpyAsync(anchor_cnt, v.acnt + (int64_t)slot * m.R, m.R * sizeof(int32_t), d2h, m.aux));
  std::vector<float> lam;
  if (lambda_nnz) {
    lam.resize((size_t)v.sx);
    HIPCHK(hipMemcpyAsync(lam.data(), v.lam + slot * v.sx, lam.size() * sizeof(float), d2h, m.aux));
  }
  HIPCHK(hipStreamSynchronize(m.aux));
  for (int r = 0; lambda_nnz && r < m.R; ++r) {   // (nonzeros of each row of the x <= c duals, host count)
    int c = 0;
    for (int j = 0; j < m.N; ++j) c += lam[(size_t)r * m.NP + j] != 0.f;
    lambda_nnz[r] = (float)c;
  }
  return NEP_OK;
}

int nep_debug_fac_state(void *model, int32_t slot, float *lambda, float *lsum, float *rho_l) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (!m.fac) return fail(NEP_ERR_ARG, "not a facility-relaxation model");
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  // (the block in flight rewrites lambda and its sums on `stream`; this read runs on the auxiliary stream)
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  const DeviceView &v = m.v;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  const size_t wN = m.N * sizeof(float), wNP = m.NP * sizeof(float);
  // rows of NP floats on the device, of N on the host: the padding columns stay behind
  if (lambda) HIPCHK(hipMemcpy2DAsync(lambda, wN, v.lam + (size_t)slot * v.sx, wNP, wN, m.R, d2h, m.aux));
  if (lsum) HIPCHK(hipMemcpy2DAsync(lsum, wN, v.lsum + (size_t)slot * v.slsum, wNP, wN, m.F, d2h, m.aux));
  if (rho_l) HIPCHK(hipMemcpy2DAsync(rho_l, wN, v.rho_l, wNP, wN, m.F, d2h, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int nep_debug_build(const nep_model_desc *desc, double *eta, double *rho, double *gam, double *rownorm, int32_t *dims) {
  if (!desc) return fail(NEP_ERR_ARG, "null argument");
  Model m;
  int rc = scratch_model(m, *desc, "nep_debug_build");
  if (rc) return rc;
  if (eta) *eta = m.eta;
  if (rho) std::memcpy(rho, m.rho.data(), m.rho.size() * sizeof(double));
  if (gam) std::memcpy(gam, m.gam.data(), m.gam.size() * sizeof(double));
  if (rownorm) std::memcpy(rownorm, m.rownorm.data(), m.rownorm.size() * sizeof(double));
  if (dims) {
    dims[0] = m.R; dims[1] = m.F; dims[2] = m.il.n_int; dims[3] = m.dl.n_dual;
  }
  return NEP_OK;
}

int nep_debug_block_split(int32_t n_nodes, int32_t n_functions, int32_t relaxation, int32_t na, int32_t *out3) {
  if (!out3 || n_nodes < 1 || n_functions < 1 || na < 1) return fail(NEP_ERR_ARG, "bad argument");
  DeviceView v{};
  v.N = n_nodes;
  v.F = n_functions;
  v.fac = relaxation == NEP_RELAX_FACILITY ? 1 : 0;
  v.NP = padded_width(n_nodes);
  if (v.NP > max_padded_width(v.fac != 0)) return fail(NEP_ERR_ARG, "n_nodes beyond the widest supported row");
  v.CPL = chunks_per_lane(v.NP);
  out3[0] = block_split(v, na);
  out3[1] = block_tile_waves(v, na, false);
  out3[2] = block_tile_waves(v, na, true);
  return NEP_OK;
}

int nep_debug_leaf_repair(const nep_model_desc *desc, const double *z_leaf, const int32_t *asg, double *upper,
                          int32_t *found, int64_t capacity, int64_t *n_entries, int32_t *row, int32_t *dst, double *val,
                          double *cpu) {
  return nep_debug_leaf_repair_from(desc, z_leaf, asg, nullptr, upper, found, capacity, n_entries, row, dst, val, cpu);
}

int nep_debug_leaf_repair_from(const nep_model_desc *desc, const double *z_leaf, const int32_t *asg, const double *load,
                               double *upper, int32_t *found, int64_t capacity, int64_t *n_entries, int32_t *row,
                               int32_t *dst, double *val, double *cpu) {
  if (!desc || !z_leaf || !asg || !upper || !found || !n_entries) return fail(NEP_ERR_ARG, "null argument");
  Model m;
  int rc = scratch_model(m, *desc, "nep_debug_leaf_repair", true);
  if (rc) return rc;
  std::vector<uint8_t> c_open((size_t)m.F * m.N);
  double nsum = 0.0;
  if (!leaf_binary(m, z_leaf, c_open.data(), &nsum)) return fail(NEP_ERR_ARG, "a leaf fixes every c and n at 0 or 1");
  LeafPoint pt;
  *found = 0;
  *upper = INF;
  *n_entries = 0;
  if (leaf_rejects(m, z_leaf, c_open.data())) return NEP_OK;
  leaf_repair(leaf_instance(m), c_open.data(), nsum, asg, pt, load);
  if (cpu && !pt.cpu.empty()) std::memcpy(cpu, pt.cpu.data(), m.N * sizeof(double));
  if (!pt.found) return NEP_OK;
  *found = 1;
  *upper = pt.obj;
  *n_entries = (int64_t)pt.row.size();
  if (capacity < *n_entries || !row || !dst || !val) return NEP_OK;
  leaf_point_out(pt, row, dst, val);
  return NEP_OK;
}

int nep_debug_leaf_move_list(const nep_model_desc *desc, const double *z_leaf, const double *table, int32_t max_moves,
                             int32_t *n_moves, int32_t *kind, int32_t *fn, int32_t *node, double *delta) {
  if (!desc || !z_leaf || !table || !n_moves) return fail(NEP_ERR_ARG, "null argument");
  if (max_moves < 0) return fail(NEP_ERR_ARG, "max_moves must be >= 0");
  if (max_moves > 0 && (!kind || !fn || !node || !delta)) return fail(NEP_ERR_ARG, "null argument");
  Model m;
  int rc = scratch_model(m, *desc, "nep_debug_leaf_move_list", true);
  if (rc) return rc;
  std::vector<uint8_t> c_open((size_t)m.F * m.N);
  double nsum = 0.0;
  if (!leaf_binary(m, z_leaf, c_open.data(), &nsum)) return fail(NEP_ERR_ARG, "a leaf fixes every c and n at 0 or 1");
  std::vector<LeafMove> mv;
  if (!leaf_rejects(m, z_leaf, c_open.data()))
    leaf_move_list(leaf_instance(m), leaf_limits(m), c_open.data(), table, max_moves, mv);
  leaf_moves_out(mv, max_moves, n_moves, kind, fn, node, delta);
  return NEP_OK;
}

int nep_debug_leaf_swap_list(int32_t F, int32_t N, const double *best, const int32_t *best_from, int32_t per_fn,
                             int32_t max_moves, int32_t *n_moves, int32_t *fn, int32_t *from, int32_t *to,
                             double *delta) {
  if (!best || !best_from || !n_moves) return fail(NEP_ERR_ARG, "null argument");
  if (F < 1 || N < 1) return fail(NEP_ERR_ARG, "bad F or N");
  if (per_fn < 1 || per_fn > kLeafSwapPerFn)
    return fail(NEP_ERR_ARG, "per_fn must be 1 .. " + std::to_string(kLeafSwapPerFn));
  if (max_moves < 0) return fail(NEP_ERR_ARG, "max_moves must be >= 0");
  if (max_moves > 0 && (!fn || !from || !to || !delta)) return fail(NEP_ERR_ARG, "null argument");
  std::vector<LeafSwap> sw;
  if (max_moves > 0) leaf_swap_select(F, N, best, best_from, per_fn, sw);
  leaf_swap_merge(sw, max_moves);
  leaf_swaps_out(sw, max_moves, n_moves, fn, from, to, delta);
  return NEP_OK;
}

int nep_debug_leaf_apply_move(int32_t F, int32_t N, int32_t has_n, const double *z_in, int32_t kind, int32_t fn,
                              int32_t node, int32_t src, double *z_out) {
  if (!z_in || !z_out) return fail(NEP_ERR_ARG, "null argument");
  if (F < 1 || N < 1) return fail(NEP_ERR_ARG, "bad F or N");
  if (!leaf_apply_move(F, N, has_n ? 1 : 0, z_in, kind, fn, node, src, z_out))
    return fail(NEP_ERR_ARG, "a move out of range (kind 0 .. 3, fn, node, a swap's src)");
  return NEP_OK;
}

int nep_debug_leaf_expand(void *model, const double *z_base, int32_t n, const int32_t *kind, const int32_t *fn,
                          const int32_t *node, const int32_t *src, uint8_t *open_out, double *nsum_out) {
  if (!model || !z_base || !kind || !fn || !node || !src || !open_out || !nsum_out)
    return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (m.step2 || m.fac) return fail(NEP_ERR_ARG, kLeafRefusal);
  if (n < 1) return fail(NEP_ERR_ARG, "n must be at least 1");
  const size_t N = m.N, F = m.F;
  std::vector<uint8_t> c_open(F * N);
  double nsum = 0.0;
  if (!leaf_binary(m, z_base, c_open.data(), &nsum)) return fail(NEP_ERR_ARG, "a leaf fixes every c and n at 0 or 1");
  int rc = ensure_leaf(m);
  if (!rc) rc = ensure_leaf_search(m);
  if (rc) return rc;
  Model::LeafWork &w = *m.leaf;
  if (w.cap < 2) return fail(NEP_ERR_ARG, "nep_debug_leaf_expand: the workspace holds one placement of this model");
  LeafSearchBase base;
  base.set(m.F, m.N, c_open.data(), m.has_n ? z_base + m.il.on : nullptr);
  for (int q = 0; q < n; ++q)
    if (!base.in_range(kind[q], fn[q], node[q], src[q]))
      return fail(NEP_ERR_ARG, "move " + std::to_string(q) + " is out of range");
  // the base into slot 0; the neighbours beside it, a chunk of free slots at a time.  cost_n = 1: LeafCtrl::base is
  // the open-node count the record carried
  std::memcpy(w.h_open, c_open.data(), F * N);
  HIPCHK(hipMemcpyAsync(const_cast<uint8_t *>(w.v.open), w.h_open, F * N, hipMemcpyHostToDevice, m.aux));
  const size_t free_slots = (size_t)w.cap - 1;
  for (size_t q0 = 0; q0 < (size_t)n; q0 += free_slots) {
    const int B = (int)std::min(free_slots, (size_t)n - q0);
    for (int q = 0; q < B; ++q) w.h_mv[q] = base.record(kind[q0 + q], fn[q0 + q], node[q0 + q], src[q0 + q]);
    const LeafView nv = leaf_view_at(w.v, 1, B);
    const LeafSearchView xs{0, 1.0, INF, w.d_mv, w.v.open, w.v.ybest};
    HIPCHK(hipMemcpyAsync(w.d_mv, w.h_mv, B * sizeof(LeafSearchMove), hipMemcpyHostToDevice, m.aux));
    HIPCHK(launch_leaf_search_expand(nv, xs, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_open + F * N, nv.open, B * F * N, hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipMemcpyAsync(w.h_ctrl + 1, nv.ctrl, B * sizeof(LeafCtrl), hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipStreamSynchronize(m.aux));
    std::memcpy(open_out + q0 * F * N, w.h_open + F * N, B * F * N);
    for (int q = 0; q < B; ++q) nsum_out[q0 + q] = w.h_ctrl[1 + q].base;
  }
  return NEP_OK;
}

int nep_debug_presolve(const nep_model_desc *desc, int32_t n, const double *lbi, const double *ubi, int32_t *ok_full,
                       int32_t *ok_node, double *box_full, double *box_node) {
  if (!desc || n < 0 || !ok_full || !ok_node) return fail(NEP_ERR_ARG, "null argument");
  Model m;
  int rc = scratch_model(m, *desc, "nep_debug_presolve");
  if (rc) return rc;
  presolve_setup(m);
  const size_t ni = (size_t)m.il.n_int;
  std::vector<double> lb, ub;
  std::vector<uint8_t> mask;
  std::vector<NodeBox> box;
  presolve_batch(m, n, lbi, ubi, box);
  for (int b = 0; b < n; ++b)
    if (box[b].bad)
      return fail(NEP_ERR_ARG, "step-2 node box " + std::to_string(b) +
                               ": moved_from / moved_to bounds must be integral (binary variables; NEP_STEP2_FULL=1 "
                               "iterates the full disruption rows)");   // (the submit path: in parallel for large models)
  for (int b = 0; b < n; ++b) {
    const double *l = lbi ? lbi + b * ni : nullptr, *u = ubi ? ubi + b * ni : nullptr;
    ok_full[b] = presolve_full(m, l, u, lb, ub, mask) ? 1 : 0;
    if (box_full) {
      std::memcpy(box_full + 2 * b * ni, lb.data(), ni * sizeof(double));
      std::memcpy(box_full + (2 * b + 1) * ni, ub.data(), ni * sizeof(double));
    }
    const NodeBox &nb = box[b];
    const PresolveScratch &sc = m.psc[nb.t];
    ok_node[b] = nb.ok ? 1 : 0;
    if (box_node) {
      double *bl = box_node + 2 * b * ni, *bu = box_node + (2 * b + 1) * ni;
      std::memcpy(bl, m.base_lb.data(), ni * sizeof(double));
      std::memcpy(bu, m.base_ub.data(), ni * sizeof(double));
      for (size_t t = nb.off; t < nb.off + nb.cnt; ++t) {
        bl[sc.ci[t]] = sc.cl[t];
        bu[sc.ci[t]] = sc.cu[t];
      }
    }
  }
  return NEP_OK;
}

}  // extern "C"
