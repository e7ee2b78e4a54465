// nep_host.cpp — host runtime of the NEPTUNE LP engine: the batched PDHG solve loop on one HIP stream (batch and
// streaming forms), solution export, and the extern "C" ABI of include/neptune_lp.h.  The model build is
// nep_model_build.cpp, the per-node presolve nep_presolve.cpp, the fixed-placement evaluator's host side
// nep_leaf_host.cpp, the nep_debug_* entries nep_debug.cpp; nep_model.h holds what they share.
#include "nep_model.h"

using namespace nep;

static thread_local std::string g_err;
namespace nep {
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
int set_error(int code, const char *msg) { return fail(code, msg ? msg : ""); }   // (nep_bnb.cpp's messages)
}

// NEP_HALPERN=0 (A/B build variant): plain restarted PDHG — every iteration w' = T(w), the anchor is
// read only on certificate iterations (restart distances)
#ifndef NEP_HALPERN
#define NEP_HALPERN 1
#endif
static constexpr bool kHalpern = NEP_HALPERN != 0;

namespace {

nep_lp_opts resolve_opts(const nep_lp_opts *opts) {
  nep_lp_opts o{};
  o.tol = 1e-7;
  o.cutoff = INF;
  o.max_iters = 200000;
  o.check_every = 64;
  o.warm_start = 0;
  o.warm_omega_floor = 2.0;
  o.warm_omega_cap = 4.0;
  if (opts) {
    if (opts->tol > 0) o.tol = opts->tol;
    o.cutoff = opts->cutoff;
    if (opts->max_iters > 0) o.max_iters = opts->max_iters;
    if (opts->check_every > 0) o.check_every = opts->check_every;
    o.warm_start = opts->warm_start;
    if (opts->warm_omega_floor != 0) o.warm_omega_floor = opts->warm_omega_floor < 0 ? 0.0 : opts->warm_omega_floor;
    o.gap_tol = opts->gap_tol;
    if (opts->warm_omega_cap != 0) o.warm_omega_cap = opts->warm_omega_cap < 0 ? 0.0 : opts->warm_omega_cap;
    o.polish_after = opts->polish_after;
    o.bound_res = opts->bound_res > 0 ? opts->bound_res : 0.0;
  }
  if (!(o.gap_tol > 0)) o.gap_tol = o.tol;
  // polishing: by default only warm-started LPs (B&B children) polish; a cold LP (a root) iterates on
  // to its own certificate, whose more converged duals its children then start from
  if (o.polish_after == 0) o.polish_after = o.warm_start ? 256.0 : -1.0;
  return o;
}

// tol / cutoff / gap tol of every LP in flight (device memory, read by the graph-replayed blocks): copied on
// the auxiliary stream when they change
static hipError_t set_prm(Model &m, double tol, double cutoff, double gap_tol) {
  if (m.prm_sent && m.prm_host[0] == tol && m.prm_host[1] == cutoff && m.prm_host[2] == gap_tol) return hipSuccess;
  m.prm_host[0] = tol;
  m.prm_host[1] = cutoff;
  m.prm_host[2] = gap_tol;
  m.prm_sent = true;
  return hipMemcpyAsync(m.d_prm, m.prm_host, sizeof(m.prm_host), hipMemcpyHostToDevice, m.aux);
}

// Start n node LPs: presolve each on the host, upload its bounds and destination mask, initialise
// the slot (cold or warm) and add it to the iterating set.  status[b] = NEP_LP_INFEASIBLE for a
// node presolve proves infeasible (it does not iterate), else NEP_LP_ITERATION_LIMIT.
int submit(Model &m, int n, const int32_t *slots, const double *lbi, const double *ubi, const nep_lp_opts *opts,
           int32_t *status, const int64_t *mi_per = nullptr, const double *br_per = nullptr) {
  if (n <= 0) return NEP_OK;
  const nep_lp_opts o = resolve_opts(opts);
  if (!m.act.empty() && o.check_every != m.run.check_every)
    return fail(NEP_ERR_STATE, "check_every cannot change while LPs are iterating");
  for (int b = 0; b < n; ++b) {
    const int s = slots[b];
    if (s < 0 || s >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[s]) return fail(NEP_ERR_STATE, "slot " + std::to_string(s) + " is still iterating");
  }
  m.run = o;
  DeviceView &v = m.v;
  v.warm_omega_floor = o.warm_omega_floor;
  v.warm_omega_cap = o.warm_omega_cap;
  v.warm_omega_ref = m.omega_ref;
  v.polish_after = (o.polish_after < 0 || m.fac) ? -1 : (int64_t)o.polish_after;   // (fac: no polishing)
  v.max_iters = o.max_iters;
  v.bound_res = o.bound_res;
  // tol / cutoff of every LP in flight: device memory, read by the (graph-replayed) blocks
  HIPCHK(set_prm(m, o.tol, o.cutoff, o.gap_tol));
  std::vector<NodeBox> box;
  const auto tp0 = std::chrono::steady_clock::now();
  presolve_batch(m, n, lbi, ubi, box);
  if (m.prof) {
    m.pr_pre += std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count();
    ++m.pr_calls;
    m.pr_lps += n;
  }
  struct StageTimer {   // (the rest of the call: staging and launches)
    Model &m;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    ~StageTimer() {
      if (m.prof) m.pr_stage += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
    }
  } stage_timer{m};
  for (int b = 0; b < n; ++b)
    if (box[b].bad)
      return fail(NEP_ERR_ARG, "step-2 node box " + std::to_string(b) +
                               ": moved_from / moved_to bounds must be integral (binary variables; NEP_STEP2_FULL=1 "
                               "iterates the full disruption rows)");
  std::vector<int32_t> fresh, off(1, 0), exact;
  std::vector<double> per_mi, per_br;   // (nep_lp_submit_ex: the fresh slots' own budget / bound stop)
  const bool per = mi_per != nullptr || br_per != nullptr;
  int max_chg = 0;
  for (int b = 0; b < n; ++b) {
    const int s = slots[b];
    const NodeBox &nb = box[b];
    status[b] = nb.ok ? NEP_LP_ITERATION_LIMIT : NEP_LP_INFEASIBLE;
    m.rc_stale[s] = nb.ok ? 0 : 1;
    if (!nb.ok) continue;
    m.busy[s] = 1;
    fresh.push_back(s);
    exact.push_back(nb.ex ? 1 : 0);
    off.push_back(off.back() + (int32_t)nb.cnt);
    max_chg = std::max(max_chg, (int)nb.cnt);
    if (per) {
      per_mi.push_back((double)(mi_per && mi_per[b] > 0 ? mi_per[b] : o.max_iters));
      per_br.push_back(br_per ? (br_per[b] > 0 ? br_per[b] : 0.0) : o.bound_res);
    }
  }
  const size_t nchg = (size_t)off.back();
  if (fresh.empty()) {
    HIPCHK(hipStreamSynchronize(m.aux));
    return NEP_OK;
  }
  const int nf = (int)fresh.size();
  // the node boxes on the device: base box copy + the packed changes scattered over it (a few
  // KB per node instead of the 2 x 8 x n_int bytes of bounds and the F x NP mask), staged through pinned
  // host memory so the call need not wait for the copies (nor for the initialisation kernels behind them)
  const size_t need_i = 2 * (size_t)nf + off.size() + nchg, need_d = 2 * nchg + (per ? 2 * (size_t)nf : 0);
  const int sk = m.sub_k;
  m.sub_k ^= 1;
  if (m.sub_pending[sk]) HIPCHK(hipEventSynchronize(m.ev_sub[sk]));   // that staging's copies have read it
  m.sub_pending[sk] = false;
  if (need_i > m.cap_sub_i[sk]) {
    if (m.h_sub_i[sk]) HIPCHK(hipHostFree(m.h_sub_i[sk]));
    m.h_sub_i[sk] = nullptr;
    m.cap_sub_i[sk] = std::max(need_i, 2 * m.cap_sub_i[sk]);
    void *h = nullptr;
    if (hipHostMalloc(&h, m.cap_sub_i[sk] * sizeof(int32_t)) != hipSuccess) return fail(NEP_ERR_NOMEM, "hipHostMalloc (submit)");
    m.h_sub_i[sk] = static_cast<int32_t *>(h);
  }
  if (need_d > m.cap_sub_d[sk]) {
    if (m.h_sub_d[sk]) HIPCHK(hipHostFree(m.h_sub_d[sk]));
    m.h_sub_d[sk] = nullptr;
    m.cap_sub_d[sk] = std::max(need_d, 2 * m.cap_sub_d[sk]);
    void *h = nullptr;
    if (hipHostMalloc(&h, m.cap_sub_d[sk] * sizeof(double)) != hipSuccess) return fail(NEP_ERR_NOMEM, "hipHostMalloc (submit)");
    m.h_sub_d[sk] = static_cast<double *>(h);
  }
  if (!m.ev_sub[sk]) HIPCHK(hipEventCreateWithFlags(&m.ev_sub[sk], hipEventDisableTiming));
  int32_t *hf = m.h_sub_i[sk], *ho = hf + nf, *hc = ho + off.size(), *he = hc + nchg;
  double *hl = m.h_sub_d[sk], *hu = hl + nchg;
  if (per) {
    std::copy(per_mi.begin(), per_mi.end(), hu + nchg);
    std::copy(per_br.begin(), per_br.end(), hu + nchg + nf);
  }
  std::copy(fresh.begin(), fresh.end(), hf);
  std::copy(off.begin(), off.end(), ho);
  std::copy(exact.begin(), exact.end(), he);
  for (int b = 0, q = 0; b < n; ++b) {   // the feasible nodes' changes, in batch order
    const NodeBox &nb = box[b];
    if (!nb.ok) continue;
    const PresolveScratch &sc = m.psc[nb.t];
    std::memcpy(hc + off[q], sc.ci.data() + nb.off, nb.cnt * sizeof(int32_t));
    std::memcpy(hl + off[q], sc.cl.data() + nb.off, nb.cnt * sizeof(double));
    std::memcpy(hu + off[q], sc.cu.data() + nb.off, nb.cnt * sizeof(double));
    ++q;
  }
  HIPCHK(hipMemcpyAsync(m.d_sub_i, hf, need_i * sizeof(int32_t), hipMemcpyHostToDevice, m.aux));
  if (need_d) HIPCHK(hipMemcpyAsync(m.d_sub_d, hl, need_d * sizeof(double), hipMemcpyHostToDevice, m.aux));
  int32_t *dn = m.d_sub_i, *doff = dn + nf, *didx = doff + off.size(), *dex = didx + nchg;
  double *dlb = m.d_sub_d, *dub = dlb + nchg;
  // the staging is free again once these copies are done (the next submit waits for this event only, not
  // for the initialisation kernels below)
  HIPCHK(hipEventRecord(m.ev_sub[sk], m.aux));
  HIPCHK(launch_node_bounds(v, dn, nf, m.d_base_lb, m.d_base_ub, m.d_base_mask, doff, didx, dlb, dub, max_chg,
                            m.aux));
  HIPCHK(launch_init_slot(v, dn, dex, nf, o.warm_start != 0, m.eta, m.omega0, per ? dub + nchg : nullptr, m.aux));
  HIPCHK(launch_x_pass(v, dn, nf, false, true, true, true, 0, m.aux));
  HIPCHK(launch_node_pass(v, dn, nf, false, true, true, true, 0, m.aux));
  HIPCHK(launch_scalar_pass(v, dn, nf, false, true, true, true, 0, o.check_every, m.aux));
  // the new slots join the block after the one in flight: `stream` waits for their initialisation
  HIPCHK(hipEventRecord(m.ev_aux, m.aux));
  HIPCHK(hipStreamWaitEvent(m.stream, m.ev_aux, 0));
  m.act.insert(m.act.end(), fresh.begin(), fresh.end());   // (d_slots follows at the next launch_block)
  m.sub_pending[sk] = true;
  return NEP_OK;
}

// Iterations [it0, it1) of a block on `n` of its `na` iterating slots, one launch chain on `s`.  (The x pass takes
// its non-temporal policy from na: speed only, and the one the launch over the whole block would get.)
hipError_t launch_iters(Model &m, const int32_t *slots, int n, int na, int it0, int it1, hipStream_t s) {
  const int ce = m.run.check_every;
  hipError_t e = hipSuccess;
  for (int it = it0; it < it1 && e == hipSuccess; ++it) {
    const bool check = it == 0, first = it == 1;
    const bool plain = !kHalpern || ce < 4 || it == 0 || it == ce - 1;
    e = launch_x_pass(m.v, slots, n, check, false, first, plain, it, s, na);
    if (e == hipSuccess) e = launch_node_pass(m.v, slots, n, check, false, first, plain, it, s);
    if (e == hipSuccess && (m.step2 || check)) e = launch_scalar_pass(m.v, slots, n, check, false, first, plain, it, ce, s);
  }
  return e;
}

// Iterations [it0, it1) of a block: one chain on `stream` (nA == 0), or its two slot groups side by side — group A,
// d_slots[0 .. nA), on `stream` and group B, d_slots[nA .. na), on `grp` — so that one group's node and scalar passes
// and the part-empty tail of its x pass run under the other group's x pass.  No kernel of an iteration reads another
// slot's state, so the groups need no order between them, and with block_split's rule every launch of a group runs
// the kernel variant the launch over all na slots runs: each LP's arithmetic, and so its bits, stay what they were.
// Ordering.  B forks from `stream` (ev_fork) behind the d_slots upload and behind every wait for a submit's
// initialisation (ev_aux) that `stream` holds, so B iterates initialised slots from the list A reads.  B joins
// (ev_join) before this returns, i.e. before the block's Ctrl copy and before anything later on `stream`: once
// advance has waited for `stream`, the slots of both groups are complete, their Ctrl is the copied one, and the reads
// of finished slots on `aux` that follow see them whole.  The join is enqueued even after a failed launch, so that a
// stream capture never ends with `grp` still forked.
hipError_t launch_span(Model &m, int na, int nA, int it0, int it1) {
  if (it0 >= it1) return hipSuccess;
  if (!nA) return launch_iters(m, m.d_slots, na, na, it0, it1, m.stream);
  hipError_t e = hipEventRecord(m.ev_fork, m.stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(m.grp, m.ev_fork, 0);
  if (e != hipSuccess) return e;
  const hipError_t ea = launch_iters(m, m.d_slots, nA, na, it0, it1, m.stream);
  const hipError_t eb = launch_iters(m, m.d_slots + nA, na - nA, na, it0, it1, m.grp);
  e = hipEventRecord(m.ev_join, m.grp);
  if (e == hipSuccess) e = hipStreamWaitEvent(m.stream, m.ev_join, 0);
  return ea != hipSuccess ? ea : eb != hipSuccess ? eb : e;
}

void drop_block_graphs(Model &m) {
  for (hipGraphExec_t &g : m.block_graph)
    if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
  m.block_graph.assign(m.max_batch + 1, nullptr);
}

// The launches of one block (iterations 0 .. ce-1 on `na` iterating slots, m.d_slots) captured
// once as a HIP graph and cached per na; m.d_slots is read by the kernels at run time, so the
// graph replays for any set of na slots.  With slot groups (nA > 0; a function of na while m.groups holds) the
// graph has two parallel branches between the fork and the join.
hipError_t block_graph(Model &m, int na, int nA, hipGraphExec_t *out) {
  const int ce = m.run.check_every;
  if (m.graph_ce != ce) {
    drop_block_graphs(m);
    m.graph_ce = ce;
  }
  if (!m.block_graph[na]) {
    hipError_t e = hipStreamBeginCapture(m.stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return e;
    const hipError_t le = launch_span(m, na, nA, 0, ce);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(m.stream, &graph);
    if (le != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); return le; }
    if (e != hipSuccess) return e;
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return e;
    m.block_graph[na] = exec;
  }
  *out = m.block_graph[na];
  return hipSuccess;
}

// One block of `ce` iterations on the iterating slots (m.act), enqueued without waiting: it == 0 is
// the certificate iteration (a plain PDHG step whose input dual is the previous block's plain
// output, so it satisfies the row sign constraints and its Lagrangian is a valid bound); restarts
// decided there take effect at it == 1; it == ce - 1 is plain again; the others are reflected
// Halpern steps.  Every 4th block runs eagerly with one steady-state x-pass launch bracketed by HIP
// events on the model's stream (nep_get_stats); the others replay the block's launches as one HIP
// graph (a block is 2-3 launches per iteration: at small sizes the iteration is launch-latency
// bound).  Where block_split allows, the slots iterate as two groups on two streams (launch_span), in the graph as
// two parallel branches.  The block ends with an async copy of every slot's Ctrl into pinned host memory.
int launch_block(Model &m) {
  DeviceView &v = m.v;
  const int ce = m.run.check_every;
  const int na = (int)m.act.size();
  const int sample_it = (ce >= 4 && m.blocks % 4 == 0) ? 2 : -1;
  m.blocks += 1;
  // the iterating slots for the kernels (read at run time, so the cached graphs replay for any set):
  // staged through pinned memory, rewritten only here — every earlier upload has completed, since a
  // block is launched only once the previous one was waited for (advance) — so no queued copy reads a
  // host buffer that the caller's next submit may reallocate (round-3 ADVICE)
  std::copy(m.act.begin(), m.act.end(), m.h_act);
  HIPCHK(hipMemcpyAsync(m.d_slots, m.h_act, na * sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
  // slot groups (launch_span): the rule is the launchers' own (nep_kernels.hip block_split)
  int nA = m.groups > 1 ? block_split(v, na) : 0;
  bool eager = sample_it >= 0 || !m.graphs_ok;
  if (!eager) {
    hipGraphExec_t g = nullptr;
    hipError_t e = block_graph(m, na, nA, &g);
    if (e != hipSuccess && nA) {
      // the forked capture or its instantiation failed: this model's blocks stay on one stream from here on
      (void)hipGetLastError();
      m.groups = 1;
      nA = 0;
      drop_block_graphs(m);
      e = block_graph(m, na, 0, &g);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      m.graphs_ok = false;   // e.g. a caller's stream that cannot be captured
      eager = true;
    } else {
      HIPCHK(hipGraphLaunch(g, m.stream));
    }
  }
  if (eager) {
    // the sampled iteration is one x-pass launch over all na slots, alone on the device between its events
    // (nep_get_stats keeps its meaning): the groups join in front of it and fork again behind its node pass
    const int s0 = sample_it >= 0 ? sample_it : ce, s1 = sample_it >= 0 ? sample_it + 1 : ce;
    HIPCHK(launch_span(m, na, nA, 0, s0));
    if (sample_it >= 0) {
      const bool plain = !kHalpern;   // (ce >= 4 and 0 < sample_it < ce - 1: a steady-state iteration)
      HIPCHK(hipEventRecord(m.ev0, m.stream));
      HIPCHK(launch_x_pass(v, m.d_slots, na, false, false, false, plain, sample_it, m.stream));
      HIPCHK(hipEventRecord(m.ev1, m.stream));
      HIPCHK(launch_node_pass(v, m.d_slots, na, false, false, false, plain, sample_it, m.stream));
      if (m.step2) HIPCHK(launch_scalar_pass(v, m.d_slots, na, false, false, false, plain, sample_it, ce, m.stream));
    }
    HIPCHK(launch_span(m, na, nA, s1, ce));
  }
  m.stats.x_pass_launches += ce;   // (iterations, whichever way they were launched)
  HIPCHK(hipMemcpyAsync(m.h_ctrl, v.ctrl, sizeof(Ctrl) * m.max_batch, hipMemcpyDeviceToHost, m.stream));
  m.stats.lp_iterations += (int64_t)na * ce;
  m.launched = m.act;
  m.inflight = true;
  m.inflight_sampled = sample_it >= 0;
  return NEP_OK;
}

// Run blocks of `check_every` PDHG iterations on every iterating slot until at least `min_done`
// of them have finished (min_done <= 0: exactly one block).  Finished slots are reported in
// done[0 .. *n_done) with their results.  Blocks are pipelined: once a block's results are read,
// the next block of the still-iterating slots is enqueued BEFORE returning, so the device keeps
// iterating while the caller branches, presolves and submits the next nodes (those join at the
// block after; their initialisation is stream-ordered behind the block in flight).
int advance(Model &m, int min_done, int32_t *n_done, int32_t *done, double *obj, double *pobj, int32_t *status,
            int64_t *iters) {
  *n_done = 0;
  while (true) {
    if (!m.inflight) {
      if (m.act.empty()) break;
      int rc = launch_block(m);
      if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(m.stream));
    m.inflight = false;
    if (m.inflight_sampled) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, m.ev0, m.ev1));
      m.stats.x_pass_ms += ms;
      m.stats.x_pass_sampled += 1;
      m.stats.x_pass_lp_iters += (int64_t)m.launched.size();
    }
    // results of the slots that block iterated (slots submitted meanwhile are not in it)
    std::vector<uint8_t> fin(m.max_batch, 0);
    for (int s : m.launched) {
      const Ctrl &c = m.h_ctrl[s];
      if (c.active) continue;
      fin[s] = 1;
      const int k = (*n_done)++;
      done[k] = s;
      status[k] = c.status;
      iters[k] = c.k;
      pobj[k] = c.pobj;
      obj[k] = c.status == NEP_LP_INFEASIBLE ? INF : (c.status == NEP_LP_OPTIMAL ? c.lagr : c.best_lagr);
      m.busy[s] = 0;
    }
    if (*n_done > 0) {
      std::vector<int32_t> still;
      for (int s : m.act)
        if (!fin[s]) still.push_back(s);
      m.act.swap(still);
    }
    // the next block runs while the caller handles the finished slots — unless more than
    // pipe_max_done slots just finished and the call returns: then the caller's refill joins the
    // very next block instead of the one after (NEP_PIPELINE_MAX_DONE; default: always pipeline)
    const bool returning = min_done <= 0 || *n_done >= min_done;
    if (!m.act.empty() && (!returning || *n_done <= m.pipe_max_done)) {
      int rc = launch_block(m);
      if (rc) return rc;
    }
    if (returning) break;
  }
  return NEP_OK;
}

int solve_batch(Model &m, int B, const int32_t *slots, const double *lbi, const double *ubi, const nep_lp_opts *opts,
                double *obj, double *pobj, int32_t *status, int64_t *iters) {
  auto t0 = std::chrono::steady_clock::now();
  if (B <= 0) return NEP_OK;
  if (B > m.max_batch) return fail(NEP_ERR_ARG, "B > max_batch");
  if (!m.act.empty()) return fail(NEP_ERR_STATE, "streamed LPs are still iterating (nep_lp_advance them first)");
  std::vector<int> where(m.max_batch, -1);
  for (int b = 0; b < B; ++b) {
    if (slots[b] < 0 || slots[b] >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (where[slots[b]] >= 0) return fail(NEP_ERR_ARG, "duplicate slot");
    where[slots[b]] = b;
  }
  int rc = submit(m, B, slots, lbi, ubi, opts, status);
  if (rc) return rc;
  for (int b = 0; b < B; ++b) {
    obj[b] = status[b] == NEP_LP_INFEASIBLE ? INF : -INF;
    pobj[b] = NAN;
    iters[b] = 0;
  }
  std::vector<int32_t> dn(m.max_batch), ds(m.max_batch);
  std::vector<double> dobj(m.max_batch), dpobj(m.max_batch);
  std::vector<int64_t> dit(m.max_batch);
  while (!m.act.empty()) {
    int32_t nd = 0;
    rc = advance(m, INT_MAX, &nd, dn.data(), dobj.data(), dpobj.data(), ds.data(), dit.data());
    if (rc) return rc;
    for (int k = 0; k < nd; ++k) {
      const int b = where[dn[k]];
      status[b] = ds[k];
      obj[b] = dobj[k];
      pobj[b] = dpobj[k];
      iters[b] = dit[k];
    }
  }
  m.stats.solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return NEP_OK;
}

// ---------------------------------------------------------------------------------------------
// auxiliary device work on finished slots (nep_aux.hip)
// ---------------------------------------------------------------------------------------------
// The solution of a slot: the certificate's repaired point when its LP was certified (that point
// is the one whose objective and feasibility the certificate proved), else the PDHG iterate.
int solution_z(Model &m, int slot, const double **z) {
  int32_t st = 0;
  HIPCHK(hipMemcpyAsync(&st, &m.v.ctrl[slot].status, sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  *z = (st == NEP_LP_OPTIMAL ? m.v.zr : m.v.zi) + (size_t)slot * m.v.sint;
  return NEP_OK;
}

int ensure_entries(Model &m, int64_t need) {
  if (need <= m.ecap) return NEP_OK;
  int64_t cap = std::max<int64_t>(need, 4096);
  int rc;
  if ((rc = dalloc(m, &m.d_erow, (size_t)cap))) return rc;
  if ((rc = dalloc(m, &m.d_ecol, (size_t)cap))) return rc;
  if ((rc = dalloc(m, &m.d_eval, (size_t)cap))) return rc;
  m.ecap = cap;
  return NEP_OK;
}

// compaction of a [rows][ld] device matrix: entries > thr, in row-major order
template <typename T>
int compact(Model &m, const T *vals, int rows, int cols, int64_t ld, double thr, int round3, int64_t capacity,
            int64_t *n_out, int32_t *orow, int32_t *ocol, double *oval) {
  int rc;
  if (!m.d_cnt) {
    const size_t n = (size_t)std::max(m.R, m.F) + 1;
    if ((rc = dalloc(m, &m.d_cnt, n))) return rc;
    if ((rc = dalloc(m, &m.d_off, n))) return rc;
  }
  hipError_t e;
  if constexpr (sizeof(T) == 4)
    e = launch_compact_f32(vals, rows, cols, ld, thr, round3, m.d_cnt, m.d_off, nullptr, nullptr, nullptr, true, m.aux);
  else
    e = launch_compact_f64(vals, rows, cols, ld, thr, round3, m.d_cnt, m.d_off, nullptr, nullptr, nullptr, true, m.aux);
  HIPCHK(e);
  int32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, m.d_off + rows, sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  *n_out = total;
  if (capacity < total || total == 0) return NEP_OK;   // size query (or nothing to write)
  if ((rc = ensure_entries(m, total))) return rc;
  if constexpr (sizeof(T) == 4)
    e = launch_compact_f32(vals, rows, cols, ld, thr, round3, m.d_cnt, m.d_off, m.d_erow, m.d_ecol, m.d_eval, false,
                           m.aux);
  else
    e = launch_compact_f64(vals, rows, cols, ld, thr, round3, m.d_cnt, m.d_off, m.d_erow, m.d_ecol, m.d_eval, false,
                           m.aux);
  HIPCHK(e);
  if (orow) HIPCHK(hipMemcpyAsync(orow, m.d_erow, total * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  if (ocol) HIPCHK(hipMemcpyAsync(ocol, m.d_ecol, total * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  if (oval) HIPCHK(hipMemcpyAsync(oval, m.d_eval, total * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int flows(Model &m, int n, const int32_t *slots, float *out, float *wout = nullptr) {
  if (n <= 0) return NEP_OK;
  if (n > m.max_batch) return fail(NEP_ERR_ARG, "n > max_batch");
  for (int b = 0; b < n; ++b) {
    if (slots[b] < 0 || slots[b] >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[slots[b]]) return fail(NEP_ERR_STATE, "slot is still iterating");
  }
  int rc;
  const size_t plane = (size_t)m.max_batch * m.F * m.N;
  if (!m.d_flows && (rc = dalloc(m, &m.d_flows, 2 * plane))) return rc;
  // pinned staging both ways: pageable copies cost ~0.3 ms per call while a block iterates (round-4 B&B
  // profile, tools/probes/bnb_profile.py: 2.5 of 10 s at 64x32)
  if (!m.h_flows) {
    void *h = nullptr;
    if (hipHostMalloc(&h, sizeof(float) * 2 * plane + sizeof(int32_t) * m.max_batch) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (flows)");
    m.h_flows = static_cast<float *>(h);
  }
  int32_t *hs = reinterpret_cast<int32_t *>(m.h_flows + 2 * plane);
  std::memcpy(hs, slots, n * sizeof(int32_t));
  const size_t cnt = (size_t)n * m.F * m.N;
  HIPCHK(hipMemcpyAsync(m.d_new, hs, n * sizeof(int32_t), hipMemcpyHostToDevice, m.aux));
  HIPCHK(launch_node_flows(m.v, m.d_new, n, m.d_flows, wout ? m.d_flows + plane : nullptr, m.aux));
  HIPCHK(hipMemcpyAsync(m.h_flows, m.d_flows, cnt * sizeof(float), hipMemcpyDeviceToHost, m.aux));
  if (wout) HIPCHK(hipMemcpyAsync(m.h_flows + plane, m.d_flows + plane, cnt * sizeof(float), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  std::memcpy(out, m.h_flows, cnt * sizeof(float));
  if (wout) std::memcpy(wout, m.h_flows + plane, cnt * sizeof(float));
  return NEP_OK;
}

int score_check(Model &m, int slot, double *out) {
  int rc;
  const size_t nfj = (size_t)m.F * m.NP, nf = (size_t)m.F * 4, nj = (size_t)m.N * 6;
  if (!m.d_score) {
    if ((rc = dalloc(m, &m.d_score, nfj + nf + nj + 16))) return rc;
    const double *p = nullptr;
    if ((rc = upload(m, &p, m.node_cost))) return rc;
    m.d_node_cost = const_cast<double *>(p);
  }
  double *cpu_fj = m.d_score, *fpart = cpu_fj + nfj, *jpart = fpart + nf, *dout = jpart + nj;
  const double *z = nullptr;
  if ((rc = solution_z(m, slot, &z))) return rc;
  HIPCHK(launch_score_check(m.v, slot, z, cpu_fj, fpart, jpart, m.d_node_cost, m.node_budget, dout, m.aux));
  double raw[16] = {0};
  HIPCHK(hipMemcpyAsync(raw, dout, 10 * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  // NEP_SC_* layout (include/neptune_lp.h)
  out[0] = raw[0];                                   // network delay  sum W D x
  out[1] = raw[6];                                   // nodes used     #{n != 0}
  out[2] = raw[7];                                   // node cost      sum n * cost
  out[3] = raw[1];                                   // c_x violations
  out[4] = raw[3];                                   // memory violations
  out[5] = raw[2];                                   // handle_all violations (sources)
  out[6] = raw[4];                                   // CPU violations
  out[7] = raw[5];                                   // n_c violations
  out[8] = raw[7] > m.node_budget + 1e-6 ? 1.0 : 0.0;   // budget violated
  out[9] = raw[8];                                   // max |sum_j x - 1| over routing rows
  out[10] = raw[9];                                  // max CPU excess over cores
  return NEP_OK;
}

}  // namespace

namespace nep {
// (nep_bnb.cpp: nep_bnb_create gives the tree nep_lp_rc_fixings only for a facility-relaxation model)
bool model_is_facility(void *model) { return model && static_cast<Model *>(model)->fac != 0; }
// (nep_bnb.cpp: nep_bnb_create gives the tree the fixed-placement evaluator only for a step-1 reference model)
bool model_has_leaf_eval(void *model) {
  return model && !static_cast<Model *>(model)->fac && !static_cast<Model *>(model)->step2;
}
}

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int nep_api_version(void) { return NEP_API_VERSION; }
const char *nep_last_error(void) { return g_err.c_str(); }

// API 9: a descriptor whose arrays are device memory (nep_model_desc.device_inputs), staged to the host: the
// build's aggregation, coefficients, presolve base box and scaling read the O(F N + N^2) instance there
struct HostDesc {
  nep_model_desc d{};
  std::vector<double> delay, workload, cpr, fmem, nmem, ncores, ncost, maxd, old;
};
static int stage_device_desc(const nep_model_desc &in, HostDesc &h) {
  h.d = in;
  h.d.device_inputs = 0;
  const size_t N = (size_t)std::max(0, in.n_nodes), F = (size_t)std::max(0, in.n_functions);
  auto get = [&](const double *src, size_t n, std::vector<double> &dst, const double **out) -> hipError_t {
    if (!src) { *out = nullptr; return hipSuccess; }
    dst.resize(n);
    *out = dst.data();
    return n ? hipMemcpy(dst.data(), src, n * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess;
  };
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = get(in.delay, N * N, h.delay, &h.d.delay);
  if (e == hipSuccess) e = get(in.workload, F * N, h.workload, &h.d.workload);
  if (e == hipSuccess) e = get(in.core_per_req, F * N, h.cpr, &h.d.core_per_req);
  if (e == hipSuccess) e = get(in.function_memory, F, h.fmem, &h.d.function_memory);
  if (e == hipSuccess) e = get(in.node_memory, N, h.nmem, &h.d.node_memory);
  if (e == hipSuccess) e = get(in.node_cores, N, h.ncores, &h.d.node_cores);
  if (e == hipSuccess) e = get(in.node_cost, N, h.ncost, &h.d.node_cost);
  if (e == hipSuccess) e = get(in.max_delay, F, h.maxd, &h.d.max_delay);
  if (e == hipSuccess) e = get(in.old_allocations, F * N, h.old, &h.d.old_allocations);
  if (e != hipSuccess) return fail(NEP_ERR_ARG, std::string("device_inputs: reading the instance arrays: ") +
                                                    hipGetErrorString(e));
  return NEP_OK;
}

int nep_model_create(const nep_model_desc *desc_in, int32_t max_batch, void *hip_stream, void **out_model) {
  if (!desc_in || !out_model) return fail(NEP_ERR_ARG, "null argument");
  HostDesc staged;
  const nep_model_desc *desc = desc_in;
  if (desc_in->device_inputs) {
    const int rs = stage_device_desc(*desc_in, staged);
    if (rs) return rs;
    desc = &staged.d;
  }
  if (max_batch <= 0) return fail(NEP_ERR_ARG, "max_batch must be positive");
  std::unique_ptr<Model> m(new Model());
  // (NEP_HOST_POWER=1: the host power iteration instead of the device's, for A/B)
  const char *hp = std::getenv("NEP_HOST_POWER");
  const bool host_power = hp && std::atoi(hp) != 0;
  int rc = build(*m, *desc, host_power);
  if (rc == NEP_OK) presolve_setup(*m);
  if (rc) return rc;
  rc = setup_device(*m, max_batch, hip_stream);
  if (rc) return rc;
  rc = setup_dense(*m, *desc);
  if (rc) return rc;
  if (!host_power && (rc = power_device(*m))) return rc;
  if (const char *e = std::getenv("NEP_ETA_SCALE")) m->eta *= std::atof(e);   // (probe: tools/probes/root_chaos_probe.py)
  if (const char *e = std::getenv("NEP_HOST_PROFILE")) m->prof = e[0] == '1';
  *out_model = m.release();
  return NEP_OK;
}

void nep_model_destroy(void *model) {
  Model *m = static_cast<Model *>(model);
  if (m && m->prof)
    std::fprintf(stderr, "[nep_lp profile] %dx%d%s | submit calls %lld lps %lld presolve %.3fs staging+launch %.3fs | "
                 "advance calls %lld %.3fs\n", m->N, m->F, m->fac ? " fac" : "", (long long)m->pr_calls,
                 (long long)m->pr_lps, m->pr_pre, m->pr_stage, (long long)m->pr_adv_calls, m->pr_adv);
  delete m;
}

int nep_model_get_info(void *model, nep_model_info *info) {
  if (!model || !info) return fail(NEP_ERR_ARG, "null argument");
  const Model &m = *static_cast<Model *>(model);
  info->n_int = m.il.n_int;
  info->n_rows = m.R;
  info->n_tiles = m.F;
  info->max_batch = m.max_batch;
  info->x_entries = (int64_t)m.R * m.N;
  // B_iter = 4 (2P + 2FN + 2N + 2m), P = x entries iterated, m = dual rows
  // (facility relaxation: the x <= c rows are dualised rows too, one per routing entry: m += R N)
  info->bytes_per_iter = 4 * (2 * (int64_t)m.R * m.N + 2 * (int64_t)m.F * m.N + 2 * (int64_t)m.N +
                              2 * ((int64_t)m.dl.n_dual + (m.fac ? (int64_t)m.R * m.N : 0)));
  info->step_size = m.eta;
  info->primal_weight0 = m.omega0;
  return NEP_OK;
}

int nep_lp_solve_batch(void *model, int32_t B, const int32_t *slots, const double *lb_int, const double *ub_int,
                       const nep_lp_opts *opts, double *obj, double *primal_obj, int32_t *status, int64_t *iters) {
  if (!model || !slots || !obj || !primal_obj || !status || !iters) return fail(NEP_ERR_ARG, "null argument");
  return solve_batch(*static_cast<Model *>(model), B, slots, lb_int, ub_int, opts, obj, primal_obj, status, iters);
}

int nep_lp_submit(void *model, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                  const nep_lp_opts *opts, int32_t *status) {
  if (!model || (n > 0 && (!slots || !status))) return fail(NEP_ERR_ARG, "null argument");
  return submit(*static_cast<Model *>(model), n, slots, lb_int, ub_int, opts, status);
}

int nep_lp_submit_ex(void *model, int32_t n, const int32_t *slots, const double *lb_int, const double *ub_int,
                     const nep_lp_opts *opts, const int64_t *max_iters, const double *bound_res, int32_t *status) {
  if (!model || (n > 0 && (!slots || !status))) return fail(NEP_ERR_ARG, "null argument");
  return submit(*static_cast<Model *>(model), n, slots, lb_int, ub_int, opts, status, max_iters, bound_res);
}

int nep_lp_advance(void *model, int32_t min_done, int32_t *n_done, int32_t *done_slots, double *obj,
                   double *primal_obj, int32_t *status, int64_t *iters) {
  if (!model || !n_done || !done_slots || !obj || !primal_obj || !status || !iters)
    return fail(NEP_ERR_ARG, "null argument");
  auto t0 = std::chrono::steady_clock::now();
  Model &m = *static_cast<Model *>(model);
  const int rc = advance(m, min_done, n_done, done_slots, obj, primal_obj, status, iters);
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  m.stats.solve_ms += 1e3 * dt;
  if (m.prof) { m.pr_adv += dt; ++m.pr_adv_calls; }
  return rc;
}

int nep_lp_active(void *model) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  return (int)static_cast<Model *>(model)->act.size();
}

int nep_lp_get_solutions(void *model, int32_t n, const int32_t *slots, double *z_out) {
  if (!model || (n > 0 && (!slots || !z_out))) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (n <= 0) return NEP_OK;
  if (n > m.max_batch) return fail(NEP_ERR_ARG, "n > max_batch");
  for (int b = 0; b < n; ++b) {
    if (slots[b] < 0 || slots[b] >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[slots[b]]) return fail(NEP_ERR_STATE, "slot is still iterating");
  }
  const size_t ni = (size_t)m.il.n_int;
  if (!m.h_sols) {
    void *hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(double) * m.max_batch * (ni + 1)) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (solutions)");
    m.h_sols = static_cast<double *>(hp);
  }
  int rc;
  if (!m.d_sols && (rc = dalloc(m, &m.d_sols, (size_t)m.max_batch * ni))) return rc;
  // (the certified point for a certified LP, else the iterate — solution_z's choice, made on the device)
  int32_t *hs = reinterpret_cast<int32_t *>(m.h_sols + (size_t)m.max_batch * ni);
  std::memcpy(hs, slots, n * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(m.d_new, hs, n * sizeof(int32_t), hipMemcpyHostToDevice, m.aux));
  HIPCHK(launch_gather_solutions(m.v, m.d_new, n, (int)ni, m.d_sols, m.aux));
  HIPCHK(hipMemcpyAsync(m.h_sols, m.d_sols, (size_t)n * ni * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  std::memcpy(z_out, m.h_sols, sizeof(double) * n * ni);
  return NEP_OK;
}

int nep_lp_get_flows_solutions(void *model, int32_t n, const int32_t *slots, float *flows_out, double *z_out) {
  if (!model || (n > 0 && (!slots || !flows_out || !z_out))) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (n <= 0) return NEP_OK;
  if (n > m.max_batch) return fail(NEP_ERR_ARG, "n > max_batch");
  for (int b = 0; b < n; ++b) {
    if (slots[b] < 0 || slots[b] >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[slots[b]]) return fail(NEP_ERR_STATE, "slot is still iterating");
  }
  const size_t ni = (size_t)m.il.n_int, plane = (size_t)m.max_batch * m.F * m.N;
  int rc;
  if (!m.d_flows && (rc = dalloc(m, &m.d_flows, 2 * plane))) return rc;
  if (!m.d_sols && (rc = dalloc(m, &m.d_sols, (size_t)m.max_batch * ni))) return rc;
  if (!m.h_flows) {
    void *h = nullptr;
    if (hipHostMalloc(&h, sizeof(float) * 2 * plane + sizeof(int32_t) * m.max_batch) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (flows)");
    m.h_flows = static_cast<float *>(h);
  }
  if (!m.h_sols) {
    void *hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(double) * m.max_batch * (ni + 1)) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (solutions)");
    m.h_sols = static_cast<double *>(hp);
  }
  // nep_lp_get_flows + nep_lp_get_solutions with one slot list, both gathers and one wait
  int32_t *hs = reinterpret_cast<int32_t *>(m.h_flows + 2 * plane);
  std::memcpy(hs, slots, n * sizeof(int32_t));
  const size_t cnt = (size_t)n * m.F * m.N;
  HIPCHK(hipMemcpyAsync(m.d_new, hs, n * sizeof(int32_t), hipMemcpyHostToDevice, m.aux));
  HIPCHK(launch_node_flows(m.v, m.d_new, n, m.d_flows, nullptr, m.aux));
  HIPCHK(launch_gather_solutions(m.v, m.d_new, n, (int)ni, m.d_sols, m.aux));
  HIPCHK(hipMemcpyAsync(m.h_flows, m.d_flows, cnt * sizeof(float), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipMemcpyAsync(m.h_sols, m.d_sols, (size_t)n * ni * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  std::memcpy(flows_out, m.h_flows, cnt * sizeof(float));
  std::memcpy(z_out, m.h_sols, sizeof(double) * n * ni);
  return NEP_OK;
}

static const char *const kRcRefusal =
    "reduced costs are kept by facility-relaxation models only (NEP_RELAX_FACILITY): the reference relaxation's bound "
    "uses repaired big-M prices and, in step 2, the exact disruption block";

// scratch of the reduced-cost calls, on first use
static int ensure_rc(Model &m) {
  const size_t ni = (size_t)m.il.n_int, B = (size_t)m.max_batch;
  if (!m.h_rc) {
    void *hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(double) * B * (ni + 2)) != hipSuccess)
      return fail(NEP_ERR_NOMEM, "hipHostMalloc (reduced costs)");
    m.h_rc = static_cast<double *>(hp);
  }
  int rc;
  if (!m.d_rc && (rc = dalloc(m, &m.d_rc, B * (ni + 1)))) return rc;
  if (!m.d_rccnt) {
    const size_t chunks = (ni + 63) / 64;
    if ((rc = dalloc(m, &m.d_rccnt, chunks + 1))) return rc;
    if ((rc = dalloc(m, &m.d_rcoff, chunks + 1))) return rc;
    if ((rc = dalloc(m, &m.d_rcidx, ni))) return rc;
    if ((rc = dalloc(m, &m.d_rcval, ni))) return rc;
  }
  return NEP_OK;
}

int nep_lp_get_reduced_costs(void *model, int32_t n, const int32_t *slots, double *rc_out, double *bound_out) {
  if (!model || (n > 0 && (!slots || !rc_out || !bound_out))) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (!m.fac) return fail(NEP_ERR_ARG, kRcRefusal);
  if (n <= 0) return NEP_OK;
  if (n > m.max_batch) return fail(NEP_ERR_ARG, "n > max_batch");
  for (int b = 0; b < n; ++b) {
    if (slots[b] < 0 || slots[b] >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[slots[b]]) return fail(NEP_ERR_STATE, "slot is still iterating");
    if (m.rc_stale[slots[b]]) return fail(NEP_ERR_STATE, "slot " + std::to_string(slots[b]) + " has no certificate check yet");
  }
  int rc = ensure_rc(m);
  if (rc) return rc;
  const size_t ni = (size_t)m.il.n_int;
  // one gather and one copy back: the n rows, then the n bounds behind them
  int32_t *hs = reinterpret_cast<int32_t *>(m.h_rc + (size_t)m.max_batch * (ni + 1));
  std::memcpy(hs, slots, n * sizeof(int32_t));
  double *d_bound = m.d_rc + (size_t)n * ni;
  HIPCHK(hipMemcpyAsync(m.d_new, hs, n * sizeof(int32_t), hipMemcpyHostToDevice, m.aux));
  HIPCHK(launch_gather_reduced_costs(m.v, m.d_new, n, (int)ni, m.d_rc, d_bound, m.aux));
  HIPCHK(hipMemcpyAsync(m.h_rc, m.d_rc, (size_t)n * (ni + 1) * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  const double *hb = m.h_rc + (size_t)n * ni;
  for (int b = 0; b < n; ++b)
    if (!(hb[b] > -INF)) return fail(NEP_ERR_STATE, "slot " + std::to_string(slots[b]) + " has no certificate check yet");
  std::memcpy(rc_out, m.h_rc, sizeof(double) * n * ni);
  std::memcpy(bound_out, hb, sizeof(double) * n);
  return NEP_OK;
}

int nep_lp_rc_fixings(void *model, int32_t slot, double cutoff, int64_t capacity, int64_t *n_fix, int32_t *idx,
                      double *val) {
  if (!model || !n_fix) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (!m.fac) return fail(NEP_ERR_ARG, kRcRefusal);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  if (cutoff != cutoff) return fail(NEP_ERR_ARG, "cutoff is NaN");
  const std::string none = "slot " + std::to_string(slot) + " has no certificate check yet";
  if (m.rc_stale[slot]) return fail(NEP_ERR_STATE, none);
  int rc = ensure_rc(m);
  if (rc) return rc;
  const int ni = m.il.n_int, chunks = (ni + 63) / 64;
  HIPCHK(launch_rc_fixings(m.v, slot, cutoff, ni, m.d_rccnt, m.d_rcoff, nullptr, nullptr, true, m.aux));
  // the total and the slot's kept bound in one wait
  int32_t total = 0;
  double lagr = -INF;
  HIPCHK(hipMemcpyAsync(&total, m.d_rcoff + chunks, sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipMemcpyAsync(&lagr, &m.v.ctrl[slot].rc_lagr, sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  if (!(lagr > -INF)) return fail(NEP_ERR_STATE, none);
  *n_fix = total;
  if (capacity < total || total == 0) return NEP_OK;   // size query (or nothing to write)
  if (!idx || !val) return fail(NEP_ERR_ARG, "null argument");
  HIPCHK(launch_rc_fixings(m.v, slot, cutoff, ni, m.d_rccnt, m.d_rcoff, m.d_rcidx, m.d_rcval, false, m.aux));
  HIPCHK(hipMemcpyAsync(idx, m.d_rcidx, total * sizeof(int32_t), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipMemcpyAsync(val, m.d_rcval, total * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int nep_lp_get_solution(void *model, int32_t slot, double *z_int, float *x_dense) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  if (z_int) {
    const double *z = nullptr;
    int rc = solution_z(m, slot, &z);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(z_int, z, m.il.n_int * sizeof(double), hipMemcpyDeviceToHost, m.aux));
  }
  if (x_dense) {
    std::vector<float> xb((size_t)m.R * m.NP);
    HIPCHK(hipMemcpyAsync(xb.data(), m.v.x + (size_t)slot * m.v.sx, xb.size() * sizeof(float), hipMemcpyDeviceToHost,
                          m.aux));
    HIPCHK(hipStreamSynchronize(m.aux));
    const int N = m.N, F = m.F;
    for (int r = 0; r < m.R; ++r) {
      const int f = m.row_f[r], src = m.row_src[r];
      const float *xr = &xb[(size_t)r * m.NP];
      for (int i = 0; i < N; ++i) {
        const bool member = src >= 0 ? (i == src) : (m.W[(size_t)f * N + i] == 0.0);
        if (!member) continue;
        std::memcpy(&x_dense[((size_t)i * F + f) * N], xr, N * sizeof(float));   // [i][f][j]
      }
    }
  }
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int nep_lp_get_rows(void *model, int32_t slot, float *xbar, int32_t *row_f, int32_t *row_src) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (xbar && m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  if (xbar) {
    HIPCHK(hipMemcpy2DAsync(xbar, m.N * sizeof(float), m.v.x + (size_t)slot * m.v.sx, m.NP * sizeof(float),
                            m.N * sizeof(float), m.R, hipMemcpyDeviceToHost, m.aux));
    HIPCHK(hipStreamSynchronize(m.aux));
  }
  if (row_f) std::memcpy(row_f, m.row_f.data(), m.R * sizeof(int32_t));
  if (row_src) std::memcpy(row_src, m.row_src.data(), m.R * sizeof(int32_t));
  return NEP_OK;
}

static_assert(sizeof(Ctrl) % 4 == 0, "copy_segments copies 4-byte words");

int nep_lp_copy_state(void *model, int32_t src, int32_t dst) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (src < 0 || dst < 0 || src >= m.max_batch || dst >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[dst]) return fail(NEP_ERR_STATE, "destination slot is still iterating");
  // (the copy runs on the aux stream, not ordered after the block in flight: an iterating source would
  // be read while the block rewrites it)
  if (m.busy[src]) return fail(NEP_ERR_STATE, "source slot is still iterating");
  if (src == dst) return NEP_OK;
  const DeviceView &v = m.v;
  // every per-slot array of the iterate, in one launch (copy_segments)
  SlotCopy c{};
  auto seg = [&](auto *base, int64_t stride) {
    c.src[c.n] = reinterpret_cast<const char *>(base + src * stride);
    c.dst[c.n] = reinterpret_cast<char *>(base + dst * stride);
    c.bytes[c.n] = stride * (int64_t)sizeof(*base);
    ++c.n;
  };
  seg(v.x, v.sx);
  seg(v.theta, (int64_t)m.R);
  seg(v.zi, v.sint);
  seg(v.y, v.sdual);
  seg(v.kty, v.skty);
  // the certificate's repaired point travels with the status it belongs to: solution_z() of a copied
  // certified slot returns the source's repaired point, not the destination's stale one
  seg(v.zr, v.sint);
  seg(v.rpart, v.srpart);
  seg(v.ctrl, (int64_t)1);
  if (m.fac) {   // the x <= c duals and their per-(f, j) sums travel with the state
    seg(v.lam, v.sx);
    seg(v.lsum, v.slsum);
    seg(v.rcbuf, v.srcbuf);   // the kept reduced costs travel with the Ctrl fields that name them (rc_best, rc_lagr)
  }
  static_assert(SlotCopy::kMax >= 11, "a facility slot copies 11 segments");
  m.rc_stale[dst] = m.rc_stale[src];
  HIPCHK(launch_copy_segments(c, m.aux));
  // no host wait: every later use of src / dst is ordered behind these copies — host reads and submits run
  // on `aux`, and a slot iterates on `stream` only after its submit's initialisation (ev_aux)
  return NEP_OK;
}

int nep_lp_copy_states(void *model, int32_t n, const int32_t *src, const int32_t *dst) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  for (int k = 0; k < n; ++k) {
    if (src[k] < 0 || dst[k] < 0 || src[k] >= m.max_batch || dst[k] >= m.max_batch)
      return fail(NEP_ERR_ARG, "slot out of range");
    if (m.busy[dst[k]]) return fail(NEP_ERR_STATE, "destination slot is still iterating");
    if (m.busy[src[k]]) return fail(NEP_ERR_STATE, "source slot is still iterating");
  }
  const DeviceView &v = m.v;
  SlotCopyN c{};
  auto seg = [&](auto *base, int64_t stride) {
    c.base[c.nseg] = reinterpret_cast<char *>(base);
    c.stride[c.nseg] = stride * (int64_t)sizeof(*base);
    ++c.nseg;
  };
  // the arrays nep_lp_copy_state copies
  seg(v.x, v.sx);
  seg(v.theta, (int64_t)m.R);
  seg(v.zi, v.sint);
  seg(v.y, v.sdual);
  seg(v.kty, v.skty);
  seg(v.zr, v.sint);
  seg(v.rpart, v.srpart);
  seg(v.ctrl, (int64_t)1);
  if (m.fac) {
    seg(v.lam, v.sx);
    seg(v.lsum, v.slsum);
    seg(v.rcbuf, v.srcbuf);
  }
  static_assert(SlotCopyN::kSeg >= 11, "a facility slot copies 11 segments");
  // the same result as n nep_lp_copy_state calls in order: a launch takes pairs while none of them reads or writes
  // a slot an earlier pair of the launch writes, or writes a slot an earlier pair reads
  std::vector<int32_t> rd, wr;
  auto flush = [&]() -> int {
    if (c.npairs) HIPCHK(launch_copy_slots(c, m.aux));
    c.npairs = 0;
    rd.clear();
    wr.clear();
    return NEP_OK;
  };
  auto has = [](const std::vector<int32_t> &a, int32_t x) { return std::find(a.begin(), a.end(), x) != a.end(); };
  for (int k = 0; k < n; ++k) {
    if (src[k] == dst[k]) continue;
    if (c.npairs == SlotCopyN::kPairs || has(wr, src[k]) || has(wr, dst[k]) || has(rd, dst[k])) {
      const int rc = flush();
      if (rc) return rc;
    }
    c.src[c.npairs] = src[k];
    c.dst[c.npairs] = dst[k];
    m.rc_stale[dst[k]] = m.rc_stale[src[k]];
    ++c.npairs;
    rd.push_back(src[k]);
    wr.push_back(dst[k]);
  }
  // (no host wait, as nep_lp_copy_state)
  return flush();
}

int nep_lp_copy_routing(void *dst_model, int32_t dst_slot, void *src_model, int32_t src_slot) {
  if (!dst_model || !src_model) return fail(NEP_ERR_ARG, "null model");
  Model &d = *static_cast<Model *>(dst_model);
  Model &s = *static_cast<Model *>(src_model);
  if (dst_slot < 0 || dst_slot >= d.max_batch || src_slot < 0 || src_slot >= s.max_batch)
    return fail(NEP_ERR_ARG, "slot out of range");
  if (d.busy[dst_slot]) return fail(NEP_ERR_STATE, "destination slot is still iterating");
  if (s.busy[src_slot]) return fail(NEP_ERR_STATE, "source slot is still iterating");
  if (d.R != s.R || d.N != s.N || d.NP != s.NP || d.F != s.F || d.row_f != s.row_f || d.row_src != s.row_src)
    return fail(NEP_ERR_ARG, "the two models' routing rows differ");
  if (&d == &s && dst_slot == src_slot) return NEP_OK;
  // the source's own queued work on its slot first (its aux stream); then the copies on the destination's
  // aux stream, waited for: the source model may rewrite its slot on its own streams right after this call
  HIPCHK(hipStreamSynchronize(s.aux));
  HIPCHK(hipMemcpyAsync(d.v.x + dst_slot * d.v.sx, s.v.x + src_slot * s.v.sx, d.v.sx * sizeof(float),
                        hipMemcpyDeviceToDevice, d.aux));
  HIPCHK(hipMemcpyAsync(d.v.theta + dst_slot * d.R, s.v.theta + src_slot * s.R, d.R * sizeof(float),
                        hipMemcpyDeviceToDevice, d.aux));
  HIPCHK(hipStreamSynchronize(d.aux));
  return NEP_OK;
}

int nep_lp_set_params(void *model, double tol, double cutoff) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  Model &m = *static_cast<Model *>(model);
  if (tol > 0) m.run.tol = tol;
  m.run.cutoff = cutoff;
  HIPCHK(set_prm(m, m.run.tol, m.run.cutoff, m.run.gap_tol));
  HIPCHK(hipStreamSynchronize(m.aux));
  return NEP_OK;
}

int nep_lp_set_reference_weight(void *model, double omega_ref) {
  if (!model) return fail(NEP_ERR_ARG, "null model");
  if (!(omega_ref >= 0.0) || !std::isfinite(omega_ref)) return fail(NEP_ERR_ARG, "omega_ref must be finite and >= 0");
  static_cast<Model *>(model)->omega_ref = omega_ref;
  return NEP_OK;
}

int nep_lp_get_flows(void *model, int32_t n, const int32_t *slots, float *flows_out) {
  if (!model || (n > 0 && (!slots || !flows_out))) return fail(NEP_ERR_ARG, "null argument");
  return flows(*static_cast<Model *>(model), n, slots, flows_out);
}

int nep_lp_get_flows_split(void *model, int32_t n, const int32_t *slots, float *flows_out, float *wflows_out) {
  if (!model || (n > 0 && (!slots || !flows_out || !wflows_out))) return fail(NEP_ERR_ARG, "null argument");
  return flows(*static_cast<Model *>(model), n, slots, flows_out, wflows_out);
}

int nep_lp_routing_entries(void *model, int32_t slot, double threshold, int32_t round3, int64_t capacity,
                           int64_t *n_entries, int32_t *row, int32_t *dst, double *val) {
  if (!model || !n_entries) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  return compact<float>(m, m.v.x + (size_t)slot * m.v.sx, m.R, m.N, m.NP, threshold, round3, capacity, n_entries, row,
                        dst, val);
}

int nep_lp_allocation_entries(void *model, int32_t slot, double threshold, int64_t capacity, int64_t *n_entries,
                              int32_t *fn, int32_t *dst) {
  if (!model || !n_entries) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  const double *z = nullptr;
  int rc = solution_z(m, slot, &z);
  if (rc) return rc;
  return compact<double>(m, z + m.il.oc, m.F, m.N, m.N, threshold, 0, capacity, n_entries, fn, dst, nullptr);
}

int nep_lp_score_check(void *model, int32_t slot, double *out) {
  if (!model || !out) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  if (m.busy[slot]) return fail(NEP_ERR_STATE, "slot is still iterating");
  return score_check(m, slot, out);
}

int nep_lp_get_diag(void *model, int32_t slot, double *out16) {
  if (!model || !out16) return fail(NEP_ERR_ARG, "null argument");
  Model &m = *static_cast<Model *>(model);
  if (slot < 0 || slot >= m.max_batch) return fail(NEP_ERR_ARG, "slot out of range");
  Ctrl c;
  // read on the auxiliary stream: submits and state copies are enqueued there without a host
  // wait, so a blocking copy on the null stream could see a slot's Ctrl before they ran
  HIPCHK(hipMemcpyAsync(&c, m.v.ctrl + slot, sizeof(Ctrl), hipMemcpyDeviceToHost, m.aux));
  HIPCHK(hipStreamSynchronize(m.aux));
  const double vals[16] = {c.pobj, c.lagr, c.best_lagr, c.pres, c.gap, c.omega, c.tau, c.sigma, c.eta,
                           (double)c.k, (double)c.k_since_restart, (double)c.status, (double)c.active,
                           c.last_restart_fpr, c.prev_fpr, m.sigma_max};
  std::memcpy(out16, vals, sizeof(vals));
  return NEP_OK;
}

int nep_get_stats(void *model, nep_stats *stats) {
  if (!model || !stats) return fail(NEP_ERR_ARG, "null argument");
  *stats = static_cast<Model *>(model)->stats;
  return NEP_OK;
}

void nep_reset_stats(void *model) {
  if (model) static_cast<Model *>(model)->stats = nep_stats{};
}

}  // extern "C"
