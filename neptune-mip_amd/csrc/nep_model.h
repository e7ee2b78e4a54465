// nep_model.h — the host runtime's model: what the translation units carved out of the host runtime share (the
// model build, nep_model_build.cpp; the node presolve, nep_presolve.cpp; the solve loop and the ABI, nep_host.cpp; the
// fixed-placement evaluator's host side, nep_leaf_host.cpp; the debug entries, nep_debug.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/neptune_lp.h"
#include "nep_launch.h"   // (with it nep_internal.h and nep_leaf.h)

namespace nep {

int fail(int code, const std::string &msg);   // sets nep_last_error's thread-local message; returns code (nep_host.cpp)
#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return fail(NEP_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

static const double INF = std::numeric_limits<double>::infinity();

struct Coo {
  std::vector<int> r, c;
  std::vector<double> v;
  void add(int row, int col, double val) {
    r.push_back(row);
    c.push_back(col);
    v.push_back(val);
  }
};

// scratch of one presolve_node() call, reset after every node (one per thread)
struct PresolveScratch {
  std::vector<int> pos, fdelta, touched, ftouched;
  std::vector<double> dmin, dmax;
  std::vector<uint8_t> rowmark;
  std::vector<uint8_t> allow;   // [F*N] the node's allowed placements (CPU cover and score-row tests)
  // the changes of the nodes this thread presolved in the current batch (capacity kept across batches: a
  // rounding leaf's ~33k changes at 256x128 would otherwise page-fault fresh buffers on every submit)
  std::vector<int32_t> ci;
  std::vector<double> cl, cu;
};

// one presolved node box: its changes of the base box (m.psc[t].ci/cl/cu [off, off + cnt)), feasibility and
// whether it fixes the objective
struct NodeBox {
  int t = 0;
  size_t off = 0, cnt = 0;
  bool ok = false, ex = false;
  bool bad = false;   // reduced step 2: a fractional moved_from / moved_to bound (not representable)
};

struct Model {
  // NEP_HOST_PROFILE=1: host seconds of nep_lp_submit (presolve / staging + launches) and nep_lp_advance,
  // printed to stderr when the model is destroyed (dev measurement)
  bool prof = false;
  double pr_pre = 0, pr_stage = 0, pr_adv = 0;
  int64_t pr_calls = 0, pr_lps = 0, pr_adv_calls = 0;
  // problem
  int N = 0, F = 0, NP = 0, variant = 0, step = 1, has_n = 0, step2 = 0;
  int fac = 0;                      // NEP_RELAX_FACILITY (include/neptune_lp.h)
  std::vector<double> rhoL;         // fac: row scale of the x[r, j] <= c[f, j] rows, per (f, j)
  std::vector<double> capn;         // [2][N] node memory, node cores
  double alpha = 0.5, M = 1e6, eps = 1e-6, sigma4 = -1, cost_n = 0, score_n_coef = 0, w_dis = 0;
  int dred = 0;                     // step 2: the reduced disruption block (DeviceView::dred)
  Coo Ks;                           // the small-variable part of the matrix the iteration runs on (scaling, power)
  bool power_host = false;          // eta from the host power iteration (nep_debug_build) or the device's
  double sT = 0, sum_old = 0;       // dred: cost per unit of T = sum c - sum old; sum of the old allocation
  int R = 0, JB = 0, CPL = 1, max_batch = 1;
  DualLayout dl{};
  IntLayout il{};
  std::vector<int> row_f, row_src, frow;
  std::vector<float> row_m, row_w, row_wobj, row_wsc;
  std::vector<double> row_wsc_d;    // the score-row weights in fp64 (presolve's proofs; row_wsc is the kernels' fp32)
  std::vector<RowInfo> rows;
  std::vector<double> W;            // [F*N]
  std::vector<double> cprh;         // [F*N] core_per_req (the presolve's CPU cover test)
  std::vector<double> wsum;         // [F] sum_i W[f, i]
  std::vector<double> nat_lb, nat_ub, cost_int;
  std::vector<double> lo, hi, rownorm, rho, gam;
  std::vector<double> mem_f;
  // non-x part of K (COO) and, per function, the total routed flow (= N sources x 1): kept for the
  // per-node row-activity test of presolve()
  std::vector<int> Kr, Kc;
  std::vector<double> Kv, ftot;
  bool x_coef_nonneg = true;   // every x coefficient outside C1/C2 is >= 0 (W, cpr, D >= 0)
  // step 2: the score / delay row's routing coefficients wsc[r] * D[src, j] (presolve: the row's smallest
  // activity over the routing simplexes of a node's allowed destinations)
  bool score_x = false;
  std::vector<double> Dh;            // [N*N] delay matrix (step 2 with score_x only)
  bool x_cost_free = true;     // no routing entry carries objective cost (step 2; W == 0)
  // node presolve as a sparse change of the base box (presolve_setup / presolve_node)
  bool base_ok = false;
  std::vector<double> base_lb, base_ub, base_amin, base_amax;
  std::vector<uint8_t> base_mask;
  std::vector<int> base_cnt, Kcp, Kcr;
  std::vector<double> Kcv;
  std::vector<PresolveScratch> psc;   // one per presolve thread (submit presolves a batch's nodes in parallel)
  double eta = 0, sigma_max = 0, omega0 = 1.0;
  double omega_ref = 0.0;           // nep_lp_set_reference_weight (0: warm-start band relative to the parent)
  // device
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // auxiliary stream: work on slots that are NOT iterating — the initialisation of newly submitted
  // slots, warm-start copies and every read of a finished slot (flows, solution, compaction, scorers)
  // — so none of it queues behind the pipelined block on `stream`; ev_aux orders `stream` after it
  hipStream_t aux = nullptr;
  hipEvent_t ev_aux = nullptr;
  // slot groups (NEP_BLOCK_GROUPS, launch_block): the second group of a block's slots iterates on `grp`, forked
  // from `stream` (ev_fork) and joined back into it (ev_join) inside the block
  hipStream_t grp = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int groups = 1;                   // 1: one chain per block; 2: two slot groups where block_split allows
  DeviceView v{};
  std::vector<void *> allocs;
  double *d_prm = nullptr;      // {tol, cutoff} of the LPs in flight (DeviceView::prm)
  double prm_host[3] = {0, 0, 0};   // tol, cutoff, gap tol of the LPs in flight
  bool prm_sent = false;            // d_prm holds prm_host (a submit with the same values skips the copy)
  int32_t *d_slots = nullptr;   // the slots currently iterating (mirror of `act`)
  int32_t *h_act = nullptr;     // pinned staging of `act` for the d_slots upload (launch_block only)
  int32_t *d_new = nullptr;     // slots being initialised by nep_lp_submit
  double *d_base_lb = nullptr, *d_base_ub = nullptr;
  uint8_t *d_base_mask = nullptr;
  // a submit's uploads, one copy each: [slots | change offsets | change indices | exact flags] and
  // [change lower bounds | change upper bounds] (capacity: every integer variable of every slot)
  int32_t *d_sub_i = nullptr;
  double *d_sub_d = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  nep_stats stats{};
  // scratch of the auxiliary kernels (nep_aux.hip), allocated on first use
  float *d_flows = nullptr;                  // [max_batch][F][N]
  int32_t *d_cnt = nullptr, *d_off = nullptr;   // [max(R, F) + 1]
  int32_t *d_erow = nullptr, *d_ecol = nullptr;
  double *d_eval = nullptr;
  int64_t ecap = 0;
  double *d_score = nullptr;                 // cpu_fj [F][NP] | fpart [F][4] | jpart [N][6] | out [16]
  double *d_node_cost = nullptr;
  std::vector<double> node_cost;
  double node_budget = 0.0;
  // one block of check_every PDHG iterations as a captured HIP graph, per iterating-slot count
  // (the launch grids depend on it); rebuilt when check_every changes
  std::vector<hipGraphExec_t> block_graph;   // [max_batch + 1], index = slots iterating
  int graph_ce = 0;
  int64_t blocks = 0;
  bool graphs_ok = true;                     // false once capture failed on this stream: eager blocks
  // streaming state
  std::vector<int32_t> act;     // slots currently iterating
  std::vector<uint8_t> busy;    // per slot: iterating
  nep_lp_opts run{};            // options of the LPs in flight
  // pipelined blocks (advance): the block launched last, not yet waited for — the slots it iterates,
  // whether it carries the sampled x-pass events — and the pinned copy of the slots' Ctrl it ends with
  bool inflight = false, inflight_sampled = false;
  int pipe_max_done = INT_MAX;
  std::vector<int32_t> launched;
  Ctrl *h_ctrl = nullptr;
  float *h_flows = nullptr;     // pinned staging of nep_lp_get_flows(_split): [2][max_batch][F*N] + slots
  double *h_sols = nullptr;     // pinned staging of nep_lp_get_solutions: [max_batch][n_int] + the slot list
  double *d_sols = nullptr;     // [max_batch][n_int]: the gathered solutions (gather_solutions)
  // reduced costs of a facility model (nep_lp_get_reduced_costs / nep_lp_rc_fixings), allocated on first use
  double *h_rc = nullptr;       // pinned staging: [max_batch][n_int + 1] (the bounds behind the rows) + the slot list
  double *d_rc = nullptr;       // [max_batch][n_int + 1]: the gathered reduced costs, then the bounds
  int32_t *d_rccnt = nullptr, *d_rcoff = nullptr;   // [ceil(n_int / 64) + 1]: fixings per wave of 64 variables, their scan
  int32_t *d_rcidx = nullptr;   // [n_int] the compacted fixings
  double *d_rcval = nullptr;
  // per slot: the LP submitted last was refused by presolve, so the slot's kept reduced costs are an earlier LP's
  std::vector<uint8_t> rc_stale;
  // fixed-placement evaluator (nep_leaf_eval; step-1 reference models): the objective's routing scale, the instance's
  // fp64 delay matrix on the host (Dh; W / cprh / capn hold the rest), and — from the first call on — the
  // device workspace of one chunk of placements, its pinned staging and the last call's points
  double kobj = 0.0;
  struct LeafWork {
    int cap = 0, threads = 64;
    LeafView v{};
    void *pinned = nullptr;
    uint8_t *h_open = nullptr;
    LeafCtrl *h_ctrl = nullptr;
    double *h_y = nullptr, *h_load = nullptr;
    int32_t *h_asg0 = nullptr;
    std::vector<LeafPoint> points;
    // the per-round repair (nep_leaf_eval_ex with repair_every >= 1; nep_leaf_heur.hip), from its first use on: the
    // device arrays, the pinned staging of the best round's [best | loadrep | asgrep] and of round_upper (which grows
    // with the call's rounds)
    bool heur = false;
    LeafHeurView hv{};
    void *pinned_h = nullptr, *pinned_ru = nullptr;
    LeafHeurBest *h_best = nullptr;
    double *h_loadrep = nullptr, *h_ru = nullptr;
    int32_t *h_asgrep = nullptr;
    int ru_stride = 0;   // round_upper holds [cap][ru_stride]
    // the priced moves (nep_leaf_moves; nep_leaf_moves.hip), from their first use on: the pinned staging of a chunk's
    // [table | fpart] (on the device the table lives in v.share, dead outside an evaluator round)
    void *pinned_m = nullptr;
    double *h_table = nullptr, *h_fpart = nullptr;
    // the priced swaps (nep_leaf_swaps; nep_leaf_swaps.hip), from their first use on: the instance's memory figures,
    // a chunk's node state and records on the device and the pinned staging of [rec | fpart | mem | ncnt]; from the
    // first call that asks for the tables on: best_from on the device (best lives in v.share) and the pinned staging
    // of a chunk's [best | best_from]
    bool swaps = false;
    LeafSwapView sv{};
    void *pinned_s = nullptr, *pinned_st = nullptr;
    LeafSwapRec *h_rec = nullptr;
    double *h_sfpart = nullptr, *h_mem = nullptr, *h_sbest = nullptr;
    int32_t *h_ncnt = nullptr, *h_sfrom = nullptr, *d_sfrom = nullptr;
    // the native search (nep_leaf_search; nep_leaf_search.hip), from its first use on: a chunk's move records on the
    // device and their pinned staging, and the nodes that may not open (leaf_node_state's -1 mark)
    bool search = false;
    LeafSearchMove *d_mv = nullptr, *h_mv = nullptr;
    uint8_t *d_over = nullptr;
    void *pinned_q = nullptr;
    ~LeafWork() {
      if (pinned_q) (void)hipHostFree(pinned_q);
      if (pinned_s) (void)hipHostFree(pinned_s);
      if (pinned_st) (void)hipHostFree(pinned_st);
      if (pinned) (void)hipHostFree(pinned);
      if (pinned_h) (void)hipHostFree(pinned_h);
      if (pinned_ru) (void)hipHostFree(pinned_ru);
      if (pinned_m) (void)hipHostFree(pinned_m);
    }
  };
  std::unique_ptr<LeafWork> leaf;
  // pinned staging of nep_lp_submit's uploads (slots, change offsets / indices / bounds, exact flags): the
  // call returns without waiting for them; two stagings alternate, and a submit waits on the event of the
  // one it rewrites (recorded after that staging's copies, two submits earlier: normally long done)
  int32_t *h_sub_i[2] = {nullptr, nullptr};
  double *h_sub_d[2] = {nullptr, nullptr};
  size_t cap_sub_i[2] = {0, 0}, cap_sub_d[2] = {0, 0};
  hipEvent_t ev_sub[2] = {nullptr, nullptr};
  bool sub_pending[2] = {false, false};
  int sub_k = 0;
  ~Model() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (aux) (void)hipStreamSynchronize(aux);
    if (grp) (void)hipStreamSynchronize(grp);
    if (h_ctrl) (void)hipHostFree(h_ctrl);
    if (h_act) (void)hipHostFree(h_act);
    if (h_flows) (void)hipHostFree(h_flows);
    if (h_sols) (void)hipHostFree(h_sols);
    if (h_rc) (void)hipHostFree(h_rc);
    leaf.reset();   // (its pinned buffers: after the streams above have drained)
    for (int k = 0; k < 2; ++k) {
      if (h_sub_i[k]) (void)hipHostFree(h_sub_i[k]);
      if (h_sub_d[k]) (void)hipHostFree(h_sub_d[k]);
      if (ev_sub[k]) (void)hipEventDestroy(ev_sub[k]);
    }
    for (void *p : allocs) (void)hipFree(p);
    for (hipGraphExec_t g : block_graph)
      if (g) (void)hipGraphExecDestroy(g);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_aux) (void)hipEventDestroy(ev_aux);
    if (aux) (void)hipStreamDestroy(aux);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (grp) (void)hipStreamDestroy(grp);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

template <typename T>
int dalloc(Model &m, T **p, size_t n) {
  void *q = nullptr;
  if (n == 0) n = 1;
  hipError_t e = hipMalloc(&q, n * sizeof(T));
  if (e != hipSuccess) return fail(NEP_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  m.allocs.push_back(q);
  *p = static_cast<T *>(q);
  return NEP_OK;
}
template <typename T>
int upload(Model &m, const T **dst, const std::vector<T> &src) {
  T *p = nullptr;
  int rc = dalloc(m, &p, src.size());
  if (rc) return rc;
  if (!src.empty()) {
    hipError_t e = hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(NEP_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  *dst = p;
  return NEP_OK;
}

// nep_model_build.cpp
int build(Model &m, const nep_model_desc &d, bool host_power = true);
int setup_device(Model &m, int max_batch, void *stream);
int setup_dense(Model &m, const nep_model_desc &d);
int power_device(Model &m);

// nep_presolve.cpp
bool presolve_full(const Model &m, const double *lbi, const double *ubi, std::vector<double> &lb,
                   std::vector<double> &ub, std::vector<uint8_t> &mask);
void presolve_setup(Model &m);
void presolve_batch(Model &m, int n, const double *lbi, const double *ubi, std::vector<NodeBox> &box);

// nep_leaf_host.cpp — what the evaluator's debug entries (nep_debug.cpp) share with it
extern const char *const kLeafRefusal;
LeafInstance leaf_instance(const Model &m);
LeafLimits leaf_limits(const Model &m);
bool leaf_binary(const Model &m, const double *z, uint8_t *c_open, double *nsum);
bool leaf_rejects(const Model &m, const double *z, const uint8_t *c_open);
void leaf_point_out(const LeafPoint &pt, int32_t *row, int32_t *dst, double *val);
void leaf_moves_out(const std::vector<LeafMove> &mv, int max_moves, int32_t *n_moves, int32_t *kind, int32_t *fn,
                    int32_t *node, double *delta);
void leaf_swaps_out(const std::vector<LeafSwap> &sw, int max_moves, int32_t *n_moves, int32_t *fn, int32_t *from,
                    int32_t *to, double *delta);
int ensure_leaf(Model &m);          // the evaluator's workspace, on first use
int ensure_leaf_search(Model &m);   // the native search's part of it (after ensure_leaf)
LeafView leaf_view_at(const LeafView &v, size_t s, int B);   // the view of the B slots from slot s on
}  // namespace nep
