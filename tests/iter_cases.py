"""Instances, node boxes and the launch-tile rule shared by the kernel-vs-mirror tests (test_gpu_iterates.py, the wide
read-out cases of test_gpu_aux.py) and their CPU checks (test_abi.py).

Instances (F = 4 functions, N nodes, MinDelayAndUtilization): every number the kernels hold in float32 is exactly
representable there (integer delays and workloads, core_per_req = k / 1024), so the fp64 mirror and the engine
iterate on the same data.  Function 0 has workload on every source (N loaded rows, no pooled row: the leaf box's
forced-open columns can only be filled by loaded rows, which keeps the C2 duals y2 busy); functions 1-3 have 8 loaded
sources and one pooled row.  Node cores are about 0.02 x the generator's usual ones (k / 64, k = 8 .. 64), so the CPU rows
C5 stay active on ~10 % of the nodes while the routing settles; the nodes a leaf box opens have the capacity to hold
everything except one small node per 256-destination chunk.
"""
import numpy as np

F = 4
CHECK_EVERY = 16
SNAPSHOTS = (1, 17, 33, 49, 65)          # certificate iterations compared (k of the engine's Ctrl)
EXTRA_CHUNK = (26, 258, 514, 1026)       # one chunk past a lane boundary, and padding (N % 4 == 2)
SLOT_COUNTS = (1, 128, 256)              # slots x F = 4 / 512 / 1024: the three tile sizes
LDS_CAP = 144 * 1024
KINDS = ("INIT", "CHECK", "FIRST", "STEADY")


VARIANT, ALPHA = "MinDelayAndUtilization", 0.5
# step 2 (delete): a score bound the uniform start violates and the settled routing meets, so the score row's dual
# moves (measured on the mirror; test_gpu_iterates.py asserts it from the mirror's records)
STEP2_KW = dict(max_score=20.0)          # (rhs 26 against a score of 48.7 at the uniform start)


def model_kw(step):
    return dict(alpha=ALPHA, **(STEP2_KW if step != 1 else {}))


def full_width():
    """Full rows (N = NP - 2 still pads two columns) at the production tile only."""
    return (254, 510, 1022, max_nodes())


def matrix():
    """(N, step, iterating slots, box of a lone slot or None: slots alternate root / leaf) of every engine run of
    test_gpu_iterates.py."""
    runs = []
    for N in EXTRA_CHUNK:
        for ns in SLOT_COUNTS:
            runs += [(N, 1, ns, box) for box in ((0, 1) if ns == 1 else (None,))]
    runs += [(258, 2, 2, None)]
    runs += [(N, 1, 256, None) for N in full_width()]
    return runs


def padded(N):
    return (N + 3) // 4 * 4


def cpl_of(N):
    chunks = padded(N) // 4
    return 1 if chunks <= 64 else 2 if chunks <= 128 else 4 if chunks <= 256 else 8


def x_lds_bytes(tw, NP, check, inline_reflect=False):
    """nep_internal.h x_lds_bytes."""
    return (2 * tw + 2) * NP * 4 + (((3 if inline_reflect else 2) * tw * NP * 4 + 4 * NP * 8) if check else 0)


def max_nodes(inline_reflect=False):
    """The largest N nep_model_create admits: the certificate pass at 4 waves within the LDS cap."""
    NP = 4
    while x_lds_bytes(4, NP + 4, True, inline_reflect) <= LDS_CAP:
        NP += 4
    return NP


def tile_waves(N, nslots, check, n_functions=F):
    """nep_kernels.hip tile_waves: waves per x_pass workgroup."""
    tw = 4
    while tw < 16 and nslots * n_functions * tw < 4096:
        tw *= 2
    if cpl_of(N) >= 8 and tw > 8:
        tw = 8
    while check and tw > 4 and x_lds_bytes(tw, padded(N), True) > LDS_CAP:
        tw //= 2
    return tw


def variants(N, nslots):
    """(CPL, TW, pass kind) of the x_pass launches of a cold LP batch of `nslots` slots."""
    return {(cpl_of(N), tile_waves(N, nslots, kind == "CHECK"), kind) for kind in KINDS}


def dispatchable():
    """Every (CPL, TW, pass kind) the launchers can dispatch for F = 4 at some admitted N and slot count."""
    out = set()
    for N in range(1, max_nodes() + 1):
        for ns in (1, 64, 127, 128, 255, 256, 1024):
            out |= variants(N, ns)
    return out


def leaf_open(N, f):
    """Open destinations of function f in the leaf box (at most 16): j = 0 and N - 1, both sides of 255 | 256, two
    inside one 16-byte chunk, and one in every 256-destination chunk index q = j >> 8 the width has (the register
    index of a sparse anchor pair), the last one included."""
    js = {0, N - 1, 8, 9, 255, 256} | set(chunk_nodes(N, f))
    if N < 64:
        js |= {13 + f}
    return sorted(j for j in js if 0 <= j < N)


def chunk_nodes(N, f):
    """Function f's own open node in every 256-destination chunk index: 256 q + 3 + f, or the chunk's first + f
    where the last chunk is that short (never the last node, which has its own role)."""
    out = []
    for q in range((padded(N) + 255) // 256):
        j = 256 * q + 3 + f
        if j >= N - 1:
            j = 256 * q + f
        if j < N - 1:
            out.append(j)
    return out


def leaf_nodes(N):
    return sorted({j for f in range(F) for j in leaf_open(N, f)})


def instance(N, step=1, seed=0):
    """Data of the N-node instance (see the module docstring); step 2: two old placements per function.
    What keeps the duals busy (the mirror's records show it; test_gpu_iterates.py asserts it):
      * y1 (C1): every entry is nonzero after the first iteration of a root LP (c = 0 under positive flow);
      * y2 (C2): function 0's own open nodes of the leaf box are 100 away from every source, itself included, so no
        row of function 0 routes there, the forced c = 1 stays unserved and its C2 dual grows, in every chunk index;
      * y5 (C5): ordinary nodes have ~0.02 x the usual cores; function 1's own open nodes have 1/16 core and a source
        with workload 50 right beside each (delay 0); the last node has 1/64 core and its own workload 8;
      * nodes 0, 8 and 9 can each hold the whole workload, so every box here is feasible."""
    from core.utils.data import Data
    rng = np.random.default_rng(1000 * N + seed)
    D = rng.integers(1, 100, size=(N, N))
    np.fill_diagonal(D, 0)
    free = np.setdiff1d(np.arange(N), leaf_nodes(N))
    W = np.zeros((F, N), np.int64)
    W[0] = rng.integers(1, 9, size=N)
    W[0, N - 1] = 8
    loaded = {}
    for f in range(1, F):
        loaded[f] = np.sort(rng.choice(free, size=min(8, free.size), replace=False))
        W[f, loaded[f]] = rng.integers(1, 51, size=loaded[f].size)
    cpr = rng.integers(10, 103, size=(F, N)) / 1024.0
    cpr[0, N - 1] = 64 / 1024.0
    cores = rng.integers(8, 65, size=N) / 64.0
    node_mem = rng.integers(64, 257, size=N).astype(float)
    fn_mem = rng.integers(4, 33, size=F).astype(float)
    for j in chunk_nodes(N, 0):
        D[:, j] = 100
    for q, j in enumerate(chunk_nodes(N, 1)):
        D[loaded[1][q], j] = 0
        W[1, loaded[1][q]] = 50
        cores[j] = 1.0 / 16
    cores[N - 1] = 1.0 / 64
    load = float((W * cpr.max(axis=1, keepdims=True)).sum())        # an upper bound on any routing's CPU load
    for j in (0, 8, 9):
        cores[j] = float(2 ** np.ceil(np.log2(load)))
    node_mem[leaf_nodes(N)] = 256.0
    d = Data([f"node_{i}" for i in range(N)], [f"ns/fn_{f}" for f in range(F)])
    d.node_memory_matrix = node_mem
    d.function_memory_matrix = fn_mem
    d.node_delay_matrix = D
    d.workload_matrix = W
    d.cores_matrix = cpr
    d.core_per_req_matrix = cpr
    d.max_delay_matrix = np.full(F, 1000)
    d.response_time_matrix = np.zeros((F, N), np.int64)
    d.node_cores_matrix = cores
    old = np.zeros((F, N), np.int64)
    for f in range(F):
        old[f, rng.choice(N, size=2, replace=False)] = 1
    d.old_allocations_matrix = old if step != 1 else np.ones_like(old)
    d.node_costs = np.full(N, 5)
    d.node_budget = 300
    return d


def boxes(N, n_int, step=1):
    """[2, n_int] lower / upper bounds: the root box (no fixing) and the leaf-type box (c = 1 on leaf_open, 0
    elsewhere; everything else free).  Step 2 (delete: sum c may not grow past the two old placements per function)
    leaves c free on leaf_open instead of forcing it to 1."""
    lb = np.full((2, n_int), -np.inf)
    ub = np.full((2, n_int), np.inf)
    ub[1, :F * N] = 0.0
    for f in range(F):
        for j in leaf_open(N, f):
            ub[1, f * N + j] = 1.0
            if step == 1:
                lb[1, f * N + j] = 1.0
    return lb, ub
