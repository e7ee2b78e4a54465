"""Instances, node boxes and the launch-tile rule shared by the kernel-vs-mirror tests (test_gpu_iterates.py, the wide
read-out cases of test_gpu_aux.py) and their CPU checks (test_abi.py); at the end of the file the same for the
facility relaxation (test_gpu_fac_iterates.py, test_ref_fac.py).

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


# the tight variant (memory rows C3 and the C7 rows active): see instance() and boxes()
TIGHT_FN_MEM = (16.0, 15.0, 14.0, 13.0)
TIGHT_NODE_MEM = 14.5
TIGHT_LAST_FN = 3                        # the smallest function: the only one the tight leaf box forces on the last node
WIDE_F = 67                              # node_pass sums per = ceil(F / 64) = 2 functions per group, last group short


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


def matrix_tight():
    """Runs on the tight instance, as (N, step, slots, box, tight, functions): the n-up box alone at every width, and
    256 slots cycling root / leaf / n-up at the widths of CPL 2 and 8."""
    return [(N, 1, 1, 2, True, F) for N in EXTRA_CHUNK] + [(N, 1, 256, None, True, F) for N in (258, 1026)]


def matrix_wide():
    """The F = WIDE_F run: root and leaf on the ordinary instance.  (Not the n-up box: at this F the mirror's records
    of it have a column deficit within the pooled / loaded shift's range at k = 49, which the mirror does not model,
    and the tight leaf box is infeasible, 17 functions sharing each forced node of TIGHT_NODE_MEM.)"""
    return [(26, 1, 2, None, False, WIDE_F)]


def normalise(run):
    """A run as (N, step, slots, box, tight, functions); box: None (slots cycle over every box of the instance) or the
    one box of every slot."""
    return tuple(run) + (False, F)[len(run) - 4:]


def slot_boxes(run):
    """Box index of every slot of a run."""
    N, step, ns, box, tight, nf = normalise(run)
    cyc = tuple(range(3 if tight else 2)) if box is None else (box,)
    return np.array([cyc[s % len(cyc)] for s in range(ns)])


def node_pass_groups(n_functions):
    """nep_kernels.hip node_pass: a node's 64 lanes each sum per = ceil(F / 64) consecutive functions; returns (per,
    lanes with a full share, functions of the one short lane or 0)."""
    per = (n_functions + 63) // 64
    return per, n_functions // per, n_functions % per


FLOOR = 64 * 2.0 ** -24
# Blocks of z / y that keep the bound of the whole array, max(8 d, FLOOR max(1, |mirror|)), instead of their own:
# name -> the measured numbers and the reason.
ABS_FLOOR_BLOCKS = {
    "y1": "at N >= 1022 the kernel is 18 .. 128 d_B and 1.5 .. 12 x the block's bound off at single snapshots where the "
          "block is nearly dead (N = 1022 root, k = 33: s_B 1.1e-14, d_B 3.4e-21, kernel 6.2e-20; N = 1026 tight root, "
          "k = 33: s_B 1.9e-15, d_B 6.9e-22, kernel 8.8e-20; N = 1026 warm n-up child, k = 1: s_B 2.3e-15, d_B 1.5e-21, "
          "kernel 3.5e-20): relative errors of 6e-6 .. 5e-5 in entries S - M c that cancel to 1e-9 of their terms, i.e. "
          "float32 noise of the column sums, of which the emulation's d_B at one snapshot is a single sample; emulating "
          "the float32 threshold sum and the row-by-row column sums did not raise that sample.  Every other snapshot "
          "and width held y1 within its own bound.",
}


def blocks_of(m):
    """{"z": [(name, offset, length)], "y": [...]} of a mirror model (ref_pdhg.RefModel): the blocks of the small
    primal and of the duals that test_gpu_iterates.py compares one by one (reduced step 2 does not iterate z beyond c
    and n; its idle disruption rows D1 / D2 / D3 are one block, which the mirror holds at 0)."""
    FN = m.F * m.N
    z = [("c", m.oc, FN), ("n", m.on, m.N)]
    y = [("y1", m.o1, FN), ("y2", m.o2, FN), ("y3", m.o3, m.N), ("y5", m.o5, m.N), ("y6", m.o6, m.N),
         ("y7", m.o7, m.N)]
    if m.step2:
        y += [("yD123", m.oD1, m.oD4 - m.oD1), ("yD4", m.oD4, 1), ("yS", m.oS, 1)]
    return {"z": z, "y": y}


def block_rows(blocks, got, ref, emu):
    """Per block B of one array: (name, d_B = max |fp32 emulation - fp64 mirror|, s_B = max |fp64 mirror|, err = max
    |got - fp64 mirror|, passes).  got is within max(8 d_B, FLOOR s_B) of the mirror — both terms relative to the
    block, and never beyond the bound this comparison had before it went block by block, max(8 d, FLOOR max(1,
    |mirror|)) with d over the whole array; a block the mirror holds at exactly 0 (s_B = 0) must be exactly 0 in got
    (either sign of zero: -0 is the same number)."""
    sel = np.concatenate([np.arange(o, o + n) for _, o, n in blocks])
    d_all = float(np.abs(emu[sel] - ref[sel]).max())
    rows = []
    for name, o, n in blocks:
        g, r, e = got[o:o + n], ref[o:o + n], emu[o:o + n]
        d, s = float(np.abs(e - r).max()), float(np.abs(r).max())
        err = np.abs(g - r)
        if s == 0.0:
            ok = not g.any()
        else:
            bound = np.minimum(max(8.0 * d, FLOOR * s), np.maximum(8.0 * d_all, FLOOR * np.maximum(1.0, np.abs(r))))
            ok = bool((err <= bound).all())
        rows.append((name, d, s, float(err.max()), ok))
    return rows


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


def variants(N, nslots, n_functions=F):
    """(CPL, TW, pass kind) of the x_pass launches of a cold LP batch of `nslots` slots."""
    return {(cpl_of(N), tile_waves(N, nslots, kind == "CHECK", n_functions), kind) for kind in KINDS}


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


def nup_nodes(N):
    """Nodes the n-up box opens (lb n = 1): function 2's own node of every 256-destination chunk index, and the
    last node."""
    return sorted(set(chunk_nodes(N, 2)) | {N - 1})


def instance(N, step=1, seed=0, tight=False, n_functions=F):
    """Data of the N-node instance (see the module docstring); step 2: two old placements per function.
    n_functions > 4: the further functions follow the recipe of functions 1-3 (8 loaded sources and a pooled row).
    tight: function f needs TIGHT_FN_MEM[f % 4] memory and the nodes of nup_nodes(N) have TIGHT_NODE_MEM: at least the
    smallest function's (the n-up box, n = 1 there, is feasible with that function alone) and below 0.3 x the
    functions' total, so the memory rows C3 there are violated while the c, pulled up by C7 under n = 1, overshoot.
    Neither option changes what the random generator draws: the default call returns the same data as before.
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
    nf = n_functions
    W = np.zeros((nf, N), np.int64)
    W[0] = rng.integers(1, 9, size=N)
    W[0, N - 1] = 8
    loaded = {}
    for f in range(1, nf):
        loaded[f] = np.sort(rng.choice(free, size=min(8, free.size), replace=False))
        W[f, loaded[f]] = rng.integers(1, 51, size=loaded[f].size)
    cpr = rng.integers(10, 103, size=(nf, N)) / 1024.0
    cpr[0, N - 1] = 64 / 1024.0
    cores = rng.integers(8, 65, size=N) / 64.0
    node_mem = rng.integers(64, 257, size=N).astype(float)
    fn_mem = rng.integers(4, 33, size=nf).astype(float)
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
    node_mem[leaf_nodes(N)] = max(256.0, float(2 ** np.ceil(np.log2(fn_mem.sum()))))     # (256 at F = 4)
    if tight:
        fn_mem = np.array([TIGHT_FN_MEM[f % F] for f in range(nf)])
        node_mem[nup_nodes(N)] = TIGHT_NODE_MEM
    d = Data([f"node_{i}" for i in range(N)], [f"ns/fn_{f}" for f in range(nf)])
    d.node_memory_matrix = node_mem
    d.function_memory_matrix = fn_mem
    d.node_delay_matrix = D
    d.workload_matrix = W
    d.cores_matrix = cpr
    d.core_per_req_matrix = cpr
    d.max_delay_matrix = np.full(nf, 1000)
    d.response_time_matrix = np.zeros((nf, N), np.int64)
    d.node_cores_matrix = cores
    old = np.zeros((nf, N), np.int64)
    for f in range(nf):
        old[f, rng.choice(N, size=2, replace=False)] = 1
    d.old_allocations_matrix = old if step != 1 else np.ones_like(old)
    d.node_costs = np.full(N, 5)
    d.node_budget = 300
    return d


def boxes(N, n_int, step=1, n_functions=F, tight=False):
    """[2, n_int] lower / upper bounds: the root box (no fixing) and the leaf-type box (c = 1 on leaf_open, 0
    elsewhere; everything else free).  Step 2 (delete: sum c may not grow past the two old placements per function)
    leaves c free on leaf_open instead of forcing it to 1.  (n_functions > F: function f opens leaf_open(N, f % F).)
    tight (step 1, the instance(tight=True) data): [3, n_int], the third row the n-up box — the root box with n = 1
    forced on nup_nodes(N), so C7 (sum_f c >= n) is violated at c = 0 and y7 moves from the first iteration, the c
    there rise until C3 (memory TIGHT_NODE_MEM) stops them, and y3 moves.  The tight leaf box forces only function
    TIGHT_LAST_FN (the smallest) at the last node and leaves the others open there: all of them at once do not fit
    its memory, and the engine's presolve proves such a box infeasible."""
    nb = 3 if tight else 2
    lb = np.full((nb, n_int), -np.inf)
    ub = np.full((nb, n_int), np.inf)
    ub[1, :n_functions * N] = 0.0
    for f in range(n_functions):
        for j in leaf_open(N, f % F):
            ub[1, f * N + j] = 1.0
            if step == 1:
                lb[1, f * N + j] = 1.0
    if tight:
        assert step == 1
        for f in range(n_functions):
            if f != TIGHT_LAST_FN:
                lb[1, f * N + N - 1] = -np.inf
        lb[2, n_functions * N + np.array(nup_nodes(N))] = 1.0
    return lb, ub


# ---------------------------------------------------------------------------------------------------------------
# facility relaxation (nep_fac.hip; test_gpu_fac_iterates.py and its CPU checks test_ref_fac.py)
# ---------------------------------------------------------------------------------------------------------------
FAC_WIDE_F = 67                          # fac_node_pass sums per = ceil(F / 64) = 2 functions per group, last group short


def fac_lds_bytes(tw, NP, check):
    """nep_internal.h fac_lds_bytes."""
    return ((2 if check else 1) * tw + tw + (tw if check else 0) + 3) * NP * 4 + 3 * NP * 8


def fac_max_nodes():
    """The largest N a facility model admits (nep_internal.h max_padded_width)."""
    NP = 4
    while fac_lds_bytes(4, NP + 4, True) <= LDS_CAP:
        NP += 4
    return NP


def fac_tile_waves(N, nslots, check, n_functions=F):
    """nep_fac.hip fac_tile_waves: waves per fac_x_pass workgroup."""
    tw = 4
    while tw < 16 and nslots * n_functions * tw < 4096:
        tw *= 2
    if cpl_of(N) >= 4 and tw > 8:
        tw = 8
    while tw > 4 and fac_lds_bytes(tw, padded(N), check) > LDS_CAP:
        tw //= 2
    return tw


def fac_variants(N, nslots, n_functions=F):
    """(CPL, TW, pass kind) of the fac_x_pass launches of a cold LP batch of `nslots` slots."""
    return {(cpl_of(N), fac_tile_waves(N, nslots, kind == "CHECK", n_functions), kind) for kind in KINDS}


def fac_dispatchable(function_counts=(F, FAC_WIDE_F)):
    """Every (CPL, TW, pass kind) the launchers can dispatch for these function counts at some admitted N and slot
    count."""
    out = set()
    for nf in function_counts:
        for N in range(1, fac_max_nodes() + 1):
            for ns in (1, 2, 7, 8, 15, 16, 64, 127, 128, 255, 256, 1024):
                out |= fac_variants(N, ns, nf)
    return out


def fac_matrix():
    """(N, F, iterating slots, box of a lone slot or None: slots alternate root / leaf) of every engine run of
    test_gpu_fac_iterates.py."""
    runs = []
    for N in EXTRA_CHUNK:
        for ns in SLOT_COUNTS:
            runs += [(N, F, ns, box) for box in ((0, 1) if ns == 1 else (None,))]
    runs += [(N, F, 256, None) for N in (254, 510, 1022, fac_max_nodes() - 2, fac_max_nodes())]
    runs += [(26, FAC_WIDE_F, 2, None)]
    return runs


def fac_instance(N, n_functions=F, seed=0):
    """Data of the N-node facility instance: the recipe of instance() (integer delays and workloads, core_per_req =
    k / 1024: float32 holds the data exactly), but function 0 loads min(37, N - 1) sources plus one pooled row — 38
    rows from N = 38 on: more than two passes of a 16-wave tile, and no multiple of 4 — and every other function 8
    sources plus the pooled row: 9 rows, so some waves of a 16-wave tile get none.  R stays near 65 at F = 4.  Leaf
    nodes (leaf_nodes) have the memory for every function at once."""
    from core.utils.data import Data
    nf = n_functions
    rng = np.random.default_rng(7000 * N + 13 * nf + seed)
    D = rng.integers(1, 100, size=(N, N))
    np.fill_diagonal(D, 0)
    free = np.setdiff1d(np.arange(N), leaf_nodes(N))
    W = np.zeros((nf, N), np.int64)
    src0 = np.r_[np.sort(rng.choice(N - 1, size=min(37, N - 1) - 1, replace=False)), N - 1]
    W[0, src0] = rng.integers(1, 9, size=src0.size)
    W[0, N - 1] = 8
    loaded = {}
    for f in range(1, nf):
        loaded[f] = np.sort(rng.choice(free, size=min(8, free.size), replace=False))
        W[f, loaded[f]] = rng.integers(1, 51, size=loaded[f].size)
    cpr = rng.integers(10, 103, size=(nf, N)) / 1024.0
    cpr[0, N - 1] = 64 / 1024.0
    cores = rng.integers(8, 65, size=N) / 64.0
    node_mem = rng.integers(64, 257, size=N).astype(float)
    fn_mem = rng.integers(4, 33, size=nf).astype(float)
    # lambda moves only where a row's reflected flow passes c: in the leaf box (c = 1) where a row sends everything to
    # one destination.  Function 0's own open node of every chunk index is 100 away from every source but one, which
    # has it at delay 0, every other node at 99 and workload 50, and so routes there alone within the first block —
    # in every 256-destination chunk index, the last included
    special = [int(i) for i in src0 if i in free]                # (sources no leaf box opens as destinations)
    for q, j in enumerate(chunk_nodes(N, 0)):
        D[:, j] = 100
        D[special[q], :] = 99
        D[special[q], special[q]] = D[special[q], j] = 0
        W[0, special[q]] = 50
    for q, j in enumerate(chunk_nodes(N, 1)):
        D[loaded[1][q], j] = 0
        W[1, loaded[1][q]] = 50
        cores[j] = 1.0 / 16
    cores[N - 1] = 1.0 / 64
    load = float((W * cpr.max(axis=1, keepdims=True)).sum())
    for j in (0, 8, 9):
        cores[j] = float(2 ** np.ceil(np.log2(load)))
    node_mem[leaf_nodes(N)] = max(256.0, float(2 ** np.ceil(np.log2(fn_mem.sum()))))
    node_mem[N - 1] = fn_mem.sum()       # the last node holds every function with no memory to spare: whenever the c
                                         # there run ahead of n, C3 is violated and y3 moves (the last chunk index)
    d = Data([f"node_{i}" for i in range(N)], [f"ns/fn_{f}" for f in range(nf)])
    d.node_memory_matrix = node_mem
    d.function_memory_matrix = fn_mem
    d.node_delay_matrix = D
    d.workload_matrix = W
    d.cores_matrix = cpr
    d.core_per_req_matrix = cpr
    d.max_delay_matrix = np.full(nf, 1000)
    d.response_time_matrix = np.zeros((nf, N), np.int64)
    d.node_cores_matrix = cores
    d.old_allocations_matrix = np.ones((nf, N), np.int64)
    d.node_costs = np.full(N, 5)
    d.node_budget = 300
    return d
