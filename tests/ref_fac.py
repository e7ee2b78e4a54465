"""Test-only numpy fp64 mirror of the facility relaxation's PDHG iteration (engine NEP_RELAX_FACILITY: fac_x_pass /
fac_node_pass in neptune-mip_amd/csrc/nep_fac.hip, scalar_pass in nep_kernels.hip), written from the model's definition
(include/neptune_lp.h, DESIGN.md §7, the header of nep_fac.hip).  Never used by the product path.

Model.  Routing rows x[r, :] on their simplexes (rows, weights and costs as ref_pdhg.RefModel builds them), small
primal z = (c [F, N], n [N]) on a box, and the dualised rows, all "<= 0":
    C3   sum_f mem_f c[f, j] - Mem_j n[j]                     dual y3[j]
    C5   sum_r w_r cpr[f_r, j] x[r, j] - cores_j n[j]          dual y5[j]
    Q    c[f, j] - n[j]                                        dual mu[f, j]
    L    x[r, j] - c[f_r, j]    (one per routing entry)        dual lambda[r, j]
y = (y3, y5, mu) is the engine's dual vector (nep_debug_state), lambda lives beside it (nep_debug_fac_state).  K and
K^T are the explicit functions K / KT below.  The scaling is an input, not re-derived: rho, gam and rownorm come from
nep_debug_build(relaxation = facility), rho_l (the row scale of L, one per (f, j)) from nep_debug_fac_state; any
positive scaling gives a valid bound, and without a device rho_l defaults to one Pock-Chambolle step from 1.
"""
import numpy as np

from ref_pdhg import INF, RefModel, _f32, proj_simplex_rows_sorted

F4 = np.float32


class RefFac:
    def __init__(self, data, variant, alpha=0.5, rho=None, gam=None, rownorm=None, rho_l=None):
        b = RefModel(data, variant, step=1, alpha=alpha)      # rows, weights, costs, natural bounds
        assert b.has_n, "the facility relaxation is a MinUtilization / MinDelayAndUtilization model"
        self.base = b
        N, F, R = b.N, b.F, b.R
        self.N, self.F, self.R = N, F, R
        FN = F * N
        self.row_f, self.row_src = b.row_f, b.row_src
        self.starts = np.flatnonzero(np.r_[True, b.row_f[1:] != b.row_f[:-1]])
        assert (b.row_f[self.starts] == np.arange(F)).all()   # every function has rows, in order
        self.w = b.row_w[:, None]
        self.cprR = b.cpr32[b.row_f]                          # [R, N] CPU per request of the row's function
        self.cpr = b.cpr32
        self.Dr = np.where(b.row_src[:, None] >= 0, b.D32[np.maximum(b.row_src, 0)], 0.0)
        self.wobj = b.row_wobj[:, None]
        self.cost_x = self.wobj * self.Dr
        self.mem_f = b.mem_f
        self.Mem = np.asarray(data.node_memory_matrix, float).reshape(N)
        self.cores = np.asarray(data.node_cores_matrix, float).reshape(N)
        self.oc, self.on, self.n_int = 0, FN, FN + N
        self.o3, self.o5, self.oQ, self.n_dual = 0, N, 2 * N, 2 * N + FN
        self.cost_int = b.cost_int.copy()
        assert self.cost_int.shape == (self.n_int,)
        self.nat_lb, self.nat_ub = b.nat_lb.copy(), b.nat_ub.copy()
        self.rho = np.ones(self.n_dual) if rho is None else np.asarray(rho, float)
        self.gam = np.ones(self.n_int) if gam is None else np.asarray(gam, float)
        self.rownorm = np.ones(self.n_dual) if rownorm is None else np.asarray(rownorm, float)
        assert self.rho.shape == (self.n_dual,) and self.gam.shape == (self.n_int,)
        if rho_l is None:
            rho_l = 1.0 / np.sqrt(1.0 + self.gam[:FN].reshape(F, N))
        self.rho_l = np.asarray(rho_l, float).reshape(F, N)
        self._eta = None
        # initial primal weight ||cost~|| / ||b~|| as nep_model_build.cpp build (C3 / C5 count their capacities)
        cn2 = (b.row_m[:, None] * self.cost_x ** 2).sum() + ((self.gam * self.cost_int) ** 2).sum()
        bn2 = ((self.rho[:N] * self.Mem) ** 2).sum() + ((self.rho[N:2 * N] * self.cores) ** 2).sum()
        self.omega0 = float(np.sqrt(cn2 / bn2)) if cn2 > 0 and bn2 > 0 else 1.0

    def colsum(self, A):
        """[F, N]: the rows A[r] of each function added up (a function's rows are consecutive)."""
        return np.add.reduceat(A, self.starts, axis=0)

    def colmax(self, A):
        return np.maximum.reduceat(A, self.starts, axis=0)

    # K (x, z) and K^T (y, lambda), unscaled
    def K(self, x, z):
        N, F = self.N, self.F
        c, n = z[:F * N].reshape(F, N), z[F * N:]
        y = np.empty(self.n_dual)
        y[:N] = (self.mem_f[:, None] * c).sum(axis=0) - self.Mem * n
        y[N:2 * N] = (self.w * self.cprR * x).sum(axis=0) - self.cores * n
        y[2 * N:] = (c - n[None, :]).ravel()
        return y, x - c[self.row_f]

    def KT(self, y, lam):
        N, F = self.N, self.F
        y3, y5, mu = y[:N], y[N:2 * N], y[2 * N:].reshape(F, N)
        gx = self.w * self.cprR * y5[None, :] + lam
        gz = np.empty(self.n_int)
        gz[:F * N] = (self.mem_f[:, None] * y3[None, :] + mu - self.colsum(lam)).ravel()
        gz[F * N:] = -self.Mem * y3 - self.cores * y5 - mu.sum(axis=0)
        return gx, gz

    @property
    def eta(self):
        """0.95 / ||K~|| of the scaled operator, by power iteration (used where no engine step size is given)."""
        if self._eta is None:
            rng = np.random.default_rng(1)
            x, z = rng.standard_normal((self.R, self.N)), rng.standard_normal(self.n_int)
            rl = self.rho_l[self.row_f]
            s = 0.0
            for _ in range(200):
                nrm = np.sqrt((x * x).sum() + (z * z).sum())
                x, z = x / nrm, z / nrm
                y, l = self.K(x, self.gam * z)
                gx, gz = self.KT(self.rho ** 2 * y, rl ** 2 * l)
                gz = gz * self.gam
                s = (x * gx).sum() + (z * gz).sum()
                x, z = gx, gz
            self._eta = 0.95 / np.sqrt(max(s, 1e-30))
        return self._eta

    def presolve(self, lbi=None, ubi=None):
        lb = self.nat_lb.copy() if lbi is None else np.maximum(self.nat_lb, lbi)
        ub = self.nat_ub.copy() if ubi is None else np.minimum(self.nat_ub, ubi)
        F, N = self.F, self.N
        c_ub = ub[:F * N].reshape(F, N)
        c_ub[:, ub[F * N:] <= 0] = np.minimum(c_ub[:, ub[F * N:] <= 0], 0.0)     # a closed node closes its c
        ok = not np.any(lb > ub + 1e-12) and bool((c_ub > 0).any(axis=1).all())
        return ok, lb, ub


def wave_sum_f32(A):
    """Row sums of a float32 [R, N] array in fac_x_pass's order: lane l of the row's wave holds the 16-byte chunks
    l, l + 64, ... (4 CPL elements) and adds them one by one, then the 64 lane sums meet in wave_sum_u's binary tree
    (neighbours, quads, the quads of a 16-lane row, the four rows).  Entries a sum leaves out are passed as +0."""
    R, N = A.shape
    chunks = (N + 3) // 4
    cpl = 1 if chunks <= 64 else 2 if chunks <= 128 else 4 if chunks <= 256 else 8
    B = np.zeros((R, 256 * cpl), F4)
    B[:, :N] = A
    B = B.reshape(R, cpl, 64, 4).transpose(0, 2, 1, 3).reshape(R, 64, 4 * cpl)
    s = np.zeros((R, 64), F4)
    for e in range(4 * cpl):
        s = s + B[:, :, e]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def certificate(m, lb, ub, xn, U):
    """The engine's certificate point (fac_x_pass / fac_node_pass CHECK): x̂ with the least c every row allows within
    the box, c = max(lb, max_r x̂[r, j]), and the least n the repaired c, its memory and x̂'s CPU allow; its objective
    and its largest violation (box excess absolute, C3 / C5 over rownorm).  U [N]: the CPU sums of x̂."""
    F, N = m.F, m.N
    lbc, ubc = lb[:F * N].reshape(F, N), ub[:F * N].reshape(F, N)
    lbn, ubn = lb[F * N:], ub[F * N:]
    cr = np.maximum(lbc, np.maximum(m.colmax(xn), 0.0))
    res = max(0.0, float((cr - ubc).max()))
    memr = (m.mem_f[:, None] * cr).sum(axis=0)
    nr = np.maximum(lbn, np.maximum(cr.max(axis=0), 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        nr = np.where(m.Mem > 0, np.maximum(nr, memr / m.Mem), nr)
        nr = np.where(m.cores > 0, np.maximum(nr, U / m.cores), nr)
    res = max(res, float((nr - ubn).max()))
    nr = np.minimum(nr, ubn)
    res = max(res, float((np.maximum(memr - m.Mem * nr, 0.0) / m.rownorm[:N]).max()),
              float((np.maximum(U - m.cores * nr, 0.0) / m.rownorm[N:2 * N]).max()))
    cc = m.cost_int[:F * N].reshape(F, N)
    pobj = float((m.cost_x * xn).sum() + (cc * cr).sum() + (m.cost_int[F * N:] * nr).sum())
    return dict(c=cr, n=nr, pobj=pobj, res=res)


def blocks(m, lbi=None, ubi=None, tol=1e-7, max_iters=100000, check_every=64, box=None, eta=None, omega0=None,
           rs_nec=0.9, fp32=False, engine=False, gap_tol=None):
    """The facility iteration in blocks of `check_every`, as ref_pdhg.blocks: iteration 0 of a block is the certificate
    iteration (a plain PDHG step), restarts take effect at iteration 1, the last iteration is plain, the others are
    reflected Halpern steps w' = lam (2 T(w) - w) + (1 - lam) w_anchor; the same restart test and weight update.
    One PDHG step T: c and n step on the previous duals (c's column uses lsum, the per-function sums of lambda the
    previous step left), x likewise; the duals step on the reflected point — lambda on (2x̂ - x) - (2ĉ - c), mu on
    (2ĉ - c) - (2n̂ - n), y3 / y5 on 2 K(ŵ) - kz with the tracked activity kz of the iterate (the same operator).
    A generator: one record per certificate iteration, right after it — k, status (None while the LP iterates), the
    iterate x, lam, lsum, z, y (and xn, the step's x̂); rc (the reduced costs of c and n the Lagrangian was priced with), lag (that
    Lagrangian), best / rc_best (the largest Lagrangian so far, strictly, and its reduced costs: what scalar_pass
    keeps in rc_lagr / rc_best and nep_lp_get_reduced_costs reports), pobj / res (the certificate point's), and the
    restart test's operands fpr, last_fpr, prev_fpr, k_since, dz, dy, restart, omega.  engine=True adds cert =
    certificate(...) (the repaired c and n) with lagr.
    box = (lb, ub): the engine's node box (nep_debug_state) instead of presolve(lbi, ubi); eta / omega0: the
    engine's step size and initial weight.
    fp32=True rounds to float32 what the kernels hold in float32 — x, its anchor and x̂; lambda, its anchor and
    lsum; tau and the Halpern weight in the x and lambda updates; cpr y5 (from the float y5 of kty), 2ĉ - c and
    sigma rho_l^2 as fac_x_pass stages them in LDS; the shifted point x - tau (wobj D - (w cpr y5 + lambda)) and
    lambda's step term by term in float32 arithmetic; the simplex threshold (sum - 1) / count with its sum added in
    float32 in the wave's order (wave_sum_f32); and, outside certificate iterations,
    the per-function CPU sums (float accumulators, times cpr in float).  Everything else stays fp64 as on the
    device."""
    F, N, R = m.F, m.N, m.R
    FN = F * N
    if box is None:
        ok, lb, ub = m.presolve(lbi, ubi)
    else:
        lb, ub = np.array(box[0], float), np.array(box[1], float)
        ok = not np.any(lb > ub + 1e-12) and bool((ub[:FN].reshape(F, N) > 0).any(axis=1).all())
    if not ok:
        yield dict(status=2, obj=INF, pobj=np.nan, iters=0, k=0)
        return
    gap_tol = tol if gap_tol is None else gap_tol
    lbc, ubc, lbn, ubn = lb[:FN].reshape(F, N), ub[:FN].reshape(F, N), lb[FN:], ub[FN:]
    mask = (ubc > 0)[m.row_f]
    ce = check_every
    rf = m.row_f
    cost_c, cost_n = m.cost_int[:FN].reshape(F, N), m.cost_int[FN:]
    gc2, gn2 = m.gam[:FN].reshape(F, N) ** 2, m.gam[FN:] ** 2
    gc, gn = m.gam[:FN].reshape(F, N), m.gam[FN:]
    r3, r5, rQ = m.rho[:N], m.rho[N:2 * N], m.rho[2 * N:].reshape(F, N)
    rl = m.rho_l
    w4, wobj4, Dr4, cpr4 = m.w.astype(F4), m.wobj.astype(F4), m.Dr.astype(F4), m.cpr.astype(F4)

    def cpu(xn, exact):
        Ux = m.colsum(m.w * xn)
        return (_f32(_f32(Ux) * m.cpr) if fp32 and not exact else Ux * m.cpr).sum(axis=0)

    x = proj_simplex_rows_sorted(np.zeros((R, N)), mask)
    if fp32:
        x = _f32(x)
    c, n = np.clip(np.zeros((F, N)), lbc, ubc), np.clip(np.zeros(N), lbn, ubn)
    lam, lsum = np.zeros((R, N)), np.zeros((F, N))
    y3, y5, mu = np.zeros(N), np.zeros(N), np.zeros((F, N))
    kz3 = (m.mem_f[:, None] * c).sum(axis=0) - m.Mem * n
    kz5 = cpu(x, False) - m.cores * n
    anchor = None
    omega, eta = (m.omega0 if omega0 is None else float(omega0)), (m.eta if eta is None else float(eta))
    om_lo, om_hi = omega * 1e-5, omega * 1e5
    k = k_since = 0
    ks_base = -ce
    restart_pending = True                     # (INIT sets every anchor)
    last_fpr, prev_fpr = -1.0, INF
    best, rc_best = -INF, None
    block = 0
    while True:
        for it in range(ce):
            check, first = it == 0, it == 1
            plain = ce < 4 or it == 0 or it == ce - 1
            if anchor is None or (first and restart_pending):
                anchor = (x.copy(), c.copy(), n.copy(), lam.copy(), y3.copy(), y5.copy(), mu.copy(), kz3.copy(),
                          kz5.copy())
            xa, ca, na, lama, y3a, y5a, mua, kz3a, kz5a = anchor
            tau, sig = eta / omega, eta * omega
            # c and n: the previous duals
            rc_c = cost_c - (m.mem_f[:, None] * y3[None, :] - lsum + mu)
            rc_n = cost_n + mu.sum(axis=0) + m.Mem * y3 + m.cores * y5
            ch = np.clip(c - tau * gc2 * rc_c, lbc, ubc)
            nh = np.clip(n - tau * gn2 * rc_n, lbn, ubn)
            refl_c = 2.0 * ch - c
            s_l = sig * rl * rl
            # x, then lambda on the reflected x and c
            if fp32:
                cy5 = cpr4 * y5.astype(F4)[None, :]
                x4, lam4 = x.astype(F4), lam.astype(F4)
                g = wobj4 * Dr4 - (w4 * cy5[rf] + lam4)
                vv4 = x4 - F4(tau) * g
                # the threshold as the kernel's Michelot iteration ends it: (sum - 1) / count over the support, the sum
                # a float32 one in the wave's order
                _, theta = proj_simplex_rows_sorted(vv4.astype(np.float64), mask, return_theta=True)
                supp = mask & (vv4.astype(np.float64) > theta[:, None])
                cnt = supp.sum(axis=1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    th4 = np.where(cnt > 0, (wave_sum_f32(np.where(supp, vv4, F4(0))) - F4(1)) /
                                   np.maximum(cnt, 1).astype(F4), F4(np.inf)).astype(F4)
                    xn4 = np.where(mask, np.maximum(vv4 - th4[:, None], F4(0)), F4(0)).astype(F4)
                d4 = (F4(2) * xn4 - x4) - refl_c.astype(F4)[rf]
                lh4 = np.minimum(F4(0), lam4 - s_l.astype(F4)[rf] * d4)
                xn, lh = xn4.astype(np.float64), lh4.astype(np.float64)
            else:
                xn = proj_simplex_rows_sorted(x - tau * (m.cost_x - (m.w * m.cprR * y5[None, :] + lam)), mask)
                lh = np.minimum(0.0, lam - s_l[rf] * ((2.0 * xn - x) - refl_c[rf]))
            # node rows and c <= n
            U = cpu(xn, check)
            act3 = (m.mem_f[:, None] * ch).sum(axis=0) - m.Mem * nh
            act5 = U - m.cores * nh
            y3h = np.minimum(0.0, y3 - sig * r3 * r3 * (2.0 * act3 - kz3))
            y5h = np.minimum(0.0, y5 - sig * r5 * r5 * (2.0 * act5 - kz5))
            muh = np.minimum(0.0, mu - sig * rQ * rQ * (refl_c - (2.0 * nh - n)[None, :]))
            if check:
                rcx = m.cost_x - (m.w * m.cprR * y5[None, :] + lam)
                lag = float(np.where(mask, rcx, INF).min(axis=1).sum() +
                            np.where(rc_c > 0, lbc * rc_c, ubc * rc_c).sum() +
                            np.where(rc_n > 0, lbn * rc_n, ubn * rc_n).sum())
                cert = certificate(m, lb, ub, xn, U)
                cert["lagr"] = lag
                pobj, res = cert["pobj"], cert["res"]
                mvz = ((xn - x) ** 2).sum() + (((ch - c) / gc) ** 2).sum() + (((nh - n) / gn) ** 2).sum()
                mvy = ((((y3h - y3) / r3) ** 2).sum() + (((y5h - y5) / r5) ** 2).sum() +
                       (((muh - mu) / rQ) ** 2).sum() + (((lh - lam) / rl[rf]) ** 2).sum())
                dsz = ((xn - xa) ** 2).sum() + (((ch - ca) / gc) ** 2).sum() + (((nh - na) / gn) ** 2).sum()
                dsy = ((((y3h - y3a) / r3) ** 2).sum() + (((y5h - y5a) / r5) ** 2).sum() +
                       (((muh - mua) / rQ) ** 2).sum() + (((lh - lama) / rl[rf]) ** 2).sum())
                rcz = np.r_[rc_c.ravel(), rc_n]
            if plain:
                x, lam, c, n, y3, y5, mu, kz3, kz5 = xn, lh, ch, nh, y3h, y5h, muh, act3, act5
            else:
                ks = ks_base + it
                hl = (ks + 1.0) / (ks + 2.0)
                if fp32:
                    l4 = F4(hl)
                    x = (l4 * (F4(2) * xn4 - x4) + (F4(1) - l4) * xa.astype(F4)).astype(np.float64)
                    lam = (l4 * (F4(2) * lh4 - lam4) + (F4(1) - l4) * lama.astype(F4)).astype(np.float64)
                else:
                    x = hl * (2.0 * xn - x) + (1.0 - hl) * xa
                    lam = hl * (2.0 * lh - lam) + (1.0 - hl) * lama
                c = hl * (2.0 * ch - c) + (1.0 - hl) * ca
                n = hl * (2.0 * nh - n) + (1.0 - hl) * na
                y3 = hl * (2.0 * y3h - y3) + (1.0 - hl) * y3a
                y5 = hl * (2.0 * y5h - y5) + (1.0 - hl) * y5a
                mu = hl * (2.0 * muh - mu) + (1.0 - hl) * mua
                kz3 = hl * (2.0 * act3 - kz3) + (1.0 - hl) * kz3a
                kz5 = hl * (2.0 * act5 - kz5) + (1.0 - hl) * kz5a
            lsum = m.colsum(lam)
            if fp32:
                lsum = _f32(lsum)
            if not check:
                continue
            k += 1 if block == 0 else ce
            k_since += 1 if block == 0 else ce
            restart_pending = False
            if lag > best:
                best, rc_best = lag, rcz
            fpr = float(np.sqrt(omega * mvz + mvy / omega))
            if last_fpr < 0:
                last_fpr = fpr
            restart = bool(fpr <= 0.2 * last_fpr or (fpr <= rs_nec * last_fpr and fpr > prev_fpr)
                           or k_since >= 0.36 * k)
            dz, dy = float(np.sqrt(dsz)), float(np.sqrt(dsy))
            rec = dict(status=None, k=k, iters=k, obj=best, lag=lag, best=best, rc=rcz, rc_best=rc_best, pobj=pobj,
                       res=res, x=x, xn=xn, lam=lam, lsum=lsum, z=np.r_[c.ravel(), n], y=np.r_[y3, y5, mu.ravel()],
                       omega=omega, fpr=fpr, last_fpr=last_fpr, prev_fpr=prev_fpr, k_since=k_since, restart=restart,
                       dz=dz, dy=dy, mvz=mvz, mvy=mvy, cert=cert if engine else None)
            if np.isfinite(best) and res <= tol and pobj - best <= gap_tol * max(1.0, abs(best)):
                yield dict(rec, status=0)
                return
            if k >= max_iters:
                yield dict(rec, status=1)
                return
            yield rec
            prev_fpr = fpr
            if restart:
                if dz > 1e-10 and dy > 1e-10:
                    omega = float(np.clip(np.exp(0.5 * np.log(dy / dz) + 0.5 * np.log(omega)), om_lo, om_hi))
                restart_pending = True
                k_since = 0
                ks_base = -1
                last_fpr = fpr
                prev_fpr = INF
            else:
                ks_base += ce
        block += 1


def restart_rule(fpr, last, prev, k_since, k, nec=0.9):
    return bool(fpr <= 0.2 * last or (fpr <= nec * last and fpr > prev) or k_since >= 0.36 * k)


def matrix_preconditions(m, recs_by_box, snapshots, tag=""):
    """What the short cold runs of test_gpu_fac_iterates.py must exercise, asserted from the fp64 mirror's records
    alone ({box: records} of one shape's root and leaf box):
      * every run stops at the last snapshot by its iteration limit, with one record per snapshot;
      * FIRST passes occur with and without a restart, in each box;
      * no restart decision flips when fpr, last_fpr and prev_fpr move by a relative 1e-3 either way, the artificial
        restart's counter is not within 1e-3 of its threshold, and dz, dy are not within 1e-3 of the 1e-10 the
        weight update tests;
      * lambda, mu (c <= n) and y5 are each nonzero, over the snapshots of each box, at a destination of every
        256-destination chunk index the width has, the last one included; y3 likewise over the snapshots of the two
        boxes together (a root LP's memory rows are violated only while c runs ahead of n, in its first dozen
        iterations: between the snapshots; the leaf box holds c = 1 against an n that starts at 0);
      * the anchors set at the restarts (the iterate of a certificate that decides a restart) have rows of support 1,
        of 2..16 and of > 16, over the two boxes (the sparse / dense anchor switch at kAnchorK = 16);
      * over the two boxes, the best bound is replaced at least once after the first certificate and is kept at
        least once (both directions of the rc_cur / rc_best double buffer)."""
    N, F = m.N, m.F
    nq = ((N + 3) // 4 * 4 + 255) // 256
    sup_classes, improved, kept, y3_hit = set(), 0, 0, set()
    for box, recs in recs_by_box.items():
        assert [r["k"] for r in recs] == list(snapshots) and recs[-1]["status"] == 1, (tag, box)
        assert {r["restart"] for r in recs[:-1]} == {True, False}, (tag, box, [r["restart"] for r in recs])
        hit = {name: set() for name in ("lam", "mu", "y3", "y5")}
        for i, r in enumerate(recs):
            if i < len(recs) - 1:
                for s in (-1e-3, 1e-3):
                    for t in (-1e-3, 1e-3):
                        for u in (-1e-3, 1e-3):
                            assert restart_rule(r["fpr"] * (1 + s), r["last_fpr"] * (1 + t), r["prev_fpr"] * (1 + u),
                                                r["k_since"], r["k"]) == r["restart"], (tag, box, r["k"])
                assert abs(r["k_since"] - 0.36 * r["k"]) > 1e-3 * 0.36 * r["k"], (tag, box, r["k"])
                for v in (r["dz"], r["dy"]):
                    assert abs(v - 1e-10) > 1e-3 * 1e-10, (tag, box, r["k"])
                if r["restart"]:
                    sup = (r["x"] > 0).sum(axis=1)
                    sup_classes |= {c for c, h in (("1", (sup == 1).any()), ("2-16", ((sup > 1) & (sup <= 16)).any()),
                                                   (">16", (sup > 16).any())) if h}
            y = r["y"]
            for name, a in (("lam", r["lam"]), ("mu", y[2 * N:].reshape(F, N)), ("y3", y[:N][None, :]),
                            ("y5", y[N:2 * N][None, :])):
                hit[name] |= set((np.nonzero(a.any(axis=0))[0] >> 8).tolist())
            if i > 0:
                improved += r["best"] > recs[i - 1]["best"]
                kept += r["best"] == recs[i - 1]["best"]
        y3_hit |= hit.pop("y3")
        for name, q in hit.items():
            assert q == set(range(nq)), (tag, box, name, sorted(q))
    assert y3_hit == set(range(nq)), (tag, "y3", sorted(y3_hit))
    assert sup_classes == {"1", "2-16", ">16"}, (tag, sup_classes)
    assert improved >= 1 and kept >= 1, (tag, improved, kept)


def solve(m, lbi=None, ubi=None, **kw):
    """blocks() run to its end; returns (last record, every certificate's [k, lag, pobj, res])."""
    trail = []
    rec = None
    for rec in blocks(m, lbi, ubi, **kw):
        if rec.get("k"):
            trail.append((rec["k"], rec["lag"], rec["pobj"], rec["res"]))
    return rec, trail
