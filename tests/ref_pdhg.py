"""Test-only numpy mirror of the MI355X LP engine (neptune-mip_amd/csrc): same structured model
(zero-workload aggregation, coefficients, Ruiz + Pock-Chambolle scaling, power-iteration step) and
the same preconditioned PDHG iteration, restarts and certificate.  Used to (a) check the C++ model
build through nep_debug_build on CPU, (b) debug the algorithm without a GPU, (c) compare kernel
iterates.  Never used by the product path.
"""
import numpy as np

INF = np.inf


class RefModel:
    def __init__(self, data, variant, step=1, alpha=0.5, soften_step1_sol=1.3, max_score=0.0,
                 prev_network_delay=0.0, M=1e6, eps=1e-6, dred=None):
        D = np.asarray(data.node_delay_matrix, float)
        W = np.asarray(data.workload_matrix, float)
        F, N = W.shape
        cpr = np.asarray(data.core_per_req_matrix, float)
        cpr = np.where(np.isfinite(cpr), cpr, np.finfo(np.float32).max)
        self.N, self.F, self.M, self.eps = N, F, M, eps
        self.variant = {"MinDelay": 0, "MinUtilization": 1, "MinDelayAndUtilization": 2}.get(variant, variant)
        self.step2 = step != 1
        self.has_n = self.variant != 0
        self.sigma4 = 1.0 if step == 3 else -1.0
        rows = []
        for f in range(F):
            zeros = 0
            for i in range(N):
                if W[f, i] != 0:
                    rows.append((f, i, 1.0, W[f, i]))
                else:
                    zeros += 1
            if zeros:
                rows.append((f, -1, float(zeros), 0.0))
        self.R = len(rows)
        self.row_f = np.array([r[0] for r in rows])
        self.row_src = np.array([r[1] for r in rows])
        self.row_m = np.array([r[2] for r in rows], np.float32).astype(float)
        self.row_w = np.array([r[3] for r in rows], np.float32).astype(float)
        kobj = 0.0
        if not self.step2:
            if self.variant == 0:
                kobj = 1.0
            elif self.variant == 2 and W.sum() != 0:
                md = np.asarray(data.max_delay_matrix, float)
                mwd = 0.0
                for f in range(F):
                    for i in range(N):
                        mwd += W[f, i] * max(d for d in D[i] if d <= md[f])
                kobj = (1 - alpha) / mwd
            self.cost_n = {1: 1.0, 2: alpha / N}.get(self.variant, 0.0)
        else:
            self.cost_n = 0.0
        self.row_wobj = (kobj * self.row_w).astype(np.float32).astype(float)
        colmaxD = D.max(axis=0)
        wsc = np.zeros(self.R)
        self.score_n_coef = 0.0
        score_rhs = INF
        if self.step2:
            md = np.asarray(data.max_delay_matrix, float)
            for r in range(self.R):
                if self.row_src[r] >= 0:
                    if self.variant == 0:
                        wsc[r] = self.row_w[r]
                    elif self.variant == 2:
                        wsc[r] = (1 - alpha) * self.row_w[r] / max(md[self.row_f[r]], colmaxD[self.row_src[r]])
            if self.variant == 0:
                score_rhs = soften_step1_sol * prev_network_delay
            else:
                score_rhs = max_score * soften_step1_sol
                self.score_n_coef = 1.0 if self.variant == 1 else alpha / N
        self.row_wsc = wsc.astype(np.float32).astype(float)
        self.D32 = D.astype(np.float32).astype(float)
        self.cpr32 = cpr.astype(np.float32).astype(float)
        FN = F * N
        # int layout
        if not self.step2:
            self.oc, self.on = 0, (FN if self.has_n else -1)
            self.n_int = FN + (N if self.has_n else 0)
        else:
            self.oc, self.omf, self.omt, self.oa, self.od = 0, FN, 2 * FN, 3 * FN, 3 * FN + 1
            self.on = 3 * FN + 2 if self.has_n else -1
            self.n_int = 3 * FN + 2 + (N if self.has_n else 0)
        self.nat_lb = np.zeros(self.n_int)
        self.nat_ub = np.ones(self.n_int)
        self.cost_int = np.zeros(self.n_int)
        if self.has_n:
            cost = np.asarray(data.node_costs, float)
            for j in range(N):
                if cost[j] > 0:
                    self.nat_ub[self.on + j] = min(1.0, data.node_budget / cost[j])
                self.cost_int[self.on + j] = self.cost_n
        old = np.asarray(data.old_allocations_matrix, float).ravel()
        sum_old = old.sum()
        if self.step2:
            w = float(FN)
            self.cost_int[self.omf:self.omf + FN] = w
            self.cost_int[self.omt:self.omt + FN] = w
            self.cost_int[self.oa] = w - 1
            self.cost_int[self.od] = w + 1
            self.nat_lb[self.oa] = self.nat_lb[self.od] = -float(FN)
            self.nat_ub[self.oa] = self.nat_ub[self.od] = 0.0
        # dual layout
        o = 0
        self.o1 = o; o += FN
        self.o2 = o; o += FN
        self.o3 = o; o += N
        self.o5 = o; o += N
        if self.has_n:
            self.o6 = o; o += N
            self.o7 = o; o += N
        if self.step2:
            self.oD1 = o; o += FN
            self.oD2 = o; o += FN
            self.oD3a, self.oD3b, self.oD4, self.oS = o, o + 1, o + 2, o + 3
            o += 4
        self.n_dual = o
        lo = np.full(o, -INF)
        hi = np.full(o, INF)
        hi[self.o1:self.o1 + FN] = 0.0
        lo[self.o2:self.o2 + FN] = -eps
        hi[self.o3:self.o3 + N] = np.asarray(data.node_memory_matrix, float)
        hi[self.o5:self.o5 + N] = np.asarray(data.node_cores_matrix, float)
        if self.has_n:
            hi[self.o6:self.o6 + N] = 0.0
            lo[self.o7:self.o7 + N] = -eps
        if self.step2:
            lo[self.oD1:self.oD1 + FN] = -old
            lo[self.oD2:self.oD2 + FN] = old
            lo[self.oD3a] = -sum_old
            lo[self.oD3b] = sum_old
            lo[self.oD4] = self.sigma4 * sum_old
            hi[self.oS] = score_rhs
        self.lo, self.hi = lo, hi
        self.mem_f = np.asarray(data.function_memory_matrix, float)
        # COO of the non-x part
        r, c, v = [], [], []

        def add(a, b, val):
            r.append(a); c.append(b); v.append(val)
        for f in range(F):
            for j in range(N):
                k = f * N + j
                add(self.o1 + k, self.oc + k, -M)
                add(self.o2 + k, self.oc + k, -1.0)
                add(self.o3 + j, self.oc + k, self.mem_f[f])
                if self.has_n:
                    add(self.o6 + j, self.oc + k, 1.0)
                    add(self.o7 + j, self.oc + k, 1.0)
                if self.step2:
                    add(self.oD1 + k, self.omf + k, 1.0)
                    add(self.oD1 + k, self.oc + k, -1.0)
                    add(self.oD2 + k, self.omt + k, 1.0)
                    add(self.oD2 + k, self.oc + k, 1.0)
                    add(self.oD3a, self.oc + k, -1.0)
                    add(self.oD3b, self.oc + k, 1.0)
                    add(self.oD4, self.oc + k, self.sigma4)
        if self.has_n:
            for j in range(N):
                add(self.o6 + j, self.on + j, -M)
                add(self.o7 + j, self.on + j, -1.0)
                if self.step2 and self.score_n_coef != 0:
                    add(self.oS, self.on + j, self.score_n_coef)
        if self.step2:
            add(self.oD3a, self.oa, -1.0)
            add(self.oD3b, self.od, -1.0)
            add(self.oD4, self.od, 1.0)
            add(self.oD4, self.oa, 1.0)
        self.Kr, self.Kc, self.Kv = np.array(r), np.array(c), np.array(v)
        # x-row norms
        xmax = np.zeros(o)
        xsum = np.zeros(o)
        for f in range(F):
            sel = self.row_f == f
            mm, ms = (self.row_m[sel].max(), self.row_m[sel].sum()) if sel.any() else (0.0, 0.0)
            xmax[self.o1 + f * N:self.o1 + (f + 1) * N] = mm
            xmax[self.o2 + f * N:self.o2 + (f + 1) * N] = mm
            xsum[self.o1 + f * N:self.o1 + (f + 1) * N] = ms
            xsum[self.o2 + f * N:self.o2 + (f + 1) * N] = ms
        wc = self.row_w[:, None] * cpr[self.row_f]            # [R, N]
        xmax[self.o5:self.o5 + N] = np.abs(wc).max(axis=0)
        xsum[self.o5:self.o5 + N] = np.abs(wc).sum(axis=0)
        if self.step2:
            sc = self._score_coef(D)
            xmax[self.oS] = np.abs(sc).max() if sc.size else 0.0
            xsum[self.oS] = np.abs(sc).sum()
        self.wc = wc
        rn = np.maximum(1.0, xmax)
        rn = np.where(np.isfinite(lo), np.maximum(rn, np.abs(np.where(np.isfinite(lo), lo, 0))), rn)
        rn = np.where(np.isfinite(hi), np.maximum(rn, np.abs(np.where(np.isfinite(hi), hi, 0))), rn)
        np.maximum.at(rn, self.Kr, np.abs(self.Kv))
        self.rownorm = rn
        # step 2, reduced disruption block (nep_model_build.cpp build): mf / mt / a / d follow from c, the
        # iteration runs on K without D1/D2/D3a/D3b and with D4 as the row sum c (coefficient 1 on every c)
        self.old = old
        self.dred = bool(self.step2 and np.isin(old, (0.0, 1.0)).all()) if dred is None else bool(dred and self.step2)
        self.sT = 0.0
        if self.dred:
            self.sT = -(w - 1) if self.sigma4 > 0 else (w + 1)
            idle = np.zeros(o, bool)
            idle[self.oD1:self.oD1 + FN] = idle[self.oD2:self.oD2 + FN] = True
            idle[[self.oD3a, self.oD3b]] = True
            keep = ~idle[self.Kr]
            keep &= ~((self.Kr == self.oD4) & ((self.Kc < self.oc) | (self.Kc >= self.oc + FN)))
            self.Kr, self.Kc, self.Kv = self.Kr[keep], self.Kc[keep], self.Kv[keep]
            self.Kv = np.where(self.Kr == self.oD4, 1.0, self.Kv)
            lo[idle] = -INF
            hi[idle] = INF
        rho = np.ones(o)
        gam = np.ones(self.n_int)
        for sweep in range(11):
            pc = sweep == 10
            a = np.abs(rho[self.Kr] * self.Kv * gam[self.Kc])
            if pc:
                rnn = rho * xsum
                np.add.at(rnn, self.Kr, a)
                cn = np.zeros(self.n_int)
                np.add.at(cn, self.Kc, a)
            else:
                rnn = rho * xmax
                np.maximum.at(rnn, self.Kr, a)
                cn = np.zeros(self.n_int)
                np.maximum.at(cn, self.Kc, a)
            rho = np.where(rnn > 0, rho / np.sqrt(np.where(rnn > 0, rnn, 1)), rho)
            gam = np.where(cn > 0, gam / np.sqrt(np.where(cn > 0, cn, 1)), gam)
        self.rho, self.gam = rho, gam
        self.sigma_max = self._power()
        self.eta = 0.95 / self.sigma_max
        # initial primal weight ||c~|| / ||b~|| (scaled space), as nep_model_build.cpp build()
        cx = self.row_wobj[:, None] * np.where(self.row_src[:, None] >= 0, D[np.maximum(self.row_src, 0)], 0.0)
        # (reduced step 2: the reduced LP's costs and row bounds at natural bounds, as nep_model_build.cpp build)
        ci = self.cost_int
        if self.dred:
            ci, _, self.lo[self.oD4], self.hi[self.oD4] = self.dred_terms(self.nat_lb, self.nat_ub)
        cn2 = (self.row_m[:, None] * cx * cx).sum() + ((gam * ci) ** 2).sum()
        bmag = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
        bn2 = ((rho * bmag) ** 2).sum()
        self.omega0 = float(np.sqrt(cn2) / np.sqrt(bn2)) if cn2 > 0 and bn2 > 0 else 1.0

    def dred_terms(self, lb, ub):
        """Reduced step 2 at a box: the iteration's costs (c: its own linear cost, mf / mt / a / d: 0), the
        objective's constant and the row sum c's bounds [L, U] (nep_device.h dred_cost / dred_bounds)."""
        FN, w = self.F * self.N, float(self.F * self.N)
        lmf, lmt = lb[self.omf:self.omf + FN], lb[self.omt:self.omt + FN]
        old0 = self.old < 0.5
        cost = self.cost_int.copy()
        cost[self.omf:self.omt + FN] = 0.0
        cost[self.oa] = cost[self.od] = 0.0
        cost[self.oc:self.oc + FN] = np.where(old0, np.where(lmf < 0.5, w, 0.0), np.where(lmt < 0.5, -w, 0.0)) + self.sT
        const = float(np.where(old0, w * (lmf + lmt), w * (lmf + 1.0)).sum()) - self.sT * self.old.sum()
        la, ua, ld, ud = lb[self.oa], ub[self.oa], lb[self.od], ub[self.od]
        if self.sigma4 > 0:
            ok = ld <= 0 <= ud
            tlo, thi = (max(0.0, -ua), -la) if ok else (1.0, 0.0)
        else:
            ok = la <= 0 <= ua
            tlo, thi = (ld, min(0.0, ud)) if ok else (1.0, 0.0)
        so = self.old.sum()
        return cost, const, so + tlo, so + thi

    def _score_coef(self, D):
        out = np.zeros((self.R, self.N))
        for r in range(self.R):
            if self.row_src[r] >= 0 and self.row_wsc[r] != 0:
                out[r] = self.row_wsc[r] * D[self.row_src[r]]
        return out

    def colsum(self, A):
        """[F, N] sums of the rows A[r] of each function, added in row order (a function's rows are consecutive):
        what np.add.at(S, row_f, A) gives, bit for bit, without its per-element dispatch."""
        S = np.zeros((self.F, self.N))
        if self.R:
            starts = np.flatnonzero(np.r_[True, self.row_f[1:] != self.row_f[:-1]])
            for a, b in zip(starts, np.r_[starts[1:], self.R]):
                S[self.row_f[a]] = np.add.reduce(A[a:b], axis=0)
        return S

    def colsum32(self, A, tw=4):
        """colsum as x_pass accumulates it on plain iterations: wave w of `tw` adds rows w, w + tw, ... of the function
        in float32, one after the other, and the waves' sums are added in float32 in wave order (tw = 4: the tile of a
        full batch, the longest chains)."""
        f4 = np.float32
        S = np.zeros((self.F, self.N), f4)
        if self.R:
            A4 = A.astype(f4)
            starts = np.flatnonzero(np.r_[True, self.row_f[1:] != self.row_f[:-1]])
            for a, b in zip(starts, np.r_[starts[1:], self.R]):
                for w in range(tw):
                    if a + w < b:
                        S[self.row_f[a]] += np.add.reduce(A4[a + w:b:tw], axis=0, dtype=f4)
        return S.astype(np.float64)

    # K·[x, z] (unscaled) and Kᵀy (unscaled)
    def K(self, x, z):
        N, F = self.N, self.F
        y = np.zeros(self.n_dual)
        S = self.colsum(self.row_m[:, None] * x)
        y[self.o1:self.o1 + F * N] += S.ravel()
        y[self.o2:self.o2 + F * N] += S.ravel()
        y[self.o5:self.o5 + N] += (self.wc * x).sum(axis=0)
        if self.step2:
            y[self.oS] += (self._score_coef(self.D32) * x).sum()
        np.add.at(y, self.Kr, self.Kv * z[self.Kc])
        return y

    def KT(self, y):
        N, F = self.N, self.F
        y12 = (y[self.o1:self.o1 + F * N] + y[self.o2:self.o2 + F * N]).reshape(F, N)
        gx = self.row_m[:, None] * y12[self.row_f] + self.wc * y[self.o5:self.o5 + N][None, :]
        if self.step2:
            gx = gx + self._score_coef(self.D32) * y[self.oS]
        gz = np.zeros(self.n_int)
        np.add.at(gz, self.Kc, self.Kv * y[self.Kr])
        return gx, gz

    def _power(self, iters=60):
        rng = np.random.default_rng(1)
        x = rng.standard_normal((self.R, self.N))
        z = rng.standard_normal(self.n_int)
        lam = 0.0
        for _ in range(iters):
            nrm = np.sqrt((x * x).sum() + (z * z).sum())
            x, z = x / nrm, z / nrm
            y = self.rho * self.K(x, self.gam * z)
            gx, gz = self.KT(self.rho * y)
            gz = gz * self.gam
            lam = (x * gx).sum() + (z * gz).sum()
            x, z = gx, gz
        return np.sqrt(max(lam, 1e-30))

    def presolve(self, lbi=None, ubi=None):
        lb = self.nat_lb.copy() if lbi is None else np.maximum(self.nat_lb, lbi)
        ub = self.nat_ub.copy() if ubi is None else np.minimum(self.nat_ub, ubi)
        N, F = self.N, self.F
        if self.has_n:
            for j in range(N):
                if ub[self.on + j] <= 0:
                    for f in range(F):
                        ub[self.oc + f * N + j] = min(ub[self.oc + f * N + j], 0.0)
        ok = not np.any(lb > ub + 1e-12)
        mask = (ub[self.oc:self.oc + F * N] > 0).reshape(F, N)
        if not mask.any(axis=1).all():
            ok = False
        return ok, lb, ub, mask


def proj_simplex_rows(V, mask):
    out = np.zeros_like(V)
    for r in range(V.shape[0]):
        v = V[r][mask[r]]
        if v.size == 0:
            continue
        u = np.sort(v)[::-1]
        css = np.cumsum(u)
        k = np.arange(1, len(u) + 1)
        rho = np.nonzero(u - (css - 1) / k > 0)[0][-1]
        theta = (css[rho] - 1) / (rho + 1)
        out[r][mask[r]] = np.maximum(v - theta, 0)
    return out


def proj_simplex_rows_sorted(V, mask, return_theta=False):
    """proj_simplex_rows with every row sorted at once: the same sort, running sums (in the same order) and
    threshold per row, so the same values bit for bit (tests/test_abi.py) — the row loop costs ~0.1 ms a row."""
    Vm = np.where(mask, V, -INF)
    u = -np.sort(-Vm, axis=1)
    with np.errstate(invalid="ignore"):
        css = np.cumsum(u, axis=1)
        k = np.arange(1, V.shape[1] + 1)
        pos = u - (css - 1) / k > 0
    cnt = mask.sum(axis=1)
    rho = V.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1)
    theta = (css[np.arange(V.shape[0]), rho] - 1) / (rho + 1)
    out = np.where(mask, np.maximum(V - theta[:, None], 0), 0.0)
    out[cnt == 0] = 0.0
    return (out, np.where(cnt == 0, INF, theta)) if return_theta else out


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _theta32(V, mask, theta):
    """The simplex threshold (S - 1) / |S| of every row as x_pass forms it on plain iterations: the sum S over the
    support {v > theta} and the quotient in float32 arithmetic (numpy's order of additions, not the wave's: the same
    size of error).  The shifted point's entries reach ~10^2 (tau |g|), so S carries an absolute error of ~10^-5 that
    rounding the fp64 threshold to float32 once does not show."""
    f4 = np.float32
    sup = mask & (V > theta[:, None])
    cnt = sup.sum(axis=1)
    S = np.where(sup, V, 0.0).astype(f4).sum(axis=1, dtype=f4)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, ((S - f4(1.0)) / cnt.astype(f4)).astype(np.float64), theta)


def _row_lagr(y, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.where(y > 0, np.where(np.isfinite(lo), y * lo, -INF),
                        np.where(y < 0, np.where(np.isfinite(hi), y * hi, -INF), 0.0))


def _price_rc(b, s, M):
    return b + M * np.minimum(s, 0.0) + np.maximum(s, 0.0)


def _price_at(b, target, M):
    d = target - b
    return np.where(d < 0, d / M, d)


def _repair_box(b, s0, z, lb, ub, M, eps, K):
    """nep_device.h repair_box, elementwise: the re-priced big-M pair (s = y1 + y2, or t = y6 + y7) of a variable
    on [lb, ub] with reduced cost price_rc(b, s) and iterate z."""
    tol = 1e-7
    inner = (z > lb + tol) & (z < ub - tol)
    at0 = (z <= lb + tol) & (lb == 0.0)
    p0 = _price_at(b, 0.0, M)
    best = np.full(np.shape(b), -INF)
    sb = np.array(s0, float, copy=True)
    for s in (s0, np.zeros_like(b), p0, -b):
        rc = _price_rc(b, s, M)
        val = np.minimum(rc * lb, rc * ub) - eps * np.maximum(s, 0.0) - K * np.maximum(s - s0, 0.0)
        take = val > best
        best = np.where(take, val, best)
        sb = np.where(take, s, sb)
    return np.where(inner | at0, p0, sb)


def engine_certificate(m, lb, ub, fmask, y, z, xn, zn, cost_x, cost_int, const, lag_plain):
    """What the kernels' certificate iteration reports (nep_kernels.hip x_pass / node_pass / scalar_pass CHECK,
    DESIGN.md §4 "Certificate", "Dual repair"), in fp64, for step 1 and the reduced step-2 block: the objective
    and the largest violation at the REPAIRED point (c clamped onto [S / M, S + eps] and n onto [sum c / M,
    sum c + eps] within their boxes, moved / allocated / deallocated the cheapest completion), the better of
    the plain Lagrangian bound and the one at the repaired big-M prices, and the column deficits the pooled /
    loaded shift would serve (c_target - eps - S: the mirror has no shift, so a caller asserts there are none).
    y, z: the iterate the iteration starts from; xn, zn: its T output."""
    if m.step2 and not m.dred:
        raise NotImplementedError("engine_certificate: the full step-2 disruption block is not mirrored")
    N, F, M, eps = m.N, m.F, m.M, m.eps
    FN = F * N
    oc = m.oc
    S = m.colsum(m.row_m[:, None] * xn)
    U = (m.wc * xn).sum(axis=0)
    y1, y2 = y[m.o1:m.o1 + FN].reshape(F, N), y[m.o2:m.o2 + FN].reshape(F, N)
    y3, y5 = y[m.o3:m.o3 + N], y[m.o5:m.o5 + N]
    yS = y[m.oS] if m.step2 else 0.0
    yD4 = y[m.oD4] if m.step2 else 0.0
    lbc, ubc = lb[oc:oc + FN].reshape(F, N), ub[oc:oc + FN].reshape(F, N)
    zc, cn = z[oc:oc + FN].reshape(F, N), zn[oc:oc + FN].reshape(F, N)
    cc = m.cost_int[oc:oc + FN].reshape(F, N)          # (the reference's cost of c: 0 on step 2)
    old = m.old.reshape(F, N)
    # deficits the certificate's shifts would serve
    tlo, thi = lbc, ubc
    if m.step2:
        tlo = np.maximum(lbc, old - ub[m.omt:m.omt + FN].reshape(F, N))
        thi = np.minimum(ubc, old + ub[m.omf:m.omf + FN].reshape(F, N))
    deficit = np.minimum(np.maximum(zc, tlo), thi) - eps - S
    # repaired prices
    ts = np.zeros(N)
    lr = 0.0
    if m.has_n:
        on = m.on
        bn = m.cost_int[on:on + N] - m.score_n_coef * yS
        ts = _repair_box(bn, y[m.o6:m.o6 + N] + y[m.o7:m.o7 + N], z[on:on + N], lb[on:on + N], ub[on:on + N], M, eps,
                         float(F))
        rcn = _price_rc(bn, ts, M)
        lr += (_row_lagr(np.minimum(ts, 0.0), m.lo[m.o6:m.o6 + N], m.hi[m.o6:m.o6 + N]) +
               _row_lagr(np.maximum(ts, 0.0), m.lo[m.o7:m.o7 + N], m.hi[m.o7:m.o7 + N]) +
               np.minimum(lb[on:on + N] * rcn, ub[on:on + N] * rcn)).sum()
    b = cc - m.mem_f[:, None] * y3[None, :] - ts[None, :]
    if m.dred:
        b = b + cost_int[oc:oc + FN].reshape(F, N) - yD4
    sr = _repair_box(b, y1 + y2, zc, lbc, ubc, M, eps, float(N))
    rcr = _price_rc(b, sr, M)
    lr += (np.minimum(lbc * rcr, ubc * rcr) - eps * np.maximum(sr, 0.0)).sum() + const
    g0 = cost_x - m.wc * y5[None, :]
    if m.step2:
        g0 = g0 - m._score_coef(m.D32) * yS
    lr += np.where(fmask[m.row_f], g0 - m.row_m[:, None] * sr[m.row_f], INF).min(axis=1).sum()
    lr += (_row_lagr(y3, m.lo[m.o3:m.o3 + N], m.hi[m.o3:m.o3 + N]) +
           _row_lagr(y5, m.lo[m.o5:m.o5 + N], m.hi[m.o5:m.o5 + N])).sum()
    if m.dred:
        lr += float(_row_lagr(np.float64(yS), m.lo[m.oS], m.hi[m.oS])) + \
            float(_row_lagr(np.float64(yD4), m.lo[m.oD4], m.hi[m.oD4]))
    lagr = max(lag_plain, lr)
    # repaired point
    loc, hic = np.maximum(lbc, S / M), np.minimum(ubc, S + eps)
    if m.step2:
        fits = np.maximum(loc, tlo) <= np.minimum(hic, thi)
        loc, hic = np.where(fits, np.maximum(loc, tlo), loc), np.where(fits, np.minimum(hic, thi), hic)
    cr = np.where(loc > hic, loc, np.minimum(np.maximum(cn, loc), hic))
    res = max(0.0, float((loc - hic).max()))
    pobj = (cost_x * xn).sum() + (cc * cr).sum()
    viol = lambda a, lo, hi: np.maximum(np.maximum(lo - a, a - hi), 0.0)   # noqa: E731
    res = max(res, float((viol((m.mem_f[:, None] * cr).sum(axis=0), m.lo[m.o3:m.o3 + N], m.hi[m.o3:m.o3 + N]) /
                          m.rownorm[m.o3:m.o3 + N]).max()),
              float((viol(U, m.lo[m.o5:m.o5 + N], m.hi[m.o5:m.o5 + N]) / m.rownorm[m.o5:m.o5 + N]).max()))
    nr = np.zeros(N)
    if m.has_n:
        sumr = cr.sum(axis=0)
        lon, hin = np.maximum(lb[on:on + N], sumr / M), np.minimum(ub[on:on + N], sumr + eps)
        nr = np.where(lon > hin, lon, np.minimum(np.maximum(zn[on:on + N], lon), hin))
        res = max(res, float((lon - hin).max()))
        pobj += (m.cost_int[on:on + N] * nr).sum()
    if m.step2:
        lmf, lmt = lb[m.omf:m.omf + FN].reshape(F, N), lb[m.omt:m.omt + FN].reshape(F, N)
        mfr, mtr = np.maximum(lmf, cr - old), np.maximum(lmt, old - cr)
        res = max(res, float((mfr - ub[m.omf:m.omf + FN].reshape(F, N)).max()),
                  float((mtr - ub[m.omt:m.omt + FN].reshape(F, N)).max()))
        pobj += (m.cost_int[m.omf:m.omf + FN] * mfr.ravel()).sum() + (m.cost_int[m.omt:m.omt + FN] * mtr.ravel()).sum()
        s = cr.sum() - m.old.sum()
        A, Dm, Kk = min(ub[m.oa], -s), min(ub[m.od], s), m.sigma4 * (-s)
        ar = max(lb[m.oa], A)
        dr = max(lb[m.od], Kk - ar)
        res = max(res, lb[m.oa] - A, dr - Dm)
        pobj += m.cost_int[m.oa] * ar + m.cost_int[m.od] * dr
        score_rep = (m._score_coef(m.D32) * xn).sum() + m.score_n_coef * nr.sum()
        res = max(res, float(viol(score_rep, m.lo[m.oS], m.hi[m.oS]) / m.rownorm[m.oS]))
    return dict(pobj=float(pobj), lagr=float(lagr), lagr_repaired=float(lr), res=float(res), deficit=deficit)


OMEGA_TRAINED = 1024      # nep_internal.h kOmegaTrained


def blocks(m, lbi=None, ubi=None, tol=1e-7, max_iters=100000, check_every=64, verbose=False, inline_reflect=False,
           box=None, eta=None, omega0=None, rs_nec=0.8, fp32=False, engine=False, start=None, warm_band=(2.0, 4.0),
           lineage=0):
    """Same algorithm as the kernels, fp64: blocks of `check_every` iterations; iteration 0 of a block
    is the certificate iteration (a plain PDHG step whose input dual is the previous block's plain
    output), restarts take effect at iteration 1, the last iteration is plain, the others are
    reflected Halpern steps w' = lam (2 T(w) - w) + (1 - lam) w_anchor.
    inline_reflect: form the dual step's reflected activity as K(2ŵ - w) from the primal points
    (what x_pass does for the per-(f, j) rows) instead of 2·Kŵ - kz with the tracked activity kz;
    the two are the same operator (K is linear).
    A generator: one record per certificate iteration, taken right after it — dict(k, status (None while the LP
    iterates), obj, pobj, lag, res, x, z, y (copies of the iterate after that plain step), fpr, last_fpr, prev_fpr,
    k_since (the restart test's operands), dz, dy, restart, omega).  solve() below runs it to its end.
    To step beside the engine (tests/test_gpu_iterates.py): box = (lb, ub) the engine's presolved node box
    (nep_debug_presolve) instead of the mirror's own presolve; eta / omega0 the engine's step size and initial primal
    weight (its power iteration agrees with the mirror's to 1 % only); rs_nec the "necessary" restart factor
    (nep_host.cpp runs 0.9; 0.8 here by default); engine=True adds record["cert"] = engine_certificate(...).
    fp32=True rounds to float32 what the kernels hold in float32 — the routing iterate x, its anchor and the
    projected x̂, the packed duals y1 + y2, cpr y5 and yS the x update reads (kty), tau and lambda in the x
    update, the shifted point x - tau (wobj D - (m kx + w cy5 + wsc yS D)) evaluated term by term in float32
    arithmetic as x_pass writes it (its terms reach tau |g| ~ 10^2 and cancel, so rounding only the result would
    miss most of the noise), the simplex threshold of the plain iterations (its sum over the support added and divided in float32: _theta32),
    and, outside certificate iterations,
    the column sums and CPU sums the duals of C1/C2/C5 take (accumulated in float32 row by row: colsum32) — everything else stays fp64 as on the device: the
    difference to the fp64 run measures the fp32 noise of the iteration itself (not the kernels' summation orders).
    start = (x, z, y, omega): a warm start from a parent's state, as nep_lp_submit with warm_start does it (init_slot
    and the INIT variants of x_pass / node_pass / scalar_pass): x is projected onto the simplexes of this box's open
    destinations (a step of length 0: closed destinations lose their mass, the rest is re-projected), z is clipped
    into the box, y is kept, the activity and the anchors are taken from that point, the iteration count, the
    restart bookkeeping and the best bound start afresh, and the primal weight goes on from the parent's omega within
    the band [max(omega0 1e-5, floor omega), omega0 1e5] — warm_band = (floor, cap) of nep_lp_opts (defaults 2, 4); the
    cap, at most cap x the parent's weight, holds only once the lineage (`lineage`: the parent's iterations and its
    ancestors') has OMEGA_TRAINED iterations behind it.  The weight itself is not clamped at the start: the band
    binds at the first restart's update."""
    if box is None:
        ok, lb, ub, fmask = m.presolve(lbi, ubi)
    else:
        lb, ub = np.array(box[0], float), np.array(box[1], float)
        fmask = (ub[m.oc:m.oc + m.F * m.N] > 0).reshape(m.F, m.N)
        ok = bool(fmask.any(axis=1).all()) and not np.any(lb > ub + 1e-12)
    if not ok:
        yield dict(status=2, obj=INF, pobj=np.nan, iters=0, k=0)
        return
    mask = fmask[m.row_f]
    ce = check_every
    r32 = _f32 if fp32 else (lambda a: a)
    FN = m.F * m.N
    cost_int, const = m.cost_int, 0.0
    if m.dred:
        cost_int, const, m.lo[m.oD4], m.hi[m.oD4] = m.dred_terms(lb, ub)
    omega, eta = (m.omega0 if omega0 is None else float(omega0)), (m.eta if eta is None else float(eta))
    om_lo, om_hi = omega * 1e-5, omega * 1e5
    if start is None:
        x = proj_simplex_rows_sorted(np.zeros((m.R, m.N)), mask)
        x = r32(x)
        z = np.clip(np.zeros(m.n_int), lb, ub)
        y = np.zeros(m.n_dual)
    else:
        x0, z0, y0, omega = r32(np.asarray(start[0], float)), start[1], start[2], float(start[3])
        x, theta = proj_simplex_rows_sorted(x0, mask, return_theta=True)
        if fp32:                                         # (an fp32 threshold, as on every pass but the certificate's)
            x = _f32(np.where(mask, np.maximum(x0 - _theta32(x0, mask, theta)[:, None], 0), 0.0))
        z = np.clip(np.array(z0, float), lb, ub)
        y = np.array(y0, float)
        if warm_band[0] > 0:
            om_lo = min(omega * warm_band[0], om_hi)
        if warm_band[1] > 0 and lineage >= OMEGA_TRAINED:
            om_hi = max(omega * warm_band[1], om_lo)
    kz = m.K(x, z)
    xa, za, ya, kza = x.copy(), z.copy(), y.copy(), kz.copy()
    k = k_since = 0
    ks_base = -ce
    restart_pending = False
    last_fpr, prev_fpr = -1.0, INF
    best = -INF
    cost_x = m.row_wobj[:, None] * np.where(m.row_src[:, None] >= 0, m.D32[np.maximum(m.row_src, 0)], 0.0)
    block = 0
    while True:
        for it in range(ce):
            check, first = it == 0, it == 1
            plain = ce < 4 or it == 0 or it == ce - 1
            if first and restart_pending:
                xa, za, ya, kza = x.copy(), z.copy(), y.copy(), kz.copy()
            tau, sig = eta / omega, eta * omega
            gx, gz = m.KT(y)
            rcx = cost_x - gx
            rcz = cost_int - gz
            if fp32:
                # the x update reads the packed fp32 duals (kty) and an fp32 tau; the Lagrangian above keeps rcx
                # and forms the shifted point in float32 arithmetic, term by term as x_pass writes it:
                # v = x - tau (wobj D - (m kx + w cy5 + wsc yS D))
                f4 = np.float32
                y12 = (y[m.o1:m.o1 + FN] + y[m.o2:m.o2 + FN]).astype(f4).reshape(m.F, m.N)
                cy5 = m.cpr32.astype(f4) * y[m.o5:m.o5 + m.N].astype(f4)[None, :]
                Dr = np.where(m.row_src[:, None] >= 0, m.D32[np.maximum(m.row_src, 0)], 0.0).astype(f4)
                gs = m.row_wsc.astype(f4) * f4(y[m.oS] if m.step2 else 0.0)
                g = m.row_wobj.astype(f4)[:, None] * Dr - (m.row_m.astype(f4)[:, None] * y12[m.row_f] +
                                                           m.row_w.astype(f4)[:, None] * cy5[m.row_f] +
                                                           gs[:, None] * Dr)
                vv = (x.astype(f4) - f4(tau) * g).astype(np.float64)
                xn, theta = proj_simplex_rows_sorted(vv, mask, return_theta=True)
                if not check:       # (plain iterations: an fp32 threshold; certificate ones refine it in fp64)
                    xn = np.where(mask, np.maximum(vv - _theta32(vv, mask, theta)[:, None], 0), 0.0)
                xn = _f32(xn)
            else:
                xn = proj_simplex_rows_sorted(x - tau * rcx, mask)
            zn = np.clip(z - tau * m.gam ** 2 * rcz, lb, ub)
            act = m.K(xn, zn)
            if fp32 and not check:
                # outside certificate iterations the column sums S (C1/C2) and the per-function CPU sums (C5, times
                # cpr) are fp32 accumulators
                # (added row by row in float32, colsum32: over the ~N rows of a function with workload everywhere the
                # error reaches several ulps, which one rounding of the fp64 sum does not show)
                dS = (m.colsum32(m.row_m[:, None] * xn) - m.colsum(m.row_m[:, None] * xn)).ravel()
                Ux = m.colsum32(m.row_w[:, None] * xn)
                act[m.o1:m.o1 + FN] += dS
                act[m.o2:m.o2 + FN] += dS
                act[m.o5:m.o5 + m.N] += _f32(Ux * m.cpr32).sum(axis=0) - (m.wc * xn).sum(axis=0)
            s = sig * m.rho ** 2
            V = y - s * (m.K(2 * xn - x, 2 * zn - z) if inline_reflect else 2 * act - kz)
            with np.errstate(invalid="ignore"):
                a = V + s * m.hi
                b = V + s * m.lo
            yn = np.where(a < 0, a, np.where(b > 0, b, 0.0))
            if check:
                lag = np.where(mask, rcx, INF).min(axis=1).sum()
                lag += np.where(rcz > 0, lb * rcz, ub * rcz).sum()
                with np.errstate(invalid="ignore"):
                    rl = np.where(y > 0, np.where(np.isfinite(m.lo), y * m.lo, -INF),
                                  np.where(y < 0, np.where(np.isfinite(m.hi), y * m.hi, -INF), 0.0))
                lag += rl.sum() + const
                pobj = (cost_x * xn).sum() + (cost_int * zn).sum() + const
                viol = np.maximum(np.maximum(m.lo - act, act - m.hi), 0.0) / m.rownorm
                res = viol.max()
                mvz = ((xn - x) ** 2).sum() + (((zn - z) / m.gam) ** 2).sum()
                mvy = (((yn - y) / m.rho) ** 2).sum()
                dsz = ((xn - xa) ** 2).sum() + (((zn - za) / m.gam) ** 2).sum()
                dsy = (((yn - ya) / m.rho) ** 2).sum()
                cert = engine_certificate(m, lb, ub, fmask, y, z, xn, zn, cost_x, cost_int, const, lag) if engine \
                    else None
            if plain:
                x, z, y, kz = xn, zn, yn, act
            else:
                ks = ks_base + it
                lam = (ks + 1.0) / (ks + 2.0)
                if fp32:
                    x = _f32(_f32(lam) * (2 * xn - x) + (1 - _f32(lam)) * xa)
                else:
                    x = lam * (2 * xn - x) + (1 - lam) * xa
                z = lam * (2 * zn - z) + (1 - lam) * za
                y = lam * (2 * yn - y) + (1 - lam) * ya
                kz = lam * (2 * act - kz) + (1 - lam) * kza
            if check:
                k += 1 if block == 0 else ce
                k_since += 1 if block == 0 else ce
                restart_pending = False
                best = max(best, lag)
                gap = pobj - lag
                if verbose:
                    print(f"{k:7d} res={res:.2e} p={pobj:.10g} L={lag:.10g} gap={gap:.2e} w={omega:.3g}")
                rec = dict(status=None, k=k, iters=k, obj=lag, lag=lag, pobj=pobj, res=res, x=x, z=z, y=y, cert=cert,
                           omega=omega, mvz=mvz, mvy=mvy)
                if np.isfinite(lag) and res <= tol and gap <= tol * max(1.0, abs(lag)):
                    yield dict(rec, status=0)
                    return
                if k >= max_iters:
                    yield dict(rec, status=1, obj=best)
                    return
                fpr = np.sqrt(omega * mvz + mvy / omega)
                if last_fpr < 0:
                    last_fpr = fpr
                restart = (fpr <= 0.2 * last_fpr or (fpr <= rs_nec * last_fpr and fpr > prev_fpr)
                           or k_since >= 0.36 * k)
                dz, dy = np.sqrt(dsz), np.sqrt(dsy)
                yield dict(rec, fpr=fpr, last_fpr=last_fpr, prev_fpr=prev_fpr, k_since=k_since, restart=restart,
                           dz=dz, dy=dy)
                prev_fpr = fpr
                if restart:
                    if dz > 1e-10 and dy > 1e-10:
                        omega = float(np.clip(np.exp(0.5 * np.log(dy / dz) + 0.5 * np.log(omega)), om_lo, om_hi))
                    elif m.dred and dy > 1e-10:      # (reduced step 2: primal static -> weight x10, scalar_pass)
                        omega = float(min(omega * 10.0, om_hi))
                    restart_pending = True
                    k_since = 0
                    ks_base = -1
                    last_fpr = fpr
                    prev_fpr = INF
                else:
                    ks_base += ce
        block += 1


def solve(m, lbi=None, ubi=None, tol=1e-7, max_iters=100000, check_every=64, verbose=False, inline_reflect=False):
    """blocks() run to its end (certified, iteration limit, or presolve-infeasible).
    Returns dict(status, obj, pobj, iters, x, z, y)."""
    for rec in blocks(m, lbi, ubi, tol=tol, max_iters=max_iters, check_every=check_every, verbose=verbose,
                      inline_reflect=inline_reflect):
        if rec["status"] is not None:
            return {k: rec[k] for k in ("status", "obj", "pobj", "iters", "x", "z", "y") if k in rec}
