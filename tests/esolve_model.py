"""The eigensolvers and the diagonal shift as plain numpy: what tests/test_esolve_cpu.py holds to oracle/_ref in every bit at T = 1, 3, 8 threads, and what
the GPU tests compare liblis_amd with in the cases the goldens do not hold.

  esolve()      the five recurrences of src/esolver/lis_esolver_pi.c, _ii.c, _rqi.c, _cg.c (lis_ecg, lis_ecr) on a CSR matrix, statement for statement.
                Element-wise statements are numpy's element-wise IEEE operations (one rounded multiply, one rounded add, no FMA); every inner product is the
                reference's sum for T threads (krylov_model.chunked_sum: T chunks by LIS_GET_ISIE, each left to right from 0.0, the partials added in
                order); A x adds a row's terms left to right from 0.0 (orc.spmv_csr); A^T x is the reference's scatter at T threads (per-thread partial
                vectors added in thread order, lis_matvec_csr.c:113-180).  The inner solves are lis_bicg / lis_cg restated (lis_solver_bicg.c:173-276,
                lis_solver_cg.c:160-234) with lis_solve_kernel's defaults: x0 = 0, -tol 1e-12 on ||r|| / ||b||, -maxiter 1000, no preconditioner.
                The 3 x 3 Rayleigh-Ritz step of lis_ecg restates src/array/lis_array.c's n = 3 branches.
  shift()       lis_matrix_shift_diagonal_{csr,csc,ell,dia,jad,bsr} (src/matrix/lis_matrix_<fmt>.c), the serial branches, on the arrays of lisdrv.matrix_arrays().
"""
import numpy as np

import krylov_model as km
import orc

F = np.float64


# ---------------------------------------------------------------------------------------------- the shift
def shift_matrix(twice=True):
    """n = 13, unsorted columns: rows with the diagonal first, last and in the middle, a row with the diagonal stored twice (twice=False: stored once -- the
    conversions to the other formats are not defined on duplicate entries), rows without a diagonal entry, an empty row, a 1-entry row."""
    rows = [
        [(0, 4.0), (3, -1.0), (7, 0.5)],                 # diagonal first
        [(4, -1.0), (0, 2.0), (1, 5.0)],                 # diagonal last
        [(1, 1.0), (2, 6.0), (5, -2.0), (2 if twice else 8, 60.0)],      # diagonal stored twice: the first one moves
        [(0, 1.5), (6, -0.5)],                           # no diagonal entry
        [(4, 3.25)],                                     # one entry, the diagonal
        [],                                              # empty row
        [(5, 1.0), (6, 7.0), (7, 1.0)],
        [(7, 8.0), (6, 1.0)],
        [(9, 2.0), (10, 1.0)],                           # no diagonal entry
        [(8, 1.0), (9, 9.0)],
        [(10, 1e-300), (12, 1.0)],                       # a tiny diagonal
        [(12, 2.0), (11, -11.0), (0, 1.0)],
        [(11, 1.0)],                                     # last row without a diagonal entry
    ]
    ptr = np.zeros(len(rows) + 1, np.int32)
    idx, val = [], []
    for i, r in enumerate(rows):
        for c, v in r:
            idx.append(c)
            val.append(v)
        ptr[i + 1] = len(idx)
    return ptr, np.array(idx, np.int32), np.array(val, np.float64)


def shift(fmt, a, value, sigma):
    """value after lis_matrix_shift_diagonal(A, sigma): a new array; `a` holds the format's index arrays under the names of lisdrv.matrix_arrays()."""
    v = np.array(value, dtype=np.float64, copy=True)
    s = F(sigma)
    n = a["n"]
    with np.errstate(all="ignore"):
        if fmt in ("csr", "csc"):
            ptr, index = a["ptr"], a["index"]
            for i in range(len(ptr) - 1):
                for j in range(int(ptr[i]), int(ptr[i + 1])):
                    if index[j] == i:
                        v[j] = v[j] - s
                        break
        elif fmt == "ell":
            for i in range(n):
                for j in range(a["maxnzr"]):
                    if a["index"][j * n + i] == i:
                        v[j * n + i] = v[j * n + i] - s
                        break
        elif fmt == "dia":
            for j in range(a["nnd"]):
                if a["index"][j] == 0:
                    for i in range(n):
                        v[j * n + i] = v[j * n + i] - s
                    break
        elif fmt == "jad":
            k = n
            for j in range(a["maxnzr"]):
                if k == 0:
                    break
                l = 0
                for i in range(int(a["ptr"][j]), int(a["ptr"][j + 1])):
                    if a["row"][l] == a["index"][i]:
                        v[i] = v[i] - s
                        k -= 1
                        if k == 0:
                            break
                    l += 1
        elif fmt == "bsr":
            bnr, bnc = a["bnr"], a["bnc"]
            bs = bnr * bnc
            for bi in range(a["nr"]):
                k, i = 0, bi * bnr
                for bj in range(int(a["bptr"][bi]), int(a["bptr"][bi + 1])):
                    bjj = int(a["bindex"][bj])
                    if bjj * bnc <= i < (bjj + 1) * bnc:
                        j = i % bnc
                        while j < bnc and k < bnr and i < n:
                            v[bj * bs + j * bnr + k] = v[bj * bs + j * bnr + k] - s
                            i += 1
                            k += 1
                            j += 1
                    if k == bnr:
                        break
        else:
            raise ValueError(fmt)
    return v


def shift_csr_values(ptr, idx, val, sigma):
    return shift("csr", dict(n=len(ptr) - 1, ptr=ptr, index=idx), val, sigma)


# ---------------------------------------------------------------------------------------------- vectors and products at T threads
class Ops:
    def __init__(self, ptr, idx, val, T):
        self.ptr, self.idx, self.T = np.asarray(ptr, np.int32), np.asarray(idx, np.int32), T
        self.n = len(ptr) - 1
        self.set_values(val)
        self._plan_t()

    def set_values(self, val):
        self.val = np.array(val, dtype=np.float64, copy=True)

    def dot(self, x, y):
        with np.errstate(all="ignore"):
            return F(km.chunked_sum(x * y, self.T))

    def nrm2(self, x):
        with np.errstate(all="ignore"):
            return np.sqrt(F(km.chunked_sum(x * x, self.T)))

    def matvec(self, x):
        return orc.spmv_csr(self.ptr, self.idx, self.val, np.ascontiguousarray(x))

    def _plan_t(self):
        """A^T x of lis_matvech_csr at T threads: thread t scatters its rows (LIS_GET_ISIE) into a work vector of its own, in row order; y[c] is the sum
        of the T work vectors' entries, thread 0 first, from 0.0.  Entries of column c grouped by (c, thread), positions in stored order."""
        n, T = self.n, self.T
        owner = np.zeros(n, np.int64)
        for t in range(T):
            lo, hi = km.isie(t, T, n)
            owner[lo:hi] = t
        groups = {}
        for i in range(n):
            for k in range(int(self.ptr[i]), int(self.ptr[i + 1])):
                groups.setdefault((int(self.idx[k]), int(owner[i])), []).append((k, i))
        self.tsteps = []
        depth = max((len(g) for g in groups.values()), default=0)
        keys = list(groups)
        for p in range(depth):
            sel = [(c * T + t, groups[(c, t)][p]) for (c, t) in keys if len(groups[(c, t)]) > p]
            self.tsteps.append((np.array([s[0] for s in sel], np.int64), np.array([s[1][0] for s in sel], np.int64), np.array([s[1][1] for s in sel], np.int64)))

    def matvech(self, x):
        n, T = self.n, self.T
        parts = np.zeros(n * T)
        with np.errstate(all="ignore"):
            for slot, k, i in self.tsteps:
                parts[slot] = parts[slot] + self.val[k] * x[i]
            parts = parts.reshape(n, T)
            y = np.zeros(n)
            for t in range(T):
                y = y + parts[:, t]
        return y


def _initial(ops, b, tol):
    """lis_solver_get_initial_residual with x0 = 0 and -conv_cond nrm2_r (lis_solver.c:957-1091): r = b, bnrm2 = 1 / ||r||; done when ||r|| bnrm2 <= tol"""
    r = b.copy()
    nrm2 = ops.nrm2(r)
    bnrm2 = F(1.0) if nrm2 == 0.0 else F(1.0) / nrm2
    return r, bnrm2, bool(nrm2 * bnrm2 <= abs(tol))


def bicg(ops, b, tol=1e-12, maxiter=1000):
    """lis_bicg, -p none.  -> x"""
    x = np.zeros(ops.n)
    r, bnrm2, done = _initial(ops, b, tol)
    if done:
        return x
    rtld = r.copy()
    p, ptld = np.zeros(ops.n), np.zeros(ops.n)
    rho_old = F(1.0)
    with np.errstate(all="ignore"):
        for _ in range(1, maxiter + 1):
            z, ztld = r, rtld                         # M = I: copies
            rho = ops.dot(rtld, z)
            if rho == 0.0:
                return x
            beta = rho / rho_old
            p = z + beta * p
            q = ops.matvec(p)
            ptld = ztld + beta * ptld
            qtld = ops.matvech(ptld)
            tmpdot1 = ops.dot(ptld, q)
            if tmpdot1 == 0.0:
                return x
            alpha = rho / tmpdot1
            x = x + alpha * p
            r = r + (-alpha) * q
            nrm2 = ops.nrm2(r) * bnrm2
            if tol >= nrm2:
                return x
            rtld = rtld + (-alpha) * qtld
            rho_old = rho
    return x


def cg(ops, b, tol=1e-12, maxiter=1000):
    """lis_cg, -p none.  -> x"""
    x = np.zeros(ops.n)
    r, bnrm2, done = _initial(ops, b, tol)
    if done:
        return x
    p = np.zeros(ops.n)
    rho_old = F(1.0)
    with np.errstate(all="ignore"):
        for _ in range(1, maxiter + 1):
            z = r
            rho = ops.dot(r, z)
            beta = rho / rho_old
            p = z + beta * p
            q = ops.matvec(p)
            dot_pq = ops.dot(p, q)
            if dot_pq == 0.0:
                return x
            alpha = rho / dot_pq
            x = x + alpha * p
            r = r + (-alpha) * q
            nrm2 = ops.nrm2(r) * bnrm2
            if tol >= nrm2:
                return x
            rho_old = rho
    return x


# ---------------------------------------------------------------------------------------------- lis_array_*, n = 3
def ritz3(A3, B3, emaxiter, tol):
    """The inverse iteration of lis_esolver_cg.c:290-305 on A3 z = B3 v (column-major 3 x 3).  -> v3"""
    v3 = np.ones(3)
    W3 = np.zeros(9)
    with np.errstate(all="ignore"):
        it = 0
        while it < emaxiter:
            it += 1
            t = F(0.0)
            for i in range(3):
                t = t + v3[i] * v3[i]
            nrm2 = np.sqrt(t)
            a = F(1.0) / nrm2
            v3 = np.array([a * v3[i] for i in range(3)])
            Bv = np.array([B3[0] * v3[0] + B3[3] * v3[1] + B3[6] * v3[2], B3[1] * v3[0] + B3[4] * v3[1] + B3[7] * v3[2], B3[2] * v3[0] + B3[5] * v3[1] + B3[8] * v3[2]])
            W3[:] = A3
            for k in range(3):
                W3[k + k * 3] = F(1.0) / W3[k + k * 3]
                for i in range(k + 1, 3):
                    t = W3[i + k * 3] * W3[k + k * 3]
                    for j in range(k + 1, 3):
                        W3[i + j * 3] = W3[i + j * 3] - t * W3[k + j * 3]
                    W3[i + k * 3] = t
            z3 = np.zeros(3)
            for i in range(3):
                z3[i] = Bv[i]
                for j in range(i):
                    z3[i] = z3[i] - W3[i + j * 3] * z3[j]
            for i in (2, 1, 0):
                for j in range(i + 1, 3):
                    z3[i] = z3[i] - W3[i + j * 3] * z3[j]
                z3[i] = z3[i] * W3[i + i * 3]
            mu3 = F(0.0)
            for i in range(3):
                mu3 = mu3 + Bv[i] * z3[i]
            q3 = np.array([-mu3 * Bv[i] + z3[i] for i in range(3)])
            t = F(0.0)
            for i in range(3):
                t = t + q3[i] * q3[i]
            if np.sqrt(t) < tol:
                break
            v3 = z3.copy()
    return v3


# ---------------------------------------------------------------------------------------------- the five loops
def _options(text):
    tok = text.split()
    o = {"e": "cr", "emaxiter": 1000, "etol": 1e-12, "shift": 0.0, "initx_ones": True}
    for k, v in zip(tok[:-1], tok[1:]):
        if k == "-e":
            o["e"] = v
        elif k == "-emaxiter":
            o["emaxiter"] = int(v)
        elif k == "-etol":
            o["etol"] = float(v)
        elif k == "-shift":
            o["shift"] = float(v)
        elif k == "-initx_ones":
            o["initx_ones"] = v in ("true", "1")
    return o


def esolve(ptr, idx, val, options, T=1, x0=None):
    """lis_esolve(A, x, ...) with -eprint mem -> dict(iter, status, evalue, resid, rhistory, x); val is left as the caller gave it (the shifted and unshifted
    values are out["value_after"]: the reference's drift)."""
    o = _options(options)
    ops = Ops(ptr, idx, val, T)
    n, tol, emaxiter, oshift = ops.n, F(o["etol"]), o["emaxiter"], F(o["shift"])
    v = np.ones(n) if o["initx_ones"] else np.array(x0, dtype=np.float64, copy=True)      # xx: ones, or a copy of the caller's x; the loop's own set_all repeats it
    rhistory = [F(1.0)]
    e = o["e"]
    with np.errstate(all="ignore"):
        def unit(u):
            return (F(1.0) / ops.nrm2(u)) * u
        if e != "rqi" and oshift != 0.0:
            ops.set_values(shift_csr_values(ptr, idx, ops.val, oshift))
        status = 4
        it = 0
        resid = F(0.0)
        if e in ("pi", "ii"):
            theta = F(0.0)
            while it < emaxiter:
                it += 1
                v = unit(v)
                y = ops.matvec(v) if e == "pi" else bicg(ops, v)
                theta = ops.dot(v, y)
                q = (-theta) * v + y
                resid = ops.nrm2(q) / abs(theta)
                v = y.copy()
                rhistory.append(resid)
                if tol >= resid:
                    status = 0
                    break
            evalue = theta + oshift if e == "pi" else F(1.0) / theta + oshift
            v = unit(v)
        elif e == "rqi":
            v = unit(v)
            y = ops.matvec(v)
            rho = ops.dot(v, y)
            while it < emaxiter:
                it += 1
                ops.set_values(shift_csr_values(ptr, idx, ops.val, rho))
                y = bicg(ops, v)
                ops.set_values(shift_csr_values(ptr, idx, ops.val, -rho))
                theta = ops.nrm2(y)
                dotvy = ops.dot(v, y)
                rho = rho + dotvy / (theta * theta)
                q = (-dotvy) * v + y
                resid = ops.nrm2(q) / abs(dotvy)
                y = (F(1.0) / theta) * y
                v = y.copy()
                rhistory.append(resid)
                if tol >= resid:
                    status = 0
                    break
            evalue = rho
            v = unit(v)
        elif e == "cg":
            x = unit(v)
            Ax = ops.matvec(x)
            p = cg(ops, x)
            Ap = x.copy()
            lam = F(0.0)
            while it < emaxiter:
                it += 1
                lam = ops.dot(x, Ax)
                r = (F(-1.0) / lam) * Ax + x
                resid = ops.nrm2(r)
                rhistory.append(resid)
                if resid < tol:
                    break
                w = unit(r.copy())
                Aw = ops.matvec(w)
                A3, B3 = np.zeros(9), np.zeros(9)
                A3[0], A3[3], A3[6] = ops.dot(w, Aw), ops.dot(x, Aw), ops.dot(p, Aw)
                A3[1] = A3[3]
                A3[4], A3[7] = ops.dot(x, Ax), ops.dot(p, Ax)
                A3[2], A3[5] = A3[6], A3[7]
                A3[8] = ops.dot(p, Ap)
                B3[0], B3[3], B3[6] = ops.dot(w, w), ops.dot(x, w), ops.dot(p, w)
                B3[1] = B3[3]
                B3[4], B3[7] = ops.dot(x, x), ops.dot(p, x)
                B3[2], B3[5] = B3[6], B3[7]
                B3[8] = ops.dot(p, p)
                v3 = ritz3(A3, B3, emaxiter, tol)
                w = v3[0] * w
                w = w + v3[2] * p
                x = w + v3[1] * x
                p = w.copy()
                Aw = v3[0] * Aw
                Aw = Aw + v3[2] * Ap
                Ax = Aw + v3[1] * Ax
                Ap = Aw.copy()
                a = F(1.0) / ops.nrm2(x)
                x, Ax = a * x, a * Ax
                a = F(1.0) / ops.nrm2(p)
                p, Ap = a * p, a * Ap
            status = 0 if resid < tol else 4
            evalue = lam + oshift
            v = x
        elif e == "cr":
            x = unit(v)
            Ax = ops.matvec(x)
            lam = ops.dot(x, Ax)
            r = (-lam) * x + Ax
            r = F(-1.0) * r
            p = r.copy()
            Ap = ops.matvec(p)
            while it < emaxiter:
                it += 1
                rAp, rp, ApAp, pAp, pp = ops.dot(r, Ap), ops.dot(r, p), ops.dot(Ap, Ap), ops.dot(p, Ap), ops.dot(p, p)
                alpha = (rAp - lam * rp) / (ApAp - F(2.0) * lam * pAp + lam * lam * pp)
                x = x + alpha * p
                Ax = ops.matvec(x)
                lam = ops.dot(x, Ax)
                nrm2 = ops.nrm2(x)
                lam = lam / (nrm2 * nrm2)
                r = (-lam) * x + Ax
                r = F(-1.0) * r
                w = r.copy()
                Aw = ops.matvec(w)
                AwAp, pAw, wAp, wp = ops.dot(Aw, Ap), ops.dot(p, Aw), ops.dot(w, Ap), ops.dot(w, p)
                beta = -(AwAp - lam * (pAw + wAp) + lam * lam * wp) / (ApAp - F(2.0) * lam * pAp + lam * lam * pp)
                p = w + beta * p
                Ap = Aw + beta * Ap
                resid = ops.nrm2(r) / abs(lam)
                rhistory.append(resid)
                if resid < tol:
                    break
            status = 0 if resid < tol else 4
            evalue = lam + oshift
            v = unit(x)
        else:
            raise ValueError(e)
        if e != "rqi" and oshift != 0.0:
            ops.set_values(shift_csr_values(ptr, idx, ops.val, -oshift))
    count = it + 1 - (1 if status != 0 else 0)
    return dict(iter=it, status=status, evalue=float(evalue), resid=float(resid), rhistory=np.array(rhistory[:count], np.float64), x=np.asarray(v, np.float64),
                value_after=ops.val)


# what the CPU test runs against oracle/_ref at T = 1, 3, 8: every solver once on the symmetric matrix with a shift, the power iteration on the
# nonsymmetric one, one solve from a given start vector.  (matrix of esolve_drv.MATRICES, options, start vector given)
MODEL_CASES = [
    ("sym7", "-e pi -shift 0.75 -etol 1e-10 -emaxiter 500 -eprint mem", False),
    ("sym7", "-e ii -shift 0.75 -etol 1e-10 -emaxiter 10 -eprint mem", False),        # (ends at the iteration limit: the other exit, and a test that stays quick)
    ("sym7", "-e rqi -shift 0 -etol 1e-10 -emaxiter 8 -eprint mem", False),            # (converges in 6 at T = 1; at T = 8 the reference needs 104)
    ("sym7", "-e cg -shift 0.75 -etol 1e-10 -emaxiter 500 -eprint mem", False),
    ("sym7", "-e cr -shift 0.75 -etol 1e-10 -emaxiter 500 -eprint mem", False),
    ("sym7", "-e cr -shift 0 -initx_ones false -etol 1e-10 -emaxiter 500 -eprint mem", True),
    ("nonsym7", "-e pi -shift 0 -etol 1e-10 -emaxiter 500 -eprint mem", False),
]
