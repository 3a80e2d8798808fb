"""A plain numpy float64 model of the device-driven Krylov loops' building blocks.  Test infrastructure only.

Written from the reference's solver loops (src/solver/lis_solver_cg.c:176-215, lis_solver_bicgstab.c:187-308,
lis_solver_bicg.c:176-262), its vector kernels (src/vector/lis_vector_opv.c, lis_vector_ops.c) and the contract of
the state block in include/liship.h -- which slot a step reads and which it writes -- not from the kernels.
tests/test_krylov_model_cpu.py composes these pieces into whole loops and pins them to the CPU oracle in every
bit; tests/test_krylov_steps_gpu.py then holds every kernel to them.

Every statement is one rounded multiply and one rounded add on numpy float64 (numpy's element-wise loops do not
contract a*x + y into a fused multiply-add), in the reference's statement order.
"""
import math

import numpy as np

# the state block (include/liship.h, LISHIP_KS_*)
(KS_RHO, KS_RHO_OLD, KS_ALPHA, KS_NALPHA, KS_BETA, KS_OMEGA, KS_NOMEGA, KS_DOT0, KS_DOT1, KS_SUM0, KS_SUM1, KS_NRM2,
 KS_BNRM, KS_TOL, KS_ITER, KS_DONE, KS_STATUS, KS_NOT_HALF, KS_NHIST) = range(19)
KS_LEN = 32
# the scalar steps (LISHIP_STEP_*)
(STEP_CG_ALPHA, STEP_CG_RESID, STEP_CG_RESID_PRE, STEP_BICGSTAB_ALPHA, STEP_BICGSTAB_HALF, STEP_BICGSTAB_OMEGA,
 STEP_BICGSTAB_RESID, STEP_BICG_ALPHA, STEP_BICG_RESID, STEP_BICG_RHO) = range(1, 11)
STEPS = tuple(range(1, 11))
STEP_NAMES = {STEP_CG_ALPHA: "cg_alpha", STEP_CG_RESID: "cg_resid", STEP_CG_RESID_PRE: "cg_resid_pre",
              STEP_BICGSTAB_ALPHA: "bicgstab_alpha", STEP_BICGSTAB_HALF: "bicgstab_half",
              STEP_BICGSTAB_OMEGA: "bicgstab_omega", STEP_BICGSTAB_RESID: "bicgstab_resid",
              STEP_BICG_ALPHA: "bicg_alpha", STEP_BICG_RESID: "bicg_resid", STEP_BICG_RHO: "bicg_rho"}
STATUS_RUNNING, STATUS_CONVERGED, STATUS_BREAKDOWN = 0.0, 1.0, 2.0

# the sums a step consumes: (first slot, count).  These are the sums the reference passes through MPI_Allreduce at that
# point of the loop (lis_vector_dot / lis_vector_nrm2, lis_vector_ops.c:119,263), in the slots liship.h names per step.
FOLD = {
    STEP_CG_ALPHA: (KS_DOT0, 1),          # <p,q>
    STEP_CG_RESID: (KS_SUM0, 1),          # sum r^2 (also the next rho)
    STEP_CG_RESID_PRE: (KS_SUM0, 2),      # sum r^2, <r,z>
    STEP_BICGSTAB_ALPHA: (KS_DOT0, 1),    # <rtld,v>
    STEP_BICGSTAB_HALF: (KS_SUM0, 1),     # sum s^2
    STEP_BICGSTAB_OMEGA: (KS_DOT0, 2),    # <t,s>, <t,t>
    STEP_BICGSTAB_RESID: (KS_SUM0, 2),    # sum r^2, <rtld,r>
    STEP_BICG_ALPHA: (KS_DOT0, 1),        # <ptld,q>
    STEP_BICG_RESID: (KS_SUM0, 1),        # sum r^2
    STEP_BICG_RHO: (KS_SUM0, 2),          # sum rtld^2 (unused), <rtld, M^-1 r>
}

_f = np.float64


def new_state(**slots):
    """a zeroed state block with NOT_HALF armed; keyword names are the KS_* names in lower case"""
    st = np.zeros(KS_LEN)
    st[KS_NOT_HALF] = 1.0
    for k, v in slots.items():
        st[globals()["KS_" + k.upper()]] = v
    return st


def rank_fold(gathered, nranks, count):
    """out[k] = sum over ranks in rank order, from 0.0, of gathered[r*count + k] (MPI_Allreduce's half on the device)"""
    g = np.asarray(gathered, dtype=np.float64)
    out = np.zeros(count)
    with np.errstate(all="ignore"):
        for k in range(count):
            s = _f(0.0)
            for r in range(nranks):
                s = s + g[r * count + k]
            out[k] = s
    return out


def step(kind, st, rhist, gathered=None, nranks=0):
    """One scalar step, in place, on the 32-double state `st` and the history array `rhist` (or None)."""
    if kind not in FOLD:
        raise ValueError("no such step: %r" % (kind,))
    with np.errstate(all="ignore"):
        _step(kind, st, rhist, gathered, nranks)


def _step(kind, st, rhist, gathered, nranks):
    st[KS_NOT_HALF] = 1.0
    if st[KS_DONE] != 0.0:
        return
    if gathered is not None:
        slot, count = FOLD[kind]
        st[slot:slot + count] = rank_fold(gathered, nranks, count)

    def completed(nrm2):                       # the iteration is counted, its residual recorded
        it = st[KS_ITER] + _f(1.0)
        st[KS_ITER] = it
        st[KS_NRM2] = nrm2
        st[KS_NHIST] = it
        if rhist is not None:
            rhist[int(it)] = nrm2

    def stop(status):
        st[KS_STATUS] = status
        st[KS_DONE] = 1.0

    def breakdown():                           # solver->iter = iter; no history entry, resid as it was
        st[KS_ITER] = st[KS_ITER] + _f(1.0)
        stop(STATUS_BREAKDOWN)

    def set_alpha(alpha):
        st[KS_ALPHA] = alpha
        st[KS_NALPHA] = -alpha

    def residual():                            # lis_solver_get_residual_nrm2_r: nrm2(r) * bnrm2
        return np.sqrt(st[KS_SUM0]) * st[KS_BNRM]

    def next_rho(rho):
        st[KS_RHO_OLD] = st[KS_RHO]
        st[KS_RHO] = rho

    if kind == STEP_CG_ALPHA:                  # lis_solver_cg.c:193-204
        if st[KS_DOT0] == 0.0:
            return breakdown()
        set_alpha(st[KS_RHO] / st[KS_DOT0])
    elif kind in (STEP_CG_RESID, STEP_CG_RESID_PRE):       # :207-215, then rho, beta of the next iteration (:180-183)
        nrm2 = residual()
        completed(nrm2)
        if st[KS_TOL] >= nrm2:
            return stop(STATUS_CONVERGED)
        next_rho(st[KS_SUM1] if kind == STEP_CG_RESID_PRE else st[KS_SUM0])
        st[KS_BETA] = st[KS_RHO] / st[KS_RHO_OLD]
    elif kind == STEP_BICGSTAB_ALPHA:          # lis_solver_bicgstab.c:193-200, :230
        if st[KS_RHO] == 0.0:
            return breakdown()
        set_alpha(st[KS_RHO] / st[KS_DOT0])
    elif kind == STEP_BICGSTAB_HALF:           # :236-254
        nrm2 = residual()
        if nrm2 <= st[KS_TOL]:
            completed(nrm2)
            st[KS_NOT_HALF] = 0.0              # the x update that follows is owed exactly now
            return stop(STATUS_CONVERGED)
        st[KS_NRM2] = nrm2
    elif kind == STEP_BICGSTAB_OMEGA:          # :267-269
        omega = st[KS_DOT0] / st[KS_DOT1]
        st[KS_OMEGA] = omega
        st[KS_NOMEGA] = -omega
    elif kind == STEP_BICGSTAB_RESID:          # :279-307, then rho, beta of the next iteration (:190, :209)
        nrm2 = residual()
        completed(nrm2)
        if st[KS_TOL] >= nrm2:
            return stop(STATUS_CONVERGED)
        if st[KS_OMEGA] == 0.0:
            return stop(STATUS_BREAKDOWN)
        next_rho(st[KS_SUM1])
        st[KS_BETA] = (st[KS_RHO] / st[KS_RHO_OLD]) * (st[KS_ALPHA] / st[KS_OMEGA])
    elif kind == STEP_BICG_ALPHA:              # lis_solver_bicg.c:187-195, :226-238
        if st[KS_RHO] == 0.0 or st[KS_DOT0] == 0.0:
            return breakdown()
        set_alpha(st[KS_RHO] / st[KS_DOT0])
    elif kind == STEP_BICG_RESID:              # :244-256
        nrm2 = residual()
        completed(nrm2)
        if st[KS_TOL] >= nrm2:
            return stop(STATUS_CONVERGED)
    elif kind == STEP_BICG_RHO:                # :258-260, then rho, beta of the next iteration (:180-197)
        next_rho(st[KS_SUM1])
        st[KS_BETA] = st[KS_RHO] / st[KS_RHO_OLD]


# ---------------------------------------------------------------- element-wise kernels (lis_vector_opv.c)
def _e(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_e
def axpy(a, x, y):
    """y[i] += a * x[i]"""
    return y + _f(a) * x


@_e
def xpay(x, a, y):
    """y[i] = x[i] + a * y[i]"""
    return x + _f(a) * y


@_e
def pmul(x, y):
    """z[i] = x[i] * y[i]"""
    return x * y


@_e
def pmul_xpay(x, d, a, y):
    """z = x.*d (Jacobi solve), then y = z + a*y"""
    z = x * d
    return z + _f(a) * y


@_e
def axpy2(a, x, b, w, y):
    """y += a*x, then y += b*w"""
    y = y + _f(a) * x
    return y + _f(b) * w


@_e
def axpy_xpay(a, x, w, b, y):
    """y += a*x, then y = w + b*y"""
    y = y + _f(a) * x
    return w + _f(b) * y


@_e
def cg_direction(alpha, beta, r, dinv, p, x, dc=None):
    """x += alpha*p on the old p (alpha None: x untouched), z = M^-1 r (copy, r.*dinv, or r*dc), p = z + beta*p.
    Returns (p, x)."""
    xn = x if alpha is None else x + _f(alpha) * p
    z = r * _f(dc) if dc is not None else (r * dinv if dinv is not None else r)
    return z + _f(beta) * p, xn


# ---------------------------------------------------------------- fused update passes: vectors and the TERMS of their sums
@_e
def cg_update(alpha, p, q, dinv, x, r):
    """x += alpha*p; r += (-alpha)*q; terms {r^2} (+ {r*(r.*dinv)} with dinv).  Returns (x, r, [terms...])."""
    xn = x + _f(alpha) * p
    rn = r + (-_f(alpha)) * q
    terms = [rn * rn]
    if dinv is not None:
        terms.append(rn * (rn * dinv))
    return xn, rn, terms


@_e
def axpy_sumsq(a, x, y):
    """y += a*x; terms {y^2}.  Returns (y, [terms])."""
    yn = y + _f(a) * x
    return yn, [yn * yn]


@_e
def axpy_sumsq_dot(a, x, y, v):
    """y += a*x; terms {y^2, v*y}"""
    yn = y + _f(a) * x
    return yn, [yn * yn, v * yn]


@_e
def cg_residual_jacobi(na, q, dinv, r, dc=None):
    """r += na*q; z = r.*dinv (or r*dc); terms {r^2, r*z}"""
    rn = r + _f(na) * q
    z = rn * (_f(dc) if dc is not None else dinv)
    return rn, [rn * rn, rn * z]


@_e
def bicgstab_end(alpha, omega, nomega, phat, t, rtld, x, r):
    """s is r[] on entry: x += alpha*phat; x += omega*s; r = s + nomega*t; terms {r^2, rtld*r}.  Returns (x, r, terms)."""
    s = r
    xn = x + _f(alpha) * phat
    xn = xn + _f(omega) * s
    rn = s + _f(nomega) * t
    return xn, rn, [rn * rn, rtld * rn]


@_e
def dot_terms(x, y):
    return x * y


def gather(index, x):
    return x[index]


def scatter_add(index, wr, y):
    """y[index[i]] += wr[i], indices unique"""
    out = y.copy()
    out[index] = y[index] + wr
    return out


# ---------------------------------------------------------------- sums
def isie(t, T, n):
    """LIS_GET_ISIE(t, T, n): the contiguous chunk of thread t of T (include/lis.h:1067-1078)"""
    if t < n % T:
        ie = n // T + 1
        is_ = ie * t
    else:
        ie = n // T
        is_ = ie * t + n % T
    return is_, is_ + ie


def _left_to_right(terms):
    """0.0 + t0 + t1 + ... one rounded add at a time (np.add.accumulate is strictly sequential)"""
    if len(terms) == 0:
        return _f(0.0)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate(([0.0], terms)))[-1]


def chunked_sum(terms, T=1):
    """the reference's sum for OMP_NUM_THREADS = T: each chunk LIS_GET_ISIE(t, T, n) left to right from 0.0, then the T
    partials added serially, chunk 0 first, from 0.0 (lis_vector_ops.c:88-107)"""
    terms = np.asarray(terms, dtype=np.float64)
    n = len(terms)
    partials = []
    for t in range(T):
        lo, hi = isie(t, T, n)
        partials.append(_left_to_right(terms[lo:hi]))
    return float(_left_to_right(np.array(partials)))


def exact_sum(terms):
    """the correctly rounded sum (tree mode is compared with it inside a bound)"""
    return math.fsum(np.asarray(terms, dtype=np.float64).tolist())
