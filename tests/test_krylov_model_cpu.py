"""tests/krylov_model.py is a reference, not a second copy of the kernels: composed into whole CG / BiCGSTAB / BiCG loops in the
order the device-driven loops launch their passes (lis_amd/csrc/host/lis_solver.c: cg_batch, bicgstab_batch, bicg_batch), with
the oracle's products and one-chunk sums, it must reproduce the CPU oracle -- iteration count, return code, residual,
every history entry and every bit of x -- however the loop ends: tolerance, maxiter, breakdown, BiCGSTAB's half step.
A kernel launched behind a raised guard does nothing, so the loops below simply stop at the first raised DONE."""
import numpy as np
import pytest

import krylov_model as km
import orc
from krylov_model import (KS_ALPHA, KS_BETA, KS_DONE, KS_DOT0, KS_DOT1, KS_ITER, KS_NALPHA, KS_NOMEGA, KS_NOT_HALF, KS_NRM2,
                          KS_OMEGA, KS_STATUS, KS_SUM0, KS_SUM1)

GRID = (6, 5, 4)


def poisson():
    return orc.poisson3d(*GRID)


def nonsym(seed=5):
    """the perturbation of test_device_loops_gpu.nonsym on the small grid: off-diagonal entries scaled independently"""
    ptr, idx, val = orc.poisson3d(*GRID)
    val = val.copy()
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    off = idx != rows
    val[off] *= np.random.default_rng(seed).uniform(0.2, 1.0, int(off.sum()))
    return ptr, idx, val


def scaled_identity(c, n=37):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, float(c))


MATRICES = {"poisson": poisson, "nonsym": nonsym, "two_i": lambda: scaled_identity(2.0), "zero": lambda: scaled_identity(0.0)}


def setup(ptr, idx, val, b, precon, tol):
    """lis_solver.c's initial residual for x0 = 0 (r = b, bnrm = 1/||r||) and the Jacobi 1/diag"""
    dinv = 1.0 / orc.csr_diagonal(ptr, idx, val) if precon == "jacobi" else None
    r = b.copy()
    nrm = np.sqrt(km.chunked_sum(r * r))
    bnrm = 1.0 if nrm == 0.0 else 1.0 / nrm
    early = (nrm * bnrm) if nrm * bnrm <= abs(tol) else None
    return dinv, r, bnrm, early


def finish(st, x, rh, maxiter):
    if st[KS_STATUS] == km.STATUS_CONVERGED:
        return x, int(st[KS_ITER]), 0, st[KS_NRM2], rh
    if st[KS_STATUS] == km.STATUS_BREAKDOWN:
        return x, int(st[KS_ITER]), 2, st[KS_NRM2], rh
    return x, maxiter + 1, 4, st[KS_NRM2], rh


def history(maxiter):
    rh = np.zeros(maxiter + 2)
    rh[0] = 1.0
    return rh


def sums(st, slot, terms):
    for k, t in enumerate(terms):
        st[slot + k] = km.chunked_sum(t)


def model_cg(ptr, idx, val, b, precon, tol, maxiter):
    n = len(b)
    x, p, rh = np.zeros(n), np.zeros(n), history(maxiter)
    dinv, r, bnrm, early = setup(ptr, idx, val, b, precon, tol)
    if early is not None:
        return x, 1, 0, early, rh
    rho = km.chunked_sum(r * (r * dinv if dinv is not None else r))
    st = km.new_state(rho=rho, rho_old=1.0, beta=rho / 1.0, bnrm=bnrm, tol=tol)
    for k in range(maxiter):
        if st[KS_DONE] != 0.0:
            break
        p, x = km.cg_direction(st[KS_ALPHA] if k else None, st[KS_BETA], r, dinv, p, x)
        q = orc.spmv_csr(ptr, idx, val, p)
        sums(st, KS_DOT0, [km.dot_terms(p, q)])
        km.step(km.STEP_CG_ALPHA, st, rh)
        if st[KS_DONE] != 0.0:
            break
        if dinv is not None:
            r, terms = km.cg_residual_jacobi(st[KS_NALPHA], q, dinv, r)
        else:
            r, terms = km.axpy_sumsq(st[KS_NALPHA], q, r)
        sums(st, KS_SUM0, terms)
        km.step(km.STEP_CG_RESID_PRE if dinv is not None else km.STEP_CG_RESID, st, rh)
    if maxiter > 0 and st[KS_STATUS] != km.STATUS_BREAKDOWN:       # the deferred x update of the last alpha
        x = km.axpy(st[KS_ALPHA], p, x)
    return finish(st, x, rh, maxiter)


def model_bicgstab(ptr, idx, val, b, precon, tol, maxiter):
    n = len(b)
    x, p, v, rh = np.zeros(n), np.zeros(n), np.zeros(n), history(maxiter)
    dinv, r, bnrm, early = setup(ptr, idx, val, b, precon, tol)
    if early is not None:
        return x, 1, 0, early, rh
    rtld = r.copy()
    st = km.new_state(rho=km.chunked_sum(rtld * r), rho_old=1.0, alpha=1.0, nalpha=-1.0, omega=1.0, nomega=-1.0, bnrm=bnrm, tol=tol)
    for k in range(maxiter):
        if st[KS_DONE] != 0.0:
            break
        p = r.copy() if k == 0 else km.axpy_xpay(st[KS_NOMEGA], v, r, st[KS_BETA], p)
        phat = km.pmul(p, dinv) if dinv is not None else p
        v = orc.spmv_csr(ptr, idx, val, phat)
        sums(st, KS_DOT0, [km.dot_terms(rtld, v)])
        km.step(km.STEP_BICGSTAB_ALPHA, st, rh)
        if st[KS_DONE] != 0.0:
            break
        r, terms = km.axpy_sumsq(st[KS_NALPHA], v, r)               # s, in r's place
        sums(st, KS_SUM0, terms)
        km.step(km.STEP_BICGSTAB_HALF, st, rh)
        if st[KS_NOT_HALF] == 0.0:                                 # the pass guarded on NOT_HALF
            x = km.axpy(st[KS_ALPHA], phat, x)
        if st[KS_DONE] != 0.0:
            break
        shat = km.pmul(r, dinv) if dinv is not None else r
        t = orc.spmv_csr(ptr, idx, val, shat)
        sums(st, KS_DOT0, [km.dot_terms(r, t), km.dot_terms(t, t)])
        km.step(km.STEP_BICGSTAB_OMEGA, st, rh)
        if dinv is not None:
            x = km.axpy2(st[KS_ALPHA], phat, st[KS_OMEGA], shat, x)
            r, terms = km.axpy_sumsq_dot(st[KS_NOMEGA], t, r, rtld)
        else:
            x, r, terms = km.bicgstab_end(st[KS_ALPHA], st[KS_OMEGA], st[KS_NOMEGA], phat, t, rtld, x, r)
        sums(st, KS_SUM0, terms)
        km.step(km.STEP_BICGSTAB_RESID, st, rh)
    return finish(st, x, rh, maxiter)


def model_bicg(ptr, idx, val, b, precon, tol, maxiter):
    n = len(b)
    x, p, ptld, rh = np.zeros(n), np.zeros(n), np.zeros(n), history(maxiter)
    dinv, r, bnrm, early = setup(ptr, idx, val, b, precon, tol)
    if early is not None:
        return x, 1, 0, early, rh
    rtld = r.copy()
    rho = km.chunked_sum(rtld * (r * dinv if dinv is not None else r))
    st = km.new_state(rho=rho, rho_old=1.0, beta=rho / 1.0, bnrm=bnrm, tol=tol)
    for k in range(maxiter):
        if st[KS_DONE] != 0.0:
            break
        if dinv is not None:
            p, ptld = km.pmul_xpay(r, dinv, st[KS_BETA], p), km.pmul_xpay(rtld, dinv, st[KS_BETA], ptld)
        else:
            p, ptld = km.xpay(r, st[KS_BETA], p), km.xpay(rtld, st[KS_BETA], ptld)
        q = orc.spmv_csr(ptr, idx, val, p)
        sums(st, KS_DOT0, [km.dot_terms(ptld, q)])
        km.step(km.STEP_BICG_ALPHA, st, rh)
        if st[KS_DONE] != 0.0:
            break
        qtld = orc.spmvh_csr(ptr, idx, val, ptld)
        x, r, terms = km.cg_update(st[KS_ALPHA], p, q, None, x, r)
        sums(st, KS_SUM0, terms)
        km.step(km.STEP_BICG_RESID, st, rh)
        if st[KS_DONE] != 0.0:
            break
        z = km.pmul(r, dinv) if dinv is not None else r
        rtld, terms = km.axpy_sumsq_dot(st[KS_NALPHA], qtld, rtld, z)
        sums(st, KS_SUM0, terms)
        km.step(km.STEP_BICG_RHO, st, rh)
    return finish(st, x, rh, maxiter)


SOLVERS = {"cg": (model_cg, orc.cg), "bicgstab": (model_bicgstab, orc.bicgstab), "bicg": (model_bicg, orc.bicg)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(solver, matrix, precon, maxiter, tol=1e-12):
    ptr, idx, val = MATRICES[matrix]()
    n = len(ptr) - 1
    b = np.random.default_rng(11).uniform(-1, 1, n)
    model, oracle = SOLVERS[solver]
    xm, itm, rcm, residm, rhm = model(ptr, idx, val, b, precon, tol, maxiter)
    xo, ito, rco, resido, rho = oracle(ptr, idx, val, b, precon=precon, tol=tol, maxiter=maxiter)
    assert (itm, rcm) == (ito, rco)
    assert bits(residm) == bits(resido)
    assert np.array_equal(bits(rhm), bits(rho))
    assert np.array_equal(bits(xm), bits(xo))
    return ito, rco


@pytest.mark.parametrize("precon", ["none", "jacobi"])
@pytest.mark.parametrize("matrix", ["poisson", "nonsym"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "bicg"])
def test_model_loops_converge_as_the_oracle(solver, matrix, precon):
    if solver == "cg" and matrix == "nonsym":
        it, rc = compare(solver, matrix, precon, 12)           # CG on a non-symmetric matrix: any dozen iterations, bit for bit
        return
    it, rc = compare(solver, matrix, precon, 300)
    assert rc == 0 and 3 < it < 300


@pytest.mark.parametrize("maxiter", [0, 1, 3])
@pytest.mark.parametrize("precon", ["none", "jacobi"])
@pytest.mark.parametrize("matrix", ["poisson", "nonsym"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "bicg"])
def test_model_loops_at_maxiter(solver, matrix, precon, maxiter):
    it, rc = compare(solver, matrix, precon, maxiter)
    assert (it, rc) == (maxiter + 1, 4)


@pytest.mark.parametrize("maxiter", [1, 3])
@pytest.mark.parametrize("precon", ["none", "jacobi"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "bicg"])
def test_model_loops_on_twice_the_identity(solver, precon, maxiter):
    """one iteration is exact; BiCGSTAB leaves at its half step (s = r - (1/2) 2r = 0) and owes x its alpha*phat"""
    it, rc = compare(solver, "two_i", precon, maxiter)
    assert (it, rc) == (1, 0)


@pytest.mark.parametrize("maxiter", [1, 3])
@pytest.mark.parametrize("solver", ["cg", "bicg"])
def test_model_loops_break_down_on_the_zero_matrix(solver, maxiter):
    """<p,q> = 0 in the first iteration: iteration 1 is counted, no history entry is written, x stays x0"""
    it, rc = compare(solver, "zero", "none", maxiter)
    assert (it, rc) == (1, 2)


def test_chunked_sum_is_the_reference_order():
    """{1e16, 1, -1e16, 1}: left to right the first 1 is absorbed (1.0); two chunks give (1e16 + 1) + (-1e16 + 1) = 0.0;
    the exact sum is 2.0.  A chunk that holds only -0.0 contributes +0.0 (it is added to 0.0)."""
    v = np.array([1e16, 1.0, -1e16, 1.0])
    assert km.chunked_sum(v, 1) == 1.0 and km.chunked_sum(v, 2) == 0.0 and km.chunked_sum(v, 4) == 1.0
    assert km.exact_sum(v) == 2.0
    assert bits(km.chunked_sum(np.array([-0.0]), 1)) == bits(0.0)
    assert [km.isie(t, 3, 10) for t in range(3)] == [(0, 4), (4, 7), (7, 10)]
    assert km.chunked_sum(np.arange(5.0), 8) == 10.0            # more chunks than terms: the empty ones add 0.0
    assert np.array_equal(km.rank_fold([1e16, 1.0, -1e16, 1.0], 4, 1), [1.0])
    assert np.array_equal(km.rank_fold([1.0, 1e16, 1.0, -1e16], 2, 2), [2.0, 0.0])
    eight = np.tile([1e16, 1.0, -1e16, 1.0], 2)                # rank order gives 1.0; from the last rank down, 0.0
    assert km.rank_fold(eight, 8, 1)[0] == 1.0 and km.rank_fold(eight[::-1].copy(), 8, 1)[0] == 0.0
