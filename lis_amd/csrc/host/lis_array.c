/*
 * lis_array.c -- the small dense routines the Lanczos and Arnoldi eigensolvers call (reference src/array/lis_array.c), public as there:
 * lis_array_nrm2 (:366-382), lis_array_cgs (:1029-1080), lis_array_qr (:1136-1175).  Host routines on host arrays, column-major n x n, restated
 * operation for operation (every product and every sum rounded once: the file is compiled without FMA contraction); they need no device.
 */
#include "lis_internal.h"

LIS_INT lis_array_nrm2(LIS_INT n, LIS_SCALAR *x, LIS_REAL *value)
{
	LIS_SCALAR t = 0.0;
	for (LIS_INT i = 0; i < n; i++) t += x[i] * x[i];
	*value = sqrt(t);
	return LIS_SUCCESS;
}

/* classical Gram-Schmidt: A = Q R, column by column; a column whose remainder is shorter than 1e-12 ends the factorisation (the later columns of Q and R stay 0) */
LIS_INT lis_array_cgs(LIS_INT n, LIS_SCALAR *a, LIS_SCALAR *q, LIS_SCALAR *r)
{
	const LIS_REAL tol = 1e-12;
	LIS_REAL nrm2;
	LIS_SCALAR *a_k = (LIS_SCALAR *)malloc((size_t)(n > 0 ? n : 1) * sizeof(LIS_SCALAR));
	if (!a_k) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(n * sizeof(LIS_SCALAR)));
	for (LIS_INT i = 0; i < n * n; i++) { q[i] = 0.0; r[i] = 0.0; }
	for (LIS_INT k = 0; k < n; k++) {
		for (LIS_INT i = 0; i < n; i++) a_k[i] = a[i + k * n];
		for (LIS_INT j = 0; j < k; j++) {
			r[j + k * n] = 0;
			for (LIS_INT i = 0; i < n; i++) r[j + k * n] += q[i + j * n] * a[i + k * n];
			for (LIS_INT i = 0; i < n; i++) a_k[i] -= r[j + k * n] * q[i + j * n];
		}
		lis_array_nrm2(n, a_k, &nrm2);
		r[k + k * n] = nrm2;
		if (nrm2 < tol) break;
		for (LIS_INT i = 0; i < n; i++) q[i + k * n] = a_k[i] / nrm2;
	}
	free(a_k);
	return LIS_SUCCESS;
}

/* the unshifted QR iteration: factor, A <- R Q, until the first subdiagonal entry |a[1]| is below 1e-12, 100000 sweeps at most.  The reference reads a[1]
 * of a 1 x 1 matrix too, one element past the array; here a 1 x 1 matrix has no subdiagonal and its error is 0 after the one sweep */
LIS_INT lis_array_qr(LIS_INT n, LIS_SCALAR *a, LIS_SCALAR *q, LIS_SCALAR *r, LIS_INT *qriter, LIS_REAL *qrerr)
{
	const LIS_INT maxiter = 100000;
	const LIS_REAL tol = 1e-12;
	LIS_REAL err = 0.0;
	LIS_INT iter = 0;
	while (iter < maxiter) {
		iter = iter + 1;
		LISCHK(lis_array_cgs(n, a, q, r));
		for (LIS_INT j = 0; j < n; j++)
			for (LIS_INT i = 0; i < n; i++) {
				a[i + j * n] = 0;
				for (LIS_INT k = 0; k < n; k++) a[i + j * n] += r[i + k * n] * q[k + j * n];
			}
		err = n > 1 ? fabs(a[1]) : 0.0;
		if (err < tol) break;
	}
	*qriter = iter;
	*qrerr = err;
	return LIS_SUCCESS;
}
