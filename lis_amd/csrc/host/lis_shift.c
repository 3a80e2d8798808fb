/*
 * lis_shift.c -- lis_matrix_shift_diagonal(A, sigma): A <- A - sigma I (reference src/matrix/lis_matrix_ops.c:781-829 and the
 * per-format routines it dispatches to).  The one matrix operation every eigensolver calls (lis_esolver.c): once around a whole solve
 * for -shift, twice per iteration for the Rayleigh quotient iteration.
 *
 * Semantics are the reference's, format by format (restated, not copied):
 *   CSR  lis_matrix_csr.c:566   the FIRST stored entry of row i whose column is i; a row without one is left alone
 *   CSC  lis_matrix_csc.c:299   the same per column, over the np columns
 *   ELL  lis_matrix_ell.c:634   the first slot j with index[j n + i] == i (padding carries index i: a row without a diagonal entry gets -sigma in its first padding slot)
 *   DIA  lis_matrix_dia.c:371   every row of the first stored diagonal with offset 0 (the serial branch, :414-421: value[j n + i]); without one, the reference walks off the
 *                               end of index[]; here nothing is shifted
 *   JAD  lis_matrix_jad.c:490   entries with index == row[position] in jagged-diagonal order until n of them were found (one chunk: the serial branch)
 *   BSR  lis_matrix_bsr.c:748   the diagonal entries of the blocks that cover rows i .. of each block row, the first covering block first
 * A split matrix (is_splited) shifts A->D only (for BSR the diagonals of its blocks), every row, whether the row had a diagonal entry or not.
 * value -= sigma rounds: shift(s) then shift(-s) does not give the bits back.  The reference has that drift and so has this library.
 *
 * Where the work happens:
 *   no HBM copy yet             the host arrays are edited; nothing else to do
 *   CSR with an HBM copy        (split or not, host-backed or living in HBM only) kernels/eigen.hip edits the copy's own value[] in place -- a split matrix's chain rows
 *                               start with their diagonal term (lis_split.c), so the same kernel serves both -- and lisd_mat_values_changed (lis_upload.c) drops what
 *                               was derived from the old values and makes the plan again from the HBM arrays.  The host arrays, where they exist, get the same edit on
 *                               the host inside lisd_mat_host_edit_begin / _end, so that the write watch (lis_pages.c) does not take it for the program's and throw the
 *                               copy away.  No matrix array crosses the bus.  The plan rebuild costs 10 ms per shift at 256^3, the host edit ~300 ms.
 *   the other five formats      the host arrays are edited as above and the HBM copy is dropped (what lis_amd_matrix_host_modified does): the next product uploads.
 *   HBM-only and not CSR        refused (such a matrix has no host arrays to edit).
 */
#include "lis_internal.h"

static void shift_host(LIS_MATRIX A, LIS_SCALAR sigma)
{
	const LIS_INT n = A->n;
	if (A->is_splited) {
		if (A->matrix_type == LIS_MATRIX_BSR) {
			const LIS_INT bnr = A->bnr, bs = A->bnr * A->bnc;
			for (LIS_INT i = 0; i < A->nr; i++)
				for (LIS_INT j = 0; j < bnr; j++) A->D->value[(size_t)i * bs + (size_t)j * bnr + j] -= sigma;
		} else for (LIS_INT i = 0; i < n; i++) A->D->value[i] -= sigma;
		return;
	}
	switch (A->matrix_type) {
	case LIS_MATRIX_CSR: case LIS_MATRIX_CSC: {
		const LIS_INT lines = A->matrix_type == LIS_MATRIX_CSR ? n : A->np;
		for (LIS_INT i = 0; i < lines; i++)
			for (LIS_INT j = A->ptr[i]; j < A->ptr[i + 1]; j++) if (A->index[j] == i) { A->value[j] -= sigma; break; }
		break; }
	case LIS_MATRIX_ELL:
		for (LIS_INT i = 0; i < n; i++)
			for (LIS_INT j = 0; j < A->maxnzr; j++) if (A->index[(size_t)j * n + i] == i) { A->value[(size_t)j * n + i] -= sigma; break; }
		break;
	case LIS_MATRIX_DIA:
		for (LIS_INT j = 0; j < A->nnd; j++) if (A->index[j] == 0) {
			for (LIS_INT i = 0; i < n; i++) A->value[(size_t)j * n + i] -= sigma;
			break;
		}
		break;
	case LIS_MATRIX_JAD: {
		LIS_INT k = n;
		for (LIS_INT j = 0; j < A->maxnzr && k > 0; j++) {
			LIS_INT l = 0;
			for (LIS_INT i = A->ptr[j]; i < A->ptr[j + 1]; i++, l++)
				if (A->row[l] == A->index[i]) { A->value[i] -= sigma; if (--k == 0) break; }
		}
		break; }
	case LIS_MATRIX_BSR: {
		const LIS_INT bnr = A->bnr, bnc = A->bnc, bs = bnr * bnc;
		for (LIS_INT bi = 0; bi < A->nr; bi++) {
			LIS_INT k = 0, i = bi * bnr;
			for (LIS_INT bj = A->bptr[bi]; bj < A->bptr[bi + 1]; bj++) {
				const LIS_INT bjj = A->bindex[bj];
				if (i >= bjj * bnc && i < (bjj + 1) * bnc)
					for (LIS_INT j = i % bnc; j < bnc && k < bnr && i < n; j++) { A->value[(size_t)bj * bs + (size_t)j * bnr + k] -= sigma; i++; k++; }
				if (k == bnr) break;
			}
		}
		break; }
	default: break;
	}
}

LIS_INT lis_matrix_shift_diagonal(LIS_MATRIX A, LIS_SCALAR sigma)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (!lisi_format_served(A->matrix_type)) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "storage format %D is not served by liblis_amd\n", A->matrix_type);
	lisd_mat *d = MDEV(A);
	if (d->device_only && !(A->matrix_type == LIS_MATRIX_CSR && d->type == LIS_MATRIX_CSR))
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "a matrix that lives in HBM only is shifted in CSR storage\n");
	if (d->solve_holds) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is held by a running solve\n");
	/* a host write the watch has seen already: that copy is stale whatever happens here */
	if (d->ready && !d->device_only && d->host_written) lisd_mat_free(A);
	const int in_hbm = d->ready && A->matrix_type == LIS_MATRIX_CSR && d->type == LIS_MATRIX_CSR && !d->split_jad && d->ptr && d->value;
	if (in_hbm) {
		if (!d->device_only) LISCHK(lisp_fill_matrix(A));     /* (host arrays still held in HBM come home BEFORE the edit, so that they get it exactly once; no conversion leaves a CSR matrix's there today) */
		HIPCHK(liship_csr_shift_diagonal_f64(d->n, d->ptr, d->index, d->value, sigma, lisg.stream));
		LISCHK(lisd_mat_values_changed(A));
		if (d->device_only) return LIS_SUCCESS;
		lisd_mat_host_edit_begin(A);
		shift_host(A, sigma);
		lisd_mat_host_edit_end(A);
		return LIS_SUCCESS;
	}
	LISCHK(lisp_fill_matrix(A));
	if (d->ready) lisd_mat_free(A);           /* the copy holds the old values (and opens the watched arrays for the edit) */
	shift_host(A, sigma);
	return LIS_SUCCESS;
}
