/*
 * lis_shift.c -- lis_matrix_shift_diagonal(A, sigma): A <- A - sigma I (reference src/matrix/lis_matrix_ops.c:781-829 and the
 * per-format routines it dispatches to).  The one matrix operation every eigensolver calls (eshift, lis_eloop.h): once around a whole solve
 * for -shift, twice per iteration for the Rayleigh quotient iteration.  Its generalized form, lis_matrix_shift_matrix(A, B, sigma):
 * A <- A - sigma B (lis_matrix_ops.c:833-856), stands in the second half of this file.
 *
 * Semantics are the reference's, format by format (restated, not copied):
 *   CSR  lis_matrix_csr.c:566   the FIRST stored entry of row i whose column is i; a row without one is left alone
 *   CSC  lis_matrix_csc.c:299   the same per column, over the np columns
 *   ELL  lis_matrix_ell.c:634   the first slot j with index[j n + i] == i (padding carries index i: a row without a diagonal entry gets -sigma in its first padding slot)
 *   DIA  lis_matrix_dia.c:371   every row of the first stored diagonal with offset 0 (the serial branch, :414-421: value[j n + i]); without one, the reference walks off the
 *                               end of index[]; here nothing is shifted
 *   JAD  lis_matrix_jad.c:490   entries with index == row[position] in jagged-diagonal order until n of them were found (one chunk: the serial branch)
 *   BSR  lis_matrix_bsr.c:748   the diagonal entries of the blocks that cover rows i .. of each block row, the first covering block first
 *   COO  lis_matrix_coo.c:357   EVERY stored entry with row == col, duplicates each
 *   DNS  lis_matrix_dns.c:244   value[i n + i], every row
 *   VBR  lis_matrix_vbr.c:937   the entries the reference's diagonal search finds: the diagonal where all blocks have one size, other entries or none on variable blocks
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
 *   VBR (copy in HBM)           one launch on the copy's value[] (kernels/vbr.hip), the host arrays edited inside the same bracket; the transposed copy comes back on its next use
 *   the other seven formats     the host arrays are edited as above and the HBM copy is dropped (what lis_amd_matrix_host_modified does): the next product uploads.
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
	case LIS_MATRIX_COO:        /* ref lis_matrix_coo.c:377-383: every stored (i,i), duplicates each */
		for (LIS_INT k = 0; k < A->nnz; k++) if (A->row[k] == A->col[k]) A->value[k] -= sigma;
		break;
	case LIS_MATRIX_DNS:        /* ref lis_matrix_dns.c:268-271: value[i*n + i] */
		for (LIS_INT i = 0; i < n; i++) A->value[(size_t)i * n + i] -= sigma;
		break;
	case LIS_MATRIX_VBR: {      /* ref lis_matrix_vbr.c:969-989: the entries its diagonal search finds (lisi_vbr_diagonal_walk) */
		const lisi_vbr_diag_t w = {NULL, sigma};
		lisi_vbr_diagonal_walk(A, &w);
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
	if (d->ready && A->matrix_type == LIS_MATRIX_VBR && d->type == LIS_MATRIX_VBR && d->value && d->row) {
		/* VBR: one launch on the copy's value[] (the search of shift_host, entry for entry), the same edit on the host arrays inside the edit bracket */
		LISCHK(lisp_fill_matrix(A));
		HIPCHK(liship_vbr_shift_diagonal_f64(A->n, d->nr, d->row, d->col, d->ptr, d->bptr, d->bindex, d->value, sigma, lisg.stream));
		LISCHK(lisd_mat_values_changed(A));
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

/* ================================================================== lis_matrix_shift_matrix(A, B, sigma): A <- A - sigma B
 * The reference goes through two dense n x n copies (src/matrix/lis_matrix_ops.c:833-856: csr -> dns, lis_matrix_axpy_dns, dns -> csr), which no pencil of
 * any interesting size survives.  What that route leaves in A -- the union of the two patterns row by row in ascending column order, every entry
 * (-sigma) * b + a in two roundings, exact zeros dropped, A's storage type kept -- is formed here by kernels/spgeam.hip on the HBM copies of a CSR A and a
 * CSR B, one rank; no matrix array crosses the bus.
 *   in place   one launch updates the rows that keep their layout where they lie and counts the others in a flag, which the host reads once.  No other row:
 *              done -- the copy's value[] changed, lisd_mat_values_changed makes the plan again.
 *   rebuilt    otherwise the rows the launch left alone are merged into three new arrays (scan, fill; the rows it did update are copied), which replace the
 *              copy's; A->nnz follows.
 * Either way A's HOST arrays are bound anew to the copy's buffers, lazily, as lis_convert_hbm.c binds those of a converted matrix (lisp_alloc_lazy): a
 * program that reads A->ptr / index / value sees the reference's arrays, brought home on that first touch, and one that only multiplies never pays for them.
 * (Where the page-fault handler is not available -- eager coherence -- they are copied home at once.)  A matrix that lives in HBM only has none.
 * A in another served storage goes X -> CSR -> shift -> X through lis_matrix_convert; a B in another storage is read from a CSR temporary.
 * Refused: a split A or B (a preconditioner that splits the matrix holds parts that would not follow), several ranks, ghost columns. */
static struct { LIS_INT in_place, nnz_before, nnz_after; } last_shift;

LIS_INT lis_amd_last_shift_matrix(LIS_INT info[3])
{
	if (!info) return LISI_ERR(LIS_ERR_ILL_ARG, "info is NULL\n");
	info[0] = last_shift.in_place; info[1] = last_shift.nnz_before; info[2] = last_shift.nnz_after;
	return LIS_SUCCESS;
}

LIS_INT lis_amd_matrix_device_csr(LIS_MATRIX A, LIS_INT **dptr, LIS_INT **dindex, LIS_SCALAR **dvalue)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisd_mat_ready(A));
	const lisd_mat *d = MDEV(A);
	if (A->matrix_type != LIS_MATRIX_CSR || d->type != LIS_MATRIX_CSR || A->is_splited || !d->ptr) return LISI_ERR(LIS_ERR_ILL_ARG, "the HBM copy of matrix A is not a CSR matrix\n");
	if (dptr) *dptr = d->ptr;
	if (dindex) *dindex = d->index;
	if (dvalue) *dvalue = d->value;
	return LIS_SUCCESS;
}

/* A's host arrays let go (freed where the matrix owns them, the caller's again where it does not) */
static void host_arrays_drop(LIS_MATRIX A)
{
	if (A->is_destroy) {
		if (!lisp_free_array(A->ptr)) free(A->ptr);
		if (!lisp_free_array(A->index)) free(A->index);
		if (!lisp_free_array(A->value)) free(A->value);
	} else lisp_matrix_release(A, 1);
	A->ptr = NULL; A->index = NULL; A->value = NULL;
}

/* ... and made anew from the copy's buffers: address space bound to them, or (no handler) plain memory filled now */
static LIS_INT host_arrays_bind(LIS_MATRIX A)
{
	lisd_mat *d = MDEV(A);
	const size_t bytes[3] = {sizeof(int) * ((size_t)d->n + 1), sizeof(int) * (size_t)d->nnz, sizeof(double) * (size_t)d->nnz};
	void *dev[3] = {d->ptr, d->index, d->value}, *h[3] = {NULL, NULL, NULL};
	int lazy = lisp_lazy();
	for (int k = 0; k < 3 && lazy; k++) if (!(h[k] = lisp_alloc_lazy(A, bytes[k], dev[k], 0))) lazy = 0;
	if (!lazy) {
		for (int k = 0; k < 3; k++) { if (h[k]) (void)lisp_free_array(h[k]); h[k] = malloc(bytes[k] ? bytes[k] : 1); }
		if (!h[0] || !h[1] || !h[2]) { free(h[0]); free(h[1]); free(h[2]); return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)bytes[2]); }
		for (int k = 0; k < 3; k++) if (bytes[k]) HIPCHK(liship_memcpy_d2h(h[k], dev[k], bytes[k], lisg.stream));
		HIPCHK(liship_stream_synchronize(lisg.stream));
	}
	A->ptr = (LIS_INT *)h[0]; A->index = (LIS_INT *)h[1]; A->value = (LIS_SCALAR *)h[2];
	A->is_destroy = LIS_TRUE;                 /* the library's arrays from here on */
	d->checked = 0;                           /* (LIS_AMD_MATRIX_CHECK hashes host arrays an upload was made from) */
	return LIS_SUCCESS;
}

/* A and B in CSR storage, their copies in HBM */
static LIS_INT shift_matrix_csr(LIS_MATRIX A, LIS_MATRIX B, LIS_SCALAR sigma)
{
	LISCHK(lisd_mat_ready(A));
	LISCHK(lisd_mat_ready(B));
	lisd_mat *d = MDEV(A);
	const lisd_mat *bd = MDEV(B);
	if (d->type != LIS_MATRIX_CSR || bd->type != LIS_MATRIX_CSR || d->split_jad || bd->split_jad || !d->ptr || !bd->ptr)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_matrix_shift_matrix: the HBM copies of A and B are not both CSR matrices\n");
	const int n = d->n, nnz0 = d->nnz;
	/* (A == B is served: the kernels read an entry of B before they write the entry of A on its column, and nothing reads B once A's arrays are replaced)
	 * work in HBM: count[n], done[n], the flag, the scan's scratch */
	int *work = NULL, *nptr = NULL, *nidx = NULL, flag = 0, nnz1 = 0;
	double *nval = NULL;
	const size_t ints = 2 * (size_t)n + 2, work_bytes = sizeof(int) * ints + sizeof(long long) * ((size_t)n / 4096 + 2);
	LISCHK(lisd_pool_get(work_bytes, (void **)&work));
	int *count = work, *done = work + n, *dflag = work + 2 * (size_t)n;
	long long *scratch = (long long *)(work + ints);
	LIS_INT err = LIS_SUCCESS;
	int rc = liship_csr_shift_matrix_try_f64(n, d->ptr, d->index, d->value, bd->ptr, bd->index, bd->value, sigma, count, done, dflag, lisg.stream);
	if (!rc) rc = liship_memcpy_d2h(&flag, dflag, sizeof(int), lisg.stream);
	if (!rc) rc = liship_stream_synchronize(lisg.stream);
	if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	if (!err && flag) {
		rc = lisd_malloc((void **)&nptr, sizeof(int) * ((size_t)n + 1));
		if (!rc) rc = liship_csr_shift_matrix_scan(n, count, nptr, scratch, &nnz1, lisg.stream);
		if (!rc) rc = lisd_malloc((void **)&nidx, sizeof(int) * (size_t)(nnz1 > 0 ? nnz1 : 1));
		if (!rc) rc = lisd_malloc((void **)&nval, sizeof(double) * (size_t)(nnz1 > 0 ? nnz1 : 1));
		if (!rc) rc = liship_csr_shift_matrix_fill_f64(n, d->ptr, d->index, d->value, bd->ptr, bd->index, bd->value, sigma, done, nptr, nidx, nval, lisg.stream);
		if (!rc) rc = liship_stream_synchronize(lisg.stream);
		if (rc) { (void)liship_free(nptr); (void)liship_free(nidx); (void)liship_free(nval); err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	}
	lisd_pool_put(work, work_bytes);
	if (err) return err;                       /* (a failing HIP call is fatal for the operation: rows may have been updated already) */
	/* the host arrays let go BEFORE the buffers they may be bound to are replaced */
	if (!d->device_only) host_arrays_drop(A);
	if (flag) {
		(void)liship_free(d->ptr); (void)liship_free(d->index); (void)liship_free(d->value);
		d->ptr = nptr; d->index = nidx; d->value = nval;
		d->nnz = nnz1; A->nnz = nnz1;
	}
	d->host_written = 0;
	last_shift.in_place = flag ? 0 : 1; last_shift.nnz_before = nnz0; last_shift.nnz_after = flag ? nnz1 : nnz0;
	LISCHK(lisd_mat_values_changed(A));
	if (!d->device_only) LISCHK(host_arrays_bind(A));
	return LIS_SUCCESS;
}

/* a CSR view of B for the kernels: B itself, or a temporary made by lis_matrix_convert (*tmp, the caller destroys it) */
static LIS_INT csr_view(LIS_MATRIX B, LIS_MATRIX *view, LIS_MATRIX *tmp)
{
	*tmp = NULL; *view = B;
	if (B->matrix_type == LIS_MATRIX_CSR) return LIS_SUCCESS;
	LISCHK(lis_matrix_duplicate(B, tmp));
	LIS_INT err = lis_matrix_set_type(*tmp, LIS_MATRIX_CSR);
	if (!err) err = lis_matrix_convert(B, *tmp);
	if (err) { lis_matrix_destroy(*tmp); *tmp = NULL; return err; }
	*view = *tmp;
	return LIS_SUCCESS;
}

LIS_INT lis_matrix_shift_matrix(LIS_MATRIX A, LIS_MATRIX B, LIS_SCALAR sigma)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisi_matrix_check(B, LISI_CHECK_ASSEMBLED));
	if (A->n != B->n || A->gn != B->gn) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A (n = %D) and matrix B (n = %D) differ in size\n", A->n, B->n);
	if (lisi_format_one_rank(A->matrix_type) || lisi_format_one_rank(B->matrix_type))      /* (a COO copy looks like CSR in HBM: the gate reads the matrix, not the copy) */
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_matrix_shift_matrix: %s storage is not shifted by a matrix -- convert to one of CSR, CSC, DIA, ELL, JAD, BSR first (A and B are untouched)\n",
		                lisi_format_name(lisi_format_one_rank(A->matrix_type) ? A->matrix_type : B->matrix_type));
	if (!lisi_format_swept(A->matrix_type) || !lisi_format_swept(B->matrix_type))
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "storage format %D is not served by liblis_amd\n", lisi_format_swept(A->matrix_type) ? B->matrix_type : A->matrix_type);
	if (lisg.nprocs > 1 || A->nprocs > 1 || A->np != A->n || B->np != B->n)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_matrix_shift_matrix is served on one rank (this job has %D)\n", (LIS_INT)lisg.nprocs);
	if (A->is_splited || B->is_splited) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_matrix_shift_matrix: a split matrix (lis_matrix_split, -p ssor | ilu | is ...) is not shifted by a matrix\n");
	if (A->matrix_type == LIS_MATRIX_BSR && A->bnr != A->bnc) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "lis_matrix_shift_matrix: BSR blocks of %D x %D are not square\n", A->bnr, A->bnc);
	lisd_mat *d = MDEV(A);
	if (d->solve_holds) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is held by a running solve\n");
	if (d->device_only && A->matrix_type != LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "a matrix that lives in HBM only is shifted in CSR storage\n");
	LISCHK(lisd_init());
	LIS_MATRIX Bcsr, Btmp;
	LISCHK(csr_view(B, &Bcsr, &Btmp));
	/* A in another storage: X -> CSR -> shift -> X (what the reference's dns -> X does to the same entries) */
	const LIS_INT type = A->matrix_type, block = A->matrix_type == LIS_MATRIX_BSR ? A->bnr : 0;
	LIS_INT err = lisi_matrix_retype(A, LIS_MATRIX_CSR, 0);
	if (!err) err = shift_matrix_csr(A, Bcsr, sigma);
	if (!err) err = lisi_matrix_retype(A, type, block);
	if (Btmp) lis_matrix_destroy(Btmp);
	return err;
}
