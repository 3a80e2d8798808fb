/*
 * lis_convert_hbm.c -- conversions in HBM (kernels/convert.hip).
 *
 * lis_matrix_convert(Ain, Aout) with Ain = a CSR matrix whose HBM copy exists: the target layout (ELL, DIA, CSC, JAD, BSR, COO or DNS) is built FROM that copy by kernels --
 * the arrays the host routines of lis_convert.c build, bit for bit -- and becomes both Aout's HBM copy and the source of Aout's HOST
 * arrays.  Those the Lis API promises (A->index, A->value ...), but a program that only multiplies never reads them: they get address
 * space without access (lis_pages.c), bound to the device buffer that holds their contents, and come home on their first touch.
 * What the product of the new matrix runs on is decided by the code mat_upload decides it with (lis_upload.c: lisd_row_form_wanted,
 * lisd_row_form_adopt, lisd_try_bsr_row_form, lisd_ell_index_codes, lisd_fmt_find_plane): the constant-coefficient row form (value
 * records) for ELL / DIA / BSR where the values allow it, CSC, JAD and COO as CSR rows in the reference's summation order, else the native arrays (DNS always).
 *
 * lisd_convert_csr is a gate, one builder per target and a tail.  A builder allocates through the context's scope (TMP) and releases a buffer when d or a lazy host
 * array takes it; it returns wherever it likes, and the gate frees what is left in the scope -- after a failure also the lazy arrays and what d holds. */
#include "lis_internal.h"

/* what only the COO and DNS builders call is referenced weakly: tests/c/upload_cases.c links this file against stubs of the calls the five older builders make, and
 * the library always holds the real ones */
extern int liship_csr_to_coo(int n, const int *ptr, int *row, void *stream) __attribute__((weak));
extern int liship_csr_to_dns_f64(int n, int np, const int *ptr, const int *index, const double *value, double *dns, void *stream) __attribute__((weak));
extern LIS_INT lis_matrix_set_coo(LIS_INT nnz, LIS_INT *row, LIS_INT *col, LIS_SCALAR *value, LIS_MATRIX A) __attribute__((weak));
extern LIS_INT lis_matrix_set_dns(LIS_SCALAR *value, LIS_MATRIX A) __attribute__((weak));

#define CONV_TMP 16
typedef struct {
	LIS_MATRIX Ain, Aout;
	const lisd_mat *sd;                /* the source's copy: CSR */
	lisd_mat *d;                       /* the target's, empty but for n, np, nnz */
	int n, np, nnz, maxlen;
	void *tmp[CONV_TMP]; int ntmp;     /* device buffers that are nobody's yet */
	void *lazy[3]; int nlazy;          /* Aout's host arrays made so far */
	void *heap[2];                     /* host memory that becomes Aout's with lis_matrix_set_<fmt> (JAD: row order, diagonal starts) */
} conv_t;

static int tmp_alloc(conv_t *c, void **out, size_t bytes)           /* HIP code, as lisd_malloc */
{
	if (c->ntmp == CONV_TMP) return LISHIP_ERR_ARG;
	const int rc = lisd_malloc(out, bytes);
	if (!rc) c->tmp[c->ntmp++] = *out;
	return rc;
}
#define TMP(p, count) HIPCHK(tmp_alloc(c, (void **)&(p), sizeof(*(p)) * (size_t)(count)))
static void *tmp_release(conv_t *c, void *p)                        /* p has an owner now */
{
	for (int i = 0; i < c->ntmp; i++) if (c->tmp[i] == p) c->tmp[i] = NULL;
	return p;
}
static void tmp_free(conv_t *c, void *p) { (void)liship_free(tmp_release(c, p)); }
static void tmp_unwind(conv_t *c, int mark)                         /* frees what was allocated since ntmp was `mark` and is still in the scope */
{
	for (int i = mark; i < c->ntmp; i++) if (c->tmp[i]) (void)liship_free(c->tmp[i]);
	c->ntmp = mark;
}

/* the next host array of Aout: address space bound to `dev`.  own: the pages own the buffer from here on (it leaves the scope; with the row form the native
 * arrays only back the host arrays and go when those have been read or the matrix dies), else the buffer is d's.  After a failure the gate undoes the set:
 * pages that were made are unmapped (freeing a buffer they own), a buffer whose pages were not made is still in the scope, or d's */
static LIS_INT lazy_bind(conv_t *c, size_t bytes, void *dev, int own)
{
	void *h = lisp_alloc_lazy(c->Aout, bytes, dev, own);
	if (!h) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "convert: address space\n");
	if (own) (void)tmp_release(c, dev);
	c->lazy[c->nlazy++] = h;
	return LIS_SUCCESS;
}

static int device_few_distinct_values(const double *dval, size_t count)
{
	double head[4096];
	const size_t take = count < 4096 ? count : 4096;
	if (take == 0 || liship_memcpy_d2h(head, dval, take * sizeof(double), lisg.stream) || liship_stream_synchronize(lisg.stream)) return 0;
	return lisd_few_distinct_values(head, take);
}

/* the three HBM arrays of a row form leave the scope: kept in d with their plan, or freed (lis_upload.c) */
#define ROW_FORM_ADOPT(rptr, ridx, rval, nnz, taken) lisd_row_form_adopt(c->d, c->n, (int *)tmp_release(c, rptr), (int *)tmp_release(c, ridx), (double *)tmp_release(c, rval), nnz, taken)

/* d gets the source's own rows */
static LIS_INT clone_csr(const lisd_mat *sd, lisd_mat *d, int n, int nnz)
{
	HIPCHK(lisd_malloc((void **)&d->ptr, sizeof(int) * ((size_t)n + 1)));
	HIPCHK(lisd_malloc((void **)&d->index, sizeof(int) * (size_t)nnz));
	HIPCHK(lisd_malloc((void **)&d->value, sizeof(double) * (size_t)nnz));
	HIPCHK(liship_memcpy_d2d(d->ptr, sd->ptr, sizeof(int) * ((size_t)n + 1), lisg.stream));
	HIPCHK(liship_memcpy_d2d(d->index, sd->index, sizeof(int) * (size_t)nnz, lisg.stream));
	HIPCHK(liship_memcpy_d2d(d->value, sd->value, sizeof(double) * (size_t)nnz, lisg.stream));
	d->type = LIS_MATRIX_CSR;
	return LIS_SUCCESS;
}

/* ---- ELL */
static LIS_INT ell_row_form(conv_t *c, int maxnzr, size_t slots, int *taken)
{
	const int mark = c->ntmp;
	int *rptr = NULL, *ridx = NULL; double *rval = NULL;
	if (tmp_alloc(c, (void **)&rptr, sizeof(int) * ((size_t)c->n + 1)) || tmp_alloc(c, (void **)&ridx, sizeof(int) * slots) || tmp_alloc(c, (void **)&rval, sizeof(double) * slots)) {
		tmp_unwind(c, mark);                                  /* an optimisation: out of memory on the way is not an error */
		return LIS_SUCCESS;
	}
	HIPCHK(liship_csr_to_ell_rows(c->n, maxnzr, c->sd->ptr, c->sd->index, c->sd->value, rptr, ridx, rval, lisg.stream));
	return ROW_FORM_ADOPT(rptr, ridx, rval, (LIS_INT)slots, taken);
}

static LIS_INT build_ell(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const int n = c->n, maxnzr = c->maxlen;
	if ((long long)n * maxnzr >= 0x7fffffffLL) return LIS_SUCCESS;
	const size_t slots = (size_t)n * (size_t)maxnzr;
	int *eidx = NULL, rowform = 0; double *eval = NULL;
	TMP(eidx, slots ? slots : 1); TMP(eval, slots ? slots : 1);
	HIPCHK(liship_csr_to_ell(n, maxnzr, c->sd->ptr, c->sd->index, c->sd->value, eidx, eval, lisg.stream));
	if (lisd_row_form_wanted(maxnzr, n) && device_few_distinct_values(c->sd->value, (size_t)c->nnz)) LISCHK(ell_row_form(c, maxnzr, slots, &rowform));
	d->maxnzr = maxnzr;
	if (!rowform) {
		d->type = LIS_MATRIX_ELL; d->index = (int *)tmp_release(c, eidx); d->value = (double *)tmp_release(c, eval);
		LISCHK(lisd_ell_index_codes(d));
		lisd_fmt_find_plane(d, NULL);
	}
	LISCHK(lazy_bind(c, sizeof(int) * slots, eidx, rowform)); LISCHK(lazy_bind(c, sizeof(double) * slots, eval, rowform));
	*built = 1;
	return lis_matrix_set_ell(maxnzr, (LIS_INT *)c->lazy[0], (LIS_SCALAR *)c->lazy[1], c->Aout);
}

/* ---- DIA (rows in ascending column order: csr2dia would sort them in place otherwise -- the host routine does that) */
static LIS_INT dia_row_form(conv_t *c, int nnd, const int *offs, const double *dval, long long *scratch, int *taken)
{
	const int n = c->n, mark = c->ntmp;
	int *count = NULL, *rptr = NULL, *ridx = NULL, rnnz = 0; double *rval = NULL;
	if (tmp_alloc(c, (void **)&count, sizeof(int) * (size_t)n) || tmp_alloc(c, (void **)&rptr, sizeof(int) * ((size_t)n + 1)) ||
	    liship_dia_row_counts(n, c->np, nnd, offs, count, rptr, scratch, &rnnz, lisg.stream) || rnnz <= 0 ||
	    tmp_alloc(c, (void **)&ridx, sizeof(int) * (size_t)rnnz) || tmp_alloc(c, (void **)&rval, sizeof(double) * (size_t)rnnz) ||
	    liship_dia_to_rows(n, c->np, nnd, offs, dval, rptr, ridx, rval, lisg.stream)) {
		tmp_unwind(c, mark);                                  /* an optimisation: whatever refuses on the way leaves the native form */
		return LIS_SUCCESS;
	}
	const LIS_INT err = ROW_FORM_ADOPT(rptr, ridx, rval, rnnz, taken);
	tmp_free(c, count);
	return err;
}

static LIS_INT build_dia(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const int n = c->n, np = c->np, span = n + np;
	int *used = NULL, *slot = NULL, *offs = NULL, nnd = 0, rowform = 0; long long *scratch = NULL; double *dval = NULL;
	TMP(used, span); TMP(slot, (size_t)span + 1); TMP(scratch, span / 4096 + 4);
	HIPCHK(liship_csr_dia_offsets(n, np, sd->ptr, sd->index, used, slot, scratch, &nnd, lisg.stream));
	if (nnd <= 0 || (long long)n * nnd >= 0x7fffffffLL) return LIS_SUCCESS;
	TMP(offs, nnd); TMP(dval, (size_t)n * (size_t)nnd);
	HIPCHK(liship_csr_to_dia(n, np, nnd, sd->ptr, sd->index, sd->value, used, slot, offs, dval, lisg.stream));
	(void)liship_stream_synchronize(lisg.stream);
	tmp_free(c, used); tmp_free(c, slot);
	if (lisd_row_form_wanted(nnd, n) && device_few_distinct_values(sd->value, (size_t)c->nnz)) LISCHK(dia_row_form(c, nnd, offs, dval, scratch, &rowform));
	tmp_free(c, scratch);
	d->nnd = nnd;
	if (!rowform) {
		int hoffs[4096];
		d->type = LIS_MATRIX_DIA; d->index = (int *)tmp_release(c, offs); d->value = (double *)tmp_release(c, dval);
		if (nnd <= 4096 && liship_memcpy_d2h(hoffs, offs, sizeof(int) * (size_t)nnd, lisg.stream) == 0 && liship_stream_synchronize(lisg.stream) == 0) lisd_fmt_find_plane(d, hoffs);
	}
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)nnd, offs, rowform)); LISCHK(lazy_bind(c, sizeof(double) * (size_t)n * (size_t)nnd, dval, rowform));
	*built = 1;
	return lis_matrix_set_dia(nnd, (LIS_INT *)c->lazy[0], (LIS_SCALAR *)c->lazy[1], c->Aout);
}

/* ---- CSC.  The host arrays: A^T row by row = A column by column, rows ascending inside a column (transpose.hip); the product's arrays: A's
 * own rows, which ARE in ascending column order here -- the order the reference's serial CSC sweep adds them in (lis_matvec_csc.c:128-144) */
static LIS_INT build_csc(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const int n = c->n, np = c->np, nnz = c->nnz;
	int *tptr = NULL, *tidx = NULL, *work = NULL; double *tval = NULL;
	TMP(tptr, (size_t)np + 1); TMP(tidx, nnz); TMP(tval, nnz); TMP(work, (size_t)np + (size_t)nnz + 4);      /* (work: as lis_matvech.c sizes it) */
	HIPCHK(liship_csr_transpose_f64(n, np, nnz, sd->ptr, sd->index, sd->value, tptr, tidx, tval, work, lisg.stream));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	tmp_free(c, work);
	LISCHK(clone_csr(sd, d, n, nnz));
	LISCHK(lisd_csr_plan(&d->plan, n, d->ptr, d->index, d->value));
	LISCHK(lazy_bind(c, sizeof(int) * ((size_t)np + 1), tptr, 1));
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)nnz, tidx, 1));
	LISCHK(lazy_bind(c, sizeof(double) * (size_t)nnz, tval, 1));
	*built = 1;
	return lis_matrix_set_csc(nnz, (LIS_INT *)c->lazy[0], (LIS_INT *)c->lazy[1], (LIS_SCALAR *)c->lazy[2], c->Aout);
}

/* ---- JAD.  The row order is the reference's unstable quicksort of the row lengths: made on the host (its recursion spread over the threads,
 * lis_convert.c), like the diagonal starts; the entries are placed here.  The product's arrays are A's own: the j-th entry of a
 * row sits on jagged diagonal j, so rows in their original order, entries in theirs, is the order lis_matvec_jad adds them in */
static LIS_INT build_jad(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const int n = c->n, nnz = c->nnz;
	LIS_INT maxnzr = 0, *perm = NULL, *jptr = NULL;
	int *dperm = NULL, *djptr = NULL, *jidx = NULL; double *jval = NULL;
	LISCHK(lisi_jad_order(c->Ain, &maxnzr, &perm, &jptr));
	c->heap[0] = perm; c->heap[1] = jptr;
	TMP(dperm, n); TMP(djptr, (size_t)maxnzr + 1); TMP(jidx, nnz); TMP(jval, nnz);
	HIPCHK(liship_memcpy_h2d(dperm, perm, sizeof(int) * (size_t)n, lisg.stream));
	HIPCHK(liship_memcpy_h2d(djptr, jptr, sizeof(int) * ((size_t)maxnzr + 1), lisg.stream));
	HIPCHK(liship_csr_to_jad(n, dperm, djptr, sd->ptr, sd->index, sd->value, jidx, jval, lisg.stream));
	LISCHK(clone_csr(sd, d, n, nnz));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	tmp_free(c, dperm); tmp_free(c, djptr);
	LISCHK(lisd_csr_plan(&d->plan, n, d->ptr, d->index, d->value));
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)nnz, jidx, 1)); LISCHK(lazy_bind(c, sizeof(double) * (size_t)nnz, jval, 1));
	LISCHK(lis_matrix_set_jad(nnz, maxnzr, perm, jptr, (LIS_INT *)c->lazy[0], (LIS_SCALAR *)c->lazy[1], c->Aout));
	c->heap[0] = c->heap[1] = NULL;                          /* Aout's now */
	*built = 1;
	return LIS_SUCCESS;
}

/* ---- BSR (rows of more than 96 distinct blocks: the count kernel refuses, the host routine serves) */
static LIS_INT build_bsr(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const int n = c->n, np = c->np, bnr = c->Aout->conv_bnr, bnc = c->Aout->conv_bnc;
	if (bnr < 1 || bnc < 1) return LIS_SUCCESS;
	const int nr = 1 + (n - 1) / bnr, pad = (bnc - n % bnc) % bnc;
	int *count = NULL, *bptr = NULL, *bindex = NULL, bnnz = 0, rowform = 0; long long *scratch = NULL; double *bval = NULL;
	TMP(count, (size_t)nr + 1); TMP(bptr, (size_t)nr + 1); TMP(scratch, nr / 4096 + 4);
	const int rc = liship_csr_bsr_count(n, np, bnr, bnc, sd->ptr, sd->index, count, bptr, scratch, &bnnz, lisg.stream);
	tmp_free(c, count); tmp_free(c, scratch);
	HIPCHK(rc);
	if (bnnz <= 0 || (long long)bnnz * bnr * bnc >= 0x7fffffffLL) return LIS_SUCCESS;
	const size_t bs = (size_t)bnr * (size_t)bnc;
	TMP(bindex, bnnz); TMP(bval, (size_t)bnnz * bs);
	HIPCHK(liship_csr_to_bsr(n, bnr, bnc, bnnz, sd->ptr, sd->index, sd->value, bptr, bindex, bval, lisg.stream));
	d->type = LIS_MATRIX_BSR; d->nr = nr; d->bnr = bnr; d->bnc = bnc;
	if (pad == 0)            /* constant coefficients: the row form; Aout's header is not filled in yet, the source's facts are the target's */
		LISCHK(lisd_try_bsr_row_form(n, np, bnr, bnc, 0, d, bptr, bindex, bval, bnnz, device_few_distinct_values(sd->value, (size_t)c->nnz), &rowform));
	if (!rowform) { d->bptr = (int *)tmp_release(c, bptr); d->bindex = (int *)tmp_release(c, bindex); d->value = (double *)tmp_release(c, bval); }
	LISCHK(lazy_bind(c, sizeof(int) * ((size_t)nr + 1), bptr, rowform));
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)bnnz, bindex, rowform));
	LISCHK(lazy_bind(c, sizeof(double) * (size_t)bnnz * bs, bval, rowform));
	LISCHK(lis_matrix_set_bsr(bnr, bnc, bnnz, (LIS_INT *)c->lazy[0], (LIS_INT *)c->lazy[1], (LIS_SCALAR *)c->lazy[2], c->Aout));
	c->Aout->pad_comm = pad; d->nc = c->Aout->nc;
	*built = 1;
	return LIS_SUCCESS;
}

/* ---- COO.  The triplets of csr2coo are the rows themselves: row[k] from the row starts, col and value copies of index and value.  The product's arrays are
 * rows in stored order (a COO copy IS CSR rows, lis_upload.c): ONE copy of col / value serves as d->index / d->value and backs the host arrays, as the
 * dense array does below; only row[] is extra, and the pages own it */
static LIS_INT build_coo(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const int n = c->n, nnz = c->nnz;
	int *crow = NULL, *ccol = NULL; double *cval = NULL;
	if (!liship_csr_to_coo || !lis_matrix_set_coo) return LIS_SUCCESS;          /* (linked without them: the host routine serves) */
	TMP(crow, nnz); TMP(ccol, nnz); TMP(cval, nnz);
	HIPCHK(liship_csr_to_coo(n, sd->ptr, crow, lisg.stream));
	HIPCHK(liship_memcpy_d2d(ccol, sd->index, sizeof(int) * (size_t)nnz, lisg.stream));
	HIPCHK(liship_memcpy_d2d(cval, sd->value, sizeof(double) * (size_t)nnz, lisg.stream));
	HIPCHK(lisd_malloc((void **)&d->ptr, sizeof(int) * ((size_t)n + 1)));
	HIPCHK(liship_memcpy_d2d(d->ptr, sd->ptr, sizeof(int) * ((size_t)n + 1), lisg.stream));
	d->type = LIS_MATRIX_CSR; d->index = (int *)tmp_release(c, ccol); d->value = (double *)tmp_release(c, cval);
	d->coo_in_order = 1;
	LISCHK(lisd_csr_plan(&d->plan, n, d->ptr, d->index, d->value));
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)nnz, crow, 1));
	LISCHK(lazy_bind(c, sizeof(int) * (size_t)nnz, ccol, 0));
	LISCHK(lazy_bind(c, sizeof(double) * (size_t)nnz, cval, 0));
	*built = 1;
	return lis_matrix_set_coo(nnz, (LIS_INT *)c->lazy[0], (LIS_INT *)c->lazy[1], (LIS_SCALAR *)c->lazy[2], c->Aout);
}

/* ---- DNS: one array serves the product and backs the host array */
static LIS_INT build_dns(conv_t *c, int *built)
{
	lisd_mat *d = c->d;
	const lisd_mat *sd = c->sd;
	const size_t count = (size_t)c->n * (size_t)c->np;
	double *dns = NULL;
	if (!liship_csr_to_dns_f64 || !lis_matrix_set_dns) return LIS_SUCCESS;      /* (linked without them: the host routine serves) */
	TMP(dns, count);
	HIPCHK(liship_csr_to_dns_f64(c->n, c->np, sd->ptr, sd->index, sd->value, dns, lisg.stream));
	d->type = LIS_MATRIX_DNS; d->value = (double *)tmp_release(c, dns);
	LISCHK(lazy_bind(c, sizeof(double) * count, dns, 0));
	*built = 1;
	return lis_matrix_set_dns((LIS_SCALAR *)c->lazy[0], c->Aout);
}

/* ---- the gate.  *done = 0: not a case for this path (the caller converts on the host) */
static const struct { LIS_INT type; int needs_sorted_rows; LIS_INT (*build)(conv_t *c, int *built); } targets[] = {
	{LIS_MATRIX_ELL, 0, build_ell}, {LIS_MATRIX_DIA, 1, build_dia}, {LIS_MATRIX_CSC, 1, build_csc}, {LIS_MATRIX_JAD, 0, build_jad}, {LIS_MATRIX_BSR, 0, build_bsr},
	{LIS_MATRIX_COO, 0, build_coo}, {LIS_MATRIX_DNS, 0, build_dns},
};
#define TARGETS ((int)(sizeof(targets) / sizeof(targets[0])))

/* what a builder left in d, and d empty again */
static void drop_target(lisd_mat *d)
{
	if (d->plan) (void)liship_csr_plan_destroy(d->plan);
	(void)liship_free(d->ptr); (void)liship_free(d->index); (void)liship_free(d->value); (void)liship_free(d->bptr); (void)liship_free(d->bindex);
	(void)liship_free(d->ell_codes); (void)liship_free(d->ell_dict);
	memset(d, 0, sizeof(*d));
}

LIS_INT lisd_convert_csr(LIS_MATRIX Ain, LIS_MATRIX Aout, int *done)
{
	*done = 0;
	const lisd_mat *sd = MDEV(Ain);
	int t = 0;
	while (t < TARGETS && targets[t].type != Aout->matrix_type) t++;
	/* (a matrix born in HBM -- lis_amd_matrix_set_csr_device / lis_amd_matrix_poisson3d -- converts like any other: nothing below reads Ain's host arrays, except JAD's
	 * row order, which is the reference's quicksort on the host) */
	if (t == TARGETS || lisg.no_device_convert || lisg.nprocs > 1 || !lisg.device_ready || (sd->device_only && targets[t].type == LIS_MATRIX_JAD) ||
	    Ain->matrix_type != LIS_MATRIX_CSR || Ain->is_splited || Ain->np != Ain->n || Ain->n <= 0 || Ain->nnz <= 0)
		return LIS_SUCCESS;
	LISCHK(lisd_mat_ready(Ain));          /* (an upload of the source costs a fraction of a pass of the host routine over it; a stale copy is rebuilt) */
	if (sd->type != LIS_MATRIX_CSR || !sd->ptr || !sd->index || !sd->value) return LIS_SUCCESS;
	conv_t c = { .Ain = Ain, .Aout = Aout, .sd = sd, .d = MDEV(Aout), .n = Ain->n, .np = Ain->np, .nnz = Ain->nnz };
	int *facts = NULL, hfacts[2] = {0, 0};          /* the longest row; whether a row is out of column order */
	HIPCHK(lisd_malloc((void **)&facts, 2 * sizeof(int)));
	int rc = liship_csr_row_facts(c.n, sd->ptr, sd->index, facts, lisg.stream);
	if (!rc) rc = liship_memcpy_d2h(hfacts, facts, sizeof(hfacts), lisg.stream);
	if (!rc) rc = liship_stream_synchronize(lisg.stream);
	(void)liship_free(facts);
	HIPCHK(rc);
	c.maxlen = hfacts[0];
	memset(c.d, 0, sizeof(*c.d));
	c.d->n = c.n; c.d->np = c.np; c.d->nnz = c.nnz;

	int built = 0;
	LIS_INT err = (targets[t].needs_sorted_rows && hfacts[1]) ? LIS_SUCCESS : targets[t].build(&c, &built);
	tmp_unwind(&c, 0);
	if (err || !built) {
		while (c.nlazy > 0) (void)lisp_free_array(c.lazy[--c.nlazy]);
		free(c.heap[0]); free(c.heap[1]);
		drop_target(c.d);
		return err;
	}
	LISCHK(lisd_convert_tail(Aout, c.d, c.n));
	*done = 1;
	return LIS_SUCCESS;
}

/* the tail of this gate and of lisd_convert_to_csr (lis_convert_tocsr.c): Aout's header holds its arrays from here on, so a failure takes the storage down with the copy */
LIS_INT lisd_convert_tail(LIS_MATRIX Aout, lisd_mat *d, int n)
{
	LIS_INT err;
	const int rc = liship_stream_synchronize(lisg.stream);
	if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	else {
		d->inner_begin = 0; d->inner_end = n;
		d->ready = 1;                                      /* the HBM copy exists: lis_matrix_assemble's eager upload finds nothing to do */
		err = lis_matrix_assemble(Aout);
	}
	if (err) lisi_matrix_storage_destroy(Aout);
	return err;
}

/* the same for a CSR target (lis_convert_tocsr.c), with what comes before it: the three buffers become Aout's HBM copy with their plan, Aout's host arrays are bound
 * to them (lazy_bind, not owning), lis_matrix_set_csr, then the tail above.  The buffers are taken whatever happens: after a failure they are freed with the copy */
LIS_INT lisd_convert_adopt_csr(LIS_MATRIX Aout, int n, int np, int nnz, int *ptr, int *index, double *value)
{
	conv_t c = { .Aout = Aout, .d = MDEV(Aout), .n = n, .np = np, .nnz = nnz };
	lisd_mat *d = c.d;
	memset(d, 0, sizeof(*d));
	d->n = n; d->np = np; d->nnz = nnz; d->type = LIS_MATRIX_CSR;
	d->ptr = ptr; d->index = index; d->value = value;
	LIS_INT err = lisd_csr_plan_cols(&d->plan, n, np, ptr, index, value);
	if (!err) err = lazy_bind(&c, sizeof(int) * ((size_t)n + 1), ptr, 0);
	if (!err) err = lazy_bind(&c, sizeof(int) * (size_t)nnz, index, 0);
	if (!err) err = lazy_bind(&c, sizeof(double) * (size_t)nnz, value, 0);
	if (!err) {
		Aout->pad = 0; Aout->pad_comm = 0;                      /* as lisi_convert_to_csr: a CSR matrix has no padding, whatever the (duplicated) tables of a BSR source said */
		if (Aout->commtable) Aout->commtable->pad = 0;
		err = lis_matrix_set_csr(nnz, (LIS_INT *)c.lazy[0], (LIS_INT *)c.lazy[1], (LIS_SCALAR *)c.lazy[2], Aout);
	}
	if (err) {
		while (c.nlazy > 0) (void)lisp_free_array(c.lazy[--c.nlazy]);
		drop_target(d);
		return err;
	}
	return lisd_convert_tail(Aout, d, n);
}

/* A host copy of a CSR matrix that lives in HBM only (lis_amd_matrix_set_csr_device / lis_amd_matrix_poisson3d): what lis_matrix_convert hands to the host routines
 * when the conversion asked for is not built in HBM -- JAD (its row order is the reference's sort on the host), DIA and CSC of rows that are not in ascending column
 * order, BSR rows of more than 96 blocks.  One rank, no ghost columns, at least one entry (what lisd_convert_csr asks too;
 * anything else is refused as before).  The caller destroys *home. */
LIS_INT lisd_csr_home(LIS_MATRIX Ain, LIS_MATRIX *home)
{
	lisd_mat *sd = MDEV(Ain);
	*home = NULL;
	if (!sd->device_only || sd->type != LIS_MATRIX_CSR || !sd->ptr || lisg.nprocs > 1 || Ain->np != Ain->n || Ain->n <= 0 || Ain->nnz <= 0)
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "matrix lives in HBM only: this conversion runs on host arrays -- convert the host matrix before uploading\n");
	const LIS_INT n = Ain->n, nnz = Ain->nnz;
	LIS_MATRIX H = NULL; LIS_INT *p = NULL, *i = NULL; LIS_SCALAR *v = NULL;
	LISCHK(lis_matrix_duplicate(Ain, &H));
	LIS_INT err = lis_matrix_malloc_csr(n, nnz, &p, &i, &v);
	if (!err) {
		int rc = liship_memcpy_d2h(p, sd->ptr, sizeof(int) * ((size_t)n + 1), lisg.stream);
		if (!rc) rc = liship_memcpy_d2h(i, sd->index, sizeof(int) * (size_t)nnz, lisg.stream);
		if (!rc) rc = liship_memcpy_d2h(v, sd->value, sizeof(double) * (size_t)nnz, lisg.stream);
		if (!rc) rc = liship_stream_synchronize(lisg.stream);
		if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc);
	}
	if (!err) err = lis_matrix_set_csr(nnz, p, i, v, H);
	if (err) { lis_free(p); lis_free(i); lis_free(v); lis_matrix_destroy(H); return err; }
	/* assembled as far as the host routines care -- they read n, np, nnz and the three arrays -- without lis_matrix_assemble, which would build an HBM copy of the copy */
	H->matrix_type = LIS_MATRIX_CSR; H->status = LIS_MATRIX_CSR;
	*home = H;
	return LIS_SUCCESS;
}
