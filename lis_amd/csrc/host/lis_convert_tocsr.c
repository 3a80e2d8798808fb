/*
 * lis_convert_tocsr.c -- the way back: lis_matrix_convert(Ain, Aout) with Aout a CSR matrix, built in HBM (kernels/convert.hip).
 *
 * lis_convert_hbm.c builds ELL, DIA, CSC, JAD, BSR, COO and DNS from a CSR copy; this file builds the CSR rows of an ELL, DIA, BSR, DNS, VBR, CSC or JAD matrix -- the
 * arrays lisi_convert_to_csr (lis_convert.c) makes on the host, in every integer and every bit -- without bringing the source's arrays home.  Callers: lis_matrix_convert
 * itself (X -> CSR, and the first half of X -> Y), and through it lis_matrix_shift_matrix of a matrix in another storage, -storage / -estorage, -p sainv.
 *
 * WHERE THE SOURCE'S ARRAYS ARE, array by array (src_int / src_dbl):
 *   1. in the source's HBM copy, when that copy is of the native family (ELL / DIA / BSR / DNS / VBR arrays as the host holds them) and current;
 *   2. in the device buffer behind a host array that is still held in HBM only (a matrix made by a conversion there whose copy is the row form: lisp_lazy_device);
 *   3. at home: uploaded into a temporary that goes when the conversion is done.  No HBM copy and no plan of the source is built for the sake of a conversion.
 * CSC and JAD need no kernel: their HBM copy IS these rows (upload_csc_as_csr / upload_jad_as_csr, build_csc / build_jad), so the copy is made ready and its three
 * arrays are copied inside HBM.
 * COO stays on the host: lis_matrix_convert_coo2csr sorts the SOURCE's three arrays in place with an unstable quicksort, a row's order is whatever that leaves and the
 * source is changed -- lisi_convert_to_csr is the only path that does that.
 *
 * The result's three buffers become Aout's HBM copy with their plan, Aout's host arrays are address space bound to them (lis_pages.c) and come home on their first
 * touch, and that tail is written once, beside lisd_convert_csr's (lisd_convert_adopt_csr, lisd_convert_tail in lis_convert_hbm.c).
 */
#include <limits.h>
#include "lis_internal.h"

#define TOCSR_TMP 16
typedef struct {
	LIS_MATRIX Ain;
	const lisd_mat *sd;
	int native;                            /* sd holds the source's native arrays, current */
	int n, np, nnz;
	void *tmp[TOCSR_TMP]; int ntmp;        /* uploads and work arrays: freed when the gate returns */
	int *count, *rptr; long long *scratch; /* work of every builder (rptr leaves the scope when the rows are built) */
	int *ridx; double *rval;
} tocsr_t;

static int tmp_alloc(tocsr_t *c, void **out, size_t bytes)          /* HIP code, as lisd_malloc */
{
	if (c->ntmp == TOCSR_TMP) return LISHIP_ERR_ARG;
	const int rc = lisd_malloc(out, bytes ? bytes : 1);
	if (!rc) c->tmp[c->ntmp++] = *out;
	return rc;
}
#define TMP(p, count) HIPCHK(tmp_alloc(c, (void **)&(p), sizeof(*(p)) * (size_t)(count)))
static void *tmp_release(tocsr_t *c, void *p)
{
	for (int i = 0; i < c->ntmp; i++) if (c->tmp[i] == p) c->tmp[i] = NULL;
	return p;
}

/* array `host` of the source in HBM (the three cases above); `native`: where the copy holds it, NULL when it does not */
static LIS_INT src_bytes(tocsr_t *c, const void *host, const void *native, size_t bytes, const void **out)
{
	void *dev = (c->native && native) ? (void *)native : lisp_lazy_device(host);
	if (!dev) {
		HIPCHK(tmp_alloc(c, &dev, bytes));
		if (bytes) HIPCHK(liship_memcpy_h2d(dev, host, bytes, lisg.stream));
	}
	*out = dev;
	return LIS_SUCCESS;
}
#define SRC(out, host, native, count) LISCHK(src_bytes(c, (host), (native), sizeof(*(host)) * (size_t)(count), (const void **)&(out)))

/* the work arrays of a count entry over m counts */
static LIS_INT work(tocsr_t *c, size_t m)
{
	TMP(c->count, m); TMP(c->rptr, (size_t)c->n + 1); TMP(c->scratch, m / 4096 + 4);
	return LIS_SUCCESS;
}
/* what a count entry answered: *go = 1 when the rows are to be filled (index and value allocated), 0 when the host routine serves (no entry kept, or more than an int counts) */
static LIS_INT counted(tocsr_t *c, int rc, int *go)
{
	*go = 0;
	if (rc == LISHIP_ERR_OVERFLOW) return LIS_SUCCESS;
	HIPCHK(rc);
	if (c->nnz <= 0) return LIS_SUCCESS;
	TMP(c->ridx, c->nnz); TMP(c->rval, c->nnz);
	*go = 1;
	return LIS_SUCCESS;
}

static LIS_INT from_ell(tocsr_t *c, int *built)
{
	const LIS_MATRIX A = c->Ain;
	const size_t slots = (size_t)c->n * (size_t)A->maxnzr;
	const int *eidx; const double *eval; int go;
	SRC(eidx, A->index, c->sd->index, slots); SRC(eval, A->value, c->sd->value, slots);
	LISCHK(work(c, (size_t)c->n));
	LISCHK(counted(c, liship_ell_csr_count(c->n, A->maxnzr, eval, c->count, c->rptr, c->scratch, &c->nnz, lisg.stream), &go));
	if (!go) return LIS_SUCCESS;
	HIPCHK(liship_ell_to_csr(c->n, A->maxnzr, eidx, eval, c->rptr, c->ridx, c->rval, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

static LIS_INT from_dia(tocsr_t *c, int *built)
{
	const LIS_MATRIX A = c->Ain;
	const int *offs; const double *dval; int go;
	SRC(offs, A->index, c->sd->index, A->nnd); SRC(dval, A->value, c->sd->value, (size_t)c->n * (size_t)A->nnd);
	LISCHK(work(c, (size_t)c->n));
	LISCHK(counted(c, liship_dia_csr_count(c->n, c->np, A->nnd, offs, dval, c->count, c->rptr, c->scratch, &c->nnz, lisg.stream), &go));
	if (!go) return LIS_SUCCESS;
	HIPCHK(liship_dia_to_csr(c->n, c->np, A->nnd, offs, dval, c->rptr, c->ridx, c->rval, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

static LIS_INT from_bsr(tocsr_t *c, int *built)
{
	const LIS_MATRIX A = c->Ain;
	const lisd_mat *sd = c->sd;
	const int *bptr, *bidx; const double *bval; int go;
	if (A->bnr < 1 || A->bnc < 1 || A->nr != 1 + (c->n - 1) / A->bnr) return LIS_SUCCESS;
	if (c->native && (sd->bnr != A->bnr || sd->bnc != A->bnc)) c->native = 0;
	SRC(bptr, A->bptr, sd->bptr, (size_t)A->nr + 1); SRC(bidx, A->bindex, sd->bindex, A->bnnz);
	SRC(bval, A->value, sd->value, (size_t)A->bnnz * (size_t)A->bnr * (size_t)A->bnc);
	LISCHK(work(c, (size_t)c->n));
	LISCHK(counted(c, liship_bsr_csr_count(c->n, A->bnr, A->bnc, bptr, bidx, bval, c->count, c->rptr, c->scratch, &c->nnz, lisg.stream), &go));
	if (!go) return LIS_SUCCESS;
	HIPCHK(liship_bsr_to_csr(c->n, A->bnr, A->bnc, bptr, bidx, bval, c->rptr, c->ridx, c->rval, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

static LIS_INT from_dns(tocsr_t *c, int *built)
{
	const LIS_MATRIX A = c->Ain;
	const double *dns; int *offsets = NULL, info[3], go;
	HIPCHK(liship_tocsr_tile_info(info));
	const size_t nslab = ((size_t)c->np + (size_t)info[1] - 1) / (size_t)info[1], cells = (size_t)c->n * nslab;
	if (nslab > 65535 || cells >= (size_t)INT_MAX) return LIS_SUCCESS;
	SRC(dns, A->value, c->sd->value, (size_t)c->n * (size_t)c->np);
	LISCHK(work(c, cells));
	TMP(offsets, cells + 1);
	LISCHK(counted(c, liship_dns_csr_count(c->n, c->np, dns, c->count, offsets, c->rptr, c->scratch, &c->nnz, lisg.stream), &go));
	if (!go) return LIS_SUCCESS;
	HIPCHK(liship_dns_to_csr(c->n, c->np, dns, offsets, c->ridx, c->rval, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

/* arrays that do not come from a checked copy are checked here before a lane takes an address from them, as upload_vbr does */
static LIS_INT from_vbr(tocsr_t *c, int *built)
{
	const LIS_MATRIX A = c->Ain;
	const lisd_mat *sd = c->sd;
	const int *row, *col, *ptr, *bptr, *bidx, *brow = (c->native ? sd->brow : NULL); const double *val; int go;
	if (A->nnz < 0 || A->bnnz < 0 || A->nr < 1 || A->nc < 1) return LIS_SUCCESS;
	if (c->native && (!sd->row || !sd->col || !sd->ptr || !sd->bptr || !sd->bindex || !sd->value || !sd->brow)) c->native = 0;
	SRC(row, A->row, sd->row, (size_t)A->nr + 1); SRC(col, A->col, sd->col, (size_t)A->nc + 1); SRC(ptr, A->ptr, sd->ptr, (size_t)A->bnnz + 1);
	SRC(bptr, A->bptr, sd->bptr, (size_t)A->nr + 1); SRC(bidx, A->bindex, sd->bindex, A->bnnz); SRC(val, A->value, sd->value, A->nnz);
	if (!c->native) {
		int flags = 0, *made = NULL;
		HIPCHK(liship_vbr_check(c->n, c->np, A->nnz, A->nr, A->nc, A->bnnz, row, col, ptr, bptr, bidx, &flags, lisg.stream));
		if (flags) return LIS_SUCCESS;                          /* (the host routine reads them as the reference does) */
		TMP(made, (size_t)c->n + 4);
		HIPCHK(liship_vbr_block_rows(c->n, A->nr, row, made, lisg.stream));
		brow = made;
	}
	LISCHK(work(c, (size_t)c->n));
	LISCHK(counted(c, liship_vbr_csr_count(c->n, row, col, ptr, bptr, bidx, brow, val, c->count, c->rptr, c->scratch, &c->nnz, lisg.stream), &go));
	if (!go) return LIS_SUCCESS;
	HIPCHK(liship_vbr_to_csr(c->n, row, col, ptr, bptr, bidx, brow, val, c->rptr, c->ridx, c->rval, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

/* CSC, JAD: the rows of the source's own HBM copy */
static LIS_INT from_rows(tocsr_t *c, int *built)
{
	LISCHK(lisd_mat_ready(c->Ain));
	const lisd_mat *sd = c->sd;
	if (sd->type != LIS_MATRIX_CSR || sd->solve_holds || sd->split_jad || !sd->ptr || !sd->index || !sd->value || sd->nnz != c->Ain->nnz || sd->nnz <= 0) return LIS_SUCCESS;
	c->nnz = sd->nnz;
	TMP(c->rptr, (size_t)c->n + 1); TMP(c->ridx, c->nnz); TMP(c->rval, c->nnz);
	HIPCHK(liship_memcpy_d2d(c->rptr, sd->ptr, sizeof(int) * ((size_t)c->n + 1), lisg.stream));
	HIPCHK(liship_memcpy_d2d(c->ridx, sd->index, sizeof(int) * (size_t)c->nnz, lisg.stream));
	HIPCHK(liship_memcpy_d2d(c->rval, sd->value, sizeof(double) * (size_t)c->nnz, lisg.stream));
	*built = 1;
	return LIS_SUCCESS;
}

/* ---- the gate.  *done = 0: not a case for this path (the caller runs lisi_convert_to_csr on the host arrays, as before).  COO is not in the table on purpose:
 * the reference's coo2csr sorts the source in place with an unstable sort, and only the host routine does exactly that */
static const struct { LIS_INT type; int native_family; LIS_INT (*build)(tocsr_t *c, int *built); } sources[] = {
	{LIS_MATRIX_ELL, 1, from_ell}, {LIS_MATRIX_DIA, 1, from_dia}, {LIS_MATRIX_BSR, 1, from_bsr}, {LIS_MATRIX_DNS, 1, from_dns}, {LIS_MATRIX_VBR, 1, from_vbr},
	{LIS_MATRIX_CSC, 0, from_rows}, {LIS_MATRIX_JAD, 0, from_rows},
};
#define SOURCES ((int)(sizeof(sources) / sizeof(sources[0])))

LIS_INT lisd_convert_to_csr(LIS_MATRIX Ain, LIS_MATRIX Aout, int *done)
{
	*done = 0;
	lisd_mat *sd = MDEV(Ain);
	int s = 0;
	while (s < SOURCES && sources[s].type != Ain->matrix_type) s++;
	if (s == SOURCES || lisg.no_device_convert || lisg.nprocs > 1 || !lisg.device_ready || sd->device_only || sd->solve_holds ||
	    Ain->is_splited || Ain->np != Ain->n || Ain->n <= 0)
		return LIS_SUCCESS;
	/* a copy that exists is held to its staleness rules (a host write that was seen: the copy goes, and the arrays are read where they are now -- at home) */
	if (sd->ready && !sd->host_written) LISCHK(lisd_mat_ready(Ain));
	tocsr_t c = { .Ain = Ain, .sd = sd, .n = Ain->n, .np = Ain->np };
	c.native = sources[s].native_family && sd->ready && !sd->host_written && sd->type == Ain->matrix_type;
	int built = 0;
	LIS_INT err = sources[s].build(&c, &built);
	if (!err && built)            /* the rows become Aout: the tail lisd_convert_csr's targets have, for a CSR target (lis_convert_hbm.c) */
		err = lisd_convert_adopt_csr(Aout, c.n, c.np, c.nnz, (int *)tmp_release(&c, c.rptr), (int *)tmp_release(&c, c.ridx), (double *)tmp_release(&c, c.rval));
	const int rc = liship_stream_synchronize(lisg.stream);           /* (the uploads and the kernels that read the temporaries have run) */
	for (int i = 0; i < c.ntmp; i++) if (c.tmp[i]) (void)liship_free(c.tmp[i]);
	if (err) return err;
	HIPCHK(rc);
	*done = built;
	return LIS_SUCCESS;
}
