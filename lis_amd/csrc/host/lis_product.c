/*
 * lis_product.c -- y = A x on device pointers, and the same product with <w,y> (and <y,y>) formed on the way:
 * lisd_spmv and lisd_spmv_dot_launch[_to], behind every lis_matvec and every Krylov iteration.
 *
 * What differs between the storage formats of the HBM copy is one row of a table (fmt_ops); when a product may run under
 * the halo exchange is one predicate (overlap_ok), and how it does is one walker (walk_overlapped).
 */
#include "lis_internal.h"

/* The launchers of one kernel family; all return HIP codes.  The table keys on the HBM copy (d->type, d->split_jad), never on
 * A->matrix_type: CSC, COO and plain JAD uploads, and the row forms of ELL / DIA / BSR, are CSR here. */
#define PRODUCT lisd_mat *d, LIS_MATRIX A, double *x, double *y                 /* y = A x: the HBM copy, its matrix, device pointers */
#define DOTS const double *w, int want_sumsq, double *result                     /* result[0] = <w,y>, result[1] = <y,y> when want_sumsq (HBM) */
typedef struct {
	int block_rows;            /* row ranges, inner_begin / inner_end and the overlap threshold count block rows (d->nr), not rows (d->n) */
	int (*whole)(PRODUCT);                     /* the whole product */
	int (*rows)(PRODUCT, int rb, int re);      /* rows [rb, re) of it, the same bits; NULL: none, so never under the halo */
	/* the product with its dot(s) in one launch; LISHIP_ERR_ARG: not this shape, then `plain` and one reduction pass.  NULL: none */
	int (*dot)(PRODUCT, DOTS);
	int (*plain)(PRODUCT);                     /* the whole product behind a refused `dot` */
} fmt_ops;

/* XCD strips (d->xs_rows, found at upload time): in front of every whole-matrix launch of a native ELL / DIA kernel, and of no row-range launch */
static void fmt_strips(const lisd_mat *d)
{
	(void)liship_spmv_formats_set_plane((d->xs_rows > 0 && (size_t)d->n * sizeof(double) > ((size_t)256 << 20)) ? d->xs_rows : 0);
}

static int csr_whole(PRODUCT) { return liship_spmv_csr_f64(d->plan, d->ptr, d->index, d->value, x, y, lisg.stream); }
static int csr_rows(PRODUCT, int rb, int re) { return liship_spmv_csr_rows_f64(d->plan, rb, re, d->ptr, d->index, d->value, x, y, lisg.stream); }
static int csr_dot(PRODUCT, DOTS) { return liship_spmv_csr_dot_f64(d->plan, d->ptr, d->index, d->value, x, y, w, want_sumsq, result, lisg.reduce_work, lisg.stream); }

static int ell_index(PRODUCT) { return liship_spmv_ell_f64(d->n, d->maxnzr, d->index, d->value, x, y, lisg.stream); }      /* the 4-byte-index kernel */
static int ell_whole(PRODUCT)
{
	fmt_strips(d);
	if (d->ell_codes) {
		const int rc = liship_spmv_ell_coded_f64(d->n, d->maxnzr, d->ell_codes, d->ell_dict, d->value, x, y, NULL, -1, NULL, NULL, lisg.stream);
		if (rc != LISHIP_ERR_ARG) return rc;
	}
	return ell_index(d, A, x, y);
}
static int ell_rows(PRODUCT, int rb, int re) { return liship_spmv_ell_rows_f64(d->n, d->maxnzr, d->index, d->ell_codes, d->ell_dict, d->value, x, y, rb, re, lisg.stream); }
static int ell_dot(PRODUCT, DOTS)
{
	fmt_strips(d);
	if (d->ell_codes)
		return liship_spmv_ell_coded_f64(d->n, d->maxnzr, d->ell_codes, d->ell_dict, d->value, x, y, w, want_sumsq ? 1 : 0, result, lisg.reduce_work, lisg.stream);
	return liship_spmv_ell_dot_f64(d->n, d->maxnzr, d->index, d->value, x, y, w, want_sumsq, result, lisg.reduce_work, lisg.stream);
}

static int dia_launch(PRODUCT) { return liship_spmv_dia_f64(d->n, d->np, d->nnd, d->index, d->value, x, y, lisg.stream); }
static int dia_whole(PRODUCT)
{
	fmt_strips(d);
	return dia_launch(d, A, x, y);
}
static int dia_rows(PRODUCT, int rb, int re) { return liship_spmv_dia_rows_f64(d->n, d->np, d->nnd, d->index, d->value, x, y, rb, re, lisg.stream); }
static int dia_dot(PRODUCT, DOTS)
{
	fmt_strips(d);
	return liship_spmv_dia_dot_f64(d->n, d->np, d->nnd, d->index, d->value, x, y, w, want_sumsq, result, lisg.reduce_work, lisg.stream);
}

static int jad_whole(PRODUCT) { return liship_spmv_jad_f64(d->n, d->maxnzr, d->row, d->ptr, d->index, d->value, x, y, lisg.stream); }

static int bsr_whole(PRODUCT) { return liship_spmv_bsr_nnz_f64(d->nr, A->bnnz, d->bnr, d->bnc, d->bptr, d->bindex, d->value, x, y, lisg.stream); }
static int bsr_rows(PRODUCT, int rb, int re) { return liship_spmv_bsr_rows_f64(d->nr, A->bnnz, d->bnr, d->bnc, d->bptr, d->bindex, d->value, x, y, rb, re, lisg.stream); }
static int bsr_dot(PRODUCT, DOTS) { return liship_spmv_bsr_dot_f64(d->nr, d->n, A->bnnz, d->bnr, d->bptr, d->bindex, d->value, x, y, w, want_sumsq, result, lisg.reduce_work, lisg.stream); }

/* split JAD (lis_split.c; d->plan holds L, d->u_plan U): y = (D x + L x) + U x, the two sparse sums each formed from 0 on their own:
 * w = L x; w = D.*x + 1*w (exact: 1*w is w); y = U x; y += 1*w (a + b and b + a are the same double) */
static int split_jad_whole(PRODUCT)
{
	int rc = liship_spmv_csr_f64(d->plan, d->ptr, d->index, d->value, x, d->jw, lisg.stream);
	if (!rc) rc = liship_pmul_xpay_f64(d->n, d->dsplit, x, 1.0, d->jw, lisg.stream);
	if (!rc) rc = liship_spmv_csr_f64(d->u_plan, d->u_ptr, d->u_index, d->u_value, x, y, lisg.stream);
	if (!rc) rc = liship_axpy_f64(d->n, 1.0, d->jw, y, lisg.stream);
	return rc;
}

/* dense: no row ranges (several ranks are refused), no fused dot (the dispatcher runs the product and one reduction pass).  The launcher is referenced weakly:
 * tests/c/product_cases.c links this file alone against stubs of the launchers of the six formats it walks, and the library always holds the real one */
extern int liship_spmv_dns_f64(int n, int np, const double *value, const double *x, double *y, void *stream) __attribute__((weak));
static int dns_whole(PRODUCT) { return liship_spmv_dns_f64 ? liship_spmv_dns_f64(d->n, d->np, d->value, x, y, lisg.stream) : LISHIP_ERR_ARG; }

/* variable blocks: like dense, no row ranges and no fused dot; weak for the same reason */
extern int liship_spmv_vbr_f64(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, const double *value,
                               const double *x, double *y, void *stream) __attribute__((weak));
static int vbr_whole(PRODUCT) { return liship_spmv_vbr_f64 ? liship_spmv_vbr_f64(d->n, d->row, d->col, d->ptr, d->bptr, d->bindex, d->brow, d->value, x, y, lisg.stream) : LISHIP_ERR_ARG; }

static const fmt_ops csr_ops = {0, csr_whole, csr_rows, csr_dot, csr_whole};
static const fmt_ops ell_ops = {0, ell_whole, ell_rows, ell_dot, ell_index};       /* (no second attempt with the codes, no strips again) */
static const fmt_ops dia_ops = {0, dia_whole, dia_rows, dia_dot, dia_launch};
static const fmt_ops jad_ops = {0, jad_whole, NULL, NULL, NULL};
static const fmt_ops bsr_ops = {1, bsr_whole, bsr_rows, bsr_dot, bsr_whole};
static const fmt_ops split_jad_ops = {0, split_jad_whole, NULL, NULL, NULL};
static const fmt_ops dns_ops = {0, dns_whole, NULL, NULL, NULL};
static const fmt_ops vbr_ops = {0, vbr_whole, NULL, NULL, NULL};

static const fmt_ops *ops_of(const lisd_mat *d)
{
	if (d->split_jad) return &split_jad_ops;           /* (its d->type is CSR: d->plan alone is only L) */
	switch (d->type) {
	case LIS_MATRIX_CSR: return &csr_ops;
	case LIS_MATRIX_ELL: return &ell_ops;
	case LIS_MATRIX_DIA: return &dia_ops;
	case LIS_MATRIX_JAD: return &jad_ops;
	case LIS_MATRIX_BSR: return &bsr_ops;
	case LIS_MATRIX_DNS: return &dns_ops;
	case LIS_MATRIX_VBR: return &vbr_ops;
	default: return NULL;
	}
}

static int exchanges(LIS_MATRIX A) { return lisg.nprocs > 1 && A->commtable; }

/* The product may run under the halo: rows [inner_begin, inner_end) reference no ghost column and are at least half of the rank's rows.  Decided rank by rank. */
static int overlap_ok(LIS_MATRIX A, const lisd_mat *d, const fmt_ops *ops) { return exchanges(A) && ops->rows && !lisg.no_overlap && d->inner_end - d->inner_begin >= (ops->block_rows ? d->nr : d->n) / 2; }

/* one product in row ranges: what the walker hands to its `part` */
typedef struct {
	const fmt_ops *ops; lisd_mat *d; LIS_MATRIX A; double *x, *y;
	const double *w; int want_sumsq, slots;           /* the fused CSR product: partial sums parked so far */
} span_t;

/* The interior rows while the halo travels, then the boundary rows in front of and behind them once the ghosts have landed (same kernels, same bits:
 * rows are independent).  An empty head or tail is not launched.  refused != NULL: an interior part that answers LISHIP_ERR_ARG sets it and ends the
 * walk, with the ghosts in; otherwise that code fails like any other. */
static LIS_INT walk_overlapped(span_t *s, int (*part)(span_t *s, int rb, int re), int *refused)
{
	const lisd_mat *d = s->d;
	const int end = s->ops->block_rows ? d->nr : d->n;
	LISCHK(lisc_halo_begin(s->A, s->x));
	const int rc = part(s, d->inner_begin, d->inner_end);
	LISCHK(lisc_halo_end(s->A, s->x));
	if (refused && rc == LISHIP_ERR_ARG) { *refused = 1; return LIS_SUCCESS; }
	HIPCHK(rc);
	if (d->inner_begin > 0) HIPCHK(part(s, 0, d->inner_begin));
	if (d->inner_end < end) HIPCHK(part(s, d->inner_end, end));
	return LIS_SUCCESS;
}

static int plain_part(span_t *s, int rb, int re) { return s->ops->rows(s->d, s->A, s->x, s->y, rb, re); }

/* every part parks its per-block partial sums behind those of the parts before it; liship_spmv_csr_dot_finish_f64 folds them */
static int csr_dot_part(span_t *s, int rb, int re)
{
	const lisd_mat *d = s->d;
	int used = 0;
	const int rc = liship_spmv_csr_rows_dot_f64(d->plan, rb, re, d->ptr, d->index, d->value, s->x, s->y, s->w, s->want_sumsq, lisg.reduce_work, s->slots, &used, lisg.stream);
	if (rc == 0) s->slots += used;
	return rc;
}

/* y = A x.  In a multi-GPU job the ghost part of x is filled first, or travels while the rows that do not touch ghosts run. */
LIS_INT lisd_spmv(LIS_MATRIX A, double *dx, double *dy)
{
	lisd_mat *d = MDEV(A);
	LISCHK(lisd_mat_ready(A));
	d->served++;
	const fmt_ops *ops = ops_of(d);
	if (!ops) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "storage format %D is not served by liblis_amd\n", d->type);
	if (overlap_ok(A, d, ops)) {
		span_t s = {ops, d, A, dx, dy, NULL, 0, 0};
		return walk_overlapped(&s, plain_part, NULL);
	}
	if (exchanges(A)) LISCHK(lisc_halo_device(A, dx));
	HIPCHK(ops->whole(d, A, dx, dy));
	return LIS_SUCCESS;
}

/* a CSR plan whose products run the team / staged kernels has no per-row-block epilogue; the fused BSR kernels want square blocks */
static int fuses(const lisd_mat *d)
{
	if (d->type == LIS_MATRIX_CSR) return !d->plan || liship_csr_plan_fused_dots(d->plan);
	return d->type != LIS_MATRIX_BSR || d->bnr == d->bnc;
}

/* y = A x with <w,y> (and <y,y>) formed in the product's epilogue when the kernel can; otherwise the product followed by one reduction pass.
 * The sums land in result[0..1] (HBM); lisd_spmv_dot_launch: in lisg.reduce_out. */
LIS_INT lisd_spmv_dot_launch_to(LIS_MATRIX A, double *dx, double *dy, const double *dw, int want_sumsq, double *result)
{
	lisd_mat *d = MDEV(A);
	LISCHK(lisd_mat_ready(A));
	d->served++;                          /* (a branch below that falls back to lisd_spmv counts the product twice: the count is a threshold, not a statistic) */
	const fmt_ops *ops = ops_of(d);
	const int fused = ops && ops->dot && !lisg.no_fusion && fuses(d);
	/* the one fused product in row ranges.  Its three parts launch at most nblocks + 2 row blocks (each cut splits one): all of them must find a slot
	 * for their partial sums BEFORE the first part is launched -- otherwise the plain overlapped product + one dot pass */
	const int in_parts = fused && ops == &csr_ops && overlap_ok(A, d, ops);
	if (!fused || (in_parts && d->plan && (size_t)liship_csr_plan_fused_slots(d->plan) > liship_reduce_work_bytes() / sizeof(double) / 4)) {
		LISCHK(lisd_spmv(A, dx, dy));
	} else {
		int rc = LISHIP_ERR_ARG;
		if (in_parts) {
			span_t s = {ops, d, A, dx, dy, dw, want_sumsq, 0};
			int refused = 0;
			LISCHK(walk_overlapped(&s, csr_dot_part, &refused));
			if (!refused) rc = liship_spmv_csr_dot_finish_f64(s.slots, want_sumsq, result, lisg.reduce_work, lisg.stream);
		} else {
			if (exchanges(A)) LISCHK(lisc_halo_device(A, dx));
			rc = ops->dot(d, A, dx, dy, dw, want_sumsq, result);
		}
		if (rc == 0) return LIS_SUCCESS;
		if (rc != LISHIP_ERR_ARG) HIPCHK(rc);
		HIPCHK(ops->plain(d, A, dx, dy));             /* refused: the whole product (the ghosts are in), then the reduction */
	}
	/* over A's n rows: the row form of a split BSR matrix (d->n) counts the padding rows of its last block row too, which would move the chunk borders of the reference-order sums */
	if (want_sumsq) HIPCHK(liship_dot2_f64(A->n, dy, dw, result, lisg.reduce_work, lisg.stream));
	else HIPCHK(liship_dot_f64(A->n, dw, dy, result, lisg.reduce_work, lisg.stream));
	return LIS_SUCCESS;
}

LIS_INT lisd_spmv_dot_launch(LIS_MATRIX A, double *dx, double *dy, const double *dw, int want_sumsq)
{
	return lisd_spmv_dot_launch_to(A, dx, dy, dw, want_sumsq, lisg.reduce_out);
}
