/*
 * lis_ilu.c -- the ILU(k) preconditioner (ref src/precon/lis_precon_iluk.c, the OpenMP branches) factorised and applied in HBM.
 *
 * Served: A in CSR storage, not split, one rank, no -scale, -adds false, -ilu_fill k >= 0.  A is never split, converted or written.
 *
 * Symbolic step (host, once per pattern, fill and block count; cached on the HBM copy of A, lisd_mat.ilu, and dropped with it):
 * the reference's pattern in the reference's term order.  Row i of L: the kept columns before i ascending -- the smallest column
 * not yet used is the next pivot, and the fill-in a pivot brings joins the list before the next one is chosen; a column A stores
 * twice stays twice.  Row i of U: the kept columns after i in A's stored order, then fill-in in the order the pivots (ascending,
 * each pivot's U row in its own order) bring it.  An entry (i, c) reached through pivot j has level lev(i, j) + lev(j, c) + 1, the
 * smallest over the pivots that reach it, and is kept while that is <= fill.  The diagonal is apart.
 * The reference runs T row blocks (LIS_GET_ISIE) of T threads and drops every entry whose column leaves the row's block:
 * block-Jacobi ILU with T blocks.  Here T = 1 (true ILU(k), independent of any core count) unless the reference-order mode asks
 * for T (lis_amd_set_reference_reductions(T)), which reproduces the reference at T threads.
 *
 * From the pattern: the forward levels (level of row i = 1 + the largest level of the rows its L pattern names), which the
 * factorisation (kernels/ilu.hip, a place of the pattern one double: bn = 1) and the forward sweep share, and four level-ordered sweep layouts (lis_sweep.c, the engine
 * SSOR runs on too): L, U, and for M^-H the transposed U^T (terms by source row ascending) and L^T (by source row descending,
 * ties by place in the source row) -- as row-wise sums these are the reference's scatters bit for bit.  The layouts hold copies of the values:
 * after every factorisation a gather kernel per layout fills them in HBM from the factor (the permutation kept from the build).
 *   psolve : x = b; forward on L (no diagonal); backward on U, then x[i] = d[i] x[i]           (ref :880-934)
 *   psolveh: x = b; forward on U^T with x[i] = d[i] x[i] first; backward on L^T (no diagonal)    (ref :1086-1140)
 * The numbers are refactorised by every lis_precon_create, from A's values as they lie in HBM.
 *
 * BSR storage (bnr == bnc in 1..3): block ILU(k) (ref :102-109, :1289-1468, :1714-1819, :2006-2037; the same kernels at bn = 2, 3).  The same entry
 * with a block where the point form has a number: the symbolic step runs unchanged on (nr, bptr, bindex) with the T row blocks of
 * LIS_GET_ISIE over the nr block rows, the schedule and the L and U layouts come from the same builders (a place holds bn*bn doubles,
 * filled by the block gather), d holds the INVERTED diagonal blocks.  The factorisation reads A's blocks in native layout: the HBM
 * copy's own arrays, or -- when the copy is held in its row form (lis_upload.c lisd_try_bsr_row_form) -- a native upload kept on the entry,
 * which dies with the copy like everything else here.  psolve only: the reference's OpenMP build applies M^-1 where M^-H is meant
 * (:2098-2165 is a copy of psolve), which this library neither reproduces nor replaces, so solvers that need M^-H are refused.
 */
#include <stdio.h>
#include "lis_krylov.h"

typedef struct {
	int used, fill, T, n;                      /* n: the rows of the pattern -- A's rows, or its block rows */
	int bn, an;                                /* a place of the pattern holds bn x bn doubles (CSR storage: 1); A's rows */
	int bsr;                                   /* A is held in BSR storage: which arrays the factorisation reads, no M^-H */
	int *d_ap, *d_ai; double *d_av;            /* BSR whose HBM copy is held in row form: A's native arrays, uploaded for the factorisation */
	int lnnz, unnz;
	int serial;                                /* some row of A stores a column twice (liship_ilu_t.serial) */
	int *lp, *lc, *up, *uc;                    /* host: the pattern in term order */
	int *d_lp, *d_lc, *d_up, *d_uc, *d_uskey, *d_uspos;     /* HBM (d_uskey == d_uc and d_uspos NULL when U's rows are ascending) */
	double *d_lval, *d_uval, *d_d;             /* HBM: the factor */
	lisi_sweep_t sched;                        /* the rows by forward level; long rows: L + U terms >= LISHIP_SWEEP_LONG_ROW */
	lisi_sweep_t sw[SW_COUNT];
	int *d_src[SW_COUNT];                      /* HBM, per place of a layout: the index into lval (L, L^T) or uval (U, U^T) */
	int factored;
	double symbolic_s;
} ilu_entry;

typedef struct {
	ilu_entry e[2];                            /* the (fill, T) pairs in use */
	int next;
} lisd_ilu;

#define ENTRY_BS(e) ((size_t)((e)->bn * (e)->bn))      /* doubles per place of the pattern */

static void entry_free(ilu_entry *e)
{
	free(e->lp); free(e->lc); free(e->up); free(e->uc);
	(void)liship_free(e->d_lp); (void)liship_free(e->d_lc); (void)liship_free(e->d_up);
	if (e->d_uskey != e->d_uc) (void)liship_free(e->d_uskey);
	(void)liship_free(e->d_uc); (void)liship_free(e->d_uspos);
	(void)liship_free(e->d_lval); (void)liship_free(e->d_uval); (void)liship_free(e->d_d);
	(void)liship_free(e->d_ap); (void)liship_free(e->d_ai); (void)liship_free(e->d_av);
	lisi_sweep_free(&e->sched);
	for (int w = 0; w < SW_COUNT; w++) { lisi_sweep_free(&e->sw[w]); (void)liship_free(e->d_src[w]); }
	memset(e, 0, sizeof(*e));
}

void lisd_ilu_free(void *p)
{
	lisd_ilu *il = (lisd_ilu *)p;
	if (!il) return;
	entry_free(&il->e[0]); entry_free(&il->e[1]);
	free(il);
}

/* ------------------------------------------------------------------ symbolic step */
typedef struct { int *v; size_t len, cap; } ivec;
static int ivec_push(ivec *a, const int *src, size_t count)
{
	if (a->len + count + 1 > a->cap) {
		size_t cap = a->cap ? a->cap : 1024;
		while (cap < a->len + count + 1) cap *= 2;
		int *v = (int *)realloc(a->v, cap * sizeof(int));
		if (!v) return 1;
		a->v = v; a->cap = cap;
	}
	if (count) memcpy(a->v + a->len, src, count * sizeof(int));
	a->len += count;
	return 0;
}

/* pattern of L and U of the n x n matrix (ptr, idx) at fill level `fill` under T row blocks */
static LIS_INT symbolic(ilu_entry *e, int n, const int *ptr, const int *idx, int fill, int T)
{
	LIS_INT err = LIS_SUCCESS;
	ivec L = {0}, U = {0}, Ulev = {0};
	int maxrow = 0;
	for (int i = 0; i < n; i++) if (ptr[i + 1] - ptr[i] > maxrow) maxrow = ptr[i + 1] - ptr[i];
	const size_t cap = (size_t)n + (size_t)maxrow + 2;
	int *blk = lisi_block_of(n, T);
	int *where = (int *)malloc(sizeof(int) * (size_t)(n + 1));       /* column -> its place in the row being built (L: lc, U: uc), -1: none */
	int *lc = (int *)malloc(sizeof(int) * cap), *ll = (int *)malloc(sizeof(int) * cap);
	int *uc = (int *)malloc(sizeof(int) * cap), *ul = (int *)malloc(sizeof(int) * cap);
	e->lp = (int *)calloc((size_t)n + 2, sizeof(int)); e->up = (int *)calloc((size_t)n + 2, sizeof(int));
	if (!blk || !where || !lc || !ll || !uc || !ul || !e->lp || !e->up) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); goto out; }
	for (int i = 0; i < n; i++) where[i] = -1;
	for (int i = 0; i < n; i++) {
		int nl = 0, nu = 0, ndiag = 0;
		for (int k = ptr[i]; k < ptr[i + 1]; k++) {
			const int c = idx[k];
			if (c < 0 || c >= n || blk[c] != blk[i]) continue;
			if (c == i) { if (++ndiag > 1) e->serial = 1; continue; }
			if (where[c] != -1) e->serial = 1;
			if (c < i) { lc[nl] = c; ll[nl] = 0; where[c] = nl++; }
			else { uc[nu] = c; ul[nu] = 0; where[c] = nu++; }
		}
		for (int p = 0; p < nl; p++) {
			int m = p;
			for (int q = p + 1; q < nl; q++) if (lc[q] < lc[m]) m = q;
			if (m != p) {
				const int cp = lc[p], cm = lc[m], t = ll[p];
				lc[p] = cm; lc[m] = cp; ll[p] = ll[m]; ll[m] = t;
				where[cm] = p; where[cp] = m;
			}
			const int piv = lc[p], plev = ll[p];
			const int *pc = U.v + e->up[piv], *pl = Ulev.v + e->up[piv];
			const int pn = e->up[piv + 1] - e->up[piv];
			for (int k = 0; k < pn; k++) {
				const int c = pc[k], lev = pl[k] + plev + 1;
				if (lev > fill) continue;
				if (c == i) continue;
				const int at = where[c];
				if (at == -1) {
					if ((size_t)(c < i ? nl : nu) + 1 >= cap) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "row %D of the ILU pattern outgrew its buffer\n", (LIS_INT)i); goto out; }
					if (c < i) { lc[nl] = c; ll[nl] = lev; where[c] = nl++; }
					else { uc[nu] = c; ul[nu] = lev; where[c] = nu++; }
				} else if (c < i) { if (lev < ll[at]) ll[at] = lev; }
				else { if (lev < ul[at]) ul[at] = lev; }
			}
		}
		for (int k = 0; k < nl; k++) where[lc[k]] = -1;
		for (int k = 0; k < nu; k++) where[uc[k]] = -1;
		if (ivec_push(&L, lc, (size_t)nl) || ivec_push(&U, uc, (size_t)nu) || ivec_push(&Ulev, ul, (size_t)nu) || L.len > 0x7fffffff || U.len > 0x7fffffff) {
			err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the ILU pattern does not fit (row %D)\n", (LIS_INT)i); goto out;
		}
		e->lp[i + 1] = (int)L.len; e->up[i + 1] = (int)U.len;
	}
	if (!L.v && ivec_push(&L, NULL, 0)) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc\n"); goto out; }
	if (!U.v && ivec_push(&U, NULL, 0)) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc\n"); goto out; }
	e->lc = L.v; L.v = NULL; e->uc = U.v; U.v = NULL;
	e->lnnz = (int)L.len; e->unnz = (int)U.len;
out:
	free(blk); free(where); free(lc); free(ll); free(uc); free(ul); free(L.v); free(U.v); free(Ulev.v);
	return err;
}

static int cmp_ll(const void *a, const void *b)
{
	const long long x = *(const long long *)a, y = *(const long long *)b;
	return x < y ? -1 : x > y;
}

/* uskey / uspos: every row of U ascending (ties by place) with the places; nothing when the rows are ascending already */
static LIS_INT upload_search_keys(ilu_entry *e)
{
	const int n = e->n;
	int sorted = 1;
	for (int i = 0; i < n && sorted; i++)
		for (int k = e->up[i] + 1; k < e->up[i + 1]; k++) if (e->uc[k] < e->uc[k - 1]) { sorted = 0; break; }
	if (sorted) { e->d_uskey = e->d_uc; e->d_uspos = NULL; return LIS_SUCCESS; }
	int maxrow = 0;
	for (int i = 0; i < n; i++) if (e->up[i + 1] - e->up[i] > maxrow) maxrow = e->up[i + 1] - e->up[i];
	int *key = (int *)malloc(sizeof(int) * (size_t)(e->unnz + 1)), *pos = (int *)malloc(sizeof(int) * (size_t)(e->unnz + 1));
	long long *tmp = (long long *)malloc(sizeof(long long) * (size_t)(maxrow + 1));
	LIS_INT err = LIS_SUCCESS;
	if (!key || !pos || !tmp) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)e->unnz); goto out; }
	for (int i = 0; i < n; i++) {
		const int u0 = e->up[i], len = e->up[i + 1] - u0;
		for (int k = 0; k < len; k++) tmp[k] = ((long long)e->uc[u0 + k] << 32) | (long long)(u0 + k);
		qsort(tmp, (size_t)len, sizeof(long long), cmp_ll);
		for (int k = 0; k < len; k++) { key[u0 + k] = (int)(tmp[k] >> 32); pos[u0 + k] = (int)(tmp[k] & 0x7fffffff); }
	}
	if ((err = lisd_upload_i(&e->d_uskey, key, (size_t)e->unnz)) || (err = lisd_upload_i(&e->d_uspos, pos, (size_t)e->unnz))) goto out;
	{	int rc = liship_stream_synchronize(lisg.stream);
		if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
out:
	free(key); free(pos); free(tmp);
	return err;
}

/* one of the four layouts, with the permutation that brings the factor's values into it (the pattern is block-filtered already) */
static LIS_INT sweep_make(ilu_entry *e, int which)
{
	const int n = e->n, lower = which == SW_L || which == SW_LT, nnz = lower ? e->lnnz : e->unnz;
	int *src = NULL, *tp = NULL, *tc = NULL, *tid = NULL;
	LIS_INT err;
	if ((err = lisi_sweep_terms(n, lower ? e->lp : e->up, lower ? e->lc : e->uc, NULL, SW_TERMS(which), &tp, &tc, &tid))) goto out;
	if ((err = lisi_sweep_build_places(&e->sw[which], n, tp, tc, NULL, SW_DESC(which), NULL, &src, (int)ENTRY_BS(e)))) goto out;   /* a place holds a block */
	for (int k = 0; k < nnz; k++) src[k] = tid[src[k]];
	if ((err = lisd_upload_i(&e->d_src[which], src, (size_t)nnz))) goto out;
	{	int rc = liship_stream_synchronize(lisg.stream);
		if (rc) err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	/* per (block) row: b and x, and the diagonal (block) where the sweep has one */
	e->sw[which].bytes = lisi_sweep_bytes_places(n, nnz, (int)ENTRY_BS(e), 16.0 * (double)e->bn + (lower ? 0.0 : 8.0 * (double)ENTRY_BS(e)));
out:
	free(src); free(tp); free(tc); free(tid);
	if (err) { lisi_sweep_free(&e->sw[which]); (void)liship_free(e->d_src[which]); e->d_src[which] = NULL; }
	return err;
}

static LIS_INT fill_sweep(ilu_entry *e, int which)
{
	const int nnz = e->sw[which].k.nnz;
	const double *from = (which == SW_L || which == SW_LT) ? e->d_lval : e->d_uval;
	if (nnz > 0 && e->bn == 1) HIPCHK(liship_permute_gather_f64(nnz, e->d_src[which], from, e->sw[which].val, lisg.stream));
	else if (nnz > 0) HIPCHK(liship_block_gather_f64(nnz, (int)ENTRY_BS(e), e->d_src[which], from, e->sw[which].val, lisg.stream));
	return LIS_SUCCESS;
}

static LIS_INT get_sweep(ilu_entry *e, int which, const liship_sweep_t **out)
{
	if (!e->sw[which].built) {
		const double t0 = lis_wtime();
		LISCHK(sweep_make(e, which));
		e->symbolic_s += lis_wtime() - t0;
		if (e->factored) LISCHK(fill_sweep(e, which));
	}
	*out = &e->sw[which].k;
	return LIS_SUCCESS;
}

/* A's pattern on the host: its own arrays, or a copy brought home when the matrix lives in HBM only */
static LIS_INT host_pattern(LIS_MATRIX A, int **ptr, int **idx, int *owned)
{
	lisd_mat *d = MDEV(A);
	*owned = 0;
	if (A->matrix_type == LIS_MATRIX_BSR) {      /* the block graph (a BSR matrix always has host arrays; those of a conversion in HBM come home here) */
		LISCHK(lisp_fill_matrix(A));
		if (!A->bptr || (!A->bindex && A->bnnz > 0)) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A has no BSR arrays\n");
		*ptr = A->bptr; *idx = A->bindex;
		return LIS_SUCCESS;
	}
	if (!d->device_only) {
		LISCHK(lisp_fill_matrix(A));
		if (A->ptr && (A->index || A->nnz == 0)) { *ptr = A->ptr; *idx = A->index; return LIS_SUCCESS; }
	}
	const size_t n = (size_t)A->n;
	*ptr = (int *)malloc(sizeof(int) * (n + 1));
	if (!*ptr) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", A->n);
	LIS_INT err = lisd_staged_d2h(*ptr, d->ptr, sizeof(int) * (n + 1));
	const size_t nnz = err ? 0 : (size_t)(*ptr)[n];
	*idx = (int *)malloc(sizeof(int) * (nnz + 1));
	if (!err && !*idx) err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)nnz);
	if (!err && nnz) err = lisd_staged_d2h(*idx, d->index, sizeof(int) * nnz);
	if (err) { free(*ptr); free(*idx); *ptr = NULL; *idx = NULL; return err; }
	*owned = 1;
	return LIS_SUCCESS;
}

static LIS_INT entry_build(LIS_MATRIX A, ilu_entry *e, int fill, int T)
{
	const int block = A->matrix_type == LIS_MATRIX_BSR;
	const int n = block ? A->nr : A->n;
	int *ptr = NULL, *idx = NULL, owned = 0;
	int *weight = NULL;
	LIS_INT err;
	const double t0 = lis_wtime();
	e->used = 1; e->fill = fill; e->T = T; e->n = n; e->bsr = block; e->bn = block ? A->bnr : 1; e->an = A->n;
	if ((long long)n * (long long)ENTRY_BS(e) >= 0x7fffffffLL) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the ILU factor does not fit\n"); goto out; }
	if ((err = host_pattern(A, &ptr, &idx, &owned))) goto out;
	if ((err = symbolic(e, n, ptr, idx, fill, T))) goto out;
	weight = (int *)malloc(sizeof(int) * (size_t)(n + 1));
	if (!weight) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)n); goto out; }
	for (int i = 0; i < n; i++) weight[i] = (e->lp[i + 1] - e->lp[i]) + (e->up[i + 1] - e->up[i]);
	if ((err = lisi_sweep_build(&e->sched, n, e->lp, e->lc, NULL, 0, weight, NULL))) goto out;
	if ((err = lisd_upload_i(&e->d_lp, e->lp, (size_t)n + 1)) || (err = lisd_upload_i(&e->d_lc, e->lc, (size_t)e->lnnz)) ||
	    (err = lisd_upload_i(&e->d_up, e->up, (size_t)n + 1)) || (err = lisd_upload_i(&e->d_uc, e->uc, (size_t)e->unnz))) goto out;
	if (((long long)e->lnnz + e->unnz) * (long long)ENTRY_BS(e) >= 0x7fffffffLL) { err = LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "the ILU factor does not fit\n"); goto out; }
	{	int rc = lisd_malloc((void **)&e->d_lval, ((size_t)e->lnnz * ENTRY_BS(e) + 2) * sizeof(double));
		if (!rc) rc = lisd_malloc((void **)&e->d_uval, ((size_t)e->unnz * ENTRY_BS(e) + 2) * sizeof(double));
		if (!rc) rc = lisd_malloc((void **)&e->d_d, ((size_t)n * ENTRY_BS(e) + 2) * sizeof(double));
		if (!rc) rc = liship_stream_synchronize(lisg.stream);
		if (rc) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto out; } }
	if ((err = upload_search_keys(e))) goto out;
	e->symbolic_s = lis_wtime() - t0;
out:
	if (owned) { free(ptr); free(idx); }
	free(weight);
	if (err) entry_free(e);
	return err;
}

/* A: an assembled CSR matrix, or a BSR matrix with square blocks of 1 .. 3, not split, on one rank */
static LIS_INT check_served(LIS_MATRIX A, LIS_INT fill)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (A->matrix_type == LIS_MATRIX_BSR) {
		if (A->bnr != A->bnc) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu on %D x %D blocks is not served: block ILU wants square blocks (A is untouched)\n", A->bnr, A->bnc);
		if (A->bnr > 3 || A->bnr < 1)
			return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu on %D x %D blocks is not served: the reference's block sweeps hold a block's result in w[3] "
			                "(lis_precon_iluk.c:1977), which defines block ILU for blocks of 1, 2 and 3 only (A is untouched)\n", A->bnr, A->bnc);
		if (A->is_splited) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu on a split BSR matrix (an earlier -p bjacobi solve splits A) is not served: lis_matrix_merge(A) first (A is untouched)\n");
	} else if (A->matrix_type != LIS_MATRIX_CSR) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu is served for CSR and BSR storage only (A is untouched)\n");
	if (A->is_splited) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu on a split matrix (an earlier -p ssor solve splits A) is not served: lis_matrix_merge(A) first (A is untouched)\n");
	if (lisg.nprocs > 1) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu is served on one rank only (A is untouched)\n");
	if (fill < 0) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-ilu_fill %D is not served: the fill level is 0 or more (A is untouched)\n", fill);
	return LIS_SUCCESS;
}

/* -p ilu on BSR storage applies M^-1 only */
static LIS_INT check_solver(LIS_MATRIX A, LIS_SOLVER solver)
{
	if (A->matrix_type == LIS_MATRIX_BSR && lisi_solver_needs_transpose(solver->options[LIS_OPTIONS_SOLVER]))
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu on BSR storage with a solver that applies M^-H (-i %D) is not served: the reference's OpenMP build applies M^-1 there "
		                "(lis_precon_iluk.c:2098-2165), which this library neither reproduces nor replaces (A is untouched)\n", solver->options[LIS_OPTIONS_SOLVER]);
	return LIS_SUCCESS;
}

/* the cache entry of (fill, T) on the HBM copy of A, its symbolic part built on first use */
static LIS_INT get_entry(LIS_MATRIX A, int fill, int T, ilu_entry **out)
{
	LISCHK(lisd_mat_ready(A));
	lisd_mat *d = MDEV(A);
	const int block = A->matrix_type == LIS_MATRIX_BSR, rows = block ? A->nr : A->n;
	if (!block && (d->type != LIS_MATRIX_CSR || !d->ptr || (A->nnz > 0 && (!d->index || !d->value)))) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu needs the CSR arrays of A in HBM\n");
	if (!d->ilu) { d->ilu = calloc(1, sizeof(lisd_ilu)); if (!d->ilu) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(lisd_ilu)); }
	lisd_ilu *il = (lisd_ilu *)d->ilu;
	ilu_entry *e = NULL;
	for (int t = 0; t < 2; t++) if (il->e[t].used && il->e[t].fill == fill && il->e[t].T == T && il->e[t].n == rows && il->e[t].bsr == block && il->e[t].bn == (block ? A->bnr : 1)) e = &il->e[t];
	if (!e) {
		e = &il->e[il->next];
		il->next ^= 1;
		entry_free(e);
		LISCHK(entry_build(A, e, fill, T));
	}
	*out = e;
	return LIS_SUCCESS;
}

/* the numbers: A's values as they lie in HBM -> lval, uval, d, then into every layout built so far */
static LIS_INT factorise(LIS_MATRIX A, ilu_entry *e)
{
	lisd_mat *d = MDEV(A);
	liship_bilu_t f;
	memset(&f, 0, sizeof(f));
	f.n = e->an; f.nr = e->n; f.bn = e->bn; f.serial = e->serial;
	if (!e->bsr) { f.aptr = d->ptr; f.aindex = d->index; f.avalue = d->value; }
	else if (d->type == LIS_MATRIX_BSR && d->bptr && (A->bnnz == 0 || (d->bindex && d->value))) { f.aptr = d->bptr; f.aindex = d->bindex; f.avalue = d->value; }
	else {                                       /* the copy is held in its row form: A's native arrays, uploaded once per entry */
		if (!e->d_ap) {
			LISCHK(lisp_fill_matrix(A));
			LISCHK(lisd_upload_i(&e->d_ap, A->bptr, (size_t)e->n + 1));
			LISCHK(lisd_upload_i(&e->d_ai, A->bindex, (size_t)A->bnnz));
			LISCHK(lisd_upload_d(&e->d_av, A->value, (size_t)A->bnnz * ENTRY_BS(e)));
			HIPCHK(liship_stream_synchronize(lisg.stream));
		}
		f.aptr = e->d_ap; f.aindex = e->d_ai; f.avalue = e->d_av;
	}
	f.lptr = e->d_lp; f.lcol = e->d_lc; f.uptr = e->d_up; f.ucol = e->d_uc; f.uskey = e->d_uskey; f.uspos = e->d_uspos;
	f.lval = e->d_lval; f.uval = e->d_uval; f.d = e->d_d;
	HIPCHK(liship_bilu_factor_f64(&f, &e->sched.k, lisg.stream));
	e->factored = 1;
	for (int w = 0; w < SW_COUNT; w++) if (e->sw[w].built) LISCHK(fill_sweep(e, w));
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ create */
LIS_INT lisi_ilu_create(LIS_SOLVER solver, LIS_PRECON precon)
{
	LIS_MATRIX A = solver->A;
	const LIS_INT storage = solver->options[LIS_OPTIONS_STORAGE], fill = solver->options[LIS_OPTIONS_FILL];
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisd_init());                         /* no device: the no-device code, before anything that could succeed */
	/* refusals first: A is left as it was */
	if (storage && (storage != A->matrix_type || (storage != LIS_MATRIX_CSR && storage != LIS_MATRIX_BSR)))
		return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu is served for the CSR or BSR storage A already has, not with a conversion by -storage %D (A is untouched)\n", storage);
	if (solver->options[LIS_OPTIONS_SCALE] != LIS_SCALE_NONE) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu together with -scale is not served (A is untouched)\n");
	if (solver->options[LIS_OPTIONS_ADDS]) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "-p ilu with -adds true is not served (A is untouched)\n");
	LISCHK(check_served(A, fill));
	LISCHK(check_solver(A, solver));
	ilu_entry *e;
	LISCHK(get_entry(A, (int)fill, lisi_sweep_blocks(), &e));
	const liship_sweep_t *s;
	LISCHK(get_sweep(e, SW_L, &s));
	LISCHK(get_sweep(e, SW_U, &s));
	LISCHK(factorise(A, e));
	precon->A = A;
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ the solve's side (the ILU row of lisi_precon_kinds) */
LIS_INT lisd_ilu_begin(LIS_MATRIX A, LIS_SOLVER solver, lisi_precon_state *st)
{
	ilu_entry *e;
	const liship_sweep_t *f, *b;
	st->A = A; st->n = A->n; st->fill = (int)solver->options[LIS_OPTIONS_FILL]; st->T = lisi_sweep_blocks();
	LISCHK(check_served(A, st->fill));
	LISCHK(check_solver(A, solver));
	LISCHK(get_entry(A, st->fill, st->T, &e));
	LISCHK(get_sweep(e, SW_L, &f));
	LISCHK(get_sweep(e, SW_U, &b));
	if (!e->factored) LISCHK(factorise(A, e));   /* (the HBM copy was rebuilt since lis_precon_create) */
	lisg.last_ilu = 1; lisg.last_ilu_fill = st->fill; lisg.last_ilu_blocks = st->T; lisg.last_ilu_bn = e->bsr ? e->bn : 0;
	lisg.last_ilu_levels = f->nlev; lisg.last_ilu_launches = f->ngroups + b->ngroups;
	return LIS_SUCCESS;
}

#define NO_BSR_TRANSPOSE "M^-H of -p ilu on BSR storage is not served: the reference's OpenMP build applies M^-1 there\n"

/* x = M^-1 b: forward on L, backward on U and D (every bn); x = M^-H b (CSR storage): forward on U^T with D first, backward on L^T */
static LIS_INT apply_on(ilu_entry *e, int transposed, const double *b, double *x)
{
	const liship_sweep_t *first, *second;
	if (transposed && e->bsr) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, NO_BSR_TRANSPOSE);
	LISCHK(get_sweep(e, transposed ? SW_UT : SW_L, &first));
	LISCHK(get_sweep(e, transposed ? SW_LT : SW_U, &second));
	if (!transposed) {
		HIPCHK(liship_bilu_sweep_f64(first, e->an, e->bn, NULL, b, x, lisg.stream));
		HIPCHK(liship_bilu_sweep_f64(second, e->an, e->bn, e->d_d, x, x, lisg.stream));
	} else {
		HIPCHK(liship_sweep_f64(first, LISHIP_SWEEP_MUL, b, x, e->d_d, lisg.stream));
		HIPCHK(liship_sweep_plain_f64(second, x, x, lisg.stream));
	}
	return LIS_SUCCESS;
}

LIS_INT lisd_ilu_apply(const lisi_precon_state *st, int transposed, const double *b, double *x)
{	/* x = M^-1 b, or M^-H b (b may be x): get_entry finds the entry begin left, or makes it again on a copy that a product rebuilt in mid-solve */
	ilu_entry *e;
	LISCHK(get_entry(st->A, st->fill, st->T, &e));
	if (!e->factored) LISCHK(factorise(st->A, e));
	return apply_on(e, transposed, b, x);
}

/* ------------------------------------------------------------------ introspection and tools (include/lis_amd.h) */
LIS_INT lis_amd_last_solve_ilu(LIS_INT *fill, LIS_INT *blocks_out, LIS_INT *levels, LIS_INT *launches_per_psolve)
{
	if (fill) *fill = lisg.last_ilu ? lisg.last_ilu_fill : 0;
	if (blocks_out) *blocks_out = lisg.last_ilu ? lisg.last_ilu_blocks : 0;
	if (levels) *levels = lisg.last_ilu ? lisg.last_ilu_levels : 0;
	if (launches_per_psolve) *launches_per_psolve = lisg.last_ilu ? lisg.last_ilu_launches : 0;
	return lisg.last_ilu;
}

LIS_INT lis_amd_last_solve_ilu_block(void) { return lisg.last_ilu ? lisg.last_ilu_bn : 0; }

static LIS_INT tool_entry(LIS_MATRIX A, LIS_INT fill, ilu_entry **e)
{
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	LISCHK(lisd_init());
	LISCHK(check_served(A, fill));
	return get_entry(A, (int)fill, lisi_sweep_blocks(), e);
}

LIS_INT lis_amd_ilu_factor(LIS_MATRIX A, LIS_INT fill, LIS_INT sizes[3])
{
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	LISCHK(factorise(A, e));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	if (sizes) { sizes[0] = e->n; sizes[1] = e->lnnz; sizes[2] = e->unnz; }
	return LIS_SUCCESS;
}

LIS_INT lis_amd_ilu_copy(LIS_MATRIX A, LIS_INT fill, LIS_INT *lptr, LIS_INT *lindex, LIS_SCALAR *lvalue,
                         LIS_INT *uptr, LIS_INT *uindex, LIS_SCALAR *uvalue, LIS_SCALAR *d)
{
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	if (!e->factored) LISCHK(factorise(A, e));
	const size_t n = (size_t)e->n;
	if (lptr) memcpy(lptr, e->lp, sizeof(int) * (n + 1));
	if (uptr) memcpy(uptr, e->up, sizeof(int) * (n + 1));
	if (lindex && e->lnnz) memcpy(lindex, e->lc, sizeof(int) * (size_t)e->lnnz);
	if (uindex && e->unnz) memcpy(uindex, e->uc, sizeof(int) * (size_t)e->unnz);
	HIPCHK(liship_stream_synchronize(lisg.stream));
	if (lvalue && e->lnnz) LISCHK(lisd_staged_d2h(lvalue, e->d_lval, sizeof(double) * (size_t)e->lnnz * ENTRY_BS(e)));
	if (uvalue && e->unnz) LISCHK(lisd_staged_d2h(uvalue, e->d_uval, sizeof(double) * (size_t)e->unnz * ENTRY_BS(e)));
	if (d && n) LISCHK(lisd_staged_d2h(d, e->d_d, sizeof(double) * n * ENTRY_BS(e)));
	return LIS_SUCCESS;
}

LIS_INT lis_amd_ilu_psolve(LIS_MATRIX A, LIS_INT fill, LIS_VECTOR B, LIS_VECTOR X, LIS_INT transposed)
{
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	if (B->n != A->n || X->n != A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match\n");
	if (e->bsr && transposed) return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, NO_BSR_TRANSPOSE);
	if (!e->factored) LISCHK(factorise(A, e));
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	if (X == B) dx = db;
	else LISCHK(lisd_vec_out(X, &dx));
	LISCHK(apply_on(e, transposed != 0, db, dx));
	return lisd_vec_done(X);
}

typedef struct { LIS_MATRIX A; ilu_entry *e; const double *b; double *x; } timed_args;
static LIS_INT factorise_once(void *ctx) { const timed_args *t = (const timed_args *)ctx; return factorise(t->A, t->e); }
static LIS_INT psolve_once(void *ctx) { const timed_args *t = (const timed_args *)ctx; return apply_on(t->e, 0, t->b, t->x); }

LIS_INT lis_amd_ilu_times(LIS_MATRIX A, LIS_INT fill, LIS_VECTOR B, LIS_VECTOR X, LIS_INT reps, double *factor_ms, double *psolve_ms)
{	/* reps factorisations and reps psolves X = M^-1 B on the library's stream, each timed by device events */
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	if (B->n != A->n || X->n != A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "sizes of A, B and X do not match\n");
	const liship_sweep_t *s;
	LISCHK(get_sweep(e, SW_L, &s));
	LISCHK(get_sweep(e, SW_U, &s));
	double *db, *dx;
	LISCHK(lisd_vec_in(B, &db));
	LISCHK(lisd_vec_out(X, &dx));
	timed_args args = {A, e, db, dx};
	LISCHK(lisi_sweep_times(reps, factorise_once, &args, factor_ms));
	LISCHK(lisi_sweep_times(reps, psolve_once, &args, psolve_ms));
	return lisd_vec_done(X);
}

LIS_INT lis_amd_ilu_info(LIS_MATRIX A, LIS_INT fill, double info[6])
{	/* {host seconds of the symbolic step and the layouts, nnz(L) + nnz(U), forward levels, launches of one factorisation as a solve
	 * with psolve alone pays it (level launches + the gathers into L and U; a solver that also calls psolveh adds two gathers),
	 * launches per psolve, bytes per psolve} at the current block count */
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	const liship_sweep_t *f, *b;
	LISCHK(get_sweep(e, SW_L, &f));
	LISCHK(get_sweep(e, SW_U, &b));
	info[0] = e->symbolic_s;
	info[1] = (double)e->lnnz + (double)e->unnz;
	info[2] = (double)e->sched.k.nlev;
	info[3] = (double)(e->sched.k.ngroups + (e->lnnz > 0) + (e->unnz > 0));
	info[4] = (double)(f->ngroups + b->ngroups);
	info[5] = e->sw[SW_L].bytes + e->sw[SW_U].bytes;
	return LIS_SUCCESS;
}

LIS_INT lis_amd_ilu_factor_info(LIS_MATRIX A, LIS_INT fill, LIS_INT info[6])
{	/* the factorisation's schedule, read-only: {levels, launches, levels on a launch of their own, rows given to a workgroup in
	 * those levels, rows given to a workgroup inside runs of small levels, 1 when such rows are factorised by one thread} */
	ilu_entry *e;
	LISCHK(tool_entry(A, fill, &e));
	lisi_sweep_census(&e->sched.k, info);
	info[5] = e->serial;
	return LIS_SUCCESS;
}
