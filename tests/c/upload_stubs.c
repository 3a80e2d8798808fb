/* Test stubs for everything lis_amd/csrc/host/lis_upload.c and lis_convert_hbm.c call (tests/test_upload_paths_cpu.py): each appends its short name and its
 * scalar arguments (sizes, widths, block sizes, never pointers) to stub_log and returns 0, or the code scripted for that hit (stub_script).  One line per
 * signature.  "HBM" is calloc memory behind a table of live allocations: copies really copy (a sanitizer build sees their bounds), a free of something that is
 * not live aborts.  Live plans and live lazy host arrays are counted the same way.  The stubs that answer facts (how many value records, the longest row ...)
 * say what the stub_* switches tell them and log nothing. */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "lis_internal.h"

lisi_globals lisg;
char stub_log[16384];
int stub_value_records, stub_coded, stub_maxlen, stub_unsorted, stub_nnd, stub_bnnz, stub_rnnz;
static const char *scripted_name; static int scripted_hit, scripted_code, seen;

/* ---- the log and the script: the k-th hit of the stub called `name` answers `code` */
void stub_reset(void)
{
	stub_log[0] = 0; scripted_name = NULL; seen = 0;
	stub_value_records = 1; stub_coded = 1; stub_maxlen = 2; stub_unsorted = 0; stub_nnd = 2; stub_bnnz = 5; stub_rnnz = 11;
}
void stub_script(const char *name, int k, int code)
{
	static char kept[64];
	snprintf(kept, sizeof(kept), "%s", name);
	scripted_name = kept; scripted_hit = k; scripted_code = code; seen = 0;
}
static int hit(const char *name, const char *fmt, ...)
{
	size_t at = strlen(stub_log);
	va_list ap;
	at += (size_t)snprintf(stub_log + at, sizeof(stub_log) - at, "%s%s", at ? " " : "", name);
	va_start(ap, fmt);
	vsnprintf(stub_log + at, sizeof(stub_log) - at, fmt, ap);
	va_end(ap);
	return (scripted_name && !strcmp(scripted_name, name) && ++seen == scripted_hit) ? scripted_code : 0;
}

/* ---- live allocations, plans, lazy arrays */
#define LIVE_MAX 256
static void *live[LIVE_MAX], *plans[LIVE_MAX];
static struct { void *host, *dev; int own; } lazies[LIVE_MAX];
static int live_add(void **table, void *p) { for (int i = 0; i < LIVE_MAX; i++) if (!table[i]) { table[i] = p; return 1; } return 0; }
static void live_drop(void **table, void *p, const char *what)
{
	for (int i = 0; i < LIVE_MAX; i++) if (table[i] == p) { table[i] = NULL; free(p); return; }
	fprintf(stderr, "upload_stubs: %s of %p, which is not live (freed twice, or never allocated)\n", what, p);
	abort();
}
static int live_count(void **table) { int c = 0; for (int i = 0; i < LIVE_MAX; i++) c += table[i] != NULL; return c; }
int stub_live_allocations(void) { return live_count(live); }
int stub_live_plans(void) { return live_count(plans); }
int stub_live_lazy(void) { int c = 0; for (int i = 0; i < LIVE_MAX; i++) c += lazies[i].host != NULL; return c; }
void stub_forget(void)                                          /* what a case left alive does not count against the next one */
{
	for (int i = 0; i < LIVE_MAX; i++) { free(live[i]); free(plans[i]); free(lazies[i].host); live[i] = plans[i] = lazies[i].host = NULL; }
}
static void *device_room(size_t bytes) { void *p = calloc(bytes ? bytes : 16, 1); if (p && !live_add(live, p)) abort(); return p; }

int liship_malloc(void **dptr, size_t bytes)
{
	const int rc = hit("malloc", "(%zu)", bytes);
	*dptr = rc ? NULL : device_room(bytes);
	return rc;
}
int liship_free(void *dptr) { if (dptr) { hit("free", "%s", ""); live_drop(live, dptr, "liship_free"); } return 0; }
int lisd_malloc(void **out, size_t bytes)                       /* as lis_device.c */
{
	int rc = liship_malloc(out, bytes);
	if (rc && lis_amd_trim_count() > 0) rc = liship_malloc(out, bytes);
	return rc;
}
int lis_amd_trim_count(void) { hit("trim", "%s", ""); return 0; }

#define COPY(name, tag) int name(void *dst, const void *src, size_t bytes, void *stream) { const int rc = hit(tag, "(%zu)", bytes); if (!rc) memcpy(dst, src, bytes); return rc; }
COPY(liship_memcpy_h2d, "h2d") COPY(liship_memcpy_d2h, "d2h") COPY(liship_memcpy_d2d, "d2d")
#define STUB(type, name, tag, params, ...) type name params { return hit(tag, __VA_ARGS__); }
#define P liship_csr_plan_t p
#define CSR const int *ptr, const int *idx, const double *val
STUB(int, liship_stream_synchronize, "sync", (void *stream), "%s", "")

/* ---- plans */
int liship_csr_plan_create(liship_csr_plan_t *plan, int n, const int *ptr, void *stream)
{
	const int rc = hit("plan", "(%d)", n);
	if (!rc) { *plan = (liship_csr_plan_t)malloc(1); if (!live_add(plans, (void *)*plan)) abort(); }
	return rc;
}
int liship_csr_plan_destroy(P) { hit("destroy", "%s", ""); live_drop(plans, (void *)p, "liship_csr_plan_destroy"); return 0; }
STUB(int, liship_csr_plan_set_ghost_columns, "ghost", (P, int ncols), "(%d)", ncols)
STUB(int, liship_csr_plan_encode_indices, "enc_idx", (P, const int *ptr, const int *idx, void *stream), "%s", "")
STUB(int, liship_csr_plan_encode_row_patterns, "enc_pat", (P, const int *ptr, void *stream), "%s", "")
STUB(int, liship_csr_plan_encode_row_values, "enc_val", (P, const int *ptr, const double *val, void *stream), "%s", "")
STUB(int, liship_csr_plan_encode_block_rows, "enc_blk", (P, int b, const int *ptr, void *stream), "(%d)", b)
STUB(int, liship_spmv_csr_set_local_short_rows, "short_rows", (int on), "(%d)", on)
STUB(int, liship_csr_plan_localize_columns, "localize", (P, const int *ptr, const int *idx, void *stream), "%s", "")
STUB(int, liship_csr_plan_scan_band, "band", (P, const int *ptr, const int *idx, void *stream), "%s", "")
STUB(int, liship_csr_plan_set_first_term_initialises, "first_term", (P, int on), "(%d)", on)
STUB(int, liship_csr_plan_reorder_with, "reorder", (P, CSR, int min_items, const int *hint, void *stream), "%s", "")
int liship_csr_plan_reorder_permutation(P, int *perm) { return 1; }
int liship_csr_plan_info(P, int *n, long long *nnz, int *nblocks) { if (nnz) *nnz = 0; return 0; }
int liship_csr_plan_value_records(P) { return stub_value_records; }
int liship_csr_plan_coded(P) { return stub_coded; }
#define FACT0(type, name) type name(P) { return 0; }
FACT0(int, liship_csr_plan_row_patterns) FACT0(int, liship_csr_plan_pattern_records) FACT0(int, liship_csr_plan_dominant_pattern) FACT0(int, liship_csr_plan_wide_dominant)
FACT0(int, liship_csr_plan_strip_rows) FACT0(int, liship_csr_plan_block_rows) FACT0(int, liship_csr_plan_block2_march) FACT0(int, liship_csr_plan_box27)
FACT0(int, liship_csr_plan_marching) FACT0(int, liship_csr_plan_lists_failed) FACT0(long long, liship_csr_plan_localized) FACT0(long long, liship_csr_plan_reordered)

/* ---- kernels/convert.hip, transpose.hip, spmv_formats.hip */
int liship_csr_row_facts(int n, const int *ptr, const int *idx, int *facts, void *stream)
{
	const int rc = hit("row_facts", "(%d)", n);
	if (!rc) { facts[0] = stub_maxlen; facts[1] = stub_unsorted; }
	return rc;
}
STUB(int, liship_csr_to_ell, "to_ell", (int n, int maxnzr, CSR, int *eidx, double *eval, void *stream), "(%d,%d)", n, maxnzr)
STUB(int, liship_csr_to_ell_rows, "to_ell_rows", (int n, int maxnzr, CSR, int *rptr, int *ridx, double *rval, void *stream), "(%d,%d)", n, maxnzr)
STUB(int, liship_ell_scan_band, "ell_band", (int n, int maxnzr, const int *idx, int *plane, void *stream), "(%d,%d)", n, maxnzr)
int liship_ell_encode_indices(int n, int maxnzr, const int *idx, unsigned char **codes, int **dict, int *ndict, void *stream)
{
	const int rc = hit("ell_codes", "(%d,%d)", n, maxnzr);
	if (!rc) { *codes = (unsigned char *)device_room((size_t)n * (size_t)maxnzr); *dict = (int *)device_room(1024); *ndict = 1; }
	return rc;
}
int liship_csr_dia_offsets(int n, int ncols, const int *ptr, const int *idx, int *used, int *slot, long long *scratch, int *nnd, void *stream)
{
	const int rc = hit("dia_offsets", "(%d,%d)", n, ncols);
	if (!rc) *nnd = stub_nnd;
	return rc;
}
STUB(int, liship_csr_to_dia, "to_dia", (int n, int ncols, int nnd, CSR, const int *used, const int *slot, int *offs, double *dval, void *stream), "(%d,%d,%d)", n, ncols, nnd)
int liship_dia_row_counts(int n, int ncols, int nnd, const int *offs, int *count, int *rptr, long long *scratch, int *rnnz, void *stream)
{
	const int rc = hit("dia_counts", "(%d,%d,%d)", n, ncols, nnd);
	if (!rc) *rnnz = stub_rnnz;
	return rc;
}
STUB(int, liship_dia_to_rows, "dia_to_rows", (int n, int ncols, int nnd, const int *offs, const double *dval, const int *rptr, int *ridx, double *rval, void *stream), "(%d,%d,%d)", n, ncols, nnd)
STUB(int, liship_csr_transpose_f64, "transpose", (int nrows, int ncols, int nnz, CSR, int *tptr, int *tidx, double *tval, int *work, void *stream), "(%d,%d,%d)", nrows, ncols, nnz)
STUB(int, liship_csr_to_jad, "to_jad", (int n, const int *perm, const int *jptr, CSR, int *jidx, double *jval, void *stream), "(%d)", n)
int liship_csr_bsr_count(int n, int np, int bnr, int bnc, const int *ptr, const int *idx, int *count, int *bptr, long long *scratch, int *bnnz, void *stream)
{
	const int rc = hit("bsr_count", "(%d,%d,%d,%d)", n, np, bnr, bnc);
	if (!rc) *bnnz = stub_bnnz;
	return rc;
}
STUB(int, liship_csr_to_bsr, "to_bsr", (int n, int bnr, int bnc, int bnnz, CSR, const int *bptr, int *bidx, double *bval, void *stream), "(%d,%d,%d,%d)", n, bnr, bnc, bnnz)
STUB(int, liship_bsr_to_rows, "bsr_to_rows", (int n, int bnr, int bnc, const int *bptr, const int *bidx, const double *bval, int *rptr, int *ridx, double *rval, void *stream), "(%d,%d,%d)", n, bnr, bnc)

/* ---- lis_pages.c */
void *lisp_alloc_lazy(void *matrix, size_t bytes, void *dev, int own)
{
	if (hit("lazy", "(%zu,own=%d)", bytes, own)) return NULL;
	for (int i = 0; i < LIVE_MAX; i++) if (!lazies[i].host) { lazies[i].host = malloc(bytes ? bytes : 1); lazies[i].dev = dev; lazies[i].own = own; return lazies[i].host; }
	abort();
}
int lisp_free_array(void *p)                                    /* frees an owned buffer, as the real one does */
{
	for (int i = 0; p && i < LIVE_MAX; i++) if (lazies[i].host == p) {
		if (lazies[i].dev && lazies[i].own) (void)liship_free(lazies[i].dev);
		free(p); lazies[i].host = NULL;
		return 1;
	}
	return 0;
}
STUB(LIS_INT, lisp_fill_matrix, "fill", (void *matrix), "%s", "")
STUB(int, lisp_adopt, "adopt", (void *matrix, void *array), "%s", "")
STUB(int, lisp_matrix_protect, "protect", (void *matrix), "%s", "")
void lisp_matrix_release(void *matrix, int forget) { hit("release", "%s", ""); }
int lisp_lazy_arrays(void *matrix) { return 0; }

/* ---- the rest of the host layer */
STUB(LIS_INT, lisd_init, "init", (void), "%s", "")
int lisi_host_threads(void) { return 1; }
void lisi_precon_release(lisd_mat *d, LIS_MATRIX A, LIS_PRECON precon) { }
LIS_INT lisi_hip_error(const char *file, const char *func, int line, int hipcode) { hit("hip_error", "(%d)", hipcode); return hipcode == 2 ? LIS_ERR_OUT_OF_MEMORY : LIS_AMD_ERR_DEVICE; }
LIS_INT lisi_error(const char *file, const char *func, int line, LIS_INT code, const char *fmt, ...) { hit("lis_error", "(%d)", (int)code); return code; }
/* the rows lis_split.c hands to the upload: `rows` rows, the first two of one entry each, heap memory that the upload frees */
static void split_part(int rows, LIS_INT **ptr, LIS_INT **idx, LIS_SCALAR **val)
{
	*ptr = (LIS_INT *)calloc((size_t)rows + 1, sizeof(LIS_INT)); *idx = (LIS_INT *)calloc(2, sizeof(LIS_INT)); *val = (LIS_SCALAR *)calloc(2, sizeof(LIS_SCALAR));
	for (int i = 1; i <= rows; i++) (*ptr)[i] = i < 2 ? i : 2;
	(*idx)[1] = 1;
}
LIS_INT lisi_split_rows(LIS_MATRIX A, LIS_INT *rows, LIS_INT **ptr, LIS_INT **idx, LIS_SCALAR **val, int *from_zero) { hit("split_rows", "%s", ""); *rows = 2; *from_zero = 0; split_part(2, ptr, idx, val); return 0; }
LIS_INT lisi_split_jad_part(LIS_MATRIX A, int upper, LIS_INT **ptr, LIS_INT **idx, LIS_SCALAR **val) { hit("split_jad_part", "(%d)", upper); split_part(A->n, ptr, idx, val); return 0; }
LIS_INT lisi_jad_order(LIS_MATRIX A, LIS_INT *maxnzr, LIS_INT **perm, LIS_INT **ptr)
{
	hit("jad_order", "%s", "");
	*maxnzr = 2; *perm = (LIS_INT *)calloc((size_t)A->n, sizeof(LIS_INT)); *ptr = (LIS_INT *)calloc(3, sizeof(LIS_INT));
	return 0;
}
/* lis_matrix_set_<fmt>: the header holds the arrays from here on */
LIS_INT lis_matrix_set_ell(LIS_INT maxnzr, LIS_INT *idx, LIS_SCALAR *val, LIS_MATRIX A) { A->maxnzr = maxnzr; A->index = idx; A->value = val; return hit("set_ell", "(%d)", maxnzr); }
LIS_INT lis_matrix_set_dia(LIS_INT nnd, LIS_INT *idx, LIS_SCALAR *val, LIS_MATRIX A) { A->nnd = nnd; A->index = idx; A->value = val; return hit("set_dia", "(%d)", nnd); }
LIS_INT lis_matrix_set_csc(LIS_INT nnz, LIS_INT *ptr, LIS_INT *idx, LIS_SCALAR *val, LIS_MATRIX A) { A->nnz = nnz; A->ptr = ptr; A->index = idx; A->value = val; return hit("set_csc", "(%d)", nnz); }
LIS_INT lis_matrix_set_jad(LIS_INT nnz, LIS_INT maxnzr, LIS_INT *perm, LIS_INT *ptr, LIS_INT *idx, LIS_SCALAR *val, LIS_MATRIX A)
{
	A->nnz = nnz; A->maxnzr = maxnzr; A->row = perm; A->ptr = ptr; A->index = idx; A->value = val;
	return hit("set_jad", "(%d,%d)", nnz, maxnzr);
}
LIS_INT lis_matrix_set_bsr(LIS_INT bnr, LIS_INT bnc, LIS_INT bnnz, LIS_INT *bptr, LIS_INT *bidx, LIS_SCALAR *val, LIS_MATRIX A)
{
	A->bnr = bnr; A->bnc = bnc; A->bnnz = bnnz; A->nc = 1 + (A->n - 1) / bnc; A->bptr = bptr; A->bindex = bidx; A->value = val;
	return hit("set_bsr", "(%d,%d,%d)", bnr, bnc, bnnz);
}
STUB(LIS_INT, lis_matrix_assemble, "assemble", (LIS_MATRIX A), "%s", "")
/* the host arrays a matrix header holds, then its HBM copy (lis_matrix.c) */
LIS_INT lisi_matrix_storage_destroy(LIS_MATRIX A)
{
	void *arr[] = {A->ptr, A->row, A->index, A->bptr, A->bindex, A->value};
	hit("storage_destroy", "%s", "");
	for (int k = 0; k < 6; k++) if (!lisp_free_array(arr[k])) free(arr[k]);
	A->ptr = A->row = A->index = A->bptr = A->bindex = NULL; A->value = NULL;
	lisd_mat_free(A);
	return 0;
}
/* lisd_csr_home's callees: not driven by the cases */
LIS_INT lis_matrix_duplicate(LIS_MATRIX Ain, LIS_MATRIX *Aout) { return LIS_ERR_NOT_IMPLEMENTED; }
LIS_INT lis_matrix_malloc_csr(LIS_INT n, LIS_INT nnz, LIS_INT **ptr, LIS_INT **idx, LIS_SCALAR **val) { return LIS_ERR_NOT_IMPLEMENTED; }
LIS_INT lis_matrix_set_csr(LIS_INT nnz, LIS_INT *ptr, LIS_INT *idx, LIS_SCALAR *val, LIS_MATRIX A) { return LIS_ERR_NOT_IMPLEMENTED; }
LIS_INT lis_matrix_destroy(LIS_MATRIX A) { return 0; }
void lis_free(void *p) { free(p); }
