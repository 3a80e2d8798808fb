/* Test stubs for everything lis_amd/csrc/host/lis_product.c calls (tests/test_product_dispatch_cpu.py): each appends its short name and its scalar
 * arguments to stub_log and returns the code scripted for that name (0 unless stub_script() said otherwise).  One STUB line per signature. */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "lis_internal.h"

lisi_globals lisg;
char stub_log[4096];
int stub_fused_dots = 1;                /* liship_csr_plan_fused_dots */
long long stub_fused_slots = 10;        /* liship_csr_plan_fused_slots; the room is STUB_ROOM slots */
#define STUB_ROOM 100
static const char *scripted_name; static int scripted_code;

void stub_reset(void) { stub_log[0] = 0; scripted_name = NULL; stub_fused_dots = 1; stub_fused_slots = 10; }
void stub_script(const char *name, int code) { scripted_name = name; scripted_code = code; }

static int hit(const char *name, const char *fmt, ...)
{
	size_t at = strlen(stub_log);
	va_list ap;
	at += (size_t)snprintf(stub_log + at, sizeof(stub_log) - at, "%s%s", at ? " " : "", name);
	va_start(ap, fmt);
	vsnprintf(stub_log + at, sizeof(stub_log) - at, fmt, ap);
	va_end(ap);
	return scripted_name && !strcmp(scripted_name, name) ? scripted_code : 0;
}
#define STUB(type, name, tag, params, ...) type name params { return hit(tag, __VA_ARGS__); }
/* a row-range launcher launches nothing for an empty range and answers 0 (spmv_csr.hip, spmv_formats.hip: `if (rb >= re) return 0`) */
#define STUB_ROWS(name, tag, params, ...) int name params { if (rb >= re) return 0; return hit(tag, __VA_ARGS__); }
#define X const double *x, double *y
#define DOT const double *w, int sq, double *result, void *work, void *stream

STUB(LIS_INT, lisc_halo_begin,  "halo_begin",  (LIS_MATRIX A, double *dx), "%s", "")
STUB(LIS_INT, lisc_halo_end,    "halo_end",    (LIS_MATRIX A, double *dx), "%s", "")
STUB(LIS_INT, lisc_halo_device, "halo_device", (LIS_MATRIX A, double *dx), "%s", "")
STUB(int, liship_spmv_formats_set_plane, "set_plane", (int rows), "(%d)", rows)
STUB(int, liship_spmv_csr_f64,     "csr",     (liship_csr_plan_t p, const int *ptr, const int *idx, const double *val, X, void *stream), "(plan=%d)", (int)(intptr_t)p)
STUB(int, liship_spmv_csr_dot_f64, "csr_dot", (liship_csr_plan_t p, const int *ptr, const int *idx, const double *val, X, DOT), "(sq=%d)", sq)
STUB(int, liship_spmv_csr_dot_finish_f64, "csr_dot_finish", (int slots, int sq, double *result, void *work, void *stream), "(slots=%d,sq=%d)", slots, sq)
STUB(int, liship_spmv_ell_f64,       "ell",       (int n, int maxnzr, const int *idx, const double *val, X, void *stream), "%s", "")
STUB(int, liship_spmv_ell_coded_f64, "ell_coded", (int n, int maxnzr, const unsigned char *codes, const int *dict, const double *val, X, DOT), "(sq=%d)", sq)
STUB(int, liship_spmv_ell_dot_f64,   "ell_dot",   (int n, int maxnzr, const int *idx, const double *val, X, DOT), "(sq=%d)", sq)
STUB(int, liship_spmv_dia_f64,       "dia",       (int n, int ncols, int nnd, const int *off, const double *val, X, void *stream), "%s", "")
STUB(int, liship_spmv_dia_dot_f64,   "dia_dot",   (int n, int ncols, int nnd, const int *off, const double *val, X, DOT), "(sq=%d)", sq)
STUB(int, liship_spmv_jad_f64,       "jad",       (int n, int maxnzr, const int *perm, const int *ptr, const int *idx, const double *val, X, void *stream), "%s", "")
STUB(int, liship_spmv_bsr_nnz_f64,   "bsr_nnz",   (int nr, int bnnz, int bnr, int bnc, const int *bptr, const int *bidx, const double *val, X, void *stream), "%s", "")
STUB(int, liship_spmv_bsr_dot_f64,   "bsr_dot",   (int nr, int n, int bnnz, int bs, const int *bptr, const int *bidx, const double *val, X, DOT), "(sq=%d)", sq)
STUB(int, liship_pmul_xpay_f64, "pmul_xpay", (int n, const double *x, const double *d, double a, double *y, void *stream), "(%d)", n)
STUB(int, liship_axpy_f64,      "axpy",      (int n, double a, const double *x, double *y, void *stream), "(%d)", n)
STUB(int, liship_dot_f64,       "dot",       (int n, const double *x, const double *y, double *result, void *work, void *stream), "(%d)", n)
STUB(int, liship_dot2_f64,      "dot2",      (int n, const double *x, const double *y, double *result, void *work, void *stream), "(%d)", n)
STUB_ROWS(liship_spmv_csr_rows_f64, "csr_rows", (liship_csr_plan_t p, int rb, int re, const int *ptr, const int *idx, const double *val, X, void *stream), "(%d,%d)", rb, re)
STUB_ROWS(liship_spmv_ell_rows_f64, "ell_rows", (int n, int maxnzr, const int *idx, const unsigned char *codes, const int *dict, const double *val, X, int rb, int re, void *stream), "(%d,%d,codes=%d)", rb, re, codes != NULL)
STUB_ROWS(liship_spmv_dia_rows_f64, "dia_rows", (int n, int ncols, int nnd, const int *off, const double *val, X, int rb, int re, void *stream), "(%d,%d)", rb, re)
STUB_ROWS(liship_spmv_bsr_rows_f64, "bsr_rows", (int nr, int bnnz, int bnr, int bnc, const int *bptr, const int *bidx, const double *val, X, int rb, int re, void *stream), "(%d,%d)", rb, re)
/* every part takes one slot per row of its range */
int liship_spmv_csr_rows_dot_f64(liship_csr_plan_t p, int rb, int re, const int *ptr, const int *idx, const double *val, X, const double *w, int sq, void *work, int slot, int *used, void *stream)
{
	*used = 0;
	if (rb >= re) return 0;
	const int rc = hit("csr_rows_dot", "(%d,%d,slot=%d,sq=%d)", rb, re, slot, sq);
	if (rc == 0) *used = re - rb;
	return rc;
}

LIS_INT lisd_mat_ready(LIS_MATRIX A) { return LIS_SUCCESS; }
int liship_csr_plan_fused_dots(liship_csr_plan_t p) { return stub_fused_dots; }
long long liship_csr_plan_fused_slots(liship_csr_plan_t p) { return stub_fused_slots; }
size_t liship_reduce_work_bytes(void) { return STUB_ROOM * 4 * sizeof(double); }
LIS_INT lisi_hip_error(const char *file, const char *func, int line, int hipcode) { hit("hip_error", "(%d)", hipcode); return 77; }
LIS_INT lisi_error(const char *file, const char *func, int line, LIS_INT code, const char *fmt, ...) { hit("lis_error", "(%d)", (int)code); return code; }
