/* Drives lisd_mat_ready (lis_amd/csrc/host/lis_upload.c) and lisd_convert_csr (lis_convert_hbm.c) over a hand-made 6 x 6 bidiagonal matrix in every format against
 * tests/c/upload_stubs.c and prints, per case, the calls that reached the stubs:
 *     "<case> | <log> | ret=<code> done=<0|1> type=<kernel family of the copy> pad=<pad_comm>"
 * then the failure sweep: for every case marked for it and every position of its log whose stub can fail, the case again with that hit answering an error --
 * HIP code 2 for an allocation, NULL for lisp_alloc_lazy, 700 for everything else --, the copies destroyed, and what is still alive counted:
 *     "sweep <case> | <position> <token> | ret=<code> done=<0|1> type=<...> | clean"      (or "LEAK allocations=.. plans=.. lazy=..")
 * tests/test_upload_paths_cpu.py asserts every line. */
#include <stdint.h>
#include <stdio.h>
#include "lis_internal.h"

extern char stub_log[];
extern int stub_value_records, stub_coded, stub_maxlen, stub_unsorted, stub_nnd, stub_bnnz, stub_rnnz;
void stub_reset(void);
void stub_script(const char *name, int k, int code);
void stub_forget(void);
int stub_live_allocations(void), stub_live_plans(void), stub_live_lazy(void);

#define CSR LIS_MATRIX_CSR
#define CSC LIS_MATRIX_CSC
#define ELL LIS_MATRIX_ELL
#define DIA LIS_MATRIX_DIA
#define JAD LIS_MATRIX_JAD
#define BSR LIS_MATRIX_BSR
enum { UPLOAD, CONVERT };

typedef struct {
	const char *name;
	int kind; LIS_INT type;              /* UPLOAD: the format of the matrix; CONVERT: the target */
	int varying;                         /* values: all 1.0, or all different (the few-distinct-values screen refuses) */
	int sweep;
	int vrec;                            /* liship_csr_plan_value_records: -1 = none, 0 = the stubs' 1, 2 = wide */
	int split, bn;                       /* UPLOAD: a split matrix; CONVERT to BSR: conv_bnr = conv_bnc (0: 2, -1: none given) */
	int maxlen, unsorted, nnd, bnnz;     /* the facts the stubs answer (0: their defaults; nnd / bnnz -1: none found) */
	int no_device_convert, ranks, split_source, ghosts, empty, device_only;
	const char *refuse; int code;        /* the first hit of this stub answers `code` */
} test_case;

static const test_case cases[] = {
	{"up_csr", UPLOAD, CSR, 1}, {"up_csc", UPLOAD, CSC, 1}, {"up_jad", UPLOAD, JAD, 1}, {"up_bsr", UPLOAD, BSR, 1},
	{"up_split_csr", UPLOAD, CSR, 1, .split = 1}, {"up_split_jad", UPLOAD, JAD, 1, .split = 1},
	{"up_ell_native", UPLOAD, ELL, 1}, {"up_ell_codes_oom", UPLOAD, ELL, 1, .refuse = "ell_codes", .code = 2},
	{"up_ell_rowform", UPLOAD, ELL, 0, 1}, {"up_ell_dropped", UPLOAD, ELL, 0, 1, .vrec = -1},
	{"up_dia_native", UPLOAD, DIA, 1}, {"up_dia_rowform", UPLOAD, DIA, 0, 1}, {"up_dia_dropped", UPLOAD, DIA, 0, 1, .vrec = -1},
	{"up_bsr_rowform", UPLOAD, BSR, 0, 1}, {"up_bsr_rowform_wide", UPLOAD, BSR, 0, 1, .vrec = 2}, {"up_bsr_dropped", UPLOAD, BSR, 0, 1, .vrec = -1},
	{"conv_ell_rowform", CONVERT, ELL, 0, 1}, {"conv_ell_dropped", CONVERT, ELL, 0, 1, .vrec = -1}, {"conv_ell_native", CONVERT, ELL, 1, 1},
	{"conv_dia_rowform", CONVERT, DIA, 0, 1}, {"conv_dia_dropped", CONVERT, DIA, 0, 1, .vrec = -1}, {"conv_dia_native", CONVERT, DIA, 1, 1},
	{"conv_csc", CONVERT, CSC, 1, 1}, {"conv_jad", CONVERT, JAD, 1, 1},
	{"conv_bsr_rowform", CONVERT, BSR, 0, 1}, {"conv_bsr_rowform_wide", CONVERT, BSR, 0, 1, .vrec = 2}, {"conv_bsr_dropped", CONVERT, BSR, 0, 1, .vrec = -1},
	{"conv_bsr_native", CONVERT, BSR, 1, 1}, {"conv_bsr_padding", CONVERT, BSR, 0, 1, .bn = 4},
	/* not a case for the conversion in HBM: *done stays 0 */
	{"not_wrong_target", CONVERT, CSR, 0, 1}, {"not_switched_off", CONVERT, ELL, 0, 1, .no_device_convert = 1}, {"not_two_ranks", CONVERT, ELL, 0, 1, .ranks = 2},
	{"not_split_source", CONVERT, ELL, 0, 1, .split_source = 1}, {"not_ghost_columns", CONVERT, ELL, 0, 1, .ghosts = 1}, {"not_empty", CONVERT, ELL, 0, 1, .empty = 1},
	{"not_device_only_jad", CONVERT, JAD, 0, 1, .device_only = 1}, {"not_unsorted_dia", CONVERT, DIA, 0, 1, .unsorted = 1}, {"not_unsorted_csc", CONVERT, CSC, 0, 1, .unsorted = 1},
	{"not_ell_too_wide", CONVERT, ELL, 0, 1, .maxlen = 357913942}, {"not_dia_none", CONVERT, DIA, 0, 1, .nnd = -1}, {"not_bsr_none", CONVERT, BSR, 0, 1, .bnnz = -1},
	{"not_bsr_no_block_size", CONVERT, BSR, 0, 1, .bn = -1},
};

/* the matrix: row i holds (i, i) and (i, i + 1); n = 6, 11 entries; BSR in 2 x 2 blocks */
enum { N = 6, NNZ = 11 };
static LIS_INT csr_ptr[] = {0, 2, 4, 6, 8, 10, 11}, csr_idx[] = {0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5};
static LIS_INT csc_ptr[] = {0, 1, 3, 5, 7, 9, 11}, csc_idx[] = {0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5};
static LIS_INT ell_idx[] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 5}, dia_idx[] = {0, 1};
static LIS_INT jad_row[] = {0, 1, 2, 3, 4, 5}, jad_ptr[] = {0, 6, 11}, jad_idx[] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5};
static LIS_INT bsr_ptr[] = {0, 2, 4, 5}, bsr_idx[] = {0, 1, 1, 2, 2};
static LIS_SCALAR values[20], diagonal[N];
static struct LIS_MATRIX_DIAG_STRUCT diag;

static const char *type_name(int type)
{
	static char other[16];
	switch (type) { case CSR: return "CSR"; case ELL: return "ELL"; case DIA: return "DIA"; case BSR: return "BSR"; }
	snprintf(other, sizeof(other), "%d", type);
	return other;
}

static void header(lisi_matrix *M, LIS_INT type)
{
	LIS_MATRIX A = &M->pub;
	memset(M, 0, sizeof(*M));
	A->n = N; A->np = N; A->gn = N; A->nnz = NNZ; A->matrix_type = type; A->status = type;
}

/* one run of a case; what it answered is left in *ret, *done, *type, *pad and stub_log; returns 1 when nothing is alive after the copies were destroyed
 * (left[]: device allocations, plans, lazy host arrays) */
static int left[3];
static int run(const test_case *t, const char *fail, int k, int code, LIS_INT *ret, int *done, int *type, int *pad)
{
	static lisi_matrix in, out;
	static char kept[16384];
	LIS_MATRIX A = &in.pub, B = &out.pub;
	stub_reset();                    /* (no script left over while the source is made) */
	for (int i = 0; i < 20; i++) values[i] = t->varying ? 1.5 * (i + 1) : 1.0;
	header(&in, t->kind == UPLOAD ? t->type : CSR);
	header(&out, t->type);
	if (t->kind == UPLOAD) {
		A->value = values; A->is_splited = t->split; A->D = &diag; diag.value = diagonal;
		switch (t->type) {
		case CSR: A->ptr = csr_ptr; A->index = csr_idx; break;
		case CSC: A->ptr = csc_ptr; A->index = csc_idx; break;
		case ELL: A->maxnzr = 2; A->index = ell_idx; break;
		case DIA: A->nnd = 2; A->index = dia_idx; break;
		case JAD: A->maxnzr = 2; A->row = jad_row; A->ptr = jad_ptr; A->index = jad_idx; break;
		default:  A->bnr = A->bnc = 2; A->nr = A->nc = 3; A->bnnz = 5; A->bptr = bsr_ptr; A->bindex = bsr_idx; break;
		}
	} else {                         /* the source: a CSR matrix whose HBM copy exists */
		lisd_mat *sd = &in.dev;
		sd->ready = 1; sd->type = CSR; sd->n = N; sd->np = N; sd->nnz = NNZ; sd->device_only = t->device_only;
		if (liship_malloc((void **)&sd->ptr, sizeof(csr_ptr)) || liship_malloc((void **)&sd->index, sizeof(csr_idx)) || liship_malloc((void **)&sd->value, sizeof(double) * NNZ)) abort();
		memcpy(sd->value, values, sizeof(double) * NNZ);
		A->is_splited = t->split_source; A->np = N + t->ghosts; if (t->empty) A->nnz = 0;
		B->conv_bnr = B->conv_bnc = t->bn < 0 ? 0 : t->bn ? t->bn : 2;
	}
	stub_reset();
	memset(&lisg, 0, sizeof(lisg));
	lisg.device_ready = 1; lisg.nprocs = t->ranks ? t->ranks : 1; lisg.no_device_convert = t->no_device_convert;
	stub_value_records = t->vrec < 0 ? 0 : t->vrec ? t->vrec : 1;
	if (t->maxlen) stub_maxlen = t->maxlen;
	stub_unsorted = t->unsorted;
	if (t->nnd) stub_nnd = 0;
	if (t->bnnz) stub_bnnz = 0;
	if (fail) stub_script(fail, k, code);
	else if (t->refuse) stub_script(t->refuse, 1, t->code);
	*done = 0;
	*ret = t->kind == UPLOAD ? lisd_mat_ready(A) : lisd_convert_csr(A, B, done);
	*type = (t->kind == UPLOAD ? &in : &out)->dev.type;
	*pad = B->pad_comm;
	strcpy(kept, stub_log);
	/* the copies go, and with them the host arrays the target's header holds */
	if (t->kind == CONVERT) {
		void *arr[] = {B->ptr, B->row, B->index, B->bptr, B->bindex, B->value};
		for (int i = 0; i < 6; i++) if (!lisp_free_array(arr[i])) free(arr[i]);
		lisd_mat_free(B);
	}
	lisd_mat_free(A);
	strcpy(stub_log, kept);
	left[0] = stub_live_allocations(); left[1] = stub_live_plans(); left[2] = stub_live_lazy();
	stub_forget();
	return left[0] == 0 && left[1] == 0 && left[2] == 0;
}

/* the stubs that stand for a call that can fail: everything but the frees, the host-side bookkeeping and the header setters */
static int fallible(const char *name)
{
	static const char *never[] = {"free", "destroy", "trim", "init", "fill", "adopt", "protect", "release", "assemble", "jad_order", "split_rows", "split_jad_part",
	                              "storage_destroy", "hip_error", "lis_error", "set_ell", "set_dia", "set_csc", "set_jad", "set_bsr"};
	for (size_t i = 0; i < sizeof(never) / sizeof(never[0]); i++) if (!strcmp(name, never[i])) return 0;
	return 1;
}

int main(void)
{
	static char success[16384];
	for (size_t ci = 0; ci < sizeof(cases) / sizeof(cases[0]); ci++) {
		const test_case *t = &cases[ci];
		LIS_INT ret; int done, type, pad;
		const int clean = run(t, NULL, 0, 0, &ret, &done, &type, &pad);
		printf("%s | %s | ret=%d done=%d type=%s pad=%d\n", t->name, stub_log, (int)ret, done, type_name(type), pad);
		if (!clean) printf("sweep %s | -1 none | ret=%d done=%d type=%s | LEAK allocations=%d plans=%d lazy=%d\n", t->name, (int)ret, done, type_name(type), left[0], left[1], left[2]);
		if (!t->sweep || !clean) continue;
		strcpy(success, stub_log);
		int position = 0;
		for (char *tok = success; *tok; position++) {
			char token[64], name[64];
			size_t len = strcspn(tok, " ");
			snprintf(token, sizeof(token), "%.*s", (int)len, tok);
			snprintf(name, sizeof(name), "%.*s", (int)strcspn(token, "("), token);
			if (fallible(name)) {
				int kth = 0;                        /* which hit of this stub the position is */
				for (const char *q = success; q <= tok; q += strcspn(q, " "), q += (*q == ' '))
					kth += !strncmp(q, name, strlen(name)) && (q[strlen(name)] == '(' || q[strlen(name)] == ' ' || q[strlen(name)] == 0);
				const int ok = run(t, name, kth, !strcmp(name, "malloc") ? 2 : 700, &ret, &done, &type, &pad);
				printf("sweep %s | %d %s | ret=%d done=%d type=%s | ", t->name, position, token, (int)ret, done, type_name(type));
				if (ok) printf("clean\n");
				else printf("LEAK allocations=%d plans=%d lazy=%d\n", left[0], left[1], left[2]);
			}
			tok += len; tok += (*tok == ' ');
		}
	}
	return 0;
}
