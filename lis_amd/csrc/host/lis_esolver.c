/*
 * lis_esolver.c -- lis_esolve / lis_gesolve: the eigen half of the Lis C API (reference src/esolver/lis_esolver.c): the object, its options and getters, the
 * descriptor table of the eigensolvers and the solve itself.  The loops stand in lis_esolver_single.c (one pair: -e pi | ii | rqi | cg | cr, and under a matrix
 * B -e gpi | gii | grqi | gcr) and lis_esolver_multi.c (several pairs, -ss >= 2: -e si | li | ai and -e gsi | gli | gai, with the getters only they fill); what
 * they share is lis_eloop.h.
 *
 * Refused, with LIS_ERR_NOT_IMPLEMENTED and before A, B or x is touched: -e si | li | ai | gsi | gli | gai with -ss 1 (the default: one pair is what -e pi / -e ii
 * and -e gpi / -e gii serve), -e si with an -ie other than pi or ii, -e gsi with an -ige other than gpi or gii (the reference's loop then applies neither matrix),
 * -e gli | gai with -ige gcg or a standard solver, a B together with a standard -e (the reference silently ignores B there), a generalized -e through lis_esolve
 * or with B = NULL (the reference's loops multiply by that NULL), -e gcg (the reference's loop never updates x and ends in NaN: -e gcr is the one that works), a
 * job of several ranks.
 * -ef quad | switch answers as lis_solve does for -f quad.
 *
 * Deliberate differences from the reference, all outside a converging solve: the arrays of the object start zeroed instead of holding heap contents; a
 * negative -emaxiter is refused; an inner solve that fails hands its code back as the return value (the reference returns LIS_SUCCESS and leaves A shifted
 * in -e rqi); work vectors of an earlier solve are released instead of leaked.
 */
#include "lis_eloop.h"

/* ------------------------------------------------------------------ one row per eigensolver, indexed by LIS_ESOLVER_*: the key -e, -ie and -ige name it by
 * and its printed name (ref lis_esolver.c:118, :124), its loop, whether it takes a B and whether it computes several pairs, its work vectors (lis_e<xx>_malloc_work:
 * `work` and, where per_ss is set, one per vector of the subspace), and the inner eigensolvers (-ie, or -ige for a generalized row) its loop can run, as a bit
 * mask with the list the refusal prints.  -e gcg has a row and no loop: refused in lis_gesolve */
#define E_(n) (1u << LIS_ESOLVER_##n)
enum { E_B = 1, E_SS = 2 };
typedef struct {
	const char *key, *name;
	LIS_INT (*run)(LIS_ESOLVER);
	unsigned flags;              /* E_B: the generalized problem, a B is needed; E_SS: several pairs, -ss >= 2 */
	int work, per_ss;
	unsigned inner;
	const char *inner_keys;
} esolver_desc;
static const esolver_desc esolvers[LIS_ESOLVER_LEN + 1] = {
	[0]                 = {"", "", NULL, 0, 0, 0, 0, NULL},
	[LIS_ESOLVER_PI]    = {"pi", "Power", lisi_epi_ii, 0, 2, 0, 0, NULL},
	[LIS_ESOLVER_II]    = {"ii", "Inverse", lisi_epi_ii, 0, 2, 0, 0, NULL},
	[LIS_ESOLVER_RQI]   = {"rqi", "Rayleigh Quotient", lisi_erqi, 0, 2, 0, 0, NULL},
	[LIS_ESOLVER_CG]    = {"cg", "CG", lisi_ecg, 0, 6, 0, 0, NULL},
	[LIS_ESOLVER_CR]    = {"cr", "CR", lisi_ecr, 0, 6, 0, 0, NULL},
	[LIS_ESOLVER_SI]    = {"si", "Subspace", lisi_esi, E_SS, 4, 1, E_(PI) | E_(II), "pi, ii"},
	[LIS_ESOLVER_LI]    = {"li", "Lanczos", lisi_eli, E_SS, 2, 1, E_(PI) | E_(II) | E_(RQI) | E_(CG) | E_(CR), "pi, ii, rqi, cg, cr"},
	[LIS_ESOLVER_AI]    = {"ai", "Arnoldi", lisi_eai, E_SS, 2, 1, E_(PI) | E_(II) | E_(RQI) | E_(CG) | E_(CR), "pi, ii, rqi, cg, cr"},
	[LIS_ESOLVER_GPI]   = {"gpi", "Generalized Power", lisi_epi_ii, E_B, 3, 0, 0, NULL},
	[LIS_ESOLVER_GII]   = {"gii", "Generalized Inverse", lisi_epi_ii, E_B, 3, 0, 0, NULL},
	[LIS_ESOLVER_GRQI]  = {"grqi", "Generalized Rayleigh Quotient", lisi_egrqi, E_B, 3, 0, 0, NULL},
	[LIS_ESOLVER_GCG]   = {"gcg", "Generalized CG", NULL, E_B, 3, 0, 0, NULL},
	[LIS_ESOLVER_GCR]   = {"gcr", "Generalized CR", lisi_egcr, E_B, 9, 0, 0, NULL},
	[LIS_ESOLVER_GSI]   = {"gsi", "Generalized Subspace", lisi_esi, E_B | E_SS, 5, 1, E_(GPI) | E_(GII), "gpi, gii"},
	[LIS_ESOLVER_GLI]   = {"gli", "Generalized Lanczos", lisi_egli, E_B | E_SS, 4, 1, E_(GPI) | E_(GII) | E_(GRQI) | E_(GCR), "gpi, gii, grqi, gcr"},
	[LIS_ESOLVER_GAI]   = {"gai", "Generalized Arnoldi", lisi_eai, E_B | E_SS, 3, 1, E_(GPI) | E_(GII) | E_(GRQI) | E_(GCR), "gpi, gii, grqi, gcr"},
};
/* the row of an -e read from the options: row 0, which is nothing, for a number outside the table */
static const esolver_desc *desc_of(LIS_INT nesolver) { return &esolvers[nesolver >= 1 && nesolver <= LIS_ESOLVER_LEN ? nesolver : 0]; }

static const char *eprint_keys[] = {"none", "mem", "out", "all"};
static const char *etruefalse_keys[] = {"false", "true"};
static const char *estorage_keys[] = {"csr", "csc", "msr", "dia", "ell", "jad", "bsr", "bsc", "vbr", "coo", "dns"};
static const char *eprecision_keys[] = {"double", "quad", "switch"};
static const char *estorage_names[] = {"CSR", "CSC", "MSR", "DIA", "ELL", "JAD", "BSR", "BSC", "VBR", "COO", "DNS"};
static const char *ereturncode_names[] = {"LIS_SUCCESS", "LIS_ILL_OPTION", "LIS_BREAKDOWN", "LIS_OUT_OF_MEMORY", "LIS_MAXITER", "LIS_NOT_IMPLEMENTED", "LIS_ERR_FILE_IO"};
#define COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))

/* ------------------------------------------------------------------ the object */
static void esolver_init(LIS_ESOLVER e)
{	/* ref lis_esolver_init, :143-187 */
	memset(e, 0, sizeof(*e));
	e->eprecision = LIS_PRECISION_DOUBLE;
	e->options[LIS_EOPTIONS_ESOLVER] = LIS_ESOLVER_CR;
	e->options[LIS_EOPTIONS_MAXITER] = 1000;
	e->options[LIS_EOPTIONS_SUBSPACE] = 1;
	e->options[LIS_EOPTIONS_MODE] = 0;
	e->options[LIS_EOPTIONS_OUTPUT] = LIS_FALSE;
	e->options[LIS_EOPTIONS_INITGUESS_ONES] = LIS_TRUE;
	e->options[LIS_EOPTIONS_INNER_ESOLVER] = LIS_ESOLVER_II;
	e->options[LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER] = LIS_ESOLVER_GII;
	e->options[LIS_EOPTIONS_STORAGE] = 0;
	e->options[LIS_EOPTIONS_STORAGE_BLOCK] = 2;
	e->options[LIS_EOPTIONS_PRECISION] = LIS_PRECISION_DOUBLE;
	e->options[LIS_EOPTIONS_RVAL] = LIS_FALSE;
	e->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN] = 1.0e-12;
	e->params[LIS_EPARAMS_SHIFT - LIS_EOPTIONS_LEN] = 0.0;
	e->params[LIS_EPARAMS_SHIFT_IM - LIS_EOPTIONS_LEN] = 0.0;
}

LIS_INT lis_esolver_create(LIS_ESOLVER *esolver)
{
	*esolver = (LIS_ESOLVER)malloc(sizeof(struct LIS_ESOLVER_STRUCT));
	if (!*esolver) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)sizeof(struct LIS_ESOLVER_STRUCT));
	esolver_init(*esolver);
	return LIS_SUCCESS;
}

static void work_destroy(LIS_ESOLVER e)
{	/* ref lis_esolver_work_destroy, :211-227 */
	if (e && e->work) {
		for (LIS_INT i = 0; i < e->worklen; i++) lis_vector_destroy(e->work[i]);
		free(e->work);
		e->work = NULL; e->worklen = 0;
	}
}

/* the arrays of the object and the eigenvectors an earlier solve left: evector has two slots more than vectors and is filled from slot 0, so the first NULL ends them */
static void arrays_free(LIS_ESOLVER e)
{
	if (e->evector) for (LIS_INT i = 0; e->evector[i]; i++) lis_vector_destroy(e->evector[i]);
	free(e->rhistory); free(e->evalue); free(e->resid); free(e->iter); free(e->iter2); free(e->evector);
	e->rhistory = NULL; e->evalue = NULL; e->resid = NULL; e->iter = NULL; e->iter2 = NULL; e->evector = NULL;
}

LIS_INT lis_esolver_destroy(LIS_ESOLVER e)
{	/* ref :231-259 */
	if (e) {
		work_destroy(e);
		arrays_free(e);
		free(e);
	}
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ options, ref :103-122 (tables), :726-1052 (lis_esolver_set_option2 and its helpers) */
#define KEYS(a) (a), sizeof((a)[0]), COUNT(a)
#define ESOLVER_KEYS &esolvers[1].key, sizeof(esolvers[0]), LIS_ESOLVER_LEN      /* the key column of the descriptor table */
static LIS_INT epick(const char *val, char lo, char hi, const void *keys, size_t stride, int nkeys, int base, LIS_INT *slot, const char *what)
{	/* a leading digit in [lo, hi]: the number (no range check here, as there); else the name, of nkeys names `stride` bytes apart; else ILL_ARG */
	if (val[0] >= lo && val[0] <= hi) { sscanf(val, "%d", slot); return LIS_SUCCESS; }
	for (int i = 0; i < nkeys; i++) if (strcmp(val, *(const char *const *)((const char *)keys + i * stride)) == 0) { *slot = i + base; return LIS_SUCCESS; }
	return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter %s is not correct\n", what);
}

static LIS_INT eset_one(const char *name, const char *val, void *object)
{
	LIS_ESOLVER e = (LIS_ESOLVER)object;
	static const struct { const char *name; int slot; } table[] = {
		{"-emaxiter", LIS_EOPTIONS_MAXITER}, {"-etol", LIS_EPARAMS_RESID}, {"-e", LIS_EOPTIONS_ESOLVER}, {"-ss", LIS_EOPTIONS_SUBSPACE}, {"-m", LIS_EOPTIONS_MODE},
		{"-shift", LIS_EPARAMS_SHIFT}, {"-shift_im", LIS_EPARAMS_SHIFT_IM}, {"-eprint", LIS_EOPTIONS_OUTPUT}, {"-initx_ones", LIS_EOPTIONS_INITGUESS_ONES},
		{"-ie", LIS_EOPTIONS_INNER_ESOLVER}, {"-ige", LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER}, {"-estorage", LIS_EOPTIONS_STORAGE},
		{"-estorage_block", LIS_EOPTIONS_STORAGE_BLOCK}, {"-ef", LIS_EOPTIONS_PRECISION}, {"-rval", LIS_EOPTIONS_RVAL},
	};
	LIS_INT *o = e->options;
	for (int i = 0; i < COUNT(table); i++) {
		if (strcmp(name, table[i].name) != 0) continue;
		const int slot = table[i].slot;
		switch (slot) {
		case LIS_EOPTIONS_ESOLVER:        return epick(val, '0', '9', ESOLVER_KEYS, 1, &o[slot], "LIS_EOPTIONS_ESOLVER");
		case LIS_EOPTIONS_INNER_ESOLVER:  return epick(val, '0', '9', ESOLVER_KEYS, 1, &o[slot], "LIS_EOPTIONS_INNER_ESOLVER");
		case LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER: return epick(val, '0', '9', ESOLVER_KEYS, 1, &o[slot], "LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER");
		case LIS_EOPTIONS_OUTPUT:         return epick(val, '0', '3', KEYS(eprint_keys), 0, &o[slot], "LIS_EOPTIONS_OUTPUT");
		case LIS_EOPTIONS_INITGUESS_ONES: case LIS_EOPTIONS_RVAL:
		                                  return epick(val, '0', '1', KEYS(etruefalse_keys), 0, &o[slot], "LIS_EOPTIONS_TRUEFALSE");
		case LIS_EOPTIONS_STORAGE:        return epick(val, '0', '9', KEYS(estorage_keys), 1, &o[slot], "LIS_EOPTIONS_STORAGE");
		case LIS_EOPTIONS_PRECISION:      return epick(val, '0', '1', KEYS(eprecision_keys), 0, &o[slot], "LIS_EOPTIONS_PRECISION");
		default:
			if (slot < LIS_EOPTIONS_LEN) sscanf(val, "%d", &o[slot]);
			else { double v; if (sscanf(val, "%lg", &v) == 1) e->params[slot - LIS_EOPTIONS_LEN] = v; }
			return LIS_SUCCESS;
		}
	}
	return LIS_SUCCESS;      /* unknown options are ignored, as in the reference */
}

static LIS_INT eset_from_tokens(char **tok, int n, LIS_ESOLVER e)
{
	const LIS_INT err = lisi_each_option(tok, n, eset_one, e);
	if (err) { work_destroy(e); e->retcode = err; }
	return err;
}

LIS_INT lis_esolver_set_option(char *text, LIS_ESOLVER esolver)
{
	char **tok;
	const int n = lisi_tokenize(text, &tok);
	const LIS_INT err = eset_from_tokens(tok, n, esolver);
	lisi_tokens_free(tok, n);
	return err;
}

LIS_INT lis_esolver_set_optionC(LIS_ESOLVER esolver) { return eset_from_tokens(lisi_cmd_argv, lisi_cmd_argc, esolver); }

/* ------------------------------------------------------------------ getters, ref :1056-1384 */
LIS_INT lis_esolver_get_iter(LIS_ESOLVER e, LIS_INT *iter) { *iter = e->iter[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_iterex(LIS_ESOLVER e, LIS_INT *iter, LIS_INT *iter_double, LIS_INT *iter_quad)
{ *iter = e->iter[0]; *iter_double = e->iter2[0]; *iter_quad = e->iter[0] - e->iter2[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_time(LIS_ESOLVER e, double *time) { *time = e->time; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_timeex(LIS_ESOLVER e, double *time, double *itime, double *ptime, double *p_c_time, double *p_i_time)
{
	*time = e->time;
	if (itime) *itime = e->itime;
	if (ptime) *ptime = e->ptime;
	if (p_c_time) *p_c_time = e->p_c_time;
	if (p_i_time) *p_i_time = e->p_i_time;
	return LIS_SUCCESS;
}
LIS_INT lis_esolver_get_residualnorm(LIS_ESOLVER e, LIS_REAL *residual) { *residual = e->resid[0]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_status(LIS_ESOLVER e, LIS_INT *status) { *status = e->retcode; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_esolver(LIS_ESOLVER e, LIS_INT *nesol) { *nesol = e->options[LIS_EOPTIONS_ESOLVER]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_esolvername(LIS_INT esolver, char *esolvername)
{
	if (esolver < 1 || esolver > LIS_ESOLVER_LEN) return LIS_FAILS;
	strcpy(esolvername, esolvers[esolver].name);
	return LIS_SUCCESS;
}

static LIS_INT history_len(LIS_ESOLVER e)
{	/* ref :1138-1142: the entries 0 .. iter of a solve that converged, 0 .. iter - 1 otherwise */
	LIS_INT len = e->iter[0] + 1;
	if (e->retcode != LIS_SUCCESS) len--;
	return len;
}

LIS_INT lis_esolver_get_rhistory(LIS_ESOLVER e, LIS_VECTOR v)
{
	const LIS_INT n = _min(v->n, history_len(e));
	LISCHK(lisd_vec_host_write(v, 1));
	for (LIS_INT i = 0; i < n; i++) v->value[i] = e->rhistory[i];
	lis_amd_vector_host_modified(v);
	return LIS_SUCCESS;
}

LIS_INT lis_esolver_output_rhistory(LIS_ESOLVER e, char *filename)
{	/* ref src/system/lis_output.c:659-728 */
	if (e->rhistory == NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "eigensolver's residual history is empty\n");
	FILE *file = fopen(filename, "w");
	if (file == NULL) return LISI_ERR(LIS_ERR_FILE_IO, "cannot open file %s\n", filename);
	const LIS_INT len = history_len(e);
	for (LIS_INT i = 0; i < len; i++) fprintf(file, "%e\n", (double)e->rhistory[i]);
	fclose(file);
	return LIS_SUCCESS;
}

/* what the subspace, Lanczos and Arnoldi solvers fill (ref :1153-1355).  On an esolver whose -e names none of them (nor a generalized form) the three that fill
 * a vector answer LIS_ERR_ILL_ARG as the reference does (:1159-1163) and the others say that they belong to those solvers; on one that names such a solver but
 * holds no ended solve -- never run, refused, failed -- every getter answers LIS_ERR_ILL_ARG */
static LIS_INT subspace_only(const char *what)
{
	return LISI_ERR(LIS_ERR_NOT_IMPLEMENTED, "%s is filled by the subspace, Lanczos and Arnoldi eigensolvers only (-e si | li | ai | gsi | gli | gai)\n", what);
}
static LIS_INT multi_filled(LIS_ESOLVER e, const char *what, LIS_INT mode, int vectors)
{
	const LIS_INT nesolver = e->options[LIS_EOPTIONS_ESOLVER], ss = e->options[LIS_EOPTIONS_SUBSPACE];
	if (!(desc_of(nesolver)->flags & E_SS)) return subspace_only(what);
	if (!e->evalue || !e->resid || !e->iter || !e->evector) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: no eigensolve has filled the esolver\n", what);
	if (mode < 0 || mode >= ss) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: mode %D is outside the subspace of %D\n", what, mode, ss);
	if (vectors) for (LIS_INT i = 0; i <= mode; i++) if (!e->evector[i]) return LISI_ERR(LIS_ERR_ILL_ARG, "%s: the solve left no eigenvector %D (-rval true computes Ritz values only)\n", what, i);
	return LIS_SUCCESS;
}
/* the three that copy the object's arrays of ss entries into a vector (ref :1153-1179, :1261-1287, :1309-1337) */
static LIS_INT per_mode(LIS_ESOLVER e, LIS_VECTOR v, int what)
{
	const LIS_INT nesolver = e->options[LIS_EOPTIONS_ESOLVER];
	if (!(desc_of(nesolver)->flags & E_SS))
		return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_ESOLVER is %D (Set Subspace, Lanczos, Arnoldi, Generalized Subspace, Generalized Lanczos, or Generalized Arnoldi)\n", nesolver);
	if (!e->evalue || !e->resid || !e->iter) return LISI_ERR(LIS_ERR_ILL_ARG, "no eigensolve has filled the esolver\n");
	const LIS_INT ss = e->options[LIS_EOPTIONS_SUBSPACE];
	LIS_INT n, gn, is, ie;
	LISCHK(lis_vector_set_size(v, 0, ss));
	LISCHK(lis_vector_get_size(v, &n, &gn));
	LISCHK(lis_vector_get_range(v, &is, &ie));
	for (LIS_INT i = 0; i < n; i++) {
		const LIS_INT ii = i + (v->origin ? 1 : 0);
		LISCHK(lis_vector_set_value(LIS_INS_VALUE, ii + is, what == 0 ? e->evalue[i + is] : what == 1 ? e->resid[i + is] : (LIS_SCALAR)e->iter[i + is], v));
	}
	if (what == 2) v->intvalue = 1;
	return LIS_SUCCESS;
}
LIS_INT lis_esolver_get_evalues(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 0); }
LIS_INT lis_esolver_get_residualnorms(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 1); }
LIS_INT lis_esolver_get_iters(LIS_ESOLVER e, LIS_VECTOR v) { return per_mode(e, v, 2); }
LIS_INT lis_esolver_get_specific_evalue(LIS_ESOLVER e, LIS_INT mode, LIS_SCALAR *evalue)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_evalue", mode, 0)); *evalue = e->evalue[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_residualnorm(LIS_ESOLVER e, LIS_INT mode, LIS_REAL *residual)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_residualnorm", mode, 0)); *residual = e->resid[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_iter(LIS_ESOLVER e, LIS_INT mode, LIS_INT *iter)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_iter", mode, 0)); *iter = e->iter[mode]; return LIS_SUCCESS; }
LIS_INT lis_esolver_get_specific_evector(LIS_ESOLVER e, LIS_INT mode, LIS_VECTOR x)
{ LISCHK(multi_filled(e, "lis_esolver_get_specific_evector", mode, 1)); return lis_vector_copy(e->evector[mode], x); }

/* ref :1201-1239: M sized gn x gn, column j = eigenvector j, every entry set (zeros included), then type and assemble.  The reference makes M a COO matrix;
 * M is assembled as CSR here -- the same entries in the same order, row by row.  Each vector comes home from HBM once */
LIS_INT lis_esolver_get_evectors(LIS_ESOLVER e, LIS_MATRIX M)
{
	const LIS_INT ss = e->options[LIS_EOPTIONS_SUBSPACE];
	LISCHK(multi_filled(e, "lis_esolver_get_evectors", ss - 1, 1));
	LIS_INT n, gn, is, ie, js = 0, err = LIS_SUCCESS;
	LISCHK(lis_matrix_set_size(M, 0, e->evector[0]->gn));
	LISCHK(lis_matrix_get_size(M, &n, &gn));
	LISCHK(lis_matrix_get_range(M, &is, &ie));
	if (e->evector[0]->origin) { is++; js++; }
	LIS_SCALAR *col = (LIS_SCALAR *)malloc((size_t)(n > 0 ? n : 1) * sizeof(LIS_SCALAR));
	if (!col) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(n * sizeof(LIS_SCALAR)));
	for (LIS_INT j = 0; j < ss && !err; j++) {
		err = lis_vector_gather(e->evector[j], col);
		for (LIS_INT i = 0; i < n && !err; i++) err = lis_matrix_set_value(LIS_INS_VALUE, i + is, j + js, col[i], M);
	}
	free(col);
	if (err) return err;
	LISCHK(lis_matrix_set_type(M, LIS_MATRIX_CSR));
	return lis_matrix_assemble(M);
}

/* ------------------------------------------------------------------ lis_esolve / lis_gesolve, ref :263-666 */
static LIS_INT work_alloc(LIS_ESOLVER e, LIS_INT count)
{	/* lis_e<xx>_malloc_work: NWORK duplicates of A's row layout */
	work_destroy(e);
	e->work = (LIS_VECTOR *)calloc((size_t)count, sizeof(LIS_VECTOR));
	if (!e->work) return LISI_ERR(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)(count * sizeof(LIS_VECTOR)));
	for (LIS_INT i = 0; i < count; i++) {
		const LIS_INT err = lis_vector_duplicate(e->A, &e->work[i]);
		if (err) { for (LIS_INT j = 0; j < i; j++) lis_vector_destroy(e->work[j]); free(e->work); e->work = NULL; return err; }
	}
	e->worklen = count;
	return LIS_SUCCESS;
}

/* a refusal of lis_gesolve: the code goes into the object and comes back */
#define REFUSE(code, ...) do { esolver->retcode = (code); return LISI_ERR(code, __VA_ARGS__); } while (0)

LIS_INT lis_gesolve(LIS_MATRIX A, LIS_MATRIX B, LIS_VECTOR x, LIS_SCALAR *evalue0, LIS_ESOLVER esolver)
{
	LIS_VECTOR xx = NULL;
	LIS_INT err;
	/* parameter check, ref :310-435 */
	LISCHK(lisi_matrix_check(A, LISI_CHECK_ASSEMBLED));
	if (x == NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "vector x is undefined\n");
	if (A->n != x->n) return LIS_ERR_ILL_ARG;
	if (A->gn <= 0) return LISI_ERR(LIS_ERR_ILL_ARG, "Size n(=%D) of matrix A is less than 0\n", A->gn);
	if (B != NULL) {                                         /* ref :323-336 */
		LISCHK(lisi_matrix_check(B, LISI_CHECK_ASSEMBLED));
		if (B->n != x->n) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix B (n = %D) and vector x (n = %D) differ in size\n", B->n, x->n);
		if (B->gn <= 0) return LISI_ERR(LIS_ERR_ILL_ARG, "Size n(=%D) of matrix B is less than 0\n", B->gn);
	}
	const LIS_INT nesolver = esolver->options[LIS_EOPTIONS_ESOLVER], ss = esolver->options[LIS_EOPTIONS_SUBSPACE], mode = esolver->options[LIS_EOPTIONS_MODE];
	const LIS_INT emaxiter = esolver->options[LIS_EOPTIONS_MAXITER], output = esolver->options[LIS_EOPTIONS_OUTPUT];
	const LIS_INT estorage = esolver->options[LIS_EOPTIONS_STORAGE], eblock = esolver->options[LIS_EOPTIONS_STORAGE_BLOCK];
	const LIS_INT eprecision = esolver->options[LIS_EOPTIONS_PRECISION];
	if (nesolver < 1 || nesolver > LIS_ESOLVER_LEN) return LISI_ERR(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_ESOLVER is %D (Set between 1 to %D)\n", nesolver, LIS_ESOLVER_LEN);
	const esolver_desc *d = &esolvers[nesolver];
	const int several = (d->flags & E_SS) != 0;
	/* what is not served, said before A or x is touched */
	if (B != NULL && !(d->flags & E_B))                    /* (the reference runs the standard loop and never reads B) */
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "generalized eigenproblems (lis_gesolve with a matrix B) are served by -e gpi | gii | grqi | gcr | gsi | gli | gai: %s (-e %s) is a standard eigensolver, which would ignore B\n",
		                d->name, d->key);
	if ((d->flags & E_B) && B == NULL)                     /* (the reference's loops multiply by that NULL) */
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "eigensolver %s (-e %s) is not served by liblis_amd without a matrix B: lis_esolve serves pi, ii, rqi, cg, cr, si, li, ai, lis_gesolve with a B gpi, gii, grqi, gcr, gsi, gli, gai\n",
		                d->name, d->key);
	if (!d->run)                                           /* -e gcg, the one row without a loop */
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "eigensolver Generalized CG (-e gcg) is not served by liblis_amd: the reference's loop never updates x from its Ritz vector and ends in NaN at every thread count; -e gcr is the generalized solver of that family that works\n");
	if (several && ss == 1)
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, (d->flags & E_B)
		                ? "eigensolver %s (-e %s) serves several pairs; a subspace of one vector (-ss 1, the default) is not served by liblis_amd: one pair is what -e gpi / -e gii serve\n"
		                : "eigensolver %s (-e %s) with a subspace of one vector (-ss 1, the default) is not served by liblis_amd: one eigenpair is what -e pi / -e ii serve\n",
		                d->name, d->key);
	if (lisg.nprocs > 1 || A->nprocs > 1) REFUSE(LIS_ERR_NOT_IMPLEMENTED, "lis_esolve is served on one rank (this job has %D)\n", (LIS_INT)lisg.nprocs);
	if (eprecision != LIS_PRECISION_DOUBLE) {
		if (lisg.quad_precision) REFUSE(LIS_ERR_NOT_IMPLEMENTED, "-ef %s: quad precision eigensolvers are not served by liblis_amd\n", eprecision == LIS_PRECISION_QUAD ? "quad" : "switch");
		REFUSE(LIS_ERR_ILL_ARG, "Quad precision is not enabled\n");
	}
	if (estorage > 0 && estorage != A->matrix_type && !lisi_format_served(estorage))
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "-estorage %D: storage format is not served by liblis_amd\n", estorage);
	if (emaxiter < 0) REFUSE(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_MAXITER(=%D) is less than 0\n", emaxiter);
	if (ss < 1 || mode < 0 || mode > ss + 1) REFUSE(LIS_ERR_ILL_ARG, "Parameters LIS_EOPTIONS_SUBSPACE(=%D), LIS_EOPTIONS_MODE(=%D) are out of range\n", ss, mode);
	if (several) {                                           /* ref :389-411, and the inner eigensolvers the loops can run: -ie's, or -ige's under a B */
		const LIS_INT ninner = esolver->options[(d->flags & E_B) ? LIS_EOPTIONS_INNER_GENERALIZED_ESOLVER : LIS_EOPTIONS_INNER_ESOLVER];
		if (ss > A->gn) REFUSE(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_SUBSPACE is %D (Set less than or equal to matrix size %D)\n", ss, A->gn);
		if (mode >= ss) REFUSE(LIS_ERR_ILL_ARG, "Parameter LIS_EOPTIONS_MODE is %D (Set less than subspace size %D)\n", mode, ss);
		/* (the reference's subspace loops apply a matrix for -ie pi | ii and -ige gpi | gii only -- neither matrix for another -ige; its gcg ends in NaN) */
		if (ninner < 1 || ninner > LIS_ESOLVER_LEN || !(d->inner >> ninner & 1u))
			REFUSE(LIS_ERR_NOT_IMPLEMENTED, (d->flags & E_B) ? "inner generalized eigensolver %D (-ige) is not served by liblis_amd for -e %s (%s)\n"
			                : "inner eigensolver %D (-ie) is not served by liblis_amd for -e %s (%s)\n", ninner, d->key, d->inner_keys);
	}
	/* (explicit: a COO copy looks like CSR in HBM, and lis_matrix_shift_matrix refuses both) */
	if (B != NULL && (lisi_format_one_rank(A->matrix_type) || lisi_format_one_rank(B->matrix_type) || lisi_format_one_rank(estorage)))
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "lis_gesolve: A and B in COO or DNS storage, or in VBR storage (or -estorage coo | dns | vbr), are not served: lis_matrix_shift_matrix does not take them (A, B and x are untouched)\n");
	if (B != NULL && (A->is_splited || B->is_splited || !lisi_format_swept(B->matrix_type) || B->np != B->n || A->np != A->n))
		REFUSE(LIS_ERR_NOT_IMPLEMENTED, "lis_gesolve: A and B must be unsplit matrices in a served storage format without ghost columns (lis_matrix_shift_matrix)\n");
	if (MDEV(A)->device_only && A->matrix_type != LIS_MATRIX_CSR) REFUSE(LIS_ERR_NOT_IMPLEMENTED, "a matrix that lives in HBM only is shifted in CSR storage\n");
	esolver->eprecision = eprecision;

	/* the arrays of the object (ss + 2 entries each, ref :438-550), zeroed */
	arrays_free(esolver);                                    /* (with the eigenvectors an earlier solve left) */
	esolver->evalue = (LIS_SCALAR *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->resid = (LIS_REAL *)calloc((size_t)ss + 2, sizeof(LIS_REAL));
	esolver->iter = (LIS_INT *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->iter2 = (LIS_INT *)calloc((size_t)ss + 2, sizeof(LIS_SCALAR));
	esolver->evector = (LIS_VECTOR *)calloc((size_t)ss + 2, sizeof(LIS_VECTOR));
	esolver->rhistory = (LIS_REAL *)calloc((size_t)emaxiter + 2, sizeof(LIS_REAL));
	if (!esolver->evalue || !esolver->resid || !esolver->iter || !esolver->iter2 || !esolver->evector || !esolver->rhistory)
		REFUSE(LIS_ERR_OUT_OF_MEMORY, "malloc size = %D\n", (LIS_INT)((emaxiter + 2) * sizeof(LIS_REAL)));
	esolver->evalue[0] = 1.0;
	esolver->evalue[ss - 1] = 1.0;
	esolver->rhistory[0] = 1.0;

	/* the initial vector, ref :481-529 */
	if ((err = lis_vector_duplicate(A, &xx))) { esolver->retcode = err; return err; }
	if (esolver->options[LIS_EOPTIONS_INITGUESS_ONES]) {
		if (output) lis_printf(LIS_COMM_WORLD, "initial vector x      : all components set to 1\n");
		err = lis_vector_set_all(1.0, xx);
	} else {
		if (output) lis_printf(LIS_COMM_WORLD, "initial vector x      : user defined\n");
		err = lis_vector_copy(x, xx);
	}
	if (err) goto fail;
	/* -estorage: the caller's matrix itself is converted and stays converted, ref :553-570 (as -storage in lis_solve) */
	if (estorage > 0 && A->matrix_type != estorage && (err = lisi_matrix_retype(A, estorage, estorage == LIS_MATRIX_BSR ? eblock : 0))) goto fail;

	esolver->A = A; esolver->B = B;
	if (output) {
		lis_printf(LIS_COMM_WORLD, "precision             : %s\n", eprecision_keys[eprecision]);
		lis_printf(LIS_COMM_WORLD, "eigensolver           : %s\n", d->name);
		lis_printf(LIS_COMM_WORLD, "convergence condition : ||lx-(B^-1)Ax||_2 <= %6.1e * ||lx||_2\n", (double)esolver->params[LIS_EPARAMS_RESID - LIS_EOPTIONS_LEN]);
		if (A->matrix_type == LIS_MATRIX_BSR) lis_printf(LIS_COMM_WORLD, "matrix storage format : %s(%D x %D)\n", estorage_names[A->matrix_type - 1], eblock, eblock);
		else lis_printf(LIS_COMM_WORLD, "matrix storage format : %s\n", estorage_names[A->matrix_type - 1]);
	}
	double time = lis_wtime();
	esolver->ptime = 0; esolver->itime = 0; esolver->p_c_time = 0; esolver->p_i_time = 0;
	if ((err = work_alloc(esolver, d->work + (d->per_ss ? ss : 0)))) goto fail;
	esolver->x = xx; esolver->xx = x;

	err = d->run(esolver);
	esolver->retcode = err;
	esolver->x = x;
	if (err && err != LIS_MAXITER) goto fail;                /* an inner solve or a device call failed: nothing to hand back */
	*evalue0 = esolver->evalue[0];
	if ((err = lis_vector_copy(xx, x))) goto fail;
	{
		const int rc = liship_stream_synchronize(lisg.stream);
		if (rc != 0) { err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); goto fail; }
	}
	esolver->time = lis_wtime() - time;
	if (output) {
		if (esolver->retcode) lis_printf(LIS_COMM_WORLD, "eigensolver status    : %s(code=%D)\n\n", ereturncode_names[esolver->retcode], esolver->retcode);
		else lis_printf(LIS_COMM_WORLD, "eigensolver status    : normal end\n\n");
	}
	esolver->iter2[mode] = esolver->iter[mode];
	lis_vector_destroy(xx);
	return LIS_SUCCESS;
fail:
	esolver->retcode = err;
	esolver->x = x;
	lis_vector_destroy(xx);
	if (several) arrays_free(esolver);            /* the getters of several pairs answer for a solve that ended */
	return err;
}

LIS_INT lis_esolve(LIS_MATRIX A, LIS_VECTOR x, LIS_SCALAR *evalue0, LIS_ESOLVER esolver)
{
	const LIS_INT err = lis_gesolve(A, NULL, x, evalue0, esolver);
	if (err) { esolver->retcode = err; return err; }
	return LIS_SUCCESS;
}
