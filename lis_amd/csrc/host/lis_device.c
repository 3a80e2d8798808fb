/*
 * lis_device.c -- the device runtime of the host layer: start-up, the work-vector pool, the residency switches, the HBM copies of
 * vectors and their staging, the reductions, and the matrices born in HBM.  The HBM copy of a matrix: lis_upload.c (from host arrays),
 * lis_convert_hbm.c (from a CSR copy in HBM); the products: lis_product.c.
 *
 * Data layout in HBM (f64):
 *   vectors   one buffer of np + pad (+ slack) doubles; owned entries [0,n), ghost entries [n,np)
 */
#include <stdio.h>
#include "lis_internal.h"

/* ------------------------------------------------------------------ runtime */
/* resident mode pays the one-off costs (runtime start-up, matrix upload, row split) where the reference pays its
 * own (lis_initialize, lis_matrix_assemble / _convert), so a driver that times a loop of lis_matvec times products */
LIS_INT lisd_init_quiet(void)
{
	int count = 0;
	if (lisg.device_ready) return LIS_SUCCESS;
	if (liship_device_count(&count) != 0 || count < 1) return LIS_ERR_NOT_IMPLEMENTED;
	return lisd_init();
}

/* the HBM copy of a matrix is built where the matrix is made (assemble / convert) once this process has used the GPU at all: the upload and
 * the plan belong to the conversion, not to the first product a driver times.  RESIDENT, and COHERENT by page protection (whose products
 * then run at resident speed from the first one on); eager COHERENT keeps building it on first use. */
void lisd_mat_eager(LIS_MATRIX A)
{
	if ((lisg.residency == LIS_AMD_RESIDENT || lisp_lazy()) && lisg.device_ready && A->status >= LIS_MATRIX_CSR) (void)lisd_mat_ready(A);
}

static LIS_INT stage_ready(void);
LIS_INT lisd_init(void)
{
	if (lisg.device_ready) return LIS_SUCCESS;
	int count = 0;
	int rc = liship_device_count(&count);
	if (rc != 0 || count < 1) {
		fprintf(stderr, "liblis_amd: no HIP device available (%s) -- this library has no CPU fallback\n",
		        rc ? liship_error_string(rc) : "device count is 0");
		return LIS_ERR_NOT_IMPLEMENTED;
	}
	if (lisg.comm_kind != 1) {           /* the RCCL bootstrap already chose the device */
		/* LIS_AMD_DEVICE, else the launcher's LOCAL_RANK (torchrun, mpirun wrappers: one process per GPU), else device 0 */
		const char *env = getenv("LIS_AMD_DEVICE");
		if (env) lisg.device = atoi(env);
		else { env = getenv("LOCAL_RANK"); lisg.device = env ? atoi(env) % count : 0; }
		if (lisg.device < 0 || lisg.device >= count) lisg.device = 0;
	}
	HIPCHK(liship_set_device(lisg.device));
	HIPCHK(liship_stream_create(&lisg.stream));
	HIPCHK(lisd_malloc(&lisg.reduce_work, liship_reduce_work_bytes()));
	HIPCHK(lisd_malloc((void **)&lisg.reduce_out, 64 * sizeof(double)));      /* (4 for the Krylov passes, LISHIP_MULTIDOT_MAX_PAIRS for lisd_multidot) */
	HIPCHK(liship_malloc_host((void **)&lisg.host_out, 4 * 64 * sizeof(double)));
	HIPCHK(liship_spmv_csr_set_long_row_tree((lisg.long_row_chain || lisg.ref_reductions) ? 0 : 1));     /* parity modes take the chain */
	if (lisg.reference_layout) LISCHK(lis_amd_set_reference_layout(1));
	if (lisg.no_team_kernels) { HIPCHK(liship_spmv_csr_set_team(0)); HIPCHK(liship_spmv_bsr_set_team(0)); }
	if (lisg.no_marching) HIPCHK(liship_spmv_csr_set_dom_march(0));
	{ const char *e = getenv("LIS_AMD_NO_LOCAL_SHORT_ROWS"); lisg.no_local_short_rows = (e && e[0] == '1'); }      /* A/B: short-row plans never try block-local columns (csr_plan_impl) */
	if (lisg.row_block_dots) HIPCHK(liship_spmv_csr_set_row_block_dots(1));
	if (lisg.ref_reductions) HIPCHK(liship_set_reference_reductions(lisg.ref_reductions));
	lisg.device_ready = 1;
	if (lisp_lazy()) (void)stage_ready();      /* the pinned staging buffers of the page-protected vectors: here, not inside a caller's first product */
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ work-vector pool
 * A Krylov solve needs 4 ... restart+3 vectors of the matrix size; hipMalloc/hipFree of tens of GiB cost more
 * than the iterations of a short solve (GMRES(30) at 512^3: 33 GiB, ~1 s).  Buffers released by a solve are
 * kept and handed to the next one that asks for the same size; lis_amd_trim() / lis_finalize() / an allocation
 * failure anywhere give them back to the driver. */
#define POOL_SLOTS 160
static struct { void *p; size_t bytes; } pool[POOL_SLOTS];

/* every HBM allocation of the host layer: when the driver is out of memory the pooled work vectors (up to 33 GiB
 * after a GMRES(30) solve at 512^3) go back to it and the request is tried once more.  Returns the HIP code. */
int lisd_malloc(void **out, size_t bytes)
{
	int rc = liship_malloc(out, bytes);
	if (rc && lis_amd_trim_count() > 0) rc = liship_malloc(out, bytes);
	return rc;
}

LIS_INT lisd_pool_get(size_t bytes, void **out)
{
	for (int i = 0; i < POOL_SLOTS; i++)
		if (pool[i].p && pool[i].bytes == bytes) { *out = pool[i].p; pool[i].p = NULL; return LIS_SUCCESS; }
	HIPCHK(lisd_malloc(out, bytes));
	return LIS_SUCCESS;
}

void lisd_pool_put(void *p, size_t bytes)
{
	if (!p) return;
	for (int i = 0; i < POOL_SLOTS; i++)
		if (!pool[i].p) { pool[i].p = p; pool[i].bytes = bytes; return; }
	(void)liship_free(p);
}

/* gives the pooled buffers back; returns how many there were */
int lis_amd_trim_count(void)
{
	int freed = 0;
	for (int i = 0; i < POOL_SLOTS; i++)
		if (pool[i].p) { (void)liship_free(pool[i].p); pool[i].p = NULL; pool[i].bytes = 0; freed++; }
	return freed;
}
LIS_INT lis_amd_trim(void) { (void)lis_amd_trim_count(); lisd_renum_cache_drop(); return LIS_SUCCESS; }

void *lis_amd_stream(void) { return lisd_init() == LIS_SUCCESS ? lisg.stream : NULL; }

LIS_INT lis_amd_synchronize(void)
{
	LISCHK(lisd_init());
	HIPCHK(liship_device_synchronize());
	return LIS_SUCCESS;
}

LIS_INT lis_amd_set_residency(LIS_INT mode)
{
	if (mode != LIS_AMD_COHERENT && mode != LIS_AMD_RESIDENT) return LISI_ERR(LIS_ERR_ILL_ARG, "unknown residency mode %D\n", mode);
	lisg.residency = mode;
	if (mode == LIS_AMD_RESIDENT) (void)lisd_init_quiet();   /* runtime start-up now, not inside the first product */
	return LIS_SUCCESS;
}
LIS_INT lis_amd_get_residency(void) { return lisg.residency; }

LIS_INT lis_amd_last_solve_uniform_jacobi(void) { return lisg.last_uniform_jacobi; }

LIS_INT lis_amd_set_row_form(LIS_INT on) { lisg.no_row_form = on ? 0 : 1; return LIS_SUCCESS; }
/* The REFERENCE LAYOUT mode (env LIS_AMD_REFERENCE_LAYOUT=1): every product streams the reference's own arrays -- CSR 4 B index[] + 8 B value[] per non-zero + ptr[]
 * (lis_matvec_csr.c:97-109 on SURVEY 8d's 12 B per non-zero + 20 B per row), ELL / DIA / BSR their native arrays -- and nothing the plan could derive from them: no
 * one-byte column codes, row patterns, value records, block-local columns, renumbering or row forms.  Same bits either way; this is the form the CSR roofline target is
 * quoted on and what bench.py's headline runs.  Applies to plans already built (the kernels' own switches) and to matrices uploaded from now on. */
static struct { int saved, codes, patterns, values, rowform, local, reorder; } ref_layout;
LIS_INT lis_amd_set_reference_layout(LIS_INT on)
{
	if (on && !ref_layout.saved) {
		ref_layout.saved = 1;
		ref_layout.codes = lisg.no_index_codes; ref_layout.patterns = lisg.no_row_patterns; ref_layout.values = lisg.no_value_records;
		ref_layout.rowform = lisg.no_row_form; ref_layout.local = lisg.no_local_columns; ref_layout.reorder = lisg.no_reorder;
		lisg.no_index_codes = lisg.no_row_patterns = lisg.no_value_records = lisg.no_row_form = lisg.no_local_columns = lisg.no_reorder = 1;
	} else if (!on && ref_layout.saved) {
		ref_layout.saved = 0;
		lisg.no_index_codes = ref_layout.codes; lisg.no_row_patterns = ref_layout.patterns; lisg.no_value_records = ref_layout.values;
		lisg.no_row_form = ref_layout.rowform; lisg.no_local_columns = ref_layout.local; lisg.no_reorder = ref_layout.reorder;
	}
	lisg.reference_layout = on ? 1 : 0;
	HIPCHK(liship_spmv_csr_set_index_codes(!lisg.no_index_codes)); HIPCHK(liship_spmv_csr_set_row_patterns(!lisg.no_row_patterns));
	HIPCHK(liship_spmv_csr_set_row_values(!lisg.no_value_records)); HIPCHK(liship_spmv_csr_set_local_columns(!lisg.no_local_columns));
	HIPCHK(liship_spmv_csr_set_reorder(lisg.no_reorder ? 0 : 1));
	return LIS_SUCCESS;
}
LIS_INT lis_amd_get_reference_layout(void) { return lisg.reference_layout; }
LIS_INT lis_amd_set_reference_reductions(LIS_INT T)
{
	if (T < 0 || liship_set_reference_reductions((int)T) != 0) return LISI_ERR(LIS_ERR_ILL_ARG, "reference-order reductions: T(=%D) out of range\n", T);
	lisg.ref_reductions = (int)T;
	/* the parity mode wants the reference's bits everywhere: hub rows go back to the left-to-right chain while it is on */
	if (lisg.device_ready) HIPCHK(liship_spmv_csr_set_long_row_tree((lisg.long_row_chain || T > 0) ? 0 : 1));
	return LIS_SUCCESS;
}
LIS_INT lis_amd_get_reference_reductions(void) { return lisg.ref_reductions; }
LIS_INT lis_amd_set_graphs(LIS_INT on) { lisg.graphs = (on != 0); return LIS_SUCCESS; }
LIS_INT lis_amd_last_solve_graph_replays(void) { return lisg.last_graph_replays; }
LIS_INT lis_amd_last_solve_renumbered(void) { return lisg.last_renumbered; }
LIS_INT lis_amd_set_loop_mode(LIS_INT mode)
{
	if (mode < LIS_AMD_LOOP_DEVICE || mode > LIS_AMD_LOOP_UNFUSED) return LISI_ERR(LIS_ERR_ILL_ARG, "unknown loop mode %D\n", mode);
	lisg.host_scalars = (mode == LIS_AMD_LOOP_HOST);
	lisg.no_fusion = (mode == LIS_AMD_LOOP_UNFUSED);
	return LIS_SUCCESS;
}

/* ------------------------------------------------------------------ vectors */
static size_t vec_len(LIS_VECTOR v) { return (size_t)(v->np + v->pad); }

LIS_INT lisd_vec_reserve(LIS_VECTOR v, size_t doubles)
{
	lisd_vec *d = VDEV(v);
	LISCHK(lisd_init());
	if (d->d && d->cap >= doubles) return LIS_SUCCESS;
	const size_t cap = doubles + 16;                      /* slack: BSR kernels read/write whole blocks */
	void *nd = NULL;
	HIPCHK(lisd_malloc(&nd, cap * sizeof(double)));
	HIPCHK(liship_memset(nd, 0, cap * sizeof(double), lisg.stream));
	if (d->d) {
		if (d->dev_valid) HIPCHK(liship_memcpy_d2d(nd, d->d, d->cap * sizeof(double), lisg.stream));
		HIPCHK(liship_stream_synchronize(lisg.stream));
		HIPCHK(liship_free(d->d));
	}
	d->d = (double *)nd;
	d->cap = cap;
	return LIS_SUCCESS;
}

/* Copies between page-protected host arrays and HBM go through two pinned staging buffers.  Handing the vector's own pages to the runtime
 * would make it register them with the driver (a pageable copy of this size pins its source), and every later mprotect of registered pages
 * is an MMU-notifier invalidation inside the kernel driver: measured 30 - 35 ms per 64 MB vector, four times the copy itself.  With the
 * staging buffers the driver never learns about the pages; the host memcpy overlaps the DMA of the previous piece. */
#define STAGE_BYTES ((size_t)16 << 20)
static struct { void *buf[2], *ev[2]; int busy[2]; } stage;
/* the staging buffers are one set per process: a thread of the program that faults on a vector (lis_pages.c) copies through them while the
 * thread that drives the library may be uploading another vector -- one copy at a time */
#include <pthread.h>
#include <unistd.h>
static pthread_mutex_t stage_lock = PTHREAD_MUTEX_INITIALIZER;

static LIS_INT stage_ready(void)
{
	if (stage.buf[0]) return LIS_SUCCESS;
	for (int k = 0; k < 2; k++) {
		HIPCHK(liship_malloc_host(&stage.buf[k], STAGE_BYTES));
		HIPCHK(liship_event_create(&stage.ev[k]));
	}
	return LIS_SUCCESS;
}

/* memcpy by the host threads (one thread moves ~10 GB/s, PCIe 5 takes 50) -- except inside the page-fault handler, which runs on whatever thread of the
 * program touched the page: no OpenMP region is opened from a signal handler (the faulting thread may sit inside a region of its own) */
static __thread int in_fault_copy;
static void copy_threads(void *dst, const void *src, size_t bytes)
{
	const size_t piece = (size_t)1 << 20;
	const long long pieces = (long long)((bytes + piece - 1) / piece);
	if (pieces < 4 || in_fault_copy) { memcpy(dst, src, bytes); return; }
	const int T = lisi_host_threads();
#pragma omp parallel for num_threads(T) schedule(static)
	for (long long i = 0; i < pieces; i++) {
		const size_t off = (size_t)i * piece, len = bytes - off < piece ? bytes - off : piece;
		memcpy((char *)dst + off, (const char *)src + off, len);
	}
}

static LIS_INT staged_h2d_locked(void *dst, const void *src, size_t bytes)
{
	LISCHK(stage_ready());
	int k = 0;
	for (size_t off = 0; off < bytes; off += STAGE_BYTES, k ^= 1) {
		const size_t len = bytes - off < STAGE_BYTES ? bytes - off : STAGE_BYTES;
		if (stage.busy[k]) { HIPCHK(liship_event_synchronize(stage.ev[k])); stage.busy[k] = 0; }
		copy_threads(stage.buf[k], (const char *)src + off, len);
		HIPCHK(liship_memcpy_h2d((char *)dst + off, stage.buf[k], len, lisg.stream));
		HIPCHK(liship_event_record(stage.ev[k], lisg.stream));
		stage.busy[k] = 1;
	}
	return LIS_SUCCESS;
}
static LIS_INT staged_h2d(void *dst, const void *src, size_t bytes)
{
	pthread_mutex_lock(&stage_lock);
	const LIS_INT err = staged_h2d_locked(dst, src, bytes);
	pthread_mutex_unlock(&stage_lock);
	return err;
}

static LIS_INT staged_d2h_locked(void *dst, const void *src, size_t bytes)
{
	LISCHK(stage_ready());
	for (int k = 0; k < 2; k++) if (stage.busy[k]) { HIPCHK(liship_event_synchronize(stage.ev[k])); stage.busy[k] = 0; }
	size_t issued = 0, landed = 0;
	int ki = 0, kl = 0;
	while (landed < bytes) {
		while (issued < bytes && issued - landed < 2 * STAGE_BYTES) {          /* keep both buffers in flight */
			const size_t len = bytes - issued < STAGE_BYTES ? bytes - issued : STAGE_BYTES;
			HIPCHK(liship_memcpy_d2h(stage.buf[ki], (const char *)src + issued, len, lisg.stream));
			HIPCHK(liship_event_record(stage.ev[ki], lisg.stream));
			issued += len; ki ^= 1;
		}
		const size_t len = bytes - landed < STAGE_BYTES ? bytes - landed : STAGE_BYTES;
		HIPCHK(liship_event_synchronize(stage.ev[kl]));
		copy_threads((char *)dst + landed, stage.buf[kl], len);
		landed += len; kl ^= 1;
	}
	return LIS_SUCCESS;
}
/* HBM -> host memory the runtime must not learn about (page-protected arrays, through their alias mapping: lis_pages.c) */
LIS_INT lisd_staged_d2h(void *dst, const void *src, size_t bytes)
{
	pthread_mutex_lock(&stage_lock);
	const LIS_INT err = staged_d2h_locked(dst, src, bytes);
	pthread_mutex_unlock(&stage_lock);
	return err;
}

/* The same copy from INSIDE the page-fault handler (lis_pages.c on_fault), i.e. on a thread of the program, possibly while the thread that drives the library is
 * enqueueing work: a stream, two pinned buffers and two events of its own (made when the handler is installed, never inside it), so that nothing is enqueued on
 * the library's stream from a foreign thread -- a stream under hipGraph capture (LIS_AMD_GRAPHS=1) would have its capture invalidated -- and the driving
 * thread's staging buffers are never waited for.  What the data depends on has been enqueued on lisg.stream by the time its pages lost their access: the copy
 * waits for an event recorded there... by THIS thread, which is legal on a capturing stream only outside the capture, so a fault during a capture waits for
 * the capture to end first (a batch of launches: microseconds).  Plain memcpy, no OpenMP. */
static struct { void *stream, *buf[2], *ev[2], *order; int ready; } fstage;
static volatile int capture_active;
static pthread_t capture_thread;                                    /* the thread that began the capture in progress */
static pthread_mutex_t fault_lock = PTHREAD_MUTEX_INITIALIZER;      /* one fault-time copy at a time; a capture begins only between two of them */
void lisd_capture_mark(int on)
{
	if (on) { pthread_mutex_lock(&fault_lock); capture_thread = pthread_self(); capture_active = 1; pthread_mutex_unlock(&fault_lock); }
	else capture_active = 0;
}
LIS_INT lisd_fault_stage_prepare(void)
{
	if (fstage.ready || !lisg.device_ready) return LIS_SUCCESS;
	HIPCHK(liship_stream_create(&fstage.stream));
	for (int k = 0; k < 2; k++) {
		HIPCHK(liship_malloc_host(&fstage.buf[k], STAGE_BYTES));
		HIPCHK(liship_event_create(&fstage.ev[k]));
	}
	HIPCHK(liship_event_create(&fstage.order));
	fstage.ready = 1;
	return LIS_SUCCESS;
}
LIS_INT lisd_staged_d2h_fault(void *dst, const void *src, size_t bytes)
{
	if (!fstage.ready) {               /* (the handler was installed before the device existed: the shared path -- with plain memcpy: no OpenMP region from inside a signal handler) */
		in_fault_copy = 1;
		const LIS_INT e = lisd_staged_d2h(dst, src, bytes);
		in_fault_copy = 0;
		return e;
	}
	LIS_INT err = LIS_SUCCESS;
	pthread_mutex_lock(&fault_lock);
	/* a capture in progress is waited out -- a batch of launches, microseconds.  Two ways this could never end, both loud instead of a silent spin:
	 * the capturing thread ITSELF faulted (nobody is left to end the capture), or the capture was abandoned on an error path without lisd_capture_mark(0) */
	if (capture_active && pthread_equal(capture_thread, pthread_self())) {
		fprintf(stderr, "liblis_amd: the thread that is capturing a hipGraph touched a page-protected array whose data lives in HBM: the copy cannot be ordered inside the capture -- aborting\n");
		abort();
	}
	for (int waited_us = 0; capture_active; waited_us += 50) {
		if (waited_us > 10 * 1000 * 1000) {
			fprintf(stderr, "liblis_amd: a hipGraph capture has not ended for 10 s while a page fault waits for it: taking the capture for abandoned\n");
			capture_active = 0;
			break;
		}
		usleep(50);
	}
	int rc = liship_event_record(fstage.order, lisg.stream);
	if (!rc) rc = liship_stream_wait_event(fstage.stream, fstage.order);
	in_fault_copy = 1;
	size_t issued = 0, landed = 0;
	int ki = 0, kl = 0;
	while (!rc && landed < bytes) {
		while (!rc && issued < bytes && issued - landed < 2 * STAGE_BYTES) {
			const size_t len = bytes - issued < STAGE_BYTES ? bytes - issued : STAGE_BYTES;
			rc = liship_memcpy_d2h(fstage.buf[ki], (const char *)src + issued, len, fstage.stream);
			if (!rc) rc = liship_event_record(fstage.ev[ki], fstage.stream);
			issued += len; ki ^= 1;
		}
		if (rc) break;
		const size_t len = bytes - landed < STAGE_BYTES ? bytes - landed : STAGE_BYTES;
		rc = liship_event_synchronize(fstage.ev[kl]);
		if (!rc) memcpy((char *)dst + landed, fstage.buf[kl], len);
		landed += len; kl ^= 1;
	}
	in_fault_copy = 0;
	if (rc) { (void)liship_stream_synchronize(fstage.stream); err = lisi_hip_error(__FILE__, __func__, __LINE__, rc); }
	pthread_mutex_unlock(&fault_lock);
	return err;
}

/* host -> HBM when the host side is the truth.  COHERENT with page protection (the default, lis_pages.c): the host array was written
 * since the last upload exactly when its pages are read + write (dev_valid == 0); eager COHERENT: always (nothing tells) */
LIS_INT lisd_vec_in(LIS_VECTOR v, double **out)
{
	lisd_vec *d = VDEV(v);
	LISCHK(lisd_vec_reserve(v, vec_len(v)));
	const int lazy = lisp_lazy() && d->region;
	const int host_is_truth = (lisg.residency == LIS_AMD_COHERENT && !lazy) ? (d->host_valid || !d->dev_valid) : !d->dev_valid;
	if (host_is_truth && v->value) {
		size_t len = d->hlen < d->cap ? d->hlen : d->cap;
		if (lazy) LISCHK(staged_h2d(d->d, v->value, len * sizeof(double)));          /* (the array has been read when this returns) */
		else HIPCHK(liship_memcpy_h2d(d->d, v->value, len * sizeof(double), lisg.stream));
		d->dev_valid = 1;
		if (lisg.residency == LIS_AMD_COHERENT) d->host_valid = 1;
		if (lazy) {
			lisp_protect(v, LISP_RO);        /* both sides agree: a host write from here on faults and marks the HBM copy stale */
			/* the protection could not be had (mprotect out of VMAs, no handler): nothing would report a host write, so the HBM copy
			 * counts as stale again and the next call uploads afresh -- slower, never wrong */
			if (lisp_state(v) != LISP_RO) d->dev_valid = 0;
		}
	}
	*out = d->d;
	return LIS_SUCCESS;
}

LIS_INT lisd_vec_out(LIS_VECTOR v, double **out)
{
	LISCHK(lisd_vec_reserve(v, vec_len(v)));
	*out = VDEV(v)->d;
	return LIS_SUCCESS;
}

LIS_INT lisd_vec_done(LIS_VECTOR v)
{
	lisd_vec *d = VDEV(v);
	d->dev_valid = 1;
	d->host_valid = 0;
	if (lisg.residency == LIS_AMD_COHERENT) {
		if (lisp_lazy() && d->region) { lisp_protect(v, LISP_NONE); if (lisp_state(v) == LISP_NONE) return LIS_SUCCESS; }   /* the first host access brings it home */
		return lisd_vec_to_host(v);
	}
	return LIS_SUCCESS;
}

LIS_INT lisd_vec_to_host(LIS_VECTOR v)
{
	lisd_vec *d = VDEV(v);
	if (lisp_lazy() && d->region) return lisp_vec_home(v);      /* through the alias mapping: the program's pages open when the data is there */
	if (d->host_valid || !d->dev_valid || !d->d || !v->value) {
		d->host_valid = 1;
		lisp_protect(v, LISP_RW);                 /* (pages of a vector protected before the mode was switched to eager) */
		return LIS_SUCCESS;
	}
	size_t len = d->hlen < d->cap ? d->hlen : d->cap;
	lisp_protect(v, LISP_RW);
	HIPCHK(liship_memcpy_d2h(v->value, d->d, len * sizeof(double), lisg.stream));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	d->host_valid = 1;
	return LIS_SUCCESS;
}

/* the library itself is about to write value[] on the host: current data first when `keep`, pages writable, HBM copy stale */
LIS_INT lisd_vec_host_write(LIS_VECTOR v, int keep)
{
	lisd_vec *d = VDEV(v);
	if (keep && !d->host_valid) LISCHK(lisd_vec_to_host(v));
	lisp_protect(v, LISP_RW);
	d->host_valid = 1;
	d->dev_valid = 0;
	return LIS_SUCCESS;
}

void lisd_vec_free(LIS_VECTOR v)
{
	lisd_vec *d = VDEV(v);
	if (d->d) { (void)liship_free(d->d); d->d = NULL; d->cap = 0; }
	d->dev_valid = 0;
}

LIS_INT lis_amd_vector_sync_host(LIS_VECTOR v) { return lisd_vec_to_host(v); }
LIS_INT lis_amd_vector_host_modified(LIS_VECTOR v) { lisp_protect(v, LISP_RW); VDEV(v)->host_valid = 1; VDEV(v)->dev_valid = 0; return LIS_SUCCESS; }
LIS_INT lis_amd_vector_device_modified(LIS_VECTOR v) { VDEV(v)->host_valid = 0; VDEV(v)->dev_valid = 1; if (lisp_lazy()) lisp_protect(v, LISP_NONE); return LIS_SUCCESS; }
LIS_INT lis_amd_vector_device_ptr(LIS_VECTOR v, LIS_SCALAR **dptr) { return lisd_vec_in(v, dptr); }

/* ------------------------------------------------------------------ reductions -> host scalars */
LIS_INT lisd_fetch(int count, double *out)
{
	if (lisg.nprocs > 1 && lisg.comm_kind == 1)        /* RCCL gathers the partials straight from HBM: one sync, not two */
		return lisc_fold(count, out);
	LISCHK(lisd_fetch_from(lisg.reduce_out, count, out));
	if (lisg.nprocs > 1) LISCHK(lisc_fold(count, out));
	return LIS_SUCCESS;
}

/* count doubles from an HBM address to the host, as they are: through the page-locked landing zone, beyond its 256 doubles straight into out */
LIS_INT lisd_fetch_from(const double *dsrc, int count, double *out)
{
	double *land = count <= 256 ? lisg.host_out : out;
	HIPCHK(liship_memcpy_d2h(land, dsrc, (size_t)count * sizeof(double), lisg.stream));
	HIPCHK(liship_stream_synchronize(lisg.stream));
	if (land != out) memcpy(out, land, (size_t)count * sizeof(double));
	return LIS_SUCCESS;
}

/* RCCL job: replace this rank's sums in HBM by the sums over all ranks, without leaving the stream */
LIS_INT lisd_globalize(double *slot, int count)
{
	if (lisg.comm_kind != 1) return LIS_SUCCESS;
	LISCHK(lisc_gather_device(slot, count));
	HIPCHK(liship_rank_fold_f64(count, lisg.gather_out, lisg.nprocs, slot, lisg.stream));
	return LIS_SUCCESS;
}

/* The middle of a modified Gram-Schmidt chain whose coefficients stay in HBM: with hdev[0] = <w, basis[0]> formed by the caller, step k = 1 .. m - 1
 * applies coefficient k - 1 (w -= hdev[k-1] * basis[k-1]) and forms hdev[k] = <w, basis[k]> in the same pass, each made global across the ranks; nothing
 * waits for the host.  How the chain starts and how it ends -- coefficient m - 1 is still to be applied -- is the caller's. */
LIS_INT lisd_mgs_chain(int n, int m, double *const *basis, double *w, double *hdev)
{
	for (int k = 1; k < m; k++) {
		HIPCHK(liship_mgs_step_f64(n, hdev + k - 1, basis[k - 1], w, basis[k], hdev + k, lisg.reduce_work, lisg.stream));
		LISCHK(lisd_globalize(hdev + k, 1));
	}
	return LIS_SUCCESS;
}

LIS_INT lisd_dot(int n, const double *dx, const double *dy, double *out)
{
	HIPCHK(liship_dot_f64(n, dx, dy, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	return lisd_fetch(1, out);
}

LIS_INT lisd_nrm2(int n, const double *dx, double *out)
{
	/* the root is taken after the cross-rank fold (ref lis_vector_ops.c:263-264) */
	HIPCHK(liship_sumsq_f64(n, dx, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	LISCHK(lisd_fetch(1, out));
	*out = sqrt(*out);
	return LIS_SUCCESS;
}

LIS_INT lisd_nrm1(int n, const double *dx, double *out)
{
	HIPCHK(liship_nrm1_f64(n, dx, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	return lisd_fetch(1, out);
}

LIS_INT lisd_dot2(int n, const double *dx, const double *dy, double *out2)
{
	HIPCHK(liship_dot2_f64(n, dx, dy, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	return lisd_fetch(2, out2);
}

/* out[k] = <dv[pairs[k][0]], dv[pairs[k][1]]>, k < K <= LISHIP_MULTIDOT_MAX_PAIRS: one pass over the vectors and one read-back (liship_multidot_f64), or -- with
 * LIS_AMD_NO_FUSION=1 / the UNFUSED loop mode, and in a multi-rank job, whose fold takes 4 sums at a time -- K dots.  The same bits either way. */
LIS_INT lisd_multidot(int n, int nvec, const double *const *dv, int K, const int (*pairs)[2], double *out)
{
	if (lisg.no_fusion || lisg.nprocs > 1) {
		for (int k = 0; k < K; k++) LISCHK(lisd_dot(n, dv[pairs[k][0]], dv[pairs[k][1]], &out[k]));
		return LIS_SUCCESS;
	}
	HIPCHK(liship_multidot_f64(n, nvec, dv, K, pairs, lisg.reduce_out, lisg.reduce_work, lisg.stream));
	return lisd_fetch(K, out);
}

/* ------------------------------------------------------------------ matrices born in HBM */
LIS_INT lis_amd_matrix_set_csr_device(LIS_INT nnz, LIS_INT np, LIS_INT *dptr, LIS_INT *dindex,
                                      LIS_SCALAR *dvalue, LIS_MATRIX A)
{
	if (!lisi_is_registered(A)) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is undefined\n");
	if (A->status != LIS_MATRIX_NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A must be sized and not yet assembled\n");
	if (np < A->n) return LISI_ERR(LIS_ERR_ILL_ARG, "np(=%D) is smaller than n(=%D)\n", np, A->n);
	LISCHK(lisd_init());
	lisd_mat *d = MDEV(A);
	d->device_only = 1;
	d->type = LIS_MATRIX_CSR;
	d->n = A->n; d->np = np; d->nnz = nnz;
	d->ptr = dptr; d->index = dindex; d->value = dvalue;
	LISCHK(lisd_csr_plan_cols(&d->plan, A->n, np, d->ptr, d->index, d->value));
	d->inner_begin = 0; d->inner_end = A->n;
	d->ready = 1;
	A->nnz = nnz; A->np = np;
	A->is_copy = LIS_FALSE;
	A->matrix_type = LIS_MATRIX_CSR;
	A->status = LIS_MATRIX_CSR;                /* assembled: there is nothing left to do on the host */
	return LIS_SUCCESS;
}

LIS_INT lis_amd_matrix_poisson3d(LIS_MATRIX A, LIS_INT l, LIS_INT m, LIS_INT n, LIS_INT sorted)
{
	if (!lisi_is_registered(A)) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A is undefined\n");
	if (A->status != LIS_MATRIX_NULL) return LISI_ERR(LIS_ERR_ILL_ARG, "matrix A must be sized and not yet assembled\n");
	const long long mn = (long long)m * n, gn = mn * l;
	if (gn != A->gn) return LISI_ERR(LIS_ERR_ILL_ARG, "grid %D x %D x %D does not match the global size\n", l, m, n);
	const long long nnz = liship_poisson3d_nnz(l, m, n, A->is, A->ie);
	if (nnz < 0) return LISI_ERR(LIS_ERR_ILL_ARG, "rows [%D,%D) are not whole grid planes of %D rows\n", A->is, A->ie, (LIS_INT)mn);
	LISCHK(lisd_init());
	const LIS_INT nloc = A->n, nlow = A->is > 0 ? (LIS_INT)mn : 0, nup = A->ie < gn ? (LIS_INT)mn : 0;
	int *dptr = NULL, *didx = NULL; double *dval = NULL;
	HIPCHK(lisd_malloc((void **)&dptr, sizeof(int) * ((size_t)nloc + 1 + 4)));
	HIPCHK(lisd_malloc((void **)&didx, sizeof(int) * ((size_t)nnz + 4)));
	HIPCHK(lisd_malloc((void **)&dval, sizeof(double) * ((size_t)nnz + 2)));
	HIPCHK(liship_poisson3d_csr(l, m, n, A->is, A->ie, sorted, dptr, didx, dval, lisg.stream));
	LISCHK(lis_amd_matrix_set_csr_device((LIS_INT)nnz, nloc + nlow + nup, dptr, didx, dval, A));
	if (A->nprocs > 1) {
		/* halo tables in closed form: one plane to/from the rank below and above (ghosts ascending: low first) */
		const LIS_INT ns = nlow + nup;
		A->l2g_map = (LIS_INT *)malloc(sizeof(LIS_INT) * (size_t)(ns > 0 ? ns : 1));
		for (LIS_INT i = 0; i < nlow; i++) A->l2g_map[i] = A->is - (LIS_INT)mn + i;
		for (LIS_INT i = 0; i < nup; i++) A->l2g_map[nlow + i] = A->ie + i;
		LIS_COMMTABLE t = (LIS_COMMTABLE)calloc(1, sizeof(struct LIS_COMMTABLE_STRUCT));
		const LIS_INT nb = (nlow ? 1 : 0) + (nup ? 1 : 0);
		t->neibpe = (LIS_INT *)malloc(sizeof(LIS_INT) * 2);
		t->import_ptr = (LIS_INT *)calloc(3, sizeof(LIS_INT)); t->export_ptr = (LIS_INT *)calloc(3, sizeof(LIS_INT));
		t->import_index = (LIS_INT *)malloc(sizeof(LIS_INT) * (size_t)(ns > 0 ? ns : 1));
		t->export_index = (LIS_INT *)malloc(sizeof(LIS_INT) * (size_t)(ns > 0 ? ns : 1));
		LIS_INT q = 0;
		if (nlow) { t->neibpe[q] = A->my_rank - 1; t->import_ptr[q + 1] = t->import_ptr[q] + nlow; t->export_ptr[q + 1] = t->export_ptr[q] + nlow;
			for (LIS_INT i = 0; i < nlow; i++) t->export_index[t->export_ptr[q] + i] = i; q++; }
		if (nup)  { t->neibpe[q] = A->my_rank + 1; t->import_ptr[q + 1] = t->import_ptr[q] + nup;  t->export_ptr[q + 1] = t->export_ptr[q] + nup;
			for (LIS_INT i = 0; i < nup; i++) t->export_index[t->export_ptr[q] + i] = nloc - (LIS_INT)mn + i; q++; }
		for (LIS_INT i = 0; i < ns; i++) t->import_index[i] = nloc + i;
		t->comm = A->comm; t->neibpetot = nb; t->imnnz = ns; t->exnnz = ns; t->wssize = ns; t->wrsize = ns;
		t->ws = (LIS_SCALAR *)malloc(sizeof(LIS_SCALAR) * (size_t)(ns > 0 ? ns : 1));
		t->wr = (LIS_SCALAR *)malloc(sizeof(LIS_SCALAR) * (size_t)(ns > 0 ? ns : 1));
		A->commtable = t;
		A->is_comm = LIS_TRUE;
		MDEV(A)->inner_begin = nlow; MDEV(A)->inner_end = nloc - nup;
	}
	return LIS_SUCCESS;
}

LIS_INT lis_amd_vector_poisson3d_rhs(LIS_VECTOR b, LIS_INT l, LIS_INT m, LIS_INT n)
{
	double *db;
	LISCHK(lisd_vec_out(b, &db));
	HIPCHK(liship_poisson3d_rhs(l, m, n, b->is, b->ie, db, lisg.stream));
	return lisd_vec_done(b);
}
