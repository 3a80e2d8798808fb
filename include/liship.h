/*
 * liship.h -- kernel-level C ABI of the MI355X (gfx950) hot path: plain device pointers and sizes.
 *
 * This is the layer a Lis maintainer binds from C: each entry point replaces one
 * OpenMP hot loop of the reference (anishida/lis 2.1.11; citations are file:line under /root/reference).
 * Everything here is hand-written HIP; there is no CPU fallback -- a call on a machine without a
 * gfx950 device fails with a HIP error code.
 *
 * Conventions
 *   - all array arguments are DEVICE pointers (hipMalloc'd), int32 indices, f64 scalars
 *     (LIS_INT / LIS_SCALAR of the reference's default build, include/lis.h:446,461);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 on success, otherwise the hipError_t of the failing runtime call, or
 *     LISHIP_ERR_ARG (-1) for an argument the kernel cannot serve;
 *   - arithmetic: one rounded multiply and one rounded add per term (no FMA contraction), rows summed
 *     strictly in stored order starting from +0.0 -- bit-identical to the reference's CPU loops.
 */
#ifndef LISHIP_H
#define LISHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISHIP_ERR_ARG (-1)

/* ------------------------------------------------------------------ device / memory utilities */
int  liship_device_count(int *count);
int  liship_set_device(int device);
int  liship_get_device(int *device);
int  liship_device_name(char *buf, int buflen);           /* e.g. "gfx950:sramecc+:xnack-" */
int  liship_malloc(void **dptr, size_t bytes);
int  liship_free(void *dptr);
int  liship_memset(void *dptr, int byte, size_t bytes, void *stream);
int  liship_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int  liship_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int  liship_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int  liship_stream_create(void **stream);
int  liship_stream_destroy(void *stream);
int  liship_stream_synchronize(void *stream);
/* watchdog for streams that carry collectives: with a limit > 0 liship_stream_synchronize polls and returns LISHIP_ERR_TIMEOUT (-2) when the stream has not
 * drained within `seconds` (a peer that never arrived); 0 = wait for ever (default) */
int  liship_set_sync_timeout(double seconds);
#define LISHIP_ERR_TIMEOUT (-2)
int  liship_device_synchronize(void);
/* hipGraph capture of whatever is enqueued on `stream` between begin and end (the Krylov loops replay a batch of
 * iterations this way when the system is small enough to be launch bound -- the reference has no counterpart: its
 * loops are host code, src/solver/lis_solver_cg.c:176-215).  capture_end always ends the capture; with exec == NULL the
 * recording is dropped.  A failed capture leaves the stream usable for plain launches. */
int  liship_graph_capture_begin(void *stream);
int  liship_graph_capture_end(void *stream, void **exec);
int  liship_graph_launch(void *exec, void *stream);
int  liship_graph_destroy(void *exec);
/* HIP-event stopwatch on `stream`: start/stop bracket a region, elapsed_ms reads it after stop+sync */
/* page-locked host memory for the scalar read-backs */
int  liship_malloc_host(void **ptr, size_t bytes);
int  liship_free_host(void *ptr);
/* stream-ordering events: record on one stream, make another stream wait (no host involvement) */
int  liship_event_create(void **event);
int  liship_event_destroy(void *event);
int  liship_event_record(void *event, void *stream);
int  liship_event_synchronize(void *event);
int  liship_stream_wait_event(void *stream, void *event);
/* the box's streaming yardstick: every workgroup sums `reads` (1, 2, 4, 8 or 13) consecutive 512-double tiles of src (reads * n doubles) into one tile of dst (n doubles),
 * nontemporal, no gather: what a kernel with the products' read : write ratio reaches on THIS box (bench.py reports it beside the product's roofline fraction); n % 512 == 0 */
int  liship_stream_yardstick(int reads, size_t n, const double *src, double *dst, int wgs_per_cu /* 0: a workgroup per tile, else persistent workgroups per CU */, void *stream);
int  liship_timer_create(void **timer);
int  liship_timer_destroy(void *timer);
int  liship_timer_start(void *timer, void *stream);
int  liship_timer_stop(void *timer, void *stream);
int  liship_timer_elapsed_ms(void *timer, float *ms);
const char *liship_error_string(int code);

/* ------------------------------------------------------------------ CSR SpMV
 * replaces lis_matvec_csr, src/matvec/lis_matvec_csr.c:90-110 (unsplit branch):
 *     y[i] = sum_{j=ptr[i]}^{ptr[i+1]-1} value[j] * x[index[j]]      (in stored order)
 *
 * A plan is the nnz-balanced row split of one matrix (merge-path coordinates row+nnz, whole rows per
 * workgroup); it depends only on ptr[] and is built once per matrix on the device. */
typedef struct liship_csr_plan_s *liship_csr_plan_t;
int  liship_csr_plan_create(liship_csr_plan_t *plan, int n, const int *ptr, void *stream);
/* Index coding (setup-time, optional, never an error when the matrix does not qualify): if the entries of the matrix sit
 * on at most 255 distinct diagonals -- every structured-grid discretisation -- the plan keeps ONE byte per non-zero
 * (the position of column - row in a sorted dictionary) and the row-gather kernel streams 9 B per non-zero instead
 * of 12.  Same terms in the same order: results are bit-identical.  The index array must stay valid (long rows, array
 * tails and row-range launches may still read it).  liship_csr_plan_coded: dictionary size, 0 if not coded.
 * liship_spmv_csr_set_index_codes(0) makes every product ignore the codes (A/B measurements). */
int  liship_csr_plan_encode_indices(liship_csr_plan_t plan, const int *ptr, const int *index, void *stream);
int  liship_csr_plan_coded(liship_csr_plan_t plan);
/* Row patterns (setup-time, optional, after liship_csr_plan_encode_indices; never an error when the matrix does not qualify):
 * when the rows of a coded matrix follow at most 255 distinct (length, offset sequence) patterns -- a 7-point stencil has 27 --
 * the plan keeps ONE byte per row (its pattern) and a 2 B row start relative to the row block instead of one byte per
 * non-zero and the 4 B row pointer: 75 instead of 83 B per stencil row.  Same terms in the same order: bit-identical.
 * liship_csr_plan_row_patterns: number of patterns, 0 if none.  liship_spmv_csr_set_row_patterns(0): A/B switch.
 * When every pattern has 1..7 offsets (and there are at most 64, n < 2^29) the plan also keeps them as 32 B records and the
 * products run through the kernel that issues its x gathers ahead of the value slice: liship_csr_plan_pattern_records = 1. */
int  liship_csr_plan_encode_row_patterns(liship_csr_plan_t plan, const int *ptr, void *stream);
int  liship_csr_plan_row_patterns(liship_csr_plan_t plan);
int  liship_csr_plan_pattern_records(liship_csr_plan_t plan);
/* When the longest pattern has 8..32 offsets (the 27-point stencil) the plan keeps 144 B records (32 byte offsets, length) and the
 * values-streamed product runs four lanes per row, the gathers leaving ahead of the value slice and the row's one ordered sum handed
 * from lane to lane in registers (spmv_csr_pattern_team_kernel): liship_csr_plan_team_records = 1. */
int  liship_csr_plan_team_records(liship_csr_plan_t plan);
/* ... and when ONE pattern carries most rows and its sorted offsets are runs of consecutive columns of one length (the box stencils), the x a
 * wavefront's 16 neighbouring rows need is staged in LDS by a few coalesced loads instead of a gather per entry (spmv_csr_pattern_team_staged_kernel):
 * liship_csr_plan_team_form = 2 (1: the gathers of the first form; 0: no team records). */
int  liship_csr_plan_team_form(liship_csr_plan_t plan);
/* 1 when a plan with WIDE value records (constant-coefficient rows of up to 32 entries) also found a dominant pattern and runs the kernel with x staged per
 * wavefront and that pattern's slots and values in scalar registers (spmv_csr_valuerecw_staged_kernel) */
int  liship_csr_plan_wide_dominant(liship_csr_plan_t plan);
/* 1 when, on top of that, the matrix is the 27-point box stencil with constant coefficients on a grid that IS a box (lines of any even length from 128 on -- round 5: partial tiles --, rows in ascending
 * column order; checked row by row at plan time) and its whole-matrix product walks the planes of 128-column tiles with each x loaded once (round 5:
 * spmv_csr_box27_march_kernel -- x and y alone are streamed); liship_spmv_csr_set_dom_march(0) keeps the staged kernel (A/B), 2 marches at any size (tests) */
int  liship_csr_plan_box27(liship_csr_plan_t plan);
/* 0 when the products of this plan run a kernel with a row split of its own (the team / staged kernels) under the switches in force: the fused entry points
 * (liship_spmv_csr_dot_f64, liship_spmv_csr_rows_dot_f64) then refuse with LISHIP_ERR_ARG and the caller runs the product and one reduction pass */
int  liship_csr_plan_fused_dots(liship_csr_plan_t plan);
long long liship_csr_plan_fused_slots(liship_csr_plan_t plan);   /* upper bound of the reduction slots the fused product needs in up to three row ranges */
int  liship_spmv_csr_set_team(int on);           /* A/B switch: 0 = the one-lane-per-row pattern kernel for these rows too (same bits) */
/* Block rows on top of the wide value records: the rows b i .. b i + b - 1 of the matrix list the SAME columns in the same order (the row form of a b x b BSR matrix,
 * liship_bsr_to_rows; b = 2, 3, 4).  When one block row pattern carries half of the block rows, the product gives a LANE a block row: each x read once from the
 * wavefront's staged window feeds the b running sums, the b x len values are kernel arguments (spmv_csr_blockrows_staged_kernel).  Optional, never an error when the
 * matrix does not qualify; row ranges that cut a block row run the row-by-row kernels.  Bits of lis_matvec_bsr.c:293-343. */
int  liship_csr_plan_encode_block_rows(liship_csr_plan_t plan, int b, const int *ptr, void *stream);
int  liship_csr_plan_block_rows(liship_csr_plan_t plan);       /* b when the plan keeps them, else 0 */
/* 1 when those block rows are the 7-point stencil in 2 x 2 blocks on a grid that is a box (lines of any even length from 128 on -- round 5: partial tiles --; checked block row by block row at plan time)
 * and the whole-matrix product walks the planes with each x loaded once (round 5: spmv_csr_block2_march_kernel); liship_spmv_csr_set_dom_march as for the others */
int  liship_csr_plan_block2_march(liship_csr_plan_t plan);
int  liship_spmv_csr_set_block_rows(int on);                   /* A/B switch: 0 = the row-by-row kernels (same bits) */
/* The z-marching form of the dominant-pattern product (7-point stencil with value records, grid lines of any even length from 128 on: the last 128-column tile of a line may be partial): 1 = on for launches of 64 workgroups and more (default), 0 = the gathering kernel, 2 = on at any size,
 * 3 = at any size, but with the faces' masks even where plan time found the grid a box (liship_csr_plan_box_planes: planes in which a slot is missing exactly where its neighbour
 * lies outside the grid -- there the kernel reads no pattern byte at all).  Same bits in every form. */
int  liship_spmv_csr_set_dom_march(int on);
int  liship_csr_plan_box_planes(liship_csr_plan_t plan);
int  liship_csr_plan_marching(liship_csr_plan_t plan);       /* the whole-matrix product: 0 = the gathering kernels, 1 = z-marching with the faces' masks, 2 = its box form (no pattern bytes) */
int  liship_spmv_csr_set_wide_union(int on);     /* plan-time A/B switch: 0 = no virtual dominant pattern (a common supersequence of the patterns rows take turns on: b x b blocked stencils), 1 = from 2^19 rows on (default), 2 = at any size */
/* Value records (setup-time, optional, after liship_csr_plan_encode_row_patterns; never an error when the matrix does not
 * qualify): when the plan has 32 B pattern records and every row of a pattern carries the same values bit for bit -- a
 * constant-coefficient stencil -- the 7 values join the 7 offsets in the record and the products read neither the value nor
 * the index array: one byte per row (the idea of CSR-VI, value indexing, applied to whole rows).  Same products in the same
 * order: bit-identical.  The value array must not change afterwards (a new plan is needed if it does).
 * Rows of one offset pattern that carry different values (a Dirichlet row stored with the interior row's sparsity) split the pattern.
 * Patterns of 8..32 offsets (no 32 B records: the 9-point stencil in 2-D, the 19- and 27-point ones in 3-D) get WIDE records when
 * there are at most 48 of them after the same splitting (400 B per pattern).
 * liship_csr_plan_value_records: 1 if the plan has them, 2 for the wide form.  liship_spmv_csr_set_row_values(0): A/B switch
 * (stream the values). */
int  liship_csr_plan_encode_row_values(liship_csr_plan_t plan, const int *ptr, const double *value, void *stream);
int  liship_csr_plan_value_records(liship_csr_plan_t plan);
/* Dominant pattern (found with the value records, nothing to call): when ONE pattern carries at least half of the rows -- the interior
 * row of a stencil: 98.8 % of the rows at 512^3 -- the plan names it, and keeps for every other pattern which of ITS slots that pattern
 * has and the pattern's values there (a boundary row is the interior row minus the neighbours that do not exist: a subsequence).  The
 * products then take the dominant pattern's offsets and values as kernel ARGUMENTS and issue its x gathers together with the load of
 * the pattern bytes -- one round trip per wavefront, no records in LDS, no barrier; wavefronts that meet another pattern fetch its 64 B
 * slot record by scalar loads, rows whose pattern is no subsequence (ghost columns of a partitioned matrix) or whose speculative
 * addresses would leave x take their own records row by row.  Same products in the same order: bit-identical.
 * liship_csr_plan_dominant_pattern: 1 if the plan has one. */
int  liship_csr_plan_dominant_pattern(liship_csr_plan_t plan);
int  liship_spmv_csr_set_row_values(int on);
int  liship_spmv_csr_set_row_patterns(int on);
int  liship_spmv_csr_set_index_codes(int on);
/* Block-local columns (setup-time, optional, never an error when the matrix does not qualify): for matrices with long rows
 * (the plan's products kernel) whose row blocks address few distinct columns -- several unknowns per node, wide bands --
 * the plan keeps per row block the sorted list of its distinct columns and per non-zero a 2 B position in that list; the
 * kernel then gathers x once per distinct column into LDS and forms the products from LDS (10 B + 4 B x distinct/entries
 * per non-zero instead of 12, a fraction of the gathers).  Same terms in the same order: bit-identical.  The index array
 * must stay valid.  liship_csr_plan_localized: total length of the lists, 0 if the plan has none.
 * liship_spmv_csr_set_local_columns(0) makes every product ignore them (A/B measurements). */
int  liship_csr_plan_localize_columns(liship_csr_plan_t plan, const int *ptr, const int *index, void *stream);
long long liship_csr_plan_localized(liship_csr_plan_t plan);
int  liship_spmv_csr_set_local_columns(int on);
/* round 5: when every list is made of TRIPLES of consecutive columns (meshes with 3 unknowns per node) the plan also keeps the triples' first columns and the kernel
 * reads one 4 B run start per triple instead of three columns (a third of the list bytes).  liship_csr_plan_local_runs: 3 when the plan has them, else 0;
 * liship_spmv_csr_set_local_runs(0): A/B switch (the full lists), same bits */
int  liship_csr_plan_local_runs(liship_csr_plan_t plan);
int  liship_spmv_csr_set_local_runs(int on);
/* 0: the block-local kernel keeps one entry per lane and step (eight 2 B position loads) instead of pairs of neighbouring entries (four 4 B loads, 16 B LDS accesses): A/B, same bits */
int  liship_spmv_csr_set_local_pairs(int on);
/* 0: plans of short rows (mean < 22 entries, no column codes) never try block-local columns (the rule of rounds 2-5); default 1 (round 6): they are tried from a mean
 * of 4 entries per row on and kept under the long rows' rule -- unstructured meshes with one unknown per node: +6 .. +39 % over the lane-per-row kernel.  Same bits. */
int  liship_spmv_csr_set_local_short_rows(int on);
/* Reordering (round 5): when the lists of a plan with block-local columns are long -- more than one listed column per `min_items_per_listed` non-zeros (0: the
 * default, 4) -- or a long-row plan could not have lists at all (more than 2048 distinct columns per row block): the signs of a numbering without locality -- the plan
 * renumbers rows and columns by graph distances found on the device (breadth-first searches from 3-4 landmarks, Morton keys, a stable radix sort: csr_order.hpp; rounds 4-5: a Cuthill-McKee walk on the host), builds P A P^T in HBM (the same entries
 * in the same in-row order) with a plan of its own, and keeps it when that plan lists at most 3/4 of the columns.  Short rows (plans of the row-gather kernel, no lists):
 * the 128 B lines of x a row block touches are counted instead -- more than one per 4 entries starts the walk, at most half of them afterwards keeps its result.
 * WHO USES IT: liship_csr_plan_reordered_form hands P A P^T out as a matrix of its own, for callers that keep whole iterations in the new numbering (lis_solve).
 * Products through the original plan keep the caller's numbering by default: a single product would have to gather x into the numbering and scatter y out of it, one
 * random access per node each, which costs what the better kernel gains (Queen class) or several times the product (scalar unknowns, short rows).
 * liship_spmv_csr_set_reorder(2) lets whole-matrix products of LONG-row plans take it all the same (row r stored where the original row lives: every y[i] is the
 * reference's sum, lis_matvec_csr.c:97-109, term by term -- the same bits; row-range products and the fused reductions keep the original numbering, and
 * liship_csr_plan_fused_dots returns 0); 1 is the default, 0 switches the reordered form off altogether (A/B).  The values are copied: a matrix whose value[] changes
 * needs a new plan, as with value records.  Never an error when the matrix does not qualify (fewer than 65 536 rows, coded indices, short lists, columns outside
 * [0, n)); 2 = out of memory, the plan unchanged.  liship_csr_plan_reordered: listed columns (lines of x for short rows) of the reordered form, 0: none. */
int  liship_csr_plan_reorder(liship_csr_plan_t plan, const int *ptr, const int *index, const double *value, int min_items_per_listed, void *stream);
/* the same with a permutation to try first (HOST, n entries: new position -> row), e.g. the one a plan of the same sparsity pattern found: a matrix whose values were
 * edited needs a new plan but not a new walk.  A hint that is not a permutation, or does not shorten the lists enough, is dropped for a walk.
 * liship_csr_plan_reorder_permutation: the permutation of the reordered form to the host (LISHIP_ERR_ARG when the plan has none). */
int  liship_csr_plan_reorder_with(liship_csr_plan_t plan, const int *ptr, const int *index, const double *value, int min_items_per_listed, const int *perm_hint, void *stream);
int  liship_csr_plan_reorder_permutation(liship_csr_plan_t plan, int *perm_host);
/* The numbering alone, for tests and tools: what liship_csr_plan_reorder would find for the device arrays ptr / index (n rows; columns [n, ncols) are ghost columns,
 * ncols <= n: none) with `landmarks` landmarks (clamped to 3..6), WITHOUT its size gate and its keep rule -- no plan, no P A P^T.  order_host[new position] = row
 * (HOST, n entries); *inner_rows_host = rows that have a component and read no ghost column (n - loose rows when there are no ghost columns).  *found = 0 and 0 returned: the
 * ordering declined (the graph is too deep for its level budget) and the outputs are not to be read; a HIP code: a runtime error; LISHIP_ERR_ARG: a null pointer
 * with n > 0 (or found itself); n = 0 is fine.  The numbering is a function of its inputs alone (distances, ties to the smallest index, a stable sort):
 * tests/order_model.py predicts it index by index. */
int  liship_csr_order(int n, int ncols, const int *ptr, const int *index, int landmarks, int *order_host, int *inner_rows_host, int *found, void *stream);
/* A rank's local matrix of a multi-rank job (columns [n, ncols) are ghost columns, lis_matrix_mpi.c:274-306): said before liship_csr_plan_reorder, the numbering is found on
 * the owned columns alone, ghost columns keep their numbers in P A P^T and the rows that read one are placed behind all the others --
 * rows [0, liship_csr_plan_reordered_inner_rows) of the reordered form touch no ghost column (they can run while the halo travels). */
int  liship_csr_plan_set_ghost_columns(liship_csr_plan_t plan, int ncols);
int  liship_csr_plan_reordered_inner_rows(liship_csr_plan_t plan);
/* 1: the plan wanted block-local column lists and has none (lists too long / trial failed): a numbering without any locality */
int  liship_csr_plan_lists_failed(liship_csr_plan_t plan);
/* out[k] = the position of row index[k] under the permutation perm (perm[new position] = row; n entries): a list of rows -- a halo export list -- in the new numbering */
int  liship_permute_rows_of_list(int n, const int *perm, int count, const int *index, int *out, void *stream);
long long liship_csr_plan_reordered(liship_csr_plan_t plan);
int  liship_spmv_csr_set_reorder(int mode);
/* the reordered form as a matrix of its own -- P A P^T: its plan (owned by `plan`), arrays and the permutation perm[new position] = original row -- for callers that keep
 * whole iterations in the new numbering (lis_solve gathers b and x0 once and scatters x back at the end: no per-product passes); LISHIP_ERR_ARG when the plan has none
 * (or it is switched off).  liship_permute_gather_f64: xp[i] = x[perm[i]]; liship_permute_scatter_f64: x[perm[i]] = xp[i] (x and xp distinct). */
int  liship_csr_plan_reordered_form(liship_csr_plan_t plan, liship_csr_plan_t *inner, const int **ptr, const int **index, const double **value, const int **perm);
int  liship_permute_gather_f64(int n, const int *perm, const double *x, double *xp, void *stream);
int  liship_permute_scatter_f64(int n, const int *perm, const double *xp, double *x, void *stream);
/* round 4: the block-local kernel keeps the 2 B positions in registers and stages 3584 items (lists <= 1024 columns) or 3072 items (longer lists) per
 * workgroup -- 39.5 KB of LDS, four workgroups per CU.  0: plans built from now on take the round-3 form (4096-item blocks, positions through LDS: three /
 * two workgroups per CU); A/B measurements, same bits either way */
int  liship_spmv_csr_set_local_register_positions(int on);
/* structured grids, values streamed (spmv_csr_pattern7_kernel): every XCD takes one eighth of every plane of the grid and walks the planes in order, so that the
 * +-plane neighbours of its rows stay in its own L2 (round 4).  0: the natural block order (A/B measurements); same bits either way */
/* the same strips for the kernels that stream index[] (spmv_csr_rowgather_kernel: the reference's 12 B per non-zero; spmv_csr_coded_kernel): a plan
 * without row patterns learns its plane from the band of the matrix -- the largest |column - row|, when at least half of the rows reach it (two passes over
 * index[] at plan time; optional, never an error when the matrix does not qualify).  liship_csr_plan_strip_rows: rows per plane, 0 = natural order */
int  liship_csr_plan_scan_band(liship_csr_plan_t plan, const int *ptr, const int *index, void *stream);
int  liship_csr_plan_strip_rows(liship_csr_plan_t plan);
int  liship_spmv_csr_set_xcd_strips(int on);
/* On by default (round 6), NOT bit-identical to the reference for the rows it touches: the part of a row beyond the LDS stage (~2100 entries) is added
 * by a workgroup-wide tree per pass instead of one left-to-right chain (a 200 000-entry row is otherwise a 200 000-long
 * dependent add chain).  Deterministic, within 1e-14 of the row's magnitude; rows that fit the stage keep the reference's bits.
 * 0 = the chain: the reference's bits for every row (LIS_AMD_LONG_ROW_CHAIN=1; implied by the reference-order reductions mode). */
int  liship_spmv_csr_set_long_row_tree(int on);
int  liship_spmv_csr_set_row_block_dots(int on);  /* 1: fused dots of the dominant-pattern product as the row blocks' partial sums (the other forms' bits); LIS_AMD_ROW_BLOCK_DOTS=1 */
int  liship_spmv_csr_switches(void);            /* bit 0 team kernels on, bit 1 row-block dots, bit 2 long-row tree (tests of the LIS_AMD_* variables) */
int  liship_spmv_csr_set_uniform_rows(int on);    /* A/B: 0 keeps the row sums of uniform-length wavefronts on the skewed schedule (same bits) */
int  liship_csr_plan_destroy(liship_csr_plan_t plan);
int  liship_csr_plan_info(liship_csr_plan_t plan, int *n, long long *nnz, int *nblocks);
/* Rows that START with their first product instead of being added to 0.0: the reference's split products compute
 * t0 = D[i]*x[i]; t0 += (L row); t0 += (U row)  (lis_matvec_csr.c:64-89 and the is_splited branches of the other formats).
 * With the flag on, every product of this plan starts its row sums at -0.0, which reproduces that sequence bit for bit
 * (signed zeros included) on rows laid out as [D, L entries, U entries]. */
int  liship_csr_plan_set_first_term_initialises(liship_csr_plan_t plan, int on);
int  liship_spmv_csr_f64(liship_csr_plan_t plan, const int *ptr, const int *index,
                         const double *value, const double *x, double *y, void *stream);
/* the product with a fused reduction epilogue: result[0] = sum_r w[r]*y[r] (w may be x: CG's <p,Ap>,
 * lis_solver_cg.c:185-188), result[1] = sum_r y[r]^2 when want_sumsq (BiCGSTAB's <t,s>,<t,t>,
 * lis_solver_bicgstab.c:262-268).  y is bit-identical to liship_spmv_csr_f64; saves a 16 B/row pass.
 * Returns LISHIP_ERR_ARG when it cannot serve the call (then use the plain product + liship_dot_f64). */
int  liship_spmv_csr_dot_f64(liship_csr_plan_t plan, const int *ptr, const int *index, const double *value,
                             const double *x, double *y, const double *w, int want_sumsq,
                             double *result, void *work, void *stream);
/* same product restricted to rows [row_begin,row_end) (used to overlap the halo exchange) */
int  liship_spmv_csr_rows_f64(liship_csr_plan_t plan, int row_begin, int row_end, const int *ptr,
                              const int *index, const double *value, const double *x, double *y,
                              void *stream);
/* The fused-reduction product of liship_spmv_csr_dot_f64 in parts: rows [row_begin,row_end) now, their per-row-block
 * partial sums parked in `work` from slot_base on (*slots_used of them); after the last part
 * liship_spmv_csr_dot_finish_f64 folds all parked partials into result[0..1].  A multi-rank job uses it to run the rows
 * that reference no ghost column while the halo travels (LIS_MATVEC_SENDRECV, include/lis_matvec.h:31-44, serialises
 * the two in the reference). */
int  liship_spmv_csr_rows_dot_f64(liship_csr_plan_t plan, int row_begin, int row_end, const int *ptr, const int *index,
                                  const double *value, const double *x, double *y, const double *w, int want_sumsq,
                                  void *work, int slot_base, int *slots_used, void *stream);
int  liship_spmv_csr_dot_finish_f64(int slots_used, int want_sumsq, double *result, void *work, void *stream);
/* tuning knobs for experiments (bench/profiling only): variant 0 = default */
int  liship_spmv_csr_set_variant(int variant);

/* ELL / DIA products with the reduction epilogue of liship_spmv_csr_dot_f64 (same contract and fallback rule) */
int  liship_spmv_ell_dot_f64(int n, int maxnzr, const int *index, const double *value, const double *x, double *y,
                             const double *w, int want_sumsq, double *result, void *work, void *stream);
/* ELL index coding (as liship_csr_plan_encode_indices): *codes / *dict are allocated on the device when the n*maxnzr
 * slots (padding included) sit on <= 255 diagonals and n is even, else stay NULL; free them with liship_free.
 * liship_spmv_ell_coded_f64: the ELL product from value + codes (9 B per slot), want_sumsq < 0 for the plain product,
 * 0 / 1 for the reduction epilogue of liship_spmv_ell_dot_f64; bit-identical to the 4 B-index kernels. */
int  liship_ell_encode_indices(int n, int maxnzr, const int *index, unsigned char **codes, int **dict, int *ndict, void *stream);
int  liship_spmv_ell_coded_f64(int n, int maxnzr, const unsigned char *codes, const int *dict, const double *value,
                               const double *x, double *y, const double *w, int want_sumsq, double *result,
                               void *work, void *stream);
int  liship_spmv_dia_dot_f64(int n, int ncols, int nnd, const int *offsets, const double *value, const double *x, double *y,
                             const double *w, int want_sumsq, double *result, void *work, void *stream);
/* ------------------------------------------------------------------ other formats
 * ELL   lis_matvec_ell  src/matvec/lis_matvec_ell.c:113-128   value/index column-major [maxnzr][n]
 * DIA   lis_matvec_dia  src/matvec/lis_matvec_dia.c:148-172   ONE-chunk layout value[d*n+i], offsets index[nnd]
 * JAD   lis_matvec_jad  src/matvec/lis_matvec_jad.c:170-196   ONE-chunk layout, y[perm[i]] = w[i]
 * BSR   lis_matvec_bsr* src/matvec/lis_matvec_bsr.c:57-858    column-major bnr x bnc blocks; like the
 *       reference it writes all nr*bnr rows, so y needs nr*bnr entries and x nc*bnc (the `pad`)
 * DIA   ncols = number of readable x entries (n, or np with ghost columns: lis_matvec_dia.c:158-162)
 * (CSC  lis_matvec_csc  src/matvec/lis_matvec_csc.c:128-144 is served by the CSR kernel on the
 *  column-ordered transpose the host layer builds at upload) */
int  liship_spmv_ell_f64(int n, int maxnzr, const int *index, const double *value,
                         const double *x, double *y, void *stream);
int  liship_spmv_dia_f64(int n, int ncols, int nnd, const int *offsets, const double *value,
                         const double *x, double *y, void *stream);
/* rows [row_begin, row_end) of the ELL / DIA product only (layouts of all n rows; codes / dict may be NULL): the parts a multi-rank
 * job launches around its halo exchange -- same bits as the whole launch */
int  liship_spmv_ell_rows_f64(int n, int maxnzr, const int *index, const unsigned char *codes, const int *dict, const double *value,
                              const double *x, double *y, int row_begin, int row_end, void *stream);
int  liship_spmv_dia_rows_f64(int n, int ncols, int nnd, const int *offsets, const double *value,
                              const double *x, double *y, int row_begin, int row_end, void *stream);
int  liship_spmv_jad_f64(int n, int maxnzr, const int *perm, const int *ptr, const int *index,
                         const double *value, const double *x, double *y, void *stream);
int  liship_spmv_bsr_f64(int nr, int bnr, int bnc, const int *bptr, const int *bindex,
                         const double *value, const double *x, double *y, void *stream);
/* the same with the number of stored blocks given (bnnz < 0: unknown), which lets the library choose between a lane
 * per block row (short block rows) and a lane per block (long ones) */
int  liship_spmv_bsr_nnz_f64(int nr, int bnnz, int bnr, int bnc, const int *bptr, const int *bindex,
                             const double *value, const double *x, double *y, void *stream);
/* which kernel liship_spmv_bsr_nnz_f64 launches for these arguments (no launch; LISHIP_ERR_ARG for nr < 0 or a block size below 1).  The choice rests on the
 * block size, bnnz / nr, liship_spmv_bsr_set_team and on whether bindex, value, x and y are 16 B aligned; every kind writes the same bits. */
#define LISHIP_BSR_GENERIC 0   /* any bnr x bnc: one lane per scalar row */
#define LISHIP_BSR_TILE    1   /* square 1..4: two phases, products through LDS */
#define LISHIP_BSR_PAIR22  2   /* 2x2: the same with a lane per block */
#define LISHIP_BSR_ROWS    3   /* square 2..4, short block rows: a lane per block row */
#define LISHIP_BSR_TEAM    4   /* square 2..4, long block rows: eight lanes per block row */
int  liship_spmv_bsr_kind(int nr, int bnnz, int bnr, int bnc, const int *bindex, const double *value, const double *x, const double *y);
/* the kind of the kernel the last liship_spmv_bsr_f64 / _nnz_f64 / _rows_f64 call of this process launched (-1: none yet; a call that launches nothing --
 * nr = 0, an empty range, a refusal -- leaves it; liship_spmv_bsr_dot_f64 does not go through the choice and leaves it too) */
int  liship_spmv_bsr_last_kind(void);
/* block rows [brb, bre) only (the array layout is that of all nr block rows): the parts of a multi-rank product around its halo exchange -- same bits, and
 * the kernel liship_spmv_bsr_kind names for the whole matrix's nr and bnnz with y + brb * bnr */
int  liship_spmv_bsr_rows_f64(int nr, int bnnz, int bnr, int bnc, const int *bptr, const int *bindex, const double *value,
                              const double *x, double *y, int brb, int bre, void *stream);
/* A/B switch: 0 keeps square blocks with long block rows (mean > 12 / 16 / 12 stored blocks per block row at 2x2 / 3x3 / 4x4) on the two-phase tile
 * kernels instead of the team-per-block-row kernel (spmv_bsr_team_kernel); same bits either way. */
int  liship_spmv_bsr_set_team(int on);
/* BSR product with the reduction epilogue (the contract of liship_spmv_csr_dot_f64): square blocks 2..4 and short block
 * rows; n = number of scalar rows (rows of the last block row beyond it are padding and stay out of the sums) */
int  liship_spmv_bsr_dot_f64(int nr, int n, int bnnz, int bs, const int *bptr, const int *bindex, const double *value,
                             const double *x, double *y, const double *w, int want_sumsq, double *result,
                             void *work, void *stream);

/* ------------------------------------------------------------------ vector kernels
 * element-wise: src/vector/lis_vector_opv.c (axpy :174, xpay :214, axpyz :253, scale :285, pmul :325,
 * pdiv :365, set_all :397, abs :428, reciprocal :458, shift :520); copy is a device memcpy. */
int  liship_axpy_f64 (int n, double alpha, const double *x, double *y, void *stream);       /* y += a*x    */
int  liship_xpay_f64 (int n, const double *x, double alpha, double *y, void *stream);       /* y = x + a*y */
int  liship_axpyz_f64(int n, double alpha, const double *x, const double *y, double *z, void *stream);
int  liship_scale_f64(int n, double alpha, double *x, void *stream);
int  liship_scale_to_f64(int n, double alpha, const double *x, double *y, void *stream);    /* y = a*x (lis_solver_gmres.c:290-296) */
int  liship_pmul_f64 (int n, const double *x, const double *y, double *z, void *stream);
int  liship_pdiv_f64 (int n, const double *x, const double *y, double *z, void *stream);
int  liship_set_all_f64(int n, double alpha, double *x, void *stream);
int  liship_abs_f64  (int n, double *x, void *stream);
int  liship_reciprocal_f64(int n, double *x, void *stream);
int  liship_shift_f64(int n, double sigma, double *x, void *stream);
int  liship_rsqrt_abs_f64(int n, double *x, void *stream);                                   /* x = 1/sqrt(|x|)   (lis_matrix_ops.c:611-614) */
/* rows of a CSR matrix scaled in HBM: value *= d[row] (symm 0, lis_matrix_csr.c:609-647) or value = value*d[row]*d[col] (symm 1, :651-690) */
int  liship_csr_scale_f64(int n, const int *ptr, const int *index, double *value, const double *d, int symm, void *stream);
/* fused forms: the SAME per-element expressions in the SAME order as the calls they replace (bit-identical),
 * one pass over HBM instead of two or three */
int  liship_axpy2_f64(int n, double a, const double *x, double b, const double *w, double *y, void *stream);       /* y += a*x; y += b*w   (lis_solver_bicgstab.c:272-273) */
int  liship_axpy_xpay_f64(int n, double a, const double *x, const double *w, double b, double *y, void *stream);   /* y += a*x; y = w + b*y (lis_solver_bicgstab.c:212-213) */
/* reductions: src/vector/lis_vector_ops.c dot :58-127, nrm2 :210-271, nrm1 :278-342, sum :418-478.
 * `result` is a DEVICE pointer to as many doubles as the entry point has sums (one, or two where its comment names two; nothing
 * behind them is written), `work` a device scratch of liship_reduce_work_bytes() whose contents on entry do not matter.
 * The ORDER of every sum is fixed and part of the contract (the Krylov iteration counts hang on its bits); it depends on n and on
 * the alignment of the arrays only.  tests/reduction_model.py restates it, tests/test_reduction_tree_gpu.py holds every entry
 * point to that:
 *   level 1   workgroups of 256 lanes, 2048 elements each, grid = max(1, ceil(((n + 1) / 2) / 1024)); every lane starts from 0.0.
 *             Every array (inputs and in-place outputs) 16 B aligned: lane t of block b takes the pairs p = 1024 b + t + 256 u,
 *             u = 0..3, p < n / 2, and adds the term of element 2p, then of 2p + 1; lane 0 of block 0 adds the last element of an
 *             odd n after its own pairs.  Any array only 8 B aligned: lane t of block b adds the elements 2048 b + t + 256 u, u = 0..7.
 *   wavefront six butterfly steps, v += v[lane ^ k] for k = 32, 16, 8, 4, 2, 1, read from lane 0
 *   workgroup the wavefronts' sums added in wavefront order, from 0.0
 *   folds     over the workgroups' partials: one partial is copied; up to 2^14 are summed by one workgroup of 1024 lanes (lane t
 *             adds partial[t], partial[t + 1024], ..., then the wavefront and workgroup steps above over 16 wavefronts); more are
 *             first summed in blocks of 2048 laid out as the 8 B aligned level 1, then folded again
 *   root      nrm2 takes sqrt once, of the final sum
 * A second sum accumulates separately, in the same order.  The fused forms add the terms their comments give, each product and
 * each sum rounded once (no FMA); -alpha and -*hprev are negations. */
size_t liship_reduce_work_bytes(void);
/* T > 0: the reductions below (and the fused update passes) add their terms in the reference's order for OMP_NUM_THREADS = T -- chunk t of T is
 * LIS_GET_ISIE(t, T, n) (include/lis.h:1067-1078), summed left to right from 0.0 by one lane, the T partials added serially in chunk order
 * (src/vector/lis_vector_ops.c:88-107) -- instead of the fixed tree; the products' fused-dot entry points then return LISHIP_ERR_ARG.  0: trees. */
int  liship_set_reference_reductions(int T);
int  liship_get_reference_reductions(void);
int  liship_dot_f64 (int n, const double *x, const double *y, double *result, void *work, void *stream);
int  liship_nrm2_f64(int n, const double *x, double *result, void *work, void *stream);
int  liship_sumsq_f64(int n, const double *x, double *result, void *work, void *stream);
int  liship_nrm1_f64(int n, const double *x, double *result, void *work, void *stream);
int  liship_sum_f64 (int n, const double *x, double *result, void *work, void *stream);
/* x += alpha*p; r += (-alpha)*q; result[0] = sum r^2   (lis_solver_cg.c:199-205: two axpys + the residual norm) */
int  liship_cg_update_f64(int n, double alpha, const double *p, const double *q, double *x, double *r,
                          double *result, void *work, void *stream);
/* the same with the Jacobi solve of the next iteration folded in: z = r.*dinv is formed per element (not
 * stored) and result = {sum r^2, sum r*z}   (lis_solver_cg.c:199-205 + :176-180 of the next iteration) */
int  liship_cg_update_jacobi_f64(int n, double alpha, const double *p, const double *q, const double *dinv,
                                 double *x, double *r, double *result, void *work, void *stream);
/* z = x.*d ; y = z + a*y   (Jacobi solve lis_precon_jacobi.c:121-124 + lis_vector_xpay, lis_solver_cg.c:183) */
int  liship_pmul_xpay_f64(int n, const double *x, const double *d, double a, double *y, void *stream);
/* y += a*x; result[0] = sum y^2            (lis_solver_bicgstab.c:233-236) */
int  liship_axpy_sumsq_f64(int n, double a, const double *x, double *y, double *result, void *work, void *stream);
/* y += a*x; result = {sum y^2, sum v*y}    (lis_solver_bicgstab.c:276-279 + :190 of the next iteration) */
int  liship_axpy_sumsq_dot_f64(int n, double a, const double *x, double *y, const double *v, double *result,
                               void *work, void *stream);
/* one modified Gram-Schmidt step of GMRES (lis_solver_gmres.c:219-227) with the coefficient read from HBM:
 * w += (-*hprev)*vprev, then result[0] = <w,vnext>, or sum w^2 when vnext is NULL.  hprev is a previous
 * result[], so a Hessenberg column needs no host synchronisation between its steps. */
int  liship_mgs_step_f64(int n, const double *hprev, const double *vprev, double *w, const double *vnext,
                         double *result, void *work, void *stream);
/* K inner products result[k] = <vecs[pairs[k][0]], vecs[pairs[k][1]]> over nvec <= LISHIP_MULTIDOT_MAX_VECS vectors of n elements in ONE pass: a
 * workgroup reads its tile of every vector once (kernels/eigen.hip).  vecs and pairs are HOST arrays (of device pointers / of indices into vecs); a pair may
 * name one vector twice, and two results may name the same pair.  Every sum is formed EXACTLY as liship_dot_f64 forms that pair alone -- the tree above, the
 * 16 B or the 8 B lane mapping chosen from that pair's own two arrays, or the T chunks of liship_set_reference_reductions(T) -- so a loop may take its
 * Gram block here or as K separate dots and find the same bits (the eigensolvers' CG and CR, host/lis_esolver_single.c; tests/test_multidot_gpu.py).  When some vector
 * is only 8 B aligned, the tiles are swept a second time for the pairs that involve one (the second sweep reads from cache).  In the reference-order mode
 * the K sums are K passes (one lane adds a chunk there: nothing to share).  Announce no liship_krylov_chain step before this call: the one pass
 * leaves it pending, where liship_dot_f64 would run it. */
#define LISHIP_MULTIDOT_MAX_VECS 8
#define LISHIP_MULTIDOT_MAX_PAIRS 36
int  liship_multidot_f64(int n, int nvec, const double *const *vecs, int K, const int (*pairs)[2], double *result, void *work, void *stream);
/* The tail of one subspace iteration (-e si, lis_esolver_si.c:301-311) in ONE pass over r and v.  sums (HBM) = {sum r^2, theta = <v,r>}, as one
 * liship_multidot_f64 pass over {r, v} with the pairs (r, r), (v, r) leaves them.  Per element, in this order, each product and each sum rounded once:
 *   q = (-theta) * v[i] + r[i]  (lis_vector_axpyz; q is not stored), q * q enters the reduction;
 *   s = (1.0 / sqrt(sums[0])) * r[i]  (lis_vector_scale; the reciprocal formed once per lane from the HBM value, as liship_scale_inv_norm_f64);  r[i] = s; v[i] = s.
 * result[0] = sum q^2, formed EXACTLY as liship_sumsq_f64 forms it on a 16 B aligned array of n elements: the tree above on the same grid, or the T chunks
 * of liship_set_reference_reductions(T).  So the six calls nrm2, dot, axpyz, nrm2, scale, copy and {multidot, this} give the same bits (11 against 6
 * n-vector streams).  r and v must be 16 B aligned and must not overlap (one array given twice included): LISHIP_ERR_ARG otherwise and for n <= 0, with
 * nothing launched.  sums and result must not overlap either.  It is one more op of the reductions above (kernels/vector_ops.hip), so a pending
 * liship_krylov_chain step runs behind it wherever liship_sumsq_f64 runs it: in the fold, after a single workgroup, in the reference-order mode. */
int  liship_ritz_tail_f64(int n, const double *sums, double *r, double *v, double *result, void *work, void *stream);
/* value[k] -= sigma for the FIRST stored entry k of each row whose column is the row; a row without one is left alone (lis_matrix_shift_diagonal_csr,
 * src/matrix/lis_matrix_csr.c:566-603, on arrays in HBM; a split matrix's chain rows start with their diagonal term, host/lis_split.c) */
int  liship_csr_shift_diagonal_f64(int n, const int *ptr, const int *index, double *value, double sigma, void *stream);
/* A <- A - sigma B on two CSR matrices of n rows in HBM (lis_matrix_shift_matrix, kernels/spgeam.hip): every row of the result holds the union of the two rows'
 * columns in ascending order, every entry is (-sigma) * b + a with an absent term counting as 0.0 -- the product and the sum rounded once each --, and an entry
 * that comes out exactly 0.0 is dropped (what the reference's dense route leaves, src/matrix/lis_matrix_ops.c:833-856).  Columns are unique within a row, in
 * any order.  One lane per row, LISHIP_SHIFT_MATRIX_ROWS rows per workgroup.
 *   _try   ONE launch.  A row whose result keeps A's layout (A's columns ascending, every surviving entry of B on a column A stores, no result 0.0) is updated in
 *          avalue[] where it lies: done[r] = 1, count[r] = its length.  Any other row is left untouched: done[r] = 0, count[r] = the length of its result,
 *          *flag += 1 (*flag is zeroed first, on the stream).  *flag == 0 afterwards: A holds A - sigma B.  count, done: n device ints, flag: one.
 *   _scan  nptr[0 .. n] = the exclusive scan of count[], *nnz (host) = nptr[n]; scratch: (n / 4096 + 2) long long in HBM.  Waits for the stream.
 *   _fill  nindex / nvalue (nptr[n] entries each): row r from nptr[r] -- a done row copied from A, any other row merged from A's untouched row and B's. */
#define LISHIP_SHIFT_MATRIX_ROWS 256
int  liship_csr_shift_matrix_try_f64(int n, const int *aptr, const int *aindex, double *avalue, const int *bptr, const int *bindex, const double *bvalue,
                                     double sigma, int *count, int *done, int *flag, void *stream);
int  liship_csr_shift_matrix_scan(int n, const int *count, int *nptr, long long *scratch, int *nnz, void *stream);
int  liship_csr_shift_matrix_fill_f64(int n, const int *aptr, const int *aindex, const double *avalue, const int *bptr, const int *bindex, const double *bvalue,
                                      double sigma, const int *done, const int *nptr, int *nindex, double *nvalue, void *stream);
/* x *= 1/sqrt(*sumsq) with sumsq in HBM  (lis_vector_nrm2 + lis_vector_scale, lis_solver_gmres.c:229-232) */
int  liship_scale_inv_norm_f64(int n, const double *sumsq, double *x, void *stream);
/* The pair passes: two vectors scaled by one factor in ONE walk (vector_pass<NT, VEC, 2, 2>, kernels/vector_pass.hpp: the 16 B walk when all four arrays are
 * 16 B aligned, else the 8 B walk; non-temporal loads beyond the Infinity Cache).  Each result is one rounded product, so both give the bits of the separate calls.
 *   liship_scale2_inv_sqrt_f64: a = 1.0 / sqrt(*s), formed once per lane from the HBM value as liship_scale_inv_norm_f64 forms it (no fabs: *s < 0 gives NaN
 *     everywhere); v[i] = a * v[i]; w[i] = a * w[i].  Behind liship_dot_f64(..., s) it is `eta = sqrt(<v,w>); scale(1/eta, v); scale(1/eta, w)` of the generalized
 *     subspace iteration (lis_esolver_si.c:604-607) in one launch and with no host wait.
 *   liship_scale2_to_f64: out0[i] = alpha * in0[i]; out1[i] = alpha * in1[i] -- `copy r -> w; copy q -> v; scale w; scale v` of the generalized Lanczos
 *     iteration (lis_esolver_li.c:546-549): one launch and 4 n-vector streams for four launches and 8.
 * The two outputs must not overlap, and an output may meet an input only as its own input, whole (out0 == in0, out1 == in1).  Any other overlap, v == w, s inside
 * v or w, a NULL array or n <= 0: LISHIP_ERR_ARG with nothing launched. */
int  liship_scale2_inv_sqrt_f64(int n, const double *s, double *v, double *w, void *stream);
int  liship_scale2_to_f64(int n, double alpha, const double *in0, const double *in1, double *out0, double *out1, void *stream);

/* ------------------------------------------------------------------ device-driven Krylov loops
 * The scalars of CG / BiCGSTAB (rho, alpha, beta, omega, the residual norm, the iteration count and the
 * convergence flag) can live in HBM: a block of LISHIP_KS_LEN doubles the host fills once.  The `_dev` forms of
 * the vector kernels read their coefficient(s) from that block at kernel start, reductions leave their sums in
 * it, and liship_krylov_step() -- one lane -- applies the reference's scalar statements between them
 * (lis_solver_cg.c:176-215, lis_solver_bicgstab.c:186-290, lis_solver_bicg.c:176-262) with the same IEEE operations the host loop would
 * use.  While a guard flag is installed (liship_krylov_guard), every vector / reduction / fused-product kernel
 * launched returns immediately if *flag != 0, so the host may enqueue a batch of iterations, read the block
 * back once, and find x, r and the iteration count exactly as the one-synchronisation-per-scalar loop leaves
 * them.  Lowered means 0.0 or -0.0; anything else, NaN included, is raised.
 * Behind a raised flag no kernel writes a vector element, and a scalar step whose state has DONE up re-arms
 * NOT_HALF and changes nothing else.  The RESULT slots of a guarded reduction, fused update pass or fused-dot
 * product are UNSPECIFIED then: the first-level kernel returns at once, but the folds that follow it when the
 * reduction takes more than one workgroup are not guarded and rewrite result[] from whatever partials the work
 * buffer holds (one workgroup, and the reference-order mode, leave result[] alone).  A device loop never reads
 * those sums again once DONE is up.
 * The installed guard and the announced step are per-process and hold the raw pointers they were given: remove the guard
 * (NULL) and withdraw the step (0) before the memory they point at is freed. */
enum {
	LISHIP_KS_RHO = 0, LISHIP_KS_RHO_OLD, LISHIP_KS_ALPHA, LISHIP_KS_NALPHA, LISHIP_KS_BETA, LISHIP_KS_OMEGA,
	LISHIP_KS_NOMEGA, LISHIP_KS_DOT0, LISHIP_KS_DOT1, LISHIP_KS_SUM0, LISHIP_KS_SUM1, LISHIP_KS_NRM2,
	LISHIP_KS_BNRM,          /* factor of the convergence test: 1/||b|| or 1/||r0|| (lis_solver.c:1792-1812) */
	LISHIP_KS_TOL,
	LISHIP_KS_ITER,          /* iterations completed (a double holding an integer) */
	LISHIP_KS_DONE,          /* 0 while iterating; the guard flag */
	LISHIP_KS_STATUS,        /* 0 running, 1 converged, 2 breakdown */
	LISHIP_KS_NOT_HALF,      /* BiCGSTAB: 0 only between the half-step convergence and its x update (every step re-arms it) */
	LISHIP_KS_NHIST,         /* residual-history entries written (a breakdown ends an iteration without one) */
	LISHIP_KS_LEN = 32
};
enum {
	LISHIP_STEP_CG_ALPHA = 1,     /* after <p,q>:            breakdown test, alpha = rho / <p,q>                */
	LISHIP_STEP_CG_RESID,         /* after the update pass:  ||r||, history, convergence, rho <- <r,r>, beta    */
	LISHIP_STEP_CG_RESID_PRE,     /* same with rho <- <r,z> (second sum)                                        */
	LISHIP_STEP_BICGSTAB_ALPHA,   /* after <rtld,v>: rho == 0 breakdown test, alpha = rho / <rtld,v>            */
	LISHIP_STEP_BICGSTAB_HALF,    /* after ||s||: convergence at the half step (lowers NOT_HALF for the x update)*/
	LISHIP_STEP_BICGSTAB_OMEGA,   /* after <t,s>,<t,t>: omega = <t,s>/<t,t>                                     */
	LISHIP_STEP_BICGSTAB_RESID,   /* after the r update: ||r||, history, convergence, omega breakdown, rho', beta */
	LISHIP_STEP_BICG_ALPHA,       /* after <p~,q>: rho == 0 and <p~,q> == 0 breakdown tests, alpha              */
	LISHIP_STEP_BICG_RESID,       /* after the x,r update: ||r||, history, convergence                          */
	LISHIP_STEP_BICG_RHO          /* after the r~ update: rho <- <r~, M^-1 r>, beta                             */
};
/* install (flag != NULL) or remove (NULL) the guard for the launches that follow */
int  liship_krylov_guard(const double *flag);
/* one scalar step on `state`; rhistory (device, may be NULL) receives the residual norm of each completed
 * iteration at [iter].  In a multi-rank job `gathered` holds nranks x count per-rank sums (rank-major), which are
 * added in rank order, from 0.0, into the slots the step reads, before it runs; NULL otherwise (nranks is then ignored).
 * Slot and count per step: CG_ALPHA, BICGSTAB_ALPHA, BICG_ALPHA: DOT0, 1;  BICGSTAB_OMEGA: DOT0, 2;
 * CG_RESID, BICGSTAB_HALF, BICG_RESID: SUM0, 1;  CG_RESID_PRE, BICGSTAB_RESID, BICG_RHO: SUM0, 2.
 * A step outside CG_ALPHA .. BICG_RHO or a NULL state: LISHIP_ERR_ARG, nothing is launched. */
int  liship_krylov_step(int step, double *state, double *rhistory, const double *gathered, int nranks, void *stream);
/* single-rank jobs: announce the step BEFORE launching the reduction whose sums it reads; it then runs in that
 * reduction's last kernel instead of a launch of its own.  liship_krylov_chain_flush runs a step that was announced
 * but found no reduction to ride in (call it after the reduction; a no-op otherwise); step 0 withdraws an announced step. */
int  liship_krylov_chain(int step, double *state, double *rhistory);
/* out[k] = sum over ranks r (in rank order, from 0.0) of gathered[r*count + k]: the device half of the cross-rank
 * fold that MPI_Allreduce does in the reference (lis_vector_ops.c:119,263), count <= 64 */
int  liship_rank_fold_f64(int count, const double *gathered, int nranks, double *out, void *stream);
int  liship_krylov_chain_flush(void *stream);
/* y = x + (*pa)*y;  y = x.*d + (*pa)*y;  y += (*pa)*x;  y += (*pa)*x, then y += (*pb)*w;  y += (*pa)*x, then y = w + (*pb)*y */
int  liship_xpay_dev_f64(int n, const double *x, const double *pa, double *y, void *stream);
int  liship_pmul_xpay_dev_f64(int n, const double *x, const double *d, const double *pa, double *y, void *stream);
int  liship_axpy_dev_f64(int n, const double *pa, const double *x, double *y, void *stream);
int  liship_axpy2_dev_f64(int n, const double *pa, const double *x, const double *pb, const double *w, double *y, void *stream);
int  liship_axpy_xpay_dev_f64(int n, const double *pa, const double *x, const double *w, const double *pb, double *y, void *stream);
/* CG with the x update deferred into the NEXT iteration's direction update, which reads p anyway (lis_solver_cg.c:199, then
 * :176-183): x += (*palpha)*p on the old p, then p = r.*dinv + (*pbeta)*p (dinv NULL: p = r + (*pbeta)*p).  Each element sees
 * the reference's operations in the reference's order -- the bits of x and p are those of the undeferred loop -- while an
 * iteration moves 80 instead of 88 B of vectors per row.  palpha NULL: first iteration, x is not touched.  The caller owes
 * the last x += alpha*p after the loop (liship_axpy_dev_f64). */
int  liship_cg_direction_dev_f64(int n, const double *palpha, const double *pbeta, const double *r, const double *dinv,
                                 double *p, double *x, void *stream);
/* r += (*pna)*q (pna holds -alpha) ; result = {sum r^2, sum r*(r.*dinv)} : the residual half of liship_cg_update_jacobi_f64
 * (without a preconditioner liship_axpy_sumsq_dev_f64 serves) */
int  liship_cg_residual_jacobi_dev_f64(int n, const double *pna, const double *q, const double *dinv, double *r,
                                       double *result, void *work, void *stream);
/* The two passes for a Jacobi preconditioner with a UNIFORM diagonal: every dinv[i] is the double dc (the caller has made sure:
 * liship_count_ne_f64 returned 0), so r[i]*dc is r[i]*dinv[i] in every bit and the array is not read -- 64 instead of 80 B of
 * vectors per row and iteration. */
int  liship_cg_direction_uniform_dev_f64(int n, const double *palpha, const double *pbeta, const double *r, double dc,
                                         double *p, double *x, void *stream);
int  liship_cg_residual_jacobi_uniform_dev_f64(int n, const double *pna, const double *q, double dc, double *r,
                                               double *result, void *work, void *stream);
/* result[0] = how many x[i] differ from `a` in any bit (a reduction like the others: work as for liship_dot_f64) */
int  liship_count_ne_f64(int n, const double *x, double a, double *result, void *work, void *stream);
/* BiCGSTAB without a preconditioner (shat is s itself): x += (*palpha)*phat, x += (*pomega)*s, r = s + (*pnomega)*t, result =
 * {sum r^2, sum rtld*r} -- lis_solver_bicgstab.c:272-279 and :190 of the next iteration in ONE pass (s is read once for the
 * iterate and the residual: 56 instead of 64 B per row); s is the content of r[] on entry */
int  liship_bicgstab_end_dev_f64(int n, const double *palpha, const double *pomega, const double *pnomega, const double *phat,
                                 const double *t, const double *rtld, double *x, double *r, double *result, void *work, void *stream);
/* the fused update passes with the coefficient in HBM (dinv may be NULL for liship_cg_update_dev_f64) */
int  liship_cg_update_dev_f64(int n, const double *palpha, const double *p, const double *q, const double *dinv,
                              double *x, double *r, double *result, void *work, void *stream);
int  liship_axpy_sumsq_dev_f64(int n, const double *pa, const double *x, double *y, double *result, void *work, void *stream);
int  liship_axpy_sumsq_dot_dev_f64(int n, const double *pa, const double *x, double *y, const double *v, double *result,
                                   void *work, void *stream);
/* z = c0*v0, z += c1*v1, ... (accumulate = 0) or z += c0*v0, ... (accumulate = 1), element by element in that
 * order: the bits of lis_vector_scale/axpy chains (lis_solver_gmres.c:290-296, :323-329) in one pass over z.
 * vs[] and coef[] are HOST arrays (passed by value to the kernel); a v that aliases z reads z as it was on entry.
 * More than 48 vectors are processed in chunks: only the first chunk may then alias z. */
int  liship_lincomb_f64(int n, int count, const double *const *vs, const double *coef, int accumulate,
                        double *z, void *stream);
/* result[0] = <x,y>, result[1] = <x,x> in one pass (BiCGSTAB's <t,s>,<t,t>, lis_solver_bicgstab.c:267-268) */
int  liship_dot2_f64(int n, const double *x, const double *y, double *result, void *work, void *stream);

/* ------------------------------------------------------------------ matrix helpers on device */
/* d[i] = first value[j] with index[j]==i in row i, else 0: lis_matrix_get_diagonal_csr,
 * src/matrix/lis_matrix_csr.c:547-558 */
int  liship_csr_diagonal_f64(int n, const int *ptr, const int *index, const double *value,
                             double *d, void *stream);
/* XCD strips of the native ELL / DIA kernels (round 6): rows per plane of the structured grid the next whole-matrix ELL / DIA launches work on -- every XCD then takes
 * one eighth of every plane and walks the planes in order, so the +-plane neighbours of a row are in its own L2 (the CSR kernels learn their plane at plan time:
 * liship_csr_plan_strip_rows).  0: the natural workgroup order.  An order of the workgroups only: the bits cannot depend on it. */
int  liship_spmv_formats_set_plane(int rows);
/* workgroups per plane that a whole-matrix ELL / DIA launch of `grid` workgroups of `rows_per_wg` rows (512: 256 lanes of two rows) takes from the plane set now;
 * 0: that launch runs in natural order (plane not whole workgroups, fewer than 64 or not a multiple of 8 workgroups per plane, fewer than four planes) */
int  liship_spmv_formats_plane_blocks(int rows_per_wg, int grid);
/* the plane of a structured grid from ELL arrays in HBM: the largest |column - row| when at least half of the rows reach it (as liship_csr_plan_scan_band), else 0 */
int  liship_ell_scan_band(int n, int maxnzr, const int *index, int *plane_rows, void *stream);
/* the same for the native ELL arrays (first slot whose index is the row; padding gives 0: src/matrix/lis_matrix_ell.c lis_matrix_get_diagonal_ell) and the
 * native DIA arrays (the stored diagonal of offset 0, one chunk value[d*n + i]: src/matrix/lis_matrix_dia.c lis_matrix_get_diagonal_dia) */
int  liship_ell_diagonal_f64(int n, int maxnzr, const int *index, const double *value, double *d, void *stream);
int  liship_dia_diagonal_f64(int n, int nnd, const int *offsets, const double *value, double *d, void *stream);
/* halo pack: ws[i] = x[export_index[i]]  (lis_send_recv, src/matrix/lis_matrix_mpi.c:904-916) */
int  liship_gather_f64(int count, const int *export_index, const double *x, double *ws, void *stream);
/* A^T of a CSR matrix in HBM, each transposed row listing its entries in the order of their positions in the
 * source arrays -- the order lis_matvech_csr's scatter adds them (lis_matvec_csr.c:213-250).  tptr: ncols+1 ints,
 * tindex / tvalue: nnz entries, work: ncols + nnz ints.  Setup-time (once per matrix). */
/* y[0..rows) = A^T x from the transposed CSR below (rows = columns of A, nsrc = rows of A), summed as the OpenMP build of lis_matvech_csr sums with
 * T threads: per thread chunk LIS_GET_ISIE(k, T, nsrc) of SOURCE rows left to right from 0.0, chunk sums in chunk order (src/matvec/lis_matvec_csr.c:
 * 207-236).  The reference-order mode's A^T x for T > 1 (T = 1 is the plain row sum). */
int  liship_spmv_csr_transposed_chunked_f64(int rows, int nsrc, int T, const int *tptr, const int *tidx, const double *tval,
                                            const double *x, double *y, void *stream);
/* the same sums for transposed rows whose entries are NOT in ascending source row (the entry point above relies on that order): each thread chunk's terms in
 * stored order.  What lis_matvech_ell's T threads form (src/matvec/lis_matvec_ell.c:182-222: the scatter walks slot after slot); T sweeps over a row. */
int  liship_spmv_csr_transposed_chunked_unordered_f64(int rows, int nsrc, int T, const int *tptr, const int *tidx, const double *tval,
                                                      const double *x, double *y, void *stream);
/* ... and for chunks with explicit borders: chunk k owns the source rows borders[k] .. borders[k + 1] (T + 1 ascending ints in HBM, borders[0] = 0), the entries of a
 * transposed row never step back to an earlier chunk.  lis_matvech_vbr's T threads own chunks of BLOCK ROWS (src/matvec/lis_matvec_vbr.c:284-300):
 * borders[k] = row[first block row of LIS_GET_ISIE(k, T, nr)]. */
int  liship_spmv_csr_transposed_bordered_f64(int rows, int T, const int *borders, const int *tptr, const int *tidx, const double *tval,
                                             const double *x, double *y, void *stream);
int  liship_csr_transpose_f64(int nrows, int ncols, int nnz, const int *ptr, const int *index, const double *value,
                              int *tptr, int *tindex, double *tvalue, int *work, void *stream);
/* ---- the same method keyed by an arbitrary key (kernels/transpose.hip): a STABLE grouping of the entries 0 .. nnz-1.  Segment c of the result lists the entries
 * with key[k] == c in ascending k: tindex = src[k], tvalue = value[k]; tptr has nkeys + 1 ints.  key = row, src = col: the CSR rows of triplets in stored order
 * (lis_matvec_coo); key = col, src = row: their transposed operator (lis_matvech_coo).  Every key must lie in [0, nkeys).  Scratch is the routine's own; it
 * synchronizes the stream.  liship_key_facts: *flags_host bit 0 = key[] is not non-decreasing, bit 1 = a key outside [0, nkeys).  liship_sorted_key_starts:
 * ptr[r] = first k with key[k] >= r, for r = 0 .. nkeys, of a non-decreasing key[].  liship_group_by_key_borders: {32, 33, 2048}, the segment lengths at which the
 * ordering kernels change (insertion sort up to 32; 33 .. 2048 ranked by a wavefront in LDS when nnz > 8 nkeys; a heap sort beyond, and for those otherwise). */
int  liship_key_facts(int nkeys, int nnz, const int *key, int *flags_host, void *stream);
int  liship_sorted_key_starts(int nkeys, int nnz, const int *key, int *ptr, void *stream);
int  liship_group_by_key_f64(int nkeys, int nnz, const int *key, const int *src, const double *value, int *tptr, int *tindex, double *tvalue, void *stream);
int  liship_group_by_key_borders(int out[3]);
/* ---- COO (kernels/coo.hip): the CSR row form of nnz triplets, rows listing their entries in ascending k -- the sums of the reference's serial lis_matvec_coo.
 * ptr: n + 1 ints of the caller's.  row[] non-decreasing: ptr[] from the row starts and *index = col, *value = value THEMSELVES (no copy); otherwise fresh arrays
 * (liship_free), grouped by liship_group_by_key_f64.  LISHIP_ERR_ARG for a row outside [0, n).  Synchronizes the stream. */
int  liship_coo_rows_f64(int n, int nnz, const int *row, const int *col, const double *value, int *ptr, int **index, double **out_value, void *stream);
/* ---- DNS (kernels/dns.hip): value[j*n + i], n rows, np columns, every entry multiplied (zeros too).
 *   liship_spmv_dns_f64     y[i] = the chain over j = 0 .. np-1 from +0.0 of value[j*n+i] * x[j], every product rounded before it is added (lis_matvec_dns)
 *   liship_spmv_dns_t_f64   y[j] = the T sums over the row chunks LIS_GET_ISIE(k, T, n), each a chain from +0.0 of value[j*n+i] * x[i], added in chunk order
 *                           from +0.0 (lis_matvech_dns of the OpenMP build at T threads; T = 1: one chain)
 * Pure streams of 8 n np bytes; value, x and y need only the alignment of a double.  liship_dns_tile_info: {rows of y per workgroup, columns per slab} of the
 * forward kernel, {entries of y per workgroup, rows per slab} of the transposed one. */
int  liship_dns_tile_info(int info[4]);
int  liship_spmv_dns_f64(int n, int np, const double *value, const double *x, double *y, void *stream);
int  liship_spmv_dns_t_f64(int n, int np, int T, const double *value, const double *x, double *y, void *stream);
/* ---- VBR (kernels/vbr.hip): nr block rows row[0 .. nr], nc block columns col[0 .. nc], block row bi = the blocks bptr[bi] .. bptr[bi+1], block bc in block
 * column bindex[bc], its (row[bi+1]-row[bi]) x (col[bj+1]-col[bj]) values column-major from value[ptr[bc]].
 *   liship_vbr_check       *flags_host = 0, or the LISHIP_VBR_BAD_* bits of what is wrong: row[] / col[] not strictly ascending from 0 to n / np, bptr[] not
 *                          ascending from 0 to bnnz, ptr[] not ascending inside [0, nnz], a bindex outside [0, nc), a block whose ptr[bc+1] - ptr[bc] is not its
 *                          size.  Reads nothing beyond the arrays' lengths whatever they hold; synchronizes the stream.  Arrays that pass cannot send a
 *                          lane of the two kernels below out of bounds
 *   liship_vbr_block_rows  brow[i] = the block row of row i, n ints (of a checked row[])
 *   liship_spmv_vbr_f64    y[i] = the chain from +0.0 over the row's blocks in stored order, a block's columns ascending, of value * x[j], every product
 *                          rounded before it is added, zeros multiplied too (lis_matvec_vbr); a row without blocks gives +0.0; y by non-temporal stores
 * One lane per row.  liship_vbr_tile_info: {rows of y per workgroup, columns of a block whose values are loaded ahead of their adds}. */
#define LISHIP_VBR_BAD_ROW    1
#define LISHIP_VBR_BAD_COL    2
#define LISHIP_VBR_BAD_BPTR   4
#define LISHIP_VBR_BAD_PTR    8
#define LISHIP_VBR_BAD_BINDEX 16
#define LISHIP_VBR_BAD_SIZE   32
int  liship_vbr_tile_info(int info[2]);
int  liship_vbr_check(int n, int np, int nnz, int nr, int nc, int bnnz, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex,
                      int *flags_host, void *stream);
int  liship_vbr_block_rows(int n, int nr, const int *row, int *brow, void *stream);
int  liship_spmv_vbr_f64(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, const double *value,
                         const double *x, double *y, void *stream);
/* value[] of a checked copy edited where it lies, one launch each: A - sigma I on the entries the reference's diagonal search finds (lis_matrix_shift_diagonal_vbr: the
 * diagonal on uniform blocks, other entries or none on variable ones), and the scalings value*d[i] (symm = 0) and value*d[i]*d[j] in that order (symm = 1), d: n doubles */
int  liship_vbr_shift_diagonal_f64(int n, int nr, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, double *value, double sigma,
                                   void *stream);
int  liship_vbr_scale_f64(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, double *value, const double *d,
                          int symm, void *stream);
/* ---- preconditioners applied as products (kernels/sainv.hip): row sums over a packed CSR {ptr, idx, val}, each sum formed from +0.0 in STORED
 * order by one lane whatever the row's length, the epilogue in the same kernel.  The transposed forms (liship_csr_transpose_f64: terms by source
 * row) are summed in T chunks of the nsrc source rows, LIS_GET_ISIE(k, T, nsrc), the chunk sums added in chunk order from +0.0 (T <= 1: one chain).
 *   sainv_gather_scale  t[r] = (row r . b) * d[r]                      lis_matvech_ilu + the scale loop of lis_psolve_sainv (lis_precon_sainv.c:763-770)
 *   sainv_rows          x[c] = sum of row c of the transposed form . t    lis_matvec_ilu's scatter (lis_matrix_ilu.c:418-436)
 *   is_psolve           y[r] = x[r] - alpha * (row r . x)              lis_psolve_is (lis_precon_is.c:449-458); y must not be x
 *   is_psolveh          y[c] = x[c] - sum of row c of the transposed form . x, tval = alpha * u    lis_psolveh_is (:505-524); y must not be x
 *   is_truncate         the first min(keep, length) entries of every row of {uptr, uidx, uval} packed at the row starts tptr: tidx, tval, and taval = alpha * value */
int  liship_sainv_gather_scale_f64(int n, const int *ptr, const int *idx, const double *val, const double *d, const double *b, double *t, void *stream);
int  liship_sainv_rows_f64(int n, int nsrc, int T, const int *tptr, const int *tidx, const double *tval, const double *t, double *x, void *stream);
int  liship_is_psolve_f64(int n, const int *ptr, const int *idx, const double *val, double alpha, const double *x, double *y, void *stream);
int  liship_is_psolveh_f64(int n, int nsrc, int T, const int *tptr, const int *tidx, const double *tval, const double *x, double *y, void *stream);
int  liship_is_truncate_f64(int n, int keep, const int *uptr, const int *uidx, const double *uval, const int *tptr, double alpha,
                            int *tidx, double *tval, double *taval, void *stream);
/* ---- storage-format conversions of a CSR matrix that lives in HBM (kernels/convert.hip): the arrays the reference's host routines
 * build (src/matrix/lis_matrix_ell.c:958-1070, lis_matrix_dia.c:1191-1304, lis_matrix_bsr.c:351-552), bit for bit, from device arrays.
 * liship_csr_row_facts: facts[0] = longest row, facts[1] = 1 when some row is not in ascending column order (two device ints).
 * ELL: value 0 on the row's own column pads short rows.  DIA (rows in ascending column order): liship_csr_dia_offsets marks the
 * offsets that occur (used: n + ncols ints; slot: n + ncols + 1; scratch: (n + ncols) / 4096 + 4 long long) and returns their number,
 * liship_csr_to_dia writes them ascending and value[d * n + i].  BSR: distinct block columns of a block row in first-seen order, blocks
 * column-major; liship_csr_bsr_count gives bptr and the block count (-1: a block row with more than 96 distinct blocks; count: nr + 1
 * ints, scratch: nr / 4096 + 4 long long).  The *_rows forms build the CSR row form of an ELL / DIA matrix (lis_upload.c, lis_convert_hbm.c): the terms of
 * a row in the format's own order, padding and explicit zeros included. */
int  liship_csr_row_facts(int n, const int *ptr, const int *index, int *facts, void *stream);
int  liship_csr_to_ell(int n, int maxnzr, const int *ptr, const int *index, const double *value, int *ell_index, double *ell_value, void *stream);
/* the row form of a BSR matrix (as liship_csr_to_ell_rows for ELL): CSR rows that list lis_matvec_bsr's terms of each scalar row -- block after block, column after column,
 * explicit zeros included -- so that the CSR kernels form the same sums and the value records apply to constant-coefficient block matrices */
int  liship_bsr_to_rows(int n, int bnr, int bnc, const int *bptr, const int *bindex, const double *value, int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_csr_to_ell_rows(int n, int maxnzr, const int *ptr, const int *index, const double *value, int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_csr_dia_offsets(int n, int ncols, const int *ptr, const int *index, int *used, int *slot, long long *scratch, int *nnd, void *stream);
int  liship_csr_to_dia(int n, int ncols, int nnd, const int *ptr, const int *index, const double *value, const int *used, const int *slot,
                       int *offsets, double *dia_value, void *stream);
int  liship_dia_row_counts(int n, int ncols, int nnd, const int *offsets, int *count, int *rptr, long long *scratch, int *rnnz, void *stream);
int  liship_dia_to_rows(int n, int ncols, int nnd, const int *offsets, const double *dia_value, const int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_csr_bsr_count(int n, int np, int bnr, int bnc, const int *ptr, const int *index, int *count, int *bptr, long long *scratch, int *bnnz, void *stream);
int  liship_csr_to_bsr(int n, int bnr, int bnc, int bnnz, const int *ptr, const int *index, const double *value, const int *bptr,
                       int *bindex, double *bsr_value, void *stream);
/* JAD from the length-sorted row order perm[n] and the jagged-diagonal starts jptr[maxnzr + 1] (both made on the host: the order is the
 * reference's unstable quicksort, lis_convert.c): entry j of row perm[s] goes to [jptr[j] + s] */
int  liship_csr_to_jad(int n, const int *perm, const int *jptr, const int *ptr, const int *index, const double *value,
                       int *jad_index, double *jad_value, void *stream);
/* COO: row[k] = the row of entry k (col and value of the triplets are index and value as they stand: lis_matrix_coo.c:753-763).  DNS: dns[j*n + i], n * np doubles,
 * zero-filled here, then every entry in stored order, so that a duplicate (i, j) leaves its last value (lis_matrix_dns.c:784-797) */
int  liship_csr_to_coo(int n, const int *ptr, int *row, void *stream);
int  liship_csr_to_dns_f64(int n, int np, const int *ptr, const int *index, const double *value, double *dns, void *stream);
/* ---- the way back: CSR rows from an ELL, DIA, BSR, DNS or VBR matrix that lives in HBM (kernels/convert.hip), the arrays of lis_matrix_convert_<fmt>2csr bit for
 * bit.  A row lists its stored entries in the source's own order -- ELL: slots j = 0 .. maxnzr-1 of value[j*n+i]; DIA: diagonals d = 0 .. nnd-1 with
 * 0 <= i + offsets[d] < ncols; BSR: the block row's blocks in stored order, columns ascending inside a block, padding columns left out; DNS: j = 0 .. np-1 of
 * value[j*n+i]; VBR: blocks in stored order, columns ascending inside a block -- and leaves out every entry with value == 0.0 (the C comparison: +0.0 and -0.0 go,
 * NaN, infinities and subnormals stay).  Values are copied, never computed with; offsets into the source are 64-bit.
 *   liship_<fmt>_csr_count  count[i] = kept entries of row i (n ints), rptr[0 .. n] = their exclusive scan (rptr[n] = the total, in HBM), *nnz = the total on the
 *                           host; scratch: (n / 4096 + 2) long long.  LISHIP_ERR_OVERFLOW when the total does not fit an int (rptr is then not to be read).
 *                           Synchronizes the stream.
 *   liship_<fmt>_to_csr     rindex[] / rvalue[] (*nnz entries each) from that rptr; a lane writes inside [rptr[i], rptr[i+1]) only
 * DNS cuts every row into slabs of info[1] columns: count[] holds n * nslab ints (nslab = ceil(np / info[1])), offsets[] their scan (n * nslab + 1 ints, row i's
 * slabs one after another), scratch (n * nslab / 4096 + 2) long long; the fill entry reads offsets[].  VBR takes arrays that passed liship_vbr_check and the
 * brow[] of liship_vbr_block_rows.  liship_tocsr_tile_info: {rows per workgroup, columns per DNS slab, counts per scan tile} -- ONE entry for the five families:
 * they share the workgroup of 256 rows and the scan, and the slab is the only figure that belongs to one of them. */
#define LISHIP_ERR_OVERFLOW (-3)
int  liship_tocsr_tile_info(int info[3]);
int  liship_ell_csr_count(int n, int maxnzr, const double *value, int *count, int *rptr, long long *scratch, int *nnz, void *stream);
int  liship_ell_to_csr(int n, int maxnzr, const int *index, const double *value, const int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_dia_csr_count(int n, int ncols, int nnd, const int *offsets, const double *value, int *count, int *rptr, long long *scratch, int *nnz, void *stream);
int  liship_dia_to_csr(int n, int ncols, int nnd, const int *offsets, const double *value, const int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_bsr_csr_count(int n, int bnr, int bnc, const int *bptr, const int *bindex, const double *value, int *count, int *rptr, long long *scratch,
                          int *nnz, void *stream);
int  liship_bsr_to_csr(int n, int bnr, int bnc, const int *bptr, const int *bindex, const double *value, const int *rptr, int *rindex, double *rvalue, void *stream);
int  liship_dns_csr_count(int n, int np, const double *value, int *count, int *offsets, int *rptr, long long *scratch, int *nnz, void *stream);
int  liship_dns_to_csr(int n, int np, const double *value, const int *offsets, int *rindex, double *rvalue, void *stream);
int  liship_vbr_csr_count(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, const double *value,
                          int *count, int *rptr, long long *scratch, int *nnz, void *stream);
int  liship_vbr_to_csr(int n, const int *row, const int *col, const int *ptr, const int *bptr, const int *bindex, const int *brow, const double *value,
                       const int *rptr, int *rindex, double *rvalue, void *stream);
/* reverse halo: y[export_index[i]] += wr[i], indices unique within one call  (lis_reduce, lis_matrix_mpi.c:988-996) */
int  liship_scatter_add_f64(int count, const int *export_index, const double *wr, double *y, void *stream);

/* ------------------------------------------------------------------ synthetic inputs
 * Rows [is,ie) of the 3-D 7-pt Poisson matrix on an l x m x n grid, generated directly in HBM with the
 * entry order of test/test3.c:114-127 (sorted!=0: ascending column as test/spmvtest3.c:192-195).
 * Columns are LOCAL: owned column g -> g-is, ghost columns -> (ie-is) + rank in ascending global order,
 * exactly as lis_matrix_g2l_csr numbers them (src/matrix/lis_matrix_mpi.c:274-306).
 * ptr has ie-is+1 entries; index/value must hold liship_poisson3d_nnz() entries. */
long long liship_poisson3d_nnz(int l, int m, int n, int is, int ie);
int  liship_poisson3d_csr(int l, int m, int n, int is, int ie, int sorted,
                          int *ptr, int *index, double *value, void *stream);
/* b = A*1 for those rows without forming A (test/test3.c:150): 6 minus the number of neighbours */
int  liship_poisson3d_rhs(int l, int m, int n, int is, int ie, double *b, void *stream);

/* ------------------------------------------------------------------ level-scheduled triangular sweeps (kernels/sptrsv.hip on kernels/level_schedule.hpp, SSOR and ILU)
 * One sweep: nlev levels, the rows of level l are rows[lptr[l] .. lptr[l+1]) (short rows first, those of LISHIP_SWEEP_LONG_ROW or more
 * terms from llong[l] on), row r's terms col/val[rptr[r] .. rptr[r+1]) in the order they are added.  groups[3g .. 3g+2] = {l0, l1, run}:
 * run = 1: levels [l0, l1) in one single-workgroup launch (each at most LISHIP_SWEEP_SMALL_LEVEL rows), run = 0: level l0 on its own.
 * lptr .. val live in HBM; groups, h_nrows, h_nshort (per level: rows, rows shorter than LISHIP_SWEEP_LONG_ROW) on the host. */
#define LISHIP_SWEEP_MUL  0     /* x[i] = (b[i] - sum v x[j]) * wd[i] */
#define LISHIP_SWEEP_SUB  1     /* x[i] -= (0.0 + sum v x[j]) * wd[i] */
#define LISHIP_SWEEP_SCAT 2     /* x[i] = b[i] - sum v (x[j] * wd[j]) */
#define LISHIP_SWEEP_PLAIN 3    /* x[i] = b[i] - sum v x[j]: liship_sweep_plain_f64 only (liship_sweep_f64 takes 0 .. 2) */
#define LISHIP_SWEEP_SMALL_LEVEL 1024
#define LISHIP_SWEEP_LONG_ROW 64
typedef struct {
	int nlev, nrows, nnz, ngroups;
	const int *lptr, *llong, *rows, *rptr, *col;
	const double *val;
	const int *groups, *h_nrows, *h_nshort;
} liship_sweep_t;
/* every row of the sweep, level after level, on `stream`; b may equal x (unused by SUB) */
int  liship_sweep_f64(const liship_sweep_t *sweep, int mode, const double *b, double *x, const double *wd, void *stream);
/* the same rows without a diagonal: x[i] = b[i] - sum v x[j]; b may equal x (ILU: forward on L, backward on L^T) */
int  liship_sweep_plain_f64(const liship_sweep_t *sweep, const double *b, double *x, void *stream);

/* ------------------------------------------------------------------ ILU(k) numerical factorisation, the point form (kernels/ilu.hip on kernels/level_schedule.hpp)
 * The block factorisation below at bn = 1 behind a struct of its own: this entry checks its arguments, translates (nr = n, bn = 1) and
 * runs the same kernels.  A = (aptr, aindex, avalue) as it lies in HBM.  The symbolic pattern: row i of L = lcol[lptr[i] .. lptr[i+1]) ascending (a column
 * held twice: twice, side by side), of U = ucol[uptr[i] .. uptr[i+1]) in term order.  To find the place of a column in row i of U:
 * uskey = the row's columns ascending (ties by position), uspos = where each of them lies in ucol / uval; uspos NULL: the rows of
 * U are ascending as they are and uskey is ucol.  Of a column held twice the later place takes A's value and the updates.
 * Output in the pattern's order: lval, uval, d[i] = 1 / pivot (no pivot check: 1 / 0 = inf goes on).
 * `schedule`: the rows by forward level (lptr, llong, rows, groups, h_nrows, h_nshort; its col / val are not read) -- the rows from
 * llong[l] on are factorised by a workgroup each, the updates of ONE pivot spread over its threads, pivots in order; the others by
 * a thread each.  serial != 0 (some row of A holds a column twice, so one pivot may update a target twice): such rows are
 * factorised by one thread of their workgroup.  Every update is one rounded product and one rounded subtraction, in pivot order. */
typedef struct {
	int n, serial;
	const int *aptr, *aindex;
	const double *avalue;
	const int *lptr, *lcol, *uptr, *ucol, *uskey, *uspos;
	double *lval, *uval, *d;
} liship_ilu_t;
int  liship_ilu_factor_f64(const liship_ilu_t *ilu, const liship_sweep_t *schedule, void *stream);

/* ------------------------------------------------------------------ ILU(k) on blocks (kernels/ilu.hip on kernels/level_schedule.hpp): THE factorisation
 * liship_ilu_t with a block where it has a number: nr = ceil(n / bn) block rows, bn = 1, 2, 3; A = (aptr, aindex, avalue) the BSR
 * arrays in native layout (block k at avalue[k*bn*bn], column-major) -- at bn = 1 a CSR matrix's own arrays, and every bit of the point form; the pattern over block rows and block columns; lval / uval
 * bn*bn doubles per pattern place, d the nr diagonal blocks, INVERTED on return (lis_array_ge, after 1.0 on the diagonal of the last
 * block's padding when bn does not divide n).  buf = L_ij Dinv_j stored, target -= buf U_jc: every entry of a product summed left to
 * right from its first product, then one subtraction.  `schedule` over the nr block rows as for liship_ilu_factor_f64: long block
 * rows a workgroup each (one whole block update per thread, pivots in order), one thread when serial != 0. */
typedef struct {
	int n, nr, bn, serial;
	const int *aptr, *aindex;
	const double *avalue;
	const int *lptr, *lcol, *uptr, *ucol, *uskey, *uspos;
	double *lval, *uval, *d;
} liship_bilu_t;
int  liship_bilu_factor_f64(const liship_bilu_t *ilu, const liship_sweep_t *schedule, void *stream);
/* one block sweep over a layout of ceil(n / bn) block rows whose val holds bn*bn doubles per place: x_i = b_i, then per term in order
 * x_i[r] = x_i[r] - ((a[r] xj[0] + a[r+bn] xj[1]) + a[r+2bn] xj[2]); dinv not NULL: x_i = dinv_i x_i at the end (same sums).  x reads
 * as +0.0 from n on and is never written there; b may equal x.  bn = 1: liship_sweep_plain_f64 (dinv NULL) or liship_sweep_f64 in mode
 * LISHIP_SWEEP_MUL with wd = dinv, after this entry's own argument checks -- the same roundings in the same order. */
int  liship_bilu_sweep_f64(const liship_sweep_t *sweep, int n, int bn, const double *dinv, const double *b, double *x, void *stream);
/* dst block p = src block perm[p], blocks of bs doubles: liship_permute_gather_f64 for the values of a block layout */
int  liship_block_gather_f64(int nblocks, int bs, const int *perm, const double *src, double *dst, void *stream);

/* ------------------------------------------------------------------ block SSOR sweeps (kernels/bsptrsv.hip on kernels/level_schedule.hpp, -p ssor on BSR storage)
 * One sweep of lis_matrix_solve_bsr / lis_matrix_solveh_bsr over a layout of ceil(n / bn) block rows whose val holds bn*bn doubles per
 * place in native column-major order; wd: the inverted blocks of omega D, one per block row.  Every scalar row is one ordered chain:
 *   transposed == 0, LISHIP_SWEEP_MUL   t = b_i; per term, c ascending: t[r] -= a(r,c) x_j[c];  x_i = wd_i t
 *                    LISHIP_SWEEP_SUB   t = +0.0; t[r] += a(r,c) x_j[c];                        x_i -= wd_i t        (b is not read)
 *   transposed != 0, LISHIP_SWEEP_MUL   t = b_i; per term: t[c] -= (sum_r a(r,c) x_j[r]);       x_i = wd_i^T t
 *                    LISHIP_SWEEP_SCAT  t = b_i; per term: t[c] -= (sum_r a(r,c) work_j[r]);    x_i = t, work_i = wd_i^T t
 * the sums over r and the products with wd_i summed left to right, from the first product for bn <= 3 and from +0.0 for bn >= 4.
 * b and x read as +0.0 from n on and x is never written there; b may equal x.  work (SCAT, bn >= 2): bn * ceil(n / bn) doubles, all
 * written.  Any other mode, bn outside 1 .. 8 or a layout of another size: LISHIP_ERR_ARG.  bn = 1: liship_sweep_f64 after this entry's
 * own argument checks -- the same roundings in the same order.  liship_bsweep_chunk(bn): the terms of a long block row whose products
 * lie in LDS at once (0: bn is not served; bn = 1: 256, the workgroup of the point sweep's level kernel, whose long rows take a product
 * per thread). */
int  liship_bsweep_f64(const liship_sweep_t *sweep, int n, int bn, int mode, int transposed, const double *b, double *x,
                       const double *wd, double *work, void *stream);
int  liship_bsweep_chunk(int bn);

/* ------------------------------------------------------------------ block diagonal (kernels/bdiag.hip, -p bjacobi)
 * d: nr = ceil(n / bn) blocks of bn x bn doubles, block b at d[b*bn*bn], entry (i, j) at i + j*bn (LIS_MATRIX_DIAG).
 * inverse: every block replaced by its inverse, by the reference's lis_array_ge (LU without pivoting, no pivot check: 1 / 0 = inf goes on), after the
 * last block got 1.0 on the diagonal of its padding when bn does not divide n.  bn <= 8: work is not read; larger: work holds nr*bn*bn doubles.
 * matvec: y[0 .. n) = D x, or D^T x block by block (transposed != 0), each row summed left to right, from the first product for bn <= 4 (transposed:
 * bn <= 3) and from +0.0 for larger blocks, as the reference's routines do; x is read as +0.0 from n on; y must not be x. */
int  liship_bdiag_inverse_f64(int n, int nr, int bn, double *d, double *work, void *stream);
int  liship_bdiag_matvec_f64(int n, int nr, int bn, int transposed, const double *d, const double *x, double *y, void *stream);

/* ------------------------------------------------------------------ double-double ("quad", -f quad) vectors and products (kernels/quad.hip on kernels/dd.hpp)
 * A vector is two arrays (hi, lo), a scalar two doubles, the matrix plain CSR.  The arithmetic is the reference's SSE2 build's (dd.hpp): the sloppy add, Dekker's
 * product with the error term from one fma, the packed form of the product (mul2) for the elements the reference takes in pairs and the scalar form (mul) for
 * the odd last element of a thread's chunk LIS_GET_ISIE(t, T, n), T that of liship_set_reference_reductions (0 and 1: one chunk).
 *   axpy   y = y + a*x        xpay   y = x + a*y        axpyz   z = y + a*x        (outputs may be inputs)
 *   muld   x = b * d, d double (Jacobi's psolve and psolveh; x may be b)           widen   hi = v, lo = 0
 *   dot    result[0 .. 2) = <x, y>, every term mul2(y_i, x_i) (the scalar form for a chunk's odd last element in the reference-order mode).  T = 0: lane g of
 *          G * 256 (G = liship_dot_dd_grid(n)) chains elements g, g + G*256, ... from (0, 0); 64 lanes fold by taking lane l + off for off = 32 .. 1, a
 *          workgroup's 4 wavefronts are added in order, the G partials go through one more workgroup the same way (lane l chains partials l, l + 256, ...).
 *          T > 0: per chunk accumulator 0 / 1 chain the terms at even / odd places, acc0 + acc1, then the odd last element; the chunk sums are added in
 *          order from (0, 0).  work: liship_dot_dd_work_bytes() of HBM
 *   spmv_csr     per row: entries j, j+1 to accumulators 0 and 1 from (0, 0) (each add(acc, muld(x[col], value))), y = acc0 + acc1, then an odd last entry is
 *                added to y.  Rows in workgroups of liship_spmv_csr_dd_rows_per_block(), their entries through LDS in stages of liship_spmv_csr_dd_stage()
 *   spmv_csr_t   y = A^T x from the transposed CSR copy (rows = the columns of A, a row's entries in ascending row of A): one chain per output from (0, 0),
 *                then one add onto (0, 0) -- the reference at one thread; at more threads the reference's A^T x has no defined bits
 * liship_dd_scalar: dd.hpp as the host compiler built it (op 0 add, 1 mul, 2 mul2, 3 muld by b.hi, 4 div, 5 two-prod by fma, 6 two-prod by Dekker's split). */
int  liship_axpy_dd_f64(int n, double ahi, double alo, const double *xhi, const double *xlo, double *yhi, double *ylo, void *stream);
int  liship_xpay_dd_f64(int n, const double *xhi, const double *xlo, double ahi, double alo, double *yhi, double *ylo, void *stream);
int  liship_axpyz_dd_f64(int n, double ahi, double alo, const double *xhi, const double *xlo, const double *yhi, const double *ylo,
                         double *zhi, double *zlo, void *stream);
int  liship_muld_dd_f64(int n, const double *bhi, const double *blo, const double *d, double *xhi, double *xlo, void *stream);
int  liship_widen_dd_f64(int n, const double *v, double *hi, double *lo, void *stream);
int  liship_dot_dd_grid(int n);
size_t liship_dot_dd_work_bytes(void);
int  liship_dot_dd_f64(int n, const double *xhi, const double *xlo, const double *yhi, const double *ylo, double *result, void *work, void *stream);
int  liship_spmv_csr_dd_rows_per_block(void);
int  liship_spmv_csr_dd_stage(void);
int  liship_spmv_csr_dd_f64(int n, const int *ptr, const int *index, const double *value, const double *xhi, const double *xlo,
                            double *yhi, double *ylo, void *stream);
int  liship_spmv_csr_t_dd_f64(int rows, const int *tptr, const int *tindex, const double *tvalue, const double *xhi, const double *xlo,
                              double *yhi, double *ylo, void *stream);
int  liship_dd_scalar(int op, double ahi, double alo, double bhi, double blo, double *out);

#ifdef __cplusplus
}
#endif
#endif
