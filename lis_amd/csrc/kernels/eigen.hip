// eigen.hip -- the kernels the eigensolvers (host/lis_esolver.c) add to the library, for gfx950 (f64):
//
//   liship_ritz_tail_f64           the tail of a subspace iteration (-e si) in one pass: the residual's sum of squares, r normalised, v = r
//   liship_multidot_f64            K inner products over V <= 8 vectors in one pass, every vector's tile read once per workgroup,
//                                  every sum in the bits liship_dot_f64 gives that pair alone (the CG / CR eigensolvers' Gram blocks)
//   liship_csr_shift_diagonal_f64  value -= sigma on the first stored entry of each row whose column is the row
//                                  (lis_matrix_shift_diagonal of a matrix that lives in HBM)
//
// The order of a sum is the contract of include/liship.h "reductions", restated by tests/reduction_model.py: level 1 in workgroups of
// 256 lanes over tiles of 2048 elements -- with the 16 B lane mapping when BOTH arrays of the pair are 16 B aligned, else the 8 B
// one --, the wavefront butterfly, the wavefronts in order, then the folds of vector_ops.hip (liship_internal_fold), which this file
// calls and does not restate.  A lane's running sum of a pair adds that pair's terms in the order the single dot's lane adds them,
// each product rounded once and each sum once (-ffp-contract=off); what another pair does in the same lane cannot change it.
//
// How one pass serves every pair without dynamic register indexing: the launcher sorts the vectors, 16 B aligned ones first, and the
// kernel -- a template on V -- forms ALL V (V + 1) / 2 unordered pairs of them at compile-time register indices; the pairs that were
// asked for are picked when the workgroup's sums are written (a multiplication commutes, so <a,b> and <b,a> are one slot).  Pairs
// among the aligned vectors take the 16 B mapping from one 16 B load per vector and step; when some vector is only 8 B aligned, a
// second sweep over the same tile forms the pairs that involve one with the 8 B mapping, and reads the tile of every vector again
// (from cache: the rare layout, an array at an odd offset).
//
// Two things a caller should know.  All V (V + 1) / 2 slots are formed whatever K is -- 21 for CG's 12 pairs, 10 for CR's 4-pair block: the
// products are free beside the loads, the price is registers (see DESIGN.md 9 for VGPRs per V) -- so pass only the vectors the pairs name.  And a
// step announced with liship_krylov_chain is NOT run by the one-pass form: unlike liship_dot_f64, its last kernel consumes no pending step, which
// stays pending for the next reduction or liship_krylov_chain_flush; the K separate dots of the reference-order mode would hand it to the first
// of them.  Announce none before this call (the eigensolver loops do not).
#include "common.hpp"
#include "liship.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE;
constexpr int U = 4;                               // 16 B steps per lane: 2048 elements per workgroup, as vector_ops.hip
constexpr int TILE_PAIRS = BLOCK * U;
constexpr long long NT_LOAD_ELEMS = 32LL << 20;    // vectors beyond 256 MiB stream past the caches (as vector_ops.hip)
constexpr int MAXV = LISHIP_MULTIDOT_MAX_VECS;
constexpr size_t MAX_PARTIALS = (1u << 20) + 4096; // vector_ops.hip: each half of the work buffer holds 2 * MAX_PARTIALS doubles

struct MdArgs {
    int n, nvec, naligned, K;
    const double *v[MAXV];                         // sorted: [0, naligned) 16 B aligned
    unsigned char slot_of[LISHIP_MULTIDOT_MAX_PAIRS];   // result k <- slot
    const double *skip;                            // the guard flag of the device-driven loops (vector_ops.hip), NULL when none
};

// slot of the unordered pair i <= j among V vectors, row-major over the upper triangle
__host__ __device__ constexpr int slot_index(int V, int i, int j) { return i * V - i * (i - 1) / 2 + (j - i); }

template <bool NT> __device__ __forceinline__ v2f64 ld2(const double *p, long long pair)
{
    const v2f64 *q = reinterpret_cast<const v2f64 *>(p) + pair;
    return NT ? __builtin_nontemporal_load(q) : *q;
}

template <int V, bool NT>
__global__ __launch_bounds__(BLOCK)
void multidot_level1(MdArgs A, int stride, double *__restrict__ partial)
{
    constexpr int S = V * (V + 1) / 2;
    __shared__ double scratch[S][NW];
    if (A.skip && A.skip[0] != 0.0) return;
    const int n = A.n, Va = A.naligned;
    double s[S];
#pragma unroll
    for (int q = 0; q < S; q++) s[q] = 0.0;

    // pairs among the 16 B aligned vectors: lane t of block b takes the element pairs p = 1024 b + t + 256 u, element 2p then 2p + 1
    if (Va > 0) {
        const long long npairs = n >> 1;
        const long long base = (long long)blockIdx.x * TILE_PAIRS + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long p = base + u * BLOCK;
            if (p < npairs) {
                v2f64 x[V];
#pragma unroll
                for (int i = 0; i < V; i++) if (i < Va) x[i] = ld2<NT>(A.v[i], p);
#pragma unroll
                for (int i = 0; i < V; i++)
#pragma unroll
                    for (int j = i; j < V; j++)
                        if (j < Va) {
                            double &acc = s[slot_index(V, i, j)];
                            acc += x[i].x * x[j].x;
                            acc += x[i].y * x[j].y;
                        }
            }
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {       // the last element of an odd n, after lane 0's own pairs
            double x[V];
#pragma unroll
            for (int i = 0; i < V; i++) if (i < Va) x[i] = A.v[i][n - 1];
#pragma unroll
            for (int i = 0; i < V; i++)
#pragma unroll
                for (int j = i; j < V; j++)
                    if (j < Va) s[slot_index(V, i, j)] += x[i] * x[j];
        }
    }
    // pairs with a vector that is only 8 B aligned: lane t of block b adds the elements 2048 b + t + 256 u, u = 0..7
    if (Va < V) {
        const long long i0 = (long long)blockIdx.x * (2 * TILE_PAIRS) + threadIdx.x;
        for (int u = 0; u < 2 * U; u++) {
            const long long e = i0 + u * BLOCK;
            if (e < n) {
                double x[V];
#pragma unroll
                for (int i = 0; i < V; i++) x[i] = A.v[i][e];
#pragma unroll
                for (int i = 0; i < V; i++)
#pragma unroll
                    for (int j = i; j < V; j++)
                        if (j >= Va) s[slot_index(V, i, j)] += x[i] * x[j];
            }
        }
    }
    // the workgroup's sums: butterfly per wavefront, the wavefronts added in order from 0.0 (block_sum of common.hpp, for every slot at once)
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int q = 0; q < S; q++) {
        const double t = wave_sum(s[q]);
        if (lane == 0) scratch[q][w] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < A.K) {
        const int q = A.slot_of[threadIdx.x];
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < NW; i++) t += scratch[q][i];
        partial[(size_t)threadIdx.x * stride + blockIdx.x] = t;
    }
}

template <int V>
int launch_level1(const MdArgs &A, int grid, int stride, double *dst, hipStream_t st)
{
    if (A.n > NT_LOAD_ELEMS) multidot_level1<V, true><<<grid, BLOCK, 0, st>>>(A, stride, dst);
    else                     multidot_level1<V, false><<<grid, BLOCK, 0, st>>>(A, stride, dst);
    LAUNCH_CHECK();
    return 0;
}

// one lane per row: the first stored entry whose column is the row (lis_matrix_csr.c:589-599), rows without one left alone
__global__ __launch_bounds__(BLOCK)
void csr_shift_diagonal_kernel(int n, const int *__restrict__ ptr, const int *__restrict__ idx, double *__restrict__ val, double sigma)
{
    const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const int e = ptr[r + 1];
    for (int k = ptr[r]; k < e; k++)
        if (idx[k] == (int)r) { val[k] -= sigma; break; }
}

// ---- the tail of a subspace iteration (lis_esolver_si.c:301-311) in one pass ---------------------------------------------------------
// sums = {sum r^2, theta = <v,r>} in HBM (one liship_multidot_f64 pass).  Per element, each product and each sum rounded once:
//   q = (-theta) * v + r        lis_vector_axpyz(-theta, v, r, q); q is not stored, q * q enters the sum
//   s = (1 / sqrt(sums[0])) * r lis_vector_scale(1 / nrm2, r); the reciprocal formed once per lane, as EW_SCALE_DEV of vector_ops.hip
//   r = s; v = s                lis_vector_copy(r, v)
// The sum of q^2 is liship_sumsq_f64's of a 16 B aligned array of n elements: the same grid, the same lane mapping, block_sum, the folds.
struct RtArgs { int n; const double *sums; double *r, *v; const double *skip; };

__device__ __forceinline__ void ritz_tail_term(double ntheta, double inv, double r, double v, double &s, double &acc)
{
    const double q = ntheta * v + r;
    acc += q * q;
    s = inv * r;
}

template <bool NT>
__global__ __launch_bounds__(BLOCK)
void ritz_tail_level1(RtArgs A, double *__restrict__ partial)
{
    __shared__ double scratch[NW];
    if (A.skip && A.skip[0] != 0.0) return;
    const int n = A.n;
    const double ntheta = -A.sums[1];
    const double inv = 1.0 / sqrt(A.sums[0]);
    double acc = 0.0;
    const long long npairs = n >> 1;
    const long long base = (long long)blockIdx.x * TILE_PAIRS + threadIdx.x;
    v2f64 r[U], v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const long long p = base + u * BLOCK;
        if (p < npairs) { r[u] = ld2<NT>(A.r, p); v[u] = ld2<NT>(A.v, p); }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const long long p = base + u * BLOCK;
        if (p < npairs) {
            v2f64 s;
            double s0, s1;
            ritz_tail_term(ntheta, inv, r[u].x, v[u].x, s0, acc);
            ritz_tail_term(ntheta, inv, r[u].y, v[u].y, s1, acc);
            s.x = s0; s.y = s1;
            __builtin_nontemporal_store(s, reinterpret_cast<v2f64 *>(A.r) + p);
            __builtin_nontemporal_store(s, reinterpret_cast<v2f64 *>(A.v) + p);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {           // the last element of an odd n, after lane 0's own pairs
        const int i = n - 1;
        double s;
        ritz_tail_term(ntheta, inv, A.r[i], A.v[i], s, acc);
        A.r[i] = s; A.v[i] = s;
    }
    const double t = block_sum<NW>(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// the reference's order for OMP_NUM_THREADS = T (reduce_ref_kernel of vector_ops.hip): workgroup c is thread c's chunk LIS_GET_ISIE(c, T, n), its lanes
// form the terms of a tile, lane 0 adds them left to right out of LDS; ritz_tail_ref_final adds the T partials in chunk order from 0.0
constexpr int RT_REF_TILE = 2048;
__global__ __launch_bounds__(BLOCK)
void ritz_tail_ref_kernel(RtArgs A, int T, double *__restrict__ partial)
{
    __shared__ double t0[RT_REF_TILE];
    if (A.skip && A.skip[0] != 0.0) return;
    const int n = A.n, c = blockIdx.x;
    const double ntheta = -A.sums[1];
    const double inv = 1.0 / sqrt(A.sums[0]);
    long long is, ie;
    if (c < n % T) { ie = n / T + 1; is = ie * c; } else { ie = n / T; is = ie * c + n % T; }
    ie += is;
    double s = 0.0;
    for (long long base = is; base < ie; base += RT_REF_TILE) {
        const int cnt = (int)(ie - base < RT_REF_TILE ? ie - base : RT_REF_TILE);
        for (int j = threadIdx.x; j < cnt; j += BLOCK) {
            const long long i = base + j;
            double out, term = 0.0;
            ritz_tail_term(ntheta, inv, A.r[i], A.v[i], out, term);      // (0.0 + q * q is q * q in every bit)
            A.r[i] = out; A.v[i] = out;
            t0[j] = term;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int j = 0; j < cnt; j++) s += t0[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[c] = s;
}

__global__ void ritz_tail_ref_final(int T, const double *__restrict__ partial, double *result, const double *skip)
{
    if (threadIdx.x != 0 || (skip && skip[0] != 0.0)) return;
    double s = 0.0;
    for (int c = 0; c < T; c++) s += partial[c];
    result[0] = s;
}

} // namespace

extern "C" int liship_ritz_tail_f64(int n, const double *sums, double *r, double *v, double *result, void *work, void *stream)
{
    if (n <= 0 || !sums || !r || !v || !result || !work) return LISHIP_ERR_ARG;
    if (!aligned16(r) || !aligned16(v)) return LISHIP_ERR_ARG;
    {	// r and v are each read and written by the lane that owns the element: arrays that overlap (one array given twice included) are refused
        const uintptr_t a = reinterpret_cast<uintptr_t>(r), b = reinterpret_cast<uintptr_t>(v), len = (uintptr_t)n * sizeof(double);
        if (a < b + len && b < a + len) return LISHIP_ERR_ARG;
    }
    RtArgs A{n, sums, r, v, liship_internal_guard()};
    double *partial = static_cast<double *>(work);
    double *spare = partial + 2 * MAX_PARTIALS;
    hipStream_t st = as_stream(stream);
    const int T = liship_internal_ref_chunks();
    if (T > 0) {
        ritz_tail_ref_kernel<<<T, BLOCK, 0, st>>>(A, T, partial);
        LAUNCH_CHECK();
        ritz_tail_ref_final<<<1, WAVE, 0, st>>>(T, partial, result, A.skip);
        LAUNCH_CHECK();
        return 0;
    }
    const int grid = (int)((((long long)n + 1) / 2 + TILE_PAIRS - 1) / TILE_PAIRS);      // liship_sumsq_f64's grid for this n: the order of the sum hangs on it
    const bool single = (grid == 1);
    double *dst = single ? result : partial;
    if (n > NT_LOAD_ELEMS) ritz_tail_level1<true><<<grid, BLOCK, 0, st>>>(A, dst);
    else                   ritz_tail_level1<false><<<grid, BLOCK, 0, st>>>(A, dst);
    LAUNCH_CHECK();
    if (single) return 0;
    return liship_internal_fold(grid, 1, grid, partial, spare, result, stream);
}

extern "C" int liship_multidot_f64(int n, int nvec, const double *const *vecs, int K, const int (*pairs)[2], double *result,
                                   void *work, void *stream)
{
    if (n < 0 || nvec < 1 || nvec > MAXV || K < 1 || K > LISHIP_MULTIDOT_MAX_PAIRS || !vecs || !pairs || !result || !work) return LISHIP_ERR_ARG;
    for (int k = 0; k < K; k++)
        if (pairs[k][0] < 0 || pairs[k][0] >= nvec || pairs[k][1] < 0 || pairs[k][1] >= nvec) return LISHIP_ERR_ARG;
    for (int i = 0; i < nvec; i++) if (!vecs[i]) return LISHIP_ERR_ARG;
    int grid = (int)((((long long)n + 1) / 2 + TILE_PAIRS - 1) / TILE_PAIRS);
    if (grid < 1) grid = 1;
    // the reference's order is one lane per chunk (vector_ops.hip reduce_ref_kernel): K of those passes, nothing to share.  The same for
    // a vector so long that K rows of workgroup partials do not fit the scratch (n beyond 2^31 / K * 2: no served matrix is that large)
    if (liship_internal_ref_chunks() > 0 || (size_t)K * (size_t)grid > 2 * MAX_PARTIALS) {
        for (int k = 0; k < K; k++) {
            const int rc = liship_dot_f64(n, vecs[pairs[k][0]], vecs[pairs[k][1]], result + k, work, stream);
            if (rc) return rc;
        }
        return 0;
    }
    MdArgs A;
    A.n = n; A.nvec = nvec; A.K = K; A.skip = liship_internal_guard();
    int place[MAXV], at = 0;
    for (int i = 0; i < nvec; i++) if (aligned16(vecs[i])) { place[i] = at; A.v[at++] = vecs[i]; }
    A.naligned = at;
    for (int i = 0; i < nvec; i++) if (!aligned16(vecs[i])) { place[i] = at; A.v[at++] = vecs[i]; }
    for (int i = nvec; i < MAXV; i++) A.v[i] = nullptr;
    for (int k = 0; k < K; k++) {
        int a = place[pairs[k][0]], b = place[pairs[k][1]];
        if (a > b) { const int t = a; a = b; b = t; }
        A.slot_of[k] = (unsigned char)slot_index(nvec, a, b);
    }
    for (int k = K; k < LISHIP_MULTIDOT_MAX_PAIRS; k++) A.slot_of[k] = 0;
    double *partial = static_cast<double *>(work);
    double *spare = partial + 2 * MAX_PARTIALS;
    hipStream_t st = as_stream(stream);
    const bool single = (grid == 1);               // one workgroup: its sums are the results (stride 1: result[k])
    double *dst = single ? result : partial;
    const int stride = single ? 1 : grid;
    int rc = LISHIP_ERR_ARG;
    switch (nvec) {
    case 1: rc = launch_level1<1>(A, grid, stride, dst, st); break;
    case 2: rc = launch_level1<2>(A, grid, stride, dst, st); break;
    case 3: rc = launch_level1<3>(A, grid, stride, dst, st); break;
    case 4: rc = launch_level1<4>(A, grid, stride, dst, st); break;
    case 5: rc = launch_level1<5>(A, grid, stride, dst, st); break;
    case 6: rc = launch_level1<6>(A, grid, stride, dst, st); break;
    case 7: rc = launch_level1<7>(A, grid, stride, dst, st); break;
    case 8: rc = launch_level1<8>(A, grid, stride, dst, st); break;
    }
    if (rc || single) return rc;
    return liship_internal_fold(grid, K, grid, partial, spare, result, stream);
}

extern "C" int liship_csr_shift_diagonal_f64(int n, const int *ptr, const int *index, double *value, double sigma, void *stream)
{
    if (n < 0 || (n > 0 && !ptr)) return LISHIP_ERR_ARG;       // (index / value may be NULL when no row has an entry: never read then)
    if (n == 0) return 0;
    const int grid = (int)(((long long)n + BLOCK - 1) / BLOCK);
    csr_shift_diagonal_kernel<<<grid, BLOCK, 0, as_stream(stream)>>>(n, ptr, index, value, sigma);
    LAUNCH_CHECK();
    return 0;
}
