// eigen.hip -- the kernels the eigensolvers (host/lis_esolver.c) add to the library, for gfx950 (f64):
//
//   liship_multidot_f64           K inner products over V <= 8 vectors in one pass, every vector's tile read once per workgroup,
//                                  every sum in the bits liship_dot_f64 gives that pair alone (the CG / CR eigensolvers' Gram blocks)
//   liship_csr_shift_diagonal_f64  value -= sigma on the first stored entry of each row whose column is the row
//                                  (lis_matrix_shift_diagonal of a matrix that lives in HBM)
// (The fused tail of a subspace iteration, liship_ritz_tail_f64, is a reduction op of vector_ops.hip: RED_RITZ_TAIL.)
//
// The order of a sum is the contract of include/liship.h "reductions", restated by tests/reduction_model.py: level 1 in workgroups of
// 256 lanes over tiles of 2048 elements -- with the 16 B lane mapping when BOTH arrays of the pair are 16 B aligned, else the 8 B
// one --, the wavefront butterfly, the wavefronts in order, then the folds of vector_ops.hip (liship_internal_fold).  The tile, the grid
// and the loads are vector_pass.hpp's; the walk is written out here, because all pairs of V vectors is another shape of pass than one
// functor per element, in the element order that header states.  A lane's running sum of a pair adds that pair's terms in the order the single dot's lane adds them,
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
#include "vector_pass.hpp"
#include "liship.h"

namespace {

constexpr int MAXV = LISHIP_MULTIDOT_MAX_VECS;

struct MdArgs {
    int n, nvec, naligned, K;
    const double *v[MAXV];                         // sorted: [0, naligned) 16 B aligned
    unsigned char slot_of[LISHIP_MULTIDOT_MAX_PAIRS];   // result k <- slot
    const double *skip;                            // the guard flag of the device-driven loops (vector_ops.hip), NULL when none
};

// slot of the unordered pair i <= j among V vectors, row-major over the upper triangle
__host__ __device__ constexpr int slot_index(int V, int i, int j) { return i * V - i * (i - 1) / 2 + (j - i); }

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
        const long long base = (long long)blockIdx.x * PAIRS_PER_BLOCK + threadIdx.x;
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
        const long long i0 = (long long)blockIdx.x * (2 * PAIRS_PER_BLOCK) + threadIdx.x;
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
    if (nt_loads(A.n)) multidot_level1<V, true><<<grid, BLOCK, 0, st>>>(A, stride, dst);       // (the kernel picks its walk per pair: MdArgs::naligned)
    else               multidot_level1<V, false><<<grid, BLOCK, 0, st>>>(A, stride, dst);
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

} // namespace

extern "C" int liship_multidot_f64(int n, int nvec, const double *const *vecs, int K, const int (*pairs)[2], double *result,
                                   void *work, void *stream)
{
    if (n < 0 || nvec < 1 || nvec > MAXV || K < 1 || K > LISHIP_MULTIDOT_MAX_PAIRS || !vecs || !pairs || !result || !work) return LISHIP_ERR_ARG;
    for (int k = 0; k < K; k++)
        if (pairs[k][0] < 0 || pairs[k][0] >= nvec || pairs[k][1] < 0 || pairs[k][1] >= nvec) return LISHIP_ERR_ARG;
    for (int i = 0; i < nvec; i++) if (!vecs[i]) return LISHIP_ERR_ARG;
    int grid = pass_grid(n);                       // liship_dot_f64's grid for this n: the order of the sums hangs on it
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
