// vector_pass.hpp -- the one statement of how a streaming pass over n-vectors maps elements to lanes (vector_ops.hip, eigen.hip).
//
// A workgroup of 256 lanes owns a tile of 2048 elements.  When every array of the pass is 16 B aligned, lane t of block b takes the
// element pairs p = 1024 b + t + 256 u, u = 0..3: all loads of the four steps are issued before the first use, then element 2p before
// 2p + 1, step by step; results leave by non-temporal 16 B stores; lane 0 of block 0 takes the last element of an odd n after its own
// pairs.  Arrays that are only 8 B aligned take the scalar walk: lane t of block b the elements 2048 b + t + 256 u, u = 0..7.
// Launch shape (measured, tools/ubench_axpy.hip, 1 GiB vectors): one-shot grid, non-temporal loads once the vectors are larger than the
// 256 MiB Infinity Cache: 4.8 -> 6.1 TB/s for axpy.
//
// The order in which a lane meets its elements is the order of every running sum a pass keeps: tests/reduction_model.py restates this
// mapping, and the bits of every reduction rest on it.  A pass is a functor over one element of vector_pass below (cg_direction_kernel; the
// form for a new fused pass).  ew_kernel and reduce_level1 (vector_ops.hip) write the walk out in this order, on the machine code their
// recorded times were measured on; multidot_level1 (eigen.hip) does too, its all-pairs form being another shape of pass.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE;
constexpr int U = 4;                               // 16 B accesses per lane per array
constexpr int PAIRS_PER_BLOCK = BLOCK * U;         // 2048 doubles per workgroup
constexpr long long NT_LOAD_ELEMS = 32LL << 20;    // vectors beyond 256 MiB: stream past the caches
constexpr size_t MAX_PARTIALS = (1u << 20) + 4096; // level-1 partials of a 2^31-element vector (+ level 2); each half of the work buffer holds twice that
constexpr int REF_TILE = 2048;                     // terms a workgroup of the reference-order kernels forms before lane 0 adds them

inline int blocks_for(long long npairs) { return (int)((npairs + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK); }
// the grid of a pass over n elements (either walk: a block's 1024 pairs are its 2048 elements)
inline int pass_grid(long long n) { return blocks_for((n + 1) / 2); }

template <bool NT> __device__ __forceinline__ v2f64 ld2(const double *p, long long pair)
{
    const v2f64 *q = reinterpret_cast<const v2f64 *>(p) + pair;
    return NT ? __builtin_nontemporal_load(q) : *q;
}
__device__ __forceinline__ void st2(double *p, long long pair, v2f64 v)
{
    __builtin_nontemporal_store(v, reinterpret_cast<v2f64 *>(p) + pair);
}

// LIS_GET_ISIE(c, T, n, is, ie) of the reference (include/lis.h:1067-1078, the static schedule of `omp for`): chunk c of T is [is, ie)
__host__ __device__ inline void chunk_bounds(int c, int T, int n, long long &is, long long &ie)
{
    if (c < n % T) { ie = n / T + 1; is = ie * c; } else { ie = n / T; is = ie * c + n % T; }
    ie += is;
}

// The pass.  f(x, o) is called once per element with x[k] = in[k][i], k < NIN, and leaves o[k] for out[k][i], k < NOUT; an out[] may be an
// in[] (each lane reads its elements before it writes them).  f may add to running sums it captured: they then hold this lane's terms in
// the order above.
template <bool NT, bool VEC, int NIN, int NOUT, class F>
__device__ __forceinline__ void vector_pass(int n, const double *const (&in)[NIN], double *const (&out)[NOUT], F &&f)
{
    auto scalar = [&](long long i) {
        double x[NIN], o[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; k++) x[k] = in[k][i];
        f(x, o);
#pragma unroll
        for (int k = 0; k < NOUT; k++) out[k][i] = o[k];
    };
    if (VEC) {
        const long long npairs = n >> 1;
        // an address is the tile's (uniform: scalar registers) + the lane's 32-bit offset inside the tile, one vector register for all arrays
        const long long tile = (long long)blockIdx.x * PAIRS_PER_BLOCK, base = tile + threadIdx.x;
        v2f64 v[U][NIN];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long p = base + u * BLOCK;
            if (p < npairs) {
#pragma unroll
                for (int k = 0; k < NIN; k++) v[u][k] = ld2<NT>(in[k] + 2 * tile, threadIdx.x + u * BLOCK);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const long long p = base + u * BLOCK;
            if (p < npairs) {
                double x[NIN], o0[NOUT], o1[NOUT];
#pragma unroll
                for (int k = 0; k < NIN; k++) x[k] = v[u][k].x;
                f(x, o0);
#pragma unroll
                for (int k = 0; k < NIN; k++) x[k] = v[u][k].y;
                f(x, o1);
#pragma unroll
                for (int k = 0; k < NOUT; k++) {
                    v2f64 r;
                    r.x = o0[k]; r.y = o1[k];
                    st2(out[k] + 2 * tile, threadIdx.x + u * BLOCK, r);
                }
            }
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) scalar(n - 1);     // the last element of an odd n, after lane 0's own pairs
    } else {                                     // arrays that are only 8 B aligned
        const long long i0 = (long long)blockIdx.x * (2 * PAIRS_PER_BLOCK) + threadIdx.x;
#pragma unroll
        for (int u = 0; u < 2 * U; u++) {
            const long long i = i0 + u * BLOCK;
            if (i < n) scalar(i);
        }
    }
}

// The launch choice: launch(nt, vec) is called with the two compile-time flags of the instantiation that serves these arrays -- the 8 B
// walk when some array is not 16 B aligned (vec false), else the 16 B walk, with non-temporal loads beyond NT_LOAD_ELEMS.
inline bool nt_loads(long long n) { return n > NT_LOAD_ELEMS; }
template <class L>
inline void launch_pass(bool vec, long long n, L &&launch)
{
    if (!vec)             launch(std::false_type{}, std::false_type{});
    else if (nt_loads(n)) launch(std::true_type{}, std::true_type{});
    else                  launch(std::false_type{}, std::true_type{});
}

} // namespace
