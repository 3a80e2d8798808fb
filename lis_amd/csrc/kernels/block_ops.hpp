// block_ops.hpp -- what the kernels on dense bn x bn blocks share (bdiag.hip: -p bjacobi; ilu.hip: -p ilu): the
// reference's block inverse, lis_array_ge, operation for operation, and the 1.0 on the diagonal of the last block's padding.
#pragma once
#include "common.hpp"

namespace {

// lis_array_ge on a block `a` with its LU copy `lu`, both indexed through accessors so that registers and HBM share the statement
template <typename A, typename L>
__device__ __forceinline__ void invert_block(const int n, A a, L lu)
{
    for (int e = 0; e < n * n; e++) lu(e) = a(e);
    for (int k = 0; k < n; k++) {
        lu(k + k * n) = 1.0 / lu(k + k * n);
        for (int i = k + 1; i < n; i++) {
            const double t = lu(i + k * n) * lu(k + k * n);
            for (int j = k + 1; j < n; j++) lu(i + j * n) -= t * lu(k + j * n);
            lu(i + k * n) = t;
        }
    }
    for (int k = 0; k < n; k++) {
        for (int i = 0; i < n; i++) {
            double t = (i == k) ? 1.0 : 0.0;
            for (int j = 0; j < i; j++) t -= lu(i + j * n) * a(j + k * n);
            a(i + k * n) = t;
        }
        for (int i = n - 1; i >= 0; i--) {
            double t = a(i + k * n);
            for (int j = i + 1; j < n; j++) t -= lu(i + j * n) * a(j + k * n);
            a(k * n + i) = t * lu(i + i * n);
        }
    }
}

struct RegRef {
    double *p;
    __device__ __forceinline__ double &operator()(int e) const { return p[e]; }
};

// the 1.0 on the padding's diagonal: block nr - 1 when n % bn != 0.  The fixed sizes walk every i under a predicate: a loop with a
// run-time bound would index the register array dynamically and send the whole block to scratch.
template <int BN>
__device__ __forceinline__ void pad_last_block(int n, int nr, int b, double *blk)
{
    const int k = n % BN;
    const bool last = k != 0 && b == nr - 1;
#pragma unroll
    for (int i = 0; i < BN; i++)
        if (last && i >= k) blk[i * (BN + 1)] = 1.0;
}

}  // namespace
