// ilu_pattern.hpp -- where a row of the ILU(k) pattern keeps a column: what the point factorisation (ilu.hip) and the block
// factorisation (bilu.hip) share.  The L part of a row is ascending, the U part has an ascending copy of its columns with the places
// (uskey / uspos; uspos NULL: U's rows are ascending as they are): a binary search in the row's own keys, the last of equal keys
// answering (the reference's jw[] keeps the later place of a column stored twice).
#pragma once
#include "common.hpp"

namespace {

// the last index in [lo, hi) whose key is c, or -1
__device__ __forceinline__ int find_last(const int *key, int lo, int hi, int c)
{
    int a = lo, b = hi;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (key[m] <= c) a = m + 1; else b = m;
    }
    return (a > lo && key[a - 1] == c) ? a - 1 : -1;
}

struct Row { int i, l0, l1, u0, u1; };

// F: a factorisation's arguments with lptr and uptr
template <class F>
__device__ __forceinline__ Row row_of(const F &f, int i)
{
    return Row{i, f.lptr[i], f.lptr[i + 1], f.uptr[i], f.uptr[i + 1]};
}

// the place (an index into lval when *lower, into uval otherwise) at which row r keeps the off-diagonal column c, or -1
template <class F>
__device__ __forceinline__ int place_index(const F &f, const Row &r, int c, bool *lower)
{
    *lower = c < r.i;
    if (c < r.i) return find_last(f.lcol, r.l0, r.l1, c);
    const int p = find_last(f.uskey, r.u0, r.u1, c);
    if (p < 0) return -1;
    return f.uspos ? f.uspos[p] : p;
}

}  // namespace
