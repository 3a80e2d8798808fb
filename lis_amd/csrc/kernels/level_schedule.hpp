// level_schedule.hpp -- the walker of a level schedule (liship_sweep_t), shared by the triangular sweeps (sptrsv.hip) and by the ILU(k)
// factorisation and block sweeps (ilu.hip).
//
// A schedule is a list of levels; the rows of one level do not depend on each other, every row depends only on rows of earlier
// levels.  Inside a level the short rows come first, the long ones last (lptr[l] .. llong[l] .. lptr[l + 1]).  Dependencies
// between levels are kernel boundaries on the stream, or __syncthreads() inside the single-workgroup kernel that runs a run of
// small levels (all of it on one CU, whose vector L1 the workgroup's waves share: no data crosses a CU).  No workgroup ever waits
// on a flag another workgroup writes.
//
// What is done to a row is the "rows" policy P, passed to the kernels by value:
//   const int *level_ptr() / level_long()                 lptr / llong of the schedule, in HBM
//   void short_row(int r)                                 the row at place r of the level order, by this thread
//   template <int BS, bool IN_RUN> void long_row(int r)   the same by this workgroup of BS threads; every thread calls it
// A policy keeps the barriers its long rows need (IN_RUN: another row of the same workgroup follows) and owns whatever LDS they use.
#pragma once
#include "common.hpp"
#include "liship.h"

constexpr int LEVEL_BLOCK = 256;        // one level per launch: a thread per short row, a workgroup per long row
constexpr int RUN_BLOCK = 1024;         // a run of small levels: one workgroup
static_assert(LISHIP_SWEEP_SMALL_LEVEL <= RUN_BLOCK, "a level of a run gives no thread of the run's workgroup more than one short row");

// one level: blocks [0, nshort_blocks) take a short row per thread, each further block one long row
template <class P>
__global__ __launch_bounds__(LEVEL_BLOCK) void level_kernel(P p, int level, int nshort_blocks)
{
    const int r0 = p.level_ptr()[level], rl = p.level_long()[level];
    if ((int)blockIdx.x < nshort_blocks) {
        const int r = r0 + (int)blockIdx.x * LEVEL_BLOCK + (int)threadIdx.x;
        if (r < rl) p.short_row(r);
    } else {
        p.template long_row<LEVEL_BLOCK, false>(rl + (int)blockIdx.x - nshort_blocks);
    }
}

// levels [l0, l1) in one workgroup, a barrier between consecutive levels
template <class P>
__global__ __launch_bounds__(RUN_BLOCK) void run_kernel(P p, int l0, int l1)
{
    for (int l = l0; l < l1; l++) {
        const int r0 = p.level_ptr()[l], rl = p.level_long()[l], r1 = p.level_ptr()[l + 1];
        for (int r = r0 + (int)threadIdx.x; r < rl; r += RUN_BLOCK) p.short_row(r);
        for (int r = rl; r < r1; r++) p.template long_row<RUN_BLOCK, true>(r);
        __syncthreads();
    }
}

// every launch of the schedule, in order, on `st`
template <class P>
int walk_levels(const liship_sweep_t *sw, const P &p, hipStream_t st)
{
    for (int g = 0; g < sw->ngroups; g++) {
        const int l0 = sw->groups[3 * g], l1 = sw->groups[3 * g + 1], run = sw->groups[3 * g + 2];
        if (run) {
            run_kernel<P><<<1, RUN_BLOCK, 0, st>>>(p, l0, l1);
        } else {
            const int nshort = sw->h_nshort[l0];
            const int nsb = (nshort + LEVEL_BLOCK - 1) / LEVEL_BLOCK;
            const int grid = nsb + (sw->h_nrows[l0] - nshort);
            level_kernel<P><<<grid, LEVEL_BLOCK, 0, st>>>(p, l0, nsb);
        }
        LAUNCH_CHECK();
    }
    return 0;
}
