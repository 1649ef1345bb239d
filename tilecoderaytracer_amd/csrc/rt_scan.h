/*
 * rt_scan.h -- stream compaction in order, without any workgroup waiting for another: the pieces a unit needs to turn a
 * per-lane flag into a dense list that keeps the lanes' order.  It is rt_adaptive.hip's pattern (flag -> counts per workgroup ->
 * two-level exclusive scan -> list) in a form a unit can include: rt_mirror_compact.hip does, and rt_indirect.hip could for its
 * dead records.  (rt_adaptive.hip keeps the kernels it was measured with.)
 *   rt_scan_rank           in a workgroup of kRankBlock lanes: a lane's rank among the workgroup's flagged lanes, and the
 *                          workgroup's count -- a ballot and a population count per wavefront, the wavefronts' counts through LDS;
 *   rt_scan_groups_kernel  level 1: workgroup g scans counts[g kScanBlock ..) on its own -- offsets[i] = the sum of the group's
 *                          counts before i -- and writes the group's sum;
 *   rt_scan_total_kernel   level 2: one workgroup walks the groups' sums kScanBlock at a time -- group_base[g] = the sum of the
 *                          groups before g -- and writes the total.
 * A flagged lane of workgroup b then has the place  group_base[b / kScanBlock] + offsets[b] + its rank.  Each kernel's
 * launches are ordered by the stream alone: no look-back, no spin, no cooperative launch.  Counts are 32-bit: a list has fewer
 * than 2^32 entries.  The kernels are templates of a unit's number (RT_INTERNAL_UNIT_*), so that a unit
 * that includes this file for rt_scan_rank alone gets none, and each unit that scans has its own.
 */
#ifndef RT_SCAN_H_
#define RT_SCAN_H_

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kRankBlock = 256;                        /* lanes of a workgroup that ranks its flags */
constexpr int kScanBlock = 1024;                       /* counts a scan step covers: kScanBlock * kRankBlock lanes */

/* the rank of this lane among the workgroup's lanes with f set, lanes in order; *count = how many there are.  wave_count:
 * kRankBlock / 64 words of LDS.  Every lane of the workgroup must call it (it synchronises the workgroup). */
__device__ __forceinline__ uint32_t rt_scan_rank(bool f, uint32_t *wave_count, uint32_t *count) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(f);
    if (lane == 0u) wave_count[w] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)(kRankBlock / 64); ++k) {
        const uint32_t c = wave_count[k];
        before += k < w ? c : 0u;
        all += c;
    }
    *count = all;
    return before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

/* kScanBlock values a step: a wavefront's inclusive scan by lane shifts, the wavefronts' sums through LDS */
__device__ __forceinline__ uint32_t rt_scan_step(uint32_t v, uint32_t *wave_sum, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, (unsigned)d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t k = 0; k < (uint32_t)(kScanBlock / 64); ++k) {
        const uint32_t c = wave_sum[k];
        before += k < w ? c : 0u;
        sum += c;
    }
    __syncthreads();                                    /* (wave_sum is written again by the next step) */
    *all = sum;
    return before + (incl - v);
}

/* the grid is ceil(n_counts / kScanBlock) workgroups of kScanBlock lanes */
template <int kUnit>
__global__ __launch_bounds__(kScanBlock) void rt_scan_groups_kernel(const uint32_t *__restrict__ counts,
                                                                          uint32_t *__restrict__ offsets, uint32_t n_counts,
                                                                          uint32_t *__restrict__ group_sums) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kScanBlock + threadIdx.x;
    uint32_t all = 0;
    const uint32_t at = rt_scan_step(i < n_counts ? counts[i] : 0u, wave_sum, &all);
    if (i < n_counts) offsets[i] = at;
    if (threadIdx.x == 0u) group_sums[blockIdx.x] = all;
}

/* one workgroup of kScanBlock lanes */
template <int kUnit>
__global__ __launch_bounds__(kScanBlock) void rt_scan_total_kernel(const uint32_t *__restrict__ group_sums,
                                                                         uint32_t *__restrict__ group_base, uint32_t n_groups,
                                                                         uint32_t *__restrict__ total) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n_groups; i0 += (uint32_t)kScanBlock) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t all = 0;
        const uint32_t at = rt_scan_step(i < n_groups ? group_sums[i] : 0u, wave_sum, &all);
        if (i < n_groups) group_base[i] = base + at;
        base += all;
    }
    if (threadIdx.x == 0u) *total = base;
}

#endif /* RT_SCAN_H_ */
