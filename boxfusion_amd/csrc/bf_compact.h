// bf_compact.h — what the hash-map kernels share (bf_cloud.hip, bf_tsdf.hip): the key hash and the stable
// compaction pieces (a block's ranks by ballot + popcount, and the one-block scan of the block counts)
#pragma once
#include "bf_common.h"

#define CLOUD_BLOCK 256
#define CLOUD_WAVES (CLOUD_BLOCK / 64)

__device__ __forceinline__ unsigned long long cloud_hash(unsigned long long k) {
    k ^= k >> 30;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27;
    k *= 0x94D049BB133111EBull;
    k ^= k >> 31;
    return k;
}

// position of this thread's item among the block's selected items, and the block's total (in every thread);
// for blocks of CLOUD_BLOCK threads
__device__ __forceinline__ int block_rank(bool sel, int& block_total) {
    __shared__ int wave_n[CLOUD_WAVES];
    const unsigned long long m = __ballot(sel);
    const int w = threadIdx.x >> 6;
    if (bf_lane() == 0) wave_n[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < CLOUD_WAVES; ++i) {
        const int n = wave_n[i];
        base += i < w ? n : 0;
        tot += n;
    }
    block_total = tot;
    return base + bf_lanes_below(m);
}

// counts [nb] -> exclusive prefix in place; marks[i] = prefix[i * stride] for i < n_marks, marks[n_marks] = total.
// One block of 1024 threads; each thread owns a contiguous chunk of the counts.
static __global__ void __launch_bounds__(1024) k_scan_counts(int* __restrict__ counts, int nb, int stride,
                                                             int* __restrict__ marks, int n_marks) {
    __shared__ int wave_sum[16];
    const int t = threadIdx.x;
    const int chunk = (nb + 1023) / 1024;
    const int lo = t * chunk < nb ? t * chunk : nb;
    const int hi = lo + chunk < nb ? lo + chunk : nb;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    // inclusive scan of s over the wave, then over the 16 waves
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (bf_lane() >= o) inc += v;
    }
    if (bf_lane() == 63) wave_sum[t >> 6] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = wave_sum[i];
        base += i < (t >> 6) ? n : 0;
        total += n;
    }
    int run = base + inc - s;
    for (int i = lo; i < hi; ++i) {
        const int c = counts[i];
        counts[i] = run;
        if (stride > 0 && i % stride == 0 && i / stride < n_marks) marks[i / stride] = run;
        run += c;
    }
    if (t == 0) marks[n_marks] = total;
}
