// bf_compact.h — the voxel-map and compaction layer of the scene kernels (bf_cloud.hip, bf_tsdf.hip): voxel keys,
// the open-addressing map over them, per-block counters, and the stable compaction (a block's ranks by ballot +
// popcount, the one-block scan of the block counts, the scatter).  bf_track.hip and bf_fern.hip take the block size.
#pragma once
#include "bf_common.h"

#define CLOUD_BLOCK 256
#define CLOUD_WAVES (CLOUD_BLOCK / 64)

typedef unsigned long long u64;

// ---- voxel keys (BF_KEY_BITS, BF_KEY_BIAS, BF_KEY_EMPTY of the public header) ---------------------------------------
#define KEY_FIELD ((1ull << BF_KEY_BITS) - 1ull)

// three whole-number floats are indices a key can hold: inside +-lim
__device__ __forceinline__ bool key_in_range(float x, float y, float z, float lim = (float)BF_KEY_BIAS) {
    return x >= -lim && x < lim && y >= -lim && y < lim && z >= -lim && z < lim;
}

__device__ __forceinline__ u64 key_pack(int x, int y, int z) {
    return ((u64)(x + BF_KEY_BIAS) << (2 * BF_KEY_BITS)) | ((u64)(y + BF_KEY_BIAS) << BF_KEY_BITS) | (u64)(z + BF_KEY_BIAS);
}

// unpacking: the index of axis a (0: x, 1: y, 2: z) of a key
__device__ __forceinline__ int key_axis(u64 key, int a) {
    return (int)((key >> ((2 - a) * BF_KEY_BITS)) & KEY_FIELD) - BF_KEY_BIAS;
}

// key of the voxel at (dx, dy, dz) from `key`, or EMPTY past the index range
__device__ __forceinline__ u64 key_neighbour(u64 key, int dx, int dy, int dz) {
    const int x = key_axis(key, 0) + dx, y = key_axis(key, 1) + dy, z = key_axis(key, 2) + dz, lim = BF_KEY_BIAS;
    if (x < -lim || x >= lim || y < -lim || y >= lim || z < -lim || z >= lim) return BF_KEY_EMPTY;
    return key_pack(x, y, z);
}

// ---- the map: open addressing over slots of STRIDE words, the key first ----------------------------------------------
__device__ __forceinline__ u64 cloud_hash(u64 k) {
    k ^= k >> 30;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27;
    k *= 0x94D049BB133111EBull;
    k ^= k >> 31;
    return k;
}

// the slot of `key` (claimed if new, then *claimed is set), or -1 when neither the key nor an empty slot was found
// in `mask + 1` probes.  Slots never empty again, so a stale read can only show EMPTY where a key now sits, and the
// compare-and-swap that follows decides; nothing here waits for another lane or wave.
template <int STRIDE>
__device__ __forceinline__ long long map_find(u64* table, u64 mask, u64 key, bool* claimed) {
    u64 s = cloud_hash(key) & mask;
    for (u64 i = 0; i <= mask; ++i, s = (s + 1) & mask) {
        u64* kp = table + s * STRIDE;
        u64 k = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == BF_KEY_EMPTY) {
            k = atomicCAS(kp, BF_KEY_EMPTY, key);
            if (k == BF_KEY_EMPTY) {
                *claimed = true;
                return (long long)s;
            }
        }
        if (k == key) return (long long)s;
    }
    return -1;
}

// the slot of `key` in a table (of one-word slots) nobody is writing, or -1
__device__ __forceinline__ int map_lookup(const u64* __restrict__ keys, u64 mask, u64 key) {
    u64 s = cloud_hash(key) & mask;
    for (u64 i = 0; i <= mask; ++i, s = (s + 1) & mask) {
        const u64 k = keys[s];
        if (k == key) return (int)s;
        if (k == BF_KEY_EMPTY) return -1;
    }
    return -1;
}

// ---- per-block counters in LDS (unsigned [BF_STATS_WORDS]): zeroed, one ballot per wave and flag, and one global
// add per block and non-zero counter at the end -------------------------------------------------------------------
__device__ __forceinline__ void stats_begin(unsigned* block_stats) {
    if (threadIdx.x < BF_STATS_WORDS) block_stats[threadIdx.x] = 0;
    __syncthreads();
}

__device__ __forceinline__ void stat_add(unsigned* block_stats, int which, bool flag) {
    const u64 m = __ballot(flag);
    if (m && bf_lane() == 0) atomicAdd(block_stats + which, (unsigned)__popcll(m));
}

__device__ __forceinline__ void stats_flush(unsigned* block_stats, u64* stats) {
    __syncthreads();
    if (threadIdx.x < BF_STATS_WORDS && block_stats[threadIdx.x]) {
        const u64 n = block_stats[threadIdx.x];
        atomicAdd(stats + threadIdx.x, n);
    }
}

// ---- stable compaction ------------------------------------------------------------------------------------------------
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

// Thread t of block b holds one item: it is kept when sel.selected(b, t) and then written by sel.write(b, t, its
// output row).  Sel is a small struct of pointers and sizes passed by value; it says which item (b, t) is.
template <typename Sel>
__global__ void __launch_bounds__(CLOUD_BLOCK) k_compact_count(Sel sel, int* __restrict__ counts) {
    int tot;
    block_rank(sel.selected(blockIdx.x, threadIdx.x), tot);
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// The scatter kernel takes Sel's members one by one (A...) and builds the Sel itself: pointers that are kernel
// arguments can be __restrict__, which those inside a by-value struct cannot, so write()'s stores need not wait for loads.
template <typename T> struct restrict_arg { typedef T type; };
template <typename T> struct restrict_arg<T*> { typedef T* __restrict__ type; };

template <typename Sel, typename... A>
__global__ void __launch_bounds__(CLOUD_BLOCK) k_compact_scatter(const int* __restrict__ prefix,
                                                                 typename restrict_arg<A>::type... a) {
    const Sel sel{a...};
    const bool keep = sel.selected(blockIdx.x, threadIdx.x);
    int tot;
    const int r = block_rank(keep, tot);
    if (keep) sel.write(blockIdx.x, threadIdx.x, (size_t)prefix[blockIdx.x] + r);
}

static inline unsigned compact_blocks(long long items) { return (unsigned)((items + CLOUD_BLOCK - 1) / CLOUD_BLOCK); }

// count, scan, scatter over nb blocks on `st` for Sel{a...}.  block_counts: int32 [nb] scratch; marks int32
// [n_marks + 1]: the first output row of block i * stride for i < n_marks, then the total (k_scan_counts).
template <typename Sel, typename... A>
static void compact(unsigned nb, int* block_counts, int stride, int* marks, int n_marks, hipStream_t st, A... a) {
    hipLaunchKernelGGL(k_compact_count<Sel>, dim3(nb), dim3(CLOUD_BLOCK), 0, st, Sel{a...}, block_counts);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, st, block_counts, (int)nb, stride, marks, n_marks);
    hipLaunchKernelGGL((k_compact_scatter<Sel, A...>), dim3(nb), dim3(CLOUD_BLOCK), 0, st, (const int*)block_counts, a...);
}
