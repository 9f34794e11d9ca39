// bf_objects.hip — objects in the scene: every point of a cloud or vertex of a mesh against every fused box
//   bf_label_points   the box that owns each point (the containing box of the smallest volume), and per box the
//                     points inside it, the points it owns and the extent of those along its own axes
// (include/boxfusion_objects.h states the rule.)  One lane per point; the box index is uniform across a wave, the
// rows come from an LDS chunk.  Per wave and box: a ballot and popcount for the counts, a wave reduction for the
// extents, then at most one integer atomic each.  No floating-point atomics: the outputs are the same bits for any grid and
// any order of arrival.  The file is compiled with contraction off: an expression rounds as it is written.
#include "bf_common.h"

#include "../../include/boxfusion_objects.h"

#include <math.h>

#define OBJ_BLOCK 256
#define OBJ_WAVES (OBJ_BLOCK / 64)
#define OBJ_MAX_BLOCKS 2048    // 8 blocks per CU: a block walks the point tiles blockIdx.x, + gridDim.x, ...
#define OBJ_STATS 5            // members of bf_obj_stat

// the order of the floats as an order of unsigned integers
__device__ __forceinline__ uint32_t obj_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

__device__ __forceinline__ float obj_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float obj_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t obj_wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t obj_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// can box row r (half-lengths already h_k + margin) contain a point of the bounding box lo..hi?  The interval of
// t_k over the bounding box is taken with the test's own operations in the test's own order: p - c, the products and
// the two sums are each monotonic in p, rounding included, so every t_k the test computes for a point of the wave
// lies in [tmin, tmax].  A row with a word that is not finite is left to the test, and so is an interval end that
// came out nan (inf - inf after an overflow): a comparison with nan is false and skips nothing.
__device__ __forceinline__ bool obj_row_may_contain(const float* r, float lox, float loy, float loz, float hix, float hiy,
                                                    float hiz) {
    bool finite = true;
#pragma unroll
    for (int w = 0; w < 15; ++w) finite = finite && isfinite(r[w]);
    if (!finite) return true;
    const float ax = lox - r[0], ay = loy - r[1], az = loz - r[2];
    const float bx = hix - r[0], by = hiy - r[1], bz = hiz - r[2];
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x0 = ax * r[3 + 3 * k], x1 = bx * r[3 + 3 * k];
        const float y0 = ay * r[4 + 3 * k], y1 = by * r[4 + 3 * k];
        const float z0 = az * r[5 + 3 * k], z1 = bz * r[5 + 3 * k];
        const float tmin = (fminf(x0, x1) + fminf(y0, y1)) + fminf(z0, z1);
        const float tmax = (fmaxf(x0, x1) + fmaxf(y0, y1)) + fmaxf(z0, z1);
        const float lim = r[12 + k];
        miss = miss || tmin > lim || tmax < -lim;
    }
    return !miss;
}

template <bool CULL>
__global__ void __launch_bounds__(OBJ_BLOCK) k_label_points(const float* __restrict__ xyz, long long n,
                                                            const float* __restrict__ boxes, int B, float margin,
                                                            int32_t* __restrict__ labels,
                                                            unsigned long long* __restrict__ counts,
                                                            uint32_t* __restrict__ extents,
                                                            unsigned long long* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float sbox[BF_OBJ_CHUNK * BF_OBJ_BOX_WORDS];
    __shared__ unsigned long long sstat[OBJ_WAVES][OBJ_STATS];
    const int lane = bf_lane(), wave = threadIdx.x >> 6;
    const int n_chunks = (B + BF_OBJ_CHUNK - 1) / BF_OBJ_CHUNK;
    const long long n_tiles = (n + OBJ_BLOCK - 1) / OBJ_BLOCK;
    unsigned long long st[OBJ_STATS] = {0, 0, 0, 0, 0};         // the wave's sums, the same in every lane
    bool staged = false;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * OBJ_BLOCK + threadIdx.x;
        const bool live = i < n;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (live) {
            px = xyz[3 * i];
            py = xyz[3 * i + 1];
            pz = xyz[3 * i + 2];
        }
        const bool fin = live && isfinite(px) && isfinite(py) && isfinite(pz);
        const unsigned long long fin_mask = __ballot(fin);
        const int n_fin = __popcll(fin_mask);
        st[BF_OBJ_STAT_POINTS] += __popcll(__ballot(live));
        st[BF_OBJ_STAT_NONFINITE] += __popcll(__ballot(live && !fin));
        float lox = 0.f, loy = 0.f, loz = 0.f, hix = 0.f, hiy = 0.f, hiz = 0.f;
        if (CULL && fin_mask) {                                  // the bounding box of the wave's finite points
            const float inf = __uint_as_float(0x7F800000u);
            lox = obj_wave_min(fin ? px : inf);
            loy = obj_wave_min(fin ? py : inf);
            loz = obj_wave_min(fin ? pz : inf);
            hix = obj_wave_max(fin ? px : -inf);
            hiy = obj_wave_max(fin ? py : -inf);
            hiz = obj_wave_max(fin ? pz : -inf);
        }
        int best = -1, inside = 0;
        float best_vol = 0.f, bt0 = 0.f, bt1 = 0.f, bt2 = 0.f;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int b0 = ch * BF_OBJ_CHUNK;
            const int cnt = B - b0 < BF_OBJ_CHUNK ? B - b0 : BF_OBJ_CHUNK;
            if (n_chunks > 1 || !staged) {                       // a single chunk is staged once per block
                __syncthreads();                                 // the previous chunk has been read
                for (int e = threadIdx.x; e < cnt * BF_OBJ_BOX_WORDS; e += OBJ_BLOCK) {
                    float v = boxes[(size_t)b0 * BF_OBJ_BOX_WORDS + e];
                    const int w = e % BF_OBJ_BOX_WORDS;
                    if (w >= 12 && w < 15) v = v + margin;       // the one add of the rule's right side
                    sbox[e] = v;
                }
                __syncthreads();
                staged = true;
            }
            if (fin_mask == 0) continue;                         // no point of this wave can be inside anything
            for (int g = 0; g < cnt; g += 64) {
                const int gc = cnt - g < 64 ? cnt - g : 64;
                unsigned long long todo = gc == 64 ? ~0ull : (1ull << gc) - 1ull;
                if (CULL) {                                      // lane l judges row g + l for the whole wave
                    const bool keep = lane < gc && obj_row_may_contain(sbox + (g + (lane < gc ? lane : 0)) * BF_OBJ_BOX_WORDS,
                                                                       lox, loy, loz, hix, hiy, hiz);
                    todo = __ballot(keep);
                }
                st[BF_OBJ_STAT_PAIR_TESTS] += (unsigned long long)__popcll(todo) * n_fin;
                while (todo) {
                    const int j = g + __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    const float4* r4 = reinterpret_cast<const float4*>(sbox + j * BF_OBJ_BOX_WORDS);
                    const float4 r0 = r4[0], r1 = r4[1], r2 = r4[2], r3 = r4[3];
                    const float dx = px - r0.x, dy = py - r0.y, dz = pz - r0.z;
                    const float t0 = (dx * r0.w + dy * r1.x) + dz * r1.y;
                    const float t1 = (dx * r1.z + dy * r1.w) + dz * r2.x;
                    const float t2 = (dx * r2.y + dy * r2.z) + dz * r2.w;
                    const bool in = fin && fabsf(t0) <= r3.x && fabsf(t1) <= r3.y && fabsf(t2) <= r3.z;
                    const unsigned long long m = __ballot(in);
                    if (m == 0) continue;
                    if (lane == 0) atomicAdd(counts + (size_t)(b0 + j) * BF_OBJ_COUNT_WORDS, (unsigned long long)__popcll(m));
                    if (in) {
                        ++inside;
                        if (best < 0 || r3.w < best_vol) {       // rows come in index order: equal volumes keep the lower
                            best = b0 + j;
                            best_vol = r3.w;
                            bt0 = t0;
                            bt1 = t1;
                            bt2 = t2;
                        }
                    }
                }
            }
        }
        if (live) labels[i] = best;
        unsigned long long rem = __ballot(best >= 0);
        st[BF_OBJ_STAT_LABELLED] += __popcll(rem);
        st[BF_OBJ_STAT_SHARED] += __popcll(__ballot(inside >= 2));
        // one round per distinct owner among the wave's points
        const uint32_t k0 = obj_key(bt0), k1 = obj_key(bt1), k2 = obj_key(bt2);
        while (rem) {
            const int b = __shfl(best, __ffsll((long long)rem) - 1, 64);
            const bool mine = best == b;
            const unsigned long long m = __ballot(mine);
            rem &= ~m;
            const uint32_t mn0 = obj_wave_min_u32(mine ? k0 : 0xFFFFFFFFu), mx0 = obj_wave_max_u32(mine ? k0 : 0u);
            const uint32_t mn1 = obj_wave_min_u32(mine ? k1 : 0xFFFFFFFFu), mx1 = obj_wave_max_u32(mine ? k1 : 0u);
            const uint32_t mn2 = obj_wave_min_u32(mine ? k2 : 0xFFFFFFFFu), mx2 = obj_wave_max_u32(mine ? k2 : 0u);
            if (lane == 0) atomicAdd(counts + (size_t)b * BF_OBJ_COUNT_WORDS + 1, (unsigned long long)__popcll(m));
            // lane l < 6 holds extent word l.  A stored word that the wave's value would not move is left alone:
            // the words only fall (min) or rise (max), so a stale read can only cost an atomic that changes nothing,
            // and the waves in the middle of an object, most of them, add no traffic to its row
            if (lane < BF_OBJ_EXTENT_WORDS) {
                uint32_t* e = extents + (size_t)b * BF_OBJ_EXTENT_WORDS + lane;
                const uint32_t v = lane == 0 ? mn0 : lane == 1 ? mx0 : lane == 2 ? mn1 : lane == 3 ? mx1 : lane == 4 ? mn2 : mx2;
                const uint32_t seen = *(const volatile uint32_t*)e;
                if (lane & 1) {
                    if (v > seen) atomicMax(e, v);
                } else {
                    if (v < seen) atomicMin(e, v);
                }
            }
        }
    }
    if (lane == 0)
        for (int s = 0; s < OBJ_STATS; ++s) sstat[wave][s] = st[s];
    __syncthreads();
    if (threadIdx.x < OBJ_STATS) {
        unsigned long long sum = 0;
        for (int w = 0; w < OBJ_WAVES; ++w) sum += sstat[w][threadIdx.x];
        if (sum) atomicAdd(stats + threadIdx.x, sum);
    }
}

static int obj_label_points(const float* xyz, long long n, const float* boxes, int B, float margin, int32_t* labels,
                            void* counts, void* extents, void* stats, int cull, void* stream) {
    if (n < 0 || B < 0 || B > BF_MAX_BOXES) return BF_ERR_ARG;
    if (n == 0) return BF_OK;
    if (!xyz || !labels || !stats) return BF_ERR_ARG;
    if (B > 0 && (!boxes || !counts || !extents)) return BF_ERR_ARG;
    const long long tiles = (n + OBJ_BLOCK - 1) / OBJ_BLOCK;
    const unsigned grid = (unsigned)(tiles < OBJ_MAX_BLOCKS ? tiles : OBJ_MAX_BLOCKS);
    if (cull)
        hipLaunchKernelGGL(k_label_points<true>, dim3(grid), dim3(OBJ_BLOCK), 0, bf_stream(stream), xyz, n, boxes, B, margin,
                           labels, (unsigned long long*)counts, (uint32_t*)extents, (unsigned long long*)stats);
    else
        hipLaunchKernelGGL(k_label_points<false>, dim3(grid), dim3(OBJ_BLOCK), 0, bf_stream(stream), xyz, n, boxes, B, margin,
                           labels, (unsigned long long*)counts, (uint32_t*)extents, (unsigned long long*)stats);
    return bf_check_launch();
}

BF_API int bf_label_points(const float* xyz, long long n, const float* boxes, int B, float margin, int32_t* labels,
                           void* counts, void* extents, void* stats, void* stream) {
    return obj_label_points(xyz, n, boxes, B, margin, labels, counts, extents, stats, 1, stream);
}

BF_API int bf_label_points_ex(const float* xyz, long long n, const float* boxes, int B, float margin, int32_t* labels,
                              void* counts, void* extents, void* stats, int cull, void* stream) {
    return obj_label_points(xyz, n, boxes, B, margin, labels, counts, extents, stats, cull != 0, stream);
}
