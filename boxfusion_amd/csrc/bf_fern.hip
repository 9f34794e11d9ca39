// bf_fern.hip — keyframe relocalisation with randomised ferns (Glocker et al.): a frame as a short binary code, the
// keyframe table searched by code distance, and the harvest that fills the table.
//   bf_fern_table_check  a host fern table against the cell grid
//   bf_fern_encode       the codes of B frames (and, on request, every cell's means)
//   bf_fern_search       the k nearest keyframes of Q codes (and, on request, the whole distance rows)
//   bf_fern_append       the code joins the table when it is far enough from its nearest keyframe
// Everything is integer arithmetic on integer sums, so any order of the additions gives the same bits as the numpy
// restatement in tests/fern_ref.py.  wave64 throughout; sums and minima by the butterfly of bf_track.hip (xor 32 ..
// 1: every lane ends with the result); no atomics.  The tracker restarts from the candidates' poses
// (boxfusion_amd/tracking.py, Relocaliser).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_fern_means    VGPR 29  SGPR 30  LDS    0 B  scratch 0 B
//   k_fern_codes    VGPR 30  SGPR 35  LDS   32 B  scratch 0 B
//   k_fern_nearest  VGPR 24  SGPR 32  LDS  256 B  scratch 0 B
//   k_fern_topk     VGPR 24  SGPR 31  LDS  256 B  scratch 0 B
//   k_fern_append   VGPR 18  SGPR 32  LDS    0 B  scratch 0 B
#include "bf_compact.h"

#define FERN_WORD 8                      // ferns per code word: a nibble each
#define FERN_NONE 0x7fffffffffffffffll   // no candidate: above every (distance << 32 | index)

// ---- cell means ------------------------------------------------------------------------------------------------------
// One wave per cell.  The cell's n = c * c pixels go round the lanes: four along a row per lane and step where the
// rows can be read as vectors (c and W multiples of 4: a float4 of depth and three words of colour, both aligned),
// one per lane and step otherwise.  R, G, B <= 255 n, millimetres <= 65535 n, n <= 4096: every sum fits 32 bits.
struct FernMeans {
    int r, g, b, d;
};

__device__ __forceinline__ void fern_pixel(float d, float max_depth, int& sd, int& m) {
    if (d > 0.f && d < max_depth) {      // NaN fails
        sd += __float2int_rn(d * 1000.0f);
        m += 1;
    }
}

// every lane of the wave must call; the result is in every lane
__device__ __forceinline__ FernMeans fern_cell_means(const float* __restrict__ depth, const uint8_t* __restrict__ rgb, int W,
                                                     int c, int y0, int x0, float max_depth, bool vec) {
    int sr = 0, sg = 0, sb = 0, sd = 0, m = 0;
    const int n = c * c;
    if (vec) {
        const int qr = c >> 2;           // quads per row of the cell
        for (int q = bf_lane(); q < qr * c; q += 64) {
            const int row = q / qr, col = (q - row * qr) << 2;
            const size_t p = (size_t)(y0 + row) * W + (size_t)(x0 + col);
            const float4 v = *reinterpret_cast<const float4*>(depth + p);
            fern_pixel(v.x, max_depth, sd, m);
            fern_pixel(v.y, max_depth, sd, m);
            fern_pixel(v.z, max_depth, sd, m);
            fern_pixel(v.w, max_depth, sd, m);
            if (rgb) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(rgb + p * 3);
                const uint32_t a = w[0], b = w[1], e = w[2];     // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
                sr += (int)(a & 255u) + (int)(a >> 24) + (int)((b >> 16) & 255u) + (int)((e >> 8) & 255u);
                sg += (int)((a >> 8) & 255u) + (int)(b & 255u) + (int)(b >> 24) + (int)((e >> 16) & 255u);
                sb += (int)((a >> 16) & 255u) + (int)((b >> 8) & 255u) + (int)(e & 255u) + (int)(e >> 24);
            }
        }
    } else {
        for (int q = bf_lane(); q < n; q += 64) {
            const int row = q / c, col = q - row * c;
            const size_t p = (size_t)(y0 + row) * W + (size_t)(x0 + col);
            fern_pixel(depth[p], max_depth, sd, m);
            if (rgb) {
                sr += rgb[p * 3];
                sg += rgb[p * 3 + 1];
                sb += rgb[p * 3 + 2];
            }
        }
    }
    sd = bf_wave_sum_i32(sd);
    m = bf_wave_sum_i32(m);
    FernMeans out = {0, 0, 0, -1};
    if (rgb) {
        out.r = (2 * bf_wave_sum_i32(sr) + n) / (2 * n);
        out.g = (2 * bf_wave_sum_i32(sg) + n) / (2 * n);
        out.b = (2 * bf_wave_sum_i32(sb) + n) / (2 * n);
    }
    if (m > 0 && 2 * m >= n) out.d = (2 * sd + m) / (2 * m);
    return out;
}

// grid (ceil(cells / 4), B): wave w of block x owns cell 4 x + w
__global__ void __launch_bounds__(CLOUD_BLOCK) k_fern_means(const float* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                            int H, int W, int c, int Wc, int cells, float max_depth, int vec,
                                                            int* __restrict__ means) {
    const int cell = blockIdx.x * CLOUD_WAVES + (threadIdx.x >> 6);
    if (cell >= cells) return;                                   // the whole wave leaves
    const size_t frame = (size_t)blockIdx.y * H * W;
    const int cy = cell / Wc, cx = cell - cy * Wc;
    const FernMeans v = fern_cell_means(depth + frame, rgb ? rgb + frame * 3 : nullptr, W, c, cy * c, cx * c, max_depth, vec != 0);
    if (bf_lane() == 0) {
        int* o = means + ((size_t)blockIdx.y * cells + cell) * 4;
        o[0] = v.r;
        o[1] = v.g;
        o[2] = v.b;
        o[3] = v.d;
    }
}

// ---- codes -----------------------------------------------------------------------------------------------------------
// grid (F / 8, B), 512 threads: wave w of block x owns fern 8 x + w, forms the means of that fern's cell itself (only
// the cells the ferns look at are read: at most F c^2 pixels of a frame) and its nibble; thread 0 packs the block's
// eight nibbles into code word x.  A cell index outside the grid gives nibble 0 and touches no pixel
// (bf_fern_table_check refuses such a table on the host).
__global__ void __launch_bounds__(64 * FERN_WORD) k_fern_codes(const float* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                               int H, int W, int c, int Wc, int cells, float max_depth, int vec,
                                                               const int* __restrict__ ferns, int words,
                                                               uint32_t* __restrict__ codes) {
    __shared__ uint32_t nib[FERN_WORD];
    const int w = threadIdx.x >> 6;
    const int* f = ferns + ((size_t)blockIdx.x * FERN_WORD + w) * 5;
    const int cell = f[0];
    uint32_t bits = 0;
    if (cell >= 0 && cell < cells) {                             // uniform over the wave
        const size_t frame = (size_t)blockIdx.y * H * W;
        const int cy = cell / Wc, cx = cell - cy * Wc;
        const FernMeans v =
            fern_cell_means(depth + frame, rgb ? rgb + frame * 3 : nullptr, W, c, cy * c, cx * c, max_depth, vec != 0);
        bits = (v.r > f[1] ? 1u : 0u) | (v.g > f[2] ? 2u : 0u) | (v.b > f[3] ? 4u : 0u) | (v.d >= 0 && v.d > f[4] ? 8u : 0u);
    }
    if (bf_lane() == 0) nib[w] = bits << (4 * w);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < FERN_WORD; ++i) word |= nib[i];
        codes[(size_t)blockIdx.y * words + blockIdx.x] = word;
    }
}

BF_API int bf_fern_table_check(const int32_t* ferns_host, int F, int cells) {
    if (!ferns_host || F <= 0 || F % FERN_WORD || cells <= 0) return BF_ERR_ARG;
    for (int f = 0; f < F; ++f)
        if (ferns_host[(size_t)f * 5] < 0 || ferns_host[(size_t)f * 5] >= cells) return BF_ERR_ARG;
    return BF_OK;
}

BF_API int bf_fern_encode(const float* depth, const uint8_t* rgb, int B, int H, int W, int cell, float max_depth,
                          const int32_t* ferns, int F, int32_t* means, uint32_t* codes, void* stream) {
    if (!depth || B <= 0 || H <= 0 || W <= 0 || cell < 1 || cell > BF_FERN_CELL_MAX || !(max_depth > 0.f) ||
        !(max_depth <= 65.535f) || (!means && !codes))
        return BF_ERR_ARG;
    if (codes && (!ferns || F <= 0 || F % FERN_WORD)) return BF_ERR_ARG;
    const int Hc = H / cell, Wc = W / cell;
    if (Hc < 1 || Wc < 1) return BF_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) / 3 || B > 65535 || (codes && F / FERN_WORD >= (1 << 30))) return BF_ERR_CAPACITY;
    const int cells = Hc * Wc;
    // rows as vectors: every quad starts at a pixel index that is a multiple of 4 from an aligned base
    const int vec = cell % 4 == 0 && W % 4 == 0 && ((uintptr_t)depth & 15) == 0 && ((uintptr_t)rgb & 3) == 0;
    hipStream_t st = bf_stream(stream);
    if (means)
        hipLaunchKernelGGL(k_fern_means, dim3((unsigned)((cells + CLOUD_WAVES - 1) / CLOUD_WAVES), (unsigned)B), dim3(CLOUD_BLOCK),
                           0, st, depth, rgb, H, W, cell, Wc, cells, max_depth, vec, means);
    if (codes)
        hipLaunchKernelGGL(k_fern_codes, dim3((unsigned)(F / FERN_WORD), (unsigned)B), dim3(64 * FERN_WORD), 0, st, depth, rgb, H,
                           W, cell, Wc, cells, max_depth, vec, ferns, F / FERN_WORD, codes);
    return bf_check_launch();
}

// ---- distance and search ---------------------------------------------------------------------------------------------
// distance = the number of ferns whose nibbles differ: per word x = a ^ b, every nibble of x folded onto its lowest bit.
__device__ __forceinline__ int fern_word_distance(uint32_t a, uint32_t b) {
    const uint32_t x = a ^ b;
    return __popc((x | x >> 1 | x >> 2 | x >> 3) & 0x11111111u);
}

__device__ __forceinline__ long long fern_wave_min(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// the block's smallest key above `prev` (FERN_NONE when there is none), in every thread; slot: this round's LDS row
__device__ __forceinline__ long long fern_block_min_above(long long key, long long prev, long long* slot) {
    const long long m = fern_wave_min(key > prev ? key : FERN_NONE);
    if (bf_lane() == 0) slot[threadIdx.x >> 6] = m;
    __syncthreads();
    long long out = slot[0];
#pragma unroll
    for (int w = 1; w < CLOUD_WAVES; ++w) out = slot[w] < out ? slot[w] : out;
    return out;
}

// grid (ceil(n_upper / 256), Q): thread t of block x owns keyframe 256 x + t, key = distance << 32 | index (unique, so
// "the smallest key above the last one" walks the order by distance, then index, without marking anything); the block's
// k smallest go to part [Q, blocks, k]
__global__ void __launch_bounds__(CLOUD_BLOCK) k_fern_nearest(const uint32_t* __restrict__ table, int capacity, int words,
                                                              const int* __restrict__ n_dev, int n_upper,
                                                              const uint32_t* __restrict__ queries, int k,
                                                              long long* __restrict__ part, int* __restrict__ rows) {
    __shared__ long long slot[BF_FERN_K_MAX][CLOUD_WAVES];
    int n = *n_dev;
    n = n < 0 ? 0 : (n > n_upper ? n_upper : n);
    n = n > capacity ? capacity : n;
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const uint32_t* q = queries + (size_t)blockIdx.y * words;
    long long key = FERN_NONE;
    if (i < n) {
        const uint32_t* row = table + (size_t)i * words;
        int d = 0;
        for (int w = 0; w < words; ++w) d += fern_word_distance(row[w], q[w]);
        key = (long long)d << 32 | (long long)i;
    }
    if (rows && i < n_upper) rows[(size_t)blockIdx.y * n_upper + i] = i < n ? (int)(key >> 32) : -1;
    long long prev = -1;
    for (int r = 0; r < k; ++r) {
        prev = fern_block_min_above(key, prev, slot[r]);
        if (threadIdx.x == 0) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * k + r] = prev;
    }
}

// grid Q: the k smallest of a query's blocks * k candidates the same way -> top i32 [Q, k, 2] (distance, index)
__global__ void __launch_bounds__(CLOUD_BLOCK) k_fern_topk(const long long* __restrict__ part, int candidates, int k,
                                                           int* __restrict__ top) {
    __shared__ long long slot[BF_FERN_K_MAX][CLOUD_WAVES];
    const long long* mine = part + (size_t)blockIdx.x * candidates;
    long long prev = -1;
    for (int r = 0; r < k; ++r) {
        long long best = FERN_NONE;
        for (int j = threadIdx.x; j < candidates; j += CLOUD_BLOCK) {
            const long long c = mine[j];
            best = c > prev && c < best ? c : best;
        }
        prev = fern_block_min_above(best, prev, slot[r]);
        if (threadIdx.x == 0) {
            int* o = top + ((size_t)blockIdx.x * k + r) * 2;
            o[0] = prev == FERN_NONE ? -1 : (int)(prev >> 32);
            o[1] = prev == FERN_NONE ? -1 : (int)(prev & 0xffffffffll);
        }
    }
}

BF_API int bf_fern_search_blocks(int n_upper) { return n_upper <= 0 ? 0 : (n_upper + CLOUD_BLOCK - 1) / CLOUD_BLOCK; }

BF_API int bf_fern_search(const uint32_t* table, int capacity, int F, const int32_t* n, int n_upper, const uint32_t* queries,
                          int Q, int k, long long* part, int32_t* top, int32_t* rows, void* stream) {
    if (!table || !n || !queries || !part || !top || capacity <= 0 || F <= 0 || F % FERN_WORD || n_upper <= 0 ||
        n_upper > capacity || Q <= 0 || k < 1 || k > BF_FERN_K_MAX)
        return BF_ERR_ARG;
    const int blocks = bf_fern_search_blocks(n_upper);
    if (Q > 65535 || (long long)blocks * k >= (1ll << 31) || (long long)Q * n_upper >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipStream_t st = bf_stream(stream);
    hipLaunchKernelGGL(k_fern_nearest, dim3((unsigned)blocks, (unsigned)Q), dim3(CLOUD_BLOCK), 0, st, table, capacity,
                       F / FERN_WORD, n, n_upper, queries, k, part, rows);
    hipLaunchKernelGGL(k_fern_topk, dim3((unsigned)Q), dim3(CLOUD_BLOCK), 0, st, (const long long*)part, blocks * k, k, top);
    return bf_check_launch();
}

// ---- conditional append ----------------------------------------------------------------------------------------------
// One wave.  best: the (distance, index) pair bf_fern_search wrote for this code with k >= 1, still on the device.
struct FernPose {
    float m[16];
};

__global__ void __launch_bounds__(64) k_fern_append(uint32_t* __restrict__ table, int capacity, int words, int* __restrict__ n_dev,
                                                    const uint32_t* __restrict__ code, const int* __restrict__ best,
                                                    int threshold, FernPose pose, int frame, float* __restrict__ poses,
                                                    int* __restrict__ ids, int* __restrict__ counters) {
    const int n = *n_dev;                                        // every lane reads it before lane 0 writes it below
    const bool add = n <= 0 || best[0] > threshold;
    const bool full = n >= capacity;
    if (add && !full) {
        const int at = n < 0 ? 0 : n;
        for (int w = threadIdx.x; w < words; w += 64) table[(size_t)at * words + w] = code[w];
        if (threadIdx.x < 16) poses[(size_t)at * 16 + threadIdx.x] = pose.m[threadIdx.x];
        if (threadIdx.x == 0) {
            ids[at] = frame;
            *n_dev = at + 1;
        }
    }
    if (threadIdx.x == 0) {
        counters[BF_FERN_COUNT_OBSERVED] += 1;
        if (add && !full) counters[BF_FERN_COUNT_ADDED] += 1;
        if (add && full) counters[BF_FERN_COUNT_DROPPED_FULL] += 1;
    }
}

BF_API int bf_fern_append(uint32_t* table, int capacity, int F, int32_t* n, const uint32_t* code, const int32_t* best,
                          int threshold, const float* pose_host, int frame, float* poses, int32_t* ids, int32_t* counters,
                          void* stream) {
    if (!table || !n || !code || !best || !pose_host || !poses || !ids || !counters || capacity <= 0 || F <= 0 ||
        F % FERN_WORD || threshold < 0)
        return BF_ERR_ARG;
    FernPose P;
    for (int i = 0; i < 16; ++i) P.m[i] = pose_host[i];
    hipLaunchKernelGGL(k_fern_append, dim3(1), dim3(64), 0, bf_stream(stream), table, capacity, F / FERN_WORD, n, code, best,
                       threshold, P, frame, poses, ids, counters);
    return bf_check_launch();
}
