// bf_level.hip — levelling a scene: which way is up, where the floor lies, how the walls run
//   bf_level_face_samples   a centroid, a unit normal and an integer weight (the area) per face of a mesh
//   bf_level_vote           the normals into a cube-map histogram of their directions
//   bf_level_score          for candidate axes, the weight parallel and the weight perpendicular to each
//   bf_level_refine         for one axis: the second moments of the parallel and the perpendicular normals, the
//                           four-fold yaw sums of the perpendicular ones and a histogram of the upward samples' heights
// (include/boxfusion_level.h states the rules.)  One lane per face or sample, a block walks the tiles blockIdx.x,
// + gridDim.x, ...  Histograms are private to a block in LDS and reach global memory once per block; sums are kept per
// lane, reduced per wave with shuffles and per block through LDS, then one integer atomic per word and block.  No
// floating-point atomics: the outputs are the same bits for any grid and any order of the samples.  The file is
// compiled with contraction off: an expression rounds as it is written.
#include "bf_common.h"

#include "../../include/boxfusion_level.h"

#include <math.h>

#define LV_BLOCK 256
#define LV_WAVES (LV_BLOCK / 64)
#define LV_MAX_BLOCKS 1024     // 4 blocks per CU
#define LV_VOTE_ROUNDS 4       // distinct bins a wave sums with shuffles before its lanes go to LDS one by one
// a block's uint32 vote table is emptied into global memory after this many tiles: 256 tiles of 256 lanes of less
// than 2^16 each stay below 2^32 (256 * 256 * 65535 = 4 294 901 760); larger weights go to global memory directly
#define LV_VOTE_FLUSH 256
#define LV_SMALL_WEIGHT 65536u

typedef unsigned long long u64;

__device__ __forceinline__ float lv_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ uint32_t lv_wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// the wave's sums st[0..N) (the same in every lane) -> stats, through LDS: one atomic per word and block
template <int N>
__device__ __forceinline__ void lv_block_add(const u64* st, u64 (*sh)[N], u64* out, int base) {
    const int lane = bf_lane(), wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int s = 0; s < N; ++s) sh[wave][s] = st[s];
    __syncthreads();
    if (threadIdx.x < N) {
        u64 sum = 0;
        for (int w = 0; w < LV_WAVES; ++w) sum += sh[w][threadIdx.x];
        if (sum) atomicAdd(out + base + threadIdx.x, sum);
    }
}

static unsigned lv_grid(long long n) {
    const long long tiles = (n + LV_BLOCK - 1) / LV_BLOCK;
    return (unsigned)(tiles < LV_MAX_BLOCKS ? tiles : LV_MAX_BLOCKS);
}

// ---- face samples ---------------------------------------------------------------------------------------
#define LV_FACE_STATS 5        // BF_LEVEL_STAT_FACES .. BF_LEVEL_STAT_FACE_SATURATED

__global__ void __launch_bounds__(LV_BLOCK) k_level_face_samples(const float* __restrict__ vertices, long long nv,
                                                                 const int32_t* __restrict__ faces, long long m,
                                                                 float area_unit, float* __restrict__ centroids,
                                                                 float* __restrict__ normals,
                                                                 uint32_t* __restrict__ weights, u64* __restrict__ stats) {
    __shared__ u64 sstat[LV_WAVES][LV_FACE_STATS];
    u64 st[LV_FACE_STATS] = {0, 0, 0, 0, 0};
    const long long n_tiles = (m + LV_BLOCK - 1) / LV_BLOCK;
    const float nan = __uint_as_float(0x7FC00000u);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * LV_BLOCK + threadIdx.x;
        const bool live = i < m;
        bool bad_index = false, nonfinite = false, zero = false, capped = false;
        float cx = nan, cy = nan, cz = nan, nx = nan, ny = nan, nz = nan;
        uint32_t w = 0;
        if (live) {
            const long long ia = faces[3 * i], ib = faces[3 * i + 1], ic = faces[3 * i + 2];
            bad_index = ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv;
            if (!bad_index) {
                const float ax = vertices[3 * ia], ay = vertices[3 * ia + 1], az = vertices[3 * ia + 2];
                const float bx = vertices[3 * ib], by = vertices[3 * ib + 1], bz = vertices[3 * ib + 2];
                const float qx = vertices[3 * ic], qy = vertices[3 * ic + 1], qz = vertices[3 * ic + 2];
                const float ex = bx - ax, ey = by - ay, ez = bz - az;
                const float fx = qx - ax, fy = qy - ay, fz = qz - az;
                const float xx = ey * fz - ez * fy, xy = ez * fx - ex * fz, xz = ex * fy - ey * fx;
                const float len = sqrtf((xx * xx + xy * xy) + xz * xz);
                nonfinite = !(isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) &&
                              isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(len));
                zero = !nonfinite && len == 0.f;
                if (!nonfinite && !zero) {
                    nx = xx / len;
                    ny = xy / len;
                    nz = xz / len;
                    cx = ((ax + bx) + qx) / 3.0f;
                    cy = ((ay + by) + qy) / 3.0f;
                    cz = ((az + bz) + qz) / 3.0f;
                    const float r = rintf((0.5f * len) / area_unit);       // >= 0, or +inf
                    capped = r > (float)BF_LEVEL_WEIGHT_CAP;
                    w = capped ? (uint32_t)BF_LEVEL_WEIGHT_CAP : (uint32_t)r;
                }
            }
            centroids[3 * i] = cx;
            centroids[3 * i + 1] = cy;
            centroids[3 * i + 2] = cz;
            normals[3 * i] = nx;
            normals[3 * i + 1] = ny;
            normals[3 * i + 2] = nz;
            weights[i] = w;
        }
        st[BF_LEVEL_STAT_FACES] += __popcll(__ballot(live));
        st[BF_LEVEL_STAT_FACE_BAD_INDEX] += __popcll(__ballot(bad_index));
        st[BF_LEVEL_STAT_FACE_NONFINITE] += __popcll(__ballot(nonfinite));
        st[BF_LEVEL_STAT_FACE_ZERO_AREA] += __popcll(__ballot(zero));
        st[BF_LEVEL_STAT_FACE_SATURATED] += __popcll(__ballot(capped));
    }
    lv_block_add<LV_FACE_STATS>(st, sstat, stats, BF_LEVEL_STAT_FACES);
}

BF_API int bf_level_face_samples(const float* vertices, long long n_vertices, const int32_t* faces, long long m,
                                 float area_unit, float* centroids, float* normals, uint32_t* weights, void* stats,
                                 void* stream) {
    if (m < 0 || n_vertices < 0 || !(area_unit > 0.f) || !isfinite(area_unit)) return BF_ERR_ARG;
    if (m == 0) return BF_OK;
    if (!faces || !centroids || !normals || !weights || !stats || (n_vertices > 0 && !vertices)) return BF_ERR_ARG;
    hipLaunchKernelGGL(k_level_face_samples, dim3(lv_grid(m)), dim3(LV_BLOCK), 0, bf_stream(stream), vertices, n_vertices,
                       faces, m, area_unit, centroids, normals, weights, (u64*)stats);
    return bf_check_launch();
}

// ---- vote -----------------------------------------------------------------------------------------------
#define LV_VOTE_STATS 3        // BF_LEVEL_STAT_VOTE_SAMPLES .. BF_LEVEL_STAT_VOTE_WEIGHT

// the bin of a direction with finite components that are not all 0
__device__ __forceinline__ int lv_bin(float x, float y, float z, int G) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const int k = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float major = k == 0 ? x : (k == 1 ? y : z);
    const float p = k == 0 ? y : x, q = k == 2 ? y : z;
    const float u = p / major, v = q / major;
    const float half = 0.5f * (float)G;
    int iu = (int)floorf((u + 1.0f) * half), iv = (int)floorf((v + 1.0f) * half);
    iu = iu > G - 1 ? G - 1 : iu;
    iv = iv > G - 1 ? G - 1 : iv;
    const int face = 2 * k + (major < 0.f ? 1 : 0);
    return (face * G + iv) * G + iu;
}

__device__ __forceinline__ void lv_vote_flush(uint32_t* table, int bins, u64* hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += LV_BLOCK) {
        const uint32_t v = table[b];
        if (v) {
            atomicAdd(hist + b, (u64)v);
            table[b] = 0;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(LV_BLOCK) k_level_vote(const float* __restrict__ normals, const uint32_t* __restrict__ weights,
                                                         long long n, int G, u64* __restrict__ hist, u64* __restrict__ stats) {
    __shared__ uint32_t table[6 * BF_LEVEL_MAX_G * BF_LEVEL_MAX_G];
    __shared__ u64 sstat[LV_WAVES][LV_VOTE_STATS];
    const int lane = bf_lane();
    const int bins = 6 * G * G;
    for (int b = threadIdx.x; b < bins; b += LV_BLOCK) table[b] = 0;
    __syncthreads();
    u64 st[LV_VOTE_STATS] = {0, 0, 0};
    const long long n_tiles = (n + LV_BLOCK - 1) / LV_BLOCK;
    int since_flush = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (since_flush == LV_VOTE_FLUSH) {                      // uniform over the block
            lv_vote_flush(table, bins, hist);
            since_flush = 0;
        }
        ++since_flush;
        const long long i = tile * LV_BLOCK + threadIdx.x;
        const bool live = i < n;
        float x = 0.f, y = 0.f, z = 0.f;
        uint32_t w = 0;
        if (live) {
            x = normals[3 * i];
            y = normals[3 * i + 1];
            z = normals[3 * i + 2];
            w = weights[i];
        }
        const bool use = live && w != 0 && isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.f && y == 0.f && z == 0.f);
        st[0] += __popcll(__ballot(live));
        st[1] += __popcll(__ballot(live && !use));
        const int bin = use ? lv_bin(x, y, z, G) : -1;
        const bool big = use && w >= LV_SMALL_WEIGHT;
        if (big) atomicAdd(hist + bin, (u64)w);
        st[2] += bf_wave_sum_i64(use ? (long long)w : 0ll);
        // a room's normals fall into a few bins: the wave sums those with shuffles, one LDS atomic each
        u64 rem = __ballot(use && !big);
        for (int round = 0; round < LV_VOTE_ROUNDS && rem; ++round) {
            const int b = __shfl(bin, __ffsll((long long)rem) - 1, 64);
            const bool mine = (rem >> lane & 1ull) && bin == b;
            rem &= ~__ballot(mine);
            const uint32_t sum = lv_wave_sum_u32(mine ? w : 0u);
            if (lane == 0) atomicAdd(table + b, sum);
        }
        if (rem >> lane & 1ull) atomicAdd(table + bin, w);
    }
    lv_vote_flush(table, bins, hist);
    lv_block_add<LV_VOTE_STATS>(st, sstat, stats, BF_LEVEL_STAT_VOTE_SAMPLES);
}

BF_API int bf_level_vote(const float* normals, const uint32_t* weights, long long n, int G, void* hist, void* stats,
                         void* stream) {
    if (n < 0 || G < 1 || G > BF_LEVEL_MAX_G) return BF_ERR_ARG;
    if (n == 0) return BF_OK;
    if (!normals || !weights || !hist || !stats) return BF_ERR_ARG;
    hipLaunchKernelGGL(k_level_vote, dim3(lv_grid(n)), dim3(LV_BLOCK), 0, bf_stream(stream), normals, weights, n, G,
                       (u64*)hist, (u64*)stats);
    return bf_check_launch();
}

// ---- score ----------------------------------------------------------------------------------------------
// the centre direction of a bin (the header's rule); bin in 0 .. 6 G G - 1
__device__ __forceinline__ void lv_centre(int bin, int G, float* dx, float* dy, float* dz) {
    const int iu = bin % G, iv = (bin / G) % G, face = bin / (G * G);
    const int k = face >> 1;
    const float s = (face & 1) ? -1.0f : 1.0f;
    const float u = (float)(2 * iu + 1 - G) / (float)G, v = (float)(2 * iv + 1 - G) / (float)G;
    const float len = sqrtf((u * u + v * v) + 1.0f);
    const float dk = s / len, dp = (u * s) / len, dq = (v * s) / len;
    *dx = k == 0 ? dk : dp;
    *dy = k == 0 ? dp : (k == 1 ? dk : dq);
    *dz = k == 2 ? dk : dq;
}

__global__ void __launch_bounds__(LV_BLOCK) k_level_score(const u64* __restrict__ hist, int G,
                                                          const int32_t* __restrict__ candidates, float cos_par,
                                                          float sin_perp, u64* __restrict__ scores) {
    __shared__ u64 spart[LV_WAVES][2];
    const int lane = bf_lane(), wave = threadIdx.x >> 6;
    const int bins = 6 * G * G;
    const int cand = candidates[blockIdx.x];
    u64 par = 0, perp = 0;
    if (cand >= 0 && cand < bins) {                              // uniform over the block
        float cx, cy, cz;
        lv_centre(cand, G, &cx, &cy, &cz);
        for (int b = threadIdx.x; b < bins; b += LV_BLOCK) {
            const u64 h = hist[b];
            if (h == 0) continue;
            float dx, dy, dz;
            lv_centre(b, G, &dx, &dy, &dz);
            const float a = fabsf(lv_dot(cx, cy, cz, dx, dy, dz));
            if (a >= cos_par) par += h;
            if (a <= sin_perp) perp += h;
        }
    }
    par = (u64)bf_wave_sum_i64((long long)par);
    perp = (u64)bf_wave_sum_i64((long long)perp);
    if (lane == 0) {
        spart[wave][0] = par;
        spart[wave][1] = perp;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 sum = 0;
        for (int w = 0; w < LV_WAVES; ++w) sum += spart[w][threadIdx.x];
        scores[2 * (size_t)blockIdx.x + threadIdx.x] = sum;
    }
}

BF_API int bf_level_score(const void* hist, int G, const int32_t* candidates, int n_candidates, float cos_par,
                          float sin_perp, void* scores, void* stream) {
    if (G < 1 || G > BF_LEVEL_MAX_G || n_candidates < 0 || n_candidates > BF_LEVEL_MAX_CANDIDATES) return BF_ERR_ARG;
    if (n_candidates == 0) return BF_OK;
    if (!hist || !candidates || !scores) return BF_ERR_ARG;
    hipLaunchKernelGGL(k_level_score, dim3(n_candidates), dim3(LV_BLOCK), 0, bf_stream(stream), (const u64*)hist, G,
                       candidates, cos_par, sin_perp, (u64*)scores);
    return bf_check_launch();
}

// ---- refine ---------------------------------------------------------------------------------------------
#define LV_REFINE_STATS 10     // BF_LEVEL_STAT_REFINE_SAMPLES .. BF_LEVEL_STAT_REFINE_WEIGHT_UP

__device__ __forceinline__ long long lv_fix(float v, float scale) { return llrintf(v * scale); }

__global__ void __launch_bounds__(LV_BLOCK) k_level_refine(const float* __restrict__ points, const float* __restrict__ normals,
                                                           const uint32_t* __restrict__ weights, long long n,
                                                           const float* __restrict__ frame, float cos_par, float sin_perp,
                                                           float h0, float height_bin, int n_bins,
                                                           long long* __restrict__ sums, u64* __restrict__ heights,
                                                           u64* __restrict__ stats) {
    __shared__ u64 shist[BF_LEVEL_MAX_HEIGHT_BINS * BF_LEVEL_HEIGHT_WORDS];
    __shared__ u64 sstat[LV_WAVES][LV_REFINE_STATS];
    __shared__ long long ssum[LV_WAVES][BF_LEVEL_SUM_WORDS];
    const int lane = bf_lane(), wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < n_bins * BF_LEVEL_HEIGHT_WORDS; b += LV_BLOCK) shist[b] = 0;
    __syncthreads();
    const float cx = frame[0], cy = frame[1], cz = frame[2];
    const float ux = frame[3], uy = frame[4], uz = frame[5];
    const float vx = frame[6], vy = frame[7], vz = frame[8];
    const float nscale = (float)(1 << BF_LEVEL_NORMAL_SHIFT), mscale = (float)(1 << BF_LEVEL_METRE_SHIFT);
    const float limit = (float)BF_LEVEL_COORD_LIMIT;
    long long acc[BF_LEVEL_SUM_WORDS];
#pragma unroll
    for (int s = 0; s < BF_LEVEL_SUM_WORDS; ++s) acc[s] = 0;
    u64 st[LV_REFINE_STATS];
#pragma unroll
    for (int s = 0; s < LV_REFINE_STATS; ++s) st[s] = 0;
    const long long n_tiles = (n + LV_BLOCK - 1) / LV_BLOCK;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * LV_BLOCK + threadIdx.x;
        const bool live = i < n;
        float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        uint32_t w32 = 0;
        if (live) {
            px = points[3 * i];
            py = points[3 * i + 1];
            pz = points[3 * i + 2];
            nx = normals[3 * i];
            ny = normals[3 * i + 1];
            nz = normals[3 * i + 2];
            w32 = weights[i];
        }
        const bool use = live && w32 != 0 && isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(nx) && isfinite(ny) &&
                         isfinite(nz);
        const long long w = (long long)w32;
        const float t = lv_dot(nx, ny, nz, cx, cy, cz);
        const bool par = use && fabsf(t) >= cos_par, perp = use && fabsf(t) <= sin_perp, up = use && t >= cos_par;
        if (par || perp) {
            const long long qxx = lv_fix(nx * nx, nscale) * w, qxy = lv_fix(nx * ny, nscale) * w, qxz = lv_fix(nx * nz, nscale) * w;
            const long long qyy = lv_fix(ny * ny, nscale) * w, qyz = lv_fix(ny * nz, nscale) * w, qzz = lv_fix(nz * nz, nscale) * w;
            if (par) {
                acc[0] += qxx, acc[1] += qxy, acc[2] += qxz, acc[3] += qyy, acc[4] += qyz, acc[5] += qzz;
            }
            if (perp) {
                acc[6] += qxx, acc[7] += qxy, acc[8] += qxz, acc[9] += qyy, acc[10] += qyz, acc[11] += qzz;
                const float pa = lv_dot(nx, ny, nz, ux, uy, uz), pb = lv_dot(nx, ny, nz, vx, vy, vz);
                const float r = sqrtf(pa * pa + pb * pb);
                if (r > 0.f) {
                    const float a = pa / r, b = pb / r, a2 = a * a, b2 = b * b;
                    acc[12] += lv_fix(1.0f - (8.0f * a2) * b2, nscale) * w;
                    acc[13] += lv_fix(((4.0f * a) * b) * (a2 - b2), nscale) * w;
                }
            }
        }
        bool inside = false;
        if (up && n_bins > 0) {
            const float d = lv_dot(px, py, pz, cx, cy, cz) - h0;
            const float fb = floorf(d / height_bin);
            const float x1 = lv_dot(px, py, pz, ux, uy, uz), x2 = lv_dot(px, py, pz, vx, vy, vz);
            inside = d >= 0.f && fb < (float)n_bins && fabsf(x1) < limit && fabsf(x2) < limit;
            if (inside) {                                         // fb in 0 .. n_bins - 1
                u64* row = shist + (int)fb * BF_LEVEL_HEIGHT_WORDS;
                atomicAdd(row, (u64)w);
                atomicAdd(row + 1, (u64)(lv_fix(d, mscale) * w));
                atomicAdd(row + 2, (u64)(lv_fix(x1, mscale) * w));
                atomicAdd(row + 3, (u64)(lv_fix(x2, mscale) * w));
            }
        }
        st[0] += __popcll(__ballot(live));
        st[1] += __popcll(__ballot(live && !use));
        st[2] += __popcll(__ballot(par));
        st[3] += __popcll(__ballot(perp));
        st[4] += __popcll(__ballot(up));
        st[5] += __popcll(__ballot(up && !inside));
        st[6] += (u64)bf_wave_sum_i64(use ? w : 0ll);
        st[7] += (u64)bf_wave_sum_i64(par ? w : 0ll);
        st[8] += (u64)bf_wave_sum_i64(perp ? w : 0ll);
        st[9] += (u64)bf_wave_sum_i64(up ? w : 0ll);
    }
#pragma unroll
    for (int s = 0; s < BF_LEVEL_SUM_WORDS; ++s) {
        const long long v = bf_wave_sum_i64(acc[s]);
        if (lane == 0) ssum[wave][s] = v;
    }
    __syncthreads();                                              // the sums and the block's height histogram are complete
    if (threadIdx.x < BF_LEVEL_SUM_WORDS) {
        long long sum = 0;
        for (int w = 0; w < LV_WAVES; ++w) sum += ssum[w][threadIdx.x];
        if (sum) atomicAdd((u64*)sums + threadIdx.x, (u64)sum);
    }
    for (int b = threadIdx.x; b < n_bins * BF_LEVEL_HEIGHT_WORDS; b += LV_BLOCK) {
        const u64 v = shist[b];
        if (v) atomicAdd(heights + b, v);
    }
    lv_block_add<LV_REFINE_STATS>(st, sstat, stats, BF_LEVEL_STAT_REFINE_SAMPLES);
}

BF_API int bf_level_refine(const float* points, const float* normals, const uint32_t* weights, long long n,
                           const float* frame, float cos_par, float sin_perp, float h0, float height_bin, int n_bins,
                           void* sums, void* heights, void* stats, void* stream) {
    if (n < 0 || n_bins < 0 || n_bins > BF_LEVEL_MAX_HEIGHT_BINS) return BF_ERR_ARG;
    if (n_bins > 0 && (!(height_bin > 0.f) || !isfinite(height_bin) || !isfinite(h0) ||
                       (double)n_bins * (double)height_bin > (double)BF_LEVEL_COORD_LIMIT))
        return BF_ERR_ARG;
    if (n == 0) return BF_OK;
    if (!points || !normals || !weights || !frame || !sums || !stats || (n_bins > 0 && !heights)) return BF_ERR_ARG;
    hipLaunchKernelGGL(k_level_refine, dim3(lv_grid(n)), dim3(LV_BLOCK), 0, bf_stream(stream), points, normals, weights, n,
                       frame, cos_par, sin_perp, h0, height_bin, n_bins, (long long*)sums, (u64*)heights, (u64*)stats);
    return bf_check_launch();
}
