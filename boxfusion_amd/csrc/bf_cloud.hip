// bf_cloud.hip — the coloured scene point cloud (demo.py:121-127, :193) and a persistent voxel map of it:
//   bf_resize_bicubic_u8  Image.fromarray(image).resize((W_d, H_d)) (demo.py:124): Pillow's 8-bit BICUBIC path,
//                         horizontal pass into a u8 intermediate, then the vertical pass; the integer coefficient
//                         and bounds tables come from the host (_lib.pil_bicubic_coeffs), the kernels apply them
//   bf_cloud_pack         torch.cat((xyz, matched_image / 255.0), -1)[valid] (demo.py:127) for a batch: a stable
//                         compaction (ballot + popcount per wave, one count per block, a scan of the block
//                         counts, the scatter); no atomic decides an output position
//   bf_cloud_integrate    the valid points into an open-addressing voxel hash map whose per-voxel state is
//                         integers only (count, in-voxel offset sums, colour sums): integer adds commute, so the
//                         table's contents are the same bits whatever order the waves arrive in
//   bf_cloud_extract      the occupied slots, compacted (in slot order)
// Voxel slot (5 x u64; low u32, high u32): key; count, sum_qx; sum_qy, sum_qz; sum_r, sum_g; sum_b, 0.
// A field holds at most 255 * 2^24 < 2^32, so the packed 64-bit adds never carry from the low field into the high.
#include "bf_compact.h"

#define PIL_PRECISION_BITS 22

// ---- Pillow 8-bit resample passes ------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t pil_clip8(int v) {
    v >>= PIL_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one thread per output byte: src [F, H, Ws, 3] -> dst [F, H, Wd, 3]
__global__ void __launch_bounds__(256) k_pil_horizontal(const uint8_t* __restrict__ src, int Ws, int Wd, long long rows,
                                                        const int* __restrict__ kk, const int* __restrict__ bounds,
                                                        int ksize, uint8_t* __restrict__ dst) {
    const long long total = rows * Wd * 3;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % 3);
        const long long px = e / 3;
        const int xo = (int)(px % Wd);
        const long long row = px / Wd;
        int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
        xmin = xmin < 0 ? 0 : (xmin > Ws ? Ws : xmin);
        n = n > ksize ? ksize : n;
        n = n > Ws - xmin ? Ws - xmin : n;
        const uint8_t* s = src + (row * Ws + xmin) * 3 + c;
        const int* k = kk + (size_t)xo * ksize;
        int acc = 1 << (PIL_PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += (int)s[3 * t] * k[t];
        dst[e] = pil_clip8(acc);
    }
}

// src [F, Hs, W, 3] -> dst [F, Hd, W, 3]
__global__ void __launch_bounds__(256) k_pil_vertical(const uint8_t* __restrict__ src, int Hs, int Hd, int W, int F,
                                                      const int* __restrict__ kk, const int* __restrict__ bounds,
                                                      int ksize, uint8_t* __restrict__ dst) {
    const long long line = (long long)W * 3;
    const long long total = (long long)F * Hd * line;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long col = e % line;
        const long long r = e / line;
        const int yo = (int)(r % Hd);
        const long long f = r / Hd;
        int ymin = bounds[2 * yo], n = bounds[2 * yo + 1];
        ymin = ymin < 0 ? 0 : (ymin > Hs ? Hs : ymin);
        n = n > ksize ? ksize : n;
        n = n > Hs - ymin ? Hs - ymin : n;
        const uint8_t* s = src + (f * Hs + ymin) * line + col;
        const int* k = kk + (size_t)yo * ksize;
        int acc = 1 << (PIL_PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += (int)s[(long long)t * line] * k[t];
        dst[e] = pil_clip8(acc);
    }
}

static inline unsigned cloud_grid(long long total) {
    const long long g = (total + 255) / 256;
    return (unsigned)(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

BF_API int bf_resize_bicubic_u8(const uint8_t* src, int F, int Hs, int Ws, int Hd, int Wd, const int* kx,
                                const int* bx, int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp,
                                uint8_t* dst, void* stream) {
    if (!src || !dst || F < 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return BF_ERR_ARG;
    const bool horiz = Ws != Wd, vert = Hs != Hd;
    if ((horiz && (!kx || !bx || ksx <= 0)) || (vert && (!ky || !by || ksy <= 0)) || (horiz && vert && !tmp))
        return BF_ERR_ARG;
    if (F == 0) return BF_OK;
    hipStream_t st = bf_stream(stream);
    if (!horiz && !vert) {
        if (hipMemcpyAsync(dst, src, (size_t)F * Hs * Ws * 3, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return BF_ERR_LAUNCH;
        return BF_OK;
    }
    const uint8_t* mid = src;
    if (horiz) {
        uint8_t* out = vert ? tmp : dst;
        const long long rows = (long long)F * Hs;
        hipLaunchKernelGGL(k_pil_horizontal, dim3(cloud_grid(rows * Wd * 3)), dim3(256), 0, st, src, Ws, Wd, rows, kx,
                           bx, ksx, out);
        mid = out;
    }
    if (vert)
        hipLaunchKernelGGL(k_pil_vertical, dim3(cloud_grid((long long)F * Hd * Wd * 3)), dim3(256), 0, st, mid, Hs, Hd,
                           Wd, F, ky, by, ksy, dst);
    return bf_check_launch();
}

// ---- bf_cloud_pack: the valid pixels of B frames, compacted (bf_compact.h) ----------------------------------------------
struct PackSel {                                                 // block b = frame b / bpf's block b % bpf
    const float* xyz;
    const uint8_t* valid;
    const uint8_t* rgb;
    int hw, bpf;
    float* out;
    __device__ bool selected(unsigned b, unsigned t) const {
        const int f = b / bpf, j = b - f * bpf, p = j * CLOUD_BLOCK + t;
        return p < hw && valid[(size_t)f * hw + p] != 0;
    }
    __device__ void write(unsigned b, unsigned t, size_t row) const {
        const int f = b / bpf, j = b - f * bpf, p = j * CLOUD_BLOCK + t;
        const size_t px = (size_t)f * hw + p;
        float* o = out + row * 6;
        const float* s = xyz + px * 3;
        const uint8_t* c = rgb + px * 3;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
        o[3] = (float)c[0] / 255.0f;
        o[4] = (float)c[1] / 255.0f;
        o[5] = (float)c[2] / 255.0f;
    }
};

BF_API size_t bf_cloud_blocks(long long items_per_group, int groups) {
    if (items_per_group <= 0 || groups <= 0) return 0;
    return (size_t)((items_per_group + CLOUD_BLOCK - 1) / CLOUD_BLOCK) * (size_t)groups;
}

BF_API int bf_cloud_pack(const float* xyz, const uint8_t* valid, const uint8_t* rgb, int B, int H, int W,
                         float* xyzrgb, int* offsets, int* block_counts, void* stream) {
    if (!xyz || !valid || !rgb || !xyzrgb || !offsets || !block_counts || B <= 0 || H <= 0 || W <= 0)
        return BF_ERR_ARG;
    const long long hw = (long long)H * W;
    const long long bpf = (hw + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
    if (hw * B >= (1ll << 31) || bpf * B >= (1ll << 31)) return BF_ERR_CAPACITY;
    compact<PackSel>((unsigned)(bpf * B), block_counts, (int)bpf, offsets, B, bf_stream(stream), xyz, valid, rgb, (int)hw,
                     (int)bpf, xyzrgb);
    return bf_check_launch();
}

// ---- voxel hash map -----------------------------------------------------------------------------------------------
// one thread per point; lanes of a wave that hold the same voxel in adjacent lanes form a run, and the run's
// first lane adds the run's sums (four 64-bit integer adds per run)
__global__ void __launch_bounds__(CLOUD_BLOCK) k_cloud_integrate(const float* __restrict__ xyz, const uint8_t* __restrict__ valid,
                                                                 const uint8_t* __restrict__ rgb, long long n, float fine_step,
                                                                 unsigned long long* __restrict__ table,
                                                                 unsigned long long mask, unsigned long long* __restrict__ stats,
                                                                 int merge) {
    __shared__ unsigned bstats[BF_STATS_WORDS];
    stats_begin(bstats);
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const int lane = bf_lane();
    bool live = p < n && valid[p] != 0;
    unsigned long long key = BF_KEY_EMPTY;
    unsigned q01 = 0, q2r = 0, gb = 0;                          // 16-bit pairs: qx | qy, qz | r, g | b
    bool nonfinite = false, out_of_range = false;
    if (live) {
        const float x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
        const float fx = floorf(x / fine_step), fy = floorf(y / fine_step), fz = floorf(z / fine_step);
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
            nonfinite = true;
        } else if (!key_in_range(fx, fy, fz, (float)BF_KEY_BIAS * BF_CLOUD_FINE_STEPS)) {
            out_of_range = true;
        } else {
            const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
            key = key_pack(ix >> 8, iy >> 8, iz >> 8);
            q01 = (unsigned)(ix & 255) | ((unsigned)(iy & 255) << 16);
            q2r = (unsigned)(iz & 255) | ((unsigned)rgb[3 * p] << 16);
            gb = (unsigned)rgb[3 * p + 1] | ((unsigned)rgb[3 * p + 2] << 16);
        }
    }
    stat_add(bstats, BF_CLOUD_STAT_NONFINITE, nonfinite);
    stat_add(bstats, BF_CLOUD_STAT_OUT_OF_RANGE, out_of_range);
    live = key != BF_KEY_EMPTY;

    // runs of equal keys over adjacent lanes (dead lanes carry EMPTY and form runs that are skipped)
    const unsigned long long prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key || (!merge && live);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const int leader = 63 - __clzll((long long)upto);
    const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
    const int run_end = above ? __ffsll((long long)above) - 1 : 64;  // first lane past this lane's run
    // segmented sums towards the run's first lane; at most 64 * 255 per 16-bit field
    unsigned s01 = q01, s2r = q2r, sgb = gb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned a = __shfl_down(s01, o, 64), b = __shfl_down(s2r, o, 64), c = __shfl_down(sgb, o, 64);
        if (lane + o < run_end) {
            s01 += a;
            s2r += b;
            sgb += c;
        }
    }
    const bool lead = live && head;
    stat_add(bstats, BF_CLOUD_STAT_RUNS, lead);
    const unsigned cnt = (unsigned)(run_end - lane);            // the run's points, in its first lane

    long long slot = -1;
    int slow = 0;
    if (lead) {
        bool claimed = false;
        slot = map_find<BF_CLOUD_SLOT_WORDS>(table, mask, key, &claimed);
        if (slot >= 0) {
            unsigned long long* w = table + slot * BF_CLOUD_SLOT_WORDS;
            const unsigned long long add0 = (unsigned long long)cnt | ((unsigned long long)(s01 & 0xFFFFu) << 32);
            const unsigned long long old = atomicAdd(w + 1, add0);
            if ((unsigned)(old & 0xFFFFFFFFull) + cnt > BF_CLOUD_MAX_COUNT) {
                atomicAdd(w + 1, 0ull - add0);                  // over the cap: take the run back, go point by point
                slow = 1;
            } else {
                atomicAdd(w + 2, (unsigned long long)(s01 >> 16) | ((unsigned long long)(s2r & 0xFFFFu) << 32));
                atomicAdd(w + 3, (unsigned long long)(s2r >> 16) | ((unsigned long long)(sgb & 0xFFFFu) << 32));
                atomicAdd(w + 4, (unsigned long long)(sgb >> 16));
            }
        }
    }
    // the run's slot and verdict, from its first lane
    slot = __shfl(slot, leader, 64);
    slow = __shfl(slow, leader, 64);
    bool refused = false;
    if (live && slow) {                                         // a voxel at its cap: each point on its own
        unsigned long long* w = table + slot * BF_CLOUD_SLOT_WORDS;
        const unsigned long long add0 = 1ull | ((unsigned long long)(q01 & 0xFFFFu) << 32);
        const unsigned long long old = atomicAdd(w + 1, add0);
        if ((unsigned)(old & 0xFFFFFFFFull) >= BF_CLOUD_MAX_COUNT) {
            atomicAdd(w + 1, 0ull - add0);
            refused = true;
        } else {
            atomicAdd(w + 2, (unsigned long long)(q01 >> 16) | ((unsigned long long)(q2r & 0xFFFFu) << 32));
            atomicAdd(w + 3, (unsigned long long)(q2r >> 16) | ((unsigned long long)(gb & 0xFFFFu) << 32));
            atomicAdd(w + 4, (unsigned long long)(gb >> 16));
        }
    }
    stat_add(bstats, BF_CLOUD_STAT_DROPPED_FULL, live && slot < 0);
    stat_add(bstats, BF_CLOUD_STAT_SATURATED, refused);
    stat_add(bstats, BF_CLOUD_STAT_STORED, live && slot >= 0 && !refused);
    stats_flush(bstats, stats);
}

BF_API int bf_cloud_integrate(const float* xyz, const uint8_t* valid, const uint8_t* rgb, long long n, float fine_step,
                              void* table, long long capacity, void* stats, int merge, void* stream) {
    if (!xyz || !valid || !rgb || !table || !stats || n < 0 || capacity <= 0 || (capacity & (capacity - 1)) ||
        !(fine_step > 0.f))
        return BF_ERR_ARG;
    if (capacity > (1ll << 40)) return BF_ERR_CAPACITY;
    if (n == 0) return BF_OK;
    const long long nb = (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
    if (nb >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_cloud_integrate, dim3((unsigned)nb), dim3(CLOUD_BLOCK), 0, bf_stream(stream), xyz, valid, rgb,
                       n, fine_step, (unsigned long long*)table, (unsigned long long)(capacity - 1),
                       (unsigned long long*)stats, merge);
    return bf_check_launch();
}

struct CloudSlotSel {                                            // thread t of block b = slot b * CLOUD_BLOCK + t
    const unsigned long long* table;
    long long cap;
    long long* key;
    unsigned* count;
    unsigned* sums;
    __device__ bool selected(unsigned b, unsigned t) const {
        const long long s = (long long)b * CLOUD_BLOCK + t;
        return s < cap && table[s * BF_CLOUD_SLOT_WORDS] != BF_KEY_EMPTY;
    }
    __device__ void write(unsigned b, unsigned t, size_t row) const {
        const unsigned long long* w = table + ((long long)b * CLOUD_BLOCK + t) * BF_CLOUD_SLOT_WORDS;
        const unsigned long long a = w[1], b2 = w[2], c = w[3], d = w[4];
        key[row] = (long long)w[0];
        count[row] = (unsigned)a;
        unsigned* q = sums + row * 6;
        q[0] = (unsigned)(a >> 32);
        q[1] = (unsigned)b2;
        q[2] = (unsigned)(b2 >> 32);
        q[3] = (unsigned)c;
        q[4] = (unsigned)(c >> 32);
        q[5] = (unsigned)d;
    }
};

BF_API int bf_cloud_extract(const void* table, long long capacity, int64_t* key, uint32_t* count, uint32_t* sums, int* n_out,
                            int* block_counts, void* stream) {
    if (!table || !key || !count || !sums || !n_out || !block_counts || capacity <= 0) return BF_ERR_ARG;
    if (capacity >= (1ll << 31)) return BF_ERR_CAPACITY;
    compact<CloudSlotSel>(compact_blocks(capacity), block_counts, 0, n_out, 0, bf_stream(stream),
                          (const unsigned long long*)table, capacity, (long long*)key, (unsigned*)count, (unsigned*)sums);
    return bf_check_launch();
}
