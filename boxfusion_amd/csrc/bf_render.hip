// bf_render.hip — a headless software rasteriser: z-buffered views of coloured points and box wireframes
//   bf_render_clear    every key of the target to "empty" (all ones)
//   bf_render_points   one thread per (point, view): world -> camera -> pixel, a square splat of atomicMin
//   bf_render_edges    one wave per (box edge, view): near clip, projection, Liang-Barsky clip to the image,
//                      at most max(W, H) + 1 samples with 1/Z interpolated linearly on the screen
//   bf_render_resolve  keys -> rgb u8 + depth f32, empty pixels take a constant or an image background
// Target: uint64 [V,H,W].  key = layer << 63 | bits(Z) << 32 | R << 24 | G << 16 | B << 8 | 0xFF with Z the
// camera-space depth (f32 > 0, so its bits are 31 bits and order like Z), layer 1 = scene, 0 = overlay.
// The key that stays at a pixel is the minimum of all candidates, and a minimum does not depend on the
// order of its operands: the image is the same bits whatever order points, edges, waves and launches
// arrive in (ties in depth go to the smaller colour word).  All f32 arithmetic runs left to right, without
// contraction and with IEEE division (DESIGN.md §4 "Renderer"; tests/render_util.py restates it in numpy).
#include "bf_common.h"

#define RENDER_BLOCK 256
#define RENDER_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RENDER_MAX_SIDE 16384
#define RENDER_MAX_VIEWS 65535

struct RenderCam {
    float fx, fy, cx, cy;
    int H, W;
};

// world -> camera of view row m = (R row-major, t): ((R0*x + R1*y) + R2*z) + t
__device__ __forceinline__ void render_to_camera(const float* __restrict__ m, float x, float y, float z, float& X,
                                                 float& Y, float& Z) {
    X = m[0] * x + m[1] * y + m[2] * z + m[9];
    Y = m[3] * x + m[4] * y + m[5] * z + m[10];
    Z = m[6] * x + m[7] * y + m[8] * z + m[11];
}

__device__ __forceinline__ unsigned long long render_key(int layer, float Z, unsigned color) {
    return ((unsigned long long)(layer != 0) << 63) | ((unsigned long long)__float_as_uint(Z) << 32) |
           (unsigned long long)color;
}

// The square (2r+1)^2 around the pixel nearest to (u, v), clipped to the image, every pixel with `key`.
// The window test runs on the floats, so the int conversion below never sees a value it cannot hold.
// A pixel whose stored key is already <= key is left alone: keys only decrease, so a stale read can only
// cost an atomic that changes nothing.  cand / issued: splat pixels inside the image / atomics issued.
__device__ __forceinline__ void render_splat(unsigned long long* __restrict__ view, const RenderCam& c, float u, float v,
                                             int r, unsigned long long key, unsigned& cand, unsigned& issued) {
    if (!(u >= (float)(-(r + 1)) && u <= (float)(c.W + r) && v >= (float)(-(r + 1)) && v <= (float)(c.H + r))) return;
    const int ix = (int)floorf(u + 0.5f), iy = (int)floorf(v + 0.5f);
    const int x0 = ix - r < 0 ? 0 : ix - r, x1 = ix + r > c.W - 1 ? c.W - 1 : ix + r;
    const int y0 = iy - r < 0 ? 0 : iy - r, y1 = iy + r > c.H - 1 ? c.H - 1 : iy + r;
    for (int y = y0; y <= y1; ++y) {
        unsigned long long* row = view + (size_t)y * c.W;
        for (int x = x0; x <= x1; ++x) {
            ++cand;
            if (*(const volatile unsigned long long*)(row + x) <= key) continue;
            atomicMin(row + x, key);
            ++issued;
        }
    }
}

__device__ __forceinline__ unsigned render_color(const uint8_t* __restrict__ c) {
    return ((unsigned)c[0] << 24) | ((unsigned)c[1] << 16) | ((unsigned)c[2] << 8) | 0xFFu;
}

// grid (blocks of points, views)
__global__ void __launch_bounds__(RENDER_BLOCK) k_render_points(const float* __restrict__ xyz, const uint8_t* __restrict__ rgb,
                                                                long long n, const float* __restrict__ cams, RenderCam c,
                                                                float near_z, float far_z, int r, int layer,
                                                                unsigned long long* __restrict__ keys,
                                                                unsigned long long* __restrict__ stats) {
    __shared__ unsigned bstats[2];
    if (stats) {
        if (threadIdx.x < 2) bstats[threadIdx.x] = 0;
        __syncthreads();
    }
    const long long p = (long long)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const int view = blockIdx.y;
    unsigned cand = 0, issued = 0;
    if (p < n) {
        const float x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
        float X, Y, Z;
        render_to_camera(cams + 12 * view, x, y, z, X, Y, Z);
        if (isfinite(X) && isfinite(Y) && isfinite(Z) && Z > near_z && Z < far_z) {
            const float u = c.fx * X / Z + c.cx, v = c.fy * Y / Z + c.cy;
            render_splat(keys + (size_t)view * c.H * c.W, c, u, v, r, render_key(layer, Z, render_color(rgb + 3 * p)),
                         cand, issued);
        }
    }
    if (stats) {                                                 // wave-uniform: every lane takes part
        const int cs = bf_wave_sum_i32((int)cand), is = bf_wave_sum_i32((int)issued);
        if (bf_lane() == 0 && cs) {
            atomicAdd(bstats, (unsigned)cs);
            atomicAdd(bstats + 1, (unsigned)is);
        }
        __syncthreads();
        if (threadIdx.x < 2 && bstats[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)bstats[threadIdx.x]);
    }
}

// the twelve edges of a box in the v0..v7 corner order (instances.py augment_vertices)
__constant__ unsigned char RENDER_EDGES[12][2] = {{0, 1}, {0, 4}, {1, 5}, {4, 5}, {2, 3}, {2, 6},
                                                  {6, 7}, {3, 7}, {0, 3}, {4, 7}, {1, 2}, {5, 6}};

// one Liang-Barsky boundary: keeps the part of t0..t1 where t * p <= q; false when none is left
__device__ __forceinline__ bool render_clip(float p, float q, float& t0, float& t1) {
    if (p == 0.f) return q >= 0.f;
    const float r = q / p;
    if (p < 0.f) {
        if (r > t1) return false;
        if (r > t0) t0 = r;
    } else {
        if (r < t0) return false;
        if (r < t1) t1 = r;
    }
    return true;
}

// grid (blocks of four edges, views); one wave per (box edge, view), every lane runs the same set-up and
// takes the samples lane, lane + 64, ...
__global__ void __launch_bounds__(RENDER_BLOCK) k_render_edges(const float* __restrict__ corners, const uint8_t* __restrict__ colors,
                                                               const uint8_t* __restrict__ mask, int B,
                                                               const float* __restrict__ cams, RenderCam c, float near_z,
                                                               int hw, int layer, unsigned long long* __restrict__ keys) {
    const int e = blockIdx.x * (RENDER_BLOCK / 64) + (threadIdx.x >> 6);
    if (e >= B * 12) return;                                     // wave-uniform
    const int box = e / 12, edge = e - box * 12, lane = bf_lane(), view = blockIdx.y;
    if (mask && mask[box] == 0) return;
    const float* cb = corners + (size_t)box * 24;
    if (__ballot(lane < 24 && !isfinite(cb[lane < 24 ? lane : 0]))) return;   // a box with a non-finite corner: skipped whole
    const float* A = cb + 3 * RENDER_EDGES[edge][0];
    const float* Bc = cb + 3 * RENDER_EDGES[edge][1];
    float Xa, Ya, Za, Xb, Yb, Zb;
    render_to_camera(cams + 12 * view, A[0], A[1], A[2], Xa, Ya, Za);
    render_to_camera(cams + 12 * view, Bc[0], Bc[1], Bc[2], Xb, Yb, Zb);
    if (!(isfinite(Xa) && isfinite(Ya) && isfinite(Za) && isfinite(Xb) && isfinite(Yb) && isfinite(Zb))) return;
    if (Za < near_z && Zb < near_z) return;
    if (Za < near_z) {                                           // the end behind the near plane moves onto it
        const float t = (near_z - Za) / (Zb - Za);
        Xa = Xa + t * (Xb - Xa);
        Ya = Ya + t * (Yb - Ya);
        Za = near_z;
    } else if (Zb < near_z) {
        const float t = (near_z - Za) / (Zb - Za);
        Xb = Xa + t * (Xb - Xa);
        Yb = Ya + t * (Yb - Ya);
        Zb = near_z;
    }
    const float ua = c.fx * Xa / Za + c.cx, va = c.fy * Ya / Za + c.cy, wa = 1.0f / Za;
    const float ub = c.fx * Xb / Zb + c.cx, vb = c.fy * Yb / Zb + c.cy, wb = 1.0f / Zb;
    if (!(isfinite(ua) && isfinite(va) && isfinite(ub) && isfinite(vb))) return;
    const float du = ub - ua, dv = vb - va, dw = wb - wa;
    float t0 = 0.f, t1 = 1.f;
    if (!render_clip(-du, ua - (-0.5f), t0, t1) || !render_clip(du, ((float)c.W - 0.5f) - ua, t0, t1) ||
        !render_clip(-dv, va - (-0.5f), t0, t1) || !render_clip(dv, ((float)c.H - 0.5f) - va, t0, t1))
        return;
    // the clipped segment spans at most the image, so n <= max(W, H) however long the edge was before the
    // clip (an edge that grazes the near plane projects to millions of pixels); the cap makes it unconditional
    const float span = fmaxf(fabsf((ua + t1 * du) - (ua + t0 * du)), fabsf((va + t1 * dv) - (va + t0 * dv)));
    const int cap = c.W > c.H ? c.W : c.H;
    const int n = span < (float)cap ? (int)ceilf(span) : cap;    // span is finite and >= 0
    const float fn = (float)(n > 1 ? n : 1), dt = t1 - t0;
    const unsigned color = render_color(colors + 3 * box);
    unsigned long long* vk = keys + (size_t)view * c.H * c.W;
    unsigned cand = 0, issued = 0;
    for (int i = lane; i <= n; i += 64) {
        const float t = t0 + dt * ((float)i / fn);
        const float u = ua + t * du, v = va + t * dv, w = wa + t * dw;
        const float Z = 1.0f / w;
        if (!(Z > 0.f && Z < __builtin_inff())) continue;
        render_splat(vk, c, u, v, hw, render_key(layer, Z, color), cand, issued);
    }
}

// four consecutive pixels per thread; vec: rgb is 4-byte and depth 16-byte aligned, so a full group goes
// out as three dwords and one float4
__global__ void __launch_bounds__(RENDER_BLOCK) k_render_resolve(const unsigned long long* __restrict__ keys, long long total,
                                                                 const uint8_t* __restrict__ bg_image, unsigned bg,
                                                                 uint8_t* __restrict__ rgb, float* __restrict__ depth, int vec) {
    const long long p0 = ((long long)blockIdx.x * RENDER_BLOCK + threadIdx.x) * 4;
    if (p0 >= total) return;
    const int m = total - p0 < 4 ? (int)(total - p0) : 4;
    uint8_t px[12];
    float d[4];
    for (int j = 0; j < m; ++j) {
        const unsigned long long k = keys[p0 + j];
        if (k == RENDER_EMPTY) {
            d[j] = 0.f;
            if (bg_image) {
                const uint8_t* s = bg_image + (p0 + j) * 3;
                px[3 * j] = s[0], px[3 * j + 1] = s[1], px[3 * j + 2] = s[2];
            } else {
                px[3 * j] = (uint8_t)(bg >> 16), px[3 * j + 1] = (uint8_t)(bg >> 8), px[3 * j + 2] = (uint8_t)bg;
            }
        } else {
            d[j] = __uint_as_float((unsigned)(k >> 32) & 0x7FFFFFFFu);
            px[3 * j] = (uint8_t)(k >> 24), px[3 * j + 1] = (uint8_t)(k >> 16), px[3 * j + 2] = (uint8_t)(k >> 8);
        }
    }
    if (vec && m == 4) {
        unsigned w[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            w[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) |
                   ((unsigned)px[4 * j + 3] << 24);
        unsigned* o = reinterpret_cast<unsigned*>(rgb + p0 * 3);
        o[0] = w[0], o[1] = w[1], o[2] = w[2];
        *reinterpret_cast<float4*>(depth + p0) = make_float4(d[0], d[1], d[2], d[3]);
    } else {
        for (int j = 0; j < m; ++j) {
            depth[p0 + j] = d[j];
            rgb[(p0 + j) * 3] = px[3 * j], rgb[(p0 + j) * 3 + 1] = px[3 * j + 1], rgb[(p0 + j) * 3 + 2] = px[3 * j + 2];
        }
    }
}

static inline bool render_target_ok(const void* keys, int V, int H, int W) {
    return keys && V >= 1 && V <= RENDER_MAX_VIEWS && H >= 1 && H <= RENDER_MAX_SIDE && W >= 1 && W <= RENDER_MAX_SIDE;
}

static inline bool render_camera_ok(const float* cams, float fx, float fy, float cx, float cy, float near_z) {
    const float inf = __builtin_inff();
    return cams && fx > 0.f && fx < inf && fy > 0.f && fy < inf && cx > -inf && cx < inf && cy > -inf && cy < inf &&
           near_z > 0.f && near_z < inf;
}

BF_API int bf_render_clear(void* keys, int V, int H, int W, void* stream) {
    if (!render_target_ok(keys, V, H, W)) return BF_ERR_ARG;
    if (hipMemsetAsync(keys, 0xFF, (size_t)V * H * W * sizeof(unsigned long long), bf_stream(stream)) != hipSuccess)
        return BF_ERR_LAUNCH;
    return BF_OK;
}

BF_API int bf_render_points(const float* xyz, const uint8_t* rgb, long long n, const float* cams, int V, float fx, float fy,
                            float cx, float cy, int H, int W, float near_z, float far_z, int radius, int layer, void* keys,
                            void* stats, void* stream) {
    if (!render_target_ok(keys, V, H, W) || !render_camera_ok(cams, fx, fy, cx, cy, near_z) || !(far_z > near_z) || n < 0 ||
        radius < 0 || radius > 4 || (layer != 0 && layer != 1))
        return BF_ERR_ARG;
    if (n == 0) return BF_OK;
    if (!xyz || !rgb) return BF_ERR_ARG;
    const long long nb = (n + RENDER_BLOCK - 1) / RENDER_BLOCK;
    if (nb >= (1ll << 31)) return BF_ERR_CAPACITY;
    const RenderCam c = {fx, fy, cx, cy, H, W};
    hipLaunchKernelGGL(k_render_points, dim3((unsigned)nb, (unsigned)V), dim3(RENDER_BLOCK), 0, bf_stream(stream), xyz, rgb,
                       n, cams, c, near_z, far_z, radius, layer, (unsigned long long*)keys, (unsigned long long*)stats);
    return bf_check_launch();
}

BF_API int bf_render_edges(const float* corners, const uint8_t* colors, const uint8_t* mask, int B, const float* cams, int V,
                           float fx, float fy, float cx, float cy, int H, int W, float near_z, int half_width, int layer,
                           void* keys, void* stream) {
    if (!render_target_ok(keys, V, H, W) || !render_camera_ok(cams, fx, fy, cx, cy, near_z) || B < 0 || half_width < 0 ||
        half_width > 2 || (layer != 0 && layer != 1))
        return BF_ERR_ARG;
    if (B == 0) return BF_OK;
    if (!corners || !colors) return BF_ERR_ARG;
    if (B > (1 << 24)) return BF_ERR_CAPACITY;
    const RenderCam c = {fx, fy, cx, cy, H, W};
    hipLaunchKernelGGL(k_render_edges, dim3(bf_cdiv((unsigned)B * 12u, RENDER_BLOCK / 64), (unsigned)V), dim3(RENDER_BLOCK), 0,
                       bf_stream(stream), corners, colors, mask, B, cams, c, near_z, half_width, layer,
                       (unsigned long long*)keys);
    return bf_check_launch();
}

BF_API int bf_render_resolve(const void* keys, int V, int H, int W, const uint8_t* bg_image, int bg_r, int bg_g, int bg_b,
                             uint8_t* rgb, float* depth, void* stream) {
    if (!render_target_ok(keys, V, H, W) || !rgb || !depth || bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 ||
        bg_b > 255)
        return BF_ERR_ARG;
    const long long total = (long long)V * H * W;
    const long long nb = ((total + 3) / 4 + RENDER_BLOCK - 1) / RENDER_BLOCK;
    if (nb >= (1ll << 31)) return BF_ERR_CAPACITY;
    const int vec = ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)depth & 15) == 0;
    hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)nb), dim3(RENDER_BLOCK), 0, bf_stream(stream),
                       (const unsigned long long*)keys, total, bg_image, ((unsigned)bg_r << 16) | ((unsigned)bg_g << 8) | (unsigned)bg_b,
                       rgb, depth, vec);
    return bf_check_launch();
}
