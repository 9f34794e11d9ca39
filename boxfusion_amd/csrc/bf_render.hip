// bf_render.hip — a headless software rasteriser: z-buffered views of coloured points and box wireframes
//   bf_render_clear    every key of the target to "empty" (all ones)
//   bf_render_points   one thread per (point, view): world -> camera -> pixel, a square splat of atomicMin
//   bf_render_edges    one wave per (box edge, view): near clip, projection, Liang-Barsky clip to the image,
//                      at most max(W, H) + 1 samples with 1/Z interpolated linearly on the screen
//   bf_render_triangles one lane per (triangle, view): vertices snapped to 1/256 px, integer edge functions with
//                      a top-left tie rule (watertight, every pixel of a closed surface exactly once), 1/Z and
//                      colour interpolated in f64; large triangles are filled by the whole wave
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

// ---- triangles -----------------------------------------------------------------------------------------
// What a lane knows of its (triangle, view) after the set-up.  Coverage is integer: the vertices snapped to
// 1/256 px, E_i(ix, iy) = C[i] + A[i] ix + B[i] iy the edge function of the edge opposite vertex i at the
// centre of pixel (ix, iy), all exact in int64 (|xs|, |ys| < 2^30, so every product is below 2^62).
struct RenderTri {
    long long A[3], B[3], C[3], area2;
    double iz[3];                                                // 1 / Z of the three vertices
    unsigned col[3];                                             // r << 16 | g << 8 | b
    float shade;
    int x0, y0, w, npx, tie;                                     // the clipped pixel rectangle; tie bit i: E_i == 0 counts
};

enum { TRI_DRAWN = 0, TRI_RANGE = 1, TRI_BOUNDS = 2, TRI_CULLED = 3, TRI_NONE = 4 };
#define RENDER_GUARD 4194304.f                                   // 2^22 px
#define RENDER_AMBIENT 0.3f
#define RENDER_SPREAD_BLOCKS 256                                 // one block per CU of the chip

__device__ __forceinline__ int render_tri_setup(const float* __restrict__ verts, const uint8_t* __restrict__ rgb, long long n,
                                                const int* __restrict__ face, const float* __restrict__ cam,
                                                const RenderCam& c, float near_z, float far_z, int cull, int shade,
                                                RenderTri& t) {
    t.npx = 0;
    int id[3] = {face[0], face[1], face[2]};
    if (id[0] < 0 || id[0] >= n || id[1] < 0 || id[1] >= n || id[2] < 0 || id[2] >= n) return TRI_BOUNDS;
    float X[3], Y[3], Z[3];
    for (int k = 0; k < 3; ++k) {
        const float* p = verts + 3 * (long long)id[k];
        const float x = p[0], y = p[1], z = p[2];
        render_to_camera(cam, x, y, z, X[k], Y[k], Z[k]);
        if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(X[k]) && isfinite(Y[k]) && isfinite(Z[k]))) return TRI_RANGE;
    }
    for (int k = 0; k < 3; ++k)
        if (!(Z[k] > near_z && Z[k] < far_z)) return TRI_RANGE;
    long long xs[3], ys[3];
    for (int k = 0; k < 3; ++k) {
        const float u = c.fx * X[k] / Z[k] + c.cx, v = c.fy * Y[k] / Z[k] + c.cy;
        if (!(fabsf(u) < RENDER_GUARD && fabsf(v) < RENDER_GUARD)) return TRI_BOUNDS;
        xs[k] = (int)rintf(u * 256.f);
        ys[k] = (int)rintf(v * 256.f);
    }
    long long area2 = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0]);
    if (area2 == 0 || (cull && area2 > 0)) return TRI_CULLED;
    int o1 = 1, o2 = 2;
    if (area2 < 0) o1 = 2, o2 = 1, area2 = -area2;
    const int ord[3] = {0, o1, o2};
    t.area2 = area2;
    t.tie = 0;
    for (int i = 0; i < 3; ++i) {
        const int a = ord[(i + 1) % 3], b = ord[(i + 2) % 3];
        const long long dx = xs[b] - xs[a], dy = ys[b] - ys[a];
        t.A[i] = -256 * dy;
        t.B[i] = 256 * dx;
        t.C[i] = dy * xs[a] - dx * ys[a];
        if (dy < 0 || (dy == 0 && dx > 0)) t.tie |= 1 << i;
        const uint8_t* q = rgb + 3 * (long long)id[ord[i]];
        t.col[i] = ((unsigned)q[0] << 16) | ((unsigned)q[1] << 8) | (unsigned)q[2];
        t.iz[i] = 1.0 / (double)Z[ord[i]];
    }
    t.shade = 1.f;
    if (shade) {                                                 // a two-sided headlight: the triangle and the view only
        const float ax = X[1] - X[0], ay = Y[1] - Y[0], az = Z[1] - Z[0];
        const float bx = X[2] - X[0], by = Y[2] - Y[0], bz = Z[2] - Z[0];
        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float gx = X[0] + X[1] + X[2], gy = Y[0] + Y[1] + Y[2], gz = Z[0] + Z[1] + Z[2];
        const float dot = nx * gx + ny * gy + nz * gz;
        const float nn = nx * nx + ny * ny + nz * nz, gg = gx * gx + gy * gy + gz * gz;
        const float q = fabsf(dot) / sqrtf(nn * gg);
        const float cs = isfinite(q) ? (q < 1.f ? q : 1.f) : 0.f;
        t.shade = RENDER_AMBIENT + (1.f - RENDER_AMBIENT) * cs;
    }
    const long long lox = min(xs[0], min(xs[1], xs[2])), hix = max(xs[0], max(xs[1], xs[2]));
    const long long loy = min(ys[0], min(ys[1], ys[2])), hiy = max(ys[0], max(ys[1], ys[2]));
    long long x0 = (lox + 255) >> 8, x1 = hix >> 8, y0 = (loy + 255) >> 8, y1 = hiy >> 8;   // >> floors
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > c.W - 1) x1 = c.W - 1;
    if (y1 > c.H - 1) y1 = c.H - 1;
    if (x0 <= x1 && y0 <= y1) {
        t.x0 = (int)x0, t.y0 = (int)y0, t.w = (int)(x1 - x0 + 1);
        t.npx = t.w * (int)(y1 - y0 + 1);                        // at most 2^28
    }
    return TRI_DRAWN;
}

// One covered pixel: perspective-correct depth and colour in f64 from the exact edge values (one division:
// everything is scaled by r = 1 / iw), then the same early-out and atomicMin as a splat.  `seen` is the
// stored key, loaded by the caller ahead of the arithmetic so that its latency runs under it.  A stored key
// whose (layer, depth) word is already smaller wins whatever the colour, so the colour is only worked out for
// a pixel that may be written.
__device__ __forceinline__ unsigned long long render_seen(const unsigned long long* px) {
    return *(const volatile unsigned long long*)px;
}

__device__ __forceinline__ void render_tri_pixel(const RenderTri& t, long long e0, long long e1, long long e2, int shade, int layer,
                                                 unsigned long long seen, unsigned long long* __restrict__ px,
                                                 unsigned long long& issued) {
    const double t0 = (double)e0 * t.iz[0], t1 = (double)e1 * t.iz[1], t2 = (double)e2 * t.iz[2];
    const double iw = (t0 + t1) + t2, r = 1.0 / iw;
    const float Z = (float)((double)t.area2 * r);
    const unsigned long long hi = render_key(layer, Z, 0u) >> 32;
    if ((seen >> 32) < hi) return;
    unsigned color = 0xFFu;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 16 - 8 * ch;
        const double c0 = (double)((t.col[0] >> sh) & 255u), c1 = (double)((t.col[1] >> sh) & 255u),
                     c2 = (double)((t.col[2] >> sh) & 255u);
        double v = ((t0 * c0 + t1 * c1) + t2 * c2) * r;
        if (shade) v = v * (double)t.shade;
        v = rint(v);
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);             // NaN cannot arise: iw > 0
        color |= (unsigned)(int)v << (24 - 8 * ch);
    }
    const unsigned long long key = render_key(layer, Z, color);
    if (seen <= key) return;
    atomicMin(px, key);
    ++issued;
}

__device__ __forceinline__ bool render_tri_covers(const RenderTri& t, long long e0, long long e1, long long e2) {
    return e0 + (t.tie & 1) > 0 && e1 + ((t.tie >> 1) & 1) > 0 && e2 + ((t.tie >> 2) & 1) > 0;
}

__device__ __forceinline__ int render_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ long long render_bcast(long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// grid (blocks of triangles, views).  Every lane sets up its own triangle; one whose clipped rectangle has fewer
// than `coop` pixels is filled by that lane, the others are taken by the whole wave one at a time, the set-up
// read from the owning lane and the rectangle's pixels strided over the 64 lanes.  Both routes evaluate the
// same integers and the same f64 expressions per pixel, so the keys do not depend on `coop`.
__global__ void __launch_bounds__(RENDER_BLOCK) k_render_triangles(const float* __restrict__ verts, const uint8_t* __restrict__ rgb,
                                                                   long long n, const int* __restrict__ faces, long long m,
                                                                   const float* __restrict__ cams, RenderCam c, float near_z,
                                                                   float far_z, int cull, int shade, int layer, int coop, int spread,
                                                                   unsigned long long* __restrict__ keys,
                                                                   unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long bstats[6];
    if (stats) {
        if (threadIdx.x < 6) bstats[threadIdx.x] = 0;
        __syncthreads();
    }
    // spread: consecutive triangles go to different waves of the block, so that a mesh of a few dozen large
    // triangles works on all four SIMDs of its CU instead of one; a launch with enough blocks for the chip keeps
    // neighbours in one wave (their faces, vertices and pixels share cache lines)
    const int view = blockIdx.y, lane = bf_lane();
    const long long f = (long long)blockIdx.x * RENDER_BLOCK +
                        (spread ? lane * (RENDER_BLOCK / 64) + (threadIdx.x >> 6) : threadIdx.x);
    unsigned long long* vk = keys + (size_t)view * c.H * c.W;
    RenderTri t;
    t.npx = 0;
    const int fate = f < m ? render_tri_setup(verts, rgb, n, faces + 3 * f, cams + 12 * view, c, near_z, far_z, cull, shade, t)
                           : TRI_NONE;
    unsigned long long covered = 0, issued = 0;
    const bool own = t.npx > 0 && t.npx < coop;
    if (own) {
        const int h = t.npx / t.w;
        for (int j = 0; j < h; ++j) {
            const int iy = t.y0 + j;
            long long e0 = t.C[0] + t.A[0] * t.x0 + t.B[0] * iy, e1 = t.C[1] + t.A[1] * t.x0 + t.B[1] * iy,
                      e2 = t.C[2] + t.A[2] * t.x0 + t.B[2] * iy;
            unsigned long long* row = vk + (size_t)iy * c.W + t.x0;
            for (int i = 0; i < t.w; ++i) {
                if (render_tri_covers(t, e0, e1, e2)) {
                    ++covered;
                    render_tri_pixel(t, e0, e1, e2, shade, layer, render_seen(row + i), row + i, issued);
                }
                e0 += t.A[0], e1 += t.A[1], e2 += t.A[2];
            }
        }
    }
    unsigned long long todo = __ballot(t.npx > 0 && !own);
    while (todo) {                                               // wave-uniform
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        RenderTri b;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            b.A[i] = render_bcast(t.A[i], src), b.B[i] = render_bcast(t.B[i], src), b.C[i] = render_bcast(t.C[i], src);
            b.iz[i] = __longlong_as_double(render_bcast(__double_as_longlong(t.iz[i]), src));
            b.col[i] = (unsigned)render_bcast((int)t.col[i], src);
        }
        b.area2 = render_bcast(t.area2, src);
        b.shade = __int_as_float(render_bcast(__float_as_int(t.shade), src));
        b.x0 = render_bcast(t.x0, src), b.y0 = render_bcast(t.y0, src), b.w = render_bcast(t.w, src);
        b.npx = render_bcast(t.npx, src), b.tie = render_bcast(t.tie, src);
        for (int k = lane; k < b.npx; k += 64) {
            const int j = (int)((unsigned)k / (unsigned)b.w), ix = b.x0 + (k - j * b.w), iy = b.y0 + j;
            const long long e0 = b.C[0] + b.A[0] * ix + b.B[0] * iy, e1 = b.C[1] + b.A[1] * ix + b.B[1] * iy,
                            e2 = b.C[2] + b.A[2] * ix + b.B[2] * iy;
            if (render_tri_covers(b, e0, e1, e2)) {
                unsigned long long* px = vk + (size_t)iy * c.W + ix;
                ++covered;
                render_tri_pixel(b, e0, e1, e2, shade, layer, render_seen(px), px, issued);
            }
        }
    }
    if (stats) {                                                 // wave-uniform: every lane takes part
        long long s[6];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = bf_wave_sum_i32(fate == i);
        s[4] = bf_wave_sum_i64((long long)covered);
        s[5] = bf_wave_sum_i64((long long)issued);
        if (lane == 0)
            for (int i = 0; i < 6; ++i)
                if (s[i]) atomicAdd(bstats + i, (unsigned long long)s[i]);
        __syncthreads();
        if (threadIdx.x < 6 && bstats[threadIdx.x]) atomicAdd(stats + threadIdx.x, bstats[threadIdx.x]);
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

BF_API int bf_render_triangles(const float* vertices, const uint8_t* rgb, long long n, const int32_t* faces, long long m,
                               const float* cams, int V, float fx, float fy, float cx, float cy, int H, int W, float near_z,
                               float far_z, int cull, int shade, int layer, int coop_pixels, void* keys, void* stats,
                               void* stream) {
    if (!render_target_ok(keys, V, H, W) || !render_camera_ok(cams, fx, fy, cx, cy, near_z) || !(far_z > near_z) || n < 0 ||
        m < 0 || (cull != 0 && cull != 1) || (shade != 0 && shade != 1) || (layer != 0 && layer != 1) || coop_pixels < 0)
        return BF_ERR_ARG;
    if (m == 0 || n == 0) return BF_OK;
    if (!vertices || !rgb || !faces) return BF_ERR_ARG;
    const long long nb = (m + RENDER_BLOCK - 1) / RENDER_BLOCK;
    if (nb >= (1ll << 31)) return BF_ERR_CAPACITY;
    const RenderCam c = {fx, fy, cx, cy, H, W};
    const int spread = nb * V < RENDER_SPREAD_BLOCKS;
    hipLaunchKernelGGL(k_render_triangles, dim3((unsigned)nb, (unsigned)V), dim3(RENDER_BLOCK), 0, bf_stream(stream), vertices,
                       rgb, n, (const int*)faces, m, cams, c, near_z, far_z, cull, shade, layer, coop_pixels, spread,
                       (unsigned long long*)keys, (unsigned long long*)stats);
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
