// bf_track.hip — camera tracking against the TSDF volume's raycast (bf_tsdf_raycast): projective point-to-plane ICP.
//   bf_depth_vertex_normal  a live depth map as camera-frame vertex and normal maps (f32)
//   bf_icp_reduce           the 6-DoF normal equations of one ICP iteration, summed in a fixed order (f64)
//   bf_grey_u8              the intensity of an RGB image (f32)
//   bf_photo_reduce         the same normal equations of the intensity residual against the last placed frame
// The 6 x 6 solve and the pose update stay on the host (boxfusion_amd/tracking.py).
#include "bf_compact.h"

#define ICP_TERMS 29                     // 21 of J^T J (upper triangle, row by row), 6 of J^T r, sum r^2, inliers
#define ICP_PER_THREAD 4                 // sampled pixels per thread
#define ICP_PER_BLOCK (CLOUD_BLOCK * ICP_PER_THREAD)

// ---- vertex / normal maps of a depth frame --------------------------------------------------------------------------------
// vertex = ((u - cx) * d / fx, (v - cy) * d / fy, d), the unprojection of bf_tsdf_touch; normal = (down - here) x
// (right - here), normalised, which faces the camera (n . vertex <= 0; flipped if it does not).  A pixel is valid
// when 0 < d < max_depth; the normal is 0 where the pixel, its right or its lower neighbour is invalid or differs
// from it by more than `jump` in depth, and in the last row and column.  An invalid pixel's vertex is 0.
__global__ void __launch_bounds__(CLOUD_BLOCK) k_depth_vertex_normal(const float* __restrict__ depth, int H, int W, float fx,
                                                                     float fy, float cx, float cy, float max_depth, float jump,
                                                                     float* __restrict__ vertex, float* __restrict__ normal) {
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int u = (int)(p % W), v = (int)(p / W);
    const float d = depth[p];
    const bool ok = d > 0.f && d < max_depth;                    // NaN fails
    float x = 0.f, y = 0.f, z = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (ok) {
        const float xu = (float)u - cx, yv = (float)v - cy;
        x = xu * d / fx;
        y = yv * d / fy;
        z = d;
        if (u + 1 < W && v + 1 < H) {
            const float dr = depth[p + 1], dd = depth[p + W];
            const bool okr = dr > 0.f && dr < max_depth && fabsf(dr - d) <= jump;
            const bool okd = dd > 0.f && dd < max_depth && fabsf(dd - d) <= jump;
            if (okr && okd) {
                const float ax = (xu + 1.0f) * dr / fx - x, ay = yv * dr / fy - y, az = dr - d;        // right - here
                const float bx = xu * dd / fx - x, by = (yv + 1.0f) * dd / fy - y, bz = dd - d;        // down - here
                float cx_ = by * az - bz * ay, cy_ = bz * ax - bx * az, cz_ = bx * ay - by * ax;       // b x a
                const float len = sqrtf(cx_ * cx_ + cy_ * cy_ + cz_ * cz_);
                if (len > 0.f) {
                    cx_ = cx_ / len;
                    cy_ = cy_ / len;
                    cz_ = cz_ / len;
                    if (cx_ * x + cy_ * y + cz_ * z > 0.f) {
                        cx_ = -cx_;
                        cy_ = -cy_;
                        cz_ = -cz_;
                    }
                    nx = cx_;
                    ny = cy_;
                    nz = cz_;
                }
            }
        }
    }
    vertex[p * 3] = x;
    vertex[p * 3 + 1] = y;
    vertex[p * 3 + 2] = z;
    normal[p * 3] = nx;
    normal[p * 3 + 1] = ny;
    normal[p * 3 + 2] = nz;
}

BF_API int bf_depth_vertex_normal(const float* depth, int H, int W, float fx, float fy, float cx, float cy, float max_depth,
                                  float jump, float* vertex, float* normal, void* stream) {
    if (!depth || !vertex || !normal || H <= 0 || W <= 0 || !(fx > 0.f) || !(fy > 0.f) || !(max_depth > 0.f) || !(jump >= 0.f))
        return BF_ERR_ARG;
    const long long hw = (long long)H * W;
    if (hw >= (1ll << 31) / 3) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_depth_vertex_normal, dim3((unsigned)((hw + CLOUD_BLOCK - 1) / CLOUD_BLOCK)), dim3(CLOUD_BLOCK), 0,
                       bf_stream(stream), depth, H, W, fx, fy, cx, cy, max_depth, jump, vertex, normal);
    return bf_check_launch();
}

// ---- the normal equations ----------------------------------------------------------------------------------------------
// Sampled pixel k = i * Ws + j (Hs = ceil(H / stride), Ws = ceil(W / stride)) is live pixel (stride i, stride j).
// Block b and thread t own k = b * 1024 + m * 256 + t, m = 0 .. 3, added in that order; then a butterfly over the
// wave's 64 lanes (xor 32, 16, .. 1: every lane ends with the same sum, formed in the same order), the block's
// four waves in wave order through LDS, and k_icp_final sums the blocks' rows the same way.  No floating-point
// atomics: the grid depends on (H, W, stride) alone, so the sums are the same bits on every run and device.
struct IcpArgs {
    double T[12];                        // the estimate, camera -> world, rows of [R | t]
    double M[12];                        // the model camera, world -> camera
    double fx, fy, cx, cy;               // the model camera's pinhole
    double dist2_max, cos_min;
};

__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// acc (per thread) -> row (32 doubles); every thread of the block must call
__device__ __forceinline__ void icp_block_sum(double* acc, double* __restrict__ row) {
    __shared__ double part[CLOUD_WAVES][BF_ICP_ROW];
#pragma unroll
    for (int i = 0; i < ICP_TERMS; ++i) {
        const double s = icp_wave_sum(acc[i]);
        if (bf_lane() == 0) part[threadIdx.x >> 6][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < BF_ICP_ROW) {
        double s = 0.0;
        if (threadIdx.x < ICP_TERMS) {
            s = part[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < CLOUD_WAVES; ++w) s += part[w][threadIdx.x];
        }
        row[threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(CLOUD_BLOCK) k_icp_reduce(const float* __restrict__ lv, const float* __restrict__ ln, int H,
                                                            int W, int stride, int Ws, int n, const float* __restrict__ mv,
                                                            const float* __restrict__ mn, int Hm, int Wm, IcpArgs A,
                                                            double* __restrict__ partials) {
    double acc[ICP_TERMS];
#pragma unroll
    for (int i = 0; i < ICP_TERMS; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int m = 0; m < ICP_PER_THREAD; ++m) {
        const long long k = (long long)blockIdx.x * ICP_PER_BLOCK + m * CLOUD_BLOCK + threadIdx.x;
        if (k >= n) continue;
        const int i = (int)(k / Ws), j = (int)(k - (long long)i * Ws);
        const size_t lp = ((size_t)i * stride * W + (size_t)j * stride) * 3;
        const double nlx = ln[lp], nly = ln[lp + 1], nlz = ln[lp + 2];
        if (nlx == 0.0 && nly == 0.0 && nlz == 0.0) continue;
        const double x = lv[lp], y = lv[lp + 1], z = lv[lp + 2];
        const double px = A.T[0] * x + A.T[1] * y + A.T[2] * z + A.T[3];
        const double py = A.T[4] * x + A.T[5] * y + A.T[6] * z + A.T[7];
        const double pz = A.T[8] * x + A.T[9] * y + A.T[10] * z + A.T[11];
        const double qz = A.M[8] * px + A.M[9] * py + A.M[10] * pz + A.M[11];
        if (!(qz > 0.0)) continue;
        const double qx = A.M[0] * px + A.M[1] * py + A.M[2] * pz + A.M[3];
        const double qy = A.M[4] * px + A.M[5] * py + A.M[6] * pz + A.M[7];
        const double fu = floor(A.fx * qx / qz + A.cx + 0.5), fv = floor(A.fy * qy / qz + A.cy + 0.5);
        if (!(fu >= 0.0 && fu < (double)Wm && fv >= 0.0 && fv < (double)Hm)) continue;
        const size_t mp = ((size_t)(int)fv * Wm + (size_t)(int)fu) * 3;
        const double nx = mn[mp], ny = mn[mp + 1], nz = mn[mp + 2];
        if (nx == 0.0 && ny == 0.0 && nz == 0.0) continue;
        const double ex = (double)mv[mp] - px, ey = (double)mv[mp + 1] - py, ez = (double)mv[mp + 2] - pz;
        if (!(ex * ex + ey * ey + ez * ez <= A.dist2_max)) continue;
        const double rx = A.T[0] * nlx + A.T[1] * nly + A.T[2] * nlz, ry = A.T[4] * nlx + A.T[5] * nly + A.T[6] * nlz,
                     rz = A.T[8] * nlx + A.T[9] * nly + A.T[10] * nlz;
        if (!(rx * nx + ry * ny + rz * nz >= A.cos_min)) continue;
        const double r = nx * ex + ny * ey + nz * ez;
        const double J0 = py * nz - pz * ny, J1 = pz * nx - px * nz, J2 = px * ny - py * nx;
        const double J[6] = {J0, J1, J2, nx, ny, nz};
        int at = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[at++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
        acc[27] += r * r;
        acc[28] += 1.0;
    }
    icp_block_sum(acc, partials + (size_t)blockIdx.x * BF_ICP_ROW);
}

__global__ void __launch_bounds__(CLOUD_BLOCK) k_icp_final(const double* __restrict__ partials, int blocks,
                                                           double* __restrict__ out) {
    double acc[ICP_TERMS];
#pragma unroll
    for (int i = 0; i < ICP_TERMS; ++i) acc[i] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += CLOUD_BLOCK) {
        const double* row = partials + (size_t)b * BF_ICP_ROW;
#pragma unroll
        for (int i = 0; i < ICP_TERMS; ++i) acc[i] += row[i];
    }
    icp_block_sum(acc, out);
}

BF_API int bf_icp_blocks(int H, int W, int stride) {
    if (H <= 0 || W <= 0 || stride <= 0) return 0;
    const long long n = (long long)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
    const long long blocks = (n + ICP_PER_BLOCK - 1) / ICP_PER_BLOCK;
    return blocks >= (1ll << 31) ? 0 : (int)blocks;
}

BF_API int bf_icp_reduce(const float* live_vertex, const float* live_normal, int H, int W, int stride, const double* T,
                         const float* model_vertex, const float* model_normal, int Hm, int Wm, const double* model_w2c,
                         double fx, double fy, double cx, double cy, double dist_max, double cos_min, double* partials,
                         double* out, void* stream) {
    if (!live_vertex || !live_normal || !T || !model_vertex || !model_normal || !model_w2c || !partials || !out || H <= 0 ||
        W <= 0 || stride <= 0 || Hm <= 0 || Wm <= 0 || !(fx > 0.0) || !(fy > 0.0) || !(dist_max >= 0.0))
        return BF_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) / 3 || (long long)Hm * Wm >= (1ll << 31) / 3) return BF_ERR_CAPACITY;
    const int blocks = bf_icp_blocks(H, W, stride);
    if (blocks <= 0) return BF_ERR_CAPACITY;
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    IcpArgs A;
    for (int i = 0; i < 12; ++i) {
        A.T[i] = T[i];
        A.M[i] = model_w2c[i];
    }
    A.fx = fx;
    A.fy = fy;
    A.cx = cx;
    A.cy = cy;
    A.dist2_max = dist_max * dist_max;
    A.cos_min = cos_min;
    hipStream_t st = bf_stream(stream);
    hipLaunchKernelGGL(k_icp_reduce, dim3((unsigned)blocks), dim3(CLOUD_BLOCK), 0, st, live_vertex, live_normal, H, W, stride,
                       Ws, Hs * Ws, model_vertex, model_normal, Hm, Wm, A, partials);
    hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(CLOUD_BLOCK), 0, st, (const double*)partials, blocks, out);
    return bf_check_launch();
}

// ---- the photometric row -------------------------------------------------------------------------------------------
// I = (float)((77 R + 150 G + 29 B + 128) >> 8) / 255.0f, one thread per pixel
__global__ void __launch_bounds__(CLOUD_BLOCK) k_grey_u8(const uint8_t* __restrict__ rgb, long long n, float* __restrict__ out) {
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int y = (77 * (int)rgb[p * 3] + 150 * (int)rgb[p * 3 + 1] + 29 * (int)rgb[p * 3 + 2] + 128) >> 8;
    out[p] = (float)y / 255.0f;
}

BF_API int bf_grey_u8(const uint8_t* rgb, int B, int H, int W, float* out, void* stream) {
    if (!rgb || !out || B <= 0 || H <= 0 || W <= 0) return BF_ERR_ARG;
    const long long n = (long long)B * H * W;
    if ((long long)H * W >= (1ll << 31) / 3 || n >= (1ll << 31) / 3) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_grey_u8, dim3((unsigned)((n + CLOUD_BLOCK - 1) / CLOUD_BLOCK)), dim3(CLOUD_BLOCK), 0, bf_stream(stream),
                       rgb, n, out);
    return bf_check_launch();
}

// The intensity residual of the live frame against the last placed frame (the reference: its intensity, its sensor
// depth, its camera M), with k_icp_reduce's pixel-to-thread assignment, sums and layout.  Per sample: p = T v,
// q = M p, (u, w) its pixel in the reference; c the bilinear intensity there and (gx, gy) that interpolant's own
// derivative; r = I_live - c, J = [p x g, g] with g = R_M^T (gx fx / qz, gy fy / qz, -(gx fx qx + gy fy qy) / qz^2).
// The four taps lie inside the reference when 0 <= floor(u) <= Wr - 2 and 0 <= floor(w) <= Hr - 2, and then so does
// the nearest pixel (floor(u + 0.5) <= floor(u) + 1): that gate comes before every reference load.
struct PhotoArgs {
    double T[12];                        // the estimate, camera -> world
    double M[12];                        // the reference camera, world -> camera
    double fx, fy, cx, cy;
    double dist_max, intensity_max;
};

__global__ void __launch_bounds__(CLOUD_BLOCK) k_photo_reduce(const float* __restrict__ lv, const float* __restrict__ li, int H,
                                                              int W, int stride, int Ws, int n, const float* __restrict__ ri,
                                                              const float* __restrict__ rd, int Hr, int Wr, PhotoArgs A,
                                                              double* __restrict__ partials) {
    double acc[ICP_TERMS];
#pragma unroll
    for (int i = 0; i < ICP_TERMS; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int m = 0; m < ICP_PER_THREAD; ++m) {
        const long long k = (long long)blockIdx.x * ICP_PER_BLOCK + m * CLOUD_BLOCK + threadIdx.x;
        if (k >= n) continue;
        const int i = (int)(k / Ws), j = (int)(k - (long long)i * Ws);
        const size_t lp = (size_t)i * stride * W + (size_t)j * stride;
        const double z = lv[lp * 3 + 2];
        if (!(z > 0.0)) continue;
        const double x = lv[lp * 3], y = lv[lp * 3 + 1];
        const double px = A.T[0] * x + A.T[1] * y + A.T[2] * z + A.T[3];
        const double py = A.T[4] * x + A.T[5] * y + A.T[6] * z + A.T[7];
        const double pz = A.T[8] * x + A.T[9] * y + A.T[10] * z + A.T[11];
        const double qz = A.M[8] * px + A.M[9] * py + A.M[10] * pz + A.M[11];
        if (!(qz > 0.0)) continue;
        const double qx = A.M[0] * px + A.M[1] * py + A.M[2] * pz + A.M[3];
        const double qy = A.M[4] * px + A.M[5] * py + A.M[6] * pz + A.M[7];
        const double u = A.fx * qx / qz + A.cx, w = A.fy * qy / qz + A.cy;
        const double u0 = floor(u), w0 = floor(w);
        if (!(u0 >= 0.0 && u0 <= (double)(Wr - 2) && w0 >= 0.0 && w0 <= (double)(Hr - 2))) continue;       // NaN fails
        const size_t rp = (size_t)(int)w0 * Wr + (size_t)(int)u0;
        const double dr = rd[(size_t)(int)floor(w + 0.5) * Wr + (size_t)(int)floor(u + 0.5)];
        if (!(dr > 0.0 && fabs(dr - qz) <= A.dist_max)) continue;
        const double fu = u - u0, fv = w - w0;
        const double i00 = ri[rp], i10 = ri[rp + 1], i01 = ri[rp + Wr], i11 = ri[rp + Wr + 1];
        const double top = i00 + fu * (i10 - i00), bot = i01 + fu * (i11 - i01);
        const double c = top + fv * (bot - top);
        const double gx = (i10 - i00) + fv * ((i11 - i01) - (i10 - i00));
        const double gy = (i01 - i00) + fu * ((i11 - i10) - (i01 - i00));
        const double r = (double)li[lp] - c;
        if (!(fabs(r) <= A.intensity_max)) continue;
        const double a = gx * A.fx, b = gy * A.fy;
        const double h0 = a / qz, h1 = b / qz, h2 = -(a * qx + b * qy) / (qz * qz);
        const double g0 = A.M[0] * h0 + A.M[4] * h1 + A.M[8] * h2, g1 = A.M[1] * h0 + A.M[5] * h1 + A.M[9] * h2,
                     g2 = A.M[2] * h0 + A.M[6] * h1 + A.M[10] * h2;
        const double J[6] = {py * g2 - pz * g1, pz * g0 - px * g2, px * g1 - py * g0, g0, g1, g2};
        int at = 0;
#pragma unroll
        for (int a_ = 0; a_ < 6; ++a_)
#pragma unroll
            for (int b_ = a_; b_ < 6; ++b_) acc[at++] += J[a_] * J[b_];
#pragma unroll
        for (int a_ = 0; a_ < 6; ++a_) acc[21 + a_] += J[a_] * r;
        acc[27] += r * r;
        acc[28] += 1.0;
    }
    icp_block_sum(acc, partials + (size_t)blockIdx.x * BF_ICP_ROW);
}

BF_API int bf_photo_reduce(const float* live_vertex, const float* live_intensity, int H, int W, int stride, const double* T,
                           const float* ref_intensity, const float* ref_depth, int Hr, int Wr, const double* ref_w2c, double fx,
                           double fy, double cx, double cy, double dist_max, double intensity_max, double* partials,
                           double* out, void* stream) {
    if (!live_vertex || !live_intensity || !T || !ref_intensity || !ref_depth || !ref_w2c || !partials || !out || H <= 0 ||
        W <= 0 || stride <= 0 || Hr <= 0 || Wr <= 0 || !(fx > 0.0) || !(fy > 0.0) || !(dist_max >= 0.0) ||
        !(intensity_max >= 0.0))
        return BF_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) / 3 || (long long)Hr * Wr >= (1ll << 31) / 3) return BF_ERR_CAPACITY;
    const int blocks = bf_icp_blocks(H, W, stride);
    if (blocks <= 0) return BF_ERR_CAPACITY;
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    PhotoArgs A;
    for (int i = 0; i < 12; ++i) {
        A.T[i] = T[i];
        A.M[i] = ref_w2c[i];
    }
    A.fx = fx;
    A.fy = fy;
    A.cx = cx;
    A.cy = cy;
    A.dist_max = dist_max;
    A.intensity_max = intensity_max;
    hipStream_t st = bf_stream(stream);
    hipLaunchKernelGGL(k_photo_reduce, dim3((unsigned)blocks), dim3(CLOUD_BLOCK), 0, st, live_vertex, live_intensity, H, W,
                       stride, Ws, Hs * Ws, ref_intensity, ref_depth, Hr, Wr, A, partials);
    hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(CLOUD_BLOCK), 0, st, (const double*)partials, blocks, out);
    return bf_check_launch();
}
