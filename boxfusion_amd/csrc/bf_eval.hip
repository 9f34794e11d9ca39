// bf_eval.hip — scoring a run against ground truth, off the timed path, all arithmetic in f64:
//   bf_gt_frustum     frustum_culling_bbox_level (data_process/filter_gt_boxes.py:24-68): which corners of the
//                     ground-truth boxes project into at least one frame of the sequence
//   bf_nn_min_dist2   the squared distance of every query to its nearest scene point, what
//                     check_bbox_proximity's KDTree query returns (filter_gt_boxes.py:75-93) before the sqrt
//   bf_obb_iou_exact  the true intersection volume and IoU of two oriented boxes: a separating-axis early out
//                     over the six face normals, then the divergence theorem over the twelve face quads, each
//                     clipped by the other box's six half-spaces (Sutherland-Hodgman, at most 10 vertices)
// The file is compiled with contraction off: an expression rounds as it is written.
#include "bf_common.h"

#include <math.h>

// the per-frame and per-face arithmetic is also callable from a host program, so that it can be stepped
// through on a CPU build
#define EV_HD __host__ __device__ __forceinline__

// ---- frustum ----------------------------------------------------------------------------------------------------
#define FR_BLOCK 256
#define FR_CHUNK 64            // poses staged per pass: 64 x 12 f64 = 6 KiB of LDS
#define FR_MAX_GROUPS 32       // pose-chunk groups of the grid (gridDim.y); a block walks every 32nd chunk

// is the world point (X, Y, Z) inside the image of the frame whose inverse pose has rows 0..2 = p[0..11]
EV_HD bool corner_in_frame(const double* p, double X, double Y, double Z, double fx, double fy, double cx, double cy,
                           double Wd, double Hd, double z_near, double z_far) {
    // np.dot(hom_corners, pose_inv.T), filter_gt_boxes.py:42-47
    const double z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
    if (!(z > z_near && z < z_far)) return false;               // both strict; false for a nan / inf pose
    const double x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3];
    const double y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
    // .astype(int) truncates toward zero (:53-54): u in (-1, 0) becomes 0 and counts as inside
    const double u = trunc(fx * x / z + cx);
    const double v = trunc(fy * y / z + cy);
    return u >= 0.0 && u < Wd && v >= 0.0 && v < Hd;
}

// one thread per corner; block (x, y) walks the pose chunks y, y + gridDim.y, ...  `seen` is zeroed by the caller
// and only ever stored 1, so blocks that write the same corner do not race on its value.
__global__ void __launch_bounds__(FR_BLOCK) k_gt_frustum(const double* __restrict__ corners, long long n_corners,
                                                         const double* __restrict__ pose_inv, int M, double fx, double fy,
                                                         double cx, double cy, double Wd, double Hd, double z_near,
                                                         double z_far, uint8_t* __restrict__ seen) {
    __shared__ double sp[FR_CHUNK * 12];
    const long long c = (long long)blockIdx.x * FR_BLOCK + threadIdx.x;
    const bool live = c < n_corners;
    double X = 0.0, Y = 0.0, Z = 0.0;
    if (live) {
        X = corners[3 * c];
        Y = corners[3 * c + 1];
        Z = corners[3 * c + 2];
    }
    bool done = !live;
    const int n_chunks = (M + FR_CHUNK - 1) / FR_CHUNK;
    for (int ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const int m0 = ch * FR_CHUNK;
        const int cnt = M - m0 < FR_CHUNK ? M - m0 : FR_CHUNK;
        __syncthreads();                                        // the previous chunk has been read
        for (int e = threadIdx.x; e < cnt * 12; e += FR_BLOCK)  // rows 0..2 of each 4x4
            sp[e] = pose_inv[(size_t)(m0 + e / 12) * 16 + e % 12];
        __syncthreads();
        if (!done && *(const volatile uint8_t*)(seen + c)) done = true;   // settled by a block of another chunk
        if (!done) {
            for (int m = 0; m < cnt; ++m) {
                if (corner_in_frame(sp + m * 12, X, Y, Z, fx, fy, cx, cy, Wd, Hd, z_near, z_far)) {
                    seen[c] = 1;
                    done = true;
                    break;
                }
            }
        }
        if (__syncthreads_and(done)) break;                     // every corner of the block is settled
    }
}

BF_API int bf_gt_frustum(const double* corners, int N, const double* pose_inv, int M, double fx, double fy, double cx,
                         double cy, int W, int H, double z_near, double z_far, uint8_t* seen, void* stream) {
    if (N < 0 || M < 0 || W <= 0 || H <= 0) return BF_ERR_ARG;
    if (N == 0 || M == 0) return BF_OK;
    if (!corners || !pose_inv || !seen) return BF_ERR_ARG;
    const long long nc = (long long)N * 8;
    const long long gx = (nc + FR_BLOCK - 1) / FR_BLOCK;
    if (gx >= (1ll << 31)) return BF_ERR_CAPACITY;
    const int n_chunks = (M + FR_CHUNK - 1) / FR_CHUNK;
    const unsigned gy = (unsigned)(n_chunks < FR_MAX_GROUPS ? n_chunks : FR_MAX_GROUPS);
    hipLaunchKernelGGL(k_gt_frustum, dim3((unsigned)gx, gy), dim3(FR_BLOCK), 0, bf_stream(stream), corners, nc, pose_inv,
                       M, fx, fy, cx, cy, (double)W, (double)H, z_near, z_far, seen);
    return bf_check_launch();
}

// ---- nearest scene point ----------------------------------------------------------------------------------------
#define NN_BLOCK 256
#define NN_CHUNK 1024          // points staged per pass: 1024 x 3 f64 = 24 KiB of LDS
#define NN_MAX_GROUPS 256      // point-chunk groups of the grid (gridDim.y); a block walks every 256th chunk

// one thread per query, one running minimum per thread; block (x, y) walks the point chunks y, y + gridDim.y, ...
// and the blocks of one query meet in an unsigned 64-bit atomicMin on the bit pattern (non-negative doubles order
// as their bits do; the caller fills d2 with +inf).  A nan distance never wins a comparison and is left out.
__global__ void __launch_bounds__(NN_BLOCK) k_nn_min_dist2(const double* __restrict__ query, int Q,
                                                           const double* __restrict__ points, long long P,
                                                           unsigned long long* __restrict__ d2) {
    __shared__ double sp[NN_CHUNK * 3];
    const int q = blockIdx.x * NN_BLOCK + threadIdx.x;
    const bool live = q < Q;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) {
        qx = query[3 * (size_t)q];
        qy = query[3 * (size_t)q + 1];
        qz = query[3 * (size_t)q + 2];
    }
    double best = __longlong_as_double(0x7FF0000000000000ll);  // +inf
    const long long n_chunks = (P + NN_CHUNK - 1) / NN_CHUNK;
    for (long long ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const long long p0 = ch * NN_CHUNK;
        const int cnt = (int)(P - p0 < NN_CHUNK ? P - p0 : NN_CHUNK);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 3; e += NN_BLOCK) sp[e] = points[p0 * 3 + e];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const double dx = qx - sp[3 * i], dy = qy - sp[3 * i + 1], dz = qz - sp[3 * i + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            best = d < best ? d : best;
        }
    }
    if (live && best < __longlong_as_double(0x7FF0000000000000ll))
        atomicMin(d2 + q, (unsigned long long)__double_as_longlong(best));
}

BF_API int bf_nn_min_dist2(const double* query, int Q, const double* points, long long P, double* d2, void* stream) {
    if (Q < 0 || P < 0) return BF_ERR_ARG;
    if (Q == 0 || P == 0) return BF_OK;
    if (!query || !points || !d2) return BF_ERR_ARG;
    if (P >= (1ll << 40)) return BF_ERR_CAPACITY;
    const unsigned gx = bf_cdiv((unsigned)Q, NN_BLOCK);
    const long long n_chunks = (P + NN_CHUNK - 1) / NN_CHUNK;
    const unsigned gy = (unsigned)(n_chunks < NN_MAX_GROUPS ? n_chunks : NN_MAX_GROUPS);
    hipLaunchKernelGGL(k_nn_min_dist2, dim3(gx, gy), dim3(NN_BLOCK), 0, bf_stream(stream), query, Q, points, P,
                       (unsigned long long*)d2);
    return bf_check_launch();
}

// ---- exact oriented-box IoU ---------------------------------------------------------------------------------------
#define IOU_BLOCK 128          // 8 pairs of 16 lanes: lane f < 6 clips face f of A, 6 <= f < 12 face f - 6 of B
#define IOU_MAXV 10            // a quad cut by six half-spaces has at most 10 vertices

struct v3 {
    double x, y, z;
};
EV_HD v3 ld3(const double* p) { return {p[0], p[1], p[2]}; }
EV_HD v3 operator+(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
EV_HD v3 operator-(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
EV_HD v3 operator*(double s, v3 a) { return {s * a.x, s * a.y, s * a.z}; }
EV_HD double dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
EV_HD v3 cross(v3 a, v3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

#define IOU_SLOTS (IOU_BLOCK / 16 * 12)   // the face lanes of a block
// the polygon of a face lane lives in its own LDS column: word ((buf * IOU_MAXV + vertex) * 3 + axis) * IOU_SLOTS +
// slot, so the face lanes of a wave touch consecutive doubles whatever vertex each of them is at
EV_HD v3 pv_load(const double* s, int buf, int i) {
    const double* p = s + (size_t)((buf * IOU_MAXV + i) * 3) * IOU_SLOTS;
    return {p[0], p[IOU_SLOTS], p[2 * IOU_SLOTS]};
}
EV_HD void pv_store(double* s, int buf, int i, v3 v) {
    double* p = s + (size_t)((buf * IOU_MAXV + i) * 3) * IOU_SLOTS;
    p[0] = v.x;
    p[IOU_SLOTS] = v.y;
    p[2 * IOU_SLOTS] = v.z;
}

// polygon `buf` (m vertices) cut by the half-space n.(X - c) - L <= eps into polygon `buf ^ 1`; returns its count.
// A vertex within eps of the plane is inside, the same band the coplanar test below uses.
EV_HD int clip_plane(double* s, int buf, int m, v3 n, v3 c, double L, double eps) {
    if (m < 3) return 0;
    int mo = 0;
    const v3 first = pv_load(s, buf, 0);
    v3 P = first;
    double sp = dot(n, P - c) - L;
    for (int i = 0; i < m; ++i) {
        const v3 Q = i + 1 < m ? pv_load(s, buf, i + 1) : first;
        const double sq = dot(n, Q - c) - L;
        const bool inp = sp <= eps, inq = sq <= eps;
        if (inp && mo < IOU_MAXV) pv_store(s, buf ^ 1, mo++, P);
        if (inp != inq && mo < IOU_MAXV) {
            const double t = sp / (sp - sq);
            pv_store(s, buf ^ 1, mo++, P + t * (Q - P));
        }
        P = Q;
        sp = sq;
    }
    return mo;
}

// the term of face lane f (f < 6: face f of a, else face f - 6 of b) in the pair's intersection volume, 0 for
// lanes 12..15 and for a separated or empty pair; *VA and *VB get the two volumes.  s: the lane's polygon column.
EV_HD double iou_face_term(const double* pa, const double* pb, int f, double* s, double* VA, double* VB) {
    double contrib = 0.0;
    const v3 ca = ld3(pa), cb = ld3(pb);
    const v3 A0 = ld3(pa + 3), A1 = ld3(pa + 6), A2 = ld3(pa + 9);
    const v3 B0 = ld3(pb + 3), B1 = ld3(pb + 6), B2 = ld3(pb + 9);
    const double LA0 = sqrt(dot(A0, A0)), LA1 = sqrt(dot(A1, A1)), LA2 = sqrt(dot(A2, A2));
    const double LB0 = sqrt(dot(B0, B0)), LB1 = sqrt(dot(B1, B1)), LB2 = sqrt(dot(B2, B2));
    *VA = 8.0 * LA0 * LA1 * LA2;
    *VB = 8.0 * LB0 * LB1 * LB2;
    bool work = *VA > 0.0 && *VB > 0.0;                     // an empty box intersects nothing
    if (work) {
        // separating axis over the six face normals (uniform over the pair's 16 lanes)
        const v3 nA0 = (1.0 / LA0) * A0, nA1 = (1.0 / LA1) * A1, nA2 = (1.0 / LA2) * A2;
        const v3 nB0 = (1.0 / LB0) * B0, nB1 = (1.0 / LB1) * B1, nB2 = (1.0 / LB2) * B2;
        const v3 d = cb - ca;
#define SEP(n, Ln, X0, X1, X2) (fabs(dot(d, n)) >= Ln + ((fabs(dot(n, X0)) + fabs(dot(n, X1))) + fabs(dot(n, X2))))
        if (SEP(nA0, LA0, B0, B1, B2) || SEP(nA1, LA1, B0, B1, B2) || SEP(nA2, LA2, B0, B1, B2) ||
            SEP(nB0, LB0, A0, A1, A2) || SEP(nB1, LB1, A0, A1, A2) || SEP(nB2, LB2, A0, A1, A2))
            work = false;
#undef SEP
        if (work && f < 12) {
            const v3 ha = (A0 + A1) + A2, hb = (B0 + B1) + B2;
            const double da = sqrt(dot(ha, ha)), db = sqrt(dot(hb, hb));
            const double eps = 1e-12 * (da > db ? da : db);
            // this lane's face: axis k and side sg of its own box; the other box cuts it
            const bool ofA = f < 6;
            const int g = ofA ? f : f - 6;
            const int k = g >> 1;
            const double sg = (g & 1) ? -1.0 : 1.0;
            const double* own = ofA ? pa : pb;
            const v3 co = ofA ? ca : cb;                    // own centre
            const v3 cc = ofA ? cb : ca;                    // cutting box: centre, unit normals, half-lengths
            const v3 n0 = ofA ? nB0 : nA0, n1 = ofA ? nB1 : nA1, n2 = ofA ? nB2 : nA2;
            const double L0 = ofA ? LB0 : LA0, L1 = ofA ? LB1 : LA1, L2 = ofA ? LB2 : LA2;
            const v3 Ak = ld3(own + 3 + 3 * k);
            const v3 U = ld3(own + 3 + 3 * ((k + 1) % 3)), V = ld3(own + 3 + 3 * ((k + 2) % 3));
            const v3 n = (sg / sqrt(dot(Ak, Ak))) * Ak;     // outward unit normal
            const v3 pc = co + sg * Ak;                     // face centre
            const v3 q0 = (pc + U) + V, q1 = (pc - U) + V, q2 = (pc - U) - V, q3 = (pc + U) - V;
            // a face of B that lies in a face plane of A with the same outward side is counted by A's lane
            bool skip = false;
            if (!ofA) {
#define COPLANAR(nn, LL, sgn)                                                                                      \
    (sgn * dot(nn, n) > 0.0 && fabs(sgn * dot(nn, q0 - cc) - LL) <= eps && fabs(sgn * dot(nn, q1 - cc) - LL) <= eps && \
     fabs(sgn * dot(nn, q2 - cc) - LL) <= eps && fabs(sgn * dot(nn, q3 - cc) - LL) <= eps)
                skip = COPLANAR(n0, L0, 1.0) || COPLANAR(n0, L0, -1.0) || COPLANAR(n1, L1, 1.0) ||
                       COPLANAR(n1, L1, -1.0) || COPLANAR(n2, L2, 1.0) || COPLANAR(n2, L2, -1.0);
#undef COPLANAR
            }
            if (!skip) {
                pv_store(s, 0, 0, q0);
                pv_store(s, 0, 1, q1);
                pv_store(s, 0, 2, q2);
                pv_store(s, 0, 3, q3);
                int m = 4;
                m = clip_plane(s, 0, m, n0, cc, L0, eps);
                m = clip_plane(s, 1, m, -1.0 * n0, cc, L0, eps);
                m = clip_plane(s, 0, m, n1, cc, L1, eps);
                m = clip_plane(s, 1, m, -1.0 * n1, cc, L1, eps);
                m = clip_plane(s, 0, m, n2, cc, L2, eps);
                m = clip_plane(s, 1, m, -1.0 * n2, cc, L2, eps);   // the result is in buffer 0
                if (m >= 3) {
                    const v3 p0 = pv_load(s, 0, 0);
                    v3 acc = {0.0, 0.0, 0.0};
                    v3 e1 = pv_load(s, 0, 1) - p0;
                    for (int i = 2; i < m; ++i) {
                        const v3 e2 = pv_load(s, 0, i) - p0;
                        acc = acc + cross(e1, e2);
                        e1 = e2;
                    }
                    // divergence theorem about A's centre: height of the face plane x area / 3
                    contrib = dot(n, pc - ca) * (0.5 * fabs(dot(acc, n))) / 3.0;
                }
            }
        }
    }
    return contrib;
}

__global__ void __launch_bounds__(IOU_BLOCK) k_obb_iou_exact(const double* __restrict__ a, const double* __restrict__ b,
                                                             long long n_pairs, int G, double* __restrict__ iou,
                                                             double* __restrict__ inter) {
    __shared__ double poly[2 * IOU_MAXV * 3 * IOU_SLOTS];
    const int f = threadIdx.x & 15;
    double* s = poly + (threadIdx.x >> 4) * 12 + (f < 12 ? f : 0);   // lanes 12..15 never touch it
    const long long pair = (long long)blockIdx.x * (IOU_BLOCK / 16) + (threadIdx.x >> 4);
    const bool live = pair < n_pairs;
    double contrib = 0.0, VA = 0.0, VB = 0.0;
    if (live) contrib = iou_face_term(a + (pair / G) * 12, b + (pair % G) * 12, f, s, &VA, &VB);
    // every lane of the wave is here: sum the pair's 16 lanes in a fixed order
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o, 16);
    if (live && f == 0) {
        const double lim = VA < VB ? VA : VB;
        double vol = contrib > 0.0 ? contrib : 0.0;            // also turns a nan into 0
        vol = vol > lim ? lim : vol;
        const double un = (VA + VB) - vol;
        iou[pair] = un > 0.0 ? vol / un : 0.0;
        if (inter) inter[pair] = vol;
    }
}

BF_API int bf_obb_iou_exact(const double* a, int P, const double* b, int G, double* iou, double* inter, void* stream) {
    if (P < 0 || G < 0) return BF_ERR_ARG;
    if (P == 0 || G == 0) return BF_OK;
    if (!a || !b || !iou) return BF_ERR_ARG;
    const long long pairs = (long long)P * G;
    const long long nb = (pairs + IOU_BLOCK / 16 - 1) / (IOU_BLOCK / 16);
    if (nb >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_obb_iou_exact, dim3((unsigned)nb), dim3(IOU_BLOCK), 0, bf_stream(stream), a, b, pairs, G, iou,
                       inter);
    return bf_check_launch();
}
