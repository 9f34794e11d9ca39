// bf_tsdf.hip — the scene mesh: a sparse truncated-signed-distance volume fused from posed depth frames, and a
// naive-surface-nets extractor over it (the reference leaves mesh.ply to open3d, data_process/README.md:48):
//   bf_tsdf_touch          the 8x8x8-voxel blocks within the truncation band of every valid depth pixel, claimed in
//                          an open-addressing hash map (map_find of bf_compact.h) and marked with the frame's bit
//   bf_tsdf_update         the touched blocks compacted (count / scan / scatter), then one workgroup per block and
//                          one thread per voxel: every frame whose bit is set is projected into and added
//   bf_tsdf_extract        the occupied slots, compacted (in slot order)
//   bf_tsdf_surface_count  over the key-sorted blocks: the cells that get a vertex, the grid edges that get a quad,
//   bf_tsdf_surface_write  their scans, and the vertices / triangles written at the scanned positions
//   bf_tsdf_raycast        the volume read back from a pose: one ray per pixel marched through the blocks to the
//                          surface, as depth / vertex / normal / colour maps (what bf_track.hip aligns a frame to)
// The volume is three arrays over `capacity` slots: keys u64 (the key of the block's three indices;
// BF_KEY_EMPTY = empty), touched u64 (bit f = frame f of the launch in flight reaches this block) and vox
// int32 [capacity, BF_TSDF_FIELDS, BF_TSDF_VOX]: per voxel (x fastest, then y, then z)
//   field 0  w      observations          <= max_weight <= 2^20
//   field 1  sum q  q = rint(min(sdf / trunc, 1) * 1024) in [-1024, 1024], |sum| <= 2^30
//   field 2  cw     coloured observations <= w
//   field 3-5  sum r, g, b                <= 255 * 2^20 < 2^28
// Integers only: adds commute, so the volume after a set of frames is the same bits whatever the frame order or
// batching, as long as no voxel reached max_weight (such a voxel refuses the observation, counted in `saturated`).
#include "bf_compact.h"

#define TSDF_BLOCK_WORDS (BF_TSDF_VOX * BF_TSDF_FIELDS)
#define TSDF_UPDATE_GRID 2048

// ---- touch: one thread per depth pixel, blockIdx.x = frame * bpf + the frame's block -------------------------------
__global__ void __launch_bounds__(CLOUD_BLOCK) k_tsdf_touch(const float* __restrict__ depth, const float* __restrict__ poses,
                                                            int hw, int W, int bpf, float fx, float fy, float cx, float cy,
                                                            float voxel, int T, float max_depth, u64* __restrict__ keys,
                                                            u64* __restrict__ touched, u64 mask, u64* __restrict__ stats) {
    __shared__ unsigned bstats[BF_STATS_WORDS];
    const int f = blockIdx.x / bpf, j = blockIdx.x - f * bpf;
    const float* P = poses + 16 * f;
    if (!bf_pose_finite(P)) {                                    // the whole frame, so the whole block: lost tracking
        if (j == 0 && threadIdx.x == 0) atomicAdd(stats + BF_TSDF_STAT_SKIPPED_POSE, 1ull);
        return;
    }
    stats_begin(bstats);
    const int p = j * CLOUD_BLOCK + threadIdx.x;
    const int lane = bf_lane();
    float d = p < hw ? depth[(size_t)f * hw + p] : 0.f;
    const bool live = d > 0.f && d < max_depth;                  // NaN fails
    const float xu = (float)(p % W) - cx, yv = (float)(p / W) - cy;
    const float bs = 8.0f * voxel;
    const u64 bit = 1ull << f;
    u64 prev_key = BF_KEY_EMPTY;                                 // the key this thread handled last
    for (int k = -T; k <= T; ++k) {
        u64 key = BF_KEY_EMPTY;
        bool out_of_range = false;
        if (live) {
            const float z = d + (float)k * voxel;
            const float xc = xu * z / fx, yc = yv * z / fy;
            const float bx = floorf((P[0] * xc + P[1] * yc + P[2] * z + P[3]) / bs);
            const float by = floorf((P[4] * xc + P[5] * yc + P[6] * z + P[7]) / bs);
            const float bz = floorf((P[8] * xc + P[9] * yc + P[10] * z + P[11]) / bs);
            if (key_in_range(bx, by, bz))
                key = key_pack((int)bx, (int)by, (int)bz);
            else
                out_of_range = true;
        }
        stat_add(bstats, BF_TSDF_STAT_OUT_OF_RANGE, out_of_range);
        // equal keys merge over this thread's adjacent samples and over adjacent lanes: one probe per run
        const u64 want = key != prev_key ? key : BF_KEY_EMPTY;
        const u64 left = __shfl_up(want, 1, 64);
        const bool head = want != BF_KEY_EMPTY && (lane == 0 || left != want);
        bool claimed = false, dropped = false;
        if (head) {
            const long long slot = map_find<1>(keys, mask, want, &claimed);
            if (slot >= 0)
                atomicOr(touched + slot, bit);
            else
                dropped = true;
        }
        stat_add(bstats, BF_TSDF_STAT_BLOCKS, claimed);
        stat_add(bstats, BF_TSDF_STAT_DROPPED_FULL, dropped);
        if (key != BF_KEY_EMPTY) prev_key = key;
    }
    stats_flush(bstats, stats);
}

BF_API int bf_tsdf_touch(const float* depth, const float* poses, int B, int H, int W, float fx, float fy, float cx,
                         float cy, float voxel, int trunc_voxels, float max_depth, void* keys, void* touched,
                         long long capacity, void* stats, void* stream) {
    if (!depth || !poses || !keys || !touched || !stats || B <= 0 || B > BF_TSDF_MAX_FRAMES || H <= 0 || W <= 0 ||
        capacity <= 0 || (capacity & (capacity - 1)) || !(voxel > 0.f) || trunc_voxels < 1 ||
        trunc_voxels > BF_TSDF_MAX_TRUNC || !(max_depth > 0.f) || !(fx > 0.f) || !(fy > 0.f))
        return BF_ERR_ARG;
    const long long hw = (long long)H * W;
    const long long bpf = (hw + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
    if (capacity >= (1ll << 31) || hw * B >= (1ll << 31) || bpf * B >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_tsdf_touch, dim3((unsigned)(bpf * B)), dim3(CLOUD_BLOCK), 0, bf_stream(stream), depth, poses,
                       (int)hw, W, (int)bpf, fx, fy, cx, cy, voxel, trunc_voxels, max_depth, (u64*)keys, (u64*)touched,
                       (u64)(capacity - 1), (u64*)stats);
    return bf_check_launch();
}

// ---- compaction (bf_compact.h) of the slots whose word is not `none`: the touched blocks (touched words, none = 0) or
// the occupied ones (keys, none = EMPTY; key_out then takes the key beside the slot)
struct SlotSel {                                                 // thread t of block b = slot b * CLOUD_BLOCK + t
    const u64* words;
    long long cap;
    u64 none;
    int* slot_out;
    long long* key_out;
    __device__ bool selected(unsigned b, unsigned t) const {
        const long long s = (long long)b * CLOUD_BLOCK + t;
        return s < cap && words[s] != none;
    }
    __device__ void write(unsigned b, unsigned t, size_t row) const {
        const long long s = (long long)b * CLOUD_BLOCK + t;
        slot_out[row] = (int)s;
        if (key_out) key_out[row] = (long long)words[s];
    }
};

// ---- update: a workgroup per touched block, a thread per voxel -----------------------------------------------------------
__global__ void __launch_bounds__(BF_TSDF_VOX) k_tsdf_update(const float* __restrict__ depth,
                                                          const uint8_t* __restrict__ rgb,
                                                          const float* __restrict__ poses, int B, int H, int W, float fx, float fy,
                                                          float cx, float cy, float voxel, int T, float max_depth,
                                                          int max_weight, const u64* __restrict__ keys,
                                                          u64* __restrict__ touched,
                                                          int* __restrict__ vox, const int* __restrict__ list,
                                                          const int* __restrict__ n_list, u64* __restrict__ stats) {
    __shared__ unsigned bstats[BF_STATS_WORDS];
    stats_begin(bstats);
    const int t = threadIdx.x;
    const int n = *n_list;
    const float trunc = (float)T * voxel;
    const size_t hw = (size_t)H * W;
    unsigned n_obs = 0, n_sat = 0;
    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        const int slot = list[b];
        const u64 key = keys[slot];
        u64 word = touched[slot] & (B < 64 ? (1ull << B) - 1ull : ~0ull);     // the frames of this launch only
        const int ix = key_axis(key, 0) * 8 + (t & 7);
        const int iy = key_axis(key, 1) * 8 + ((t >> 3) & 7);
        const int iz = key_axis(key, 2) * 8 + (t >> 6);
        const float px = ((float)ix + 0.5f) * voxel, py = ((float)iy + 0.5f) * voxel, pz = ((float)iz + 0.5f) * voxel;
        int* vb = vox + (size_t)slot * TSDF_BLOCK_WORDS + t;
        int w = vb[0], sq = vb[BF_TSDF_VOX], cw = vb[2 * BF_TSDF_VOX], sr = vb[3 * BF_TSDF_VOX], sg = vb[4 * BF_TSDF_VOX],
            sb = vb[5 * BF_TSDF_VOX];
        while (word) {
            const int f = __ffsll((long long)word) - 1;          // the same in every thread of the workgroup
            word &= word - 1;
            const float* P = poses + 16 * f;
            const float dx = px - P[3], dy = py - P[7], dz = pz - P[11];
            const float z = P[2] * dx + P[6] * dy + P[10] * dz;
            if (!(z > 0.f)) continue;
            const float x = P[0] * dx + P[4] * dy + P[8] * dz, y = P[1] * dx + P[5] * dy + P[9] * dz;
            const float fu = floorf(fx * x / z + cx + 0.5f), fv = floorf(fy * y / z + cy + 0.5f);
            if (!(fu >= 0.f && fu < (float)W && fv >= 0.f && fv < (float)H)) continue;
            const size_t pix = (size_t)f * hw + (size_t)(int)fv * W + (int)fu;
            const float d = depth[pix];
            if (!(d > 0.f && d < max_depth)) continue;
            const float sdf = d - z;
            if (sdf < -trunc) continue;
            if (w >= max_weight) {
                ++n_sat;
                continue;
            }
            sq += (int)rintf(fminf(sdf / trunc, 1.0f) * 1024.0f);
            w += 1;
            ++n_obs;
            if (rgb && sdf <= trunc) {
                const uint8_t* c = rgb + pix * 3;
                sr += c[0];
                sg += c[1];
                sb += c[2];
                cw += 1;
            }
        }
        vb[0] = w;
        vb[BF_TSDF_VOX] = sq;
        vb[2 * BF_TSDF_VOX] = cw;
        vb[3 * BF_TSDF_VOX] = sr;
        vb[4 * BF_TSDF_VOX] = sg;
        vb[5 * BF_TSDF_VOX] = sb;
        __syncthreads();                                         // every thread has read the word
        if (t == 0) touched[slot] = 0;
    }
    n_obs = (unsigned)bf_wave_sum_i32((int)n_obs);
    n_sat = (unsigned)bf_wave_sum_i32((int)n_sat);
    if (bf_lane() == 0) {
        if (n_obs) atomicAdd(bstats + BF_TSDF_STAT_OBSERVATIONS, n_obs);
        if (n_sat) atomicAdd(bstats + BF_TSDF_STAT_SATURATED, n_sat);
    }
    stats_flush(bstats, stats);
}

BF_API int bf_tsdf_update(const float* depth, const uint8_t* rgb, const float* poses, int B, int H, int W, float fx,
                          float fy, float cx, float cy, float voxel, int trunc_voxels, float max_depth, int max_weight,
                          const void* keys, void* touched, int32_t* vox, long long capacity, int* list, int* n_list,
                          int* block_counts, void* stats, void* stream) {
    if (!depth || !poses || !keys || !touched || !vox || !list || !n_list || !block_counts || !stats || B <= 0 ||
        B > BF_TSDF_MAX_FRAMES || H <= 0 || W <= 0 || capacity <= 0 || (capacity & (capacity - 1)) || !(voxel > 0.f) ||
        trunc_voxels < 1 || trunc_voxels > BF_TSDF_MAX_TRUNC || !(max_depth > 0.f) || max_weight < 1 ||
        max_weight > BF_TSDF_MAX_WEIGHT || !(fx > 0.f) || !(fy > 0.f))
        return BF_ERR_ARG;
    if (capacity >= (1ll << 31) || (long long)H * W * B >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipStream_t st = bf_stream(stream);
    compact<SlotSel>(compact_blocks(capacity), block_counts, 0, n_list, 0, st, (const u64*)touched, capacity, (u64)0, list,
                     (long long*)nullptr);
    // the list's length is on the device: enough workgroups to fill the machine twice over stride over it
    const unsigned grid = (unsigned)(capacity < TSDF_UPDATE_GRID ? capacity : TSDF_UPDATE_GRID);
    hipLaunchKernelGGL(k_tsdf_update, dim3(grid), dim3(BF_TSDF_VOX), 0, st, depth, rgb, poses, B, H, W, fx, fy, cx, cy, voxel,
                       trunc_voxels, max_depth, max_weight, (const u64*)keys, (u64*)touched, (int*)vox, (const int*)list,
                       (const int*)n_list, (u64*)stats);
    return bf_check_launch();
}

BF_API int bf_tsdf_extract(const void* keys, long long capacity, int64_t* key, int* slot, int* n_out, int* block_counts,
                           void* stream) {
    if (!keys || !key || !slot || !n_out || !block_counts || capacity <= 0) return BF_ERR_ARG;
    if (capacity >= (1ll << 31)) return BF_ERR_CAPACITY;
    compact<SlotSel>(compact_blocks(capacity), block_counts, 0, n_out, 0, bf_stream(stream), (const u64*)keys, capacity,
                     (u64)BF_KEY_EMPTY, slot, (long long*)key);
    return bf_check_launch();
}

// ---- naive surface nets over the key-sorted blocks -------------------------------------------------------------------------
// A block's cells are the 8^3 cubes whose minimum corner is one of its voxel centres; their corners are the
// block's own samples and the low faces of the seven blocks towards +x / +y / +z.
// bit 25 of a staged sample's word: w > 0; bit 24: cw > 0; bits 0-23: the rounded mean colour
#define SURF_EDGE 9
#define SURF_SAMPLES (SURF_EDGE * SURF_EDGE * SURF_EDGE)

// WRITE = false: bitmap [n,8] (bit c of word z: cell (c & 7, c >> 3, z) gets a vertex), eflags [n,512] (bits 0-2:
// the cell's edge from its minimum corner along x / y / z changes sign; bit 3: that corner is inside), vcount [n],
// rank_of_slot.  WRITE = true: the vertices at vcount (now the exclusive prefix) + the cell's rank.
template <bool WRITE>
__global__ void __launch_bounds__(BF_TSDF_VOX) k_tsdf_cells(const u64* __restrict__ keys, u64 mask, const int* __restrict__ vox,
                                                         const long long* __restrict__ skey, const int* __restrict__ sslot,
                                                         int* __restrict__ rank_of_slot, u64* __restrict__ bitmap,
                                                         uint8_t* __restrict__ eflags, int* __restrict__ vcount, float voxel,
                                                         float* __restrict__ verts, uint8_t* __restrict__ vrgb) {
    __shared__ float s_val[SURF_SAMPLES];
    __shared__ unsigned s_tag[SURF_SAMPLES];
    __shared__ int nslot[8];
    __shared__ int wave_n[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const u64 key = (u64)skey[b];
    if (t < 8) {
        int s = sslot[b];
        if (t) {
            const u64 nk = key_neighbour(key, t & 1, (t >> 1) & 1, t >> 2);
            s = nk == BF_KEY_EMPTY ? -1 : map_lookup(keys, mask, nk);
        }
        nslot[t] = s;
    }
    __syncthreads();
    for (int j = t; j < SURF_SAMPLES; j += BF_TSDF_VOX) {
        const int x = j % SURF_EDGE, y = (j / SURF_EDGE) % SURF_EDGE, z = j / (SURF_EDGE * SURF_EDGE);
        const int s = nslot[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
        float val = 0.f;
        unsigned tag = 0;
        if (s >= 0) {
            const int* v = vox + (size_t)s * TSDF_BLOCK_WORDS + ((x & 7) | ((y & 7) << 3) | ((z & 7) << 6));
            const int w = v[0];
            if (w > 0) {
                val = (float)v[BF_TSDF_VOX] / (float)w;
                tag = 1u << 25;
                const int cw = v[2 * BF_TSDF_VOX];
                if (cw > 0) {
                    const unsigned h = (unsigned)cw >> 1, c = (unsigned)cw;
                    tag |= (1u << 24) | (((unsigned)v[3 * BF_TSDF_VOX] + h) / c) |
                           ((((unsigned)v[4 * BF_TSDF_VOX] + h) / c) << 8) | ((((unsigned)v[5 * BF_TSDF_VOX] + h) / c) << 16);
                }
            }
        }
        s_val[j] = val;
        s_tag[j] = tag;
    }
    __syncthreads();
    const int x = t & 7, y = (t >> 3) & 7, z = t >> 6;
    const int base = x + SURF_EDGE * y + SURF_EDGE * SURF_EDGE * z;
    float sv[8];
    unsigned tg[8];
    bool valid = true;
    int n_in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int j = base + (c & 1) + SURF_EDGE * ((c >> 1) & 1) + SURF_EDGE * SURF_EDGE * (c >> 2);
        sv[c] = s_val[j];
        tg[c] = s_tag[j];
        valid = valid && (tg[c] >> 25);
        n_in += sv[c] < 0.f;
    }
    const bool active = valid && n_in > 0 && n_in < 8;
    const u64 m = __ballot(active);
    if (bf_lane() == 0) wave_n[z] = __popcll(m);
    __syncthreads();
    if (!WRITE) {
        if (bf_lane() == 0) bitmap[(size_t)b * 8 + z] = m;
        unsigned fl = 0;
        if (active)
            fl = (unsigned)((sv[0] < 0.f) != (sv[1] < 0.f)) | ((unsigned)((sv[0] < 0.f) != (sv[2] < 0.f)) << 1) |
                 ((unsigned)((sv[0] < 0.f) != (sv[4] < 0.f)) << 2) | ((unsigned)(sv[0] < 0.f) << 3);
        eflags[(size_t)b * BF_TSDF_VOX + t] = (uint8_t)fl;
        if (t == 0) {
            int tot = 0;
            for (int i = 0; i < 8; ++i) tot += wave_n[i];
            vcount[b] = tot;
            rank_of_slot[sslot[b]] = b;
        }
        return;
    }
    if (!active) return;
    int rank = vcount[b] + bf_lanes_below(m);
    for (int i = 0; i < z; ++i) rank += wave_n[i];
    // the mean of the crossings of the sign-changing edges: four x-edges, four y-edges, four z-edges
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int ne = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int ax = e >> 2, i = e & 3;
        const int ca = ax == 0 ? 2 * i : (ax == 1 ? (i & 1) + 4 * (i >> 1) : i);
        const int cb = ca + (1 << ax);
        const float a = sv[ca], bb = sv[cb];
        if ((a < 0.f) != (bb < 0.f)) {
            const float tt = a / (a - bb);
            sx += ax == 0 ? tt : (float)(ca & 1);
            sy += ax == 1 ? tt : (float)((ca >> 1) & 1);
            sz += ax == 2 ? tt : (float)(ca >> 2);
            ++ne;
        }
    }
    const float cnt = (float)ne;
    const int ix = key_axis(key, 0) * 8 + x;
    const int iy = key_axis(key, 1) * 8 + y;
    const int iz = key_axis(key, 2) * 8 + z;
    float* o = verts + (size_t)rank * 3;
    o[0] = (((float)ix + 0.5f) + sx / cnt) * voxel;
    o[1] = (((float)iy + 0.5f) + sy / cnt) * voxel;
    o[2] = (((float)iz + 0.5f) + sz / cnt) * voxel;
    unsigned r = 0, g = 0, bl = 0, nc = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if ((tg[c] >> 24) & 1u) {
            r += tg[c] & 255u;
            g += (tg[c] >> 8) & 255u;
            bl += (tg[c] >> 16) & 255u;
            ++nc;
        }
    uint8_t* oc = vrgb + (size_t)rank * 3;
    oc[0] = (uint8_t)(nc ? (r + nc / 2) / nc : 128u);
    oc[1] = (uint8_t)(nc ? (g + nc / 2) / nc : 128u);
    oc[2] = (uint8_t)(nc ? (bl + nc / 2) / nc : 128u);
}

// the vertex of cell (x, y, z) of the block at sorted position r (coordinates in 0..7), or -1 if it has none
__device__ __forceinline__ int tsdf_cell_vertex(const u64* __restrict__ bitmap, const int* __restrict__ vprefix, int r, int x,
                                                int y, int z) {
    const u64* bm = bitmap + (size_t)r * 8;
    const int c = x + 8 * y;
    const u64 word = bm[z];
    if (!((word >> c) & 1ull)) return -1;
    int v = vprefix[r] + __popcll(c ? word & ((1ull << c) - 1ull) : 0ull);
    for (int i = 0; i < z; ++i) v += __popcll(bm[i]);
    return v;
}

// a quad per sign-changing edge (from the cell's minimum corner along axis a) whose four cells have a vertex: the
// cells at 0, -e_b, -e_b-e_c, -e_c with (a, b, c) cyclic run counter-clockwise seen from +a
template <bool WRITE>
__global__ void __launch_bounds__(BF_TSDF_VOX) k_tsdf_faces(const u64* __restrict__ keys, u64 mask,
                                                         const long long* __restrict__ skey,
                                                         const int* __restrict__ rank_of_slot, const u64* __restrict__ bitmap,
                                                         const uint8_t* __restrict__ eflags, const int* __restrict__ vprefix,
                                                         int* __restrict__ fcount, int* __restrict__ faces) {
    __shared__ int nrank[8];
    __shared__ int wave_n[8];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 8) {
        int r = b;
        if (t) {
            const u64 nk = key_neighbour((u64)skey[b], -(t & 1), -((t >> 1) & 1), -(t >> 2));
            const int s = nk == BF_KEY_EMPTY ? -1 : map_lookup(keys, mask, nk);
            r = s < 0 ? -1 : rank_of_slot[s];
        }
        nrank[t] = r;
    }
    __syncthreads();
    const unsigned fl = eflags[(size_t)b * BF_TSDF_VOX + t];
    const int xyz[3] = {t & 7, (t >> 3) & 7, t >> 6};
    int quad[3][4];
    int nq = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        quad[a][0] = -1;
        if (!((fl >> a) & 1u)) continue;
        const int bx = (a + 1) % 3, cx = (a + 2) % 3;
        bool all = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int c[3] = {xyz[0], xyz[1], xyz[2]};
            c[bx] -= (k == 1 || k == 2);
            c[cx] -= (k == 2 || k == 3);
            const int r = nrank[(c[0] < 0) | ((c[1] < 0) << 1) | ((c[2] < 0) << 2)];
            const int v = r < 0 ? -1 : tsdf_cell_vertex(bitmap, vprefix, r, c[0] & 7, c[1] & 7, c[2] & 7);
            quad[a][k] = v;
            all = all && v >= 0;
        }
        if (!all) quad[a][0] = -1;
        nq += all;
    }
    // exclusive prefix of nq over the workgroup, in cell order
    int inc = nq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (bf_lane() >= o) inc += v;
    }
    if (bf_lane() == 63) wave_n[t >> 6] = inc;
    __syncthreads();
    int at = inc - nq, tot = 0;
    for (int i = 0; i < 8; ++i) {
        at += i < (t >> 6) ? wave_n[i] : 0;
        tot += wave_n[i];
    }
    if (!WRITE) {
        if (t == 0) fcount[b] = tot;
        return;
    }
    int* o = faces + ((size_t)fcount[b] + at) * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (quad[a][0] < 0) continue;
        const bool fwd = (fl >> 3) & 1u;                         // inside at the minimum corner: the normal is +a
        const int v0 = quad[a][0], v1 = fwd ? quad[a][1] : quad[a][3], v2 = quad[a][2], v3 = fwd ? quad[a][3] : quad[a][1];
        o[0] = v0;
        o[1] = v1;
        o[2] = v2;
        o[3] = v0;
        o[4] = v2;
        o[5] = v3;
        o += 6;
    }
}

static bool tsdf_surface_args(const void* keys, long long capacity, const void* skey, const void* sslot, int n,
                              const void* rank_of_slot, const void* bitmap, const void* eflags, const void* vprefix,
                              const void* fprefix) {
    return keys && skey && sslot && rank_of_slot && bitmap && eflags && vprefix && fprefix && n > 0 && capacity > 0 &&
           !(capacity & (capacity - 1)) && capacity < (1ll << 31) && n <= capacity;
}

BF_API int bf_tsdf_surface_count(const void* keys, long long capacity, const int32_t* vox, const int64_t* skey,
                                 const int* sslot, int n, int* rank_of_slot, void* bitmap, uint8_t* eflags, int* vprefix,
                                 int* fprefix, int* totals, void* stream) {
    if (!tsdf_surface_args(keys, capacity, skey, sslot, n, rank_of_slot, bitmap, eflags, vprefix, fprefix) || !vox || !totals)
        return BF_ERR_ARG;
    if ((long long)n * BF_TSDF_VOX * 3 >= (1ll << 31)) return BF_ERR_CAPACITY;      // vertex and quad indices are int32
    hipStream_t st = bf_stream(stream);
    const u64 mask = (u64)(capacity - 1);
    // -1 everywhere: an occupied block that the caller did not list has no vertices for its neighbours
    if (hipMemsetAsync(rank_of_slot, 0xFF, (size_t)capacity * sizeof(int), st) != hipSuccess) return BF_ERR_LAUNCH;
    hipLaunchKernelGGL(k_tsdf_cells<false>, dim3(n), dim3(BF_TSDF_VOX), 0, st, (const u64*)keys, mask, (const int*)vox,
                       (const long long*)skey, sslot, rank_of_slot, (u64*)bitmap, eflags, vprefix, 0.f, nullptr, nullptr);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, st, vprefix, n, 0, totals, 0);
    hipLaunchKernelGGL(k_tsdf_faces<false>, dim3(n), dim3(BF_TSDF_VOX), 0, st, (const u64*)keys, mask, (const long long*)skey,
                       (const int*)rank_of_slot, (const u64*)bitmap, (const uint8_t*)eflags, (const int*)vprefix, fprefix,
                       nullptr);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, st, fprefix, n, 0, totals + 1, 0);
    return bf_check_launch();
}

BF_API int bf_tsdf_surface_write(const void* keys, long long capacity, const int32_t* vox, const int64_t* skey,
                                 const int* sslot, int n, const int* rank_of_slot, const void* bitmap, const uint8_t* eflags,
                                 const int* vprefix, const int* fprefix, float voxel, float* verts, uint8_t* vrgb, int* faces,
                                 void* stream) {
    if (!tsdf_surface_args(keys, capacity, skey, sslot, n, rank_of_slot, bitmap, eflags, vprefix, fprefix) || !vox || !verts ||
        !vrgb || !faces || !(voxel > 0.f))
        return BF_ERR_ARG;
    hipStream_t st = bf_stream(stream);
    const u64 mask = (u64)(capacity - 1);
    hipLaunchKernelGGL(k_tsdf_cells<true>, dim3(n), dim3(BF_TSDF_VOX), 0, st, (const u64*)keys, mask, (const int*)vox,
                       (const long long*)skey, sslot, (int*)rank_of_slot, (u64*)bitmap, (uint8_t*)eflags, (int*)vprefix, voxel,
                       verts, vrgb);
    hipLaunchKernelGGL(k_tsdf_faces<true>, dim3(n), dim3(BF_TSDF_VOX), 0, st, (const u64*)keys, mask, (const long long*)skey,
                       rank_of_slot, (const u64*)bitmap, eflags, vprefix, (int*)fprefix, faces);
    return bf_check_launch();
}

// ---- raycast: the volume read back as a predicted depth / vertex / normal map ---------------------------------------------
// One thread per pixel, one wave per 8 x 8 pixel tile (lane = x + 8 y), so that the rays of a wave stay in the same
// blocks.  The ray of pixel (u, v) is o + d t with o the pose's translation, d = R (a, b, 1), a = (u - cx) / fx,
// b = (v - cy) / fy, and t the depth in the camera; len = sqrt(a a + b b + 1) metres per unit of t.  All f32, left
// to right, no contraction.
//   field   s(p): g = p / voxel - 0.5, i = floor(g), f = g - i; the eight voxels i + (c & 1, (c >> 1) & 1, c >> 2) must
//           all exist with w >= min_weight; their values (float)q / (float)w / 1024 are interpolated along x, then y,
//           then z, each as lo + f * (hi - lo).
//   step    t starts at near.  While t < far and fewer than max_steps steps were made:
//           the block floor(p / (8 voxel)) is absent (or past the index range): t += max(min over the axes with
//           d_i != 0 of (bound_i - p_i) / d_i, 0) + 0.25 voxel / len, bound_i the block's face the ray leaves through;
//           the sample is forgotten.
//           the block is present and s(p) invalid: t += voxel / len; the sample is forgotten.
//           s(p) valid: t += max(0.5 |s| trunc, 0.25 voxel) / len -- at most half the truncation distance, at least a
//           quarter voxel, so a surface as thin as the band cannot be stepped over.
//   hit     s < 0 is inside and s >= 0 outside (zero is outside, as in the surface extractor).  The first step from a
//           valid outside sample to the next sample, valid and inside, is the hit: t_hit = t0 + (t1 - t0) * s0 / (s0 - s1).
//           A step from a valid inside sample to a valid outside one ends the ray: the camera is behind that surface.
//   normal  the central differences of s at p_hit +- voxel / 2 along x, y, z, normalised; a pixel with an invalid tap or
//           a zero gradient is no hit.
// counters (u64 [BF_STATS_WORDS], BF_TSDF_RAY_*): hits, rays ended behind a surface, rays that left the range (or ran
// out of steps), views skipped for a non-finite pose, rays whose hit had no normal.

// the slot of block (bx, by, bz) as floats (whole numbers), through the lane's one-entry cache; -1: absent or out of range
__device__ __forceinline__ int rc_block(const u64* __restrict__ keys, u64 mask, float bx, float by, float bz, u64& ckey,
                                        int& cslot) {
    if (!key_in_range(bx, by, bz)) return -1;
    const u64 key = key_pack((int)bx, (int)by, (int)bz);
    if (key != ckey) {
        ckey = key;
        cslot = map_lookup(keys, mask, key);
    }
    return cslot;
}

// the word index of voxel (ix, iy, iz)'s w, or -1
__device__ __forceinline__ long long rc_voxel(const u64* __restrict__ keys, u64 mask, int ix, int iy, int iz, u64& ckey,
                                              int& cslot) {
    const u64 key = key_pack(ix >> 3, iy >> 3, iz >> 3);
    if (key != ckey) {
        ckey = key;
        cslot = map_lookup(keys, mask, key);
    }
    if (cslot < 0) return -1;
    return (long long)cslot * TSDF_BLOCK_WORDS + ((ix & 7) | ((iy & 7) << 3) | ((iz & 7) << 6));
}

__device__ __forceinline__ bool rc_sample(const u64* __restrict__ keys, u64 mask, const int* __restrict__ vox, float voxel,
                                          int min_weight, float px, float py, float pz, u64& ckey, int& cslot, float* s) {
    const float gx = px / voxel - 0.5f, gy = py / voxel - 0.5f, gz = pz / voxel - 0.5f;
    const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
    const float lim = 8388600.0f;                                // below 2^23: every corner's block index is within 2^20
    if (!(x0 >= -lim && x0 < lim && y0 >= -lim && y0 < lim && z0 >= -lim && z0 < lim)) return false;
    const float tx = gx - x0, ty = gy - y0, tz = gz - z0;
    const int ix = (int)x0, iy = (int)y0, iz = (int)z0;
    float v[8];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = 0.f;
        if (!ok) continue;
        const long long at = rc_voxel(keys, mask, ix + (c & 1), iy + ((c >> 1) & 1), iz + (c >> 2), ckey, cslot);
        if (at < 0) {
            ok = false;
            continue;
        }
        const int w = vox[at];
        if (w < min_weight) {
            ok = false;
            continue;
        }
        v[c] = (float)vox[at + BF_TSDF_VOX] / (float)w / 1024.0f;
    }
    if (!ok) return false;
    const float c00 = v[0] + tx * (v[1] - v[0]), c10 = v[2] + tx * (v[3] - v[2]);
    const float c01 = v[4] + tx * (v[5] - v[4]), c11 = v[6] + tx * (v[7] - v[6]);
    const float c0 = c00 + ty * (c10 - c00), c1 = c01 + ty * (c11 - c01);
    *s = c0 + tz * (c1 - c0);
    return true;
}

__device__ __forceinline__ void rc_count(u64* counters, int which, bool flag) {
    const u64 m = __ballot(flag);
    if (m && bf_lane() == (int)(__ffsll((long long)m) - 1)) atomicAdd(counters + which, (u64)__popcll(m));
}

__global__ void __launch_bounds__(CLOUD_BLOCK) k_tsdf_raycast(const u64* __restrict__ keys, u64 mask, const int* __restrict__ vox,
                                                              const float* __restrict__ poses, int H, int W, int tiles_x,
                                                              int tiles, int bpv, float fx, float fy, float cx, float cy,
                                                              float voxel, int T, float near_z, float far_z, int min_weight,
                                                              int max_steps, float* __restrict__ depth,
                                                              float* __restrict__ vertex, float* __restrict__ normal,
                                                              uint8_t* __restrict__ rgb, u64* __restrict__ counters) {
    const int view = blockIdx.x / bpv;
    const int tile = (blockIdx.x - view * bpv) * CLOUD_WAVES + (threadIdx.x >> 6);
    if (tile >= tiles) return;                                   // the whole wave
    const int lane = bf_lane();
    const int u = (tile % tiles_x) * 8 + (lane & 7), v = (tile / tiles_x) * 8 + (lane >> 3);
    const bool in_image = u < W && v < H;
    const float* P = poses + 16 * view;
    const bool finite = bf_pose_finite(P);
    const size_t pix = ((size_t)view * H + (in_image ? v : 0)) * W + (in_image ? u : 0);
    float out_d = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    unsigned cr = 0, cg = 0, cb = 0;
    bool hit = false, behind = false, left = false, no_normal = false;
    if (!finite) {
        if (tile == 0 && lane == 0) atomicAdd(counters + BF_TSDF_RAY_SKIPPED_POSE, 1ull);
    } else if (in_image) {
        const float a = ((float)u - cx) / fx, b = ((float)v - cy) / fy;
        const float dx = P[0] * a + P[1] * b + P[2], dy = P[4] * a + P[5] * b + P[6], dz = P[8] * a + P[9] * b + P[10];
        const float ox = P[3], oy = P[7], oz = P[11];
        const float len = sqrtf(a * a + b * b + 1.0f);
        const float trunc = (float)T * voxel, bs = 8.0f * voxel;
        const float min_m = 0.25f * voxel;
        u64 ckey = BF_KEY_EMPTY;
        int cslot = -1;
        float t = near_z, t0 = 0.f, s0 = 0.f;
        bool have = false;                                       // (t0, s0) is a valid sample, the one before this
        bool done = false;
        for (int n = 0; n < max_steps && !done; ++n) {
            if (!(t < far_z)) break;
            const float px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;
            const float bx = floorf(px / bs), by = floorf(py / bs), bz = floorf(pz / bs);
            if (rc_block(keys, mask, bx, by, bz, ckey, cslot) < 0) {
                float e = INFINITY;
                if (dx != 0.f) e = fminf(e, ((dx > 0.f ? (bx + 1.0f) * bs : bx * bs) - px) / dx);
                if (dy != 0.f) e = fminf(e, ((dy > 0.f ? (by + 1.0f) * bs : by * bs) - py) / dy);
                if (dz != 0.f) e = fminf(e, ((dz > 0.f ? (bz + 1.0f) * bs : bz * bs) - pz) / dz);
                t = t + (fmaxf(e, 0.f) + min_m / len);
                have = false;
                continue;
            }
            float s;
            if (!rc_sample(keys, mask, vox, voxel, min_weight, px, py, pz, ckey, cslot, &s)) {
                t = t + voxel / len;
                have = false;
                continue;
            }
            if (have && s0 >= 0.f && s < 0.f) {
                const float th = t0 + (t - t0) * (s0 / (s0 - s));
                out_d = th;
                hit = done = true;
                continue;
            }
            if (have && s0 < 0.f && s >= 0.f) {
                behind = done = true;
                continue;
            }
            t0 = t;
            s0 = s;
            have = true;
            t = t + fmaxf(0.5f * fabsf(s) * trunc, min_m) / len;
        }
        left = !hit && !behind;
        if (hit) {
            vx = ox + dx * out_d;
            vy = oy + dy * out_d;
            vz = oz + dz * out_d;
            const float h = 0.5f * voxel;
            float xp, xm, yp, ym, zp, zm;
            bool ok = rc_sample(keys, mask, vox, voxel, min_weight, vx + h, vy, vz, ckey, cslot, &xp);
            ok = ok && rc_sample(keys, mask, vox, voxel, min_weight, vx - h, vy, vz, ckey, cslot, &xm);
            ok = ok && rc_sample(keys, mask, vox, voxel, min_weight, vx, vy + h, vz, ckey, cslot, &yp);
            ok = ok && rc_sample(keys, mask, vox, voxel, min_weight, vx, vy - h, vz, ckey, cslot, &ym);
            ok = ok && rc_sample(keys, mask, vox, voxel, min_weight, vx, vy, vz + h, ckey, cslot, &zp);
            ok = ok && rc_sample(keys, mask, vox, voxel, min_weight, vx, vy, vz - h, ckey, cslot, &zm);
            float norm = 0.f;
            if (ok) {
                nx = xp - xm;
                ny = yp - ym;
                nz = zp - zm;
                norm = sqrtf(nx * nx + ny * ny + nz * nz);
            }
            if (ok && norm > 0.f) {
                nx = nx / norm;
                ny = ny / norm;
                nz = nz / norm;
                if (rgb) {
                    cr = cg = cb = 128u;
                    const float qx = floorf(vx / voxel), qy = floorf(vy / voxel), qz = floorf(vz / voxel);
                    const float lim = 8388600.0f;
                    if (qx >= -lim && qx < lim && qy >= -lim && qy < lim && qz >= -lim && qz < lim) {
                        const long long at = rc_voxel(keys, mask, (int)qx, (int)qy, (int)qz, ckey, cslot);
                        if (at >= 0) {
                            const int cw = vox[at + 2 * BF_TSDF_VOX];
                            if (cw > 0) {
                                const unsigned hw = (unsigned)cw >> 1, c = (unsigned)cw;
                                cr = ((unsigned)vox[at + 3 * BF_TSDF_VOX] + hw) / c;
                                cg = ((unsigned)vox[at + 4 * BF_TSDF_VOX] + hw) / c;
                                cb = ((unsigned)vox[at + 5 * BF_TSDF_VOX] + hw) / c;
                            }
                        }
                    }
                }
            } else {
                hit = false;
                no_normal = true;
                out_d = vx = vy = vz = nx = ny = nz = 0.f;
            }
        }
    }
    rc_count(counters, BF_TSDF_RAY_HITS, hit);
    rc_count(counters, BF_TSDF_RAY_BEHIND, behind);
    rc_count(counters, BF_TSDF_RAY_LEFT_RANGE, left);
    rc_count(counters, BF_TSDF_RAY_NO_NORMAL, no_normal);
    if (!in_image) return;
    depth[pix] = out_d;
    vertex[pix * 3] = vx;
    vertex[pix * 3 + 1] = vy;
    vertex[pix * 3 + 2] = vz;
    normal[pix * 3] = nx;
    normal[pix * 3 + 1] = ny;
    normal[pix * 3 + 2] = nz;
    if (rgb) {
        rgb[pix * 3] = (uint8_t)cr;
        rgb[pix * 3 + 1] = (uint8_t)cg;
        rgb[pix * 3 + 2] = (uint8_t)cb;
    }
}

BF_API int bf_tsdf_raycast(const void* keys, const int32_t* vox, long long capacity, const float* poses, int V, int H, int W,
                           float fx, float fy, float cx, float cy, float voxel, int trunc_voxels, float near_z, float far_z,
                           int min_weight, int max_steps, float* depth, float* vertex, float* normal, uint8_t* rgb,
                           void* counters, void* stream) {
    if (!keys || !vox || !poses || !depth || !vertex || !normal || !counters || V <= 0 || H <= 0 || W <= 0 || capacity <= 0 ||
        (capacity & (capacity - 1)) || !(voxel > 0.f) || trunc_voxels < 1 || trunc_voxels > BF_TSDF_MAX_TRUNC ||
        !(near_z >= 0.f) || !(far_z > near_z) || !(far_z < INFINITY) || min_weight < 1 || max_steps < 1 || !(fx > 0.f) ||
        !(fy > 0.f))
        return BF_ERR_ARG;
    const long long tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
    const long long bpv = (tiles + CLOUD_WAVES - 1) / CLOUD_WAVES;
    if (capacity >= (1ll << 31) || (long long)H * W * V >= (1ll << 31) / 3 || bpv * V >= (1ll << 31)) return BF_ERR_CAPACITY;
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)(bpv * V)), dim3(CLOUD_BLOCK), 0, bf_stream(stream), (const u64*)keys,
                       (u64)(capacity - 1), (const int*)vox, poses, H, W, (int)tiles_x, (int)tiles, (int)bpv, fx, fy, cx, cy,
                       voxel, trunc_voxels, near_z, far_z, min_weight, max_steps, depth, vertex, normal, rgb, (u64*)counters);
    return bf_check_launch();
}
