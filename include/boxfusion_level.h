/*
 * boxfusion_level.h — the levelling entry points of libboxfusion_hip.so: which way is up in a scene that
 * was tracked from scratch, where its floor lies and how its walls run.  An extension of boxfusion_hip.h
 * with the same conventions (caller-owned device pointers, `stream` a hipStream_t as void*, a bf_status
 * returned, no process-wide state); the status codes are the core header's and are not restated here.
 *
 * No counterpart in the reference: its sequences come with a gravity-aligned world.  The fused surface of
 * an indoor scene is mostly a floor and walls (a Manhattan world): floor normals are parallel to up, wall
 * normals are perpendicular to it and cluster four-fold about it.  Four kernels reduce oriented samples
 * (point, unit normal, integer weight) to integer sums; the host solves a 3 x 3 problem from them
 * (boxfusion_amd/scene_level.py).  Every sum is an integer atomic: the outputs are the same bits whatever
 * the launch geometry or the order of the samples.  All f32 arithmetic below is written with every
 * operation rounded on its own (the file is compiled with contraction off and IEEE division and sqrt).
 */
#ifndef BOXFUSION_LEVEL_H
#define BOXFUSION_LEVEL_H

#include "boxfusion_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BF_LEVEL_WEIGHT_CAP 65535       /* the largest weight bf_level_face_samples gives a face */
#define BF_LEVEL_MAX_G 32               /* cube-map cells per face edge, at most */
#define BF_LEVEL_MAX_CANDIDATES 6144    /* 6 G G at the largest G: candidates of one bf_level_score call */
#define BF_LEVEL_MAX_HEIGHT_BINS 1024   /* bins of bf_level_refine's height histogram, at most */
#define BF_LEVEL_HEIGHT_WORDS 4         /* int64 words of a height bin: w, w q(h - h0), w q(p.e1), w q(p.e2) */
#define BF_LEVEL_SUM_WORDS 14           /* int64 words of bf_level_refine's sums */
#define BF_LEVEL_NORMAL_SHIFT 20        /* products of normal components are held in units of 2^-20 */
#define BF_LEVEL_METRE_SHIFT 16         /* heights and horizontal coordinates in units of 2^-16 m */
#define BF_LEVEL_COORD_LIMIT (1 << 20)  /* metres: |p.e1|, |p.e2| and the height range stay below it */
#define BF_LEVEL_STATS_WORDS 24         /* uint64 words of the stats tensor all four kernels add to */

/* Overflow.  With W the sum of the weights given to one call (at most BF_LEVEL_WEIGHT_CAP per face from
 * bf_level_face_samples, so W < 2^16 n):
 *   a histogram bin of bf_level_vote holds at most W;
 *   a word of bf_level_refine's sums is at most 2^20 W in magnitude (|n_i n_j| <= 1, |1 - 8 a^2 b^2| <= 1,
 *   |4 a b (a^2 - b^2)| <= 1), so the int64 sums are exact for W < 2^43: 2^27 saturated faces;
 *   a word of a height bin is at most 2^16 L W with L the larger of the height range and the horizontal
 *   reach in metres, L < BF_LEVEL_COORD_LIMIT = 2^20, so exact for W < 2^27 at that limit and for
 *   W < 2^41 (2^25 saturated faces) in a scene that spans 64 m. */

typedef enum {
    BF_LEVEL_STAT_FACES = 0,            /* bf_level_face_samples: faces given */
    BF_LEVEL_STAT_FACE_BAD_INDEX,       /* of them with a vertex index outside 0 .. n_vertices - 1 */
    BF_LEVEL_STAT_FACE_NONFINITE,       /* else with a coordinate, or a cross product's length, that is not finite */
    BF_LEVEL_STAT_FACE_ZERO_AREA,       /* else with a cross product of length 0 */
    BF_LEVEL_STAT_FACE_SATURATED,       /* else with rint(area / area_unit) above BF_LEVEL_WEIGHT_CAP */
    BF_LEVEL_STAT_VOTE_SAMPLES,         /* bf_level_vote: samples given */
    BF_LEVEL_STAT_VOTE_SKIPPED,         /* of them skipped: weight 0, a component not finite, or all three 0 */
    BF_LEVEL_STAT_VOTE_WEIGHT,          /* the weight of the others: the histogram's total */
    BF_LEVEL_STAT_REFINE_SAMPLES,       /* bf_level_refine: samples given */
    BF_LEVEL_STAT_REFINE_SKIPPED,       /* of them skipped: weight 0 or a word of the point or normal not finite */
    BF_LEVEL_STAT_REFINE_PAR,           /* samples of the parallel set */
    BF_LEVEL_STAT_REFINE_PERP,          /* samples of the perpendicular set */
    BF_LEVEL_STAT_REFINE_UP,            /* samples of the upward set */
    BF_LEVEL_STAT_REFINE_OUTSIDE,       /* of the upward set, outside the height range or the coordinate limit */
    BF_LEVEL_STAT_REFINE_WEIGHT,        /* the weight of the samples not skipped */
    BF_LEVEL_STAT_REFINE_WEIGHT_PAR,    /* of the parallel set */
    BF_LEVEL_STAT_REFINE_WEIGHT_PERP,   /* of the perpendicular set */
    BF_LEVEL_STAT_REFINE_WEIGHT_UP      /* of the upward set, the samples outside included */
} bf_level_stat;

/* Oriented samples of a triangle mesh, one per face.
 *   vertices f32 [n_vertices,3], faces i32 [m,3]
 * With a, b, c the face's vertices in its index order, in f32:
 *   e = b - a, f = c - a,  x = (e.y f.z - e.z f.y,  e.z f.x - e.x f.z,  e.x f.y - e.y f.x),
 *   len = sqrtf((x.x x.x + x.y x.y) + x.z x.z),  normal = x / len (three divisions),
 *   centroid = ((a + b) + c) / 3.0f per component,  area = 0.5f len,
 *   weight = min(rintf(area / area_unit), BF_LEVEL_WEIGHT_CAP)  (ties to even).
 * For the surface of bf_tsdf_surface_write the normal points to free space.  A face with an index out of
 * range, else with a vertex coordinate or len that is not finite, else with len == 0 gets weight 0 and a
 * centroid and normal of NaN, and is counted; so is a face whose weight was capped.  A small face may
 * round to weight 0: it is not counted here, bf_level_vote and bf_level_refine skip it.
 *   centroids f32 [m,3], normals f32 [m,3], weights u32 [m]: written
 *   stats uint64 [BF_LEVEL_STATS_WORDS], added to (BF_LEVEL_STAT_FACE*)
 * m < 0, n_vertices < 0, area_unit not finite or not > 0, or a null pointer where m > 0: BF_ERR_ARG.
 * m == 0 launches nothing. */
int bf_level_face_samples(const float* vertices, long long n_vertices, const int32_t* faces, long long m,
                          float area_unit, float* centroids, float* normals, uint32_t* weights,
                          void* stats, void* stream);

/* Vote the normals into a cube map of G x G cells per face.
 *   normals f32 [n,3], weights u32 [n]
 * For a normal (x, y, z): the axis k is 0 when |x| >= |y| and |x| >= |z|, else 1 when |y| >= |z|, else 2
 * (ties go to the lowest axis); the cube face is 2 k + (the component k is negative); with p < q the other
 * two axes, u = n_p / n_k and v = n_q / n_k (f32 divisions by the signed major component),
 *   iu = min((int)floorf((u + 1.0f) * (0.5f G)), G - 1), iv the same from v,
 *   bin = (face G + iv) G + iu.
 * A sample with weight 0, a component that is not finite or all components 0 is skipped and counted.
 *   hist uint64 [6 G G], added to: the weight per bin
 *   stats uint64 [BF_LEVEL_STATS_WORDS], added to (BF_LEVEL_STAT_VOTE_*)
 * The samples need not come from faces: a raycast's or a depth frame's normal map votes the same way.
 * G outside 1 .. BF_LEVEL_MAX_G, n < 0 or a null pointer where n > 0: BF_ERR_ARG.  n == 0 launches nothing. */
int bf_level_vote(const float* normals, const uint32_t* weights, long long n, int G, void* hist, void* stats,
                  void* stream);

/* The centre direction of a bin, the one rule bf_level_score and the host share: with face, iv, iu from
 * bin = (face G + iv) G + iu, k = face / 2, s = 1.0f for an even face and -1.0f for an odd one,
 *   u = (float)(2 iu + 1 - G) / (float)G,  v = (float)(2 iv + 1 - G) / (float)G,
 *   len = sqrtf((u u + v v) + 1.0f),
 *   d_k = s / len,  d_p = (u s) / len,  d_q = (v s) / len   (p < q the other two axes).
 *
 * Score candidate axes against the histogram.
 *   hist uint64 [6 G G], candidates i32 [n_candidates]: bin indices
 * For candidate j with centre direction c and every bin with centre direction d and weight h:
 *   dot = (c.x d.x + c.y d.y) + c.z d.z,
 *   par[j] = sum of h over fabsf(dot) >= cos_par,  perp[j] = sum of h over fabsf(dot) <= sin_perp.
 *   scores uint64 [n_candidates,2], written: par, perp.  A candidate outside 0 .. 6 G G - 1 scores 0, 0.
 * One workgroup per candidate.  G outside 1 .. BF_LEVEL_MAX_G, n_candidates outside
 * 0 .. BF_LEVEL_MAX_CANDIDATES or a null pointer where n_candidates > 0: BF_ERR_ARG.  n_candidates == 0
 * launches nothing. */
int bf_level_score(const void* hist, int G, const int32_t* candidates, int n_candidates, float cos_par,
                   float sin_perp, void* scores, void* stream);

/* One pass over the samples for an axis c and a horizontal basis e1, e2.
 *   points f32 [n,3], normals f32 [n,3], weights u32 [n]
 *   frame f32 [9] on the device: c, e1, e2
 * A sample with weight 0 or a non-finite word in its point or normal is skipped and counted.  For the
 * others, with dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z in f32 and w the weight:
 *   t = dot(n, c);  parallel set: fabsf(t) >= cos_par;  perpendicular set: fabsf(t) <= sin_perp;
 *   upward set: t >= cos_par (the floor, not the ceiling).
 *   sums int64 [BF_LEVEL_SUM_WORDS], added to:
 *     0..5   over the parallel set, w llrintf((n_i n_j) 1048576.0f) for ij = xx, xy, xz, yy, yz, zz
 *     6..11  the same over the perpendicular set
 *     12,13  over the perpendicular set, with pa = dot(n, e1), pb = dot(n, e2), r = sqrtf(pa pa + pb pb)
 *            and, where r > 0, a = pa / r, b = pb / r, a2 = a a, b2 = b b:
 *            w llrintf((1.0f - (8.0f a2) b2) 1048576.0f)  and  w llrintf((((4.0f a) b) (a2 - b2)) 1048576.0f);
 *            a sample with r == 0 adds nothing to these two
 *   heights int64 [n_bins,BF_LEVEL_HEIGHT_WORDS], added to, over the upward set: with h = dot(p, c),
 *     d = h - h0, fb = floorf(d / height_bin), x1 = dot(p, e1), x2 = dot(p, e2), a sample is inside when
 *     d >= 0, fb < n_bins, fabsf(x1) < BF_LEVEL_COORD_LIMIT and fabsf(x2) < BF_LEVEL_COORD_LIMIT, and then adds
 *     to bin (int)fb:  w,  w llrintf(d 65536.0f),  w llrintf(x1 65536.0f),  w llrintf(x2 65536.0f);
 *     the others of the upward set are counted (BF_LEVEL_STAT_REFINE_OUTSIDE).  n_bins == 0: no height
 *     histogram, heights may be null and every sample of the upward set counts as outside.
 *   stats uint64 [BF_LEVEL_STATS_WORDS], added to (BF_LEVEL_STAT_REFINE_*)
 * n < 0, n_bins outside 0 .. BF_LEVEL_MAX_HEIGHT_BINS, with n_bins > 0 a height_bin that is not finite or
 * not > 0 or n_bins height_bin > BF_LEVEL_COORD_LIMIT or an h0 that is not finite, or a null pointer where
 * n > 0: BF_ERR_ARG.  n == 0 launches nothing. */
int bf_level_refine(const float* points, const float* normals, const uint32_t* weights, long long n,
                    const float* frame, float cos_par, float sin_perp, float h0, float height_bin, int n_bins,
                    void* sums, void* heights, void* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BOXFUSION_LEVEL_H */
