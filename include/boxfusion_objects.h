/*
 * boxfusion_objects.h — the object-level entry points of libboxfusion_hip.so: which points of a scene
 * lie in which fused box.  An extension of boxfusion_hip.h with the same conventions (caller-owned
 * device pointers, `stream` a hipStream_t as void*, a bf_status returned, no process-wide state); the
 * status codes, BF_STATS_WORDS and BF_MAX_BOXES are the core header's and are not restated here.
 *
 * No counterpart in the reference: it ends at the fused boxes.  The idea is the one its ground-truth
 * filter applies (data_process/filter_gt_boxes.py:75-93: a box is real when scene points are near it),
 * turned towards the predictions.
 */
#ifndef BOXFUSION_OBJECTS_H
#define BOXFUSION_OBJECTS_H

#include "boxfusion_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BF_OBJ_BOX_WORDS 16             /* f32 words of a box row */
#define BF_OBJ_COUNT_WORDS 2            /* uint64 words of a counts row: support, owned */
#define BF_OBJ_EXTENT_WORDS 6           /* uint32 words of an extents row: min, max of t_0, t_1, t_2 */
#define BF_OBJ_CHUNK 128                /* box rows staged in LDS per pass */

typedef enum {
    BF_OBJ_STAT_POINTS = 0,             /* points given */
    BF_OBJ_STAT_NONFINITE,              /* of them with a coordinate that is not finite (label -1, never tested) */
    BF_OBJ_STAT_LABELLED,               /* points with a label >= 0 */
    BF_OBJ_STAT_SHARED,                 /* points inside two or more boxes */
    BF_OBJ_STAT_PAIR_TESTS              /* point-box containment tests evaluated */
} bf_obj_stat;

/* Label every point with the box that owns it.
 *   xyz    f32 [n,3]
 *   boxes  f32 [B,BF_OBJ_BOX_WORDS]: centre c (words 0..2), three unit axes a_0 a_1 a_2 (3..11),
 *          half-lengths h_0 h_1 h_2 (12..14), volume (15).  A row of NaN contains nothing.
 * Point p is inside box b when, for k = 0, 1, 2, in f32 and with every operation rounded on its own,
 *   d = p - c,  t_k = (d.x a_k.x + d.y a_k.y) + d.z a_k.z,  fabsf(t_k) <= h_k + margin
 * (a point on a face is inside).  labels[i] is the containing box with the smallest word 15, the lowest
 * index among equals (a box takes a point from the owner so far only with a strictly smaller word 15),
 * and -1 when no box contains the point or a coordinate is not finite.
 *   labels   i32 [n], written
 *   counts   uint64 [B,BF_OBJ_COUNT_WORDS], added to: points inside b whoever owns them; points labelled b
 *   extents  uint32 [B,BF_OBJ_EXTENT_WORDS]: min t_0, max t_0, min t_1, max t_1, min t_2, max t_2 over
 *            the points labelled b, as order-preserving keys of the f32 bits (sign bit flipped for a clear
 *            sign bit, every bit flipped for a set one).  The caller sets the min words to 0xFFFFFFFF and
 *            the max words to 0; they are lowered and raised with integer atomicMin / atomicMax.
 *   stats    uint64 [BF_STATS_WORDS], added to in the order of BF_OBJ_STAT_*
 * Integer atomics only: every output is the same bits whatever the launch geometry or the order of
 * arrival.  B > BF_MAX_BOXES, n < 0 or a null pointer where n > 0: BF_ERR_ARG.  n == 0 launches
 * nothing; B == 0 labels every point -1. */
int bf_label_points(const float* xyz, long long n, const float* boxes, int B, float margin,
                    int32_t* labels, void* counts, void* extents, void* stats, void* stream);

/* The same with the per-wave cull switched by the caller (a test / benchmark hook; cull = 1 is what
 * bf_label_points runs).  With the cull a wave takes the bounding box of its points and, for every
 * box row, the interval each t_k can take over that bounding box, and skips the rows whose interval
 * misses [-(h_k + margin), h_k + margin]: rounding is monotonic, so the interval holds every t_k the
 * test itself would compute and no containing pair is ever skipped.  labels, counts and extents are
 * the same bits with and without it; BF_OBJ_STAT_PAIR_TESTS shows what it saves. */
int bf_label_points_ex(const float* xyz, long long n, const float* boxes, int B, float margin,
                       int32_t* labels, void* counts, void* extents, void* stats, int cull, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BOXFUSION_OBJECTS_H */
