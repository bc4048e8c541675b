/*
 * youth_loop.h — loop closing: keyframe signatures, verified loop edges and a
 * pose graph.
 *
 * Tracking composes frame-to-frame poses, so its error accumulates.  A
 * youth_loop keeps keyframes on the GPU, finds earlier keyframes that look
 * like a new one (a coarse integer signature, one kernel), verifies each
 * candidate with the RGB-D alignment of youth_rgbd.h run forward and backward,
 * and reports the pairs that pass as edges of a pose graph.
 * youth_posegraph_optimize (host, fp64) spreads the edges' corrections over
 * the keyframe poses.  Opt-in and beside what exists.  Numpy restatement:
 * tests/loop_truth.py.
 *
 * Signature.  A GX x GY = 20 x 15 grid; cell (i, j) covers columns
 * [i W / GX, (i+1) W / GX) and rows [j H / GY, (j+1) H / GY) (integer floor).
 * Per cell: n pixels, cnt pixels with d > 0, sumD over those, sumY over all
 * pixels of the uint8 intensity (youth_rgbd.h's Y).  The cell is valid iff
 * cnt > 0 and 4 cnt >= n; dm = (sumD + cnt / 2) / cnt if valid, else 0;
 * ym = (sumY + n / 2) / n.  All sums exact.  One uint32 per cell, cell index
 * j GX + i: bits 0..15 dm, 16..23 ym, bit 31 valid; YOUTH_LOOP_CELLS words
 * per frame.
 *
 * Distance.  Per cell c = min(|dm_q - dm_k|, cap) when both cells are valid,
 * cap when exactly one is, 0 when neither; plus ly |ym_q - ym_k| in all three
 * cases.  D(q, k) is the sum over the cells, uint32.
 *
 * Plain C99; streams travel as void*; return codes are youth_icp.h's YOUTH_OK /
 * YOUTH_E* (or a count >= 0).  Lives in libyouth_icp.so.  An object is used by
 * one thread at a time.
 */
#ifndef YOUTH_LOOP_H
#define YOUTH_LOOP_H

#include <stdint.h>

#include "youth_icp.h"
#include "youth_rgbd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOUTH_LOOP_GX 20
#define YOUTH_LOOP_GY 15
#define YOUTH_LOOP_CELLS 300
#define YOUTH_LOOP_MAX_KEYFRAMES 512   /* also the pose graph's node limit */
#define YOUTH_LOOP_MAX_CANDIDATES 16

typedef struct youth_loop_params {
    int      min_gap;         /* candidates k of keyframe q have q - k >= min_gap (>= 1) */
    int      max_candidates;  /* verified per close, 1 .. YOUTH_LOOP_MAX_CANDIDATES */
    uint32_t max_cell_dist;   /* prefilter: D <= max_cell_dist * YOUTH_LOOP_CELLS */
    uint32_t cap;             /* depth term's cap per cell, raw depth units (<= 65535) */
    uint32_t ly;              /* weight of the intensity term (<= 64) */
    float    min_overlap;     /* last-iteration geometric count >= min_overlap W H, both ways */
    float    max_gray_rms;    /* photometric RMS in grey levels, both ways */
    float    fb_rot_deg;      /* rotation angle of T_fwd T_bwd */
    float    fb_trans_m;      /* translation norm of T_fwd T_bwd */
} youth_loop_params;

/* min_gap 10, max_candidates 4, max_cell_dist 400, cap 1000, ly 4,
 * min_overlap 0.10, max_gray_rms 1.5, fb_rot_deg 0.5, fb_trans_m 0.010. */
youth_loop_params youth_loop_default_params(void);

/* A verified pair of keyframes i < j: Z ~ X_i^-1 X_j for camera -> world poses
 * X (P_i = Z P_j), fp64 row-major 4x4.  Also an edge of the pose graph, where
 * odometry edges carry the same fields with the measures zero. */
typedef struct youth_loop_edge {
    int32_t i, j;
    double  Z[16];
    double  w;            /* weight in the pose graph's cost; 1 for a verified pair */
    double  overlap;      /* the smaller geometric count of both ways / (W H) */
    double  gray_rms;     /* the larger photometric RMS of both ways, grey levels */
    double  fb_rot_deg;   /* forward x backward consistency */
    double  fb_trans_m;
} youth_loop_edge;

typedef struct youth_loop youth_loop;

/* A store for max_keyframes (2 .. YOUTH_LOOP_MAX_KEYFRAMES) keyframes of W x H
 * (W >= 20, H >= 15, the frame limits of youth_icp_create) on `device`, with
 * its own youth_rgbd context for the verification.  K NULL: the viewer's
 * intrinsics; params NULL: the defaults.  NULL on failure. */
youth_loop* youth_loop_create(int device, int W, int H, int max_keyframes,
                              const youth_intrinsics* K, const youth_loop_params* params);
void youth_loop_destroy(youth_loop* lp);
const char* youth_loop_last_error(void);

/* Stage entry: n frames (depth [n][H][W] int16, intensity [n][H][W] uint8, on
 * the device) -> d_sig [n][YOUTH_LOOP_CELLS]; asynchronous on `stream`.
 * 0 <= n <= 65535; W < 20 or H < 15 is YOUTH_EINVAL. */
int youth_loop_signature_device(int device, const int16_t* d_depth, const uint8_t* d_gray, int n,
                                int W, int H, uint32_t* d_sig, void* stream);

/* nq HOST signatures against the stored keyframes' -> HOST D [nq][n_kf] with
 * the object's cap and ly; returns n_kf.  Synchronous. */
int youth_loop_distances(youth_loop* lp, const uint32_t* sig_q, int nq, uint32_t* D);

/* Add a keyframe: its depth and intensity (device) or depth and RGB (host,
 * uint8 [H][W][3]), its camera -> world pose (fp64 4x4, finite) and a tag of
 * the caller's.  Returns its index; synchronous. */
int youth_loop_add_keyframe_device(youth_loop* lp, const int16_t* d_depth, const uint8_t* d_gray,
                                   const double T_wc[16], uint32_t tag);
int youth_loop_add_keyframe_host(youth_loop* lp, const int16_t* depth, const uint8_t* rgb,
                                 const double T_wc[16], uint32_t tag);

/* The candidates of keyframe kf: stored keyframes k with kf - k >= min_gap and
 * D <= max_cell_dist * YOUTH_LOOP_CELLS, lowest D first, ties by lower index,
 * at most min(k, max_candidates) into idx / dist (each nullable).  Returns
 * their number. */
int youth_loop_candidates(youth_loop* lp, int kf, int k, int* idx, uint32_t* dist);

/* Retrieve the candidates of keyframe kf and verify them: one RGB-D batch of
 * every candidate forward (source kf, target k) and backward, from the
 * identity, youth_rgbd_default_params() (or the schedule of
 * youth_loop_set_levels).  A candidate becomes the edge
 * (k, kf, Z = T_fwd) iff both statuses are 0 and the four gates of
 * youth_loop_params hold.  Returns the number of edges added. */
int youth_loop_close(youth_loop* lp, int kf);

/* Verify coarse to fine: the level schedule (youth_rgbd.h) of
 * the object's own RGB-D context; n = 0 (the default) switches it off.  The
 * last level must have stride 1 and at least one iteration: the four gates
 * read the last level's statistics, the overlap against W H, and the status
 * gate the OR of all levels' status words.  YOUTH_EINVAL otherwise, with the
 * schedule left as it was. */
int youth_loop_set_levels(youth_loop* lp, const youth_rgbd_level* levels, int n);
/* At most cap levels into out (nullable with cap 0); returns their number. */
int youth_loop_get_levels(const youth_loop* lp, youth_rgbd_level* out, int cap);

/* The measures of the candidates the last youth_loop_close verified, accepted
 * or not (i = k, j = kf, w = 1 accepted / 0 rejected): at most cap into out.
 * Returns their number. */
int youth_loop_last_verified(const youth_loop* lp, youth_loop_edge* out, int cap);

int youth_loop_keyframes(const youth_loop* lp);
/* The edges so far, in the order found: at most cap into out (nullable with
 * cap 0); returns the number of edges the object holds. */
int youth_loop_edges(youth_loop* lp, youth_loop_edge* out, int cap);
/* Keyframe kf's pose and tag (each nullable). */
int youth_loop_get_keyframe(const youth_loop* lp, int kf, double T_wc[16], uint32_t* tag);
/* Forget every keyframe and edge. */
int youth_loop_clear(youth_loop* lp);

/* ------------------------------------------------------------ pose graph --
 * Host only, fp64.  Nodes are camera -> world poses X [n][16]; edge (i, j, Z, w)
 * has E = Z^-1 X_i^-1 X_j and e = [Log_SO3(R_E); t_E]; the cost is
 * sum w (w_rot |e_w|^2 + w_trans |e_t|^2).  Node 0 is fixed.  Gauss-Newton with
 * analytic Jacobians and a dense Cholesky of the 6 (n - 1) system, at most
 * max_iters iterations, stopping when the update's largest entry is below
 * 1e-12; rotations are re-orthonormalised after every update. */
typedef struct youth_posegraph_params {
    double w_rot, w_trans;   /* finite, > 0 */
    int    max_iters;        /* >= 0 */
} youth_posegraph_params;

/* 1, 1, 20. */
youth_posegraph_params youth_posegraph_default_params(void);

/* X in/out.  cost_before / cost_after nullable; params NULL: the defaults.
 * YOUTH_EINVAL for non-finite input, n < 2, n > YOUTH_LOOP_MAX_KEYFRAMES, an
 * edge index out of range or i == j, a weight < 0, or a graph whose system is
 * not positive definite (a node no edge reaches); YOUTH_ENOMEM.  X is written
 * only on success; the text of the last error is youth_posegraph_last_error(). */
int youth_posegraph_optimize(int n, double* X, int n_edges, const youth_loop_edge* edges,
                             const youth_posegraph_params* params, double* cost_before,
                             double* cost_after);
const char* youth_posegraph_last_error(void);

/* Re-hang n_frames poses on optimised keyframes: kf_frame [n_kf] ascending
 * frame indices of the keyframes (kf_frame[0] = 0), X_kf_old / X_kf_new their
 * poses before and after; X [n_frames][16] in/out:
 * X'_f = X_new_kf (X_old_kf^-1 X_f) for the last keyframe kf at or before f. */
int youth_posegraph_interpolate(int n_frames, double* X, int n_kf, const int32_t* kf_frame,
                                const double* X_kf_old, const double* X_kf_new);

/* ------------------------------------------------------------ the drop-in --
 * With YOUTH_SLAM_LOOP=1 in the environment of initSlamModule (and colour
 * frames: YOUTH_SLAM_RGBD=1 or YOUTH_SLAM_MAP_COLOR=1 carries them) the SLAM
 * module keeps keyframes and closes loops in its worker.  A recorded frame
 * becomes a keyframe when it has moved YOUTH_SLAM_LOOP_KF_M metres (default
 * 0.10) or YOUTH_SLAM_LOOP_KF_DEG degrees (default 10) from the last one; the
 * first frame always is.  YOUTH_SLAM_LOOP_MIN_GAP overrides min_gap.
 * YOUTH_SLAM_LOOP_LEVELS sets the closer's level schedule: `auto`
 * (youth_rgbd_default_levels for the frame size) or a list stride:iterations
 * such as 8:10,1:10; unset: none; a malformed value is logged once and
 * ignored.  The live
 * trajectory is never rewritten.  saveSlamMap then writes the optimised
 * keyframe poses to <map_file>_keyframes.txt and the corrected trajectory to
 * <map_file>_trajectory_closed.txt.  Without the variable the module behaves
 * as it does without this header and these return 0. */
int youth_slam_loop_keyframes(void);
int youth_slam_loop_edges(youth_loop_edge* out, int cap);   /* as youth_loop_edges */
/* The keyframes' trajectory indices, at most cap into frame_index; returns their number. */
int youth_slam_loop_keyframe_frames(int32_t* frame_index, int cap);
/* The corrected trajectory: optimise the keyframes, re-hang every frame; at
 * most n poses into T_wc [n][16]; returns their number. */
int youth_slam_loop_trajectory(int n, double* T_wc);

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_LOOP_H */
