/*
 * youth_rgbd.h — RGB-D alignment: a photometric term beside point-to-plane ICP.
 *
 * Depth alone leaves the pose undetermined where the scene is a near-frontal
 * wall (a valley of the point-to-plane cost).  This path adds
 * the colour frame the sensor delivers with every depth frame: each
 * Gauss-Newton iteration sums the geometric term of youth_icp.h (spec a7/a8 in
 * the survey arithmetic, unchanged) and a photometric term on 8-bit intensity
 * into one 6x6 system.  Opt-in and beside the depth-only paths, which compute
 * what they always did.  Definition: DESIGN.md §13; numpy restatement:
 * tests/rgbd_truth.py.
 *
 *   intensity   Y = (77 R + 150 G + 29 B + 128) >> 8, uint8 [H][W]
 *   target      gx = Y[v][u+1] - Y[v][u-1], gy = Y[v+1][u] - Y[v-1][u],
 *               photometric-valid iff 1 <= u <= W-2 and 1 <= v <= H-2
 *   per pixel   (accepted by the geometric gate, target pixel (u', v') valid)
 *               It = Y_t[v'][u'] + 0.5 (gx du + gy dv),  du = uf - u', dv = vf - v'
 *               rp = (It - Y_s[v][u]) w,  w = lambda / 255
 *               h  = (gx kx / P'z, gy ky / P'z, -(hx P'x + hy P'y) / P'z),
 *               kx = 0.5 w fx, ky = 0.5 w fy;  Jp = [P' x h, h]
 *   sums        A = sum J J^T + sum Jp Jp^T, b = sum J r + sum Jp rp (exact fp64
 *               products), then the solve and update of youth_icp.h (a10)
 *
 * Plain C99; streams travel as void*; return codes are youth_icp.h's YOUTH_OK /
 * YOUTH_E*.  Lives in libyouth_icp.so.
 */
#ifndef YOUTH_RGBD_H
#define YOUTH_RGBD_H

#include <stdint.h>

#include "youth_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fp64 values in one record of the joint normal equations:
 * [0..20] upper triangle of A, [21..26] b, [27] sum r^2 and [28] count of the
 * geometric term, [29] sum rp^2 and [30] count of the photometric term.  With
 * lambda = 0 the first YOUTH_NEQ values are the depth-only record. */
#define YOUTH_RGBD_NEQ 31

typedef struct youth_rgbd_params {
    int   iters;        /* fixed Gauss-Newton iterations, no early exit */
    float dist_thresh;  /* the geometric gate |P' - P_t| < dist_thresh (m) */
    float lambda;       /* metres of geometric residual per unit of intensity in [0, 1] */
} youth_rgbd_params;

/* 10 iterations, dist_thresh 0.10, lambda 0.1. */
youth_rgbd_params youth_rgbd_default_params(void);

typedef struct youth_rgbd_ctx youth_rgbd_ctx;

/* Human-readable text of the last error on this thread ("" if none). */
const char* youth_rgbd_last_error(void);

/* Device workspace for max_frames pairs of W x H (the limits of
 * youth_icp_create: 3 <= W, H <= 16384, W*H <= 2^26, max_frames >= 2).  K NULL:
 * the viewer's intrinsics; params NULL: the defaults.  iters >= 0, dist_thresh
 * and lambda finite, dist_thresh > 0, lambda >= 0 (NULL and YOUTH_EINVAL in
 * youth_rgbd_last_error otherwise; YOUTH_ENODEV without a device).  The
 * environment variable YOUTH_RGBD_CHUNKS=k, read here, makes every iteration
 * launch k workgroups per pair (at most one per 1024 pixels) instead of the
 * planned number: a test knob, results move in the last bits of the sums only. */
youth_rgbd_ctx* youth_rgbd_create(int device, int W, int H, int max_frames,
                                  const youth_intrinsics* K, const youth_rgbd_params* params);
void youth_rgbd_destroy(youth_rgbd_ctx* ctx);

/* RGB [n][H][W][3] -> intensity [n][H][W], both uint8 on `device`;
 * asynchronous on `stream`.  0 <= n <= 65535. */
int youth_rgbd_luma_device(int device, const uint8_t* d_rgb, uint8_t* d_gray, int n, int W, int H,
                           void* stream);

/* Device-resident align of n_pairs pairs with the semantics of
 * youth_icp_align_pairs_device: depth [n_pairs][H][W] int16, intensity
 * [n_pairs][H][W] uint8, all on the device and alive until the align has
 * completed on `stream`; T_init nullable HOST [n_pairs][16] fp64 (finite);
 * d_T_out nullable DEVICE [n_pairs][16] fp32; asynchronous.  n_pairs <=
 * max_frames.  One launch per iteration plus the target preps. */
int youth_rgbd_align_pairs_device(youth_rgbd_ctx* ctx, const int16_t* d_src_depth,
                                  const uint8_t* d_src_gray, const int16_t* d_dst_depth,
                                  const uint8_t* d_dst_gray, int n_pairs, const double* T_init,
                                  float* d_T_out, void* stream);

/* Streamed sequence: the n_frames - 1 relative poses T_k (P_k = T_k P_{k+1}) of
 * d_depth / d_gray [n_frames][H][W]; every frame is prepped once.
 * 2 <= n_frames <= max_frames + 1. */
int youth_rgbd_align_sequence_device(youth_rgbd_ctx* ctx, const int16_t* d_depth,
                                     const uint8_t* d_gray, int n_frames, float* d_T_out,
                                     void* stream);

/* Block until the context's last enqueued work on `stream` is done. */
int youth_rgbd_sync(youth_rgbd_ctx* ctx, void* stream);

/* Results of the last align (synchronises): T64 [n][16] fp64, T32 [n][16] fp32,
 * status [n] YOUTH_STATUS_* bits; each nullable. */
int youth_rgbd_get_poses(youth_rgbd_ctx* ctx, int n, double* T64, float* T32, int32_t* status);

/* Per iteration of the last align, the record's values 27..30:
 * stats [n][iters][4] = sum r^2, geometric count, sum rp^2, photometric count. */
int youth_rgbd_get_stats(youth_rgbd_ctx* ctx, int n, int iters, double* stats);

/* --- Level schedule: coarse to fine -----------------------
 * The align converges only from nearby; run first on a sub-sampled copy of
 * the frames it converges from much further.  A level (s, iters), s one of
 * 1, 2, 4, 8, 16, is the align above, unchanged, on
 *
 *   frames   W_s = (W + s - 1) / s, H_s likewise;
 *            depth_s[j][i] = depth[s j][s i], gray_s[j][i] = gray[s j][s i]
 *            (plain decimation, no averaging)
 *   camera   K_s = {fx / s, fy / s, cx / s, cy / s, depth_scale}: fp32
 *            divisions by a power of two, hence exact, so the back-projected
 *            point of level pixel (i, j) is bit for bit the full-resolution
 *            point of pixel (s i, s j)
 *
 * with normals and intensity gradients formed on the level's own grid by the
 * rules above.  A schedule is 1 .. YOUTH_RGBD_MAX_LEVELS levels of strictly
 * decreasing stride, every W_s, H_s >= 3, iters >= 0.  Level 0 starts from
 * T_init (or the identity), level l from level l - 1's final fp64 pose; each
 * level runs with the context's dist_thresh and lambda; the result is the last
 * level's pose (its stride need not be 1) and the status the OR of all levels'
 * status words.  Numpy restatement: tests/rgbd_levels_truth.py. */
typedef struct youth_rgbd_level { int stride; int iters; } youth_rgbd_level;
#define YOUTH_RGBD_MAX_LEVELS 4

/* The schedule the measurements of §16 were made with: the largest s of 8, 4, 2
 * with W / s >= 80 and H / s >= 60 at 10 iterations, then 1:10 (8 at 640x480,
 * 4 at 320x240, 2 at 160x120); 1:10 alone for smaller frames.  Returns the
 * number of levels written to out. */
int youth_rgbd_default_levels(int W, int H, youth_rgbd_level out[YOUTH_RGBD_MAX_LEVELS]);

/* Set the context's schedule (n = 0: off, the default).  With one set,
 * youth_rgbd_align_pairs_device and youth_rgbd_align_sequence_device run it
 * (one decimation launch for all coarse levels and frames of the call, every
 * frame prepped once per level, no host synchronisation between levels) and
 * params.iters is not used; youth_rgbd_get_poses and youth_rgbd_get_stats
 * report the last level, the former with the OR status.  The streaming
 * tracker runs a schedule of its own (youth_rgbd_track_set_levels below), not
 * this one: youth_rgbd_track_submit is YOUTH_EINVAL while this one is set, and
 * this call while frames are pending.  YOUTH_EINVAL leaves the schedule as it
 * was.  Allocates one workspace per coarse level. */
int youth_rgbd_set_levels(youth_rgbd_ctx* ctx, const youth_rgbd_level* levels, int n);

/* At most cap levels into out (nullable with cap 0); returns their number. */
int youth_rgbd_get_levels(const youth_rgbd_ctx* ctx, youth_rgbd_level* out, int cap);

/* One level of the last scheduled align (synchronises): its final poses T64
 * [n][16] and its own status words [n]; each nullable. */
int youth_rgbd_get_level_poses(youth_rgbd_ctx* ctx, int level, int n, double* T64, int32_t* status);

/* youth_rgbd_get_stats of one level; iters: that level's. */
int youth_rgbd_get_level_stats(youth_rgbd_ctx* ctx, int level, int n, int iters, double* stats);

/* --- Stage-level entry points (validation / parity tests) --------------- */

/* The decimation alone (k_rgbd_decimate, the single-stride case of the
 * schedule's launch): n frames depth [n][H][W] int16 and intensity [n][H][W]
 * uint8 on `device` -> d_depth_out / d_gray_out [n][H_s][W_s], nothing written
 * outside them.  stride 2, 4, 8 or 16; 0 <= n <= 65535; asynchronous on
 * `stream`. */
int youth_rgbd_decimate_device(int device, const int16_t* d_depth, const uint8_t* d_gray, int n,
                               int W, int H, int stride, int16_t* d_depth_out, uint8_t* d_gray_out,
                               void* stream);

/* The target preparation alone: n frames of `channels` = 3 (RGB [n][H][W][3])
 * or 1 (intensity [n][H][W]) on the device -> d_gray (nullable) [n][H][W] uint8
 * and d_photo (nullable) [n][H*W] packed words: bits 0..7 Y, 8..16 gx + 255,
 * 17..25 gy + 255, bit 31 the valid bit (gx = gy = 0 where it is clear).
 * Asynchronous on `stream`. */
int youth_rgbd_prep_device(youth_rgbd_ctx* ctx, const uint8_t* d_in, int channels, int n,
                           uint8_t* d_gray, uint32_t* d_photo, void* stream);

/* One association + reduction pass for one pair of HOST frames at a given fp32
 * pose T12 (3x4 row-major): neq31 [YOUTH_RGBD_NEQ].  Synchronous. */
int youth_rgbd_reduce_host(youth_rgbd_ctx* ctx, const int16_t* src_depth, const uint8_t* src_gray,
                           const int16_t* dst_depth, const uint8_t* dst_gray, const float* T12,
                           double* neq31);

/* Host frames in (depth [n_frames][H][W] int16, rgb [n_frames][H][W][3]),
 * relative poses out: T_rel [n_frames - 1][16] fp64 (P_k = T_rel[k] P_{k+1}) and
 * status [n_frames - 1] (nullable).  Upload, intensity, the sequence align and
 * the download; synchronous.  Returns n_frames - 1 or a negative YOUTH_E* code. */
int youth_rgbd_track_host_sequence(youth_rgbd_ctx* ctx, const int16_t* depth, const uint8_t* rgb,
                                   int n_frames, double* T_rel, int32_t* status);

/* --- Streaming tracker -----------------------------------
 * Frames submitted as they arrive, each aligned to the frame before it,
 * results collected in order: youth_icp_track_submit / _collect with colour.
 * Frames are HOST pointers, depth int16 [H][W] and RGB uint8 [H][W][3].  A
 * frame inside a buffer of youth_icp_host_alloc (page-locked; colour takes
 * (3 W H + 1) / 2 of its values) is fetched by the GPU in place and must stay
 * unchanged until it has been collected; any other frame is copied into
 * page-locked staging before the call returns.  The tracker shares the
 * context's workspace with the entry points above: do not call those while
 * frames are pending; after one of them the next frame starts a new sequence.
 * An RGB-D align contains no wait between workgroups, so its status never
 * carries YOUTH_STATUS_TIMEOUT and there is no realign. */

/* Frames per submission, 1 <= b <= YOUTH_TRACK_MAX_BATCH (default 1).  Fixes
 * the launch geometry of every later submission, whatever its size, so a
 * frame's pose does not depend on how the sequence was split.  Needs
 * max_frames >= 2 b and no frame pending.  Returns the previous value. */
int youth_rgbd_track_set_batch(youth_rgbd_ctx* ctx, int b);

/* Filter every ingested depth frame once (youth_filter.h) before anything else
 * reads it; NULL (the default) switches it off.  No frame pending. */
int youth_rgbd_track_set_depth_filter(youth_rgbd_ctx* ctx, const youth_filter_params* P);

/* The streaming tracker's own schedule (n = 0: off, the default).  Rules of
 * youth_rgbd_set_levels, and the last level has stride 1.  With one set every
 * tracked pair is the scheduled align of that pair from the identity: level l
 * on the plainly decimated frames (with the depth filter on: of the filtered
 * frame), from level l - 1's fp64 pose read on the device; params.iters is not
 * used; youth_rgbd_track_collect returns the last level's pose and the OR of
 * all levels' status words.  No frame pending.  The next frame starts a new
 * sequence.  YOUTH_EINVAL leaves it as it was.  Allocates one workspace per
 * coarse level; youth_rgbd_track_set_batch keeps the schedule. */
int youth_rgbd_track_set_levels(youth_rgbd_ctx* ctx, const youth_rgbd_level* levels, int n);

/* At most cap levels into out (nullable with cap 0); returns their number. */
int youth_rgbd_track_get_levels(const youth_rgbd_ctx* ctx, youth_rgbd_level* out, int cap);

/* Of the frame youth_rgbd_track_collect returned last: every level's final
 * pose T64 [n_levels][16] and own status word [n_levels] (each nullable).
 * Returns n_levels, 0 if that frame had no reference or no schedule is set. */
int youth_rgbd_track_last_levels(youth_rgbd_ctx* ctx, double* T64, int32_t* status);

/* 1 <= n_frames <= b frames, asynchronous; frame i is aligned to frame i - 1,
 * the first to the last frame submitted before.  At most two submissions may be
 * in flight (YOUTH_EINVAL beyond). */
int youth_rgbd_track_submit(youth_rgbd_ctx* ctx, const int16_t* const* depth,
                            const uint8_t* const* rgb, int n_frames);

/* The oldest uncollected frame: returns its YOUTH_STATUS_* bits or a negative
 * code; T_rel [16] fp64 with P_ref = T_rel P_new; *has_ref (nullable) 0 and
 * the identity for the first frame after create or reset. */
int youth_rgbd_track_collect(youth_rgbd_ctx* ctx, double* T_rel, int* has_ref);

/* Frames submitted and not yet collected (0 for NULL). */
int youth_rgbd_track_pending(const youth_rgbd_ctx* ctx);

/* The next frame starts a new sequence.  No frame pending (YOUTH_EINVAL). */
int youth_rgbd_track_reset(youth_rgbd_ctx* ctx);

/* Stage entry: the ingest kernel alone (k_rgbd_pull).  m <=
 * YOUTH_TRACK_MAX_BATCH host frames -> DEVICE d_depth [m][H][W] int16, d_gray
 * [m][H][W] uint8 (the intensity above) and, unless NULL, d_rgb [m][H][W][3].
 * Asynchronous on `stream`; frames outside youth_icp_host_alloc buffers are
 * staged first. */
int youth_rgbd_pull_host(youth_rgbd_ctx* ctx, const int16_t* const* depth,
                         const uint8_t* const* rgb, int m, int16_t* d_depth, uint8_t* d_gray,
                         uint8_t* d_rgb, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_RGBD_H */
