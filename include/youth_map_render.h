/*
 * youth_map_render.h — the voxel map seen from a pose: int16 depth and uint8
 * RGB frames rendered from a youth_map on the GPU.  Included
 * by youth_map.h, of whose interface it is a part; it stands in a file of its
 * own so that youth_map.h keeps the sixteen functions it declared before.
 *
 * Definition.  A view is a world -> camera pose V (fp32 row-major 3x4),
 * intrinsics K, a size W x H, max_splat (1..16) and min_count (>= 1).  All
 * arithmetic is fp32 with every operation rounded (IEEE division, no fma).
 * Each stored voxel (ix, iy, iz) with count >= min_count does the following.
 *   centroid, per axis a:
 *     c = (float)sum_q[a] / (float)count
 *     p_a = ((float)i_a + (c + 0.5f) * 0.00390625f) / vpm
 *   camera point, per row r of V:
 *     ((V[r][0]*p_x + V[r][1]*p_y) + V[r][2]*p_z) + V[r][3]     -> (xc, yc, zc)
 *   depth:
 *     d = rintf(zc * K.depth_scale)
 *     skipped unless zc > 0 and 1 <= d <= 32767 (NaN fails)
 *   pixel:
 *     uf = (xc * K.fx) / zc + K.cx;  vf = (yc * K.fy) / zc + K.cy
 *     skipped unless -32 < uf < W + 32 and -32 < vf < H + 32 (NaN fails),
 *     tested in float before any integer conversion
 *   footprint:
 *     s = clamp(ceilf(K.fx / (vpm * zc)), 1, max_splat)   (clamped in float,
 *         then converted: an infinite quotient gives max_splat)
 *     h = 0.5f * (float)(s - 1)
 *     u0 = (int)floorf((uf - h) + 0.5f);  v0 likewise from vf
 *     the voxel covers the pixels [u0, u0+s) x [v0, v0+s), clipped to the frame
 *   value:
 *     mean colour per channel (sum_c + count/2) / count in uint32 (it cannot
 *     overflow: 2^24 * 255 + 2^23 < 2^32)
 *     the 64-bit value is (d << 24) | (R << 16) | (G << 8) | B
 * A pixel takes the MINIMUM value over all voxels that cover it: the nearest
 * depth, ties broken by the smaller packed colour.  An uncovered pixel is depth
 * 0 and colour 0.  Minimum is associative and commutative, so the output is one
 * bit pattern for any launch geometry, slot order or kernel variant.
 *
 * Bias.  The z-buffer keeps the nearest voxel, so over a noisy map the depth
 * is biased toward the camera by about the noise's spread.
 *
 * K must be finite with fx, fy, depth_scale > 0.  Rendering reads the map and
 * never changes it.  The z-buffer belongs to the map: a map renders one call
 * at a time.  Two kernels give the same bytes: with YOUTH_MAP_RENDER_QUEUE=1
 * (read at youth_map_create; the default) a workgroup compacts its surviving
 * voxels into an LDS queue and all its threads drain the covered pixels, with
 * =0 every thread walks the footprints of its own voxels.
 */
#ifndef YOUTH_MAP_RENDER_H
#define YOUTH_MAP_RENDER_H

#include "youth_map.h"

#ifdef __cplusplus
extern "C" {
#endif

struct youth_map_view {
    int W, H;            /* 1 <= W, H <= 16384, W*H <= 2^26 */
    int max_splat;       /* 1..16; 0 = 16 */
    uint32_t min_count;  /* >= 1; 0 = 1 */
};

/* Host only, no device needed.  V = the inverse of the rigid camera -> world
 * pose T_world (fp64 row-major 4x4; its last row is not read): rotation
 * R' = transpose(R), translation
 *   t'_r = -((R[0][r]*t0 + R[1][r]*t1) + R[2][r]*t2)      in fp64, in that order,
 * each of the 12 values rounded to fp32.  Any non-finite input or output is
 * YOUTH_EINVAL. */
int youth_map_view_from_pose(const double T_world[16], float V[12]);

/* n_views (1..65535) views of one size from device poses:
 *   d_V      [n][12] fp32 world -> camera
 *   d_depth  [n][H][W] int16
 *   d_rgb    [n][H][W][3] uint8, or NULL
 *   K        NULL: the viewer's intrinsics for W x H (youth_viewer.h)
 * Enqueued on `stream` (NULL: the map's stream); asynchronous.  The ordering
 * rule of youth_map_integrate_device holds: work given on another stream must
 * be ordered by the caller against the map's other calls.  A violated limit is
 * YOUTH_EINVAL with an error text and no launch. */
int youth_map_render_device(youth_map* map, int n_views, const struct youth_map_view* view,
                            const youth_intrinsics* K, const float* d_V, int16_t* d_depth,
                            uint8_t* d_rgb, void* stream);

/* One view into host buffers.  T_world: host fp64 row-major 4x4 camera ->
 * world (a SLAM trajectory entry), through youth_map_view_from_pose; NULL =
 * the identity.  rgb may be NULL.  Returns when the buffers are written. */
int youth_map_render_host(youth_map* map, const struct youth_map_view* view,
                          const youth_intrinsics* K, const double* T_world, int16_t* depth,
                          uint8_t* rgb);

/* The drop-in (youth_map.h): the SLAM module's map rendered into host
 * buffers; K NULL = the intrinsics the module tracks W x H frames with;
 * T_world NULL = the last recorded pose.  Runs under the trajectory lock, so
 * no resetSlam falls between reading the pose and rendering.  1 rendered; 0
 * when the module keeps no map, no pose is recorded yet or the render failed
 * (outputs untouched). */
int youth_slam_map_render(const struct youth_map_view* view, const youth_intrinsics* K,
                          const double* T_world, int16_t* depth, uint8_t* rgb);

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_MAP_RENDER_H */
