/*
 * youth_map.h — C-ABI of the voxel map on MI355X: world-frame point fusion of
 * the tracked frames into one bounded, de-duplicated, coloured point map
 * (DESIGN.md §10).
 *
 * The reference keeps no map of its own making (saveSlamMap hands the job to
 * ORB-SLAM3, SLAM.cpp:177-198); the viewer list (youth_viewer.h) is one
 * frame's points, emitted again every frame.  A youth_map accumulates every
 * integrated frame's world points in a sparse voxel grid on the GPU: a hash
 * table of integer records, so the map is one bit pattern whatever the launch
 * shape, the order of the frames or their split over calls.
 *
 * Definition.  A map has a resolution vpm (voxels per metre, fp32 > 0) and a
 * slot capacity.  Pixel (u, v) of a frame with depth d, intrinsics K and
 * camera -> world pose T (fp32 row-major 3x4) contributes iff d > 0 and
 * (max_depth == 0 or d <= max_depth).  Its world point (X, Y, Z) is the one
 * youth_cloud_build_device_posed emits, before the display flip:
 *   z = (float)d / K.depth_scale; x = (((float)u - K.cx) * z) / K.fx; y likewise;
 *   X = fmaf(T[2], z, fmaf(T[1], y, fmaf(T[0], x, T[3])))        (Y, Z likewise)
 * (no pose = the identity matrix through the same chain).  Per axis a:
 *   s = a * vpm; fl = floorf(s);
 *   out of range (skipped, counted) unless -1048576.0f <= fl < 1048576.0f
 *   (NaN fails too); i = (int32)fl; f = s - fl; q = min(255, (uint32)(f * 256.0f)).
 * The voxel is (ix, iy, iz); its record sums count, q per axis and R, G, B
 * with unsigned 32-bit integer adds.  A voxel may take 2^24 points before a
 * sum can wrap (2^24 * 255 < 2^32); at 30 Hz that is more than six days of one
 * pixel-sized surface patch seen by every frame.
 *
 * Full table.  Probing is bounded: a point that finds neither its key nor an
 * empty slot within the bound is dropped and counted (stats.dropped), never
 * waited for.  Which points were dropped may differ between runs; everything
 * else is exact.
 *
 * A map is used by one thread at a time; its device calls on one stream run in
 * order.  Plain C99, no HIP or torch types (streams travel as void*).  Entry
 * points return YOUTH_OK (0) / a count >= 0, or a negative YOUTH_E* code
 * (youth_icp.h); the text of the last error is youth_map_last_error().
 */
#ifndef YOUTH_MAP_H
#define YOUTH_MAP_H

#include <stddef.h>
#include <stdint.h>

#include "youth_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One voxel, 40 bytes of integers. */
typedef struct youth_voxel {
    int32_t  ix, iy, iz;   /* floor(world * vpm) per axis, each in [-2^20, 2^20) */
    uint32_t count;        /* points fused into the voxel */
    uint32_t sum_q[3];     /* sum of q per axis (q: the point's place inside the voxel, 0..255) */
    uint32_t sum_c[3];     /* sum of R, G, B; all 0 without colour */
} youth_voxel;

/* Counters since create / the last clear (a struct tag only: the function of
 * the same name fills it). */
struct youth_map_stats {
    uint64_t integrated;    /* points added to a voxel */
    uint64_t out_of_range;  /* contributing pixels whose voxel index left [-2^20, 2^20) */
    uint64_t dropped;       /* points that found no slot within the probe bound */
    uint64_t occupied;      /* slots holding a voxel (= youth_map_voxels); an upper bound on
                               the voxels once something was removed (youth_map_remove.h) */
    uint64_t direct;        /* points sent straight to the global table: their workgroup's
                               LDS table was full (every point with YOUTH_MAP_LDS=0) */
    uint64_t capacity;      /* slots of the table */
};

typedef struct youth_map youth_map;

/* A map of vpm voxels per metre (finite, > 0) with capacity_slots slots
 * (rounded up to a power of two; 64 <= slots <= 2^28) on HIP device `device`.
 * The environment variable YOUTH_MAP_LDS=0, read here, sends every point
 * straight to the global table (no per-workgroup aggregation);
 * YOUTH_MAP_RENDER_QUEUE=0, read here too, picks the render's other splat
 * kernel (youth_map_render.h).  NULL on failure. */
youth_map* youth_map_create(int device, float vpm, long long capacity_slots);
void youth_map_destroy(youth_map* map);
const char* youth_map_last_error(void);

/* Empty the map and zero its counters (asynchronous, the map's stream). */
int youth_map_clear(youth_map* map);

/* Pixels with d > max_depth (raw depth units) do not contribute; 0 = no gate
 * (the default).  Applies to the integrations enqueued after it. */
int youth_map_set_max_depth(youth_map* map, int max_depth);

/* Device-resident batch of n_frames W x H frames (W, H <= 16384, W*H <= 2^26,
 * n_frames <= 65535):
 *   d_depth   [n][H][W] int16, raw depth units
 *   d_rgb     [n][H][W][3] uint8 RGB, or NULL (sum_c stays 0)
 *   K         NULL: the viewer's intrinsics (youth_viewer.h)
 *   d_T_world [n][12] fp32 row-major 3x4 camera -> world, or NULL (identity)
 * Enqueued on `stream` (NULL: the map's stream); asynchronous.  Work given on
 * another stream must be ordered by the caller against clear / extract /
 * stats, which run on the map's stream. */
int youth_map_integrate_device(youth_map* map, const int16_t* d_depth, const uint8_t* d_rgb,
                               int n_frames, int W, int H, const youth_intrinsics* K,
                               const float* d_T_world, void* stream);

/* One host frame.  T_world: host fp64 row-major 4x4 camera -> world (a SLAM
 * trajectory entry) or NULL; its first 12 entries are rounded to fp32 (the
 * rule of youth_viewer.h) and must be finite (else YOUTH_EINVAL).  The host
 * buffers are free again on return. */
int youth_map_integrate_host(youth_map* map, const int16_t* depth, const uint8_t* rgb, int W,
                             int H, const youth_intrinsics* K, const double* T_world);

/* Slots holding a key: the voxels in the map, or an upper bound on them once
 * something was removed (youth_map_remove.h); waits for the map's stream. */
long long youth_map_voxels(youth_map* map);

/* The map's records sorted by (iz, iy, ix) into out[cap]; returns their exact
 * number, or YOUTH_EINVAL when cap is below youth_map_voxels.  Waits for the
 * map's stream; integration may continue afterwards. */
int youth_map_extract(youth_map* map, youth_voxel* out, int cap);

/* The counters; waits for the map's stream. */
int youth_map_stats(youth_map* map, struct youth_map_stats* stats);

/* Wait for the work enqueued on `stream` (NULL: the map's stream). */
int youth_map_sync(youth_map* map, void* stream);

/* Host only, no device needed.  The derived float form of n records:
 * xyzrgb[k] = {x, y, z, r, g, b} with, per axis,
 *   (i + ((double)sum_q / count + 0.5) / 256) / vpm      (fp64, rounded to fp32)
 * and colour (double)sum_c / count / 255.  A record with count 0 is invalid
 * (YOUTH_EINVAL). */
int youth_map_points(const youth_voxel* voxels, int n, float vpm, float* xyzrgb);

/* ASCII PLY, one vertex per record in the given order: float x y z, uchar
 * red green blue (the mean colour rounded), uint count. */
int youth_map_write_ply(const char* path, const youth_voxel* voxels, int n, float vpm);

/* ------------------------------------------------------------ the drop-in --
 * With YOUTH_SLAM_MAP_VPM=<float> in the environment of initSlamModule
 * (optional YOUTH_SLAM_MAP_SLOTS, default 4194304, and
 * YOUTH_SLAM_MAP_MAX_DEPTH, raw depth units) the SLAM module keeps a map:
 * its worker integrates every frame whose pose it records, with that pose.
 * processSlamFrame does not queue colour, so the module's map is colourless
 * (sum_c = 0).  resetSlam and the start of a new sequence empty it;
 * saveSlamMap additionally writes <map_file>_map.ply.  Without the variable
 * the module behaves as it does without this header. */
long long youth_slam_map_voxels(void);                    /* 0 when disabled */
int youth_slam_map_extract(youth_voxel* out, int cap);    /* as youth_map_extract; 0 when disabled */
float youth_slam_map_vpm(void);                           /* 0 when disabled */


#ifdef __cplusplus
}
#endif

/* Rendering the map into depth and colour frames from any pose (DESIGN.md
 * §12): part of this interface, kept in a file of its own. */
#include "youth_map_render.h"

/* Taking frames out of the map again, moving them to other poses and
 * re-integrating the SLAM module's map after a loop closure (DESIGN.md §10,
 * §15): part of this interface, kept in a file of its own. */
#include "youth_map_remove.h"

#endif /* YOUTH_MAP_H */
