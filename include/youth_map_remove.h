/*
 * youth_map_remove.h -- the voxel map's second half (included by youth_map.h,
 * DESIGN.md §10 and §15): taking integrated frames out of a youth_map again,
 * moving them to other poses, compacting the table, and the SLAM module's
 * re-integration of its map after a loop closure.  Plain C99; conventions and
 * error codes as in youth_map.h.
 */
#ifndef YOUTH_MAP_REMOVE_H
#define YOUTH_MAP_REMOVE_H

#include "youth_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Removal.
 * Every accumulation is an unsigned 32-bit add, so a frame can be taken out
 * again by the same sums subtracted.  The contract: removal is exact, the map
 * being bit for bit the one the remaining frames alone would give, iff the
 * frame went in with bit-identical inputs (depth, colour or its absence, W, H,
 * K, the fp32 pose, the map's max_depth and vpm) and stats.dropped == 0, then
 * and since.  Nothing is checked beyond what the counters of
 * youth_map_remove_stats show: a point whose voxel is not in the table is
 * counted as missing and skipped; a voxel whose count was smaller than what is
 * subtracted counts an underflow event (how many depends on how the launch
 * grouped its points; only zero against non-zero is defined) and the map is
 * invalid until cleared.
 *
 * A voxel emptied by removal keeps its slot (count 0, after an exact removal
 * every sum 0), which is reused when the voxel is integrated again.  Such a
 * slot is no record: youth_map_extract, the renders and the PLY skip it.
 * youth_map_voxels and stats.occupied keep meaning "slots holding a key": once
 * something was removed, and until youth_map_compact, they are an upper bound
 * on the number of records (and the room youth_map_extract asks for);
 * youth_map_extract returns the exact number. */

/* As youth_map_integrate_device, taking the frames out; removes with the
 * map's current max_depth. */
int youth_map_remove_device(youth_map* map, const int16_t* d_depth, const uint8_t* d_rgb,
                            int n_frames, int W, int H, const youth_intrinsics* K,
                            const float* d_T_world, void* stream);

/* As youth_map_integrate_host, taking the frame out. */
int youth_map_remove_host(youth_map* map, const int16_t* depth, const uint8_t* rgb, int W, int H,
                          const youth_intrinsics* K, const double* T_world);

/* Moves n_frames frames from the poses d_T_old to the poses d_T_new (both
 * device [n][12] fp32, neither NULL): two launches on `stream`, the removal
 * first.  A frame whose twelve floats are bitwise equal in the two arrays is
 * skipped by both. */
int youth_map_move_device(youth_map* map, const int16_t* d_depth, const uint8_t* d_rgb,
                          int n_frames, int W, int H, const youth_intrinsics* K,
                          const float* d_T_old, const float* d_T_new, void* stream);

/* Rebuilds the table without the vacated slots: every record moves to a fresh
 * table of the same capacity, which replaces the old one; stats.occupied
 * becomes the number of records, the other counters carry over.  Records and
 * renders are the same before and after.  Waits for the map's stream; work on
 * other streams must have finished.  All or nothing: YOUTH_ENOMEM when the
 * second table cannot be allocated or a voxel found no slot in it within the
 * probe bound, and the map is then unchanged. */
int youth_map_compact(youth_map* map);

/* Counters of removal since create / the last clear, and one scan of the
 * table made by this call (a struct tag only, as youth_map_stats). */
struct youth_map_remove_stats {
    uint64_t removed;    /* points taken out of a voxel (counted as stats.integrated is) */
    uint64_t missing;    /* points whose voxel was not in the table */
    uint64_t underflow;  /* events: a voxel's count was below what was subtracted */
    uint64_t live;       /* slots holding a record (count > 0) */
    uint64_t vacant;     /* slots holding a key with count 0 */
    uint64_t stale;      /* vacant slots with a non-zero sum: an inexact removal */
};
int youth_map_remove_stats(youth_map* map, struct youth_map_remove_stats* out);

/* ------------------------------------------------------------ the drop-in --
 * Re-integration after a loop closure.  With YOUTH_SLAM_MAP_KEEP=<n> (read
 * with the YOUTH_SLAM_MAP_* variables of youth_map.h; unset or 0: off) the module keeps, on the device
 * and in recording order, every integrated frame's depth, its colour when
 * carried, and the fp32 pose it was integrated with, for at most n frames
 * (grown in chunks of 64).  Frames past n, past a failed allocation, or of
 * another size than the first are integrated but not kept (logged once).
 * resetSlam and a new sequence's origin empty the store with the map.
 *
 * youth_slam_map_reintegrate moves kept frame i < n from its stored pose to
 * T_wc[i] (host fp64 row-major 4x4, rounded to fp32 by the rule of
 * youth_map_integrate_host) and stores the new pose.  Any corrected trajectory
 * is accepted (youth_slam_loop_trajectory gives one); every entry must be
 * finite, which is checked before anything is launched (YOUTH_EINVAL, the map
 * unchanged).  Runs under the module's trajectory lock, as
 * youth_slam_map_render does.  Returns the number of frames whose pose
 * changed, 0 when the map or the store is off, or a negative code.
 *
 * saveSlamMap, with YOUTH_SLAM_LOOP=1 and the store on, writes
 * <map_file>_map.ply first as ever, then re-integrates the kept frames with
 * the corrected trajectory, compacts the map and writes
 * <map_file>_map_closed.ply.  The live trajectory stays untouched: frames
 * recorded later are still integrated with their live poses, and the module's
 * map is the re-integrated one from then on. */
int youth_slam_map_reintegrate(int n, const double* T_wc);
int youth_slam_map_kept(void);                            /* frames in the store */

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_MAP_REMOVE_H */
