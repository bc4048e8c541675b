// The SLAM module's door to the voxel map (include/youth_map.h).  slam_api.cpp
// knows the map only through this table, which slam_map.cpp registers from a
// static initialiser: a build of slam_api.cpp without that unit (the host-only
// sanitizer drivers) links as before and finds the table null.
#ifndef YOUTH_SLAM_MAP_HOOKS_H
#define YOUTH_SLAM_MAP_HOOKS_H

#include <stdint.h>

#include "youth_icp.h"

struct youth_map_view;   // youth_map_render.h

struct youth_slam_map_hooks {
    // initSlamModule: read YOUTH_SLAM_MAP_* and create the map (or leave it off)
    void (*start)(int device);
    // stopSlamModule, after the worker has been joined
    void (*stop)(void);
    // a recorded frame and its camera -> world pose (fp64 4x4); returns when
    // the frame's buffers have been read; rgb: the frame's colour (uint8
    // [h][w][3]), null when colour is not carried
    void (*integrate)(const int16_t* depth, const uint8_t* rgb, int w, int h,
                      const youth_intrinsics* K, const double* T_world);
    // resetSlam / a new sequence's origin
    void (*clear)(void);
    // saveSlamMap: <base>_map.ply; 1 written or map off, 0 failed
    int (*save)(const char* base);
    // youth_slam_map_render, called under the trajectory lock with the pose
    // resolved: 1 rendered, 0 map off or failed (outputs untouched)
    int (*render)(const struct youth_map_view* view, const youth_intrinsics* K,
                  const double* T_world, int16_t* depth, uint8_t* rgb);
    // The two below stand last and may be null (a table aggregate-initialised
    // without them, as the sanitizer drivers' is): null means off.
    // youth_slam_map_reintegrate, called under the trajectory lock: the kept
    // frames i < n moved to T_wc[i] (fp64 4x4 each); the number of frames whose
    // pose changed, 0 when the map or its frame store is off, or a negative code
    int (*reintegrate)(int n, const double* T_wc);
    // saveSlamMap with loop closing on, after save and under the trajectory
    // lock: re-integrate with the corrected trajectory, compact, write
    // <base>_map_closed.ply; 1 written or nothing to do (store off), 0 failed
    int (*save_closed)(const char* base, int n, const double* T_wc);
};

extern "C" void youth_slam_set_map_hooks(const youth_slam_map_hooks* hooks);

#endif  // YOUTH_SLAM_MAP_HOOKS_H
