// The SLAM module's door to the streaming RGB-D tracker (include/youth_rgbd.h,
// youth_rgbd_track_*).  slam_api.cpp knows the tracker only through this table,
// which slam_rgbd.cpp registers from a static initialiser, as slam_map.cpp does
// for the map: a build of slam_api.cpp without that unit (the host-only
// sanitizer drivers) links as before, finds the table null and refuses
// YOUTH_SLAM_RGBD.
#ifndef YOUTH_SLAM_RGBD_HOOKS_H
#define YOUTH_SLAM_RGBD_HOOKS_H

#include <stdint.h>

#include "youth_icp.h"

struct youth_slam_rgbd_hooks {
    // initSlamModule: read YOUTH_SLAM_RGBD_LAMBDA, YOUTH_ICP_DEPTH_FILTER and YOUTH_SLAM_RGBD_LEVELS
    void (*start)(void);
    // a tracker for W x H frames, `batch` frames per submission at most, two
    // submissions in flight; null on failure (last_error says why)
    void* (*create)(int device, int w, int h, int batch, const youth_intrinsics* K);
    void (*destroy)(void* trk);
    // youth_rgbd_track_submit / _collect / _reset on the tracker
    int (*submit)(void* trk, const int16_t* const* depth, const uint8_t* const* rgb, int n);
    int (*collect)(void* trk, double* T_rel, int* has_ref);
    int (*reset)(void* trk);
    const char* (*last_error)(void);
};

extern "C" void youth_slam_set_rgbd_hooks(const youth_slam_rgbd_hooks* hooks);

#endif  // YOUTH_SLAM_RGBD_HOOKS_H
