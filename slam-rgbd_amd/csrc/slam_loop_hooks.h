// The SLAM module's door to the loop closer (include/youth_loop.h, "the
// drop-in").  slam_api.cpp knows it only through this table, which
// slam_loop.cpp registers from a static initialiser, as slam_map.cpp does for
// the map: a build of slam_api.cpp without that unit (the host-only sanitizer
// drivers) links as before and finds the table null.
#ifndef YOUTH_SLAM_LOOP_HOOKS_H
#define YOUTH_SLAM_LOOP_HOOKS_H

#include <stdint.h>

#include <vector>

#include "youth_icp.h"

struct youth_slam_loop_hooks {
    // initSlamModule: read YOUTH_SLAM_LOOP* (or leave loop closing off)
    void (*start)(int device);
    // stopSlamModule, after the worker has been joined
    void (*stop)(void);
    // a recorded frame, its camera -> world pose (fp64 4x4) and its timestamp:
    // the arguments of the map's integrate plus the timestamp; returns when
    // the frame's buffers have been read
    void (*frame)(const int16_t* depth, const uint8_t* rgb, int w, int h, const youth_intrinsics* K,
                  const double* T_world, uint32_t ts);
    // resetSlam / a new sequence's origin
    void (*clear)(void);
    // saveSlamMap: false when loop closing is off (the outputs untouched);
    // else the optimised keyframes and the corrected trajectory, timestamps
    // and 16 fp64 values per pose
    bool (*corrected)(std::vector<uint32_t>& kf_ts, std::vector<double>& kf_T,
                      std::vector<uint32_t>& ts, std::vector<double>& T);
};

extern "C" void youth_slam_set_loop_hooks(const youth_slam_loop_hooks* hooks);

#endif  // YOUTH_SLAM_LOOP_HOOKS_H
