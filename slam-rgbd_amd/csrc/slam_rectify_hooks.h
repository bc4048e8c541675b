// The SLAM module's door to the lens rectifier (include/youth_rectify.h, "the
// drop-in").  slam_api.cpp knows it only through this table, which
// slam_rectify.cpp registers from a static initialiser, as slam_map.cpp does
// for the map: a build of slam_api.cpp without that unit (the host-only
// sanitizer drivers) links as before and finds the table null.
#ifndef YOUTH_SLAM_RECTIFY_HOOKS_H
#define YOUTH_SLAM_RECTIFY_HOOKS_H

#include <stdint.h>

#include "youth_icp.h"

struct youth_slam_rectify_hooks {
    // initSlamModule: read YOUTH_SLAM_RECTIFY and the YAML's coefficients (or
    // leave rectification off); config_file may be null, W / H 0 = any size
    void (*start)(int device, const char* config_file, const youth_intrinsics* K, int W, int H);
    // stopSlamModule, after the worker has been joined
    void (*stop)(void);
    // the worker, just before a submit: n frames of w x h, rectified in place
    // (rgb[i] may be null: that frame carries no colour).  0: done, or not
    // this module's business (off, or not the YAML's size); < 0: failed, the
    // text is last_error()
    int (*frames)(int16_t* const* depth, uint8_t* const* rgb, int n, int w, int h);
    const char* (*last_error)(void);
};

extern "C" void youth_slam_set_rectify_hooks(const youth_slam_rectify_hooks* hooks);

#endif  // YOUTH_SLAM_RECTIFY_HOOKS_H
