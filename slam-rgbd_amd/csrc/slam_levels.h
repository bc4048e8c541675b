// The drop-in's reading of a level schedule from an environment variable
// (YOUTH_SLAM_LOOP_LEVELS in slam_loop.cpp, YOUTH_SLAM_RGBD_LEVELS in
// slam_rgbd.cpp).  Host-only, header-only.
#ifndef YOUTH_SLAM_LEVELS_H
#define YOUTH_SLAM_LEVELS_H

#include <stdio.h>
#include <string.h>

#include "youth_rgbd.h"

// A parsed value: n = -1 `auto` (the default schedule of the frame size), 0
// none, else the list.
struct youth_slam_levels {
    int n = 0;
    youth_rgbd_level at[YOUTH_RGBD_MAX_LEVELS] = {};

    // the schedule for W x H frames into lv; returns its number of levels
    int resolve(int w, int h, youth_rgbd_level lv[YOUTH_RGBD_MAX_LEVELS]) const
    {
        if (n < 0) return youth_rgbd_default_levels(w, h, lv);
        memcpy(lv, at, sizeof(at));
        return n;
    }
};

// "auto" or "s:n,s:n,..." (1 .. YOUTH_RGBD_MAX_LEVELS items of two non-negative
// integers) -> out; false: malformed, out untouched.  The schedule's own rules
// are the library's (youth_loop_set_levels, youth_rgbd_track_set_levels).
inline bool youth_slam_parse_levels(const char* text, youth_slam_levels* out)
{
    if (strcmp(text, "auto") == 0) {
        out->n = -1;
        return true;
    }
    youth_rgbd_level lv[YOUTH_RGBD_MAX_LEVELS] = {};
    int n = 0;
    const char* p = text;
    for (;;) {
        int s = 0, it = 0, used = 0;
        if (n == YOUTH_RGBD_MAX_LEVELS || sscanf(p, "%9d:%9d%n", &s, &it, &used) != 2 || s < 0 || it < 0)
            return false;
        for (int k = 0; k < used; ++k)
            if (!strchr("0123456789:", p[k])) return false;
        lv[n++] = youth_rgbd_level{s, it};
        p += used;
        if (*p == '\0') break;
        if (*p++ != ',') return false;
    }
    memcpy(out->at, lv, sizeof(lv));
    out->n = n;
    return true;
}

#endif  // YOUTH_SLAM_LEVELS_H
