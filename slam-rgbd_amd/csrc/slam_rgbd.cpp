// slam_rgbd.cpp — the SLAM module's RGB-D tracking (YOUTH_SLAM_RGBD=1): the
// glue between the RGB-D worker of slam_api.cpp and the streaming tracker of
// include/youth_rgbd.h.
//
// Its own translation unit so that slam_api.cpp needs no symbol of the
// tracker: the hook table below is registered from a static initialiser, and a
// build without this file (the host-only sanitizer drivers) runs with the table
// null.  Host-only C++: no HIP types.  The worker thread alone creates, feeds
// and destroys a tracker; start() runs in initSlamModule before the worker
// exists.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include "slam_levels.h"
#include "slam_rgbd_hooks.h"
#include "youth_rgbd.h"

namespace {

youth_rgbd_params g_prm;
bool g_flt_on = false;
youth_filter_params g_flt{8, 96};
youth_slam_levels g_levels;    // YOUTH_SLAM_RGBD_LEVELS (slam_levels.h)

void rgbd_start(void)
{
    g_prm = youth_rgbd_default_params();
    if (const char* e = getenv("YOUTH_SLAM_RGBD_LAMBDA")) {
        char* end = nullptr;
        const float lam = strtof(e, &end);
        if (end != e && std::isfinite(lam) && lam >= 0.0f)
            g_prm.lambda = lam;
        else
            fprintf(stderr, "youth_icp: YOUTH_SLAM_RGBD_LAMBDA=%s ignored (want a finite value >= 0)\n", e);
    }
    // youth_icp_create's reading of the variable, for this tracker
    g_flt_on = false;
    g_flt = youth_filter_params{8, 96};
    const char* df = getenv("YOUTH_ICP_DEPTH_FILTER");
    if (df && *df && strcmp(df, "0") != 0) {
        youth_filter_params fp{8, 96};
        char tail = 0;
        if (strcmp(df, "1") == 0 || (sscanf(df, "%d,%d%c", &fp.t0, &fp.t2, &tail) == 2 && fp.t0 >= 1 &&
                                     fp.t0 <= 255 && fp.t2 >= 0 && fp.t2 <= 1000)) {
            g_flt = fp;
            g_flt_on = true;
        }  // else youth_icp_create has said that it is ignored
    }
    g_levels = youth_slam_levels{};
    if (const char* e = getenv("YOUTH_SLAM_RGBD_LEVELS"))
        if (*e && !youth_slam_parse_levels(e, &g_levels))
            fprintf(stderr, "youth_icp: YOUTH_SLAM_RGBD_LEVELS=%s is not `auto` or a list like 8:10,1:10; "
                            "ignored\n", e);
}

void* rgbd_create(int device, int w, int h, int batch, const youth_intrinsics* K)
{
    youth_rgbd_ctx* r = youth_rgbd_create(device, w, h, 2 * batch, K, &g_prm);
    if (!r) return nullptr;
    if (youth_rgbd_track_set_batch(r, batch) < 0 ||
        (g_flt_on && youth_rgbd_track_set_depth_filter(r, &g_flt) < 0)) {
        youth_rgbd_destroy(r);  // the refusal's text stands
        return nullptr;
    }
    if (g_levels.n != 0) {
        youth_rgbd_level lv[YOUTH_RGBD_MAX_LEVELS] = {};
        const int n = g_levels.resolve(w, h, lv);
        if (youth_rgbd_track_set_levels(r, lv, n) < 0) {
            fprintf(stderr, "youth_icp: YOUTH_SLAM_RGBD_LEVELS=%s ignored: %s\n",
                    getenv("YOUTH_SLAM_RGBD_LEVELS") ? getenv("YOUTH_SLAM_RGBD_LEVELS") : "",
                    youth_rgbd_last_error());
            g_levels.n = 0;  // logged once
        }
    }
    return r;
}

void rgbd_destroy(void* t) { youth_rgbd_destroy(static_cast<youth_rgbd_ctx*>(t)); }

int rgbd_submit(void* t, const int16_t* const* depth, const uint8_t* const* rgb, int n)
{
    return youth_rgbd_track_submit(static_cast<youth_rgbd_ctx*>(t), depth, rgb, n);
}

int rgbd_collect(void* t, double* T_rel, int* has_ref)
{
    return youth_rgbd_track_collect(static_cast<youth_rgbd_ctx*>(t), T_rel, has_ref);
}

int rgbd_reset(void* t) { return youth_rgbd_track_reset(static_cast<youth_rgbd_ctx*>(t)); }

const youth_slam_rgbd_hooks g_hooks = {rgbd_start,   rgbd_create, rgbd_destroy,        rgbd_submit,
                                       rgbd_collect, rgbd_reset,  youth_rgbd_last_error};

struct Registrar {
    Registrar() { youth_slam_set_rgbd_hooks(&g_hooks); }
} g_registrar;

}  // namespace
