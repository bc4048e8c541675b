// slam_map.cpp — the SLAM module's voxel map (include/youth_map.h, "the
// drop-in"): the glue between the worker of slam_api.cpp and a youth_map.
//
// Its own translation unit so that slam_api.cpp needs no symbol of the map:
// the hook table below is registered from a static initialiser, and a build
// without this file (the host-only sanitizer drivers) runs with the table
// null.  Host-only C++: no HIP types.
//
// Threads: the worker integrates and clears (slam_api.cpp calls both under its
// trajectory lock, so a reset cannot fall between a pose's recording and its
// frame's integration); API threads start / stop the module, save, query and
// render (youth_slam_map_render holds the trajectory lock too).
// Everything here runs under g_map_mu, always taken after the trajectory lock
// where both are held.
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "slam_map_hooks.h"
#include "youth_map.h"

namespace {

std::mutex g_map_mu;
youth_map* g_map = nullptr;   // null: the map is off
float g_map_vpm = 0.0f;

void map_start(int device)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (g_map) youth_map_destroy(g_map);
    g_map = nullptr;
    g_map_vpm = 0.0f;
    const char* ev = getenv("YOUTH_SLAM_MAP_VPM");
    if (!ev || !*ev) return;
    const float vpm = strtof(ev, nullptr);
    long long slots = 1LL << 22;
    if (const char* es = getenv("YOUTH_SLAM_MAP_SLOTS")) slots = atoll(es);
    g_map = youth_map_create(device, vpm, slots);
    if (!g_map) {
        fprintf(stderr, "youth_icp: map not started: %s\n", youth_map_last_error());
        return;
    }
    if (const char* ed = getenv("YOUTH_SLAM_MAP_MAX_DEPTH")) {
        if (youth_map_set_max_depth(g_map, atoi(ed)) < 0)
            fprintf(stderr, "youth_icp: YOUTH_SLAM_MAP_MAX_DEPTH ignored: %s\n", youth_map_last_error());
    }
    g_map_vpm = vpm;
    fprintf(stderr, "youth_icp: voxel map on (%g voxels per metre)\n", (double)vpm);
}

void map_stop(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (g_map) youth_map_destroy(g_map);
    g_map = nullptr;
    g_map_vpm = 0.0f;
}

void map_integrate(const int16_t* depth, const uint8_t* rgb, int w, int h, const youth_intrinsics* K,
                   const double* T_world)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (!g_map) return;
    // synchronous: the frame's buffers are free again when this returns; rgb
    // (YOUTH_SLAM_MAP_COLOR / YOUTH_SLAM_RGBD) gives the voxels their colour
    if (youth_map_integrate_host(g_map, depth, rgb, w, h, K, T_world) < 0)
        fprintf(stderr, "youth_icp: map integration failed: %s\n", youth_map_last_error());
}

void map_clear(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (g_map && youth_map_clear(g_map) < 0)
        fprintf(stderr, "youth_icp: map clear failed: %s\n", youth_map_last_error());
}

int map_save(const char* base)
{
    std::vector<youth_voxel> vox;
    float vpm;
    {
        std::lock_guard<std::mutex> lk(g_map_mu);
        if (!g_map) return 1;
        vpm = g_map_vpm;
        const long long n = youth_map_voxels(g_map);
        if (n < 0) return 0;
        vox.resize((size_t)n);
        if (youth_map_extract(g_map, vox.data(), (int)n) != (int)n) return 0;
    }
    const std::string path = std::string(base) + "_map.ply";
    return youth_map_write_ply(path.c_str(), vox.data(), (int)vox.size(), vpm) == YOUTH_OK;
}

int map_render(const struct youth_map_view* view, const youth_intrinsics* K, const double* T_world,
               int16_t* depth, uint8_t* rgb)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (!g_map) return 0;
    if (youth_map_render_host(g_map, view, K, T_world, depth, rgb) < 0) {
        fprintf(stderr, "youth_icp: map render failed: %s\n", youth_map_last_error());
        return 0;
    }
    return 1;
}

const youth_slam_map_hooks g_hooks = {map_start, map_stop, map_integrate,
                                      map_clear, map_save, map_render};

struct Registrar {
    Registrar() { youth_slam_set_map_hooks(&g_hooks); }
} g_registrar;

}  // namespace

extern "C" {

long long youth_slam_map_voxels(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (!g_map) return 0;
    const long long n = youth_map_voxels(g_map);
    return n < 0 ? 0 : n;
}

int youth_slam_map_extract(youth_voxel* out, int cap)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (!g_map) return 0;
    return youth_map_extract(g_map, out, cap);
}

float youth_slam_map_vpm(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    return g_map_vpm;
}

}  // extern "C"
