// The SLAM module's lens rectification (include/youth_rectify.h, "the
// drop-in"): with YOUTH_SLAM_RECTIFY=1 and a YAML whose
// distortion coefficients are not all zero, the worker's frames of the YAML's
// size are rectified in place (Ko = K) just before they are submitted, so the
// tracker, a realign, the map and the loop closer all see the same
// ideal-pinhole frame.  Also the YAML's distortion keys
// (youth_parse_camera_yaml_distortion), which youth_parse_camera_yaml leaves
// unread.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>

#include "slam_rectify_hooks.h"
#include "youth_rectify.h"

extern "C" int youth_parse_camera_yaml_distortion(const char* path, youth_distortion* D)
{
    if (!path || !D) return 0;
    FILE* f = fopen(path, "r");
    if (!f) return 0;
    youth_distortion d = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        char* p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == '#' || *p == '\0' || *p == '\n') continue;
        char* colon = strchr(p, ':');
        if (!colon) continue;
        std::string key(p, colon - p);
        while (!key.empty() && (key.back() == ' ' || key.back() == '\t')) key.pop_back();
        char* end = nullptr;
        const double val = strtod(colon + 1, &end);
        if (end == colon + 1) continue;  // not a number
        if (key == "Camera.k1") d.k1 = (float)val;
        else if (key == "Camera.k2") d.k2 = (float)val;
        else if (key == "Camera.p1") d.p1 = (float)val;
        else if (key == "Camera.p2") d.p2 = (float)val;
        else if (key == "Camera.k3") d.k3 = (float)val;
    }
    fclose(f);
    *D = d;
    return 1;
}

namespace {

std::mutex g_mu;  // start / stop against the worker's frames
std::atomic<bool> g_on{false};
int g_device = 0;
youth_intrinsics g_K;
youth_distortion g_D;
int g_cfg_W = 0, g_cfg_H = 0;
youth_rectify* g_rect = nullptr;  // made by the worker at the first frame of the YAML's size
int g_rect_W = 0, g_rect_H = 0;
thread_local std::string g_text;

void drop_object()
{
    if (g_rect) youth_rectify_destroy(g_rect);
    g_rect = nullptr;
    g_rect_W = g_rect_H = 0;
}

void rectify_start(int device, const char* config_file, const youth_intrinsics* K, int W, int H)
{
    std::lock_guard<std::mutex> lk(g_mu);
    drop_object();
    g_on.store(false);
    youth_distortion D;
    if (!config_file || !K || !youth_parse_camera_yaml_distortion(config_file, &D)) return;
    if (D.k1 == 0.0f && D.k2 == 0.0f && D.p1 == 0.0f && D.p2 == 0.0f && D.k3 == 0.0f) return;
    const char* ev = getenv("YOUTH_SLAM_RECTIFY");
    if (!(ev && *ev && strcmp(ev, "0") != 0)) {
        fprintf(stderr, "youth_icp: %s has lens distortion (k1 %g k2 %g p1 %g p2 %g k3 %g), which is ignored: "
                        "set YOUTH_SLAM_RECTIFY=1 to rectify frames before tracking\n",
                config_file, (double)D.k1, (double)D.k2, (double)D.p1, (double)D.p2, (double)D.k3);
        return;
    }
    g_device = device;
    g_K = *K;
    g_D = D;
    g_cfg_W = W;
    g_cfg_H = H;
    g_on.store(true);
    fprintf(stderr, "youth_icp: lens rectification on (k1 %g k2 %g p1 %g p2 %g k3 %g)\n", (double)D.k1,
            (double)D.k2, (double)D.p1, (double)D.p2, (double)D.k3);
}

void rectify_stop(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    drop_object();
    g_on.store(false);
}

int rectify_frames(int16_t* const* depth, uint8_t* const* rgb, int n, int w, int h)
{
    if (!g_on.load()) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_on.load()) return 0;
    if ((g_cfg_W != 0 && g_cfg_W != w) || (g_cfg_H != 0 && g_cfg_H != h)) return 0;
    if (!g_rect || g_rect_W != w || g_rect_H != h) {
        drop_object();
        const int rc = youth_rectify_create(g_device, w, h, &g_K, &g_D, nullptr, &g_rect);
        if (rc) {
            g_text = youth_rectify_last_error();
            return rc;
        }
        g_rect_W = w;
        g_rect_H = h;
    }
    int with = 0;
    for (int i = 0; i < n; ++i) with += rgb && rgb[i] != nullptr;
    int rc = 0;
    if (with == 0 || with == n) {
        rc = youth_rectify_host_frames(g_rect, depth, with ? rgb : nullptr, n);
    } else {
        // some frames of the batch came without colour: one by one
        for (int i = 0; i < n && rc == 0; ++i)
            rc = youth_rectify_host_frames(g_rect, depth + i, rgb[i] ? rgb + i : nullptr, 1);
    }
    if (rc) g_text = youth_rectify_last_error();
    return rc;
}

const char* rectify_last_error(void) { return g_text.c_str(); }

const youth_slam_rectify_hooks g_hooks = {rectify_start, rectify_stop, rectify_frames, rectify_last_error};

struct Registrar {
    Registrar() { youth_slam_set_rectify_hooks(&g_hooks); }
} g_registrar;

}  // namespace

extern "C" int youth_slam_rectify_active(void) { return g_on.load() ? 1 : 0; }
