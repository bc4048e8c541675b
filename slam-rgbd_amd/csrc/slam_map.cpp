// slam_map.cpp — the SLAM module's voxel map (include/youth_map.h, "the
// drop-in"): the glue between the worker of slam_api.cpp and a youth_map.
//
// Its own translation unit so that slam_api.cpp needs no symbol of the map:
// the hook table below is registered from a static initialiser, and a build
// without this file (the host-only sanitizer drivers) runs with the table
// null.  Host code against the HIP headers (no kernel): the frame store
// below holds device memory.
//
// The frame store (YOUTH_SLAM_MAP_KEEP=<n>): every integrated frame's depth,
// colour and fp32 pose stay on the device, in recording order, so that the
// frames can be moved to a corrected trajectory (youth_slam_map_reintegrate,
// youth_map_move_device).  It grows by chunks of 64 frames, each a set of
// hip_host.h's device buffers allocated once; a kept frame is integrated from
// its place in the store, which is bit for bit what youth_map_integrate_host
// does with its staging copy.
//
// Threads: the worker integrates and clears (slam_api.cpp calls both under its
// trajectory lock, so a reset cannot fall between a pose's recording and its
// frame's integration); API threads start / stop the module, save, query and
// render (youth_slam_map_render holds the trajectory lock too).
// Everything here runs under g_map_mu, always taken after the trajectory lock
// where both are held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "hip_host.h"
#include "slam_map_hooks.h"
#include "youth_map.h"

namespace {

std::mutex g_map_mu;
youth_map* g_map = nullptr;   // null: the map is off
float g_map_vpm = 0.0f;
int g_map_device = 0;

// ---- the frame store (under g_map_mu) ----
constexpr int kChunk = 64;    // frames per chunk
struct Chunk {
    int16_t* depth = nullptr;   // [kChunk][h][w]
    uint8_t* rgb = nullptr;     // [kChunk][h][w][3], null without colour
    float* T = nullptr;         // [kChunk][12] the poses the frames are in the map with
    float* T_new = nullptr;     // [kChunk][12] the poses of a move
    size_t depth_cap = 0, rgb_cap = 0, T_cap = 0, T_new_cap = 0;
};
youth::ErrorText g_keep_err;
int g_keep_max = 0;             // YOUTH_SLAM_MAP_KEEP; 0: off
int g_kept = 0;                 // frames in the store
long long g_not_kept = 0;       // integrated but not kept
bool g_keep_failed = false;     // an allocation failed: nothing further is kept
int g_keep_w = 0, g_keep_h = 0;
bool g_keep_rgb = false;
youth_intrinsics g_keep_K;
std::vector<Chunk> g_chunks;
std::vector<float> g_keep_T;    // host mirror of the stored poses, [kept][12]

void keep_free()
{
    if (!g_chunks.empty() && hipSetDevice(g_map_device) == hipSuccess) {
        for (Chunk& c : g_chunks) {
            (void)hipFree(c.depth);
            (void)hipFree(c.rgb);
            (void)hipFree(c.T);
            (void)hipFree(c.T_new);
        }
    }
    g_chunks.clear();
    g_keep_T.clear();
    g_kept = 0;
    g_not_kept = 0;
    g_keep_failed = false;
    g_keep_w = g_keep_h = 0;
}

// resetSlam / a new sequence: the store is emptied, its chunks stay for reuse
void keep_forget()
{
    g_keep_T.clear();
    g_kept = 0;
    g_not_kept = 0;
}

void keep_skip(const char* why)
{
    if (g_not_kept++ == 0)
        fprintf(stderr, "youth_icp: map frames are integrated but no longer kept: %s\n", why);
}

// fp64 4x4 -> the fp32 3x4 of youth_map_integrate_host; false: not finite
bool pose32(const double* T_world, float* T32)
{
    for (int q = 0; q < 12; ++q) {
        T32[q] = (float)T_world[q];
        if (!std::isfinite(T_world[q]) || !std::isfinite(T32[q])) return false;
    }
    return true;
}

// The frame into the store's next place and from there into the map.  false:
// not kept (the caller integrates it the plain way).
bool keep_and_integrate(const int16_t* depth, const uint8_t* rgb, int w, int h,
                        const youth_intrinsics* K, const double* T_world)
{
    if (g_keep_max <= 0) return false;
    float T32[12];
    // a frame without a finite pose is refused by the plain way too
    if (!T_world || !K || !pose32(T_world, T32)) return false;
    if (g_keep_failed) {
        keep_skip("a device allocation failed");
        return false;
    }
    if (g_kept >= g_keep_max) {
        keep_skip("YOUTH_SLAM_MAP_KEEP frames are stored");
        return false;
    }
    const bool same_shape = w == g_keep_w && h == g_keep_h && (rgb != nullptr) == g_keep_rgb;
    if (g_kept == 0) {
        // the first frame of a sequence sets the store's shape; chunks of
        // another shape are of no use to it
        if (!same_shape) keep_free();
        g_keep_w = w;
        g_keep_h = h;
        g_keep_rgb = rgb != nullptr;
        g_keep_K = *K;
    } else if (!same_shape || memcmp(K, &g_keep_K, sizeof(*K)) != 0) {
        keep_skip("the frame's size, colour or intrinsics differ from the first frame's");
        return false;
    }
    if (hipSetDevice(g_map_device) != hipSuccess) return false;
    const size_t N = (size_t)w * h;
    const int ci = g_kept / kChunk, at = g_kept % kChunk;
    if (ci == (int)g_chunks.size()) {
        Chunk c;
        if (youth::grow_device_buffer(g_keep_err, &c.depth, &c.depth_cap, (size_t)kChunk * N) < 0 ||
            (rgb && youth::grow_device_buffer(g_keep_err, &c.rgb, &c.rgb_cap, (size_t)kChunk * N, 3) < 0) ||
            youth::grow_device_buffer(g_keep_err, &c.T, &c.T_cap, (size_t)kChunk, 12) < 0 ||
            youth::grow_device_buffer(g_keep_err, &c.T_new, &c.T_new_cap, (size_t)kChunk, 12) < 0) {
            (void)hipGetLastError();
            (void)hipFree(c.depth);
            (void)hipFree(c.rgb);
            (void)hipFree(c.T);
            (void)hipFree(c.T_new);
            g_keep_failed = true;
            keep_skip("a device allocation failed");
            return false;
        }
        g_chunks.push_back(c);
    }
    Chunk& c = g_chunks[ci];
    int16_t* d_depth = c.depth + (size_t)at * N;
    uint8_t* d_rgb = rgb ? c.rgb + (size_t)at * N * 3 : nullptr;
    float* d_T = c.T + (size_t)at * 12;
    // synchronous copies: the frame's buffers are free again on return
    if (hipMemcpy(d_depth, depth, N * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
        (rgb && hipMemcpy(d_rgb, rgb, N * 3, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(d_T, T32, sizeof(T32), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        keep_skip("a copy to the device failed");
        return false;
    }
    if (youth_map_integrate_device(g_map, d_depth, d_rgb, 1, w, h, K, d_T, nullptr) < 0 ||
        youth_map_sync(g_map, nullptr) < 0) {
        fprintf(stderr, "youth_icp: map integration failed: %s\n", youth_map_last_error());
        return true;   // not in the map, not in the store
    }
    g_keep_T.insert(g_keep_T.end(), T32, T32 + 12);
    ++g_kept;
    return true;
}

// under g_map_mu: kept frames i < n from their stored poses to T_wc[i]
int reintegrate_locked(int n, const double* T_wc)
{
    if (!g_map || g_keep_max <= 0) return 0;
    if (n < 0 || (n > 0 && !T_wc)) return YOUTH_EINVAL;
    // all of T_wc is checked before anything is launched
    std::vector<float> T_new((size_t)n * 12);
    for (int i = 0; i < n; ++i)
        if (!pose32(T_wc + (size_t)i * 16, T_new.data() + (size_t)i * 12)) {
            fprintf(stderr, "youth_icp: map not re-integrated: pose %d is not finite\n", i);
            return YOUTH_EINVAL;
        }
    const int m = n < g_kept ? n : g_kept;
    if (hipSetDevice(g_map_device) != hipSuccess) return YOUTH_EHIP;
    int changed = 0;
    for (int c0 = 0; c0 < m; c0 += kChunk) {
        const int nf = m - c0 < kChunk ? m - c0 : kChunk;
        const float* to = T_new.data() + (size_t)c0 * 12;
        float* from = g_keep_T.data() + (size_t)c0 * 12;
        int ch = 0;
        for (int i = 0; i < nf; ++i) ch += memcmp(to + i * 12, from + i * 12, 12 * sizeof(float)) != 0;
        if (!ch) continue;
        Chunk& c = g_chunks[c0 / kChunk];
        const size_t bytes = (size_t)nf * 12 * sizeof(float);
        if (hipMemcpy(c.T_new, to, bytes, hipMemcpyHostToDevice) != hipSuccess) return YOUTH_EHIP;
        int rc = youth_map_move_device(g_map, c.depth, g_keep_rgb ? c.rgb : nullptr, nf, g_keep_w,
                                       g_keep_h, &g_keep_K, c.T, c.T_new, nullptr);
        if (rc == YOUTH_OK) rc = youth_map_sync(g_map, nullptr);
        if (rc < 0) {
            fprintf(stderr, "youth_icp: map re-integration failed: %s\n", youth_map_last_error());
            return rc;
        }
        // the frames are now in the map with the new poses
        if (hipMemcpy(c.T, to, bytes, hipMemcpyHostToDevice) != hipSuccess) return YOUTH_EHIP;
        memcpy(from, to, bytes);
        changed += ch;
    }
    return changed;
}

void map_start(int device)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    keep_free();
    g_keep_max = 0;
    if (g_map) youth_map_destroy(g_map);
    g_map = nullptr;
    g_map_vpm = 0.0f;
    g_map_device = device;
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
    if (const char* ek = getenv("YOUTH_SLAM_MAP_KEEP")) g_keep_max = atoi(ek) > 0 ? atoi(ek) : 0;
    if (g_keep_max > 0)
        fprintf(stderr, "youth_icp: voxel map keeps up to %d frames for re-integration\n", g_keep_max);
}

void map_stop(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    keep_free();
    g_keep_max = 0;
    if (g_map) youth_map_destroy(g_map);
    g_map = nullptr;
    g_map_vpm = 0.0f;
}

void map_integrate(const int16_t* depth, const uint8_t* rgb, int w, int h, const youth_intrinsics* K,
                   const double* T_world)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    if (!g_map) return;
    if (keep_and_integrate(depth, rgb, w, h, K, T_world)) return;
    // synchronous: the frame's buffers are free again when this returns; rgb
    // (YOUTH_SLAM_MAP_COLOR / YOUTH_SLAM_RGBD) gives the voxels their colour
    if (youth_map_integrate_host(g_map, depth, rgb, w, h, K, T_world) < 0)
        fprintf(stderr, "youth_icp: map integration failed: %s\n", youth_map_last_error());
}

void map_clear(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    keep_forget();
    if (g_map && youth_map_clear(g_map) < 0)
        fprintf(stderr, "youth_icp: map clear failed: %s\n", youth_map_last_error());
}

// under g_map_mu: the map's records
bool records_locked(std::vector<youth_voxel>& vox)
{
    const long long n = youth_map_voxels(g_map);
    if (n < 0) return false;
    vox.resize((size_t)n);
    const int got = youth_map_extract(g_map, vox.data(), (int)n);
    if (got < 0) return false;
    vox.resize((size_t)got);   // fewer than the slots once something was removed
    return true;
}

int map_save(const char* base)
{
    std::vector<youth_voxel> vox;
    float vpm;
    {
        std::lock_guard<std::mutex> lk(g_map_mu);
        if (!g_map) return 1;
        vpm = g_map_vpm;
        if (!records_locked(vox)) return 0;
    }
    const std::string path = std::string(base) + "_map.ply";
    return youth_map_write_ply(path.c_str(), vox.data(), (int)vox.size(), vpm) == YOUTH_OK;
}

int map_reintegrate(int n, const double* T_wc)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    return reintegrate_locked(n, T_wc);
}

int map_save_closed(const char* base, int n, const double* T_wc)
{
    std::vector<youth_voxel> vox;
    float vpm;
    {
        std::lock_guard<std::mutex> lk(g_map_mu);
        if (!g_map || g_keep_max <= 0) return 1;
        vpm = g_map_vpm;
        if (reintegrate_locked(n, T_wc) < 0) return 0;
        if (youth_map_compact(g_map) < 0) {
            fprintf(stderr, "youth_icp: map not compacted: %s\n", youth_map_last_error());
            return 0;
        }
        if (!records_locked(vox)) return 0;
    }
    const std::string path = std::string(base) + "_map_closed.ply";
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

const youth_slam_map_hooks g_hooks = {map_start, map_stop,   map_integrate,   map_clear,
                                      map_save,  map_render, map_reintegrate, map_save_closed};

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

int youth_slam_map_kept(void)
{
    std::lock_guard<std::mutex> lk(g_map_mu);
    return g_map ? g_kept : 0;
}

}  // extern "C"
