// slam_loop.cpp — the SLAM module's loop closer (include/youth_loop.h, "the
// drop-in"): the glue between the worker of slam_api.cpp and a youth_loop.
//
// Its own translation unit, registered through a hook table from a static
// initialiser, as slam_map.cpp is.  Host-only C++: no HIP types.
//
// The worker hands over every recorded frame under its trajectory lock.  This
// unit keeps its own copy of the recorded poses, picks keyframes by motion,
// stores them in the youth_loop and closes each as it is added.  The live
// trajectory is never touched: the corrected one is computed on demand from
// the copy (odometry edges between consecutive keyframes, the verified loop
// edges, youth_posegraph_optimize, youth_posegraph_interpolate).
//
// Everything here runs under g_loop_mu, always taken after the trajectory lock
// where both are held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "slam_levels.h"
#include "slam_loop_hooks.h"
#include "youth_loop.h"

namespace {

std::mutex g_loop_mu;
bool g_on = false;             // YOUTH_SLAM_LOOP=1 and nothing has switched it off
int g_device = 0;
double g_kf_m = 0.10, g_kf_deg = 10.0;
int g_min_gap = 0;             // 0: the default of youth_loop_default_params
youth_slam_levels g_levels;    // YOUTH_SLAM_LOOP_LEVELS (slam_levels.h)
youth_loop* g_lp = nullptr;    // made with the first frame, for its size
int g_w = 0, g_h = 0;
bool g_full = false;           // the store is full: no further keyframes
std::vector<uint32_t> g_ts;    // every recorded frame
std::vector<double> g_T;       // [frames][16]
std::vector<int32_t> g_kf;     // the keyframes' frame indices

void drop_object()
{
    if (g_lp) youth_loop_destroy(g_lp);
    g_lp = nullptr;
    g_w = g_h = 0;
}

void forget()
{
    g_ts.clear();
    g_T.clear();
    g_kf.clear();
    g_full = false;
    if (g_lp) youth_loop_clear(g_lp);
}

void loop_start(int device)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    drop_object();
    forget();
    const char* ev = getenv("YOUTH_SLAM_LOOP");
    g_on = ev && *ev && strcmp(ev, "0") != 0;
    if (!g_on) return;
    g_device = device;
    g_kf_m = 0.10;
    g_kf_deg = 10.0;
    g_min_gap = 0;
    if (const char* e = getenv("YOUTH_SLAM_LOOP_KF_M")) g_kf_m = atof(e);
    if (const char* e = getenv("YOUTH_SLAM_LOOP_KF_DEG")) g_kf_deg = atof(e);
    if (const char* e = getenv("YOUTH_SLAM_LOOP_MIN_GAP")) g_min_gap = atoi(e);
    g_levels = youth_slam_levels{};
    if (const char* e = getenv("YOUTH_SLAM_LOOP_LEVELS"))
        if (*e && !youth_slam_parse_levels(e, &g_levels))
            fprintf(stderr, "youth_icp: YOUTH_SLAM_LOOP_LEVELS=%s is not `auto` or a list like 8:10,1:10; "
                            "ignored\n", e);
    fprintf(stderr, "youth_icp: loop closing on (a keyframe every %g m / %g deg)\n", g_kf_m, g_kf_deg);
}

void loop_stop(void)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    drop_object();
    forget();
    g_on = false;
}

void loop_clear(void)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    forget();
}

// rotation angle (degrees) and translation norm of A^-1 B
void motion(const double* A, const double* B, double* deg, double* m)
{
    // R = R_A^T R_B, t = R_A^T (t_B - t_A)
    double R[9], d[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]}, t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            R[r * 3 + c] = A[r] * B[c] + A[4 + r] * B[4 + c] + A[8 + r] * B[8 + c];
        t[r] = A[r] * d[0] + A[4 + r] * d[1] + A[8 + r] * d[2];
    }
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
    *deg = atan2(sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (R[0] + R[4] + R[8] - 1.0)) * (180.0 / M_PI);
    *m = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
}

void loop_frame(const int16_t* depth, const uint8_t* rgb, int w, int h, const youth_intrinsics* K,
                const double* T_world, uint32_t ts)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    if (!g_on) return;
    if (!rgb) {
        fprintf(stderr, "youth_icp: loop closing needs colour frames (YOUTH_SLAM_RGBD=1 or "
                        "YOUTH_SLAM_MAP_COLOR=1); it stays off\n");
        g_on = false;
        return;
    }
    if (g_lp && (w != g_w || h != g_h)) drop_object();   // a new frame size: its sequence started anew
    if (!g_lp) {
        youth_loop_params P = youth_loop_default_params();
        if (g_min_gap > 0) P.min_gap = g_min_gap;
        g_lp = youth_loop_create(g_device, w, h, YOUTH_LOOP_MAX_KEYFRAMES, K, &P);
        if (!g_lp) {
            fprintf(stderr, "youth_icp: loop closing not started: %s\n", youth_loop_last_error());
            g_on = false;
            return;
        }
        g_w = w;
        g_h = h;
        if (g_levels.n != 0) {
            youth_rgbd_level lv[YOUTH_RGBD_MAX_LEVELS] = {};
            const int n = g_levels.resolve(w, h, lv);
            if (youth_loop_set_levels(g_lp, lv, n) < 0) {
                fprintf(stderr, "youth_icp: YOUTH_SLAM_LOOP_LEVELS ignored: %s\n", youth_loop_last_error());
                g_levels.n = 0;   // logged once
            }
        }
    }
    const int f = (int)g_ts.size();
    g_ts.push_back(ts);
    g_T.insert(g_T.end(), T_world, T_world + 16);
    bool is_kf = g_kf.empty();
    if (!is_kf) {
        double deg, m;
        motion(g_T.data() + (size_t)g_kf.back() * 16, T_world, &deg, &m);
        is_kf = m > g_kf_m || deg > g_kf_deg;
    }
    if (!is_kf || g_full) return;
    if (youth_loop_keyframes(g_lp) >= YOUTH_LOOP_MAX_KEYFRAMES) {
        fprintf(stderr, "youth_icp: loop closing: %d keyframes stored, no further ones\n",
                YOUTH_LOOP_MAX_KEYFRAMES);
        g_full = true;
        return;
    }
    const int idx = youth_loop_add_keyframe_host(g_lp, depth, rgb, T_world, (uint32_t)f);
    if (idx < 0) {
        fprintf(stderr, "youth_icp: keyframe not stored: %s\n", youth_loop_last_error());
        return;
    }
    g_kf.push_back(f);
    const int added = youth_loop_close(g_lp, idx);
    if (added < 0)
        fprintf(stderr, "youth_icp: loop closing failed: %s\n", youth_loop_last_error());
    else if (added > 0)
        fprintf(stderr, "youth_icp: keyframe %d (frame %d) closes %d loop%s\n", idx, f, added,
                added == 1 ? "" : "s");
}

// under g_loop_mu: the keyframe poses optimised (X_new) beside the recorded ones (X_old)
bool optimise(std::vector<double>& X_old, std::vector<double>& X_new)
{
    const int n = (int)g_kf.size();
    X_old.resize((size_t)n * 16);
    for (int k = 0; k < n; ++k)
        memcpy(X_old.data() + (size_t)k * 16, g_T.data() + (size_t)g_kf[k] * 16, 16 * sizeof(double));
    X_new = X_old;
    if (n < 2) return true;
    std::vector<youth_loop_edge> edges((size_t)(n - 1));
    for (int k = 1; k < n; ++k) {   // odometry: Z = X_{k-1}^-1 X_k
        youth_loop_edge& e = edges[k - 1];
        memset(&e, 0, sizeof(e));
        e.i = k - 1;
        e.j = k;
        e.w = 1.0;
        const double* A = X_old.data() + (size_t)(k - 1) * 16;
        const double* B = X_old.data() + (size_t)k * 16;
        const double d[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                e.Z[r * 4 + c] = A[r] * B[c] + A[4 + r] * B[4 + c] + A[8 + r] * B[8 + c];
            e.Z[r * 4 + 3] = A[r] * d[0] + A[4 + r] * d[1] + A[8 + r] * d[2];
        }
        e.Z[15] = 1.0;
    }
    const int n_loop = youth_loop_edges(g_lp, nullptr, 0);
    if (n_loop > 0) {
        edges.resize((size_t)(n - 1 + n_loop));
        youth_loop_edges(g_lp, edges.data() + (n - 1), n_loop);
    }
    if (youth_posegraph_optimize(n, X_new.data(), (int)edges.size(), edges.data(), nullptr, nullptr,
                                 nullptr) < 0) {
        fprintf(stderr, "youth_icp: pose graph not optimised: %s\n", youth_posegraph_last_error());
        X_new = X_old;
        return false;
    }
    return true;
}

// under g_loop_mu: the corrected trajectory into T (a copy of g_T re-hung)
bool corrected_locked(std::vector<double>& X_new, std::vector<double>& T)
{
    std::vector<double> X_old;
    T = g_T;
    if (g_kf.empty()) {
        X_new.clear();
        return true;
    }
    if (!optimise(X_old, X_new)) return false;
    return youth_posegraph_interpolate((int)g_ts.size(), T.data(), (int)g_kf.size(), g_kf.data(),
                                       X_old.data(), X_new.data()) == YOUTH_OK;
}

bool loop_corrected(std::vector<uint32_t>& kf_ts, std::vector<double>& kf_T, std::vector<uint32_t>& ts,
                    std::vector<double>& T)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    if (!g_on) return false;
    corrected_locked(kf_T, T);   // on failure: the recorded poses
    ts = g_ts;
    kf_ts.clear();
    for (int32_t f : g_kf) kf_ts.push_back(g_ts[f]);
    return true;
}

const youth_slam_loop_hooks g_hooks = {loop_start, loop_stop, loop_frame, loop_clear, loop_corrected};

struct Registrar {
    Registrar() { youth_slam_set_loop_hooks(&g_hooks); }
} g_registrar;

}  // namespace

extern "C" {

int youth_slam_loop_keyframes(void)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    return g_on ? (int)g_kf.size() : 0;
}

int youth_slam_loop_edges(youth_loop_edge* out, int cap)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    if (!g_on || !g_lp) return 0;
    return youth_loop_edges(g_lp, out, cap);
}

int youth_slam_loop_keyframe_frames(int32_t* frame_index, int cap)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    if (!g_on || !frame_index || cap <= 0) return 0;
    const int m = cap < (int)g_kf.size() ? cap : (int)g_kf.size();
    memcpy(frame_index, g_kf.data(), (size_t)m * sizeof(int32_t));
    return m;
}

int youth_slam_loop_trajectory(int n, double* T_wc)
{
    std::lock_guard<std::mutex> lk(g_loop_mu);
    if (!g_on || !T_wc || n <= 0) return 0;
    std::vector<double> X_new, T;
    corrected_locked(X_new, T);
    const int m = n < (int)g_ts.size() ? n : (int)g_ts.size();
    memcpy(T_wc, T.data(), (size_t)m * 16 * sizeof(double));
    return m;
}

}  // extern "C"
