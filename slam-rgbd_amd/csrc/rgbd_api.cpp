// rgbd_api.cpp — the C API of the RGB-D context (include/youth_rgbd.h;
// definition: DESIGN.md §13, §16): create and destroy, the pair and sequence
// align, the level schedule, the poses and stats of the last call, the device
// and stage-level entry points.  Host code only: kernels are reached through
// the launch layers of rgbd_align.hip (rgbd_host.h) and icp_kernels.hip
// (icp_host.h).

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rgbd_host.h"

using namespace youth_icp;
using namespace youth_rgbd;

static int rgbd_size_ok(const char* who, int n, int W, int H)
{
    if (n < 0 || n > youth::kMaxFrames || !youth::frame_size_ok(W, H, 3))
        return g_icp_err.set(YOUTH_EINVAL,
                             "%s: %d frames of %dx%d (need 0 <= frames <= 65535, 3 <= W, H <= 16384, "
                             "W*H <= 2^26)",
                             who, n, W, H);
    return YOUTH_OK;
}

namespace youth_rgbd {

int rgbd_ensure_stats(youth_rgbd_ctx* r, int iters)
{
    return grow_device_buffer(g_icp_err, &r->d_stats, &r->stats_iters, iters, (size_t)r->frames * 4);
}

}  // namespace youth_rgbd

// Targets prepped (records by k_prep, words by k_rgbd_prep) into workspace
// frames [0, n_tgt); then the initial poses (dTi: device, or null for the
// identity) and `iters` launches.  Pair p: source frame src0 + p, target
// frame tgt0 + p.
static int rgbd_align_from(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc,
                           const uint8_t* gsrc, const int16_t* dtgt, const uint8_t* gtgt, int n_tgt,
                           int src0, int tgt0, int n_pairs, const double* dTi, int iters,
                           float* d_T_out)
{
    youth_icp_ctx* c = r->icp;
    r->trk_ref = -1;  // the workspace is shared: the streaming tracker starts anew
    int rc = rgbd_ensure_stats(r, iters > 0 ? iters : 1);
    if (rc) return rc;
    rc = launch_prep(c, s, dtgt, n_tgt, 0, false);
    if (rc) return rc;
    rc = rgbd_launch_prep(s, gtgt, 1, n_tgt, c->W, c->H, nullptr, r->d_photo);
    if (rc) return rc;
    rc = launch_init(c, s, dTi, n_pairs, iters, false);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_arrivals, 0, (size_t)c->max_frames * sizeof(unsigned), s));
    for (int it = 0; it < iters; ++it) {
        rc = rgbd_launch_reduce(r, s, dsrc, gsrc, src0, tgt0, n_pairs, it, iters, nullptr);
        if (rc) return rc;
    }
    r->last_pairs = n_pairs;
    r->last_iters = iters;
    r->last_stream = s;
    if (!d_T_out) return YOUTH_OK;
    return export_poses(c, s, n_pairs, d_T_out, false);
}

// The schedule's align: the frames of every coarse level in one decimation
// (set 0: n_src source frames, set 1: n_tgt target frames, or none where the
// targets are the sources' buffer, the sequence), then level after level on
// its workspace, each from the pose the level before it left on the device.
static int rgbd_align_levels(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc,
                             const uint8_t* gsrc, int n_src, const int16_t* dtgt,
                             const uint8_t* gtgt, int n_tgt, int src0, int tgt0, int n_pairs,
                             const double* T_init_host, float* d_T_out)
{
    const bool same = dtgt == dsrc && gtgt == gsrc;
    DecimJob job{};
    job.depth[0] = dsrc, job.gray[0] = gsrc, job.n[0] = n_src;
    job.depth[1] = dtgt, job.gray[1] = gtgt, job.n[1] = same ? 0 : n_tgt;
    const youth_rgbd_ctx::Schedule& S = r->sched;
    for (int l = 0; l < S.n; ++l) {
        const youth_rgbd_ctx::Level& L = S.at[l];
        if (L.lv.stride == 1) continue;
        const int k = job.n_lv++;
        job.stride[k] = L.lv.stride;
        job.dout[0][k] = L.depth, job.gout[0][k] = L.gray;
        job.dout[1][k] = L.depth + L.off, job.gout[1][k] = L.gray + L.off;
    }
    int rc = rgbd_launch_decimate(s, job, r->icp->W, r->icp->H);
    if (rc) return rc;
    const double* dTi = nullptr;
    for (int l = 0; l < S.n; ++l) {
        const youth_rgbd_ctx::Level& L = S.at[l];
        if (L.ctx != r) {
            rc = bind_device(L.ctx->icp);
            if (rc) return rc;
        }
        if (l == 0) {
            rc = upload_T_init(L.ctx->icp, s, T_init_host, n_pairs, &dTi);
            if (rc) return rc;
        }
        const bool full = L.lv.stride == 1;
        const int16_t* ds = full ? dsrc : L.depth;
        const uint8_t* gs = full ? gsrc : L.gray;
        const int16_t* dt = full ? dtgt : same ? ds : L.depth + L.off;
        const uint8_t* gt = full ? gtgt : same ? gs : L.gray + L.off;
        rc = rgbd_align_from(L.ctx, s, ds, gs, dt, gt, n_tgt, src0, tgt0, n_pairs, dTi, L.lv.iters,
                             l == S.n - 1 ? d_T_out : nullptr);
        if (rc) return rc;
        dTi = L.ctx->icp->d_T64;
    }
    r->trk_ref = -1;
    r->last_pairs = n_pairs;
    r->last_stream = s;
    return YOUTH_OK;
}

// The align of the context: its schedule where one is set, else prm.iters
// iterations at full resolution.
static int rgbd_align(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc, const uint8_t* gsrc,
                      int n_src, const int16_t* dtgt, const uint8_t* gtgt, int n_tgt, int src0,
                      int tgt0, int n_pairs, const double* T_init_host, float* d_T_out)
{
    if (r->sched.n > 0)
        return rgbd_align_levels(r, s, dsrc, gsrc, n_src, dtgt, gtgt, n_tgt, src0, tgt0, n_pairs,
                                 T_init_host, d_T_out);
    const double* dTi = nullptr;
    int rc = upload_T_init(r->icp, s, T_init_host, n_pairs, &dTi);
    if (rc) return rc;
    return rgbd_align_from(r, s, dsrc, gsrc, dtgt, gtgt, n_tgt, src0, tgt0, n_pairs, dTi,
                           r->prm.iters, d_T_out);
}

static bool rgbd_stride_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8 || s == 16; }

// ------------------------------------------------------ level schedule --
namespace youth_rgbd {

void rgbd_drop_schedule(youth_rgbd_ctx::Schedule& S, const youth_rgbd_ctx* owner)
{
    for (youth_rgbd_ctx::Level& L : S.at) {
        if (L.ctx && L.ctx != owner) youth_rgbd_destroy(L.ctx);
        if (L.depth) (void)hipFree(L.depth);
        if (L.gray) (void)hipFree(L.gray);
        L = youth_rgbd_ctx::Level{};
    }
    S.n = 0;
}

int rgbd_check_levels(const char* who, const youth_rgbd_ctx* r, const youth_rgbd_level* levels,
                      int n, bool full_last)
{
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (n < 0 || n > YOUTH_RGBD_MAX_LEVELS)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d levels (need 0 .. %d)", who, n,
                             YOUTH_RGBD_MAX_LEVELS);
    if (n > 0 && !levels) return g_icp_err.set(YOUTH_EINVAL, "%s: null levels", who);
    if (r->sub_n > 0)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames pending (collect them first)", who,
                             rgbd_track_pending(r));
    const youth_icp_ctx* c = r->icp;
    for (int l = 0; l < n; ++l) {
        const int s = levels[l].stride;
        if (!rgbd_stride_ok(s))
            return g_icp_err.set(YOUTH_EINVAL, "%s: level %d has stride %d (need 1, 2, 4, 8 or 16)", who,
                                 l, s);
        if (l > 0 && s >= levels[l - 1].stride)
            return g_icp_err.set(YOUTH_EINVAL, "%s: strides %d, %d of levels %d, %d do not decrease",
                                 who, levels[l - 1].stride, s, l - 1, l);
        if (levels[l].iters < 0)
            return g_icp_err.set(YOUTH_EINVAL, "%s: level %d has %d iterations (need >= 0)", who, l,
                                 levels[l].iters);
        if ((c->W + s - 1) / s < 3 || (c->H + s - 1) / s < 3)
            return g_icp_err.set(YOUTH_EINVAL, "%s: level %d of stride %d is %dx%d (need >= 3x3)", who,
                                 l, s, (c->W + s - 1) / s, (c->H + s - 1) / s);
    }
    if (full_last && n > 0 && levels[n - 1].stride != 1)
        return g_icp_err.set(YOUTH_EINVAL,
                             "%s: the last level has stride %d (the tracker's schedule ends at "
                             "stride 1)",
                             who, levels[n - 1].stride);
    return YOUTH_OK;
}

int rgbd_build_schedule(const char* who, youth_rgbd_ctx* r, const youth_rgbd_level* levels, int n,
                        bool frames, youth_rgbd_ctx::Schedule& next)
{
    youth_icp_ctx* c = r->icp;
    for (int l = 0; l < n; ++l) {
        youth_rgbd_ctx::Level& L = next.at[l];
        const int s = levels[l].stride;
        L.lv = levels[l];
        L.ctx = r;
        if (s == 1) continue;  // this context itself, the caller's frames
        const int Ws = (c->W + s - 1) / s, Hs = (c->H + s - 1) / s;
        // fp32 divisions by a power of two: exact
        const youth_intrinsics Ks{c->K.fx / (float)s, c->K.fy / (float)s, c->K.cx / (float)s,
                                  c->K.cy / (float)s, c->K.ds};
        const youth_rgbd_params P{levels[l].iters, r->prm.dist_thresh, r->prm.lambda};
        L.ctx = youth_rgbd_create(c->device, Ws, Hs, r->frames - 1, &Ks, &P);
        if (!L.ctx) {
            rgbd_drop_schedule(next, r);
            return g_icp_err.code();  // youth_rgbd_create's text stands
        }
        if (!frames) continue;
        L.off = ((size_t)r->frames * Ws * Hs + 15) / 16 * 16;
        hipError_t e = hipMalloc(&L.depth, 2 * L.off * sizeof(int16_t));
        if (e == hipSuccess) e = hipMalloc(&L.gray, 2 * L.off);
        if (e != hipSuccess) {
            rgbd_drop_schedule(next, r);
            return g_icp_err.set(e == hipErrorOutOfMemory ? YOUTH_ENOMEM : YOUTH_EHIP,
                                 "%s: hipMalloc: %s", who, hipGetErrorString(e));
        }
    }
    next.n = n;
    return YOUTH_OK;
}

}  // namespace youth_rgbd

extern "C" {

const char* youth_rgbd_last_error(void) { return g_icp_err.c_str(); }

youth_rgbd_params youth_rgbd_default_params(void)
{
    youth_rgbd_params p;
    p.iters = 10;
    p.dist_thresh = 0.10f;
    p.lambda = 0.1f;
    return p;
}

void youth_rgbd_destroy(youth_rgbd_ctx* r)
{
    if (!r) return;
    if (r->icp) (void)hipSetDevice(r->icp->device);
    if (r->icp && r->trk_sched.n > 0) {  // its levels ran on this context's streams
        (void)hipStreamSynchronize(r->icp->stream);
        if (r->icp->xfer) (void)hipStreamSynchronize(r->icp->xfer);
    }
    rgbd_drop_schedule(r->sched, r);
    rgbd_drop_schedule(r->trk_sched, r);
    if (r->icp) {
        (void)hipSetDevice(r->icp->device);
        if (r->last_stream) (void)hipStreamSynchronize(r->last_stream);
        (void)hipStreamSynchronize(r->icp->stream);
        if (r->icp->xfer) (void)hipStreamSynchronize(r->icp->xfer);
    }
    void* bufs[] = {r->d_photo, r->d_gray, r->d_rgb, r->d_part, r->d_stats, r->d_neq, r->d_raw};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (auto& q : r->sub) {
        void* pinned[] = {q.res, q.stage_d, q.stage_c};
        for (void* b : pinned)
            if (b) (void)hipHostFree(b);
        if (q.h2d) (void)hipEventDestroy(q.h2d);
        if (q.done) (void)hipEventDestroy(q.done);
    }
    if (r->pull_stage_d) (void)hipHostFree(r->pull_stage_d);
    if (r->pull_stage_c) (void)hipHostFree(r->pull_stage_c);
    if (r->pull_ev) (void)hipEventDestroy(r->pull_ev);
    youth_icp_destroy(r->icp);
    delete r;
}

youth_rgbd_ctx* youth_rgbd_create(int device, int W, int H, int max_frames,
                                  const youth_intrinsics* K, const youth_rgbd_params* params)
{
    const youth_rgbd_params prm = params ? *params : youth_rgbd_default_params();
    if (prm.iters < 0 || !std::isfinite(prm.dist_thresh) || !(prm.dist_thresh > 0.0f) ||
        !std::isfinite(prm.lambda) || prm.lambda < 0.0f) {
        g_icp_err.set(YOUTH_EINVAL,
                      "youth_rgbd_create: bad parameters: iters %d, dist_thresh %g, lambda %g (need "
                      "iters >= 0, dist_thresh > 0 and lambda >= 0, both finite)",
                      prm.iters, (double)prm.dist_thresh, (double)prm.lambda);
        return nullptr;
    }
    if (!youth::frame_size_ok(W, H, 3) || max_frames < 2 || max_frames > youth::kMaxFrames) {
        g_icp_err.set(YOUTH_EINVAL,
                      "youth_rgbd_create: bad size %dx%d / max_frames %d (need 3 <= W, H <= 16384, "
                      "W*H <= 2^26, 2 <= max_frames <= 65535)",
                      W, H, max_frames);
        return nullptr;
    }
    const youth_icp_params ip{prm.iters, prm.dist_thresh};
    // one frame more than pairs: a sequence of max_frames pairs stages
    // max_frames + 1 host frames
    youth_icp_ctx* c = youth_icp_create(device, W, H, max_frames + 1, K, &ip);
    if (!c) return nullptr;  // youth_icp_create's text stands
    auto* r = new youth_rgbd_ctx();
    r->icp = c;
    r->prm = prm;
    r->frames = max_frames + 1;
    r->pk.w = prm.lambda / 255.0f;
    r->pk.kx = (0.5f * r->pk.w) * c->K.fx;
    r->pk.ky = (0.5f * r->pk.w) * c->K.fy;
    const char* ck = getenv("YOUTH_RGBD_CHUNKS");  // test knob
    if (ck && atoi(ck) > 0) r->chunks = atoi(ck);
    const char* pw = getenv("YOUTH_RGBD_PULL_WG");  // tuning knob (tools/rgbd_track_bench.py)
    if (pw && atoi(pw) > 0) r->pull_wg = std::min(atoi(pw), 1024);
    const size_t N = (size_t)c->N, F = (size_t)r->frames;
    hipError_t e;
    if ((e = hipMalloc(&r->d_photo, F * N * sizeof(unsigned))) != hipSuccess ||
        (e = hipMalloc(&r->d_gray, F * N)) != hipSuccess ||
        (e = hipMalloc(&r->d_neq, kRgbdNeq * sizeof(double))) != hipSuccess) {
        g_icp_err.set(e == hipErrorOutOfMemory ? YOUTH_ENOMEM : YOUTH_EHIP,
                      "youth_rgbd_create: hipMalloc: %s", hipGetErrorString(e));
        youth_rgbd_destroy(r);
        return nullptr;
    }
    if (rgbd_ensure_stats(r, prm.iters > 0 ? prm.iters : 1) != YOUTH_OK) {
        youth_rgbd_destroy(r);
        return nullptr;
    }
    return r;
}

int youth_rgbd_luma_device(int device, const uint8_t* d_rgb, uint8_t* d_gray, int n, int W, int H,
                           void* stream)
{
    static const char* who = "youth_rgbd_luma_device";
    if (!d_rgb || !d_gray) return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    int rc = rgbd_size_ok(who, n, W, H);
    if (rc) return rc;
    rc = youth::check_device(g_icp_err, who, device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return rgbd_launch_prep((hipStream_t)stream, d_rgb, 3, n, W, H, d_gray, nullptr);
}

int youth_rgbd_prep_device(youth_rgbd_ctx* r, const uint8_t* d_in, int channels, int n,
                           uint8_t* d_gray, uint32_t* d_photo, void* stream)
{
    static const char* who = "youth_rgbd_prep_device";
    if (!r || !d_in || (channels != 1 && channels != 3) || n < 0 || n > youth::kMaxFrames)
        return g_icp_err.set(YOUTH_EINVAL, "%s: bad arguments (channels %d, %d frames)", who, channels,
                             n);
    int rc = bind_device(r->icp);
    if (rc) return rc;
    return rgbd_launch_prep(pick_stream(r->icp, stream), d_in, channels, n, r->icp->W, r->icp->H,
                            d_gray, d_photo);
}

int youth_rgbd_align_pairs_device(youth_rgbd_ctx* r, const int16_t* d_src_depth,
                                  const uint8_t* d_src_gray, const int16_t* d_dst_depth,
                                  const uint8_t* d_dst_gray, int n_pairs, const double* T_init,
                                  float* d_T_out, void* stream)
{
    static const char* who = "youth_rgbd_align_pairs_device";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (!d_src_depth || !d_src_gray || !d_dst_depth || !d_dst_gray)
        return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (n_pairs <= 0 || n_pairs > r->frames - 1)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d pairs (need 1 .. max_frames = %d)", who, n_pairs,
                             r->frames - 1);
    int rc = bind_device(r->icp);
    if (rc) return rc;
    return rgbd_align(r, pick_stream(r->icp, stream), d_src_depth, d_src_gray, n_pairs, d_dst_depth,
                      d_dst_gray, n_pairs, 0, 0, n_pairs, T_init, d_T_out);
}

int youth_rgbd_align_sequence_device(youth_rgbd_ctx* r, const int16_t* d_depth,
                                     const uint8_t* d_gray, int n_frames, float* d_T_out,
                                     void* stream)
{
    static const char* who = "youth_rgbd_align_sequence_device";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (!d_depth || !d_gray) return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (n_frames < 2 || n_frames > r->frames)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames (need 2 .. max_frames + 1 = %d)", who,
                             n_frames, r->frames);
    int rc = bind_device(r->icp);
    if (rc) return rc;
    // every frame but the last is a target, prepped once; pair k: source frame
    // k + 1, target frame k
    return rgbd_align(r, pick_stream(r->icp, stream), d_depth, d_gray, n_frames, d_depth, d_gray,
                      n_frames - 1, 1, 0, n_frames - 1, nullptr, d_T_out);
}

int youth_rgbd_sync(youth_rgbd_ctx* r, void* stream)
{
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_sync: null context");
    int rc = bind_device(r->icp);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(pick_stream(r->icp, stream)));
    return YOUTH_OK;
}

// youth_rgbd_get_poses on one workspace (a context without a schedule, or a level's)
static int rgbd_get_poses_of(youth_rgbd_ctx* r, int n, double* T64, float* T32, int32_t* status)
{
    if (!r || n < 0 || n > r->frames - 1)
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_get_poses: bad arguments (%d poses)", n);
    youth_icp_ctx* c = r->icp;
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = r->last_stream ? r->last_stream : c->stream;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(s));
        return YOUTH_OK;
    }
    if (T64)
        HIP_TRY(hipMemcpyAsync(T64, c->d_T64, (size_t)n * 16 * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    if (T32) {
        rc = export_poses(c, s, n, c->d_Tout, false);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(T32, c->d_Tout, (size_t)n * 16 * sizeof(float),
                               hipMemcpyDeviceToHost, s));
    }
    if (status)
        HIP_TRY(hipMemcpyAsync(status, c->d_status, (size_t)n * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

static int rgbd_get_stats_of(youth_rgbd_ctx* r, int n, int iters, double* stats)
{
    if (!r || !stats || n < 0 || n > r->last_pairs || iters != r->last_iters || iters < 1 ||
        iters > r->stats_iters)
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_get_stats: bad arguments (%d pairs, %d iterations)",
                             n, iters);
    int rc = bind_device(r->icp);
    if (rc) return rc;
    hipStream_t s = r->last_stream ? r->last_stream : r->icp->stream;
    if (n > 0)
        HIP_TRY(hipMemcpyAsync(stats, r->d_stats, (size_t)n * iters * 4 * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

int youth_rgbd_get_poses(youth_rgbd_ctx* r, int n, double* T64, float* T32, int32_t* status)
{
    if (!r || r->sched.n == 0) return rgbd_get_poses_of(r, n, T64, T32, status);
    // the last level's poses; the status words of all levels ORed
    int rc = rgbd_get_poses_of(r->sched.at[r->sched.n - 1].ctx, n, T64, T32, status);
    if (rc || !status || n == 0) return rc;
    std::vector<int32_t> st((size_t)n);
    for (int l = 0; l < r->sched.n - 1; ++l) {
        rc = rgbd_get_poses_of(r->sched.at[l].ctx, n, nullptr, nullptr, st.data());
        if (rc) return rc;
        for (int p = 0; p < n; ++p) status[p] |= st[p];
    }
    return YOUTH_OK;
}

int youth_rgbd_get_stats(youth_rgbd_ctx* r, int n, int iters, double* stats)
{
    if (!r || r->sched.n == 0) return rgbd_get_stats_of(r, n, iters, stats);
    return rgbd_get_stats_of(r->sched.at[r->sched.n - 1].ctx, n, iters, stats);
}

int youth_rgbd_default_levels(int W, int H, youth_rgbd_level out[YOUTH_RGBD_MAX_LEVELS])
{
    if (!out) return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_default_levels: null output");
    int n = 0;
    for (int s = 8; s >= 2; s /= 2)
        if (W / s >= 80 && H / s >= 60) {
            out[n++] = youth_rgbd_level{s, 10};
            break;
        }
    out[n++] = youth_rgbd_level{1, 10};
    return n;
}

int youth_rgbd_set_levels(youth_rgbd_ctx* r, const youth_rgbd_level* levels, int n)
{
    static const char* who = "youth_rgbd_set_levels";
    int rc = rgbd_check_levels(who, r, levels, n, false);
    if (rc) return rc;
    rc = bind_device(r->icp);
    if (rc) return rc;
    // the new schedule beside the old one, which stays if anything fails
    youth_rgbd_ctx::Schedule next;
    rc = rgbd_build_schedule(who, r, levels, n, true, next);
    if (rc) return rc;
    // nothing of the old schedule is in flight once its streams are idle
    if (r->last_stream) HIP_TRY(hipStreamSynchronize(r->last_stream));
    rgbd_drop_schedule(r->sched, r);
    r->sched = next;
    return YOUTH_OK;
}

int youth_rgbd_get_levels(const youth_rgbd_ctx* r, youth_rgbd_level* out, int cap)
{
    if (!r || cap < 0 || (cap > 0 && !out))
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_get_levels: bad arguments");
    for (int l = 0; l < std::min(cap, r->sched.n); ++l) out[l] = r->sched.at[l].lv;
    return r->sched.n;
}

int youth_rgbd_get_level_poses(youth_rgbd_ctx* r, int level, int n, double* T64, int32_t* status)
{
    if (!r || level < 0 || level >= r->sched.n)
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_get_level_poses: level %d of %d", level,
                             r ? r->sched.n : 0);
    return rgbd_get_poses_of(r->sched.at[level].ctx, n, T64, nullptr, status);
}

int youth_rgbd_get_level_stats(youth_rgbd_ctx* r, int level, int n, int iters, double* stats)
{
    if (!r || level < 0 || level >= r->sched.n)
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_get_level_stats: level %d of %d", level,
                             r ? r->sched.n : 0);
    return rgbd_get_stats_of(r->sched.at[level].ctx, n, iters, stats);
}

int youth_rgbd_decimate_device(int device, const int16_t* d_depth, const uint8_t* d_gray, int n, int W,
                               int H, int stride, int16_t* d_depth_out, uint8_t* d_gray_out,
                               void* stream)
{
    static const char* who = "youth_rgbd_decimate_device";
    if (!d_depth || !d_gray || !d_depth_out || !d_gray_out)
        return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (stride == 1 || !rgbd_stride_ok(stride))
        return g_icp_err.set(YOUTH_EINVAL, "%s: stride %d (need 2, 4, 8 or 16)", who, stride);
    int rc = rgbd_size_ok(who, n, W, H);
    if (rc) return rc;
    rc = youth::check_device(g_icp_err, who, device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    DecimJob job{};
    job.depth[0] = d_depth, job.gray[0] = d_gray, job.n[0] = n;
    job.n_lv = 1;
    job.stride[0] = stride;
    job.dout[0][0] = d_depth_out, job.gout[0][0] = d_gray_out;
    return rgbd_launch_decimate((hipStream_t)stream, job, W, H);
}

int youth_rgbd_reduce_host(youth_rgbd_ctx* r, const int16_t* src_depth, const uint8_t* src_gray,
                           const int16_t* dst_depth, const uint8_t* dst_gray, const float* T12,
                           double* neq31)
{
    static const char* who = "youth_rgbd_reduce_host";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (!src_depth || !src_gray || !dst_depth || !dst_gray || !T12 || !neq31)
        return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T12[i])) return g_icp_err.set(YOUTH_EINVAL, "%s: non-finite pose", who);
    youth_icp_ctx* c = r->icp;
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t N = c->N;
    r->trk_ref = -1;  // the workspace is shared: the streaming tracker starts anew
    // frame 0 the source, frame 1 the target
    HIP_TRY(hipMemcpyAsync(c->d_depth, src_depth, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_depth + N, dst_depth, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r->d_gray, src_gray, N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r->d_gray + N, dst_gray, N, hipMemcpyHostToDevice, s));
    rc = launch_prep(c, s, c->d_depth + N, 1, 1, false);
    if (rc) return rc;
    rc = rgbd_launch_prep(s, r->d_gray + N, 1, 1, c->W, c->H, nullptr, r->d_photo + N);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_T32, T12, 12 * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->d_arrivals, 0, sizeof(unsigned), s));
    rc = rgbd_launch_reduce(r, s, c->d_depth, r->d_gray, 0, 1, 1, 0, r->prm.iters, r->d_neq);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(neq31, r->d_neq, kRgbdNeq * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

}  // extern "C"
