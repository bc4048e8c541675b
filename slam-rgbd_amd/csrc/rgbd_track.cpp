// rgbd_track.cpp — the streaming RGB-D tracker (include/youth_rgbd.h,
// youth_rgbd_track_*): host frames submitted in
// submissions of up to trk_b, each frame aligned to the one before it, results
// collected in order; the staging of pageable frames; youth_rgbd_pull_host and
// youth_rgbd_track_host_sequence.  Host code only: kernels are reached through
// the launch layers of rgbd_align.hip (rgbd_host.h) and icp_kernels.hip
// (icp_host.h).

#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "rgbd_host.h"

using namespace youth_icp;
using namespace youth_rgbd;

extern "C" int youth_rgbd_track_host_sequence(youth_rgbd_ctx* r, const int16_t* depth,
                                              const uint8_t* rgb, int n_frames, double* T_rel,
                                              int32_t* status)
{
    static const char* who = "youth_rgbd_track_host_sequence";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (!depth || !rgb || !T_rel) return g_icp_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (n_frames < 2 || n_frames > r->frames)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames (need 2 .. max_frames + 1 = %d)", who,
                             n_frames, r->frames);
    youth_icp_ctx* c = r->icp;
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t N = c->N;
    if (!r->d_rgb) HIP_TRY(hipMalloc(&r->d_rgb, (size_t)r->frames * N * 3));
    HIP_TRY(hipMemcpyAsync(c->d_depth, depth, (size_t)n_frames * N * sizeof(int16_t),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(r->d_rgb, rgb, (size_t)n_frames * N * 3, hipMemcpyHostToDevice, s));
    rc = rgbd_launch_prep(s, r->d_rgb, 3, n_frames, c->W, c->H, r->d_gray, nullptr);
    if (rc) return rc;
    rc = youth_rgbd_align_sequence_device(r, c->d_depth, r->d_gray, n_frames, nullptr, s);
    if (rc) return rc;
    rc = youth_rgbd_get_poses(r, n_frames - 1, T_rel, nullptr, status);
    if (rc) return rc;
    return n_frames - 1;
}

// ==================================================== streaming tracker ==
// youth_rgbd_track_* (DESIGN.md §14).  One submission of m <= trk_b frames:
//
//   transfer stream  wait for the last reader of the bank; k_rgbd_pull of the
//                    m frames into the bank's depth (or the filter's raw
//                    staging) and intensity slots; the depth filter; event
//   context stream   wait for that event; the reference's record and word
//                    copied into slot 0; k_prep and k_rgbd_prep<1> of the m
//                    new frames into slots 1 .. m; k_init; prm.iters launches
//                    of k_rgbd_reduce over the pairs (frame i against frame
//                    i - 1, the first against slot 0) on the geometry of
//                    trk_b pairs; poses and statuses to the submission's
//                    pinned result slot; event
//
// With the tracker's own level schedule (trk_sched) the
// transfer stream also decimates the bank's (filtered) frames into every
// coarse level's bank, one k_rgbd_decimate launch, and the context stream runs
// its part level by level, coarse to fine, each level on its own workspace at
// the same bank and slot indices, from the poses the level before it left on
// the device; every level's poses and statuses go to the result slot.
//
// Every frame is prepped once, as a new frame; what a pair computes depends on
// its two frames, on trk_b and on the schedule, not on the submission it
// travelled in.
// k_rgbd_reduce holds no wait (its last arriver sums, handoff_publish /
// handoff_sum), so no status here carries YOUTH_STATUS_TIMEOUT.

// Page-locked staging for m frames (grown while nothing reads it).
static int rgbd_ensure_stage(youth_rgbd_ctx* r, int16_t** d, uint8_t** c, int* cap, int m)
{
    if (*cap >= m) return YOUTH_OK;
    const size_t N = (size_t)r->icp->N;
    if (*d) (void)hipHostFree(*d);
    if (*c) (void)hipHostFree(*c);
    *d = nullptr;
    *c = nullptr;
    *cap = 0;
    HIP_TRY(hipHostMalloc((void**)d, (size_t)m * N * sizeof(int16_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)c, (size_t)m * N * 3, hipHostMallocDefault));
    *cap = m;
    return YOUTH_OK;
}

// Whether every frame lies in page-locked memory the GPU may read in place.
static bool rgbd_frames_pinned(const youth_rgbd_ctx* r, const int16_t* const* depth,
                               const uint8_t* const* rgb, int m)
{
    const size_t N = (size_t)r->icp->N;
    for (int i = 0; i < m; ++i)
        if (!host_alloc_covers_bytes(depth[i], N * sizeof(int16_t)) ||
            !host_alloc_covers_bytes(rgb[i], N * 3))
            return false;
    return true;
}

// The frames k_rgbd_pull reads: the caller's where page-locked, else copies in
// the staging (streaming stores: the GPU reads them next, host_copy.h).
static void rgbd_stage_frames(const youth_rgbd_ctx* r, const int16_t* const* depth,
                              const uint8_t* const* rgb, int m, int16_t* stage_d, uint8_t* stage_c,
                              const int16_t** d_out, const uint8_t** c_out)
{
    const size_t N = (size_t)r->icp->N;
    for (int i = 0; i < m; ++i) {
        d_out[i] = depth[i];
        c_out[i] = rgb[i];
        if (!stage_d) continue;
        if (!host_alloc_covers_bytes(depth[i], N * sizeof(int16_t))) {
            youth::stream_copy(stage_d + (size_t)i * N, depth[i], N * sizeof(int16_t));
            d_out[i] = stage_d + (size_t)i * N;
        }
        if (!host_alloc_covers_bytes(rgb[i], N * 3)) {
            youth::stream_copy(stage_c + (size_t)i * N * 3, rgb[i], N * 3);
            c_out[i] = stage_c + (size_t)i * N * 3;
        }
    }
}

static int rgbd_check_frames(const char* who, const int16_t* const* depth,
                             const uint8_t* const* rgb, int m, int max_m)
{
    if (!depth || !rgb) return g_icp_err.set(YOUTH_EINVAL, "%s: null frame array", who);
    if (m < 1 || m > max_m)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames (need 1 .. %d)", who, m, max_m);
    for (int i = 0; i < m; ++i)
        if (!depth[i] || !rgb[i])
            return g_icp_err.set(YOUTH_EINVAL, "%s: frame %d has a null %s pointer", who, i,
                                 depth[i] ? "colour" : "depth");
    return YOUTH_OK;
}

int youth_rgbd::rgbd_track_pending(const youth_rgbd_ctx* r)
{
    int n = 0;
    for (int k = 0; k < r->sub_n; ++k) {
        const auto& q = r->sub[(r->sub_head + k) % 2];
        n += q.m - q.next;
    }
    return n;
}

// Lazily: the transfer stream, the two submissions' events and result slots.
static int rgbd_ensure_track(youth_rgbd_ctx* r)
{
    youth_icp_ctx* c = r->icp;
    if (!c->xfer) HIP_TRY(hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking));
    for (auto& q : r->sub) {
        if (!q.h2d) HIP_TRY(hipEventCreateWithFlags(&q.h2d, hipEventDisableTiming));
        if (!q.done) HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
        const int n_lv = std::max(1, r->trk_sched.n);
        if (q.res_cap < r->trk_b || q.res_lv < n_lv) {
            if (q.res) (void)hipHostFree(q.res);
            q.res = nullptr;
            q.res_cap = q.res_lv = 0;
            HIP_TRY(hipHostMalloc((void**)&q.res, (size_t)n_lv * r->trk_b * 17 * sizeof(double),
                                  hipHostMallocDefault));
            q.res_cap = r->trk_b;
            q.res_lv = n_lv;
        }
    }
    return YOUTH_OK;
}

// One level's share of a submission on the context stream: Lr the level's
// workspace (the context itself at stride 1), whose banks hold the m new
// frames; dTi the level's initial poses on the device (null: the identity).
static int rgbd_track_level(youth_rgbd_ctx* r, youth_rgbd_ctx* Lr, hipStream_t s, int m, int iters,
                            const double* dTi)
{
    youth_icp_ctx* c = Lr->icp;
    const size_t N = (size_t)c->N;
    const int d0 = r->trk_bank * r->trk_b;  // first depth / intensity slot of the bank
    const int ref = r->trk_ref;
    if (ref > 0) {
        HIP_TRY(hipMemcpyAsync(c->d_rec, c->d_rec + (size_t)ref * c->P, c->P * sizeof(float4),
                               hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(Lr->d_photo, Lr->d_photo + (size_t)ref * N, N * sizeof(unsigned),
                               hipMemcpyDeviceToDevice, s));
    }
    int rc = launch_prep(c, s, c->d_depth + (size_t)d0 * N, m, 1, false);
    if (rc) return rc;
    rc = rgbd_launch_prep(s, Lr->d_gray + (size_t)d0 * N, 1, m, c->W, c->H, nullptr, Lr->d_photo + N);
    if (rc) return rc;
    // without a reference the first frame is prepped only
    const int pairs = ref >= 0 ? m : m - 1;
    if (pairs > 0) {
        rc = rgbd_ensure_stats(Lr, iters > 0 ? iters : 1);
        if (rc) return rc;
        rc = launch_init(c, s, dTi, pairs, iters, false);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->d_arrivals, 0, (size_t)pairs * sizeof(unsigned), s));
        // pair p: source slot src0 + p of the bank, target record slot tgt0 + p
        const int src0 = ref >= 0 ? d0 : d0 + 1, tgt0 = ref >= 0 ? 0 : 1;
        for (int it = 0; it < iters; ++it) {
            rc = rgbd_launch_reduce(Lr, s, c->d_depth, Lr->d_gray, src0, tgt0, pairs, it, iters,
                                    nullptr, r->trk_b);
            if (rc) return rc;
        }
        Lr->last_pairs = pairs;
        Lr->last_iters = iters;
    }
    Lr->last_stream = s;
    return YOUTH_OK;
}

static int rgbd_track_enqueue(youth_rgbd_ctx* r, youth_rgbd_ctx::Sub& q,
                              const int16_t* const* depth, const uint8_t* const* rgb, int m)
{
    youth_icp_ctx* c = r->icp;
    hipStream_t s = c->stream, xs = c->xfer;
    const size_t N = (size_t)c->N;
    const int d0 = r->trk_bank * r->trk_b;  // first depth / intensity slot of the bank
    int16_t* const dbank = c->d_depth + (size_t)d0 * N;
    uint8_t* const gbank = r->d_gray + (size_t)d0 * N;
    const youth_rgbd_ctx::Schedule& S = r->trk_sched;
    // the bank's last reader is the submission that used this entry before
    if (q.m > 0) HIP_TRY(hipStreamWaitEvent(xs, q.done, 0));
    int rc = rgbd_launch_pull(r, xs, depth, rgb, m, r->flt_on ? r->d_raw : dbank, gbank, nullptr);
    if (rc) return rc;
    if (r->flt_on) {
        rc = youth_depth_filter_device(c->device, r->d_raw, dbank, m, c->W, c->H, &r->flt, xs);
        if (rc) return g_icp_err.set(rc, "depth filter: %s", youth_depth_filter_last_error());
    }
    // every coarse level's frames in one decimation of the bank's (filtered)
    // frames, into the same slots of the level's own banks
    DecimJob job{};
    job.depth[0] = dbank, job.gray[0] = gbank, job.n[0] = m;
    for (int l = 0; l < S.n; ++l) {
        const youth_rgbd_ctx::Level& L = S.at[l];
        if (L.ctx == r) continue;
        const size_t Ns = (size_t)L.ctx->icp->N;
        const int k = job.n_lv++;
        job.stride[k] = L.lv.stride;
        job.dout[0][k] = L.ctx->icp->d_depth + (size_t)d0 * Ns;
        job.gout[0][k] = L.ctx->d_gray + (size_t)d0 * Ns;
    }
    rc = rgbd_launch_decimate(xs, job, c->W, c->H);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(q.h2d, xs));
    HIP_TRY(hipStreamWaitEvent(s, q.h2d, 0));
    const int pairs = r->trk_ref >= 0 ? m : m - 1;
    const int n_lv = std::max(1, S.n);
    int32_t* const res_st = reinterpret_cast<int32_t*>(q.res + (size_t)q.res_lv * q.res_cap * 16);
    const double* dTi = nullptr;
    for (int l = 0; l < n_lv; ++l) {
        youth_rgbd_ctx* Lr = S.n > 0 ? S.at[l].ctx : r;
        const int iters = S.n > 0 ? S.at[l].lv.iters : r->prm.iters;
        rc = rgbd_track_level(r, Lr, s, m, iters, dTi);
        if (rc) return rc;
        youth_icp_ctx* lc = Lr->icp;
        dTi = lc->d_T64;
        if (pairs <= 0) continue;
        // every level's poses and status words to the pinned result slot
        HIP_TRY(hipMemcpyAsync(q.res + (size_t)l * q.res_cap * 16, lc->d_T64,
                               (size_t)pairs * 16 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(res_st + (size_t)l * q.res_cap, lc->d_status,
                               (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    r->last_stream = s;
    HIP_TRY(hipEventRecord(q.done, s));
    return YOUTH_OK;
}

extern "C" {

int youth_rgbd_track_set_batch(youth_rgbd_ctx* r, int b)
{
    static const char* who = "youth_rgbd_track_set_batch";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (b < 1 || b > YOUTH_TRACK_MAX_BATCH)
        return g_icp_err.set(YOUTH_EINVAL, "%s: batch %d (need 1 .. %d)", who, b,
                             YOUTH_TRACK_MAX_BATCH);
    if (2 * b > r->frames - 1)
        return g_icp_err.set(YOUTH_EINVAL, "%s: batch %d needs max_frames >= %d (the context has %d)",
                             who, b, 2 * b, r->frames - 1);
    if (r->sub_n > 0)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames pending (collect them first)", who,
                             rgbd_track_pending(r));
    const int old = r->trk_b;
    r->trk_b = b;
    r->trk_bank = 0;
    for (auto& q : r->sub) q.m = 0;  // collected: nothing reads the banks
    return old;
}

int youth_rgbd_track_set_depth_filter(youth_rgbd_ctx* r, const youth_filter_params* P)
{
    static const char* who = "youth_rgbd_track_set_depth_filter";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (P && !filter_params_ok(P))
        return g_icp_err.set(YOUTH_EINVAL, "%s: t0 %d, t2 %d (need 1 <= t0 <= 255, 0 <= t2 <= 1000)",
                             who, P->t0, P->t2);
    if (r->sub_n > 0)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames pending (collect them first)", who,
                             rgbd_track_pending(r));
    if (P) r->flt = *P;
    r->flt_on = P != nullptr;
    return YOUTH_OK;
}

int youth_rgbd_track_submit(youth_rgbd_ctx* r, const int16_t* const* depth,
                            const uint8_t* const* rgb, int n_frames)
{
    static const char* who = "youth_rgbd_track_submit";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (r->sched.n > 0)
        return g_icp_err.set(YOUTH_EINVAL,
                             "%s: the context has an align schedule (youth_rgbd_set_levels; 0 levels "
                             "switch it off); the streaming tracker runs its own, "
                             "youth_rgbd_track_set_levels",
                             who);
    int rc = rgbd_check_frames(who, depth, rgb, n_frames, r->trk_b);
    if (rc) return rc;
    if (r->sub_n >= 2)
        return g_icp_err.set(YOUTH_EINVAL, "%s: two submissions in flight (collect one first)", who);
    youth_icp_ctx* c = r->icp;
    rc = bind_device(c);
    if (rc) return rc;
    rc = rgbd_ensure_track(r);
    if (rc) return rc;
    if (r->flt_on) {
        rc = grow_device_buffer(g_icp_err, &r->d_raw, &r->trk_raw_cap, r->trk_b, (size_t)c->N);
        if (rc) return rc;
    }
    auto& q = r->sub[(r->sub_head + r->sub_n) % 2];
    const int16_t* dp[YOUTH_TRACK_MAX_BATCH];
    const uint8_t* cp[YOUTH_TRACK_MAX_BATCH];
    const bool stage = !rgbd_frames_pinned(r, depth, rgb, n_frames);
    if (stage) {  // the entry's staging is free: its last submission has been collected
        rc = rgbd_ensure_stage(r, &q.stage_d, &q.stage_c, &q.stage_cap, r->trk_b);
        if (rc) return rc;
    }
    rgbd_stage_frames(r, depth, rgb, n_frames, stage ? q.stage_d : nullptr, q.stage_c, dp, cp);
    rc = rgbd_track_enqueue(r, q, dp, cp, n_frames);
    if (rc) {
        // nothing of these frames is kept: wait for what was enqueued, and the
        // next frame starts a new sequence (the record slots may be half written)
        (void)hipStreamSynchronize(c->xfer);
        (void)hipStreamSynchronize(c->stream);
        r->trk_ref = -1;
        return rc;
    }
    q.m = n_frames;
    q.next = 0;
    q.n_lv = r->trk_sched.n;
    q.first_has_ref = r->trk_ref >= 0 ? 1 : 0;
    r->trk_ref = n_frames;  // the last new frame's record / word slot
    r->trk_bank ^= 1;
    ++r->sub_n;
    return YOUTH_OK;
}

int youth_rgbd_track_collect(youth_rgbd_ctx* r, double* T_rel, int* has_ref)
{
    static const char* who = "youth_rgbd_track_collect";
    if (!r || !T_rel) return g_icp_err.set(YOUTH_EINVAL, "%s: null %s", who, r ? "T_rel" : "context");
    if (r->sub_n == 0) return g_icp_err.set(YOUTH_EINVAL, "%s: no frame pending", who);
    int rc = bind_device(r->icp);
    if (rc) return rc;
    auto& q = r->sub[r->sub_head];
    // always polled: YOUTH_ICP_TRACK_WAIT is the depth tracker's switch
    const hipError_t e = wait_event_polled(q.done, true);
    const int i = q.next++;
    if (q.next == q.m) {
        r->sub_head ^= 1;
        --r->sub_n;
    }
    HIP_TRY(e);
    const int has = (i > 0 || q.first_has_ref) ? 1 : 0;
    if (has_ref) *has_ref = has;
    for (int k = 0; k < 16; ++k) T_rel[k] = (k % 5) == 0 ? 1.0 : 0.0;
    r->last_lv_n = 0;
    if (!has) return 0;
    const int p = q.first_has_ref ? i : i - 1;
    const int n_lv = std::max(1, q.n_lv);
    const int32_t* res_st = reinterpret_cast<const int32_t*>(q.res + (size_t)q.res_lv * q.res_cap * 16);
    int32_t st = 0;  // the OR of all levels' status words
    for (int l = 0; l < n_lv; ++l) {
        const double* Tl = q.res + ((size_t)l * q.res_cap + p) * 16;
        const int32_t sl = res_st[(size_t)l * q.res_cap + p];
        st |= sl;
        if (q.n_lv > 0) {
            memcpy(r->last_lv_T[l], Tl, 16 * sizeof(double));
            r->last_lv_st[l] = sl;
        }
        if (l == n_lv - 1)
            for (int k = 0; k < 12; ++k) T_rel[k] = Tl[k];
    }
    r->last_lv_n = q.n_lv;
    return st;
}

int youth_rgbd_track_pending(const youth_rgbd_ctx* r) { return r ? rgbd_track_pending(r) : 0; }

int youth_rgbd_track_reset(youth_rgbd_ctx* r)
{
    static const char* who = "youth_rgbd_track_reset";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    if (r->sub_n > 0)
        return g_icp_err.set(YOUTH_EINVAL, "%s: %d frames pending (collect them first)", who,
                             rgbd_track_pending(r));
    r->trk_ref = -1;
    return YOUTH_OK;
}

int youth_rgbd_track_set_levels(youth_rgbd_ctx* r, const youth_rgbd_level* levels, int n)
{
    static const char* who = "youth_rgbd_track_set_levels";
    int rc = rgbd_check_levels(who, r, levels, n, true);
    if (rc) return rc;
    rc = bind_device(r->icp);
    if (rc) return rc;
    // the new schedule beside the old one, which stays if anything fails
    youth_rgbd_ctx::Schedule next;
    rc = rgbd_build_schedule(who, r, levels, n, false, next);
    if (rc) return rc;
    // no frame pending: the old levels' work on this context's streams has run
    rgbd_drop_schedule(r->trk_sched, r);
    r->trk_sched = next;
    r->trk_ref = -1;  // the next frame starts a new sequence, at every level
    r->last_lv_n = 0;
    return YOUTH_OK;
}

int youth_rgbd_track_get_levels(const youth_rgbd_ctx* r, youth_rgbd_level* out, int cap)
{
    if (!r || cap < 0 || (cap > 0 && !out))
        return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_track_get_levels: %s",
                             r ? "bad arguments" : "null context");
    for (int l = 0; l < std::min(cap, r->trk_sched.n); ++l) out[l] = r->trk_sched.at[l].lv;
    return r->trk_sched.n;
}

int youth_rgbd_track_last_levels(youth_rgbd_ctx* r, double* T64, int32_t* status)
{
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "youth_rgbd_track_last_levels: null context");
    for (int l = 0; l < r->last_lv_n; ++l) {
        if (T64) {
            memcpy(T64 + (size_t)l * 16, r->last_lv_T[l], 12 * sizeof(double));
            const double row[4] = {0.0, 0.0, 0.0, 1.0};
            memcpy(T64 + (size_t)l * 16 + 12, row, sizeof(row));
        }
        if (status) status[l] = r->last_lv_st[l];
    }
    return r->last_lv_n;
}

int youth_rgbd_pull_host(youth_rgbd_ctx* r, const int16_t* const* depth, const uint8_t* const* rgb,
                         int m, int16_t* d_depth, uint8_t* d_gray, uint8_t* d_rgb, void* stream)
{
    static const char* who = "youth_rgbd_pull_host";
    if (!r) return g_icp_err.set(YOUTH_EINVAL, "%s: null context", who);
    int rc = rgbd_check_frames(who, depth, rgb, m, YOUTH_TRACK_MAX_BATCH);
    if (rc) return rc;
    if (!d_depth || !d_gray) return g_icp_err.set(YOUTH_EINVAL, "%s: null destination", who);
    rc = bind_device(r->icp);
    if (rc) return rc;
    hipStream_t s = pick_stream(r->icp, stream);
    const int16_t* dp[YOUTH_TRACK_MAX_BATCH];
    const uint8_t* cp[YOUTH_TRACK_MAX_BATCH];
    const bool stage = !rgbd_frames_pinned(r, depth, rgb, m);
    if (stage) {
        // one staging for this entry point: the pull before it must have read it
        if (!r->pull_ev) HIP_TRY(hipEventCreateWithFlags(&r->pull_ev, hipEventDisableTiming));
        HIP_TRY(hipEventSynchronize(r->pull_ev));
        rc = rgbd_ensure_stage(r, &r->pull_stage_d, &r->pull_stage_c, &r->pull_stage_cap,
                               YOUTH_TRACK_MAX_BATCH);
        if (rc) return rc;
    }
    rgbd_stage_frames(r, depth, rgb, m, stage ? r->pull_stage_d : nullptr, r->pull_stage_c, dp, cp);
    rc = rgbd_launch_pull(r, s, dp, cp, m, d_depth, d_gray, d_rgb);
    if (rc) return rc;
    if (stage) HIP_TRY(hipEventRecord(r->pull_ev, s));
    return YOUTH_OK;
}

}  // extern "C"
