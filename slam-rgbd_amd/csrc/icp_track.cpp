// icp_track.cpp — the pipelined tracker (include/youth_icp.h,
// youth_icp_track_*): frames submitted one at a time or in micro-batches, each
// aligned to the frame before it, results collected in order; the depth filter
// in front of it; the page-locked buffers it reads in place.  Host code only.
// Two helpers at the tail serve rgbd_track.cpp as well (icp_host.h):
// host_alloc_covers_bytes and wait_event_polled.

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <thread>

#include "icp_host.h"
#include "youth_filter.h"

using namespace youth_icp;

extern "C" {

// ------------------------------------------------------ frame tracking --
// Lazily: the transfer stream and the ring's events.  The pinned staging
// frame and result slot of a ring entry are allocated when a submission first
// uses that entry (track_entry_pinned), so a context that keeps at most two
// frames in flight (the SLAM worker) pins two frames, not the ring's 16
// (16 x W x H x 2 bytes is 512 MB at 4096 x 4096).
static int ensure_track(youth_icp_ctx* c)
{
    if (c->trk[kTrackDepth - 1].done_nf) return YOUTH_OK;
    if (!c->xfer) HIP_TRY(hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking));
    for (auto& q : c->trk) {
        if (!q.h2d) HIP_TRY(hipEventCreateWithFlags(&q.h2d, hipEventDisableTiming));
        if (!q.done) HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
        if (!q.done_nf)
            HIP_TRY(hipEventCreateWithFlags(&q.done_nf,
                                            hipEventDisableTiming | hipEventDisableSystemFence));
    }
    return YOUTH_OK;
}

// The ring holds trk_cap entries and grows only when a submission would put
// more than trk_cap frames in flight: it is rotated so the oldest in-flight
// entry is entry 0 (indices in trk_dslot_last follow), then extended, so the
// in-flight entries stay consecutive modulo the new size.
static void track_grow(youth_icp_ctx* c, int need)
{
    if (need <= c->trk_cap) return;
    const int cap = c->trk_cap, h = c->trk_head;
    if (h) {
        youth_icp_ctx::TrackSlot tmp[kTrackDepth];
        for (int i = 0; i < cap; ++i) tmp[i] = c->trk[(h + i) % cap];
        for (int i = 0; i < cap; ++i) c->trk[i] = tmp[i];
        for (int& d : c->trk_dslot_last)
            if (d >= 0) d = (d - h + cap) % cap;
        c->trk_head = 0;
    }
    c->trk_cap = std::min(kTrackDepth, need);
}

static int track_entry_pinned(youth_icp_ctx* c, int e, bool staging)
{
    auto& q = c->trk[e];
    if (staging && !q.pinned)
        HIP_TRY(hipHostMalloc((void**)&q.pinned, (size_t)c->N * sizeof(int16_t),
                              hipHostMallocDefault));
    if (!q.res) HIP_TRY(hipHostMalloc((void**)&q.res, 17 * sizeof(double), hipHostMallocCoherent));
    return YOUTH_OK;
}

// Depth slots of the tracker (device staging of host frames): two halves of
// B slots (B = the largest micro-batch the context has room for: a launch
// takes consecutive slots of one half, the other half stays with the launch
// before), or 2 (one frame per launch).  Record slots: B + 1 (a micro-batch
// preps its B new frames beside the reference), at least 2.
static int trk_half(const youth_icp_ctx* c)
{
    return std::max(1, std::min(kCoopMaxChain, c->max_frames / 2));
}
static int trk_depth_slots(const youth_icp_ctx* c) { return 2 * trk_half(c); }
static int trk_record_slots(const youth_icp_ctx* c)
{
    return std::max(2, std::min(kCoopMaxChain + 1, c->max_frames));
}

// Whether m consecutive frames can be aligned as one k_icp_coop micro-batch:
// every pair on the single-pair plan (bit-identical to track_frame), the m
// grids co-resident, room for the slots.
static bool trk_chain_fits(const youth_icp_ctx* c, int m)
{
    if (m < 2 || m > kCoopMaxChain || m > trk_half(c) || trk_record_slots(c) < m + 1 ||
        c->prm.iters <= 0 || c->coop_refuse)
        return false;
    int npx = 0, G = 0;
    if (!coop_plan(c, 1, &npx, &G)) return false;
    return (long long)m * G <=
           (long long)c->n_cu *
               c->coop_bpc[c->coop_threads == 256][variant(c) * 2 + (c->fast ? 1 : 0)][npx];
}

// m consecutive host frames (m = 1, or a micro-batch that trk_chain_fits):
// staged into m consecutive depth slots not read by the previous launch,
// H2D on the transfer stream (after the last launch that read those slots),
// then ONE launch on the context stream: prep only (no reference yet), the
// single-pair align with the fused prep of the new frame, or the chained
// micro-batch (pair i aligns frame i to frame i-1, frame -1 = the
// reference).  One completion event for the launch, shared by its entries.
// frames (nullable): the m frames are the caller's page-locked buffers,
// copied H2D in place (no staging copy; youth_icp_track_submit_pinned).
// Page-locked buffers handed out by youth_icp_host_alloc, by base address:
// k_pull_frames reads a caller's frame in place only when it lies inside one
// of them (youth_icp_track_submit_pinned); any other pointer goes through
// hipMemcpyAsync, so a pageable buffer passed by mistake is copied by the
// runtime instead of faulting the GPU.
static std::mutex g_host_mu;
static std::map<uintptr_t, size_t> g_host_bufs;  // base -> bytes (host_alloc_covers_bytes, below)

// the SLAM module's event trace (slam_api.cpp, youth_slam_trace_enable):
// steps inside a submission, YOUTH_SLAM_EV_SUBMIT_STEP.  Weak: a program
// linking this unit without slam_api.cpp records nothing.
extern "C" __attribute__((weak)) void youth_slam_trace_hook(int kind, int arg);
static inline void trace_step(int step)
{
    if (youth_slam_trace_hook) youth_slam_trace_hook(YOUTH_SLAM_EV_SUBMIT_STEP, step);
}

// Raw staging of the filter: the frames of one launch (the transfer stream
// pulls, then filters, launch after launch in order), two for a realign.
static int trk_raw_slots(const youth_icp_ctx* c) { return std::max(2, trk_half(c)); }

static int ensure_raw(youth_icp_ctx* c)
{
    if (c->d_raw) return YOUTH_OK;
    HIP_TRY(hipMalloc(&c->d_raw, (size_t)trk_raw_slots(c) * c->N * sizeof(int16_t)));
    return YOUTH_OK;
}

// The depth filter (depth_filter.hip, youth_filter.h): d_raw[0 .. n) ->
// dst[0 .. n) on `stream`
static int track_filter(youth_icp_ctx* c, int n, int16_t* dst, hipStream_t stream)
{
    const int rc = youth_depth_filter_device(c->device, c->d_raw, dst, n, c->W, c->H, &c->flt, stream);
    if (rc) return g_icp_err.set(rc, "depth filter: %s", youth_depth_filter_last_error());
    return YOUTH_OK;
}

int youth_icp_set_depth_filter(youth_icp_ctx* c, const youth_filter_params* P)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "set_depth_filter: null context");
    if (P && !filter_params_ok(P))
        return g_icp_err.set(YOUTH_EINVAL,
                             "set_depth_filter: t0 %d, t2 %d (need 1 <= t0 <= 255, 0 <= t2 <= 1000)",
                             P->t0, P->t2);
    if (c->trk_n > 0)
        return g_icp_err.set(YOUTH_EINVAL, "set_depth_filter: %d frames in flight (collect them first)",
                             c->trk_n);
    if (P) {
        int rc = bind_device(c);
        if (rc) return rc;
        rc = ensure_raw(c);
        if (rc) return rc;
        c->flt = *P;
    }
    c->flt_on = P != nullptr;
    return YOUTH_OK;
}

int youth_icp_get_depth_filter(const youth_icp_ctx* c, youth_filter_params* out)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "get_depth_filter: null context");
    if (c->flt_on && out) *out = c->flt;
    return c->flt_on ? 1 : 0;
}

static int track_submit_frames(youth_icp_ctx* c, const int16_t* depth, int m,
                               const double* T_init, const int16_t* const* frames = nullptr)
{
    hipStream_t s = c->stream;
    const size_t N = c->N;
    const int nds = trk_depth_slots(c), nrs = trk_record_slots(c);
    // depth slots: the half the previous launch did not use
    const int half = nds / 2;
    const int d0 = c->trk_prev_d0 >= half || c->trk_prev_d0 < 0 ? 0 : half;
    // record slots for the new frames: the first m that are not the reference
    const int ref = c->track_ref;
    int rs[kCoopMaxChain] = {};
    for (int r = 0, k = 0; r < nrs && k < m; ++r)
        if (r != ref) rs[k++] = r;
    int qi[kCoopMaxChain];
    if (c->flt_on) {   // enabled by the environment: the staging comes with the first frame
        const int rc = ensure_raw(c);
        if (rc) return rc;
    }
    // where the upload lands: the depth slots, or the filter's raw staging
    int16_t* const land = c->flt_on ? c->d_raw : c->d_depth + (size_t)d0 * N;
    track_grow(c, c->trk_n + m);
    for (int i = 0; i < m; ++i) {
        qi[i] = (c->trk_head + c->trk_n + i) % c->trk_cap;
        const int rc = track_entry_pinned(c, qi[i], !frames);  // before anything is enqueued
        if (rc) return rc;
    }
    trace_step(1);
    auto& ql = c->trk[qi[m - 1]];
    // the caller's buffers are free on return: copy into the entries' pinned
    // staging, then H2D after the last launch that read these depth slots
    // the copies' stream: the transfer stream (overlaps the launch before),
    // or with YOUTH_ICP_TRACK_COPY=compute the launch stream itself (A/B)
    hipStream_t xs = c->trk_copy_compute ? s : c->xfer;
    if (!frames) {
        const size_t fb = N * sizeof(int16_t);
        if (c->trk_copy_helpers > 0 && (size_t)m * fb >= c->trk_copy_min) {
            if (!c->copy_pool) c->copy_pool.reset(new youth::HostCopyPool(c->trk_copy_helpers));
            youth::HostCopyPool::Seg seg[kCoopMaxChain];
            for (int i = 0; i < m; ++i) seg[i] = {c->trk[qi[i]].pinned, depth + (size_t)i * N, fb};
            // ~4 pieces per copier per micro-batch: late wake-ups even out
            const size_t piece = (size_t)m * fb / (4 * (c->trk_copy_helpers + 1));
            c->copy_pool->run(seg, m, std::max(piece, (size_t)64 << 10));
        } else {
            for (int i = 0; i < m; ++i) memcpy(c->trk[qi[i]].pinned, depth + (size_t)i * N, fb);
        }
    }
    hipEvent_t waited[kCoopMaxChain];
    int nw = 0;
    for (int i = 0; i < m; ++i) {
        const int last = c->trk_dslot_last[d0 + i];
        if (last < 0 || xs == s) continue;
        // the slots of one earlier launch share its event: wait once per event
        hipEvent_t ev = c->trk[last].ev;
        bool dup = false;
        for (int k = 0; k < nw; ++k) dup |= waited[k] == ev;
        if (!dup) {
            HIP_TRY(hipStreamWaitEvent(xs, ev, 0));
            waited[nw++] = ev;
        }
    }
    trace_step(2);
    // the caller's frames are pulled in place only when youth_icp_host_alloc
    // made them (the staging buffers always are page-locked)
    bool pull = !c->trk_copy_sdma;
    for (int i = 0; pull && frames && i < m; ++i)
        pull = host_alloc_covers_bytes(frames[i], N * sizeof(int16_t));
    if (pull) {
        const int16_t* src[kCoopMaxChain];
        for (int i = 0; i < m; ++i) src[i] = frames ? frames[i] : c->trk[qi[i]].pinned;
        // ~16 workgroups per launch: 2 per frame in a micro-batch of 8 (one
        // per free CU, profiles/r05/slam_pull_reserve_r5s.txt), 16 for a
        // single frame (its latency)
        const int wg = c->trk_pull_wg > 0 ? c->trk_pull_wg : std::max(2, 16 / m);
        // its LDS reservation (unused) keeps a workgroup off the CUs where a
        // micro-batch grid's workgroup sits (~143 KB of 160 at 640x480), so
        // the pull runs on the CUs the plan left free instead of slowing the
        // grid's barriers (youth_icp_track_set_batch)
        const int rc = launch_pull_frames(c, xs, src, m, land, (int)N, wg);
        if (rc) return rc;
    } else {
        for (int i = 0; i < m; ++i)
            HIP_TRY(hipMemcpyAsync(land + (size_t)i * N,
                                   frames ? frames[i] : c->trk[qi[i]].pinned, N * sizeof(int16_t),
                                   hipMemcpyHostToDevice, xs));
    }
    if (c->flt_on) {   // raw staging -> depth slots, before the H2D event
        const int rc = track_filter(c, m, c->d_depth + (size_t)d0 * N, xs);
        if (rc) return rc;
    }
    trace_step(3);
    if (xs != s) {
        HIP_TRY(hipEventRecord(ql.h2d, xs));
        HIP_TRY(hipStreamWaitEvent(s, ql.h2d, 0));
    }
    trace_step(4);
    const int16_t* dsrc = c->d_depth + (size_t)d0 * N;
    int rc = YOUTH_OK;
    bool kernel_result = false;  // k_icp_coop stored the result(s) to host memory
    if (ref < 0) {
        // first frame of a sequence: prep only (m == 1)
        rc = launch_prep(c, s, dsrc, 1, rs[0], false);
    } else if (m == 1) {
        // source: the new frame's depth; target: ref's records; the new frame
        // is prepped beside the iterations as the next reference.  k_icp_coop
        // writes the result into the pinned slot itself; any other kernel path
        // copies it
        const PrepJob job{dsrc, 1, rs[0], false};
        c->coop_res_host = ql.res;
        rc = run_iterations(c, s, dsrc, 0, ref, 1, T_init, nullptr, nullptr, &job);
        c->coop_res_host = nullptr;
        kernel_result = c->last_coop;
        if (rc == YOUTH_OK && !c->last_coop) {
            HIP_TRY(hipMemcpyAsync(ql.res, c->d_T64, 16 * sizeof(double), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(ql.res + 16, c->d_status, sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
        }
    } else {
        PrepJob job{dsrc, m, 0, false};
        job.chain = true;
        for (int i = 0; i < m; ++i) {
            job.tgt_slot[i] = i == 0 ? ref : rs[i - 1];
            job.prep_slot[i] = rs[i];
            job.res[i] = c->trk[qi[i]].res;
        }
        rc = run_iterations(c, s, dsrc, 0, 0, m, nullptr, nullptr, nullptr, &job);
        kernel_result = true;
        if (rc == YOUTH_OK) ++c->trk_chained;
    }
    trace_step(5);
    if (rc) {
        // nothing of these frames is kept; wait for what was enqueued so the
        // staging buffers and the slots are not in use by dropped frames
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(c->xfer);
        return rc;
    }
    // no result to publish (first frame) or k_icp_coop stored it to host
    // memory itself: no system-scope fence; else the copies' result needs it
    hipEvent_t ev = (ref < 0 || kernel_result) ? ql.done_nf : ql.done;
    HIP_TRY(hipEventRecord(ev, s));
    for (int i = 0; i < m; ++i) {
        auto& q = c->trk[qi[i]];
        q.ev = ev;
        q.has_ref = (i > 0 || ref >= 0) ? 1 : 0;
        c->trk_dslot_last[d0 + i] = qi[m - 1];
    }
    c->trk_prev_d0 = d0;
    c->track_ref = rs[m - 1];
    c->trk_n += m;
    return YOUTH_OK;
}

int youth_icp_track_submit(youth_icp_ctx* c, const int16_t* depth, const double* T_init)
{
    if (!c || !depth) return g_icp_err.set(YOUTH_EINVAL, "track_submit: bad arguments");
    if (c->trk_n >= kTrackDepth)
        return g_icp_err.set(YOUTH_EINVAL, "track_submit: %d frames in flight (collect one first)",
                             kTrackDepth);
    if (T_init)
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(T_init[i]))
                return g_icp_err.set(YOUTH_EINVAL, "T_init: non-finite entry in pair 0");
    int rc = bind_device(c);
    if (rc) return rc;
    rc = ensure_track(c);
    if (rc) return rc;
    return track_submit_frames(c, depth, 1, T_init);
}

// youth_icp_track_submit_batch (depth: n_frames consecutive frames, staged)
// and youth_icp_track_submit_pinned (frames: the caller's page-locked buffers).
static int track_submit_many(youth_icp_ctx* c, const int16_t* depth,
                             const int16_t* const* frames, int n_frames)
{
    if (c->trk_n + n_frames > kTrackDepth)
        return g_icp_err.set(YOUTH_EINVAL, "track_submit_batch: %d + %d frames in flight (max %d)",
                             c->trk_n, n_frames, kTrackDepth);
    int rc = bind_device(c);
    if (rc) return rc;
    rc = ensure_track(c);
    if (rc) return rc;
    const size_t N = c->N;
    int done = 0;
    if (c->track_ref < 0) {  // no reference yet: the first frame is only prepped
        rc = track_submit_frames(c, depth, 1, nullptr, frames);
        if (rc) return rc;
        done = 1;
    }
    // the rest in the longest chains that fit, else one launch per frame
    while (done < n_frames) {
        int m = n_frames - done;
        while (m > 1 && !trk_chain_fits(c, m)) --m;
        rc = track_submit_frames(c, frames ? nullptr : depth + (size_t)done * N, m, nullptr,
                                 frames ? frames + done : nullptr);
        if (rc) return rc;
        if (m > 1) c->trk_chained_frames += m;
        done += m;
    }
    return YOUTH_OK;
}

int youth_icp_track_submit_batch(youth_icp_ctx* c, const int16_t* depth, int n_frames)
{
    if (!c || !depth || n_frames < 1 || n_frames > YOUTH_TRACK_MAX_BATCH)
        return g_icp_err.set(YOUTH_EINVAL, "track_submit_batch: bad arguments (%d frames)", n_frames);
    return track_submit_many(c, depth, nullptr, n_frames);
}

int youth_icp_track_submit_pinned(youth_icp_ctx* c, const int16_t* const* frames, int n_frames)
{
    if (!c || !frames || n_frames < 1 || n_frames > YOUTH_TRACK_MAX_BATCH)
        return g_icp_err.set(YOUTH_EINVAL, "track_submit_pinned: bad arguments (%d frames)", n_frames);
    for (int i = 0; i < n_frames; ++i)
        if (!frames[i]) return g_icp_err.set(YOUTH_EINVAL, "track_submit_pinned: frame %d is null", i);
    return track_submit_many(c, nullptr, frames, n_frames);
}

int16_t* youth_icp_host_alloc(size_t values)
{
    if (!values) return nullptr;
    int16_t* p = nullptr;
    if (hipHostMalloc((void**)&p, values * sizeof(int16_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_bufs[(uintptr_t)p] = values * sizeof(int16_t);
    return p;
}

void youth_icp_host_free(int16_t* p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_bufs.erase((uintptr_t)p);
    }
    (void)hipHostFree(p);
}

int youth_icp_track_collect(youth_icp_ctx* c, double* T_rel, int* has_ref)
{
    // YOUTH_ICP_TRACK_WAIT=sync keeps the blocking wait only (A/B)
    static const bool poll = [] {
        const char* e = getenv("YOUTH_ICP_TRACK_WAIT");
        return !(e && strcmp(e, "sync") == 0);
    }();
    if (!c || !T_rel) return g_icp_err.set(YOUTH_EINVAL, "track_collect: bad arguments");
    if (c->trk_n == 0) return g_icp_err.set(YOUTH_EINVAL, "track_collect: no frame in flight");
    int rc = bind_device(c);
    if (rc) return rc;
    auto& q = c->trk[c->trk_head];
    c->trk_head = (c->trk_head + 1) % c->trk_cap;
    --c->trk_n;
    HIP_TRY(wait_event_polled(q.ev, poll));
    if (has_ref) *has_ref = q.has_ref;
    if (!q.has_ref) {
        for (int i = 0; i < 16; ++i) T_rel[i] = (i % 5) == 0 ? 1.0 : 0.0;
        return 0;
    }
    for (int i = 0; i < 12; ++i) T_rel[i] = q.res[i];
    T_rel[12] = 0.0;
    T_rel[13] = 0.0;
    T_rel[14] = 0.0;
    T_rel[15] = 1.0;
    int32_t st;
    memcpy(&st, q.res + 16, sizeof(st));
    return st;
}

int youth_icp_track_pending(const youth_icp_ctx* c)
{
    return c ? c->trk_n : 0;
}

// A tracker align that came back with YOUTH_STATUS_TIMEOUT (its cooperative
// grid was not co-resident: another process held CUs, or the test hook) is
// aligned again here from host copies of its two frames, synchronously.
// Everything the tracker has enqueued finishes first, so the depth slots
// 0 / 1 and a record slot other than the reference's are free to use, and
// the tracker continues afterwards as if nothing had happened (its reference
// records are untouched; a timed-out launch still preps every tile of its
// frames, because its workgroups prep before they wait).
//   1. the context's own single-pair plan: the cooperative kernel preps the
//      target and aligns, with the npx / G / tile mapping the tracker's
//      single-frame and chained launches use, so a successful retry gives the
//      pose the undisturbed launch would have, bit for bit;
//   2. if that times out too, the persistent k_prep + k_icp, which waits only
//      on workgroups that are running (no co-residency assumption): the same
//      pose up to fp64 summation order (~1e-16 relative).
int youth_icp_track_realign(youth_icp_ctx* c, const int16_t* ref_depth, const int16_t* depth,
                            const double* T_init, double* T_rel)
{
    if (!c || !ref_depth || !depth || !T_rel)
        return g_icp_err.set(YOUTH_EINVAL, "track_realign: bad arguments");
    if (T_init)
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(T_init[i]))
                return g_icp_err.set(YOUTH_EINVAL, "T_init: non-finite entry in pair 0");
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s));
    if (c->xfer) HIP_TRY(hipStreamSynchronize(c->xfer));
    const size_t N = c->N;
    const int rslot = c->track_ref == 0 ? 1 : 0;
    if (c->flt_on) {
        rc = ensure_raw(c);
        if (rc) return rc;
    }
    int16_t* const land = c->flt_on ? c->d_raw : c->d_depth;
    HIP_TRY(hipMemcpyAsync(land, depth, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(land + N, ref_depth, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    if (c->flt_on) {
        rc = track_filter(c, 2, c->d_depth, s);
        if (rc) return rc;
    }
    const PrepJob job{c->d_depth + N, 1, rslot, true};
    c->coop_res_host = nullptr;
    int32_t st = YOUTH_STATUS_TIMEOUT;
    for (int attempt = 0; attempt < 2 && (st & YOUTH_STATUS_TIMEOUT); ++attempt) {
        const bool coop_was = c->coop;
        if (attempt == 1) c->coop = false;  // the persistent kernel
        if (attempt == 0 && c->realign_stall) {  // test hook: this coop launch loses a row
            c->coop_stall_once = 0;
            c->coop_stall_left = 1;
        }
        rc = run_iterations(c, s, c->d_depth, 0, rslot, 1, T_init, nullptr, nullptr, &job);
        const bool ran_coop = c->last_coop;
        if (attempt == 1) c->coop = coop_was;
        if (rc) return rc;
        double T[16];
        unsigned err = 0;
        HIP_TRY(hipMemcpyAsync(T, c->d_T64, sizeof(T), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&st, c->d_status, sizeof(st), hipMemcpyDeviceToHost, s));
        if (!ran_coop)  // the persistent kernel's spin bound lands in the queue's error word
            HIP_TRY(hipMemcpyAsync(&err, c->d_head + kQError, sizeof(err), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (err) st |= YOUTH_STATUS_TIMEOUT;
        for (int i = 0; i < 12; ++i) T_rel[i] = T[i];
        T_rel[12] = T_rel[13] = T_rel[14] = 0.0;
        T_rel[15] = 1.0;
        if (!(st & YOUTH_STATUS_TIMEOUT)) ++c->trk_realigned[ran_coop ? 0 : 1];
        // a refused cooperative launch already ran the persistent path
        if (!ran_coop) break;
    }
    if (st & YOUTH_STATUS_TIMEOUT) ++c->trk_realigned[2];
    return st;
}

long long youth_icp_track_realigned(const youth_icp_ctx* c, long long* persistent, long long* failed)
{
    if (persistent) *persistent = c ? c->trk_realigned[1] : 0;
    if (failed) *failed = c ? c->trk_realigned[2] : 0;
    return c ? c->trk_realigned[0] : 0;
}

int youth_icp_track_host_sequence(youth_icp_ctx* c, const int16_t* frames, int n_frames,
                                  double* T_rel, int32_t* status)
{
    if (!c || !frames || n_frames < 0 || !T_rel)
        return g_icp_err.set(YOUTH_EINVAL, "track_host_sequence: bad arguments");
    if (c->trk_n) return g_icp_err.set(YOUTH_EINVAL, "track_host_sequence: submitted frames not collected");
    const size_t N = c->N;
    int written = 0, collected = 0;
    auto collect = [&]() -> int {
        double T[16];
        int has = 0;
        int st = youth_icp_track_collect(c, T, &has);
        const int f = collected++;  // sequence index of the collected frame
        if (st < 0) return st;
        // a timed-out align is aligned again against the frame before it
        // (frame 0's reference came from an earlier call: its status keeps
        // the TIMEOUT bit)
        if (has && (st & YOUTH_STATUS_TIMEOUT) && f >= 1) {
            const int st2 = youth_icp_track_realign(c, frames + (size_t)(f - 1) * N,
                                                    frames + (size_t)f * N, nullptr, T);
            if (st2 < 0) return st2;
            st = st2;
        }
        if (has) {
            memcpy(T_rel + (size_t)written * 16, T, sizeof(T));
            if (status) status[written] = st;
            ++written;
        }
        return YOUTH_OK;
    };
    // batch: frames per submission (1: one launch per frame, as the SLAM
    // worker at camera rate; 2: micro-batches of two frames when they fit one
    // cooperative grid, the pose of each frame bit-identical either way)
    const int batch = c->trk_batch;
    for (int f = 0; f < n_frames;) {
        const int m = std::min(batch, n_frames - f);
        // keep two submissions in flight: two frames, or two micro-batches
        while (c->trk_n + m > (batch > 1 ? 2 * batch : 2)) {
            const int rc = collect();
            if (rc) {
                while (c->trk_n) (void)collect();
                return rc;
            }
        }
        const int rc = m == 1 ? youth_icp_track_submit(c, frames + (size_t)f * N, nullptr)
                              : youth_icp_track_submit_batch(c, frames + (size_t)f * N, m);
        if (rc) {
            while (c->trk_n) (void)collect();
            return rc;
        }
        f += m;
    }
    while (c->trk_n) {
        const int rc = collect();
        if (rc) {
            while (c->trk_n) (void)collect();
            return rc;
        }
    }
    return written;
}

int youth_icp_track_frame(youth_icp_ctx* c, const int16_t* depth, const double* T_init,
                          double* T_rel, int* has_ref)
{
    if (!c || !depth || !T_rel) return g_icp_err.set(YOUTH_EINVAL, "track_frame: bad arguments");
    if (c->trk_n) return g_icp_err.set(YOUTH_EINVAL, "track_frame: submitted frames not collected");
    const int rc = youth_icp_track_submit(c, depth, T_init);
    if (rc) return rc;
    return youth_icp_track_collect(c, T_rel, has_ref);
}

int youth_icp_track_set_batch(youth_icp_ctx* c, int frames)
{
    if (!c || frames < 1 || frames > YOUTH_TRACK_MAX_BATCH)
        return g_icp_err.set(YOUTH_EINVAL, "track_set_batch: bad arguments (%d)", frames);
    const int old = c->trk_batch;
    c->trk_batch = frames;
    // batch mode: the fewest source pixels per lane whose workgroups for
    // `frames` pairs fit one grid (512-thread workgroups at 221 VGPRs are one
    // per CU: 256 per grid; 640x480: 5 px per lane, 120 workgroups per pair),
    // for every coop launch of the context, so batched and per-frame
    // submissions stay bit-identical
    c->coop_px = c->coop_px_env;
    if (frames > 1) {
        const int v = variant(c) * 2 + (c->fast ? 1 : 0);
        // the plan leaves trk_pull_reserve CUs free for the next micro-batch's
        // k_pull_frames (the co-residency limit itself stays the whole chip);
        // the same plan on either copy path, so their poses are bit-identical
        const int free_cu = std::min(c->trk_pull_reserve, c->n_cu / 2);
        for (int npx = 1; npx <= kCoopMaxPx; ++npx) {
            const long long G = (c->N + (long long)npx * c->coop_threads - 1) /
                                ((long long)npx * c->coop_threads);
            if (frames * G <= (long long)(c->n_cu - free_cu) * c->coop_bpc[c->coop_threads == 256][v][npx]) {
                c->coop_px = npx;
                break;
            }
        }
    }
    return old;
}

long long youth_icp_track_chained(const youth_icp_ctx* c) { return c ? c->trk_chained : 0; }

long long youth_icp_track_chained_frames(const youth_icp_ctx* c)
{
    return c ? c->trk_chained_frames : 0;
}

void youth_icp_track_reset(youth_icp_ctx* c)
{
    if (c) c->track_ref = -1;
}

}  // extern "C"

namespace youth_icp {

// For this tracker's depth frames and the RGB-D tracker's depth and colour
// frames (rgbd_track.cpp): all lie in buffers of youth_icp_host_alloc.
bool host_alloc_covers_bytes(const void* p, size_t bytes)
{
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_bufs.upper_bound(a);
    if (it == g_host_bufs.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

// A collect (here and in rgbd_track.cpp) waits for its frame by polling the
// event for up to 2 ms before the runtime's blocking wait: a sleeping wait's
// wake-up cost a backlogged SLAM worker up to ~0.6 ms per micro-batch
// (profiles/r04/slamtrace_r4k.txt).  poll false: the blocking wait only.
hipError_t wait_event_polled(hipEvent_t ev, bool poll)
{
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t r = hipEventQuery(ev);
            if (r != hipErrorNotReady) return r;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    return hipEventSynchronize(ev);
}

}  // namespace youth_icp
