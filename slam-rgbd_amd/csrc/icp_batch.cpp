// icp_batch.cpp — the one-shot host batch API (include/youth_icp.h):
// youth_icp_align_batch on one device, youth_icp_shard_range and
// youth_icp_align_batch_multi over every visible one.  Host code only.

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "icp_host.h"

using namespace youth_icp;

extern "C" {

// One cached context per device (guarded by that device's mutex), reused while
// the frame size, intrinsics and capacity fit.
static std::mutex g_batch_mu[64];
static youth_icp_ctx* g_batch_ctx[64] = {};

// Pairs per pipelined chunk of the host-buffer batch API (n_pairs: no
// pipelining).  YOUTH_ICP_BATCH_CHUNK overrides (0 disables).
static int batch_chunk(int n_pairs)
{
    if (const char* e = getenv("YOUTH_ICP_BATCH_CHUNK")) {
        const int v = atoi(e);
        return v <= 0 ? n_pairs : std::min(v, n_pairs);
    }
    // 16-pair chunks run the persistent kernel: copy ~ align.  8-pair chunks
    // (cooperative kernel) ran at 34 K on one box and 20-24 K on another, next to
    // the in-flight copies (profiles/r01/hostio_sweep.txt)
    return n_pairs >= 32 ? 16 : n_pairs;
}

// Workspace for an align of n_pairs whichever kernel path it takes
// (cooperative, persistent or per-iteration), so that no hipFree/hipMalloc
// runs while earlier chunks of a pipelined call are in flight.
static int reserve_for(youth_icp_ctx* c, int n_pairs)
{
    int chunk = 0;
    const int nb = reduce_geometry(c, n_pairs, &chunk);
    size_t need = (size_t)nb * n_pairs * kPartStride;
    int npx = 0, G = 0;
    if (coop_plan(c, n_pairs, &npx, &G))
        need = std::max(need, (size_t)2 * n_pairs * G * kPartStride);
    int rc = ensure_partials(c, need);
    if (rc) return rc;
    return ensure_stats(c, c->prm.iters > 0 ? c->prm.iters : 1);
}

// The host batch align of n_pairs pairs on ONE device: H2D of both depth
// stacks, align, poses (and per-pair status, nullable) back into the
// caller's rows.  Batches of >= 32 pairs are pipelined in chunks: chunk k's
// H2D on a transfer stream overlaps the align of chunk k-1 (every chunk has
// its own device frames, so nothing is reused inside one call).  On any error
// both streams are drained before returning, so no copy still reads the
// caller's buffers.  Caller holds g_batch_mu[dev].
static int batch_on_device(int dev, const int16_t* src, const int16_t* dst, int n_pairs, int W,
                           int H, const youth_intrinsics& Kd, int iters, float* T_out,
                           int32_t* status_out, int32_t* assoc_out)
{
    youth_icp_params P = youth_default_params();
    P.iters = iters;
    youth_icp_ctx*& slot = g_batch_ctx[dev];
    youth_icp_ctx* c = slot;
    const bool same = c && c->W == W && c->H == H && c->max_frames >= 2 * n_pairs &&
                      c->K.fx == Kd.fx && c->K.fy == Kd.fy && c->K.cx == Kd.cx &&
                      c->K.cy == Kd.cy && c->K.ds == Kd.depth_scale;
    if (!same) {
        if (c) youth_icp_destroy(c);
        slot = nullptr;
        c = youth_icp_create(dev, W, H, 2 * n_pairs, &Kd, &P);
        // youth_icp_create's text stands; of its codes only "no HIP device"
        // is passed on, every other failure (a bad size too) reads YOUTH_EHIP
        if (!c)
            return g_icp_err.code() == YOUTH_ENODEV ? YOUTH_ENODEV : YOUTH_EHIP;
        slot = c;
    }
    c->prm = P;
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    if (!c->xfer) HIP_TRY(hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking));
    // per-pair status on every call: a timed-out cooperative chunk is realigned below
    if (!c->d_status_out)
        HIP_TRY(hipMalloc(&c->d_status_out, (size_t)c->max_frames * sizeof(int32_t)));
    auto drain = [c, s](int code) {
        (void)hipStreamSynchronize(c->xfer);
        (void)hipStreamSynchronize(s);
        return code;
    };
    const size_t N = c->N;
    int16_t* d_s = c->d_depth;
    int16_t* d_d = c->d_depth + (size_t)n_pairs * N;
    const int chunk = assoc_out ? n_pairs : batch_chunk(n_pairs);
    const int n_chunks = (n_pairs + chunk - 1) / chunk;
    rc = reserve_for(c, chunk);
    if (!rc && n_pairs % chunk) rc = reserve_for(c, n_pairs % chunk);
    if (rc) return rc;
    while ((int)c->xfer_ev.size() < n_chunks) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->xfer_ev.push_back(e);
    }
    youth_lanes first_lanes{};
    bool mixed = false;
    for (int k = 0; k < n_chunks; ++k) {
        const size_t p0 = (size_t)k * chunk;
        const int cnt = (int)std::min<size_t>(chunk, n_pairs - p0);
        const size_t bytes = (size_t)cnt * N * sizeof(int16_t);
        hipError_t e = hipMemcpyAsync(d_s + p0 * N, src + p0 * N, bytes, hipMemcpyHostToDevice,
                                      c->xfer);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_d + p0 * N, dst + p0 * N, bytes, hipMemcpyHostToDevice, c->xfer);
        if (e == hipSuccess) e = hipEventRecord(c->xfer_ev[k], c->xfer);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, c->xfer_ev[k], 0);
        if (e != hipSuccess)
            return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
        rc = youth_icp_align_pairs_device(c, d_s + p0 * N, d_d + p0 * N, cnt, nullptr,
                                          c->d_Tout + p0 * 16, s);
        if (rc) return drain(rc);
        // a tail chunk may take another kernel (and lane partition) than the
        // full chunks: youth_icp_get_lanes then reports the call as mixed
        if (k == 0)
            first_lanes = c->lanes;
        else
            mixed |= memcmp(&first_lanes, &c->lanes, sizeof(youth_lanes)) != 0;
        if ((e = launch_status_out(c, s, cnt, c->d_status_out + p0)) != hipSuccess)
            return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
    }
    // A chunk of <= 16 pairs is one cooperative launch sized to an idle
    // device; on a GPU shared with other processes its grid may not be
    // co-resident, and it then times out (kCoopSpinMax polls, ~50 ms) with
    // partly iterated poses.  Such a chunk is aligned again, synchronously, on
    // the persistent k_prep + k_icp, which waits only on running workgroups:
    // the same poses up to fp64 summation order (its depth frames are still
    // on the device).  The caller never receives a TIMEOUT pose from here.
    {
        std::vector<int32_t> st((size_t)n_pairs);
        hipError_t e = hipMemcpyAsync(st.data(), c->d_status_out, (size_t)n_pairs * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
        for (int k = 0; k < n_chunks; ++k) {
            const size_t p0 = (size_t)k * chunk;
            const int cnt = (int)std::min<size_t>(chunk, n_pairs - p0);
            bool to = false;
            for (int i = 0; i < cnt; ++i) to |= (st[p0 + i] & YOUTH_STATUS_TIMEOUT) != 0;
            if (!to) continue;
            fprintf(stderr, "youth_icp: align_batch: a cooperative launch of %d pair(s) timed out "
                            "(GPU shared with another process?); realigned on the persistent kernel\n",
                    cnt);
            const bool coop_was = c->coop;
            c->coop = false;
            rc = youth_icp_align_pairs_device(c, d_s + p0 * N, d_d + p0 * N, cnt, nullptr,
                                              c->d_Tout + p0 * 16, s);
            c->coop = coop_was;
            if (rc) return drain(rc);
            ++c->batch_realigned;
            mixed = true;  // this chunk's lane partition is the persistent kernel's
            if ((e = launch_status_out(c, s, cnt, c->d_status_out + p0)) != hipSuccess)
                return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
        }
    }
    if (assoc_out) {
        int nb = 0;
        const youth_lanes align_lanes = c->lanes;  // youth_icp_get_lanes reports the align's
        rc = launch_reduce(c, s, d_s, 0, 0, n_pairs, true, &nb);
        c->lanes = align_lanes;
        if (rc) return drain(rc);
        hipError_t e = hipMemcpyAsync(assoc_out, c->d_assoc, (size_t)n_pairs * N * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, s);
        if (e != hipSuccess)
            return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
    }
    c->lanes_mixed = mixed;
    hipError_t e = hipMemcpyAsync(T_out, c->d_Tout, (size_t)n_pairs * 16 * sizeof(float),
                                  hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && status_out)
        e = hipMemcpyAsync(status_out, c->d_status_out, (size_t)n_pairs * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return drain(g_icp_err.set(YOUTH_EHIP, "align_batch: %s", hipGetErrorString(e)));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

int youth_icp_align_batch(const int16_t* src, const int16_t* dst, int n_pairs, int W, int H,
                          const youth_intrinsics* K, int iters, float* T_out,
                          int32_t* assoc_out)
{
    if (!src || !dst || n_pairs <= 0 || W < 3 || H < 3 || iters < 0 || !T_out)
        return g_icp_err.set(YOUTH_EINVAL, "align_batch: bad arguments %d", n_pairs);
    std::lock_guard<std::mutex> lk(g_batch_mu[0]);
    const youth_intrinsics Kd = K ? *K : youth_default_intrinsics(W, H);
    return batch_on_device(0, src, dst, n_pairs, W, H, Kd, iters, T_out, nullptr, assoc_out);
}

// Contiguous shard [first, first + count) of n pairs for part r of k (the
// first n % k parts get one more), as youth_dist.pair_range on the bench side.
static void shard_range(int n, int k, int r, int* first, int* count)
{
    const int q = n / k, m = n % k;
    *first = r * q + std::min(r, m);
    *count = q + (r < m ? 1 : 0);
}

int youth_icp_shard_range(int n_pairs, int n_parts, int part, int* first, int* count)
{
    if (n_pairs < 0 || n_parts <= 0 || part < 0 || part >= n_parts || !first || !count)
        return g_icp_err.set(YOUTH_EINVAL, "shard_range: bad arguments");
    shard_range(n_pairs, n_parts, part, first, count);
    return YOUTH_OK;
}

int youth_icp_align_batch_multi(const int16_t* src, const int16_t* dst, int n_pairs, int W,
                                int H, const youth_intrinsics* K, int iters, const int* devices,
                                int n_devices, float* T_out, int32_t* status_out)
{
    if (!src || !dst || n_pairs <= 0 || W < 3 || H < 3 || iters < 0 || !T_out)
        return g_icp_err.set(YOUTH_EINVAL, "align_batch_multi: bad arguments %d", n_pairs);
    const int ndev = youth_icp_device_count();
    if (ndev <= 0) return g_icp_err.set(YOUTH_ENODEV, "align_batch_multi: no HIP device");
    std::vector<int> devs;
    if (devices && n_devices > 0) {
        for (int i = 0; i < n_devices; ++i) {
            if (devices[i] < 0 || devices[i] >= ndev || devices[i] >= 64)
                return g_icp_err.set(YOUTH_EINVAL, "align_batch_multi: no HIP device %d", devices[i]);
            if (std::find(devs.begin(), devs.end(), devices[i]) != devs.end())
                return g_icp_err.set(YOUTH_EINVAL, "align_batch_multi: device %d listed twice",
                                     devices[i]);
            devs.push_back(devices[i]);
        }
    } else {
        for (int d = 0; d < std::min(ndev, 64); ++d) devs.push_back(d);
    }
    const int parts = std::min((int)devs.size(), n_pairs);
    const youth_intrinsics Kd = K ? *K : youth_default_intrinsics(W, H);
    const size_t N = (size_t)W * H;
    std::vector<int> rcs(parts, YOUTH_OK);
    std::vector<std::string> errs(parts);
    auto work = [&](int r) {
        int first = 0, cnt = 0;
        shard_range(n_pairs, parts, r, &first, &cnt);
        std::lock_guard<std::mutex> lk(g_batch_mu[devs[r]]);
        rcs[r] = batch_on_device(devs[r], src + (size_t)first * N, dst + (size_t)first * N, cnt, W,
                                 H, Kd, iters, T_out + (size_t)first * 16,
                                 status_out ? status_out + first : nullptr, nullptr);
        if (rcs[r]) errs[r] = g_icp_err.c_str();  // thread-local: carried to the caller below
    };
    // one host thread per device; shard 0 runs on the calling thread
    std::vector<std::thread> th;
    for (int r = 1; r < parts; ++r) th.emplace_back(work, r);
    work(0);
    for (auto& t : th) t.join();
    for (int r = 0; r < parts; ++r)
        if (rcs[r]) {
            return g_icp_err.set(rcs[r], "device %d: %s", devs[r], errs[r].c_str());
        }
    return YOUTH_OK;
}

}  // extern "C"
