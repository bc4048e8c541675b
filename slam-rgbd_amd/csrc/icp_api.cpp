// icp_api.cpp — the C API of the ICP context (include/youth_icp.h): create and
// destroy, the setters and getters, the last error's text, the device entry
// points and the stage-level host entry points.  Host code only: kernels are
// reached through the launch layer of icp_kernels.hip (icp_host.h).

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "icp_host.h"

using namespace youth_icp;

namespace youth_icp {

thread_local youth::ErrorText g_icp_err;

hipStream_t pick_stream(youth_icp_ctx* c, void* stream)
{
    return stream ? (hipStream_t)stream : c->stream;
}

int bind_device(youth_icp_ctx* c)
{
    HIP_TRY(hipSetDevice(c->device));
    return YOUTH_OK;
}

}  // namespace youth_icp

// FastK of the intrinsics: h = RN(1/y), l = RN((1 - y h) / y) with the
// residual 1 - y h exact (fma) and the quotient rounded once from fp64 (any
// l is safe: k_verify_fastdiv decides whether the pair is used).
static FastK fast_consts(const youth_intrinsics& K)
{
    auto hl = [](float y, float& h, float& l) {
        h = 1.0f / y;
        l = (float)((double)std::fma(-y, h, 1.0f) / (double)y);
    };
    FastK F;
    hl(K.fx, F.hfx, F.lfx);
    hl(K.fy, F.hfy, F.lfy);
    hl(K.depth_scale, F.hds, F.lds);
    return F;
}

// Whether k_icp's aligned pixel loop may form a lane's centred column
// coordinates by additions: ((float)(u & ~3) - cx) + (u & 3) must equal the
// spec's (float)u - cx for every column.  It does when cx is near the frame's
// centre (the difference then keeps cx's ulp); a principal point far to one
// side (e.g. cx = 20.9316 at W = 640: 9 columns) can make the difference
// round, and such intrinsics take the unaligned loop, which converts every
// column (tests/test_gpu_reduce.py::test_off_centre_principal_point).
static bool centred_exact(float cx, int W)
{
    for (int u = 0; u < W; ++u) {
        volatile float a = (float)u - cx;
        volatile float b0 = (float)(u & ~3) - cx;
        volatile float b = b0 + (float)(u & 3);
        if (a != b) return false;
    }
    return true;
}

// Whether the identity lemma's bound holds for these intrinsics (icp_device.h
// ident_accumulate): projecting a back-projected pixel returns
// its column within ~5 2^-24 |u - cx|, far below the half pixel the floor
// allows, as long as no operation of the round trip under- or overflows.
// With the principal point within 2^16 of the frame (|u - cx| < 2^17: 0.03 px)
// and focal lengths and depth scale in [2^-20, 2^20], every intermediate of
// (u - cx) z / fx and fx x / z stays a normal number for the depths 1 ..
// 32767 and z = d / ds stays inside the projection's fast range.  Intrinsics
// outside (none in practice) keep the general first iteration.
static bool ident_first_ok(const youth_intrinsics& K)
{
    auto mid = [](float v) { return v >= 0x1p-20f && v <= 0x1p20f; };
    return mid(K.fx) && mid(K.fy) && mid(K.depth_scale) && std::fabs(K.cx) <= 0x1p16f &&
           std::fabs(K.cy) <= 0x1p16f;
}

extern "C" {

youth_intrinsics youth_default_intrinsics(int width, int height)
{
    youth_intrinsics K;
    K.fx = 570.3f;  // viewerModule.c:344-345, astra_orb_slam3_rgbd.yaml:9-10
    K.fy = 570.3f;
    K.cx = (float)(width / 2);  // integer W/2 as in viewerModule.c:344
    K.cy = (float)(height / 2);
    K.depth_scale = 1000.0f;  // astra_orb_slam3_rgbd.yaml:35
    return K;
}

youth_icp_params youth_default_params(void)
{
    youth_icp_params p;
    p.iters = 10;
    p.dist_thresh = 0.10f;
    return p;
}

const char* youth_icp_last_error(void) { return g_icp_err.c_str(); }

int youth_icp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int youth_icp_fastdiv_enabled(youth_icp_ctx* c) { return c && c->fast ? 1 : 0; }

int youth_icp_set_spec(youth_icp_ctx* c, int spec)
{
    if (!c || (spec != YOUTH_SPEC_FMA && spec != YOUTH_SPEC_SURVEY))
        return g_icp_err.set(YOUTH_EINVAL, "set_spec: bad arguments (%d)", spec);
    const int old = c->spec;
    c->spec = spec;
    return old;
}

int youth_icp_set_reduce(youth_icp_ctx* c, int mode)
{
    if (!c || (mode != YOUTH_REDUCE_EXACT && mode != YOUTH_REDUCE_LANE32))
        return g_icp_err.set(YOUTH_EINVAL, "set_reduce: bad arguments (%d)", mode);
    const int old = c->reduce;
    c->reduce = mode;
    return old;
}

int youth_icp_get_reduce(const youth_icp_ctx* c)
{
    return c ? c->reduce : g_icp_err.set(YOUTH_EINVAL, "get_reduce: null context");
}

int youth_icp_get_lanes(const youth_icp_ctx* c, youth_lanes* out)
{
    if (!c || !out) return g_icp_err.set(YOUTH_EINVAL, "get_lanes: bad arguments");
    if (!c->has_lanes) return g_icp_err.set(YOUTH_EINVAL, "get_lanes: no align has run");
    if (c->lanes_mixed)
        return g_icp_err.set(YOUTH_EINVAL, "get_lanes: the last call ran launches of more than one "
                             "lane partition");
    *out = c->lanes;
    return YOUTH_OK;
}

int youth_icp_set_concurrency(youth_icp_ctx* c, int contexts)
{
    if (!c || contexts < 1 || contexts > YOUTH_ICP_MAX_CONCURRENCY)
        return g_icp_err.set(YOUTH_EINVAL, "set_concurrency: bad arguments (%d)", contexts);
    const int old = c->share;
    c->share = contexts;
    return old;
}

int youth_icp_get_spec(const youth_icp_ctx* c)
{
    return c ? c->spec : g_icp_err.set(YOUTH_EINVAL, "get_spec: null context");
}

void youth_icp_destroy(youth_icp_ctx* c)
{
    if (!c) return;
    // best-effort teardown: errors here cannot be reported to anyone useful
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto* v : {&c->ev_live, &c->ev_free})
        for (auto& e : *v) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
    if (c->xfer) (void)hipStreamSynchronize(c->xfer);
    for (hipEvent_t e : c->xfer_ev) (void)hipEventDestroy(e);
    for (auto& q : c->trk) {
        if (q.pinned) (void)hipHostFree(q.pinned);
        if (q.res) (void)hipHostFree(q.res);
        if (q.h2d) (void)hipEventDestroy(q.h2d);
        if (q.done) (void)hipEventDestroy(q.done);
        if (q.done_nf) (void)hipEventDestroy(q.done_nf);
    }
    void* bufs[] = {c->d_depth, c->d_rec,   c->d_xyz,      c->d_T64, c->d_T32,   c->d_status,
                    c->d_Tinit, c->d_stats, c->d_partials, c->d_neq, c->d_assoc, c->d_Tout,
                    c->d_flag,  c->d_arrivals, c->d_arr_it, c->d_epoch, c->d_head,
                    c->d_coop,  c->d_status_out, c->d_coop_part, c->d_raw};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    coop_forget_stream(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->xfer) (void)hipStreamDestroy(c->xfer);
    delete c;
}

youth_icp_ctx* youth_icp_create(int device, int W, int H, int max_frames,
                                const youth_intrinsics* K, const youth_icp_params* P)
{
    if (!youth::frame_size_ok(W, H, 3) || max_frames < 2) {
        g_icp_err.set(YOUTH_EINVAL,
                      "youth_icp_create: bad size %dx%d / max_frames %d (need 3 <= W, H <= 16384, "
                      "W*H <= 2^26, max_frames >= 2)",
                      W, H, max_frames);
        return nullptr;
    }
    const int ndev = youth_icp_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) {
        g_icp_err.set(YOUTH_ENODEV, "youth_icp_create: no HIP device %d", device);
        return nullptr;
    }
    auto* c = new youth_icp_ctx();
    for (int& d : c->trk_dslot_last) d = -1;
    c->device = device;
    c->W = W;
    c->H = H;
    c->N = W * H;
    c->P = ((size_t)c->N + 4 + 255) / 256 * 256;
    c->max_frames = max_frames;
    const youth_intrinsics Kd = K ? *K : youth_default_intrinsics(W, H);
    c->K = Intr{Kd.fx, Kd.fy, Kd.cx, Kd.cy, Kd.depth_scale};
    c->F = fast_consts(Kd);
    c->centred_exact = centred_exact(Kd.cx, W);
    c->prm = P ? *P : youth_default_params();
    auto fail = [&](const char* what, hipError_t e) -> youth_icp_ctx* {
        g_icp_err.set(YOUTH_EHIP, "youth_icp_create: %s (%d)", what, (int)e);
        youth_icp_destroy(c);
        return nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return fail("hipStreamCreate", e);
    const size_t MF = (size_t)max_frames;
    const size_t rec_bytes = c->P * sizeof(float4) * MF;
    if ((e = hipMalloc(&c->d_depth, MF * c->N * sizeof(int16_t))) != hipSuccess)
        return fail("hipMalloc depth", e);
    if ((e = hipMalloc(&c->d_rec, rec_bytes)) != hipSuccess) return fail("hipMalloc rec", e);
    // the pad beyond N of every frame must read as an invalid point (z = 0)
    if ((e = hipMemset(c->d_rec, 0, rec_bytes)) != hipSuccess) return fail("memset rec", e);
    if ((e = hipMalloc(&c->d_T64, MF * 16 * sizeof(double))) != hipSuccess)
        return fail("hipMalloc T64", e);
    if ((e = hipMalloc(&c->d_T32, MF * 12 * sizeof(float))) != hipSuccess)
        return fail("hipMalloc T32", e);
    if ((e = hipMalloc(&c->d_status, MF * sizeof(int32_t))) != hipSuccess)
        return fail("hipMalloc status", e);
    if ((e = hipMalloc(&c->d_Tinit, MF * 16 * sizeof(double))) != hipSuccess)
        return fail("hipMalloc Tinit", e);
    if ((e = hipMalloc(&c->d_neq, MF * kNeq * sizeof(double))) != hipSuccess)
        return fail("hipMalloc neq", e);
    if ((e = hipMalloc(&c->d_Tout, MF * 16 * sizeof(float))) != hipSuccess)
        return fail("hipMalloc Tout", e);
    if ((e = hipMalloc(&c->d_flag, 16)) != hipSuccess) return fail("hipMalloc flag", e);
    if ((e = hipMalloc(&c->d_epoch, MF * sizeof(unsigned))) != hipSuccess)
        return fail("hipMalloc epoch", e);
    if ((e = hipMalloc(&c->d_head, kQWords * 4)) != hipSuccess) return fail("hipMalloc head", e);
    if ((e = hipMemset(c->d_head, 0, kQWords * 4)) != hipSuccess) return fail("memset head", e);
    {
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
            return fail("hipGetDeviceProperties", e);
        c->n_cu = prop.multiProcessorCount;
        const char* what = nullptr;
        if ((e = fill_occupancy(c, &what)) != hipSuccess) return fail(what, e);
        const char* np = getenv("YOUTH_ICP_NO_PERSISTENT");
        c->persistent = !(np && *np && *np != '0');
        // A/B and test knob: k_icp's first iteration on the general path
        const char* nif = getenv("YOUTH_ICP_NO_IDENT_FIRST");
        c->ident_first = ident_first_ok(Kd) && !(nif && *nif && *nif != '0');
        const char* ifm = getenv("YOUTH_ICP_IDENT_FIRST");  // "icp": not inside the prep pass
        c->ident_prep = !(ifm && strcmp(ifm, "icp") == 0);
        const char* pbd = getenv("YOUTH_ICP_PREP_BAND");    // tuning knob
        if (pbd && atoi(pbd) >= 1) c->prep_band = atoi(pbd);
        const char* cth = getenv("YOUTH_ICP_COOP_THREADS");
        if (cth && atoi(cth) == 256) c->coop_threads = 256;
        const char* nc = getenv("YOUTH_ICP_NO_COOP");
        c->coop = !(nc && *nc && *nc != '0');
        const char* cpd = getenv("YOUTH_ICP_COOP_POLL_DELAY");  // tuning knob
        if (cpd && atoi(cpd) >= 0) c->coop_poll_delay = atoi(cpd);
        const char* cpx = getenv("YOUTH_ICP_COOP_PX");
        if (cpx && atoi(cpx) >= 1 && atoi(cpx) <= kCoopMaxPx) c->coop_px = atoi(cpx);
        c->coop_px_env = c->coop_px;
        const char* cl = getenv("YOUTH_ICP_COOP_LAUNCH");
        c->coop_launch = !cl ? 0 : strcmp(cl, "runtime") == 0 ? 1 : strcmp(cl, "plain") == 0 ? 2 : 0;
        const char* tcp = getenv("YOUTH_ICP_TRACK_COPY");
        c->trk_copy_compute = tcp && strcmp(tcp, "compute") == 0;
        c->trk_copy_sdma = tcp && (strcmp(tcp, "sdma") == 0 || c->trk_copy_compute);
        const char* pwg = getenv("YOUTH_ICP_PULL_WG");
        c->trk_pull_wg = pwg && atoi(pwg) > 0 ? std::min(atoi(pwg), 1024) : 0;
        const char* plds = getenv("YOUTH_ICP_PULL_LDS");
        if (plds && atoi(plds) >= 0) c->trk_pull_lds = std::min(atoi(plds), 64 << 10);
        const char* pres = getenv("YOUTH_ICP_PULL_RESERVE_CU");
        if (pres && atoi(pres) >= 0) c->trk_pull_reserve = atoi(pres);
        const char* cpt = getenv("YOUTH_ICP_COPY_THREADS");
        if (cpt && atoi(cpt) >= 0) c->trk_copy_helpers = std::min(atoi(cpt), 15);
        // test hooks (tests/): YOUTH_ICP_TEST_COOP_STALL=<chunk>[:<launches>]
        // makes the context's first <launches> (default 1) cooperative
        // launches lose chunk <chunk>'s iteration-1 row of pair 0, so they
        // time out (the tracker's realign path); YOUTH_ICP_TEST_REFUSE_COOP=1
        // refuses every cooperative launch as the runtime would (the
        // persistent fallback of run_iterations).  Either one is announced on
        // stderr: a stray variable must not pass for a device fault
        const char* cst = getenv("YOUTH_ICP_TEST_COOP_STALL");
        if (cst && atoi(cst) >= 0) {
            c->coop_stall_once = atoi(cst);
            const char* colon = strchr(cst, ':');
            c->coop_stall_left = colon && atoi(colon + 1) > 0 ? atoi(colon + 1) : 1;
            fprintf(stderr, "youth_icp: TEST HOOK YOUTH_ICP_TEST_COOP_STALL=%s active: the first %d "
                            "cooperative launch(es) of this context time out\n",
                    cst, c->coop_stall_left);
        }
        const char* sit = getenv("YOUTH_ICP_TEST_COOP_STALL_ITER");
        if (sit && atoi(sit) >= 0) c->coop_stall_iter = atoi(sit);
        const char* rst = getenv("YOUTH_ICP_TEST_REALIGN_STALL");
        c->realign_stall = rst && *rst && *rst != '0';
        if (c->realign_stall)
            fprintf(stderr, "youth_icp: TEST HOOK YOUTH_ICP_TEST_REALIGN_STALL active: the "
                            "cooperative launch of every youth_icp_track_realign times out\n");
        const char* crf = getenv("YOUTH_ICP_TEST_REFUSE_COOP");
        c->coop_refuse = crf && *crf && *crf != '0';
        if (c->coop_refuse)
            fprintf(stderr, "youth_icp: TEST HOOK YOUTH_ICP_TEST_REFUSE_COOP active: cooperative "
                            "launches of this context are refused\n");
        const char* nqs = getenv("YOUTH_ICP_QUEUES");
        if (nqs && atoi(nqs) >= 1 && atoi(nqs) <= kMaxQueues) c->queues = atoi(nqs);
        // A/B and test knob: k_icp's pixel loop without its phase priority
        // (icp_kernels.hip "Phase priority")
        const char* ipr = getenv("YOUTH_ICP_PRIO");
        if (ipr && (*ipr == '0' || *ipr == '1') && !ipr[1]) c->issue_prio = *ipr - '0';
        const char* pxm = getenv("YOUTH_ICP_PREP_XCD_MAP");
        if (pxm && (*pxm == '1' || *pxm == '2')) c->prep_xcd_map = *pxm - '0';
        const char* cts = getenv("YOUTH_ICP_COOP_TILE_SRC");
        if (cts && *cts == '0') c->coop_tile_src = false;
        const char* cmp = getenv("YOUTH_ICP_COOP_MAX_PAIRS");
        if (cmp && atoi(cmp) >= 0) c->coop_max_pairs = atoi(cmp);
        // spec a7/a8 arithmetic: "survey" (SURVEY §8a literally) or "fma"
        const char* sp = getenv("YOUTH_ICP_SPEC");
        if (sp && strcmp(sp, "survey") == 0) c->spec = kSpecSurvey;
        if (sp && strcmp(sp, "fma") == 0) c->spec = kSpecFma;
        // spec a9 reduction: "lane32" (SURVEY §8a a9 as worded) or "exact"
        const char* rd = getenv("YOUTH_ICP_REDUCE");
        if (rd && strcmp(rd, "lane32") == 0) c->reduce = YOUTH_REDUCE_LANE32;
        if (rd && strcmp(rd, "exact") == 0) c->reduce = YOUTH_REDUCE_EXACT;
        // the tracker's depth filter: "1" (defaults), "t0,t2", unset / "0" (off)
        const char* df = getenv("YOUTH_ICP_DEPTH_FILTER");
        if (df && *df && strcmp(df, "0") != 0) {
            youth_filter_params fp{8, 96};
            char tail = 0;
            const bool ok = strcmp(df, "1") == 0 ||
                            (sscanf(df, "%d,%d%c", &fp.t0, &fp.t2, &tail) == 2 &&
                             filter_params_ok(&fp));
            if (ok) {
                c->flt = fp;
                c->flt_on = true;   // the raw staging comes with the first tracked frame
            } else {
                fprintf(stderr, "youth_icp: YOUTH_ICP_DEPTH_FILTER=%s ignored (want 1, 0 or t0,t2 "
                                "with 1 <= t0 <= 255, 0 <= t2 <= 1000): the depth filter stays off\n",
                        df);
            }
        }
    }
    if ((e = hipMalloc(&c->d_coop, 2 * kCoopSetWords * sizeof(unsigned))) != hipSuccess)
        return fail("hipMalloc coop", e);
    if ((e = hipMemset(c->d_coop, 0, 2 * kCoopSetWords * sizeof(unsigned))) != hipSuccess)
        return fail("memset coop", e);
    const size_t arr_bytes = (MF * sizeof(unsigned) + 15) / 16 * 16;
    if ((e = hipMalloc(&c->d_arrivals, arr_bytes)) != hipSuccess)
        return fail("hipMalloc arrivals", e);
    if ((e = hipMemset(c->d_arrivals, 0, arr_bytes)) != hipSuccess)
        return fail("memset arrivals", e);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return fail("sync", e);
    if (ensure_stats(c, c->prm.iters > 0 ? c->prm.iters : 1) != YOUTH_OK ||
        verify_fastdiv(c) != YOUTH_OK) {
        youth_icp_destroy(c);
        return nullptr;
    }
    return c;
}

int youth_icp_align_pairs_device(youth_icp_ctx* c, const int16_t* d_src, const int16_t* d_dst,
                                 int n_pairs, const double* T_init, float* d_T_out,
                                 void* stream)
{
    if (!c || !d_src || !d_dst || n_pairs <= 0 || n_pairs > c->max_frames)
        return g_icp_err.set(YOUTH_EINVAL, "align_pairs: bad arguments %d", n_pairs);
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = pick_stream(c, stream);
    // targets -> records [0, n); sources are read straight from d_src
    const PrepJob job{d_dst, n_pairs, 0, true};
    bool exported = false;
    rc = run_iterations(c, s, d_src, 0, 0, n_pairs, T_init, d_T_out, &exported, &job);
    if (rc) return rc;
    return exported ? YOUTH_OK : export_poses(c, s, n_pairs, d_T_out, true);
}

int youth_icp_align_sequence_device(youth_icp_ctx* c, const int16_t* d_frames, int n_frames,
                                    float* d_T_out, void* stream)
{
    if (!c || !d_frames || n_frames < 2 || n_frames - 1 > c->max_frames)
        return g_icp_err.set(YOUTH_EINVAL, "align_sequence: bad arguments %d", n_frames);
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = pick_stream(c, stream);
    // every frame but the last is a target: one record set per frame, reused;
    // pair k: source depth frame k+1, target record frame k
    const PrepJob job{d_frames, n_frames - 1, 0, true};
    bool exported = false;
    rc = run_iterations(c, s, d_frames, 1, 0, n_frames - 1, nullptr, d_T_out, &exported,
                        &job);
    if (rc) return rc;
    return exported ? YOUTH_OK : export_poses(c, s, n_frames - 1, d_T_out, true);
}

int youth_icp_sync(youth_icp_ctx* c, void* stream)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "sync: null context");
    int rc = bind_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(pick_stream(c, stream)));
    return YOUTH_OK;
}

int youth_icp_get_poses(youth_icp_ctx* c, int n, double* T64, float* T32, int32_t* status)
{
    if (!c || n < 0 || n > c->max_frames)
        return g_icp_err.set(YOUTH_EINVAL, "get_poses: bad arguments %d", n);
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->last_stream ? c->last_stream : c->stream;
    if (T64)
        HIP_TRY(hipMemcpyAsync(T64, c->d_T64, (size_t)n * 16 * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    if (T32) {
        rc = export_poses(c, s, n, c->d_Tout, true);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(T32, c->d_Tout, (size_t)n * 16 * sizeof(float),
                               hipMemcpyDeviceToHost, s));
    }
    unsigned err = 0;
    if (status) {
        HIP_TRY(hipMemcpyAsync(status, c->d_status, (size_t)n * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        // a timed-out launch (either kernel path) marks every pair
        HIP_TRY(hipMemcpyAsync(&err, c->d_head + kQError, sizeof(unsigned),
                               hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (status && err)
        for (int i = 0; i < n; ++i) status[i] |= YOUTH_STATUS_TIMEOUT;
    return YOUTH_OK;
}

int youth_icp_get_stats(youth_icp_ctx* c, int n, int iters, double* count, double* sum_r2)
{
    if (!c || n < 0 || n > c->max_frames || iters != c->last_iters || iters > c->stats_iters)
        return g_icp_err.set(YOUTH_EINVAL, "get_stats: bad arguments %d", iters);
    int rc = bind_device(c);
    if (rc) return rc;
    std::vector<double> st((size_t)n * iters * 2);
    hipStream_t s = c->last_stream ? c->last_stream : c->stream;
    HIP_TRY(hipMemcpyAsync(st.data(), c->d_stats, st.size() * sizeof(double),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < (size_t)n * iters; ++i) {
        if (count) count[i] = st[2 * i];
        if (sum_r2) sum_r2[i] = st[2 * i + 1];
    }
    return YOUTH_OK;
}

int youth_icp_set_timing(youth_icp_ctx* c, int enable)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "set_timing: null context");
    int rc = bind_device(c);
    if (rc) return rc;
    rc = ev_harvest(c);
    if (rc) return rc;
    c->timing = enable != 0;
    c->timing_iter_only = enable == 2;
    for (int k = 0; k < 3; ++k) {
        c->t_ms[k] = 0.0;
        c->t_n[k] = 0;
    }
    return YOUTH_OK;
}

int youth_icp_selftest_projdiv(int device, long long n, unsigned long long seed,
                               long long* bit_mismatches, long long* proj_mismatches)
{
    if (n < 0) return g_icp_err.set(YOUTH_EINVAL, "selftest_projdiv: n < 0");
    const int ndev = youth_icp_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev)
        return g_icp_err.set(YOUTH_ENODEV, "selftest_projdiv: no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    unsigned long long* d_bad = nullptr;
    HIP_TRY(hipMalloc(&d_bad, 2 * sizeof(unsigned long long)));
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemset(d_bad, 0, sizeof(h));
    if (e == hipSuccess) e = launch_selftest(0, (unsigned long long)n, seed, d_bad);
    if (e == hipSuccess) e = hipMemcpy(h, d_bad, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return g_icp_err.set(YOUTH_EHIP, "selftest_projdiv: %s", hipGetErrorString(e));
    if (bit_mismatches) *bit_mismatches = (long long)h[0];
    if (proj_mismatches) *proj_mismatches = (long long)h[1];
    return YOUTH_OK;
}

int youth_icp_selftest_projquot(int device, long long n, unsigned long long seed,
                                long long* quot_mismatches, long long* proj_mismatches,
                                long long* floor_mismatches)
{
    if (n < 0) return g_icp_err.set(YOUTH_EINVAL, "selftest_projquot: n < 0");
    const int ndev = youth_icp_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev)
        return g_icp_err.set(YOUTH_ENODEV, "selftest_projquot: no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    unsigned long long* d_bad = nullptr;
    HIP_TRY(hipMalloc(&d_bad, 3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0, 0, 0};
    hipError_t e = hipMemset(d_bad, 0, sizeof(h));
    if (e == hipSuccess) e = launch_selftest(1, (unsigned long long)n, seed, d_bad);
    if (e == hipSuccess) e = hipMemcpy(h, d_bad, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return g_icp_err.set(YOUTH_EHIP, "selftest_projquot: %s", hipGetErrorString(e));
    if (quot_mismatches) *quot_mismatches = (long long)h[0];
    if (proj_mismatches) *proj_mismatches = (long long)h[1];
    if (floor_mismatches) *floor_mismatches = (long long)h[2];
    return YOUTH_OK;
}

int youth_icp_selftest_normalize(int device, long long n, unsigned long long seed,
                                 long long* sqrt_mismatches, long long* quot_mismatches,
                                 long long* fast_cases)
{
    if (n < 0) return g_icp_err.set(YOUTH_EINVAL, "selftest_normalize: n < 0");
    const int ndev = youth_icp_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev)
        return g_icp_err.set(YOUTH_ENODEV, "selftest_normalize: no HIP device %d", device);
    HIP_TRY(hipSetDevice(device));
    unsigned long long* d_bad = nullptr;
    HIP_TRY(hipMalloc(&d_bad, 3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0, 0, 0};
    hipError_t e = hipMemset(d_bad, 0, sizeof(h));
    if (e == hipSuccess) e = launch_selftest(2, (unsigned long long)n, seed, d_bad);
    if (e == hipSuccess) e = hipMemcpy(h, d_bad, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess)
        return g_icp_err.set(YOUTH_EHIP, "selftest_normalize: %s", hipGetErrorString(e));
    if (sqrt_mismatches) *sqrt_mismatches = (long long)h[0];
    if (quot_mismatches) *quot_mismatches = (long long)h[1];
    if (fast_cases) *fast_cases = (long long)h[2];
    return YOUTH_OK;
}

int youth_icp_get_sched_stats(youth_icp_ctx* c, unsigned* spins, unsigned* waited_items)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "get_sched_stats: null context");
    int rc = bind_device(c);
    if (rc) return rc;
    unsigned h[kQWords];
    HIP_TRY(hipMemcpyAsync(h, c->d_head, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (spins) *spins = h[kQSpins];
    if (waited_items) *waited_items = h[kQWaited];
    return YOUTH_OK;
}

int youth_icp_get_plan(youth_icp_ctx* c, int* workgroups_per_pair, int* px_per_lane)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "get_plan: null context");
    if (workgroups_per_pair) *workgroups_per_pair = c->last_coop ? c->last_coop_G : 0;
    if (px_per_lane) *px_per_lane = c->last_coop ? c->last_coop_px : 0;
    return c->last_coop ? 1 : c->persistent ? 0 : 2;
}

int youth_icp_get_first_iter(youth_icp_ctx* c)
{
    if (!c) return g_icp_err.set(YOUTH_EINVAL, "get_first_iter: null context");
    return c->last_first_form;
}

int youth_icp_get_timing(youth_icp_ctx* c, int kind, double* total_ms, int* launches)
{
    if (!c || kind < 0 || kind > 2) return g_icp_err.set(YOUTH_EINVAL, "get_timing: bad kind %d", kind);
    int rc = bind_device(c);
    if (rc) return rc;
    rc = ev_harvest(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->t_ms[kind];
    if (launches) *launches = c->t_n[kind];
    return YOUTH_OK;
}

int youth_icp_prepare_host(youth_icp_ctx* c, const int16_t* depth, int n_frames,
                           int want_normals, float* X, float* Y, float* Z, float* NX,
                           float* NY, float* NZ)
{
    if (!c || !depth || n_frames <= 0 || n_frames > c->max_frames)
        return g_icp_err.set(YOUTH_EINVAL, "prepare_host: bad arguments %d", n_frames);
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t N = c->N;
    HIP_TRY(hipMemcpyAsync(c->d_depth, depth, (size_t)n_frames * N * sizeof(int16_t),
                           hipMemcpyHostToDevice, s));
    // no X/Y/Z wanted: the align path's record kernel (k_prep without planes)
    rc = launch_prep(c, s, c->d_depth, n_frames, 0, X || Y || Z);
    if (rc) return rc;
    float* outs[6] = {X, Y, Z, NX, NY, NZ};
    for (int f = 0; f < n_frames; ++f)
        for (int k = 0; k < 6; ++k) {
            if (!outs[k] || (k >= 3 && !want_normals)) continue;
            float* dst = outs[k] + (size_t)f * N;
            if (k < 3) {
                const float* base = c->d_xyz + (size_t)f * 3 * c->P + (size_t)k * c->P;
                HIP_TRY(hipMemcpyAsync(dst, base, N * sizeof(float), hipMemcpyDeviceToHost, s));
            } else {  // component k-2 of the {z, nx, ny, nz} records
                const float* base = reinterpret_cast<const float*>(c->d_rec + (size_t)f * c->P) +
                                    (k - 2);
                HIP_TRY(hipMemcpy2DAsync(dst, sizeof(float), base, sizeof(float4), sizeof(float),
                                         N, hipMemcpyDeviceToHost, s));
            }
        }
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

int youth_icp_reduce_host(youth_icp_ctx* c, const int16_t* src, const int16_t* dst,
                          const float* T12, int32_t* assoc, double* neq)
{
    if (!c || !src || !dst || !T12) return g_icp_err.set(YOUTH_EINVAL, "reduce_host: bad arguments");
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t N = c->N;
    HIP_TRY(hipMemcpyAsync(c->d_depth, src, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_depth + N, dst, N * sizeof(int16_t), hipMemcpyHostToDevice, s));
    rc = launch_prep(c, s, c->d_depth + N, 1, 1, false);  // target -> record frame 1
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_T32, T12, 12 * sizeof(float), hipMemcpyHostToDevice, s));
    int nb = 0;
    rc = launch_reduce(c, s, c->d_depth, 0, 1, 1, assoc != nullptr, &nb);
    if (rc) return rc;
    rc = launch_solve_sums(c, s, nb);
    if (rc) return rc;
    if (neq)
        HIP_TRY(hipMemcpyAsync(neq, c->d_neq, kNeq * sizeof(double), hipMemcpyDeviceToHost, s));
    if (assoc)
        HIP_TRY(hipMemcpyAsync(assoc, c->d_assoc, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

int youth_icp_solve_host(youth_icp_ctx* c, const double* neq, double* T64)
{
    if (!c || !neq || !T64) return g_icp_err.set(YOUTH_EINVAL, "solve_host: bad arguments");
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->d_neq, neq, kNeq * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_T64, T64, 16 * sizeof(double), hipMemcpyHostToDevice, s));
    rc = launch_solve_neq(c, s);
    if (rc) return rc;
    int32_t st = 0;
    HIP_TRY(hipMemcpyAsync(T64, c->d_T64, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&st, c->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return st;
}

}  // extern "C"
