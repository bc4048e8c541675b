// Loop closing on gfx950 (C-ABI: include/youth_loop.h; definition: DESIGN.md
// §15): the frame signature and its distance as kernels, and the youth_loop
// object: keyframe store, retrieval and the RGB-D verification of candidates.
//
//   k_loop_signature  one workgroup of 256 threads per (cell row, frame): the
//                     H / 15 image rows of a cell row are one contiguous range
//                     of both planes, read once, 3 B/px.  A thread owns one
//                     16-pixel unit of a column position (two 16-byte depth
//                     loads, one 16-byte intensity load) and walks down the
//                     rows, so where a unit lies inside one cell (every unit
//                     when W / 20 is a multiple of 16, e.g. 640 and 1280) its
//                     sums stay in registers for the whole pass and reach LDS
//                     in one flush; a unit that straddles cells flushes at
//                     each change of cell.  LDS holds the 20 cells' integer
//                     sums (64-bit for depth: a cell may hold 896 K pixels of
//                     32767); 20 threads turn them into records.  No global
//                     atomics, nothing to zero, one launch.
//   k_loop_distance   one wave per (query, keyframe): 300 cells over 64 lanes,
//                     a shuffle reduction.
//
// Everything is integer, so a record is one bit pattern whatever the launch
// shape or the load width.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "hip_host.h"
#include "youth_loop.h"
#include "youth_rgbd.h"

namespace {

constexpr int kGX = YOUTH_LOOP_GX, kGY = YOUTH_LOOP_GY, kCells = YOUTH_LOOP_CELLS;
constexpr int kSigThreads = 256;
constexpr int kSigUnit = 16;   // pixels per thread and row

// the cell column of pixel column x: the i with floor(i W / GX) <= x < floor((i + 1) W / GX)
__device__ __forceinline__ int cell_of(int x, int W) { return ((x + 1) * kGX - 1) / W; }

struct CellAcc {
    int cell = -1;
    unsigned cnt = 0, sumY = 0;
    unsigned long long sumD = 0;
};

__device__ __forceinline__ void flush(CellAcc& a, unsigned* s_cnt, unsigned* s_sumY,
                                      unsigned long long* s_sumD)
{
    if (a.cell >= 0) {
        atomicAdd(&s_cnt[a.cell], a.cnt);
        atomicAdd(&s_sumY[a.cell], a.sumY);
        atomicAdd(&s_sumD[a.cell], a.sumD);
    }
    a.cnt = 0;
    a.sumY = 0;
    a.sumD = 0;
}

// kVec: W % 16 == 0 and both planes 16-byte aligned, so every unit lies in one
// row and moves as three 16-byte words.
template <bool kVec>
__global__ __launch_bounds__(kSigThreads) void k_loop_signature(const int16_t* __restrict__ depth,
                                                                const uint8_t* __restrict__ gray,
                                                                int W, int H,
                                                                uint32_t* __restrict__ sig)
{
    __shared__ unsigned long long s_sumD[kGX];
    __shared__ unsigned s_cnt[kGX], s_sumY[kGX];
    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    const size_t frame = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const int16_t* __restrict__ dp = depth + frame;
    const uint8_t* __restrict__ gp = gray + frame;
    const int y0 = j * H / kGY, y1 = (j + 1) * H / kGY;
    if (tid < kGX) {
        s_sumD[tid] = 0;
        s_cnt[tid] = 0;
        s_sumY[tid] = 0;
    }
    __syncthreads();

    // units per row; a row narrower than the workgroup leaves room for R rows
    // per pass, a wider one is walked in column steps of the workgroup
    const int upr = (W + kSigUnit - 1) / kSigUnit;
    const int R = upr <= kSigThreads ? kSigThreads / upr : 1;
    const int r = tid / upr, c0 = tid - r * upr;
    const int cstep = upr <= kSigThreads ? upr : kSigThreads;
    CellAcc acc;
    if (r < R) {
        for (int c = c0; c < upr; c += cstep) {
            const int x0 = c * kSigUnit;
            const int xl = min(x0 + kSigUnit, W) - 1;   // the unit's last pixel inside the row
            const int ci0 = cell_of(x0, W);
            const bool single = cell_of(xl, W) == ci0;
            if (ci0 != acc.cell) {
                flush(acc, s_cnt, s_sumY, s_sumD);
                acc.cell = ci0;
            }
            for (int y = y0 + r; y < y1; y += R) {
                const size_t at = (size_t)y * W + x0;
                int d[kSigUnit];
                unsigned g4[kSigUnit / 4];   // 4 intensities per word, pixel p in byte p % 4
                if (kVec) {
                    const uint4 da = *reinterpret_cast<const uint4*>(dp + at);
                    const uint4 db = *reinterpret_cast<const uint4*>(dp + at + 8);
                    const uint4 ga = *reinterpret_cast<const uint4*>(gp + at);
                    const unsigned dw[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        d[2 * k] = (int)(dw[k] << 16) >> 16;
                        d[2 * k + 1] = (int)dw[k] >> 16;
                    }
                    g4[0] = ga.x, g4[1] = ga.y, g4[2] = ga.z, g4[3] = ga.w;
                } else {
#pragma unroll
                    for (int k = 0; k < kSigUnit / 4; ++k) g4[k] = 0;
#pragma unroll
                    for (int p = 0; p < kSigUnit; ++p) {
                        const bool in = x0 + p < W;
                        d[p] = in ? (int)dp[at + p] : 0;
                        g4[p / 4] |= (in ? (unsigned)gp[at + p] : 0u) << (8 * (p % 4));
                    }
                }
                if (single) {
                    unsigned sd = 0;
#pragma unroll
                    for (int p = 0; p < kSigUnit; ++p) {
                        const bool v = d[p] > 0;
                        acc.cnt += v ? 1u : 0u;
                        sd += v ? (unsigned)d[p] : 0u;
                    }
#pragma unroll
                    for (int k = 0; k < kSigUnit / 4; ++k)
                        acc.sumY = __builtin_amdgcn_sad_u8(g4[k], 0u, acc.sumY);   // + its 4 bytes
                    acc.sumD += sd;   // 16 * 32767 fits 32 bits
                } else {
                    // the unit crosses cell borders: a pixel at a time, the
                    // sums flushed at every change of cell
                    int cell = ci0, nb = (ci0 + 1) * W / kGX;
#pragma unroll
                    for (int p = 0; p < kSigUnit; ++p) {   // unrolled: d and g4 stay in registers
                        if (x0 + p >= W) break;
                        if (x0 + p >= nb) {   // cells are at least one pixel wide
                            ++cell;
                            nb = (cell + 1) * W / kGX;
                        }
                        if (cell != acc.cell) {
                            flush(acc, s_cnt, s_sumY, s_sumD);
                            acc.cell = cell;
                        }
                        const bool v = d[p] > 0;
                        acc.cnt += v ? 1u : 0u;
                        acc.sumD += v ? (unsigned)d[p] : 0u;
                        acc.sumY += (g4[p / 4] >> (8 * (p % 4))) & 255u;
                    }
                }
            }
        }
    }
    flush(acc, s_cnt, s_sumY, s_sumD);
    __syncthreads();
    if (tid < kGX) {
        const unsigned n = (unsigned)(((tid + 1) * W / kGX - tid * W / kGX) * (y1 - y0));   // <= 896 K
        const unsigned cnt = s_cnt[tid];
        const bool valid = cnt > 0 && 4u * cnt >= n;
        const unsigned dm = valid ? (unsigned)((s_sumD[tid] + cnt / 2) / cnt) : 0u;
        const unsigned ym = (s_sumY[tid] + n / 2) / n;
        sig[((size_t)blockIdx.y * kGY + j) * kGX + tid] = dm | (ym << 16) | (valid ? 0x80000000u : 0u);
    }
}

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

__global__ __launch_bounds__(64) void k_loop_distance(const uint32_t* __restrict__ sig_q,
                                                      const uint32_t* __restrict__ sig_k, int n,
                                                      unsigned cap, unsigned ly,
                                                      uint32_t* __restrict__ D)
{
    const int k = blockIdx.x, q = blockIdx.y, lane = threadIdx.x;
    const uint32_t* a = sig_q + (size_t)q * kCells;
    const uint32_t* b = sig_k + (size_t)k * kCells;
    unsigned s = 0;
    for (int c = lane; c < kCells; c += 64) {
        const unsigned ra = a[c], rb = b[c];
        const unsigned va = ra >> 31, vb = rb >> 31;
        const unsigned dd = min(absdiff(ra & 0xffffu, rb & 0xffffu), cap);
        s += (va & vb) ? dd : (va ^ vb) ? cap : 0u;
        s += ly * absdiff((ra >> 16) & 255u, (rb >> 16) & 255u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) D[(size_t)q * n + k] = s;
}

}  // namespace

// =============================================================== host side ==

// The loop closer's channel (hip_host.h): youth_loop_last_error reads it.
static thread_local youth::ErrorText g_loop_err;
#define HIP_ERR g_loop_err

static int launch_signature(const int16_t* d_depth, const uint8_t* d_gray, int n, int W, int H,
                            uint32_t* d_sig, hipStream_t s)
{
    const bool vec = W % 16 == 0 && (((uintptr_t)d_depth | (uintptr_t)d_gray) & 15) == 0;
    hipLaunchKernelGGL(vec ? k_loop_signature<true> : k_loop_signature<false>, dim3(kGY, n),
                       dim3(kSigThreads), 0, s, d_depth, d_gray, W, H, d_sig);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

static int launch_distance(const uint32_t* d_q, int nq, const uint32_t* d_k, int n,
                           const youth_loop_params& P, uint32_t* d_D, hipStream_t s)
{
    hipLaunchKernelGGL(k_loop_distance, dim3(n, nq), dim3(64), 0, s, d_q, d_k, n, (unsigned)P.cap,
                       (unsigned)P.ly, d_D);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

struct youth_loop {
    int device = 0, W = 0, H = 0, max_kf = 0;
    size_t N = 0;
    youth_loop_params prm;
    youth_rgbd_params rp;
    youth_rgbd_ctx* rgbd = nullptr;
    hipStream_t stream = nullptr;
    // the store, [max_kf] each
    int16_t* d_depth = nullptr;
    uint8_t* d_gray = nullptr;
    uint32_t* d_sig = nullptr;
    // the verification batch, [2 max_candidates] pairs: source and target planes
    int16_t *b_sd = nullptr, *b_dd = nullptr;
    uint8_t *b_sg = nullptr, *b_dg = nullptr;
    uint8_t* d_rgb = nullptr;    // one host keyframe's colour on its way to intensity
    uint32_t* d_q = nullptr;     // query records of youth_loop_distances
    int q_cap = 0;
    uint32_t* d_D = nullptr;     // distances, [q_cap or 1][max_kf]
    int D_cap = 0;
    struct Kf {
        double T[16];
        uint32_t tag;
    };
    std::vector<Kf> kfs;
    std::vector<youth_loop_edge> edges, verified;
};

static int loop_bind(youth_loop* lp)
{
    HIP_TRY(hipSetDevice(lp->device));
    return YOUTH_OK;
}

static int params_check(const char* who, const youth_loop_params& P)
{
    if (P.min_gap < 1 || P.max_candidates < 1 || P.max_candidates > YOUTH_LOOP_MAX_CANDIDATES ||
        P.cap > 65535u || P.ly > 64u || P.max_cell_dist > 65535u + 64u * 255u ||
        !std::isfinite(P.min_overlap) || !std::isfinite(P.max_gray_rms) || !std::isfinite(P.fb_rot_deg) ||
        !std::isfinite(P.fb_trans_m) || P.min_overlap < 0.0f || P.max_gray_rms < 0.0f ||
        P.fb_rot_deg < 0.0f || P.fb_trans_m < 0.0f)
        return g_loop_err.set(YOUTH_EINVAL,
                              "%s: bad parameters (need min_gap >= 1, 1 <= max_candidates <= %d, cap <= "
                              "65535, ly <= 64, finite gates >= 0)",
                              who, YOUTH_LOOP_MAX_CANDIDATES);
    return YOUTH_OK;
}

static bool finite16(const double* T)
{
    for (int a = 0; a < 16; ++a)
        if (!std::isfinite(T[a])) return false;
    return true;
}

static int add_check(const char* who, youth_loop* lp, const void* a, const void* b, const double* T)
{
    if (!lp || !a || !b || !T) return g_loop_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if (!finite16(T)) return g_loop_err.set(YOUTH_EINVAL, "%s: the pose is not finite", who);
    if ((int)lp->kfs.size() >= lp->max_kf)
        return g_loop_err.set(YOUTH_EINVAL, "%s: the store is full (%d keyframes)", who, lp->max_kf);
    return loop_bind(lp);
}

// the stored planes of slot `at` are in place: its record, then the bookkeeping
static int add_finish(youth_loop* lp, int at, const double* T, uint32_t tag)
{
    int rc = launch_signature(lp->d_depth + (size_t)at * lp->N, lp->d_gray + (size_t)at * lp->N, 1, lp->W,
                              lp->H, lp->d_sig + (size_t)at * kCells, lp->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(lp->stream));
    youth_loop::Kf kf;
    memcpy(kf.T, T, sizeof(kf.T));
    kf.T[12] = kf.T[13] = kf.T[14] = 0.0;
    kf.T[15] = 1.0;
    kf.tag = tag;
    lp->kfs.push_back(kf);
    return at;
}

// D of query record(s) on the device against the first n stored keyframes -> host
static int distances_to_host(youth_loop* lp, const uint32_t* d_q, int nq, int n, uint32_t* D)
{
    int rc = youth::grow_device_buffer(g_loop_err, &lp->d_D, &lp->D_cap, nq, (size_t)lp->max_kf);
    if (rc) return rc;
    rc = launch_distance(d_q, nq, lp->d_sig, n, lp->prm, lp->d_D, lp->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(D, lp->d_D, (size_t)nq * n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           lp->stream));
    HIP_TRY(hipStreamSynchronize(lp->stream));
    return YOUTH_OK;
}

static void mat_mul4(const double* A, const double* B, double* C)
{
    double O[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
            O[i * 4 + j] = s;
        }
    memcpy(C, O, sizeof(O));
}

extern "C" {

const char* youth_loop_last_error(void) { return g_loop_err.c_str(); }

youth_loop_params youth_loop_default_params(void)
{
    youth_loop_params p;
    p.min_gap = 10;
    p.max_candidates = 4;
    p.max_cell_dist = 400;
    p.cap = 1000;
    p.ly = 4;
    p.min_overlap = 0.10f;
    // between the largest value over accurate pairs (1.13) and the smallest
    // over wrong ones (2.10) measured at 640x480
    p.max_gray_rms = 1.5f;
    p.fb_rot_deg = 0.5f;
    p.fb_trans_m = 0.010f;
    return p;
}

int youth_loop_signature_device(int device, const int16_t* d_depth, const uint8_t* d_gray, int n, int W,
                                int H, uint32_t* d_sig, void* stream)
{
    static const char* who = "youth_loop_signature_device";
    if (!d_depth || !d_gray || !d_sig) return g_loop_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (n < 0 || n > youth::kMaxFrames || W < kGX || H < kGY || !youth::frame_size_ok(W, H, 3))
        return g_loop_err.set(YOUTH_EINVAL,
                              "%s: %d frames of %dx%d (need 0 <= frames <= 65535, 20 <= W <= 16384, 15 <= H "
                              "<= 16384, W*H <= 2^26)",
                              who, n, W, H);
    int rc = youth::check_device(g_loop_err, who, device);
    if (rc) return rc;
    if (n == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(device));
    return launch_signature(d_depth, d_gray, n, W, H, d_sig, (hipStream_t)stream);
}

void youth_loop_destroy(youth_loop* lp)
{
    if (!lp) return;
    if (hipSetDevice(lp->device) == hipSuccess) {
        if (lp->stream) (void)hipStreamSynchronize(lp->stream);
        youth_rgbd_destroy(lp->rgbd);
        void* bufs[] = {lp->d_depth, lp->d_gray, lp->d_sig, lp->b_sd, lp->b_dd, lp->b_sg,
                        lp->b_dg,    lp->d_rgb,  lp->d_q,   lp->d_D};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (lp->stream) (void)hipStreamDestroy(lp->stream);
    }
    delete lp;
}

youth_loop* youth_loop_create(int device, int W, int H, int max_keyframes, const youth_intrinsics* K,
                              const youth_loop_params* params)
{
    static const char* who = "youth_loop_create";
    const youth_loop_params P = params ? *params : youth_loop_default_params();
    if (params_check(who, P)) return nullptr;
    if (W < kGX || H < kGY || !youth::frame_size_ok(W, H, 3) || max_keyframes < 2 ||
        max_keyframes > YOUTH_LOOP_MAX_KEYFRAMES) {
        g_loop_err.set(YOUTH_EINVAL,
                       "%s: %dx%d, %d keyframes (need 20 <= W <= 16384, 15 <= H <= 16384, W*H <= 2^26, 2 <= "
                       "keyframes <= %d)",
                       who, W, H, max_keyframes, YOUTH_LOOP_MAX_KEYFRAMES);
        return nullptr;
    }
    if (youth::check_device(g_loop_err, who, device)) return nullptr;
    youth_loop* lp = new (std::nothrow) youth_loop();
    if (!lp) {
        g_loop_err.set(YOUTH_ENOMEM, "%s: allocation failed", who);
        return nullptr;
    }
    lp->device = device;
    lp->W = W;
    lp->H = H;
    lp->N = (size_t)W * H;
    lp->max_kf = max_keyframes;
    lp->prm = P;
    lp->rp = youth_rgbd_default_params();
    const size_t N = lp->N, F = (size_t)max_keyframes, B = 2 * (size_t)P.max_candidates;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&lp->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&lp->d_depth, F * N * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc(&lp->d_gray, F * N);
    if (e == hipSuccess) e = hipMalloc(&lp->d_sig, F * kCells * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&lp->b_sd, B * N * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc(&lp->b_dd, B * N * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc(&lp->b_sg, B * N);
    if (e == hipSuccess) e = hipMalloc(&lp->b_dg, B * N);
    if (e == hipSuccess) e = hipMalloc(&lp->d_rgb, 3 * N);
    if (e != hipSuccess) {
        g_loop_err.set(e == hipErrorOutOfMemory ? YOUTH_ENOMEM : YOUTH_EHIP, "%s: %s%s", who,
                       e == hipErrorOutOfMemory ? "allocation failed: " : "", hipGetErrorString(e));
        youth_loop_destroy(lp);
        return nullptr;
    }
    lp->rgbd = youth_rgbd_create(device, W, H, (int)B, K, &lp->rp);
    if (!lp->rgbd) {
        g_loop_err.set(YOUTH_EINVAL, "%s: %s", who, youth_rgbd_last_error());
        youth_loop_destroy(lp);
        return nullptr;
    }
    return lp;
}

int youth_loop_set_levels(youth_loop* lp, const youth_rgbd_level* levels, int n)
{
    static const char* who = "youth_loop_set_levels";
    if (!lp) return g_loop_err.set(YOUTH_EINVAL, "%s: null object", who);
    if (n > 0 && !levels) return g_loop_err.set(YOUTH_EINVAL, "%s: null levels", who);
    if (n > 0 && n <= YOUTH_RGBD_MAX_LEVELS && (levels[n - 1].stride != 1 || levels[n - 1].iters < 1))
        return g_loop_err.set(YOUTH_EINVAL,
                              "%s: the last level is %d:%d (the gates need stride 1 and an iteration)",
                              who, levels[n - 1].stride, levels[n - 1].iters);
    int rc = loop_bind(lp);
    if (rc) return rc;
    rc = youth_rgbd_set_levels(lp->rgbd, levels, n);
    if (rc < 0) return g_loop_err.set(rc, "%s: %s", who, youth_rgbd_last_error());
    return YOUTH_OK;
}

int youth_loop_get_levels(const youth_loop* lp, youth_rgbd_level* out, int cap)
{
    if (!lp || cap < 0 || (cap > 0 && !out))
        return g_loop_err.set(YOUTH_EINVAL, "youth_loop_get_levels: bad arguments");
    return youth_rgbd_get_levels(lp->rgbd, out, cap);
}

int youth_loop_keyframes(const youth_loop* lp) { return lp ? (int)lp->kfs.size() : 0; }

int youth_loop_clear(youth_loop* lp)
{
    if (!lp) return g_loop_err.set(YOUTH_EINVAL, "youth_loop_clear: null object");
    lp->kfs.clear();
    lp->edges.clear();
    lp->verified.clear();
    return YOUTH_OK;
}

int youth_loop_get_keyframe(const youth_loop* lp, int kf, double T_wc[16], uint32_t* tag)
{
    if (!lp || kf < 0 || kf >= (int)lp->kfs.size())
        return g_loop_err.set(YOUTH_EINVAL, "youth_loop_get_keyframe: keyframe %d of %d", kf,
                              lp ? (int)lp->kfs.size() : 0);
    if (T_wc) memcpy(T_wc, lp->kfs[kf].T, 16 * sizeof(double));
    if (tag) *tag = lp->kfs[kf].tag;
    return YOUTH_OK;
}

int youth_loop_edges(youth_loop* lp, youth_loop_edge* out, int cap)
{
    if (!lp || cap < 0 || (cap > 0 && !out))
        return g_loop_err.set(YOUTH_EINVAL, "youth_loop_edges: bad arguments");
    const int m = std::min(cap, (int)lp->edges.size());
    for (int k = 0; k < m; ++k) out[k] = lp->edges[k];
    return (int)lp->edges.size();
}

int youth_loop_last_verified(const youth_loop* lp, youth_loop_edge* out, int cap)
{
    if (!lp || cap < 0 || (cap > 0 && !out))
        return g_loop_err.set(YOUTH_EINVAL, "youth_loop_last_verified: bad arguments");
    const int m = std::min(cap, (int)lp->verified.size());
    for (int k = 0; k < m; ++k) out[k] = lp->verified[k];
    return m;
}

int youth_loop_add_keyframe_device(youth_loop* lp, const int16_t* d_depth, const uint8_t* d_gray,
                                   const double T_wc[16], uint32_t tag)
{
    int rc = add_check("youth_loop_add_keyframe_device", lp, d_depth, d_gray, T_wc);
    if (rc) return rc;
    const int at = (int)lp->kfs.size();
    HIP_TRY(hipMemcpyAsync(lp->d_depth + (size_t)at * lp->N, d_depth, lp->N * sizeof(int16_t),
                           hipMemcpyDeviceToDevice, lp->stream));
    HIP_TRY(hipMemcpyAsync(lp->d_gray + (size_t)at * lp->N, d_gray, lp->N, hipMemcpyDeviceToDevice,
                           lp->stream));
    return add_finish(lp, at, T_wc, tag);
}

int youth_loop_add_keyframe_host(youth_loop* lp, const int16_t* depth, const uint8_t* rgb,
                                 const double T_wc[16], uint32_t tag)
{
    int rc = add_check("youth_loop_add_keyframe_host", lp, depth, rgb, T_wc);
    if (rc) return rc;
    const int at = (int)lp->kfs.size();
    HIP_TRY(hipMemcpyAsync(lp->d_depth + (size_t)at * lp->N, depth, lp->N * sizeof(int16_t),
                           hipMemcpyHostToDevice, lp->stream));
    HIP_TRY(hipMemcpyAsync(lp->d_rgb, rgb, 3 * lp->N, hipMemcpyHostToDevice, lp->stream));
    if (youth_rgbd_luma_device(lp->device, lp->d_rgb, lp->d_gray + (size_t)at * lp->N, 1, lp->W, lp->H,
                               lp->stream) < 0)
        return g_loop_err.set(YOUTH_EHIP, "youth_loop_add_keyframe_host: %s", youth_rgbd_last_error());
    return add_finish(lp, at, T_wc, tag);
}

int youth_loop_distances(youth_loop* lp, const uint32_t* sig_q, int nq, uint32_t* D)
{
    static const char* who = "youth_loop_distances";
    if (!lp || !sig_q || !D || nq < 0 || nq > youth::kMaxFrames)
        return g_loop_err.set(YOUTH_EINVAL, "%s: bad arguments (%d queries)", who, nq);
    const int n = (int)lp->kfs.size();
    if (nq == 0 || n == 0) return n;
    int rc = loop_bind(lp);
    if (rc) return rc;
    rc = youth::grow_device_buffer(g_loop_err, &lp->d_q, &lp->q_cap, nq, (size_t)kCells);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(lp->d_q, sig_q, (size_t)nq * kCells * sizeof(uint32_t), hipMemcpyHostToDevice,
                           lp->stream));
    rc = distances_to_host(lp, lp->d_q, nq, n, D);
    return rc ? rc : n;
}

int youth_loop_candidates(youth_loop* lp, int kf, int k, int* idx, uint32_t* dist)
{
    static const char* who = "youth_loop_candidates";
    if (!lp || kf < 0 || kf >= (int)lp->kfs.size() || k < 0)
        return g_loop_err.set(YOUTH_EINVAL, "%s: keyframe %d of %d", who, kf, lp ? (int)lp->kfs.size() : 0);
    const int n = kf - lp->prm.min_gap + 1;   // keyframes 0 .. kf - min_gap
    if (n <= 0) return 0;
    int rc = loop_bind(lp);
    if (rc) return rc;
    std::vector<uint32_t> D((size_t)n);
    rc = distances_to_host(lp, lp->d_sig + (size_t)kf * kCells, 1, n, D.data());
    if (rc) return rc;
    std::vector<int> order;
    const uint32_t limit = lp->prm.max_cell_dist * (uint32_t)kCells;
    for (int c = 0; c < n; ++c)
        if (D[c] <= limit) order.push_back(c);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return D[a] < D[b]; });
    const int m = std::min({(int)order.size(), k, lp->prm.max_candidates});
    for (int c = 0; c < m; ++c) {
        if (idx) idx[c] = order[c];
        if (dist) dist[c] = D[order[c]];
    }
    return m;
}

int youth_loop_close(youth_loop* lp, int kf)
{
    static const char* who = "youth_loop_close";
    if (!lp) return g_loop_err.set(YOUTH_EINVAL, "%s: null object", who);
    int cand[YOUTH_LOOP_MAX_CANDIDATES];
    const int K = youth_loop_candidates(lp, kf, lp->prm.max_candidates, cand, nullptr);
    if (K < 0) return K;
    lp->verified.clear();
    if (K == 0) return 0;
    const size_t N = lp->N;
    // pair p < K: source kf, target cand[p]; pair K + p: the other way round
    for (int p = 0; p < 2 * K; ++p) {
        const int src = p < K ? kf : cand[p - K], dst = p < K ? cand[p] : kf;
        HIP_TRY(hipMemcpyAsync(lp->b_sd + p * N, lp->d_depth + src * N, N * sizeof(int16_t),
                               hipMemcpyDeviceToDevice, lp->stream));
        HIP_TRY(hipMemcpyAsync(lp->b_dd + p * N, lp->d_depth + dst * N, N * sizeof(int16_t),
                               hipMemcpyDeviceToDevice, lp->stream));
        HIP_TRY(hipMemcpyAsync(lp->b_sg + p * N, lp->d_gray + src * N, N, hipMemcpyDeviceToDevice,
                               lp->stream));
        HIP_TRY(hipMemcpyAsync(lp->b_dg + p * N, lp->d_gray + dst * N, N, hipMemcpyDeviceToDevice,
                               lp->stream));
    }
    // the gates read the last level's statistics where a schedule is set
    youth_rgbd_level lv[YOUTH_RGBD_MAX_LEVELS];
    const int n_lv = youth_rgbd_get_levels(lp->rgbd, lv, YOUTH_RGBD_MAX_LEVELS);
    const int iters = n_lv > 0 ? lv[n_lv - 1].iters : lp->rp.iters;
    double T[2 * YOUTH_LOOP_MAX_CANDIDATES][16];
    int32_t st[2 * YOUTH_LOOP_MAX_CANDIDATES];
    std::vector<double> stats((size_t)2 * K * iters * 4);
    if (youth_rgbd_align_pairs_device(lp->rgbd, lp->b_sd, lp->b_sg, lp->b_dd, lp->b_dg, 2 * K, nullptr,
                                      nullptr, lp->stream) < 0 ||
        youth_rgbd_get_poses(lp->rgbd, 2 * K, &T[0][0], nullptr, st) < 0 ||
        youth_rgbd_get_stats(lp->rgbd, 2 * K, iters, stats.data()) < 0)
        return g_loop_err.set(YOUTH_EHIP, "%s: %s", who, youth_rgbd_last_error());
    const double area = (double)N;
    int added = 0;
    for (int p = 0; p < K; ++p) {
        youth_loop_edge e;
        memset(&e, 0, sizeof(e));
        e.i = cand[p];
        e.j = kf;
        double rms[2], ov[2];
        for (int d = 0; d < 2; ++d) {
            double* Td = T[p + d * K];
            Td[12] = Td[13] = Td[14] = 0.0;
            Td[15] = 1.0;
            const double* s = stats.data() + ((size_t)(p + d * K) * iters + (iters - 1)) * 4;
            ov[d] = s[1] / area;
            rms[d] = s[3] > 0.0 ? (255.0 / (double)lp->rp.lambda) * sqrt(s[2] / s[3]) : INFINITY;
        }
        memcpy(e.Z, T[p], sizeof(e.Z));
        double E[16];
        mat_mul4(T[p], T[p + K], E);
        const double vx = 0.5 * (E[9] - E[6]), vy = 0.5 * (E[2] - E[8]), vz = 0.5 * (E[4] - E[1]);
        e.fb_rot_deg = atan2(sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (E[0] + E[5] + E[10] - 1.0)) *
                       (180.0 / M_PI);
        e.fb_trans_m = sqrt(E[3] * E[3] + E[7] * E[7] + E[11] * E[11]);
        e.overlap = std::min(ov[0], ov[1]);
        e.gray_rms = std::max(rms[0], rms[1]);
        const bool ok = st[p] == 0 && st[p + K] == 0 && finite16(T[p]) && finite16(T[p + K]) &&
                        e.overlap >= (double)lp->prm.min_overlap &&
                        e.gray_rms <= (double)lp->prm.max_gray_rms &&
                        e.fb_rot_deg <= (double)lp->prm.fb_rot_deg &&
                        e.fb_trans_m <= (double)lp->prm.fb_trans_m;
        e.w = ok ? 1.0 : 0.0;
        lp->verified.push_back(e);
        if (ok) {
            lp->edges.push_back(e);
            ++added;
        }
    }
    return added;
}

}  // extern "C"
