// Edge-preserving depth filter on gfx950 (C-ABI: include/youth_filter.h;
// definition: DESIGN.md §11).
//
// A 5x5 joint filter on the raw int16 depth whose range gate widens with the
// square of the depth, as the sensor's noise does.  Everything is integer, so
// the output is one bit pattern whatever the launch shape.
//
//   k_depth_filter   one 64 x 16 output tile per workgroup of 256 threads.
//                    The tile and its halo (2 rows above and below, 4 columns
//                    left and right so that the 8-byte words stay aligned) are
//                    staged in LDS as int16, 2880 bytes.  A cell that cannot
//                    contribute (outside the frame, or depth <= 0) is staged
//                    as kFar, a depth further than the widest gate from every
//                    valid centre, so the tap loop needs neither a bounds nor
//                    a validity test: the range gate rejects it.  Each thread
//                    then produces 4 consecutive pixels of one row from 5 LDS
//                    rows of 3 8-byte reads.
//
// Per tap: delta, delta^2 (24-bit multiply), T^2 - delta^2, clamp at 0 (the
// gate), the weight (a shift), den += w, s += w * delta (24-bit
// multiply-add): 7 integer lane-ops, ~190 per pixel with the quotient.
// num = s + T * den restates the definition's sum of w * (delta + T).  One
// division per pixel: a float reciprocal (the quotient is < 512, so the
// estimate is within 1 of it) and an integer correction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.h"
#include "youth_filter.h"

namespace {

constexpr int kFltThreads = 256;
constexpr int kFltTW = 64, kFltTH = 16;          // output tile
constexpr int kFltPadX = 4, kFltPadY = 2;        // staged halo
constexpr int kFltLW = kFltTW + 2 * kFltPadX;    // 72 int16 per LDS row (144 B)
constexpr int kFltLH = kFltTH + 2 * kFltPadY;    // 20 LDS rows
// A non-contributing cell.  Against a centre c in [1, 32767] its delta lies in
// [-33767, -1001]: beyond the widest gate (255), inside 24 bits, and its
// square inside 31.
constexpr int kFar = -1000;

__device__ __forceinline__ int16_t flt_cell(int16_t d) { return d > 0 ? d : (int16_t)kFar; }

// kVec: W % 4 == 0 and both frame bases 8-byte aligned, so every aligned group
// of 4 pixels lies inside one row and moves as one 8-byte word.
template <bool kVec>
__global__ __launch_bounds__(kFltThreads) void k_depth_filter(const int16_t* __restrict__ in,
                                                              int16_t* __restrict__ out, int W,
                                                              int H, int tiles_x, unsigned t0,
                                                              unsigned t2)
{
    __shared__ __attribute__((aligned(16))) int16_t tile[kFltLH][kFltLW];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const size_t frame = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const int16_t* __restrict__ src = in + frame;
    int16_t* __restrict__ dst = out + frame;
    const int x0 = bx * kFltTW, y0 = by * kFltTH;

    // this thread's 4 pixels, and their raw centres (an invalid one is copied)
    const int tx = tid & 15, ty = tid >> 4;
    const int px = x0 + 4 * tx, py = y0 + ty;
    const bool row_in = py < H && px < W;
    short4 raw = {0, 0, 0, 0};
    if (row_in) {
        const int16_t* p = src + (size_t)py * W + px;
        if (kVec) {
            raw = *reinterpret_cast<const short4*>(p);
        } else {
            raw.x = p[0];
            if (px + 1 < W) raw.y = p[1];
            if (px + 2 < W) raw.z = p[2];
            if (px + 3 < W) raw.w = p[3];
        }
    }

    if (kVec) {
        constexpr int kWords = kFltLW / 4;   // 18 8-byte words per LDS row
        for (int i = tid; i < kFltLH * kWords; i += kFltThreads) {
            const int ly = i / kWords, lw = i - ly * kWords;
            const int gy = y0 - kFltPadY + ly, gx = x0 - kFltPadX + 4 * lw;
            short4 v = {(short)kFar, (short)kFar, (short)kFar, (short)kFar};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {   // gx % 4 == 0: gx + 3 < W too
                const short4 d = *reinterpret_cast<const short4*>(src + (size_t)gy * W + gx);
                v.x = flt_cell(d.x);
                v.y = flt_cell(d.y);
                v.z = flt_cell(d.z);
                v.w = flt_cell(d.w);
            }
            *reinterpret_cast<short4*>(&tile[ly][4 * lw]) = v;
        }
    } else {
        for (int i = tid; i < kFltLH * kFltLW; i += kFltThreads) {
            const int ly = i / kFltLW, lx = i - ly * kFltLW;
            const int gy = y0 - kFltPadY + ly, gx = x0 - kFltPadX + lx;
            int16_t v = (int16_t)kFar;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = flt_cell(src[(size_t)gy * W + gx]);
            tile[ly][lx] = v;
        }
    }
    __syncthreads();
    if (!row_in) return;

    const int rawv[4] = {raw.x, raw.y, raw.z, raw.w};
    int c[4], T[4], TT[4], s[4];
    unsigned den[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = rawv[j] > 0 ? rawv[j] : 1;   // an invalid centre computes on, unused
        const unsigned h = (unsigned)c[j] >> 4;
        const unsigned g = t0 + (__umul24(__umul24(h, h), t2) >> 16);
        T[j] = (int)(g < 255u ? g : 255u);
        TT[j] = __mul24(T[j], T[j]);
        s[j] = 0;
        den[j] = 0;
    }
    constexpr int ws[5] = {1, 2, 4, 2, 1};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        // LDS columns 4 tx .. 4 tx + 11; pixel j's taps are columns 4 tx + 2 + j + k
        const short4* p = reinterpret_cast<const short4*>(&tile[ty + r][4 * tx]);
        const short4 a = p[0], b = p[1], e = p[2];
        const int v[8] = {a.z, a.w, b.x, b.y, b.z, b.w, e.x, e.y};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int dl = v[j + k] - c[j];
                int q = TT[j] - __mul24(dl, dl);
                q = q > 0 ? q : 0;                          // |dl| < T, else no weight
                const int w = q * (ws[r] * ws[k]);          // a shift; < 2^20
                den[j] += (unsigned)w;
                s[j] += __mul24(w, dl);                     // |sum| <= 100 * 255^2 * 255 < 2^31
            }
        }
    }
    int16_t res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // a valid centre's own tap gives den >= 16 T^2; an invalid centre may see 0
        const unsigned d = den[j] ? den[j] : 1u;
        const unsigned num = (unsigned)s[j] + __umul24((unsigned)T[j], d);   // d < 2^23
        const unsigned n = num + (d >> 1);
        unsigned qt = (unsigned)((float)n * __builtin_amdgcn_rcpf((float)d));
        const int rem = (int)(n - __umul24(qt, d));         // in (-d, 2 d)
        if (rem < 0) --qt;
        else if ((unsigned)rem >= d) ++qt;
        res[j] = rawv[j] > 0 ? (int16_t)(c[j] - T[j] + (int)qt) : (int16_t)rawv[j];
    }
    int16_t* o = dst + (size_t)py * W + px;
    if (kVec) {
        *reinterpret_cast<short4*>(o) = short4{res[0], res[1], res[2], res[3]};
    } else {
        o[0] = res[0];
        if (px + 1 < W) o[1] = res[1];
        if (px + 2 < W) o[2] = res[2];
        if (px + 3 < W) o[3] = res[3];
    }
}

}  // namespace

// =============================================================== host side ==

// The depth filter's channel (hip_host.h): youth_depth_filter_last_error reads it.
static thread_local youth::ErrorText g_filter_err;
#define HIP_ERR g_filter_err

static int filter_check(const char* who, const void* in, const void* out, int n_frames, int W,
                        int H, const youth_filter_params* P, bool may_alias)
{
    if (!in || !out) return g_filter_err.set(YOUTH_EINVAL, "%s: null buffer", who);
    if (n_frames < 0 || n_frames > youth::kMaxFrames || !youth::frame_size_ok(W, H, 3))
        return g_filter_err.set(YOUTH_EINVAL,
                                "%s: %d frames of %dx%d (need 0 <= frames <= 65535, 3 <= W, H <= 16384, "
                                "W*H <= 2^26)",
                                who, n_frames, W, H);
    if (P && (P->t0 < 1 || P->t0 > 255 || P->t2 < 0 || P->t2 > 1000))
        return g_filter_err.set(YOUTH_EINVAL, "%s: t0 %d, t2 %d (need 1 <= t0 <= 255, 0 <= t2 <= 1000)",
                                who, P->t0, P->t2);
    const size_t bytes = (size_t)n_frames * W * H * sizeof(int16_t);
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (!may_alias && a < b + bytes && b < a + bytes)
        return g_filter_err.set(YOUTH_EINVAL, "%s: the output overlaps the input", who);
    return YOUTH_OK;
}

extern "C" {

const char* youth_depth_filter_last_error(void) { return g_filter_err.c_str(); }

youth_filter_params youth_depth_filter_default_params(void)
{
    youth_filter_params p;
    p.t0 = 8;
    p.t2 = 96;
    return p;
}

int youth_depth_filter_device(int device, const int16_t* d_in, int16_t* d_out, int n_frames, int W,
                              int H, const youth_filter_params* P, void* stream)
{
    static const char* who = "youth_depth_filter_device";
    int rc = filter_check(who, d_in, d_out, n_frames, W, H, P, false);
    if (rc) return rc;
    rc = youth::check_device(g_filter_err, who, device);
    if (rc) return rc;
    if (n_frames == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(device));
    const youth_filter_params p = P ? *P : youth_depth_filter_default_params();
    const int tiles_x = (W + kFltTW - 1) / kFltTW, tiles_y = (H + kFltTH - 1) / kFltTH;
    // W % 4 == 0 keeps every frame of the batch as aligned as the first
    const bool vec = W % 4 == 0 && (((uintptr_t)d_in | (uintptr_t)d_out) & 7) == 0;
    hipLaunchKernelGGL(vec ? k_depth_filter<true> : k_depth_filter<false>,
                       dim3(tiles_x * tiles_y, n_frames), dim3(kFltThreads), 0, (hipStream_t)stream,
                       d_in, d_out, W, H, tiles_x, (unsigned)p.t0, (unsigned)p.t2);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int youth_depth_filter_host(int device, const int16_t* in, int16_t* out, int n_frames, int W, int H,
                            const youth_filter_params* P)
{
    static const char* who = "youth_depth_filter_host";
    // the host buffers may be one and the same: the filter runs between two
    // device buffers
    int rc = filter_check(who, in, out, n_frames, W, H, P, true);
    if (rc) return rc;
    rc = youth::check_device(g_filter_err, who, device);
    if (rc) return rc;
    if (n_frames == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n_frames * W * H * sizeof(int16_t);
    int16_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, 2 * bytes));
    int16_t* d_out = d + bytes / sizeof(int16_t);
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(d, in, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        rc = youth_depth_filter_device(device, d, d_out, n_frames, W, H, P, s);
        if (rc == YOUTH_OK) e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, s);
    }
    if (s) {
        const hipError_t e2 = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e2;
        (void)hipStreamDestroy(s);
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return g_filter_err.set(YOUTH_EHIP, "%s: %s", who, hipGetErrorString(e));
    return YOUTH_OK;
}

}  // extern "C"
