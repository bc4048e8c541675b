// Lens rectifier on gfx950 (C-ABI: include/youth_rectify.h; definition:
// DESIGN.md §17).
//
// The sensor's frames, distorted by the Brown-Conrady model (k1 k2 p1 p2 k3),
// are resampled into the frames of an ideal pinhole camera.  The forward model
// is closed-form in the direction a rectifier needs: output pixel -> source
// position, fp32 as written, then 1/32-px fixed point.  From there everything
// is integer, and there are no atomics, so the output is one bit pattern
// whatever the launch shape.
//
//   k_rectify_map   the map as data: two uint32 per output pixel.
//   k_rectify       the resampling pass, one launch per batch (the frame on
//                   gridDim.y).  A lane owns 4 adjacent output pixels of a
//                   row; it takes their map words from the rectifier's map
//                   (kMap) or recomputes them, reads 4 taps per pixel through
//                   unaligned 2-byte (depth) and 1-byte (colour) loads, and
//                   stores 8 B of depth and 12 B (4 B with one channel) of
//                   colour (kVec), or element by element on ragged widths and
//                   odd bases.  An uncovered pixel, or one past the row's end,
//                   reads the taps of pixel (0, 0), which every frame has
//                   (W, H >= 2), and selects 0: no lane branches on its data.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_host.h"
#include "youth_rectify.h"

namespace {

constexpr int kRectThreads = 256;
constexpr unsigned kCovered = 0x80000000u;

struct RectCam {
    float fx, fy, cx, cy;      // the sensor's camera
    float fxo, fyo, cxo, cyo;  // the output camera
    float k1, k2, p1, p2, k3;
};

// The map words of output pixel (u, v): youth_rectify.h, operation by operation.
__device__ __forceinline__ uint2 rect_map(const RectCam& c, int u, int v, int W, int H)
{
    const float x = ((float)u - c.cxo) / c.fxo;
    const float y = ((float)v - c.cyo) / c.fyo;
    const float xx = x * x, yy = y * y;
    const float r2 = xx + yy;
    const float rad = 1.0f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const float xy = x * y;
    const float tx = (2.0f * c.p1) * xy + c.p2 * (r2 + 2.0f * xx);
    const float ty = c.p1 * (r2 + 2.0f * yy) + (2.0f * c.p2) * xy;
    const float us = c.fx * (x * rad + tx) + c.cx;
    const float vs = c.fy * (y * rad + ty) + c.cy;
    // false for NaN; a covered position is at most 16383, so the fixed point fits
    const bool cov = us >= 0.0f && us <= (float)(W - 1) && vs >= 0.0f && vs <= (float)(H - 1);
    const int U = cov ? (int)floorf(us * 32.0f + 0.5f) : 0;
    const int V = cov ? (int)floorf(vs * 32.0f + 0.5f) : 0;
    const int ix = min(U >> 5, W - 2), iy = min(V >> 5, H - 2);
    const unsigned a = (unsigned)(U - 32 * ix), b = (unsigned)(V - 32 * iy);
    uint2 m;
    m.x = cov ? (kCovered | (b << 6) | a) : 0u;
    m.y = cov ? (unsigned)(iy * W + ix) : 0u;
    return m;
}

__global__ __launch_bounds__(kRectThreads) void k_rectify_map(RectCam cam, uint2* __restrict__ map,
                                                              int W, int H)
{
    const unsigned i = blockIdx.x * kRectThreads + threadIdx.x;
    if (i >= (unsigned)(W * H)) return;
    const int v = (int)(i / (unsigned)W), u = (int)(i - (unsigned)v * (unsigned)W);
    map[i] = rect_map(cam, u, v, W, H);
}

// One depth pixel from its 4 taps: the nearest tap n, copied when <= 0, else
// the gated bilinear mean around it.
__device__ __forceinline__ int rect_depth(int d00, int d10, int d01, int d11, unsigned a, unsigned b)
{
    const int top = a >= 16u ? d10 : d00, bot = a >= 16u ? d11 : d01;
    const int n = b >= 16u ? bot : top;
    const int c = n > 0 ? n : 1;   // an invalid centre computes on, unused
    const unsigned h = (unsigned)c >> 4;
    const unsigned g = 8u + (__umul24(__umul24(h, h), 96u) >> 16);
    const int T = (int)(g < 255u ? g : 255u);
    const unsigned wa[2] = {32u - a, a}, wb[2] = {32u - b, b};
    const int d[4] = {d00, d10, d01, d11};
    unsigned den = 0, num = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dl = d[k] - c;
        const bool on = d[k] > 0 && dl < T && -dl < T;
        const unsigned w = on ? __umul24(wa[k & 1], wb[k >> 1]) : 0u;
        den += w;
        num += __umul24(w, (unsigned)(dl + T));   // dl + T in [1, 509] where w != 0
    }
    // the nearest tap gives den >= 256 for a valid centre; an invalid one may see 0
    const unsigned dd = den ? den : 1u;
    const unsigned nn = num + (dd >> 1);          // < 2^20: exact as a float
    unsigned q = (unsigned)((float)nn * __builtin_amdgcn_rcpf((float)dd));
    const int rem = (int)(nn - __umul24(q, dd));  // the estimate is within 1 of the quotient
    if (rem < 0) --q;
    else if ((unsigned)rem >= dd) ++q;
    return n > 0 ? c - T + (int)q : n;
}

__device__ __forceinline__ unsigned rect_blend(unsigned c00, unsigned c10, unsigned c01, unsigned c11,
                                               unsigned w00, unsigned w10, unsigned w01, unsigned w11)
{
    return (__umul24(w00, c00) + __umul24(w10, c10) + __umul24(w01, c01) + __umul24(w11, c11) + 512u) >> 10;
}

struct alignas(4) RectRgb4 {
    unsigned x, y, z;   // 4 RGB pixels
};

// kVec: W % 4 == 0, the depth output 8-byte and the colour output 4-byte
// aligned, so a lane's 4 pixels lie inside one row and leave as whole words.
// Either plane pair may be null (wave-uniform).
template <bool kVec, bool kMap>
__global__ __launch_bounds__(kRectThreads) void k_rectify(RectCam cam, const uint2* __restrict__ map,
                                                          const int16_t* __restrict__ din,
                                                          int16_t* __restrict__ dout,
                                                          const uint8_t* __restrict__ cin,
                                                          uint8_t* __restrict__ cout, int ch, int W,
                                                          int H, int groups_x)
{
    const unsigned g = blockIdx.x * kRectThreads + threadIdx.x;
    const int row = (int)(g / (unsigned)groups_x);
    if (row >= H) return;
    const int px = 4 * (int)(g - (unsigned)row * (unsigned)groups_x);
    const size_t frame = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const size_t o = (size_t)row * W + px;   // this lane's first pixel in the frame

    uint2 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = kVec || px + j < W;
        if (kMap)
            m[j] = map[in ? o + j : 0];
        else
            m[j] = rect_map(cam, px + j, row, W, H);
        if (!in) m[j] = uint2{0u, 0u};
    }

    if (din) {
        const int16_t* __restrict__ src = din + frame;
        int16_t res[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int16_t* p = src + m[j].y;
            const int v = rect_depth(p[0], p[1], p[W], p[W + 1], m[j].x & 63u, (m[j].x >> 6) & 63u);
            res[j] = (m[j].x & kCovered) ? (int16_t)v : (int16_t)0;
        }
        int16_t* q = dout + frame + o;
        if (kVec) {
            *reinterpret_cast<short4*>(q) = short4{res[0], res[1], res[2], res[3]};
        } else {
            q[0] = res[0];
            if (px + 1 < W) q[1] = res[1];
            if (px + 2 < W) q[2] = res[2];
            if (px + 3 < W) q[3] = res[3];
        }
    }

    if (cin && ch == 3) {
        const uint8_t* __restrict__ src = cin + frame * 3;
        unsigned c[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = m[j].x & 63u, b = (m[j].x >> 6) & 63u;
            const unsigned w00 = __umul24(32u - a, 32u - b), w10 = __umul24(a, 32u - b);
            const unsigned w01 = __umul24(32u - a, b), w11 = __umul24(a, b);
            const uint8_t* p = src + (size_t)m[j].y * 3;
            const uint8_t* r = p + (size_t)W * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned v = rect_blend(p[k], p[3 + k], r[k], r[3 + k], w00, w10, w01, w11);
                c[3 * j + k] = (m[j].x & kCovered) ? v : 0u;
            }
        }
        uint8_t* q = cout + (frame + o) * 3;
        if (kVec) {
            RectRgb4 w;
            w.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            w.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
            w.z = c[8] | (c[9] << 8) | (c[10] << 16) | (c[11] << 24);
            *reinterpret_cast<RectRgb4*>(q) = w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < W) {
                    q[3 * j] = (uint8_t)c[3 * j];
                    q[3 * j + 1] = (uint8_t)c[3 * j + 1];
                    q[3 * j + 2] = (uint8_t)c[3 * j + 2];
                }
        }
    } else if (cin) {
        const uint8_t* __restrict__ src = cin + frame;
        unsigned c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = m[j].x & 63u, b = (m[j].x >> 6) & 63u;
            const uint8_t* p = src + m[j].y;
            const unsigned v = rect_blend(p[0], p[1], p[W], p[W + 1], __umul24(32u - a, 32u - b),
                                          __umul24(a, 32u - b), __umul24(32u - a, b), __umul24(a, b));
            c[j] = (m[j].x & kCovered) ? v : 0u;
        }
        uint8_t* q = cout + frame + o;
        if (kVec) {
            *reinterpret_cast<unsigned*>(q) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < W) q[j] = (uint8_t)c[j];
        }
    }
}

}  // namespace

// =============================================================== host side ==

// The rectifier's channel (hip_host.h): youth_rectify_last_error reads it.
static thread_local youth::ErrorText g_rectify_err;
#define HIP_ERR g_rectify_err

struct youth_rectify {
    int device = 0, W = 0, H = 0;
    RectCam cam{};
    uint2* d_map = nullptr;   // [H][W], written once by create
    long long covered = 0;
    // The apply kernel reads d_map or recomputes the words per pixel: the
    // measured choice, YOUTH_RECTIFY_MAP=0/1 at create for A/B.
    bool use_map = false;
    hipStream_t stream = nullptr;   // the host entry points' own stream
    // device staging of the host entry points, in frames
    int16_t *s_din = nullptr, *s_dout = nullptr;
    uint8_t *s_cin = nullptr, *s_cout = nullptr;
    size_t cap_d = 0, cap_c = 0;    // elements
};

static bool finite_all(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

// The arguments of the three apply entry points; may_alias: host buffers, which
// the kernel never sees.
static int rect_check(const char* who, const youth_rectify* r, const void* din, const void* dout,
                      const void* cin, const void* cout, int channels, int n_frames, bool may_alias)
{
    if (!r) return g_rectify_err.set(YOUTH_EINVAL, "%s: null rectifier", who);
    if ((din == nullptr) != (dout == nullptr) || (cin == nullptr) != (cout == nullptr))
        return g_rectify_err.set(YOUTH_EINVAL, "%s: a plane pair needs both its input and its output", who);
    if (!din && !cin) return g_rectify_err.set(YOUTH_EINVAL, "%s: neither depth nor colour given", who);
    if (cin && channels != 1 && channels != 3)
        return g_rectify_err.set(YOUTH_EINVAL, "%s: %d colour channels (need 1 or 3)", who, channels);
    if (n_frames < 0 || n_frames > youth::kMaxFrames)
        return g_rectify_err.set(YOUTH_EINVAL, "%s: %d frames (need 0 <= frames <= 65535)", who, n_frames);
    if (may_alias) return YOUTH_OK;
    const size_t N = (size_t)n_frames * r->W * r->H;
    const size_t nd = N * sizeof(int16_t), nc = N * (size_t)(cin ? channels : 0);
    if (ranges_overlap(dout, nd, din, nd) || ranges_overlap(dout, nd, cin, nc) ||
        ranges_overlap(cout, nc, din, nd) || ranges_overlap(cout, nc, cin, nc) ||
        ranges_overlap(dout, nd, cout, nc))
        return g_rectify_err.set(YOUTH_EINVAL, "%s: an output overlaps an input or the other output", who);
    return YOUTH_OK;
}

// Staging for n frames: depth planes, colour planes of `ch` bytes a pixel.
static int rect_stage(youth_rectify* r, bool depth, int ch, int n)
{
    const size_t N = (size_t)n * r->W * r->H;
    if (depth && N > r->cap_d) {
        size_t c0 = r->cap_d, c1 = r->cap_d;
        int rc = youth::grow_device_buffer(g_rectify_err, &r->s_din, &c0, N);
        if (rc == YOUTH_OK) rc = youth::grow_device_buffer(g_rectify_err, &r->s_dout, &c1, N);
        r->cap_d = rc == YOUTH_OK ? N : 0;
        if (rc) return rc;
    }
    if (ch && N * ch > r->cap_c) {
        size_t c0 = r->cap_c, c1 = r->cap_c;
        int rc = youth::grow_device_buffer(g_rectify_err, &r->s_cin, &c0, N * ch);
        if (rc == YOUTH_OK) rc = youth::grow_device_buffer(g_rectify_err, &r->s_cout, &c1, N * ch);
        r->cap_c = rc == YOUTH_OK ? N * ch : 0;
        if (rc) return rc;
    }
    return YOUTH_OK;
}

static void rect_launch(const youth_rectify* r, const int16_t* din, int16_t* dout, const uint8_t* cin,
                        uint8_t* cout, int ch, int n, hipStream_t s)
{
    const int W = r->W, H = r->H;
    const int groups_x = (W + 3) / 4;
    const unsigned blocks = (unsigned)(((long long)groups_x * H + kRectThreads - 1) / kRectThreads);
    // W % 4 == 0 keeps every frame of the batch as aligned as the first
    const bool vec = W % 4 == 0 && ((uintptr_t)dout & 7) == 0 && ((uintptr_t)cout & 3) == 0;
    auto k = vec ? (r->use_map ? k_rectify<true, true> : k_rectify<true, false>)
                 : (r->use_map ? k_rectify<false, true> : k_rectify<false, false>);
    hipLaunchKernelGGL(k, dim3(blocks, n), dim3(kRectThreads), 0, s, r->cam, r->d_map, din, dout, cin,
                       cout, ch, W, H, groups_x);
}

static void rect_launch_map(const youth_rectify* r, uint2* d_map, hipStream_t s)
{
    const unsigned blocks = (unsigned)(((long long)r->W * r->H + kRectThreads - 1) / kRectThreads);
    hipLaunchKernelGGL(k_rectify_map, dim3(blocks), dim3(kRectThreads), 0, s, r->cam, d_map, r->W, r->H);
}

extern "C" {

const char* youth_rectify_last_error(void) { return g_rectify_err.c_str(); }

void youth_rectify_destroy(youth_rectify* r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) {
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    (void)hipFree(r->d_map);
    (void)hipFree(r->s_din);
    (void)hipFree(r->s_dout);
    (void)hipFree(r->s_cin);
    (void)hipFree(r->s_cout);
    delete r;
}

int youth_rectify_create(int device, int W, int H, const youth_intrinsics* K, const youth_distortion* D,
                         const youth_intrinsics* Ko, youth_rectify** out)
{
    static const char* who = "youth_rectify_create";
    if (out) *out = nullptr;
    if (!K || !D || !out) return g_rectify_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if (!youth::frame_size_ok(W, H, 2))
        return g_rectify_err.set(YOUTH_EINVAL, "%s: %dx%d frames (need 2 <= W, H <= 16384, W*H <= 2^26)",
                                 who, W, H);
    const youth_intrinsics O = Ko ? *Ko : *K;
    const float kv[10] = {K->fx, K->fy, K->cx, K->cy, K->depth_scale, O.fx, O.fy, O.cx, O.cy, O.depth_scale};
    if (!finite_all(kv, 10) || !(K->fx > 0.0f) || !(K->fy > 0.0f) || !(O.fx > 0.0f) || !(O.fy > 0.0f))
        return g_rectify_err.set(YOUTH_EINVAL, "%s: a camera needs finite values and focal lengths > 0", who);
    const float dv[5] = {D->k1, D->k2, D->p1, D->p2, D->k3};
    if (!finite_all(dv, 5))
        return g_rectify_err.set(YOUTH_EINVAL, "%s: non-finite distortion coefficient (%g %g %g %g %g)", who,
                                 (double)D->k1, (double)D->k2, (double)D->p1, (double)D->p2, (double)D->k3);
    if (O.depth_scale != K->depth_scale)
        return g_rectify_err.set(YOUTH_EINVAL, "%s: the output camera's depth scale %g differs from the sensor's %g",
                                 who, (double)O.depth_scale, (double)K->depth_scale);
    int rc = youth::check_device(g_rectify_err, who, device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    youth_rectify* r = new youth_rectify;
    r->device = device;
    r->W = W;
    r->H = H;
    r->cam = RectCam{K->fx, K->fy, K->cx, K->cy, O.fx, O.fy, O.cx, O.cy, D->k1, D->k2, D->p1, D->p2, D->k3};
    if (const char* e = getenv("YOUTH_RECTIFY_MAP")) r->use_map = atoi(e) != 0;
    const size_t N = (size_t)W * H;
    std::vector<uint2> host(N);
    hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&r->d_map, N * sizeof(uint2));
    if (e == hipSuccess) {
        rect_launch_map(r, r->d_map, r->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), r->d_map, N * sizeof(uint2), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) {
        youth_rectify_destroy(r);
        return g_rectify_err.set(YOUTH_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    for (const uint2& m : host) r->covered += m.x >> 31;
    *out = r;
    return YOUTH_OK;
}

long long youth_rectify_covered(const youth_rectify* r) { return r ? r->covered : 0; }

int youth_rectify_map_device(youth_rectify* r, uint32_t* d_map, void* stream)
{
    static const char* who = "youth_rectify_map_device";
    if (!r || !d_map) return g_rectify_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if ((uintptr_t)d_map & 7) return g_rectify_err.set(YOUTH_EINVAL, "%s: the map needs an 8-byte aligned base", who);
    HIP_TRY(hipSetDevice(r->device));
    rect_launch_map(r, reinterpret_cast<uint2*>(d_map), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int youth_rectify_device(youth_rectify* r, const int16_t* d_depth_in, int16_t* d_depth_out,
                         const uint8_t* d_rgb_in, uint8_t* d_rgb_out, int channels, int n_frames, void* stream)
{
    static const char* who = "youth_rectify_device";
    const int rc = rect_check(who, r, d_depth_in, d_depth_out, d_rgb_in, d_rgb_out, channels, n_frames, false);
    if (rc) return rc;
    if (n_frames == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(r->device));
    rect_launch(r, d_depth_in, d_depth_out, d_rgb_in, d_rgb_out, d_rgb_in ? channels : 0, n_frames,
                (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int youth_rectify_host(youth_rectify* r, const int16_t* depth_in, int16_t* depth_out, const uint8_t* rgb_in,
                       uint8_t* rgb_out, int channels, int n_frames)
{
    static const char* who = "youth_rectify_host";
    int rc = rect_check(who, r, depth_in, depth_out, rgb_in, rgb_out, channels, n_frames, true);
    if (rc) return rc;
    if (n_frames == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(r->device));
    const int ch = rgb_in ? channels : 0;
    rc = rect_stage(r, depth_in != nullptr, ch, n_frames);
    if (rc) return rc;
    const size_t N = (size_t)n_frames * r->W * r->H;
    hipStream_t s = r->stream;
    hipError_t e = hipSuccess;
    if (depth_in) e = hipMemcpyAsync(r->s_din, depth_in, N * sizeof(int16_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && ch) e = hipMemcpyAsync(r->s_cin, rgb_in, N * ch, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        rect_launch(r, depth_in ? r->s_din : nullptr, depth_in ? r->s_dout : nullptr, ch ? r->s_cin : nullptr,
                    ch ? r->s_cout : nullptr, ch, n_frames, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && depth_in)
        e = hipMemcpyAsync(depth_out, r->s_dout, N * sizeof(int16_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && ch) e = hipMemcpyAsync(rgb_out, r->s_cout, N * ch, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return g_rectify_err.set(YOUTH_EHIP, "%s: %s", who, hipGetErrorString(e));
    return YOUTH_OK;
}

int youth_rectify_host_frames(youth_rectify* r, int16_t* const* depth, uint8_t* const* rgb, int n)
{
    static const char* who = "youth_rectify_host_frames";
    if (!r || !depth) return g_rectify_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if (n < 0 || n > youth::kMaxFrames)
        return g_rectify_err.set(YOUTH_EINVAL, "%s: %d frames (need 0 <= frames <= 65535)", who, n);
    for (int i = 0; i < n; ++i)
        if (!depth[i] || (rgb && !rgb[i])) return g_rectify_err.set(YOUTH_EINVAL, "%s: frame %d is null", who, i);
    if (n == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(r->device));
    const int ch = rgb ? 3 : 0;
    const int rc = rect_stage(r, true, ch, n);
    if (rc) return rc;
    const size_t N = (size_t)r->W * r->H;
    hipStream_t s = r->stream;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        e = hipMemcpyAsync(r->s_din + i * N, depth[i], N * sizeof(int16_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && ch) e = hipMemcpyAsync(r->s_cin + i * N * 3, rgb[i], N * 3, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) {
        rect_launch(r, r->s_din, r->s_dout, ch ? r->s_cin : nullptr, ch ? r->s_cout : nullptr, ch, n, s);
        e = hipGetLastError();
    }
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        e = hipMemcpyAsync(depth[i], r->s_dout + i * N, N * sizeof(int16_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && ch) e = hipMemcpyAsync(rgb[i], r->s_cout + i * N * 3, N * 3, hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return g_rectify_err.set(YOUTH_EHIP, "%s: %s", who, hipGetErrorString(e));
    return YOUTH_OK;
}

}  // extern "C"
