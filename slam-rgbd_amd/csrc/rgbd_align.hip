// rgbd_align.hip — RGB-D alignment on gfx950 (C-ABI: include/youth_rgbd.h;
// definition: DESIGN.md §13): k_rgbd_prep, k_rgbd_reduce and their host side.
// A unit of its own on the ICP context and launch layer of icp_host.h (the
// depth-only kernels it needs, k_prep, k_init and k_finish, run through that
// layer) and on icp_device.h's device code.  k_rgbd_reduce shares with
// k_reduce, as one text: the back-projection of a lane's four pixels
// (backproject4), a7 (survey_project), a7's gate with a8 and the exact a9
// (match_accumulate<kSpecSurvey>), the wave reduce-scatter, the hand-off to
// the pair's last workgroup with its fixed-order sum (handoff_publish,
// handoff_sum) and the a10 solve.  Its own: the intensity word, §13's
// photometric term and its two extra sums, the stats layout and neq_out.
//
//   k_rgbd_prep    once per target frame: RGB -> Y (or a grey copy) and one
//                  32-bit word per pixel {Y, gx + 255, gy + 255, valid}.  Four
//                  pixels of a row per thread.  Not LDS-staged: the rows above
//                  and below and the two columns beside the four are read from
//                  global memory again and come from cache.  The geometric
//                  records {z, nx, ny, nz} come from k_prep, unchanged.
//   k_rgbd_reduce  one launch per iteration, k_reduce's fused-solve form
//                  with the photometric term beside it: a workgroup takes a
//                  chunk of a pair's source pixels, four per lane and step,
//                  branch-free under lane masks; the 16-byte record and the
//                  4-byte photometric word of a lane's four pixels are
//                  gathered back to back; exact fp64
//                  products into 29 per-lane sums and two wave counts; wave
//                  reduce-scatter, one partial row [pair][chunk][31] and an
//                  arrival ticket; the pair's last workgroup adds the rows in a
//                  fixed order and runs the a10 solve and update.
//                  23 B/px/iteration: depth 2, Y 1, record 16, word 4.
//   k_rgbd_decimate  the level schedule's frames: every
//                  coarse level's plainly decimated depth and intensity of
//                  every frame of a call in one launch; a level then runs the
//                  kernels above, unchanged, on a context of its own size.
//
// Always the survey arithmetic of a7/a8 (no FMA, IEEE division) and the exact
// reduction of a9, whatever the ICP context's spec and reduce modes are.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "icp_device.h"
#include "icp_host.h"
#include "youth_filter.h"
#include "youth_rgbd.h"

using namespace youth_icp;

namespace {

constexpr int kRgbdNeq = YOUTH_RGBD_NEQ;
constexpr int kRgbdStride = 32;          // doubles per partial row (31 + a pad)
constexpr int kRgbdPrepThreads = 256;
constexpr unsigned kPhotoValid = 0x80000000u;

// host constants of §13: w = lambda / 255, kx = (0.5 w) fx, ky = (0.5 w) fy
struct PhotoK {
    float w, kx, ky;
};

__device__ __forceinline__ unsigned luma8(unsigned r, unsigned g, unsigned b)
{
    return (77u * r + 150u * g + 29u * b + 128u) >> 8;
}

// Y of pixel (row, x) of a frame of kCh channels; the caller keeps it inside
template <int kCh>
__device__ __forceinline__ unsigned load_y1(const uint8_t* __restrict__ f, int row, int x, int W)
{
    const uint8_t* p = f + ((size_t)row * W + x) * kCh;
    return kCh == 1 ? (unsigned)p[0] : luma8(p[0], p[1], p[2]);
}

// Y of pixels (row, x0 .. x0 + 3).  kVec: W % 4 == 0 and a 4-byte aligned
// frame base, so the four pixels lie in the row and move as one (grey) or
// three (RGB) aligned words; else each pixel alone, columns clamped to W - 1.
template <int kCh, bool kVec>
__device__ __forceinline__ void load_y4(const uint8_t* __restrict__ f, int row, int x0, int W,
                                        unsigned y[4])
{
    if (kVec) {
        const unsigned* q = reinterpret_cast<const unsigned*>(f + ((size_t)row * W + x0) * kCh);
        if (kCh == 1) {
            const unsigned a = q[0];
            y[0] = a & 255u;
            y[1] = (a >> 8) & 255u;
            y[2] = (a >> 16) & 255u;
            y[3] = a >> 24;
        } else {
            const unsigned a = q[0], b = q[1], c = q[2];
            y[0] = luma8(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
            y[1] = luma8(a >> 24, b & 255u, (b >> 8) & 255u);
            y[2] = luma8((b >> 16) & 255u, b >> 24, c & 255u);
            y[3] = luma8((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = load_y1<kCh>(f, row, min(x0 + k, W - 1), W);
    }
}

// grid (ceil(ceil(W / 4) H / 256), frames).  gray / photo may be null.
template <int kCh, bool kVec>
__global__ __launch_bounds__(kRgbdPrepThreads) void k_rgbd_prep(const uint8_t* __restrict__ in,
                                                                uint8_t* __restrict__ gray,
                                                                unsigned* __restrict__ photo, int W,
                                                                int H)
{
    const int gpr = (W + 3) >> 2;  // groups of four pixels per row
    const int idx = blockIdx.x * kRgbdPrepThreads + threadIdx.x;
    if (idx >= gpr * H) return;
    const int v = idx / gpr;
    const int x0 = (idx - v * gpr) * 4;
    const size_t N = (size_t)W * H;
    const uint8_t* __restrict__ f = in + (size_t)blockIdx.y * N * kCh;

    // rows and columns clamped into the frame: a clamped read feeds only a
    // border pixel, whose gradient is defined as 0
    unsigned yc[4], yu[4], yd[4];
    load_y4<kCh, kVec>(f, v, x0, W, yc);
    load_y4<kCh, kVec>(f, max(v - 1, 0), x0, W, yu);
    load_y4<kCh, kVec>(f, min(v + 1, H - 1), x0, W, yd);
    const unsigned row[6] = {load_y1<kCh>(f, v, max(x0 - 1, 0), W), yc[0], yc[1], yc[2], yc[3],
                             load_y1<kCh>(f, v, min(x0 + 4, W - 1), W)};
    const bool vin = v >= 1 && v <= H - 2;
    unsigned word[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int u = x0 + k;
        const bool valid = vin && u >= 1 && u <= W - 2;
        const int gx = valid ? (int)row[k + 2] - (int)row[k] : 0;
        const int gy = valid ? (int)yd[k] - (int)yu[k] : 0;
        word[k] = yc[k] | ((unsigned)(gx + 255) << 8) | ((unsigned)(gy + 255) << 17) |
                  (valid ? kPhotoValid : 0u);
    }
    const size_t o = (size_t)blockIdx.y * N + (size_t)v * W + x0;
    if (kVec) {
        if (gray)
            *reinterpret_cast<unsigned*>(gray + o) =
                yc[0] | (yc[1] << 8) | (yc[2] << 16) | (yc[3] << 24);
        if (photo) *reinterpret_cast<uint4*>(photo + o) = uint4{word[0], word[1], word[2], word[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) {
                if (gray) gray[o + k] = (uint8_t)yc[k];
                if (photo) photo[o + k] = word[k];
            }
    }
}

// The streaming tracker's ingest: m page-locked host frames,
// depth int16 [N] and RGB uint8 [N][3] each, fetched over PCIe by the GPU
// itself, as k_pull_frames does for depth alone and for its reason (a copy
// engine transfer stalled the submitting thread for milliseconds about once
// per run).  RGB crosses the bus once and leaves as intensity: 5 B/px in,
// 3 B/px out (depth 2, Y 1); the RGB bytes are written only where the caller
// wants them (rgb non-null: 8 B/px out).  grid (wg, m), 64 lanes; depth as
// 16-byte non-temporal loads, four in flight per lane; colour in units of 16
// pixels, three 16-byte loads and one 16-byte Y store, two units in flight.
// Each vector body runs where its source and destinations are 16-byte
// aligned, the rest of the frame (or all of it) element by element with the
// same integer arithmetic: the bytes are the same either way.  No LDS, no
// atomics, nothing waits on another workgroup.
struct RgbdFramePtrs {
    const int16_t* depth[YOUTH_TRACK_MAX_BATCH];
    const uint8_t* rgb[YOUTH_TRACK_MAX_BATCH];
};

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// four pixels' Y from their twelve bytes in three words (load_y4's unpacking)
__device__ __forceinline__ unsigned luma_word(unsigned a, unsigned b, unsigned c)
{
    return luma8(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u) |
           (luma8(a >> 24, b & 255u, (b >> 8) & 255u) << 8) |
           (luma8((b >> 16) & 255u, b >> 24, c & 255u) << 16) |
           (luma8((c >> 8) & 255u, (c >> 16) & 255u, c >> 24) << 24);
}

__device__ __forceinline__ v4u luma_unit(v4u a, v4u b, v4u c)
{
    return v4u{luma_word(a.x, a.y, a.z), luma_word(a.w, b.x, b.y), luma_word(b.z, b.w, c.x),
               luma_word(c.y, c.z, c.w)};
}

__global__ __launch_bounds__(64) void k_rgbd_pull(RgbdFramePtrs fp, int16_t* __restrict__ depth,
                                                  uint8_t* __restrict__ gray,
                                                  uint8_t* __restrict__ rgb, int N, int m)
{
    const int f = blockIdx.y;
    if (f >= m) return;
    const int stride = gridDim.x * 64;
    const int t0 = blockIdx.x * 64 + threadIdx.x;
    {
        const int16_t* __restrict__ s16 = fp.depth[f];
        int16_t* __restrict__ d16 = depth + (size_t)f * N;
        int done = 0;
        if ((((uintptr_t)s16 | (uintptr_t)d16) & 15) == 0) {
            const v4u* __restrict__ s = reinterpret_cast<const v4u*>(s16);
            v4u* __restrict__ d = reinterpret_cast<v4u*>(d16);
            const int nv = N / 8;
            int i = t0;
            for (; i + 3 * stride < nv; i += 4 * stride) {
                const v4u a = __builtin_nontemporal_load(s + i);
                const v4u b = __builtin_nontemporal_load(s + i + stride);
                const v4u c = __builtin_nontemporal_load(s + i + 2 * stride);
                const v4u e = __builtin_nontemporal_load(s + i + 3 * stride);
                d[i] = a;
                d[i + stride] = b;
                d[i + 2 * stride] = c;
                d[i + 3 * stride] = e;
            }
            for (; i < nv; i += stride) d[i] = __builtin_nontemporal_load(s + i);
            done = nv * 8;
        }
        for (int i = done + t0; i < N; i += stride) d16[i] = s16[i];
    }
    const uint8_t* __restrict__ sc = fp.rgb[f];
    uint8_t* __restrict__ g8 = gray + (size_t)f * N;
    uint8_t* __restrict__ c8 = rgb ? rgb + (size_t)f * N * 3 : nullptr;
    int done = 0;
    if ((((uintptr_t)sc | (uintptr_t)g8 | (uintptr_t)c8) & 15) == 0) {
        const v4u* __restrict__ s = reinterpret_cast<const v4u*>(sc);
        v4u* __restrict__ g = reinterpret_cast<v4u*>(g8);
        v4u* __restrict__ c = reinterpret_cast<v4u*>(c8);
        const int nu = N / 16;  // units of 16 pixels: 48 bytes in, 16 bytes of Y out
        int i = t0;
        for (; i + stride < nu; i += 2 * stride) {
            const int j = i + stride;
            const v4u a0 = __builtin_nontemporal_load(s + 3 * (size_t)i);
            const v4u a1 = __builtin_nontemporal_load(s + 3 * (size_t)i + 1);
            const v4u a2 = __builtin_nontemporal_load(s + 3 * (size_t)i + 2);
            const v4u b0 = __builtin_nontemporal_load(s + 3 * (size_t)j);
            const v4u b1 = __builtin_nontemporal_load(s + 3 * (size_t)j + 1);
            const v4u b2 = __builtin_nontemporal_load(s + 3 * (size_t)j + 2);
            g[i] = luma_unit(a0, a1, a2);
            g[j] = luma_unit(b0, b1, b2);
            if (c) {
                c[3 * (size_t)i] = a0;
                c[3 * (size_t)i + 1] = a1;
                c[3 * (size_t)i + 2] = a2;
                c[3 * (size_t)j] = b0;
                c[3 * (size_t)j + 1] = b1;
                c[3 * (size_t)j + 2] = b2;
            }
        }
        for (; i < nu; i += stride) {
            const v4u a0 = __builtin_nontemporal_load(s + 3 * (size_t)i);
            const v4u a1 = __builtin_nontemporal_load(s + 3 * (size_t)i + 1);
            const v4u a2 = __builtin_nontemporal_load(s + 3 * (size_t)i + 2);
            g[i] = luma_unit(a0, a1, a2);
            if (c) {
                c[3 * (size_t)i] = a0;
                c[3 * (size_t)i + 1] = a1;
                c[3 * (size_t)i + 2] = a2;
            }
        }
        done = nu * 16;
    }
    for (int i = done + t0; i < N; i += stride) {
        const unsigned r = sc[3 * (size_t)i], gg = sc[3 * (size_t)i + 1], b = sc[3 * (size_t)i + 2];
        g8[i] = (uint8_t)luma8(r, gg, b);
        if (c8) {
            c8[3 * (size_t)i] = (uint8_t)r;
            c8[3 * (size_t)i + 1] = (uint8_t)gg;
            c8[3 * (size_t)i + 2] = (uint8_t)b;
        }
    }
}

// a7's gate, a8 and the exact a9 by icp_device.h's match_accumulate, then
// §13's photometric term where the gate accepted the pixel and the target's
// word is valid.  acc: [0..26] A and b of both terms, [27] sum r^2, [29] sum rp^2.
template <bool kFast>
__device__ __forceinline__ void rgbd_accumulate(float qx, float qy, float qz, f4v t, unsigned pw,
                                                float ys, float uf, float vf, float fu, float fv,
                                                LaneMask inm, const Intr& K, const FastK& F,
                                                float thr2, const PhotoK& pk, double* acc,
                                                int& cnt_g, int& cnt_p)
{
    const LaneMask okm =
        match_accumulate<kSpecSurvey, kFast, true>(qx, qy, qz, t, fu, fv, inm, K, F, thr2, acc);
    const LaneMask pvm = okm & mask_ult(~kPhotoValid, pw);
    if (lane_in(pvm)) {
        const float yt = (float)(pw & 255u);
        const float gx = (float)((int)((pw >> 8) & 511u) - 255);
        const float gy = (float)((int)((pw >> 17) & 511u) - 255);
        const float du = uf - fu, dv = vf - fv;
        const float it = yt + 0.5f * (gx * du + gy * dv);
        const float rp = (it - ys) * pk.w;
        // IEEE divisions, as the definition words them
        const float hx = (gx * pk.kx) / qz;
        const float hy = (gy * pk.ky) / qz;
        const float hz = -((hx * qx + hy * qy) / qz);
        const float Jp[6] = {qy * hz - qz * hy, qz * hx - qx * hz, qx * hy - qy * hx, hx, hy, hz};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int bb = a; bb < 6; ++bb) {
                acc[k] = fma((double)Jp[a], (double)Jp[bb], acc[k]);
                ++k;
            }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = fma((double)Jp[a], (double)rp, acc[21 + a]);
        acc[29] = fma((double)rp, (double)rp, acc[29]);
    }
    // both counts per wave on the scalar unit
    cnt_g += __builtin_popcountll(okm);
    cnt_p += __builtin_popcountll(pvm);
}

// k_reduce's per-iteration pose state (stats: [pair][iters][4] here) and
// neq_out (stage-level entry point): the pair's last workgroup stores the 31
// sums there instead of solving.
struct RgbdState : PoseState {
    double* neq_out;  // [pair][31] or null
};

// grid (chunks, pairs).  kAligned: W % 4 == 0, the depth base 8-byte and the
// intensity base 4-byte aligned, centred columns exact (centred_exact): a
// lane's four pixels share a row and load as one word each.
template <bool kFast, bool kAligned>
__global__ __launch_bounds__(kRedThreads) void k_rgbd_reduce(
    const int16_t* __restrict__ dsrc, const uint8_t* __restrict__ gsrc,
    const float4* __restrict__ recs, size_t P, const unsigned* __restrict__ photo, PairMap pm, int W,
    int H, Intr K, FastK F, float thr2, PhotoK pk, int chunk, double* __restrict__ partials,
    RgbdState ps)
{
    __shared__ double red[kRedThreads / 64][kRgbdNeq];
    const int p = blockIdx.y;
    const int b = blockIdx.x;
    const int N = W * H;
    const int16_t* __restrict__ sD = dsrc + (size_t)(pm.src0 + p) * N;
    const uint8_t* __restrict__ sG = gsrc + (size_t)(pm.src0 + p) * N;
    // the pair's target records and words through buffer descriptors: a gather
    // past them (an unmatched lane's index) returns 0, an invalid record / word
    const __amdgpu_buffer_rsrc_t rrec = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(recs + (size_t)(pm.tgt0 + p) * P), (short)0,
        (int)(P * sizeof(float4)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rpho = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned*>(photo + (size_t)(pm.tgt0 + p) * N), (short)0,
        N * (int)sizeof(unsigned), 0x00020000);
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = ps.T32[p * 12 + k];

    double acc[kRgbdNeq];
#pragma unroll
    for (int k = 0; k < kRgbdNeq; ++k) acc[k] = 0.0;
    int cnt_g = 0, cnt_p = 0;

    const int start = b * chunk;
    const int end = min(start + chunk, N);
    const int stepV = kRedStep / W;
    const int stepU = kRedStep - stepV * W;
    int i = start + threadIdx.x * 4;
    int v0 = i / W;
    int u0 = i - v0 * W;
    for (; i < end; i += kRedStep) {
        const short4 d4 = load_depth4<kAligned>(sD, i, end);
        const int dd[4] = {d4.x, d4.y, d4.z, d4.w};
        unsigned g4;
        if (kAligned) {
            g4 = *reinterpret_cast<const unsigned*>(sG + i);
        } else {
            g4 = sG[i];
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (i + q < end) g4 |= (unsigned)sG[i + q] << (8 * q);
        }
        float qx[4], qy[4], qz[4], uf[4], vf[4], fu[4], fv[4];
        LaneMask in[4];
        int j[4];
        backproject4<kFast, kAligned>(
            dd, i, end, u0, v0, W, K, F,
            [&](int q, float sx, float sy, float sz) __attribute__((always_inline)) {
                survey_project(T, sx, sy, sz, K, W, H, qx[q], qy[q], qz[q], uf[q], vf[q], fu[q],
                               fv[q], in[q], j[q]);
            });
        u0 += stepU;
        v0 += stepV;
        if (u0 >= W) {
            u0 -= W;
            ++v0;
        }
        // eight gathers back to back: the records, then the words
        f4v t[4];
        unsigned pw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            t[q] = __builtin_bit_cast(
                f4v, __builtin_amdgcn_raw_buffer_load_b128(rrec, (int)((unsigned)j[q] * 16u), 0, 0));
#pragma unroll
        for (int q = 0; q < 4; ++q)
            pw[q] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rpho, (int)((unsigned)j[q] * 4u),
                                                                   0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            rgbd_accumulate<kFast>(qx[q], qy[q], qz[q], t[q], pw[q],
                                   (float)((g4 >> (8 * q)) & 255u), uf[q], vf[q], fu[q], fv[q],
                                   in[q], K, F, thr2, pk, acc, cnt_g, cnt_p);
    }
    // the wave's counts, carried by lane 0 into the wave / workgroup sums
    const int ln = threadIdx.x & 63;
    acc[28] = ln == 0 ? (double)cnt_g : 0.0;
    acc[30] = ln == 0 ? (double)cnt_p : 0.0;

    // wave reduce-scatter, then the four waves in fixed order through LDS
    const int wave = threadIdx.x >> 6;
    {
        double tot;
        wave_reduce_scatter<kRgbdNeq>(acc, ln, tot);
        if (!(ln & 1) && (ln >> 1) < kRgbdNeq) red[wave][ln >> 1] = tot;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;  // wave 0 publishes and, if last, solves
    const int lane = threadIdx.x;
    const int nblk = gridDim.x;
    double* mine = partials + ((size_t)p * nblk + b) * kRgbdStride;
    double s = 0.0;
    if (lane < kRgbdNeq) {
#pragma unroll
        for (int w = 0; w < kRedThreads / 64; ++w) s += red[w][lane];
    }
    // k_reduce's hand-off (icp_device.h): only the pair's last arriver goes on
    if (!handoff_publish<kRgbdNeq>(mine, ps, p, nblk, lane, s)) return;
    double neq[kRgbdNeq];
    handoff_sum<kRgbdNeq, kRgbdStride>(partials, p, nblk, lane, neq);
    if (lane == 0) {
        ps.arrivals[p] = 0;  // re-armed for the next launch (stream order)
        if (ps.stats) {
            double* st = ps.stats + ((size_t)p * ps.iters + ps.it) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) st[q] = neq[27 + q];
        }
        if (ps.neq_out) {
#pragma unroll
            for (int q = 0; q < kRgbdNeq; ++q) ps.neq_out[(size_t)p * kRgbdNeq + q] = neq[q];
        } else {
            // a10 unchanged on (A, b): its gates read the geometric count [28]
            solve_update(neq, ps.T64 + (size_t)p * 16, ps.T32 + (size_t)p * 12, ps.status + p);
        }
    }
}

// The level schedule's frames: plain decimation, out[j][i] =
// in[s j][s i], of both planes, for every coarse level of a schedule and every
// frame of a call in one launch.  Strides are powers of two, so a pixel of a
// coarser level is a pixel of every finer one: a thread takes a unit of 16
// pixels of a row the finest coarse level keeps (rows y = smin ky), reads it
// once and emits each level whose stride divides y from the same registers.
// Two frame sets (a pair call's sources and targets) share the launch.
// kVec: W % 16 == 0 and every base 16-byte aligned, so a unit lies in one row
// and moves as three 16-byte loads (the rows' cache lines are fetched whole
// either way) and a level's 16 / s pixels as one aligned store per plane; else
// guarded element loads of the kept pixels and element stores.  3 B/px of the
// kept rows in, 3 B per level pixel out.  No LDS, no atomics.
constexpr int kDecThreads = 256;
constexpr int kDecUnit = 16;
constexpr int kDecMaxLv = YOUTH_RGBD_MAX_LEVELS;

struct DecimJob {
    const int16_t* depth[2];  // set k: [n[k]][H][W]
    const uint8_t* gray[2];
    int n[2];
    int n_lv;                 // levels to emit, strides decreasing
    int stride[kDecMaxLv];    // each of 2, 4, 8, 16
    int16_t* dout[2][kDecMaxLv];  // [set][level]: [n[set]][H_s][W_s]
    uint8_t* gout[2][kDecMaxLv];
};

// dw: the unit's depths, pixel p in half p % 2 of word p / 2; gw: its
// intensities, pixel p in byte p % 4 of word p / 4.  Emits pixels 0, S, 2 S, ...
template <int S, bool kVec>
__device__ __forceinline__ void decim_emit(const unsigned (&dw)[8], const unsigned (&gw)[4], int x0,
                                           int y, int W, int H, int frame,
                                           int16_t* __restrict__ dout, uint8_t* __restrict__ gout)
{
    constexpr int C = kDecUnit / S;  // level pixels of the unit
    const int Ws = (W + S - 1) / S, Hs = (H + S - 1) / S;
    const size_t at = ((size_t)frame * Hs + y / S) * Ws + x0 / S;
    unsigned d[C], g[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int p = k * S;
        d[k] = (dw[p >> 1] >> (16 * (p & 1))) & 0xffffu;
        g[k] = (gw[p >> 2] >> (8 * (p & 3))) & 0xffu;
    }
    if constexpr (!kVec) {
#pragma unroll
        for (int k = 0; k < C; ++k)
            if (x0 + k * S < W) {  // so column (x0 + k S) / S < W_s
                dout[at + k] = (int16_t)d[k];
                gout[at + k] = (uint8_t)g[k];
            }
    } else if constexpr (C == 8) {
        *reinterpret_cast<uint4*>(dout + at) = uint4{d[0] | (d[1] << 16), d[2] | (d[3] << 16),
                                                     d[4] | (d[5] << 16), d[6] | (d[7] << 16)};
        *reinterpret_cast<uint2*>(gout + at) =
            uint2{g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24),
                  g[4] | (g[5] << 8) | (g[6] << 16) | (g[7] << 24)};
    } else if constexpr (C == 4) {
        *reinterpret_cast<uint2*>(dout + at) = uint2{d[0] | (d[1] << 16), d[2] | (d[3] << 16)};
        *reinterpret_cast<unsigned*>(gout + at) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    } else if constexpr (C == 2) {
        *reinterpret_cast<unsigned*>(dout + at) = d[0] | (d[1] << 16);
        *reinterpret_cast<unsigned short*>(gout + at) = (unsigned short)(g[0] | (g[1] << 8));
    } else {
        dout[at] = (int16_t)d[0];
        gout[at] = (uint8_t)g[0];
    }
}

// grid (bpf (n[0] + n[1])): bpf workgroups per frame, over ceil(W / 16) units x
// ceil(H / smin) kept rows; smin: the job's last (smallest) stride.
template <bool kVec>
__global__ __launch_bounds__(kDecThreads) void k_rgbd_decimate(DecimJob job, int W, int H, int smin,
                                                               int bpf)
{
    const int upr = (W + kDecUnit - 1) / kDecUnit;
    const int rows = (H + smin - 1) / smin;
    const int fb = (int)(blockIdx.x / (unsigned)bpf);
    const int idx = ((int)blockIdx.x - fb * bpf) * kDecThreads + (int)threadIdx.x;
    if (idx >= upr * rows) return;
    const int ky = idx / upr;
    const int x0 = (idx - ky * upr) * kDecUnit;
    const int y = ky * smin;
    // the job's arrays are read at constant indices only (they stay in SGPRs)
    const bool second = fb >= job.n[0];
    const int frame = second ? fb - job.n[0] : fb;
    const int16_t* __restrict__ dp = second ? job.depth[1] : job.depth[0];
    const uint8_t* __restrict__ gp = second ? job.gray[1] : job.gray[0];
    const size_t in = ((size_t)frame * H + y) * W + x0;
    unsigned dw[8], gw[4];
    if (kVec) {
        const uint4 da = *reinterpret_cast<const uint4*>(dp + in);
        const uint4 db = *reinterpret_cast<const uint4*>(dp + in + 8);
        const uint4 ga = *reinterpret_cast<const uint4*>(gp + in);
        dw[0] = da.x, dw[1] = da.y, dw[2] = da.z, dw[3] = da.w;
        dw[4] = db.x, dw[5] = db.y, dw[6] = db.z, dw[7] = db.w;
        gw[0] = ga.x, gw[1] = ga.y, gw[2] = ga.z, gw[3] = ga.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) dw[k] = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) gw[k] = 0u;
#pragma unroll
        for (int p = 0; p < kDecUnit; p += 2)  // odd pixels belong to no level
            if ((p & (smin - 1)) == 0 && x0 + p < W) {
                dw[p >> 1] = (unsigned)(unsigned short)dp[in + p];
                gw[p >> 2] |= (unsigned)gp[in + p] << (8 * (p & 3));
            }
    }
#pragma unroll
    for (int l = 0; l < kDecMaxLv; ++l) {
        if (l >= job.n_lv) break;
        const int s = job.stride[l];
        if (y & (s - 1)) continue;  // the level does not keep this row
        int16_t* __restrict__ dq = second ? job.dout[1][l] : job.dout[0][l];
        uint8_t* __restrict__ gq = second ? job.gout[1][l] : job.gout[0][l];
        switch (s) {
        case 2: decim_emit<2, kVec>(dw, gw, x0, y, W, H, frame, dq, gq); break;
        case 4: decim_emit<4, kVec>(dw, gw, x0, y, W, H, frame, dq, gq); break;
        case 8: decim_emit<8, kVec>(dw, gw, x0, y, W, H, frame, dq, gq); break;
        default: decim_emit<16, kVec>(dw, gw, x0, y, W, H, frame, dq, gq); break;
        }
    }
}

}  // namespace

// =============================================================== host side ==

struct youth_rgbd_ctx {
    youth_icp_ctx* icp = nullptr;  // records, poses, status, arrival counters, staging depth
    youth_rgbd_params prm{};
    PhotoK pk{};
    int frames = 0;                // frames the workspace holds: max_frames + 1
    int chunks = 0;                // YOUTH_RGBD_CHUNKS (0: planned)
    unsigned* d_photo = nullptr;   // [frames][N] packed words of the targets
    uint8_t* d_gray = nullptr;     // [frames][N] staging for the host entry points
    uint8_t* d_rgb = nullptr;      // [frames][N][3] (lazy: youth_rgbd_track_host_sequence)
    double* d_part = nullptr;      // [pair][chunk][kRgbdStride]
    size_t part_cap = 0;           // doubles
    double* d_stats = nullptr;     // [frames][stats_iters][4]
    int stats_iters = 0;
    double* d_neq = nullptr;       // [kRgbdNeq]
    int last_pairs = 0, last_iters = 0;
    hipStream_t last_stream = nullptr;

    // level schedule (youth_rgbd_set_levels).  A level's
    // workspace is a context of its own, W_s x H_s under K_s (this one for
    // stride 1); a coarse level's frames are decimated into depth / gray: the
    // call's sources (or its sequence) from element 0, its targets from
    // element off.
    struct Level {
        youth_rgbd_level lv{};
        youth_rgbd_ctx* ctx = nullptr;
        int16_t* depth = nullptr;
        uint8_t* gray = nullptr;
        size_t off = 0;  // elements, a multiple of 16
    };
    struct Schedule {
        int n = 0;
        Level at[YOUTH_RGBD_MAX_LEVELS];
    } sched;
    // the streaming tracker's own schedule (youth_rgbd_track_set_levels): the
    // same workspaces, without the decimated frames: a coarse level's banks
    // and slots are its context's own, at the parent's bank and slot indices
    Schedule trk_sched;
    // of the frame youth_rgbd_track_collect returned last
    int last_lv_n = 0;
    double last_lv_T[YOUTH_RGBD_MAX_LEVELS][16] = {};
    int32_t last_lv_st[YOUTH_RGBD_MAX_LEVELS] = {};

    // streaming tracker (youth_rgbd_track_*).  Depth and
    // intensity: two banks of trk_b frame slots, a submission's frames in the
    // bank the one before it did not use.  Records and words: slot 0 the
    // reference, slots 1 .. m the submission's frames (one bank: preps and
    // iterations of all submissions are ordered on the context's stream).
    int trk_b = 1;            // frames per submission at most; fixes the reduce geometry
    int trk_ref = -1;         // record / word slot of the reference (-1: none yet)
    int trk_bank = 0;         // bank of the next submission
    bool flt_on = false;
    youth_filter_params flt{8, 96};
    int16_t* d_raw = nullptr;  // [trk_raw_cap][N] unfiltered frames of one submission
    int trk_raw_cap = 0;
    int pull_wg = 0;           // YOUTH_RGBD_PULL_WG: k_rgbd_pull workgroups per frame (0: auto)
    hipEvent_t pull_ev = nullptr;  // youth_rgbd_pull_host: staging -> device done
    int16_t* pull_stage_d = nullptr;  // its pinned staging of pageable frames
    uint8_t* pull_stage_c = nullptr;
    int pull_stage_cap = 0;
    struct Sub {
        int m = 0, next = 0;      // frames of the submission, the next to collect
        int first_has_ref = 0;
        double* res = nullptr;    // pinned: [res_lv][res_cap][16] poses, then [res_lv][res_cap]
                                  // status words; without a schedule one level
        int res_cap = 0;          // frames `res` holds per level
        int res_lv = 0;           // levels `res` holds
        int n_lv = 0;             // levels of the submission (0: no schedule)
        int16_t* stage_d = nullptr;  // pinned staging of pageable frames [stage_cap][N]
        uint8_t* stage_c = nullptr;  //                                   [stage_cap][N][3]
        int stage_cap = 0;
        hipEvent_t h2d = nullptr, done = nullptr;
    } sub[2];
    int sub_head = 0, sub_n = 0;  // oldest submission in flight, submissions in flight
};

static int rgbd_track_pending(const youth_rgbd_ctx* r);

static int rgbd_size_ok(const char* who, int n, int W, int H)
{
    if (n < 0 || n > youth::kMaxFrames || !youth::frame_size_ok(W, H, 3))
        return g_icp_err.set(YOUTH_EINVAL,
                             "%s: %d frames of %dx%d (need 0 <= frames <= 65535, 3 <= W, H <= 16384, "
                             "W*H <= 2^26)",
                             who, n, W, H);
    return YOUTH_OK;
}

// k_rgbd_prep over n frames of `channels` channels; gray / photo nullable
static int rgbd_launch_prep(hipStream_t s, const uint8_t* in, int channels, int n, int W, int H,
                            uint8_t* gray, unsigned* photo)
{
    if (n <= 0) return YOUTH_OK;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(gray) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(photo) & 15) == 0;
    const long long groups = (long long)((W + 3) / 4) * H;
    const dim3 grid((unsigned)((groups + kRgbdPrepThreads - 1) / kRgbdPrepThreads), (unsigned)n);
    auto kern = channels == 3 ? (vec ? k_rgbd_prep<3, true> : k_rgbd_prep<3, false>)
                              : (vec ? k_rgbd_prep<1, true> : k_rgbd_prep<1, false>);
    hipLaunchKernelGGL(kern, grid, dim3(kRgbdPrepThreads), 0, s, in, gray, photo, W, H);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

// chunks per pair and pixels per chunk of one iteration's launch
static int rgbd_geometry(const youth_rgbd_ctx* r, int n_pairs, int* chunk_out)
{
    if (!r->chunks) return reduce_geometry(r->icp, n_pairs, chunk_out);
    const int N = r->icp->N;
    return round_chunks(N, std::min(r->chunks, (N + kRedStep - 1) / kRedStep), chunk_out);
}

static int rgbd_ensure_stats(youth_rgbd_ctx* r, int iters)
{
    return grow_device_buffer(g_icp_err, &r->d_stats, &r->stats_iters, iters, (size_t)r->frames * 4);
}

// One k_rgbd_reduce launch over n_pairs pairs: iteration `it` of `iters` with
// its fused solve, or (neq_out) the sums alone.
// geo_pairs: the pair count the chunks are planned for (0: n_pairs).
static int rgbd_launch_reduce(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc,
                              const uint8_t* gsrc, PairMap pm, int n_pairs, int it, int iters,
                              double* neq_out, int geo_pairs = 0)
{
    youth_icp_ctx* c = r->icp;
    int chunk = 0;
    const int nb = rgbd_geometry(r, geo_pairs > 0 ? geo_pairs : n_pairs, &chunk);
    int rc = grow_device_buffer(g_icp_err, &r->d_part, &r->part_cap,
                                (size_t)nb * n_pairs * kRgbdStride);
    if (rc) return rc;
    const float thr2 = r->prm.dist_thresh * r->prm.dist_thresh;
    const bool aligned = (reinterpret_cast<uintptr_t>(dsrc) % 8 == 0) &&
                         (reinterpret_cast<uintptr_t>(gsrc) % 4 == 0) && (c->W % 4 == 0) &&
                         c->centred_exact;
    const RgbdState ps{{c->d_T64, c->d_T32, c->d_status, neq_out ? nullptr : r->d_stats,
                        c->d_arrivals, it, iters},
                       neq_out};
    auto kern = c->fast ? (aligned ? k_rgbd_reduce<true, true> : k_rgbd_reduce<true, false>)
                        : (aligned ? k_rgbd_reduce<false, true> : k_rgbd_reduce<false, false>);
    hipLaunchKernelGGL(kern, dim3(nb, n_pairs), dim3(kRedThreads), 0, s, dsrc, gsrc, c->d_rec, c->P,
                       r->d_photo, pm, c->W, c->H, c->K, c->F, thr2, r->pk, chunk, r->d_part, ps);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

// Targets prepped (records by k_prep, words by k_rgbd_prep) into workspace
// frames [0, n_tgt); then the initial poses (dTi: device, or null for the
// identity) and `iters` launches.
static int rgbd_align_from(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc,
                           const uint8_t* gsrc, const int16_t* dtgt, const uint8_t* gtgt, int n_tgt,
                           PairMap pm, int n_pairs, const double* dTi, int iters, float* d_T_out)
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
        rc = rgbd_launch_reduce(r, s, dsrc, gsrc, pm, n_pairs, it, iters, nullptr);
        if (rc) return rc;
    }
    r->last_pairs = n_pairs;
    r->last_iters = iters;
    r->last_stream = s;
    if (!d_T_out) return YOUTH_OK;
    return export_poses(c, s, n_pairs, d_T_out, false);
}

// k_rgbd_decimate over the job's frames, W x H each
static int rgbd_launch_decimate(hipStream_t s, const DecimJob& job, int W, int H)
{
    const int nf = job.n[0] + job.n[1];
    if (nf <= 0 || job.n_lv <= 0) return YOUTH_OK;
    const int smin = job.stride[job.n_lv - 1];
    uintptr_t bits = 0;
    for (int k = 0; k < 2; ++k) {
        if (job.n[k] <= 0) continue;
        bits |= reinterpret_cast<uintptr_t>(job.depth[k]) | reinterpret_cast<uintptr_t>(job.gray[k]);
        for (int l = 0; l < job.n_lv; ++l)
            bits |= reinterpret_cast<uintptr_t>(job.dout[k][l]) |
                    reinterpret_cast<uintptr_t>(job.gout[k][l]);
    }
    const bool vec = W % kDecUnit == 0 && (bits & 15) == 0;
    const long long units = (long long)((W + kDecUnit - 1) / kDecUnit) * ((H + smin - 1) / smin);
    const long long bpf = (units + kDecThreads - 1) / kDecThreads;
    if (bpf * nf >= (1LL << 24))  // a launch's threads fit 32 bits
        return g_icp_err.set(YOUTH_EINVAL, "decimation: %d frames of %dx%d are too many for one launch",
                             nf, W, H);
    hipLaunchKernelGGL(vec ? k_rgbd_decimate<true> : k_rgbd_decimate<false>,
                       dim3((unsigned)(bpf * nf)), dim3(kDecThreads), 0, s, job, W, H, smin, (int)bpf);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

// The schedule's align: the frames of every coarse level in one decimation
// (set 0: n_src source frames, set 1: n_tgt target frames, or none where the
// targets are the sources' buffer, the sequence), then level after level on
// its workspace, each from the pose the level before it left on the device.
static int rgbd_align_levels(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc,
                             const uint8_t* gsrc, int n_src, const int16_t* dtgt,
                             const uint8_t* gtgt, int n_tgt, PairMap pm, int n_pairs,
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
        rc = rgbd_align_from(L.ctx, s, ds, gs, dt, gt, n_tgt, pm, n_pairs, dTi, L.lv.iters,
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
                      int n_src, const int16_t* dtgt, const uint8_t* gtgt, int n_tgt, PairMap pm,
                      int n_pairs, const double* T_init_host, float* d_T_out)
{
    if (r->sched.n > 0)
        return rgbd_align_levels(r, s, dsrc, gsrc, n_src, dtgt, gtgt, n_tgt, pm, n_pairs, T_init_host,
                                 d_T_out);
    const double* dTi = nullptr;
    int rc = upload_T_init(r->icp, s, T_init_host, n_pairs, &dTi);
    if (rc) return rc;
    return rgbd_align_from(r, s, dsrc, gsrc, dtgt, gtgt, n_tgt, pm, n_pairs, dTi, r->prm.iters,
                           d_T_out);
}

// A schedule of `owner` emptied: its child workspaces (which wait for their
// streams) and its frames released.
static void rgbd_drop_schedule(youth_rgbd_ctx::Schedule& S, const youth_rgbd_ctx* owner)
{
    for (youth_rgbd_ctx::Level& L : S.at) {
        if (L.ctx && L.ctx != owner) youth_rgbd_destroy(L.ctx);
        if (L.depth) (void)hipFree(L.depth);
        if (L.gray) (void)hipFree(L.gray);
        L = youth_rgbd_ctx::Level{};
    }
    S.n = 0;
}

static bool rgbd_stride_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8 || s == 16; }

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
                      d_dst_gray, n_pairs, PairMap{0, 0}, n_pairs, T_init, d_T_out);
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
                      n_frames - 1, PairMap{1, 0}, n_frames - 1, nullptr, d_T_out);
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

// The rules of a schedule for context r (`who` speaks); full_last: the last
// level has stride 1 (the tracker's).
static int rgbd_check_levels(const char* who, const youth_rgbd_ctx* r, const youth_rgbd_level* levels,
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

// A checked schedule's workspaces into `next` (emptied again on failure): per
// coarse level a context of W_s x H_s under K_s for r's max_frames and, with
// `frames`, room for the decimated frames of a call.
static int rgbd_build_schedule(const char* who, youth_rgbd_ctx* r, const youth_rgbd_level* levels,
                               int n, bool frames, youth_rgbd_ctx::Schedule& next)
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
    rc = rgbd_launch_reduce(r, s, c->d_depth, r->d_gray, PairMap{0, 1}, 1, 0, r->prm.iters, r->d_neq);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(neq31, r->d_neq, kRgbdNeq * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOUTH_OK;
}

int youth_rgbd_track_host_sequence(youth_rgbd_ctx* r, const int16_t* depth, const uint8_t* rgb,
                                   int n_frames, double* T_rel, int32_t* status)
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

}  // extern "C"

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

static int rgbd_launch_pull(youth_rgbd_ctx* r, hipStream_t s, const int16_t* const* depth,
                            const uint8_t* const* rgb, int m, int16_t* d_depth, uint8_t* d_gray,
                            uint8_t* d_rgb)
{
    RgbdFramePtrs fp{};
    for (int i = 0; i < m; ++i) {
        fp.depth[i] = depth[i];
        fp.rgb[i] = rgb[i];
    }
    // ~32 workgroups per launch, as k_pull_frames: the bus's latency is hidden
    // by loads in flight, not by occupancy
    const int wg = r->pull_wg > 0 ? r->pull_wg : std::max(4, 32 / m);
    hipLaunchKernelGGL(k_rgbd_pull, dim3(wg, m), dim3(64), 0, s, fp, d_depth, d_gray, d_rgb,
                       r->icp->N, m);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
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

static int rgbd_track_pending(const youth_rgbd_ctx* r)
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

// youth_icp_track_collect's wait: poll the event for up to 2 ms before the
// runtime's blocking wait (a sleeping wait's wake-up costs a backlogged worker
// more than the align it waits for)
static hipError_t rgbd_track_wait(hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    return hipEventSynchronize(ev);
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
        const PairMap pm{ref >= 0 ? d0 : d0 + 1, ref >= 0 ? 0 : 1};
        for (int it = 0; it < iters; ++it) {
            rc = rgbd_launch_reduce(Lr, s, c->d_depth, Lr->d_gray, pm, pairs, it, iters, nullptr,
                                    r->trk_b);
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
    const hipError_t e = rgbd_track_wait(q.done);
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
