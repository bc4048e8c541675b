// rgbd_align.hip — RGB-D alignment on gfx950 (C-ABI: include/youth_rgbd.h;
// definition: DESIGN.md §13): the kernel unit.  It holds every RGB-D
// __global__ kernel on icp_device.h's device code and, after them, the launch
// layer (rgbd_host.h): the only code that names these kernels.  The C API is
// in rgbd_api.cpp and rgbd_track.cpp; the depth-only kernels it needs (k_prep,
// k_init, k_finish) run through icp_host.h's layer.  k_rgbd_reduce shares with
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

#include <algorithm>

#include "icp_device.h"
#include "rgbd_host.h"

using namespace youth_icp;
using namespace youth_rgbd;

namespace {

constexpr int kRgbdPrepThreads = 256;
constexpr unsigned kPhotoValid = 0x80000000u;

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
constexpr int kDecMaxLv = YOUTH_RGBD_MAX_LEVELS;  // DecimJob's levels (rgbd_host.h)

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

// ============================================================ launch layer ==
// The functions of rgbd_host.h that name a kernel: each picks the variant its
// arguments allow and launches it.  Nothing else in the library does.

// chunks per pair and pixels per chunk of one iteration's launch
static int rgbd_geometry(const youth_rgbd_ctx* r, int n_pairs, int* chunk_out)
{
    if (!r->chunks) return reduce_geometry(r->icp, n_pairs, chunk_out);
    const int N = r->icp->N;
    return round_chunks(N, std::min(r->chunks, (N + kRedStep - 1) / kRedStep), chunk_out);
}

namespace youth_rgbd {

int rgbd_launch_prep(hipStream_t s, const uint8_t* in, int channels, int n, int W, int H,
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

int rgbd_launch_reduce(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc, const uint8_t* gsrc,
                       int src0, int tgt0, int n_pairs, int it, int iters, double* neq_out,
                       int geo_pairs)
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
                       r->d_photo, PairMap{src0, tgt0}, c->W, c->H, c->K, c->F, thr2, r->pk, chunk,
                       r->d_part, ps);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int rgbd_launch_decimate(hipStream_t s, const DecimJob& job, int W, int H)
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

int rgbd_launch_pull(youth_rgbd_ctx* r, hipStream_t s, const int16_t* const* depth,
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

}  // namespace youth_rgbd
