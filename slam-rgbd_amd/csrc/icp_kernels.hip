// icp_kernels.hip — MI355X (gfx950) kernels of the RGBD frame-to-frame ICP path.
//
// Hot path.  Reference boundary:
// Youth.Source/AlgorithmModule/SLAM.cpp:54 (TrackRGBD, the pose maths this
// replaces) and viewerModule.c:341-345 (the back-projection formula).
//
//   k_prep    target frames: int16 depth -> one 16-byte record {z, nx, ny, nz}
//             per pixel.  64x16 tiles; the (16+2) x (64+2) back-projected
//             neighbourhood is staged in LDS for the central-difference
//             normals.
//   k_reduce  per ICP iteration: source pixels straight from the int16 depth
//             (back-projected in registers), transform -> project -> ONE
//             16-byte record fetch -> gate -> residual -> Jacobian -> 29 fp64
//             accumulators per lane fed with exact fp32 products; wave
//             butterfly + LDS across waves -> one 29-double partial per
//             workgroup.  No atomics: deterministic.  18 B/px/iteration.
//   k_solve   one wave per pair: sums the partials in fixed order, LDL^T 6x6
//             solve, SE(3) exp, T <- exp(xi) T in fp64 on device, fp32 pose
//             for the next k_reduce.  No host round trip between iterations.
//
// Compiled with -ffp-contract=off: every fp32 expression rounds exactly as
// written, identical to the C oracle (oracle/icp_oracle.c) — XYZ, normals and
// association indices are bit-exact given the same fp32 pose.  The
// back-projection divides use a 2-instruction sequence only after
// k_verify_fastdiv has proven it equal to IEEE division on the ENTIRE domain
// those divides can see (d in [1, 32767], u in [0, W), v in [0, H)); otherwise
// the IEEE path is compiled in.
//
// This unit holds every depth-only __global__ kernel and, after them, the
// launch layer (icp_host.h): the only code that names these kernels.  The
// device code shared with rgbd_align.hip is in icp_device.h; the C API is in
// icp_api.cpp, icp_batch.cpp and icp_track.cpp.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <mutex>

#include "icp_device.h"
#include "icp_host.h"

namespace {

// -------------------------------------------------- self-checks on device --
// Exhaustive check of div_fast against IEEE division over the whole
// back-projection domain: z = d/ds (d in [1, 32767]); ((u - cx) z)/fx
// (u in [0, W)); ((v - cy) z)/fy (v in [0, H)).  Also covers the target
// recompute in k_reduce (tz is some d/ds, u' in [0, W), v' in [0, H)).
__global__ void k_verify_fastdiv(Intr K, FastK F, int W, int H, unsigned* bad)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (d > 32767) return;
    const float zi = (float)d / K.ds;
    unsigned nb = (div_fast((float)d, F.hds, F.lds) != zi);
    for (int u = blockIdx.y; u < W; u += gridDim.y) {
        const float n = ((float)u - K.cx) * zi;
        nb += (div_fast(n, F.hfx, F.lfx) != n / K.fx);
    }
    for (int v = blockIdx.y; v < H; v += gridDim.y) {
        const float n = ((float)v - K.cy) * zi;
        nb += (div_fast(n, F.hfy, F.lfy) != n / K.fy);
    }
    if (nb) atomicAdd(bad, nb);
}

// Self-test of the projection reciprocal (proj_rcp_rn) against IEEE 1.0f / den:
// bad[0]: bitwise mismatches over EVERY fp32 den in [2^-60, 2^60] (the
//         guarded range: exhaustive, ~1.0e9 values; must be 0);
// bad[1]: mismatches of the projected pixel floor(fma(num, rz, c + 0.5)) and
//         its in-range test [0, 65536) between proj_rcp_rn and 1.0f / den on
//         `n` SplitMix64 cases (den any positive finite fp32 incl. outside the
//         guard, num random with exponent in [-80, 80] or next to a
//         half-integer quotient, c in [0, 4096); must be 0).
__device__ __forceinline__ unsigned long long sm64(unsigned long long& x)
{
    unsigned long long z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ void k_selftest_projdiv(unsigned long long n, unsigned long long seed,
                                   unsigned long long* bad)
{
    unsigned long long b0 = 0, b1 = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr unsigned kLo = 0x21800000u, kHi = 0x5D800000u;  // 2^-60, 2^60
    for (unsigned long long b = kLo + tid; b <= kHi; b += stride) {
        const float den = __uint_as_float((unsigned)b);
        b0 += __float_as_uint(proj_rcp_rn(den)) != __float_as_uint(1.0f / den);
    }
    for (unsigned long long i = tid; i < n; i += stride) {
        unsigned long long st = seed ^ (i * 0xD1B54A32D192ED03ull);
        const unsigned long long r1 = sm64(st), r2 = sm64(st), r3 = sm64(st);
        const int ed = (i & 7) == 7 ? (int)(r1 % 254) - 126 : (int)(r1 % 121) - 60;
        const float den = __uint_as_float((unsigned)((ed + 127) << 23) | (unsigned)(r2 & 0x7FFFFF));
        float num;
        if (i & 1) {  // quotient next to a half-integer: the rounding-critical case
            const float m = (float)((int)(r3 % 8192) - 4096) + 0.5f;
            num = den * m;
            num = __uint_as_float(__float_as_uint(num) + (unsigned)((int)((r3 >> 20) & 7) - 3));
        } else {
            const int e = (int)((r3 >> 8) % 161) - 80;
            num = __uint_as_float((unsigned)((e + 127) << 23) | (unsigned)(r3 & 0x7FFFFF) |
                                  (unsigned)((r3 >> 63) << 31));
        }
        const float c = (float)(r2 >> 52);  // [0, 4096)
        const float ui = floorf(fmaf(num, 1.0f / den, c + 0.5f));
        const float uf = floorf(fmaf(num, proj_rcp_rn(den), c + 0.5f));
        const bool ii = (ui >= 0.0f) & (ui < 65536.0f), inf_ = (uf >= 0.0f) & (uf < 65536.0f);
        if (ii != inf_ || (ii && ui != uf)) ++b1;
    }
    if (b0) atomicAdd(bad + 0, b0);
    if (b1) atomicAdd(bad + 1, b1);
}

// Self-test of kSpecSurvey's projection quotient (proj_quot with
// proj_recip) against IEEE n / den:
//   bad[0]: bitwise quotient mismatches over `n` SplitMix64 cases with den
//           in the guard [2^-60, 2^60] and n of exponent in [-60, 60],
//           half of them next to a rounding midpoint of n / den (n =
//           RN(den (m + ulp(m)/2)) +- a few ulps);
//   bad[1]: mismatches of the projected pixel floor((q + c) + 0.5) and its
//           in-range test [0, 65536), den anywhere in the positive finite
//           fp32 range (outside the guard the kernels divide with IEEE),
//           c in [0, 4096): must be 0 for both;
//   bad[2]: floor_i32 against (int)floorf over ALL 2^32 bit patterns except
//           NaN and denormals: value mismatches where |x| < 2^30, and
//           in-range disagreements ((unsigned)r < 16384 vs 0 <= floorf(x) <
//           16384) anywhere: must be 0.
__device__ __forceinline__ float survey_quot(float n, float den)
{
    if (proj_den_ok(den)) return proj_quot(n, den, proj_recip(den));
    return n / den;
}
__global__ void k_selftest_projquot(unsigned long long n, unsigned long long seed,
                                    unsigned long long* bad)
{
    unsigned long long b0 = 0, b1 = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long i = tid; i < n; i += stride) {
        unsigned long long st = seed ^ (i * 0xD1B54A32D192ED03ull);
        const unsigned long long r1 = sm64(st), r2 = sm64(st), r3 = sm64(st);
        // guard-range quotient check
        {
            const int ed = (int)(r1 % 121) - 60;
            const float den = __uint_as_float((unsigned)((ed + 127) << 23) | (unsigned)(r2 & 0x7FFFFF));
            float num;
            if (i & 1) {
                const int em = (int)((r3 >> 40) % 41) - 20;
                const float m = __uint_as_float((unsigned)((em + 127) << 23) | (unsigned)(r3 & 0x7FFFFF));
                const double mid = (double)m + 0.5 * ((double)__uint_as_float(__float_as_uint(m) + 1u) - (double)m);
                num = (float)((double)den * mid);
                num = __uint_as_float(__float_as_uint(num) + (unsigned)((int)((r3 >> 23) & 7) - 3));
            } else {
                const int e = (int)((r3 >> 8) % 121) - 60;
                num = __uint_as_float((unsigned)((e + 127) << 23) | (unsigned)(r3 & 0x7FFFFF) |
                                      (unsigned)((r3 >> 63) << 31));
            }
            b0 += __float_as_uint(survey_quot(num, den)) != __float_as_uint(num / den);
        }
        // projected pixel, den over the whole positive range
        {
            const int ed = (i & 7) == 7 ? (int)(r2 % 254) - 126 : (int)(r2 % 121) - 60;
            const float den = __uint_as_float((unsigned)((ed + 127) << 23) | (unsigned)(r1 & 0x7FFFFF));
            float num;
            if (i & 2) {
                const float m = (float)((int)(r3 % 8192) - 4096) + 0.5f;
                num = den * m;
                num = __uint_as_float(__float_as_uint(num) + (unsigned)((int)((r3 >> 20) & 7) - 3));
            } else {
                const int e = (int)((r3 >> 8) % 161) - 80;
                num = __uint_as_float((unsigned)((e + 127) << 23) | (unsigned)(r3 & 0x7FFFFF) |
                                      (unsigned)((r3 >> 63) << 31));
            }
            const float c = (float)(r1 >> 52);
            const float ui = floorf((num / den + c) + 0.5f);
            const float uf = floorf((survey_quot(num, den) + c) + 0.5f);
            const bool ii = (ui >= 0.0f) & (ui < 65536.0f), inf_ = (uf >= 0.0f) & (uf < 65536.0f);
            if (ii != inf_ || (ii && ui != uf)) ++b1;
        }
    }
    unsigned long long b2 = 0;
    for (unsigned long long b = tid; b < (1ull << 32); b += stride) {
        const float x = __uint_as_float((unsigned)b);
        if (x != x || (x != 0.0f && fabsf(x) < 0x1p-126f)) continue;  // NaN, denormal
        const float f = floorf(x);
        const int r = floor_i32(x);
        const bool in_ref = (f >= 0.0f) & (f < 16384.0f);
        const bool in_got = (unsigned)r < 16384u;
        b2 += (in_ref != in_got) || (fabsf(x) < 0x1p30f && r != (int)f);
    }
    if (b0) atomicAdd(bad + 0, b0);
    if (b1) atomicAdd(bad + 1, b1);
    if (b2) atomicAdd(bad + 2, b2);
}

// Self-test of k_prep's fast normalisation (sqrt_rn_mid, norm_div):
//   bad[0]: sqrt_rn_mid(x) != sqrtf(x) over EVERY fp32 x in [2^-96, 2^118];
//   bad[1]: bitwise differences of (nx, ny, nz) vs c / sqrtf(len2) over `n`
//           random vectors (components of mixed magnitude down to 2^-110,
//           each +-0 with probability 1/8), wherever norm_fast_ok holds,
//           plus every vector where norm_fast_ok_bits differs from it;
//   bad[2]: number of random vectors that took the fast path (coverage).
__global__ void k_selftest_normalize(unsigned long long n, unsigned long long seed,
                                     unsigned long long* bad)
{
    unsigned long long b0 = 0, b1 = 0, nf = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr unsigned kLo = 0x0F800000u, kHi = 0x7A800000u;  // 2^-96, 2^118
    for (unsigned long long b = kLo + tid; b <= kHi; b += stride) {
        const float x = __uint_as_float((unsigned)b);
        b0 += __float_as_uint(sqrt_rn_mid(x)) != __float_as_uint(sqrtf(x));
    }
    for (unsigned long long i = tid; i < n; i += stride) {
        unsigned long long st = seed ^ (i * 0xD1B54A32D192ED03ull);
        const int e0 = (int)(sm64(st) % 131) - 70;  // leading exponent in [-70, 60]
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long r = sm64(st);
            const int e = max(e0 - (int)((r >> 32) % 48), -126);
            const unsigned sign = (unsigned)(r >> 63) << 31;
            c[k] = ((r >> 56) & 7) == 0
                       ? __uint_as_float(sign)
                       : __uint_as_float(sign | (unsigned)((e + 127) << 23) |
                                         (unsigned)(r & 0x7FFFFF));
        }
        const float len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
        b1 += norm_fast_ok_bits(len2, c[0], c[1], c[2]) != norm_fast_ok(len2, c[0], c[1], c[2]);
        if (!(len2 > 0.0f) || !norm_fast_ok(len2, c[0], c[1], c[2])) continue;
        ++nf;
        const float len = sqrt_rn_mid(len2), r = proj_recip(len), ref = sqrtf(len2);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            b1 += __float_as_uint(norm_div(c[k], len, r)) != __float_as_uint(c[k] / ref);
    }
    if (b0) atomicAdd(bad + 0, b0);
    if (b1) atomicAdd(bad + 1, b1);
    if (nf) atomicAdd(bad + 2, nf);
}

// ------------------------------------------------------------------ k_prep --
// grid (ceil(W/64), ceil(H/16), n_frames): frame f reads depth + f*N and
// writes the target records of workspace frame out0 + f (and, when xyz is
// non-null, its X/Y/Z planes: stage-level API only).  Normals (spec a6):
// n = normalize((P(u+1)-P(u-1)) x (P(v+1)-P(v-1))); (0,0,0) on the 1-px
// border, if the centre or any of the 4 neighbours is invalid, or if the
// cross product is zero; oriented so n.P <= 0.
// One kTileW x kTH tile of target records (and optional X/Y/Z planes) by a
// workgroup of kThreads: the (kTH+2) x (kTileW+2) back-projected
// neighbourhood is staged in the LDS planes sX/sY/sZ ([kTH+2][kLdsW]), then
// each thread forms the records of column tx = t & 63, rows ty, ty +
// kThreads/64, ...  kSc1: records are stored write-through (16-byte sc1
// buffer stores) for an in-launch hand-off (k_icp_coop).  Contains a
// workgroup barrier (every thread must call it); a caller reusing the LDS
// planes for another tile adds one more before it.
template <bool kFast, bool kWide, bool kSc1, int kThreads, int kTH, int kTW = kTileW>
__device__ __forceinline__ void prep_tile(const int16_t* __restrict__ dep, float4* __restrict__ R,
                                          int W, int H, size_t P, const Intr& K, const FastK& F,
                                          float* __restrict__ X, int x0, int y0, float* sX,
                                          float* sY, float* sZ)
{
    constexpr int kLH = kTH + 2;
    constexpr int kLW = kTW + 2;
    static_assert(kTW % 64 == 0 && kThreads % kTW == 0, "rows of whole waves");
    // the record loop below covers kTH rows in steps of kThreads / kTW: a
    // tile height that is not a multiple would leave its bottom rows unwritten
    static_assert(kTH % (kThreads / kTW) == 0, "tile rows a multiple of the rows per step");
    // the three LDS planes of the halo'd tile must fit a workgroup's 160 KB
    static_assert(3 * (kTH + 2) * (kTW + 2) * sizeof(float) <= 160 * 1024, "LDS planes fit");
    const int tx = threadIdx.x % kTW;
    const int ty = threadIdx.x / kTW;
    if (kWide) {
        // W % 4 == 0 (and an 8-byte-aligned frame): the tile's own columns
        // [x0, x0 + kTW) as kTW / 4 aligned 8-byte words per halo row (each
        // word's 4 pixels all inside or all outside the image, so no lane
        // straddles an edge and every pixel of a word is stored), then the two
        // edge columns x0 - 1 and x0 + kTW one pixel per lane.  An outside
        // pixel back-projects d = 0 at its own (u, v), as before.
        // Words load through a buffer descriptor over the frame: a row
        // outside the image or a word past the right edge takes the offset
        // W H 2 (the descriptor's size: past it, with no 32-bit wrap of
        // offset + bytes), which the range check returns as 0 (no branch, no
        // 64-bit address arithmetic).  The edge pixels are loaded first, so
        // their latency overlaps the words' instead of adding a round trip
        // before the barrier.
        static_assert(2 * kLH <= kThreads, "one edge pixel per thread");
        const bool edge = threadIdx.x < 2 * kLH;
        const int ely = threadIdx.x >> 1, eright = threadIdx.x & 1;
        const int egy = y0 - 1 + ely, egx = eright ? x0 + kTW : x0 - 1;
        const __amdgpu_buffer_rsrc_t rdep = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<int16_t*>(dep), (short)0, W * H * (int)sizeof(int16_t), 0x00020000);
        const bool ein = edge & ((unsigned)egy < (unsigned)H) & ((unsigned)egx < (unsigned)W);
        unsigned short dedge =
            __builtin_amdgcn_raw_buffer_load_b16(rdep, ein ? (egy * W + egx) * 2 : W * H * 2, 0, 0);
        // every word of the thread is requested before the first is used
        // (kIt loads in flight: 2 at 128 x 24 by 512 threads)
        constexpr int kWords = kTW / 4;  // 32 at 128: a shift, not a divide
        constexpr int kIt = (kLH * kWords + kThreads - 1) / kThreads;
        short4 wd[kIt];
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int e = threadIdx.x + it * kThreads;
            const int ly = e / kWords;
            const int gy = y0 - 1 + ly;
            const int c = x0 + 4 * (e - ly * kWords);
            const bool inside = (e < kLH * kWords) & ((unsigned)gy < (unsigned)H) & (c < W);
            wd[it] = __builtin_bit_cast(
                short4, __builtin_amdgcn_raw_buffer_load_b64(rdep, inside ? (gy * W + c) * 2 : W * H * 2, 0, 0));
        }
        // the loads above stay where they are: each result passes through an
        // empty asm here (the frame pointer is __restrict__, so a memory
        // clobber would not pin them), one wait for all of them
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            unsigned long long v = __builtin_bit_cast(unsigned long long, wd[it]);
            asm volatile("" : "+v"(v));
            wd[it] = __builtin_bit_cast(short4, v);
        }
        {
            unsigned v = dedge;
            asm volatile("" : "+v"(v));
            dedge = (unsigned short)v;
        }
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int e = threadIdx.x + it * kThreads;
            if (e >= kLH * kWords) break;
            const int ly = e / kWords;
            const int m = e - ly * kWords;
            const int gy = y0 - 1 + ly;
            const int c = x0 + 4 * m;
            const short4 d4 = wd[it];
            const int dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int lx = 4 * m + 1 + q;  // LDS column of pixel c + q
                float x, y, z;
                backproject<kFast>(dv[q], c + q, gy, K, F, x, y, z);
                sX[ly * kLW + lx] = x;
                sY[ly * kLW + lx] = y;
                sZ[ly * kLW + lx] = z;
            }
        }
        if (edge) {
            float x, y, z;
            backproject<kFast>((int)(short)dedge, egx, egy, K, F, x, y, z);
            const int lx = eright ? kLW - 1 : 0;
            sX[ely * kLW + lx] = x;
            sY[ely * kLW + lx] = y;
            sZ[ely * kLW + lx] = z;
        }
    } else {
        for (int e = threadIdx.x; e < kLH * kLW; e += kThreads) {
            const int ly = e / kLW;
            const int lx = e - ly * kLW;
            const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
            float x = 0.0f, y = 0.0f, z = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H)
                backproject<kFast>(dep[(size_t)gy * W + gx], gx, gy, K, F, x, y, z);
            sX[ly * kLW + lx] = x;
            sY[ly * kLW + lx] = y;
            sZ[ly * kLW + lx] = z;
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rrec =
        __builtin_amdgcn_make_buffer_rsrc(R, (short)0, (int)(P * sizeof(float4)), 0x00020000);
    // the row of each step is wave-uniform (ty = wave index): its tests and
    // offsets stay on the scalar unit
    const int tyw = __builtin_amdgcn_readfirstlane(ty);
#pragma unroll
    for (int k = 0; k < kTH / (kThreads / kTW); ++k) {
        const int row = tyw + (kThreads / kTW) * k;
        const int gx = x0 + tx, gy = y0 + row;
        if (gx >= W || gy >= H) continue;
        const size_t i = (size_t)gy * W + gx;
        const int ly = row + 1, lx = tx + 1;
        const int o = ly * kLW + lx;
        const float px = sX[o], py = sY[o], pz = sZ[o];
        if (X) {
            // an invalid pixel's point is (+0, +0, +0) (spec a2): its x, y
            // are (u - cx) 0 / fx, which is -0 left of and above the principal
            // point under the IEEE division (the fast one's n l term happens
            // to give +0 under the viewer's camera).  Only the stored planes
            // show the sign; the records never read an invalid point's x, y
            X[i] = pz > 0.0f ? px : 0.0f;
            X[P + i] = pz > 0.0f ? py : 0.0f;
            X[2 * P + i] = pz;
        }
        // every lane forms the record from its LDS neighbours (the halo
        // exists for every pixel of the tile): prep_record, icp_device.h
        const bool inner = (gx > 0) & (gy > 0) & (gx < W - 1) & (gy < H - 1);
        const float zl = sZ[o - 1], zr = sZ[o + 1];
        const float zu = sZ[o - kLW], zd = sZ[o + kLW];
        const float xr = sX[o + 1], xl = sX[o - 1];
        const float yr = sY[o + 1], yl = sY[o - 1];
        const float xd = sX[o + kLW], xu = sX[o - kLW];
        const float yd = sY[o + kLW], yu = sY[o - kLW];
        const float4 rec = prep_record(px, py, pz, xl, yl, zl, xr, yr, zr, xu, yu, zu, xd, yd, zd, inner);
        if (kSc1) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, rec), rrec,
                                                   (int)(i * sizeof(float4)), 0, 16);
        } else {
            // non-temporal (aux 2: nt): k_prep's 16 B/px stream of records is
            // read back by k_icp only after the whole batch is written (610 vs
            // 626 us per 512 frames, profiles/r02/ab_s30.txt, ab_s31.txt);
            // through the frame's buffer descriptor: a 32-bit byte offset
            // instead of 64-bit address arithmetic per record
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, rec), rrec,
                                                   (int)(i * sizeof(float4)), 0, 2);
        }
    }
}

// The persistent path's per-call state, set by k_prep's tile-(0,0) blocks
// (k_init's work folded in: one launch and its gap less per align): pair p's
// T64/T32 from T_init (or identity), status 0, epoch 0, arrival tickets 0;
// block (0,0,0) also zeroes the queue words.  n == 0: nothing.
struct InitArgs {
    const double* T_init;
    int n;
    double* T64;
    float* T32;
    int32_t* status;
    unsigned* epoch;
    unsigned* arrivals;  // [pair][iters]
    int iters;
    unsigned* head_err;
};

__device__ __forceinline__ void init_pairs(const InitArgs& ia, int tx, int ty, int f, int n_frames)
{
    if (tx != 0 || ty != 0) return;
    if (f == 0 && threadIdx.x < kMaxQueues && ia.head_err) {
        if (threadIdx.x == 0) {
            ia.head_err[kQHead] = 0u;
            ia.head_err[kQError] = 0u;
            ia.head_err[kQSpins] = 0u;
            ia.head_err[kQWaited] = 0u;
        }
        ia.head_err[kQHeads + kQHeadStride * threadIdx.x] = 0u;  // queue heads
    }
    const int t = threadIdx.x;
    for (int p = f; p < ia.n; p += n_frames) {
        if (t < 16) {
            const double v = ia.T_init ? ia.T_init[(size_t)p * 16 + t] : ((t % 5) == 0 ? 1.0 : 0.0);
            ia.T64[(size_t)p * 16 + t] = v;
            if (t < 12) ia.T32[(size_t)p * 12 + t] = (float)v;
        } else if (t == 16) {
            ia.status[p] = 0;
            ia.epoch[p] = 0u;
        } else {
            for (int k = t - 17; k < ia.iters; k += kPrepThreads - 17)
                ia.arrivals[(size_t)p * ia.iters + k] = 0u;
        }
    }
}

// One workgroup per 64 x 48 tile; a 1-D grid of tiles_x x tiles_y x n_frames
// workgroups.  xcd_map = 1: workgroups are dealt round-robin over the 8 XCDs
// (b and b + 8 share one; MI355X_MICROARCH.md "Workgroup dispatch"), so
// workgroup b takes tile t = (its XCD's share start) + b / 8: each XCD walks
// ONE contiguous run of tiles (frame-major, row-major within a frame), and a
// tile's horizontal and vertical halo lines belong to tiles that the same
// XCD processes at about the same time, i.e. are hits in that XCD's L2
// instead of fetches of lines that neighbouring tiles on other XCDs own.
// xcd_map = 2: each XCD takes whole rows of tiles, rows dealt round-robin
// (row R on XCD R % 8, its tiles in order), so the 8 XCDs work on 8
// adjacent tile rows of one frame at a time: a tile's horizontal halo lines
// belong to its own row (same XCD) and only the top / bottom halo rows (2 of
// 50) come from another XCD's row.  The grid is padded to a multiple of 8
// rows x tiles_x; padding workgroups return -1.
// xcd_map = 0: t = b (row-major over the frames: neighbours on other XCDs).
__device__ __forceinline__ int xcd_tile(int b, int total)
{
    const int q = total >> 3, r = total & 7, x = b & 7, j = b >> 3;
    return x < r ? x * (q + 1) + j : r * (q + 1) + (x - r) * q + j;
}
__device__ __forceinline__ int xcd_row_tile(int b, int tiles_x, int rows)
{
    const int j = b >> 3;
    const int R = (j / tiles_x) * 8 + (b & 7);
    return R < rows ? R * tiles_x + (j - (j / tiles_x) * tiles_x) : -1;
}

template <bool kFast, bool kWide>
__global__ __launch_bounds__(kPrepThreads) void k_prep(const int16_t* __restrict__ depth, int out0,
                                                      int W, int H, size_t P, Intr K, FastK F,
                                                      float4* __restrict__ recs,
                                                      float* __restrict__ xyz, InitArgs ia,
                                                      int tiles_x, int tiles_y, int n_frames,
                                                      int xcd_map)
{
    const int total = tiles_x * tiles_y * n_frames;
    const int t = xcd_map == 1   ? xcd_tile((int)blockIdx.x, total)
                  : xcd_map == 2 ? xcd_row_tile((int)blockIdx.x, tiles_x, tiles_y * n_frames)
                                 : (int)blockIdx.x;
    if (t < 0) return;  // grid padding (xcd_map 2)
    const int per = tiles_x * tiles_y;
    const int f = t / per;
    const int r = t - f * per;
    const int ty = r / tiles_x;
    const int tx = r - ty * tiles_x;
    init_pairs(ia, tx, ty, f, n_frames);
    __shared__ float sX[(kPrepTH + 2) * (kPrepTW + 2)];
    __shared__ float sY[(kPrepTH + 2) * (kPrepTW + 2)];
    __shared__ float sZ[(kPrepTH + 2) * (kPrepTW + 2)];
    const size_t N = (size_t)W * (size_t)H;
    prep_tile<kFast, kWide, false, kPrepThreads, kPrepTH, kPrepTW>(
        depth + (size_t)f * N, recs + (size_t)(out0 + f) * P, W, H, P, K, F,
        xyz ? xyz + (size_t)(out0 + f) * 3 * P : nullptr, tx * kPrepTW, ty * kPrepTH, sX, sY, sZ);
}

// ----------------------------------------------------------------- k_solve --
// Spec a10 on one wave per pair; the solve itself is icp_device.h's
// solve_update.

// Out-of-line copy for k_icp: inlined there, the solve's loop-invariant
// constants are hoisted into the kernel prologue and spilled across the
// pixel loop (128-VGPR budget), then reloaded from scratch on the pair's
// critical path.  A call keeps its registers to itself.
__device__ __attribute__((noinline)) int solve_update_wave_call(const double* neq, double* T64,
                                                                float* T32, int lane)
{
    return solve_update_wave(neq, T64, T32, lane);
}

// Sum the nblk partials of pair p in a fixed order: lanes 0..28 take the
// first half of the workgroups, lanes 32..60 the second, then one add.
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int nblk,
                                             double* sh)
{
    const int lane = threadIdx.x;
    const int half = (nblk + 1) >> 1;
    const int k = lane & 31;
    double s = 0.0;
    if (k < kNeq) {
        const int b0 = lane < 32 ? 0 : half;
        const int b1 = lane < 32 ? half : nblk;
        for (int bb = b0; bb < b1; ++bb) s += part[(size_t)bb * kNeq + k];
    }
    const double hi = __shfl_down(s, 32, 64);
    if (lane < kNeq) sh[lane] = s + hi;
    __syncthreads();
}


// grid n_pairs, one wave each.
__global__ __launch_bounds__(64) void k_solve(const double* __restrict__ partials,
                                              int nblk, int it, int iters,
                                              double* __restrict__ T64,
                                              float* __restrict__ T32,
                                              int32_t* __restrict__ status,
                                              double* __restrict__ stats,
                                              double* __restrict__ neq_out)
{
    __shared__ double sh[kNeq];
    const int p = blockIdx.x;
    sum_partials(partials + (size_t)p * nblk * kNeq, nblk, sh);
    if (threadIdx.x == 0) {
        if (stats) {
            stats[((size_t)p * iters + it) * 2 + 0] = sh[28];
            stats[((size_t)p * iters + it) * 2 + 1] = sh[27];
        }
        if (neq_out) {
            for (int k = 0; k < kNeq; ++k) neq_out[(size_t)p * kNeq + k] = sh[k];
        } else {
            solve_update(sh, T64 + (size_t)p * 16, T32 + (size_t)p * 12, status + p);
        }
    }
}

// Solve from a given record (stage-level validation entry point).
__global__ void k_solve_neq(const double* __restrict__ neq, double* T64, float* T32,
                            int32_t* status)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double sh[kNeq];
        for (int k = 0; k < kNeq; ++k) sh[k] = neq[k];
        *status = 0;
        solve_update(sh, T64, T32, status);
    }
}

// T64 <- T_init (or identity), T32 <- float(T64), status <- 0; zero the
// persistent kernel's epoch/arrival words and its dequeue head + error flag
// (G16: every polled word is re-initialised on every call).
__global__ void k_init(const double* __restrict__ T_init, int n, double* T64, float* T32,
                       int32_t* status, unsigned* epoch, unsigned* arrivals, int iters,
                       unsigned* head_err)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 && head_err) {  // one 128-B line each (kQ*): no false sharing
        head_err[kQHead] = 0u;     // dequeue head (contended atomic)
        head_err[kQError] = 0u;    // timeout flag (polled by waiters)
        head_err[kQSpins] = 0u;    // epoch polls (scheduler telemetry)
        head_err[kQWaited] = 0u;   // items that had to wait for their pair's pose
        for (int q = 0; q < kMaxQueues; ++q) head_err[kQHeads + kQHeadStride * q] = 0u;
    }
    if (p >= n) return;
    for (int i = 0; i < 16; ++i) {
        const double v = T_init ? T_init[(size_t)p * 16 + i] : ((i % 5) == 0 ? 1.0 : 0.0);
        T64[(size_t)p * 16 + i] = v;
        if (i < 12) T32[(size_t)p * 12 + i] = (float)v;
    }
    status[p] = 0;
    if (epoch) epoch[p] = 0u;
    if (arrivals)
        for (int k = 0; k < iters; ++k) arrivals[(size_t)p * iters + k] = 0u;
}


// ---------------------------------------------------------------- k_reduce --
// Spec a7-a9 for four consecutive source pixels per lane per step.
//   source  int16 depth (2 B/px), back-projected in registers (8-byte load
//           per lane when the frame is 8-byte aligned and W % 4 == 0);
//   target  ONE aligned 16-byte record fetch {z, nx, ny, nz} per pixel; the
//           target's x, y are recomputed from z with k_prep's expression, so
//           they are bit-identical to what k_prep would have stored.
// Branch-free: invalid lanes compute on safe values and are masked, so the
// four fetches issue back to back.  Accumulators are fp64 fed with exact
// fp32 products: the result equals the oracle's row-major fp64 sum up to
// fp64 summation order.  (tools/kbench: 205 us for the first SoA version ->
// 107 us for this one at 64 pairs, partial sums unchanged.)  The per-pixel
// code (xform_project, match_accumulate), the wave reduce-scatter and the
// fused solve's hand-off are icp_device.h's, shared with k_rgbd_reduce.

// Phase priority of k_icp's pixel loop (kPhase with prio, wave-uniform:
// IterState.prio, YOUTH_ICP_PRIO; k_reduce keeps the plain form).  The loop is
// bound by VALU issue at four waves per SIMD, and the SIMD picks the wave to
// issue from by priority, then age (MI355X_MICROARCH.md "Two waves per SIMD",
// item 2).  A step is a projection phase (four back-projections and
// projections, ending in the four record gathers and the depth prefetch) and
// a match phase that consumes the records.  The wave runs its projection
// phase at priority 1 and drops to 0 right after its last load is issued, so
// a wave that has not yet asked for its records issues ahead of the match
// phases of waves that already hold theirs, and its memory round trip runs
// behind their arithmetic instead of after it: -2.5 % on k_icp at no VALU
// instruction and no register (profiles/issue_order/).  Priority is 0 again
// before the step's first wait for a record, so it is 0 wherever the loop is
// left, at every barrier and at every poll of another workgroup's progress
// after it: a raised wave never waits on the waves it outranks.

// Accumulate source pixels [start, end) of one pair into acc (spec a7-a9).
template <int kSp, bool kAssoc, bool kFast, bool kAligned, bool kPhase = false>
__device__ __forceinline__ void accumulate_chunk(const int16_t* __restrict__ sD,
                                                 const float4* __restrict__ rec, int rec_bytes,
                                                 const float* __restrict__ T, int start, int end,
                                                 int W, int H, const Intr& K, const FastK& F,
                                                 float thr2, double* acc,
                                                 int32_t* __restrict__ arow, bool prio = false)
{
    // the pair's target records through a buffer descriptor (wave-uniform
    // base): a gather costs one 32-bit byte offset instead of 64-bit address
    // arithmetic
    const __amdgpu_buffer_rsrc_t rrec = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(rec), (short)0, rec_bytes, 0x00020000);
    // (u0, v0) of pixel i advance incrementally (no integer division per
    // step); with kAligned (W % 4 == 0, i % 4 == 0) a lane's four pixels
    // share one row.  The match conditions are lane masks (xform_project,
    // match_accumulate), so the four gathers issue back to back; an
    // unmatched pixel's gather is dropped by its mask.
    const int stepV = kRedStep / W;
    const int stepU = kRedStep - stepV * W;
    int i = start + threadIdx.x * 4;
    int v0 = i / W;
    int u0 = i - v0 * W;
    int cnt = 0;
    // lane32: this lane's fp32 sums over its whole share of the chunk,
    // converted to fp64 once at the end (acc enters zeroed)
    float facc[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) facc[q] = 0.0f;
    // kAligned: the next step's depth is loaded while this step's gathers
    // and sums run (8 bytes per lane in flight), through a buffer descriptor
    // over the frame, so the load past the last step returns 0 instead of
    // faulting; its value is then never used
    const __amdgpu_buffer_rsrc_t rdep = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int16_t*>(sD), (short)0, W * H * (int)sizeof(int16_t), 0x00020000);
    short4 dnext = kAligned && i < end ? __builtin_bit_cast(short4, __builtin_amdgcn_raw_buffer_load_b64(
                                                                       rdep, i * 2, 0, 0))
                                       : short4{};
    for (; i < end; i += kRedStep) {
        // (s_setprio is a scalar instruction: the guard is an SGPR condition)
        if (kPhase && prio) __builtin_amdgcn_s_setprio(1);
        const short4 d4 = kAligned ? dnext : load_depth4<kAligned>(sD, i, end);
        const int dd[4] = {d4.x, d4.y, d4.z, d4.w};
        float qx[4], qy[4], qz[4], fu[4], fv[4];
        LaneMask in[4];
        int j[4];
        backproject4<kFast, kAligned>(
            dd, i, end, u0, v0, W, K, F,
            [&](int q, float sx, float sy, float sz) __attribute__((always_inline)) {
                xform_project<kSp>(T, sx, sy, sz, K, W, H, qx[q], qy[q], qz[q], fu[q], fv[q],
                                   in[q], j[q]);
            });
        u0 += stepU;
        v0 += stepV;
        if (u0 >= W) {
            u0 -= W;
            ++v0;
        }
        // four 16-byte fetches back to back, then the next step's depth
        // (a gather issued behind its own projection, three quarters of the
        // phase earlier for the first, measured 10 % slower: HISTORY.md)
        f4v t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            t[q] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rrec, (int)((unsigned)j[q] * 16u),
                                                                                 0, 0));
        // (issued after the gathers: loads retire in order, so the match
        // waits for gather q, vmcnt(4 - q), never wait for the depth)
        asm volatile("" ::: "memory");
        if (kAligned)
            dnext = __builtin_bit_cast(
                short4, __builtin_amdgcn_raw_buffer_load_b64(rdep, (i + kRedStep) * 2, 0, 0));
        // every load of the step is issued: the match phase yields (a no-op
        // at priority 0)
        if (kPhase) __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            LaneMask okm;
            if constexpr (sp_lane32(kSp))
                okm = match_accumulate<kSp, kFast, false>(qx[q], qy[q], qz[q], t[q], fu[q], fv[q],
                                                          in[q], K, F, thr2, facc);
            else
                okm = match_accumulate<kSp, kFast, true>(qx[q], qy[q], qz[q], t[q], fu[q], fv[q],
                                                         in[q], K, F, thr2, acc);
            if (kAssoc && (i + q) < end) arow[i + q] = lane_in(okm) ? j[q] : -1;
            // matches counted per wave on the scalar unit (s_bcnt1 of the
            // match mask) instead of a per-lane select and add
            cnt += __builtin_popcountll(okm);

        }
    }
    if constexpr (sp_lane32(kSp)) {
#pragma unroll
        for (int q = 0; q < 28; ++q) acc[q] = (double)facc[q];
    }
    // the wave's count, carried by lane 0 into the wave / workgroup sums
    acc[28] += (threadIdx.x & 63) == 0 ? (double)cnt : 0.0;
}

// accumulate_chunk at the identity pose (k_icp's iteration 0 of an align
// without T_init, exact reduction): the same lanes take the same pixels in
// the same order, so the sums are accumulate_chunk's bit for bit, but each
// pixel's record is the one at its own index (ident_accumulate): a lane's
// four records are 64 contiguous bytes, requested before the back-projection
// instead of gathered after the projection.  A pixel at or past `end` has
// depth 0 (unaligned form), one past N reads the frame's zeroed pad.
template <int kSp, bool kFast, bool kAligned>
__device__ __forceinline__ void accumulate_chunk_ident(const int16_t* __restrict__ sD,
                                                       const float4* __restrict__ rec,
                                                       int rec_bytes, int start, int end, int W,
                                                       int H, const Intr& K, const FastK& F,
                                                       float thr2, double* acc)
{
    static_assert(!sp_lane32(kSp), "the lane32 sums keep the general path");
    const __amdgpu_buffer_rsrc_t rrec = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(rec), (short)0, rec_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rdep = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int16_t*>(sD), (short)0, W * H * (int)sizeof(int16_t), 0x00020000);
    const int stepV = kRedStep / W;
    const int stepU = kRedStep - stepV * W;
    int i = start + threadIdx.x * 4;
    int v0 = i / W;
    int u0 = i - v0 * W;
    int cnt = 0;
    short4 dnext = kAligned && i < end ? __builtin_bit_cast(short4, __builtin_amdgcn_raw_buffer_load_b64(
                                                                       rdep, i * 2, 0, 0))
                                       : short4{};
    for (; i < end; i += kRedStep) {
        const short4 d4 = kAligned ? dnext : load_depth4<kAligned>(sD, i, end);
        const int dd[4] = {d4.x, d4.y, d4.z, d4.w};
        f4v t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            t[q] = __builtin_bit_cast(
                f4v, __builtin_amdgcn_raw_buffer_load_b128(rrec, (i + q) * 16, 0, 0));
        asm volatile("" ::: "memory");
        if (kAligned)
            dnext = __builtin_bit_cast(
                short4, __builtin_amdgcn_raw_buffer_load_b64(rdep, (i + kRedStep) * 2, 0, 0));
        float sx[4], sy[4], sz[4];
        backproject4<kFast, kAligned>(dd, i, end, u0, v0, W, K, F,
                                      [&](int q, float x, float y, float z)
                                          __attribute__((always_inline)) {
                                              sx[q] = x;
                                              sy[q] = y;
                                              sz[q] = z;
                                          });
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int u = u0 + q, v = v0;  // backproject4's pixel q
            if (!kAligned) {
                const bool wrap = u >= W;
                u = wrap ? u - W : u;
                v = wrap ? v + 1 : v;
            }
            const LaneMask okm = ident_accumulate<kSp, kFast, true>(
                sx[q], sy[q], sz[q], t[q], (float)u, (float)v, K, F, thr2, acc);
            cnt += __builtin_popcountll(okm);
        }
        u0 += stepU;
        v0 += stepV;
        if (u0 >= W) {
            u0 -= W;
            ++v0;
        }
    }
    acc[28] += (threadIdx.x & 63) == 0 ? (double)cnt : 0.0;
}


template <int kSp, bool kAssoc, bool kFast, bool kAligned, bool kFuse>
__global__ __launch_bounds__(kRedThreads) void k_reduce(
    const int16_t* __restrict__ dsrc, const float4* __restrict__ recs, size_t P, PairMap pm,
    int W, int H, Intr K, FastK F, float thr2, int chunk, double* __restrict__ partials,
    int32_t* __restrict__ assoc, PoseState ps)
{
    __shared__ double red[kRedThreads / 64][kNeq];
    const int p = blockIdx.y;
    const int b = blockIdx.x;
    const int N = W * H;
    const int16_t* sD = dsrc + (size_t)(pm.src0 + p) * N;
    const float4* rec = recs + (size_t)(pm.tgt0 + p) * P;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = ps.T32[p * 12 + k];

    double acc[kNeq];
#pragma unroll
    for (int k = 0; k < kNeq; ++k) acc[k] = 0.0;

    const int start = b * chunk;
    const int end = min(start + chunk, N);
    int32_t* arow = kAssoc ? assoc + (size_t)p * N : nullptr;
    accumulate_chunk<kSp, kAssoc, kFast, kAligned>(sD, rec, (int)(P * sizeof(float4)), T, start, end,
                                              W, H, K, F, thr2, acc, arow);
    // wave reduce-scatter, then the four waves in fixed order through LDS
    const int wave = threadIdx.x >> 6;
    {
        const int ln = threadIdx.x & 63;
        double tot;
        wave_reduce_scatter<kNeq>(acc, ln, tot);
        if (!(ln & 1) && (ln >> 1) < kNeq) red[wave][ln >> 1] = tot;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;  // wave 0 publishes (and, if last, solves)
    const int lane = threadIdx.x;
    const int nblk = gridDim.x;
    double* mine = partials + ((size_t)p * nblk + b) * kNeq;
    double s = 0.0;
    if (lane < kNeq) {
#pragma unroll
        for (int w = 0; w < kRedThreads / 64; ++w) s += red[w][lane];
    }
    if (!kFuse) {
        if (lane < kNeq) mine[lane] = s;
        return;
    }
    // the hand-off (icp_device.h): only the pair's last arriver goes on
    if (!handoff_publish<kNeq>(mine, ps, p, nblk, lane, s)) return;
    double neq[kNeq];
    handoff_sum<kNeq, kNeq>(partials, p, nblk, lane, neq);
    if (lane == 0) {
        ps.arrivals[p] = 0;  // re-armed for the next launch (stream order)
        if (ps.stats) {
            ps.stats[((size_t)p * ps.iters + ps.it) * 2 + 0] = neq[28];
            ps.stats[((size_t)p * ps.iters + ps.it) * 2 + 1] = neq[27];
        }
        solve_update(neq, ps.T64 + (size_t)p * 16, ps.T32 + (size_t)p * 12, ps.status + p);
    }
}

// Fixed-order sum of a pair's nblk partial rows (kPartStride doubles each,
// written with sc1 stores by other workgroups, read with sc1 loads only).
// Called by every thread of the workgroup.  Thread (column j, piece q) with
// j < kSumCols loads rows j, j + 16, ... in batches of kBatch 16-byte pieces
// and adds each batch as a pairwise tree, batches in order; then wave 0
// lane l < kNeq adds the 16 column sums of value l as a pairwise tree.  The
// tree keeps the dependent fp64 adds per value at ~8 + batches instead of the
// 16 + rows of a running sum (the solve waits on it every iteration).  Returns
// the pair total of value `lane` in wave 0's lanes < kNeq (0 elsewhere).
template <int kN>
__device__ __forceinline__ double tree_sum(const double* v)
{
    if constexpr (kN == 1) {
        return v[0];
    } else {
        return tree_sum<kN / 2>(v) + tree_sum<kN / 2>(v + kN / 2);
    }
}

template <int kBatch>
__device__ __forceinline__ double sum_pair_rows(__amdgpu_buffer_rsrc_t rpart, int nblk,
                                                double (*colsum)[kPartStride])
{
    const int t = threadIdx.x;
    const int j = t / kPieces, q = t - j * kPieces;
    if (j < kSumCols) {
        double s0 = 0.0, s1 = 0.0;
        for (int bb = j; bb < nblk; bb += kBatch * kSumCols) {
            u4v v[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int b = bb + i * kSumCols;
                // aux 16 = sc1 (bypass this CU's L1: written by other CUs)
                v[i] = b < nblk ? __builtin_bit_cast(
                                      u4v, __builtin_amdgcn_raw_buffer_load_b128(
                                               rpart, (b * kPartStride + 2 * q) * 8, 0, 16))
                                : u4v{0u, 0u, 0u, 0u};
            }
            double a0[kBatch], a1[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                a0[i] = __hiloint2double((int)v[i].y, (int)v[i].x);
                a1[i] = __hiloint2double((int)v[i].w, (int)v[i].z);
            }
            s0 += tree_sum<kBatch>(a0);
            s1 += tree_sum<kBatch>(a1);
        }
        colsum[j][2 * q] = s0;
        colsum[j][2 * q + 1] = s1;
    }
    __syncthreads();
    double tsum = 0.0;
    if (t < kNeq) {
        double c[kSumCols];
#pragma unroll
        for (int jj = 0; jj < kSumCols; ++jj) c[jj] = colsum[jj][t];
        tsum = tree_sum<kSumCols>(c);
    }
    return tsum;
}

// ------------------------------------------------------------------- k_icp --
// ONE persistent launch for all `iters` iterations of a batch.
//
// Work item = (iteration k, pair p, chunk c), ordered iteration-major:
//   item = (k * n_pairs + p) * nblk + c.
// Workgroups take items from one dynamic dequeue counter.  An item of
// iteration k >= 1 waits until epoch[p] >= k, i.e. until iteration k-1 of
// pair p has been solved.  Every item it can wait on has a SMALLER index, so
// it was dequeued earlier by a running workgroup, and the earliest
// unfinished item never waits: the scheme cannot deadlock, whatever the
// residency (no co-residency assumption; cdna_hip_programming.md §1).  Every
// spin is bounded; a timeout sets *error and the workgroup exits, and the
// host reports it as YOUTH_STATUS_TIMEOUT (the GPU never hangs).
//
// Hand-offs (G16 / MI355X_MICROARCH "Valid forms" row 1): partials, T64 and
// T32 are written with sc1 stores, the storing wave drains (vmcnt(0)), then
// ONE agent-scope atomic (arrival ticket) or flag store (epoch); every read
// of handed-off bytes is an sc1 load by the wave that saw the ticket/flag.
struct IterState {
    double* T64;          // [pair][16]
    float* T32;           // [pair][12]
    int32_t* status;      // [pair]
    double* stats;        // [pair][iters][2] or null
    unsigned* arrivals;   // [pair][iters], zeroed per call
    unsigned* epoch;      // [pair], zeroed per call
    unsigned* head;       // queue words (telemetry at kQSpins / kQWaited), zeroed per call
    unsigned* error;      // timeout flag, zeroed per call
    float* T_out;         // [pair][16] fp32 4x4 written by the final solve, or null
    int iters, n_pairs, nblk, chunk;
    int nq;               // work queues (1..kMaxQueues): heads at head[kQHeads + 32 q]
    int ident_first;      // every pose starts at identity: iteration 0 takes accumulate_chunk_ident
    int first;            // first iteration to run (1: k_prep_ident ran iteration 0 and set epoch = 1)
    int prio;             // != 0: the pixel loop's projection phase at wave priority 1 (YOUTH_ICP_PRIO)
};

// One dequeue: from the workgroup's current queue q, moving on to the next
// queue when q is drained (each queue holds the pairs p = q (mod nq), items
// (iteration, pair, chunk) in that order).  Returns the item in the global
// numbering item = (k n_pairs + p) nblk + c, or `total` when every queue is
// drained.  The queues hold iterations is.first .. iters - 1 (first = 1 when
// k_prep_ident ran iteration 0 and left epoch[p] = 1).  Dependencies stay inside a queue (an item waits only on earlier
// items of its own pairs, dequeued before it by running workgroups), so
// every queue is deadlock-free on its own, as the single queue was; nq > 1
// spreads the contended returning atomics over nq words (one per 128-B line):
// MI355X_MICROARCH.md "dequeue": one head word pulled by 256+ CUs costs
// ~3 us per dequeue, 8 per-XCD heads ~1.2 us.
// Split in two so the first take's round trip can overlap other memory
// traffic: icp_dequeue_issue takes a ticket from queue q's head (the atomic),
// icp_dequeue_from decodes it, moving on to the next queues (synchronously)
// while q is drained.
__device__ __forceinline__ unsigned icp_dequeue_issue(const IterState& is, int q)
{
    return __hip_atomic_fetch_add(is.head + (kQHeads - kQHead) + q * kQHeadStride, 1u,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int icp_dequeue_from(const IterState& is, int& q, unsigned first,
                                                int total)
{
    unsigned t = first;
    for (int v = 0; v < is.nq; ++v) {
        const int npq = (is.n_pairs - q + is.nq - 1) / is.nq;
        if (v > 0 && npq > 0) t = icp_dequeue_issue(is, q);
        if (npq > 0) {
            const int per = npq * is.nblk;
            const int i = (int)t;
            if (i < (is.iters - is.first) * per) {
                const int k0 = i / per;
                const int rem = i - k0 * per;
                const int k = is.first + k0;
                const int pl = rem / is.nblk;
                const int c = rem - pl * is.nblk;
                return (k * is.n_pairs + q + is.nq * pl) * is.nblk + c;
            }
        }
        q = q + 1 == is.nq ? 0 : q + 1;
    }
    return total;
}
__device__ __forceinline__ int icp_dequeue(const IterState& is, int& q, int total)
{
    return icp_dequeue_from(is, q, icp_dequeue_issue(is, q), total);
}

constexpr unsigned kSpinMax = 1u << 23;  // x s_sleep(8) ~ seconds: a bound, never reached

__device__ __forceinline__ unsigned ld_u32_sc1(const unsigned* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_u64_sc1(const void* p)
{
    return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_u64_sc1(void* p, unsigned long long v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_u32_sc1(void* p, unsigned v)
{
    __hip_atomic_store(reinterpret_cast<unsigned*>(p), v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// Queue side of a work item, run by thread 0 after its workgroup published
// its previous partial (so a waiting workgroup never holds work another one
// waits for): wait (bounded) until pair p's pose epoch reaches k, then copy
// the pose into LDS.  Returns the item, or `total` when the queue is drained
// or after a timeout (error flag set).
__device__ __forceinline__ int icp_claim(const IterState& is, int item, int total, int per_iter,
                                         float* sh_T)
{
    if (item >= total) return total;
    const int k = item / per_iter;
    const int p = (item - k * per_iter) / is.nblk;
    if (k > 0) {
        unsigned spins = 0;
        while (ld_u32_sc1(is.epoch + p) < (unsigned)k) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > kSpinMax || ld_u32_sc1(is.error) != 0u) {
                __hip_atomic_fetch_or(is.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return total;
            }
        }
        if (spins) {  // scheduler telemetry (youth_icp_get_sched_stats)
            __hip_atomic_fetch_add(is.head + (kQSpins - kQHead), spins, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(is.head + (kQWaited - kQHead), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // the pose of (p, k): sc1 loads after the epoch matched
    unsigned long long v[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = ld_u64_sc1(is.T32 + p * 12 + 2 * q);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        sh_T[2 * q] = __uint_as_float((unsigned)v[q]);
        sh_T[2 * q + 1] = __uint_as_float((unsigned)(v[q] >> 32));
    }
    return item;
}

// Persistent ICP: ONE launch runs every iteration of every pair.  Work items
// (k, p, c) = (iteration, pair, pixel chunk) are dequeued in that order from
// one agent-scope counter; item (k, p, c) needs pair p's pose after k
// updates, published by the LAST workgroup to finish a chunk of (p, k-1)
// (arrival ticket), which sums the pair's partials in fixed order, solves and
// bumps epoch[p].  Per item: pixel loop -> wave reduce-scatter -> barrier ->
// wave 0 publishes the partial, takes the ticket (and, if last, solves) ->
// thread 0 dequeues and claims the next item -> barrier.
// (Dequeuing ahead from wave 1 so that waves 1-3 skip the second barrier
// measured no faster: DESIGN.md §5.)
// Wave priority is raised in the pixel loop only (is.prio, accumulate_chunk)
// and is 0 at every barrier here and in icp_claim's polls.  (Raising the
// hand-off chain too, wave 0 from its publish to the ticket and the last
// arriver through sum, solve and publish, measured -0.35 %: HISTORY.md.)
template <int kSp, bool kFast, bool kAligned>
__global__ __launch_bounds__(kRedThreads, 4) void k_icp(const int16_t* __restrict__ dsrc,
                                                    const float4* __restrict__ recs, size_t P,
                                                    PairMap pm, int W, int H, Intr K, FastK F,
                                                    float thr2, double* __restrict__ partials,
                                                    IterState is)
{
    __shared__ double red[kRedThreads / 64][kNeq];
    __shared__ double colsum[kSumCols][kPartStride];
    __shared__ double sh_neq[kNeq];
    __shared__ double sh_T64[12];
    __shared__ float sh_T32n[12];
    __shared__ int sh_item;
    __shared__ int sh_next;
    __shared__ int sh_last;
    __shared__ float sh_T[12];
    const int N = W * H;
    const int per_iter = is.n_pairs * is.nblk;
    const int total = is.iters * per_iter;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    // thread 0's current queue: workgroups are dealt to the queues
    // round-robin (b and b + 8 share an XCD, so with 8 queues each XCD pulls
    // from its own head)
    // (thread 1 keeps it: it dequeues the next item while wave 0 publishes)
    int myq = (int)(blockIdx.x % (unsigned)is.nq);
    if (threadIdx.x == 1) sh_next = icp_dequeue(is, myq, total);
    __syncthreads();
    if (threadIdx.x == 0) sh_item = icp_claim(is, sh_next, total, per_iter, sh_T);
    __syncthreads();
    for (;;) {
        // LDS-broadcast values are wave-uniform: readfirstlane keeps them
        // (and everything derived from them) in SGPRs
        const int item = __builtin_amdgcn_readfirstlane(sh_item);
        if (item >= total) return;
        const int k = item / per_iter;
        const int rem = item - k * per_iter;
        const int p = rem / is.nblk;
        const int c = rem - p * is.nblk;
        float T[12];
#pragma unroll
        for (int q = 0; q < 12; ++q)
            T[q] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh_T[q])));

        double acc[kNeq];
#pragma unroll
        for (int q = 0; q < kNeq; ++q) acc[q] = 0.0;
        const int start = c * is.chunk;
        const int end = min(start + is.chunk, N);
        // iteration 0 from the identity pose: every pixel matches the record
        // at its own index (wave-uniform choice per item; the same sums)
        bool ident = false;
        if constexpr (!sp_lane32(kSp)) ident = (k == 0) & (is.ident_first != 0);
        if (ident) {
            if constexpr (!sp_lane32(kSp))
                accumulate_chunk_ident<kSp, kFast, kAligned>(
                    dsrc + (size_t)(pm.src0 + p) * N, recs + (size_t)(pm.tgt0 + p) * P,
                    (int)(P * sizeof(float4)), start, end, W, H, K, F, thr2, acc);
        } else {
            accumulate_chunk<kSp, false, kFast, kAligned, true>(
                dsrc + (size_t)(pm.src0 + p) * N, recs + (size_t)(pm.tgt0 + p) * P,
                (int)(P * sizeof(float4)), T, start, end, W, H, K, F, thr2, acc, nullptr,
                is.prio != 0);
        }
        {
            double tot;
            wave_reduce_scatter<kNeq>(acc, lane, tot);
            if (!(lane & 1) && (lane >> 1) < kNeq) red[wave][lane >> 1] = tot;
        }
        __syncthreads();

        if (wave == 0) {
            // ---- publish this chunk's partial, take the arrival ticket; lane
            // 1 takes the next item from the queue meanwhile (its round trip
            // overlaps the stores' drain; the item is claimed, i.e. waited
            // on, only after this workgroup has published: the queue stays
            // deadlock-free)
            unsigned first = 0u;
            if (lane == 1) first = icp_dequeue_issue(is, myq);
            double sum = 0.0;
            if (lane < kPartStride) {
                if (lane < kNeq) {  // the waves' sums as a pairwise tree (2 dependent adds)
                    double r[kRedThreads / 64];
#pragma unroll
                    for (int w = 0; w < kRedThreads / 64; ++w) r[w] = red[w][lane];
                    sum = tree_sum<kRedThreads / 64>(r);
                }
                st_u64_sc1(partials + ((size_t)p * is.nblk + c) * kPartStride + lane,
                           (unsigned long long)__double_as_longlong(sum));
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) {
                const unsigned ticket = __hip_atomic_fetch_add(
                    is.arrivals + (size_t)p * is.iters + k, 1u, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
                sh_last = ticket == (unsigned)is.nblk - 1;
            }
            if (lane == 1) sh_next = icp_dequeue_from(is, myq, first, total);
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(sh_last)) {
            // ---- last arriver of (p, k): every wave sums a share of the
            // pair's partials (sum_pair_rows: sc1 16-byte loads, one batch
            // for <= 256 chunks, fixed tree order); wave 0 solves, publishes
            // the pose, then the epoch.
            const __amdgpu_buffer_rsrc_t rpart = __builtin_amdgcn_make_buffer_rsrc(
                partials + (size_t)p * is.nblk * kPartStride, (short)0,
                is.nblk * kPartStride * (int)sizeof(double), 0x00020000);
            if (threadIdx.x >= 64 && threadIdx.x < 64 + 12)
                sh_T64[threadIdx.x - 64] = __longlong_as_double(
                    (long long)ld_u64_sc1(is.T64 + (size_t)p * 16 + (threadIdx.x - 64)));
            const double tsum = sum_pair_rows<8>(rpart, is.nblk, colsum);
            if (wave == 0) {
                if (lane < kNeq) sh_neq[lane] = tsum;
                // the fp32 pose published when the solve skips the update (status != 0)
                if (lane < 12) sh_T32n[lane] = (float)sh_T64[lane];
                if (is.stats && lane == 0) {
                    is.stats[((size_t)p * is.iters + k) * 2 + 0] = readlane64(tsum, 28);
                    is.stats[((size_t)p * is.iters + k) * 2 + 1] = readlane64(tsum, 27);
                }
                const int st = solve_update_wave_call(sh_neq, sh_T64, sh_T32n, lane);
                if (st && lane == 0)
                    __hip_atomic_fetch_or(is.status + p, st, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                // publish: lanes < 12 store the pose (sc1), the wave drains, then the epoch
                if (lane < 12) {
                    st_u64_sc1(is.T64 + (size_t)p * 16 + lane,
                               (unsigned long long)__double_as_longlong(sh_T64[lane]));
                    st_u32_sc1(is.T32 + (size_t)p * 12 + lane, __float_as_uint(sh_T32n[lane]));
                }
                // the pair's final pose as the fp32 4x4 output (k_finish folded in)
                if (k == is.iters - 1 && is.T_out && lane < 16)
                    is.T_out[(size_t)p * 16 + lane] =
                        lane < 12 ? sh_T32n[lane] : (lane == 15 ? 1.0f : 0.0f);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) st_u32_sc1(is.epoch + p, (unsigned)(k + 1));
            }
        }
        // ---- next item (this workgroup has published: waiting is safe)
        if (threadIdx.x == 0) sh_item = icp_claim(is, sh_next, total, per_iter, sh_T);
        __syncthreads();
    }
}

// ------------------------------------------------------------ k_prep_ident --
// k_prep with the FIRST ICP iteration inside it, for aligns that start at the
// identity pose (no T_init, exact reduction; run_iterations).  There every
// source pixel matches the target record at its own index (icp_device.h
// ident_accumulate), and k_prep holds that record in registers, and the
// target's point in its LDS planes, when it stores it.  So the prep pass also
// loads the pair's source depth at the pixel (2 B/px) and runs the gate, r, J
// and the 29 sums, and k_icp runs iterations 1 .. iters - 1 only.  With them
// the pass is bound by VALU issue, not by its 16 B/px store stream (~186 VALU
// instructions per pixel, the SIMDs' issue slots full by the counters: DESIGN.md
// §5).
//   * A UNIT is one wave (a 64-thread workgroup) on 64 adjacent columns and a
//     band of `band` consecutive rows of one frame, lane l on column x0 + l:
//     no LDS planes and no barrier.  The wave walks down its columns with the
//     points of rows y - 1, y, y + 1 in registers (the vertical neighbours) and
//     takes the horizontal neighbours' points from lanes l - 1 and l + 1 by
//     whole-wave DPP shifts; lanes 0 and 63 take columns x0 - 1 and x0 + 64
//     from one more 2-byte load per row.  prep_record (icp_device.h) forms the
//     record, as in prep_tile.  Rows y0 - 1 and y0 + band are the band's halo:
//     loaded like any row, no record stored.
//   * Memory order: every iteration requests the depth words of the row two
//     ahead BEFORE it stores its record, so the wait for a row's words is a
//     counted one that leaves the younger loads and every record store in
//     flight; the loop never drains the memory counter (checked in the .s).
//     Each wave is an independent stream of loads and stores, 16 per CU.
//   * Units are ordered frame-major, then by band, then by column block:
//     waves that run together write adjacent 1-KB row segments.  At its end a
//     unit reduces once (wave_reduce_scatter), publishes one partial row and
//     takes one ticket on arrivals[p] (handoff_publish).
//   * The pair's last arriver adds the rows in fixed order (handoff_sum),
//     solves from the identity pose and writes everything k_init would have
//     written and iteration 0 would have left: T64 / T32, status,
//     stats[p][0], epoch[p] = 1, k_icp's tickets zeroed, and with iters == 1
//     the fp32 4x4 output.  It re-arms arrivals[p] for the next launch.
//   * No spin and no wait on another workgroup.  A frame that is no pair's
//     target only gets its records.
// The sums equal k_icp's iteration 0 up to fp64 summation order.
struct IdentArgs {
    const int16_t* dsrc;  // source depth frames
    PairMap pm;           // pair p: source frame src0 + p, target record frame tgt0 + p
    int n_pairs, iters;
    float thr2;
    double* partials;     // [pair][units per frame][kPartStride]
    double* T64;          // [pair][16]
    float* T32;           // [pair][12]
    int32_t* status;      // [pair]
    double* stats;        // [pair][iters][2] or null
    unsigned* epoch;      // [pair]
    unsigned* arr_it;     // [pair][iters] k_icp's arrival tickets
    unsigned* arrivals;   // [pair] this kernel's tickets: zero at launch, re-armed by the last arriver
    float* T_out;         // [pair][16] or null (written when iters == 1)
    unsigned* head_err;   // queue words, zeroed by workgroup 0
};

// Lane l takes v of lane l - 1 (from_left: wave_shr:1) or l + 1 (from_right:
// wave_shl:1); the lane without that neighbour (0, 63) keeps `edge`.  Every
// lane of the wave must be active: a disabled source lane leaves `edge` too.
__device__ __forceinline__ float from_left(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v),
                                                      0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_right(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v),
                                                      0x130, 0xf, 0xf, false));
}

// What a unit loads for the iteration of row y, two iterations ahead of it.
// The words as loaded (int16 bits, one register each): converted where they
// are used, so nothing touches a word between its request and its use.
struct PrepRowIn {
    unsigned t;  // target depth at (x, y + 1): the row that enters the window
    unsigned e;  // lanes 0 / 63: target depth at (x0 - 1, y) / (x0 + 64, y)
    unsigned s;  // source depth at (x, y)
};

template <int kSp, bool kFast>
__global__ __launch_bounds__(kPrepColW) void k_prep_ident(const int16_t* depth, int out0, int W,
                                                         int H, size_t P, Intr K, FastK F,
                                                         float4* recs, IdentArgs ia, int blocks_x,
                                                         int bands, int band)
{
    static_assert(!sp_lane32(kSp), "exact sums only");
    static_assert(kPrepColW == 64 && kMaxQueues <= kPrepColW, "one wave per unit");
    __shared__ double sh_neq[32 + 16];  // the last arriver's solve: [kNeq] sums, [16] T64
    __shared__ float sh_T32[12];
    const int lane = threadIdx.x;
    const int per = blocks_x * bands;  // units per frame
    const int f = (int)blockIdx.x / per;
    const int unit = (int)blockIdx.x - f * per;
    const int bi = unit / blocks_x;
    const int x0 = (unit - bi * blocks_x) * kPrepColW;
    const int y0 = bi * band, y1 = min(y0 + band, H);
    if (blockIdx.x == 0 && lane < kMaxQueues && ia.head_err) {
        if (lane == 0) {
            ia.head_err[kQHead] = 0u;
            ia.head_err[kQError] = 0u;
            ia.head_err[kQSpins] = 0u;
            ia.head_err[kQWaited] = 0u;
        }
        ia.head_err[kQHeads + kQHeadStride * lane] = 0u;
    }
    const int N = W * H;
    const int p = out0 + f - ia.pm.tgt0;  // the pair whose target this frame is
    const bool paired = (unsigned)p < (unsigned)ia.n_pairs;  // wave-uniform
    // Depth words load through buffer descriptors over the frame: a row or a
    // column outside the image takes an offset >= N 2 (the descriptor's size),
    // which the range check returns as 0 with no branch: an outside pixel
    // back-projects d = 0 at its own (u, v), as in prep_tile.  A frame that is
    // no pair's target has an empty source descriptor: every source depth is
    // 0, nothing matches and the sums stay untouched.
    const __amdgpu_buffer_rsrc_t rdep = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int16_t*>(depth + (size_t)f * N), (short)0, N * (int)sizeof(int16_t), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int16_t*>(ia.dsrc + (size_t)(ia.pm.src0 + (paired ? p : 0)) * N), (short)0,
        paired ? N * (int)sizeof(int16_t) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrec = __builtin_amdgcn_make_buffer_rsrc(
        recs + (size_t)(out0 + f) * P, (short)0, (int)(P * sizeof(float4)), 0x00020000);
    const int oob = N * 2;
    const int gx = x0 + lane;
    const int col2 = gx < W ? gx * 2 : oob;
    // the column beside the block: x0 - 1 in lane 0, x0 + 64 in lane 63 (the
    // other lanes load nothing and never use what they back-project from it)
    const int ex = lane == 0 ? x0 - 1 : x0 + kPrepColW;
    const bool eload = ((lane == 0) | (lane == kPrepColW - 1)) & ((unsigned)ex < (unsigned)W);
    const int ecol2 = eload ? ex * 2 : oob;
    // a column >= W stores nothing: its offset is past the record descriptor
    const int rcol = gx < W ? gx * (int)sizeof(float4) : (int)(P * sizeof(float4));

    // the row tests are wave-uniform: they and the row offsets stay scalar
    auto row2 = [&](int y, bool want) { return (want & ((unsigned)y < (unsigned)H)) ? y * W * 2 : oob; };
    auto load_tgt = [&](int off) {
        return (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rdep, off, 0, 0);
    };
    auto load_row = [&](int y) {
        const int rd = row2(y + 1, y < y1), rc = row2(y, y < y1);
        PrepRowIn r;
        r.t = load_tgt(col2 + rd);
        r.e = load_tgt(ecol2 + rc);
        r.s = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, col2 + rc, 0, 0);
        return r;
    };

    double acc[kNeq];
#pragma unroll
    for (int q = 0; q < kNeq; ++q) acc[q] = 0.0;
    int cnt = 0;  // this lane's matches (exact in the fp64 sum, whatever the order)

    // the window: rows y - 1 (u*), y (c*), y + 1 (d*) of this lane's column
    const int t_up = (short)load_tgt(col2 + row2(y0 - 1, true));
    const int t_c = (short)load_tgt(col2 + row2(y0, true));
    PrepRowIn in0 = load_row(y0), in1 = load_row(y0 + 1);
    float ux, uy, uz, cx, cy, cz;
    backproject<kFast>(t_up, gx, y0 - 1, K, F, ux, uy, uz);
    backproject<kFast>(t_c, gx, y0, K, F, cx, cy, cz);
    // One row: `in` holds the words of row y, requested two rows ago.  Once
    // they are taken, the same registers are requested for row y + 2, BEFORE
    // this row's record is stored: the wait for `in` is then a counted one that
    // covers neither the younger loads nor any store.  The loop runs two rows
    // per iteration so that in0 / in1 keep their registers (a copy from one to
    // the other would wait for the younger request).
    auto row = [&](int y, PrepRowIn& in) __attribute__((always_inline)) {
        // taken through an empty asm: the values below are new ones to the
        // compiler, so the request for row y + 2 lands in the registers of
        // `in` itself and the loop ends without copying a word still in flight
        int dt = (short)in.t, de = (short)in.e, dsr = (short)in.s;
        asm volatile("" : "+v"(dt), "+v"(de), "+v"(dsr));
        in = load_row(y + 2);
        float dx, dy, dz, ox, oy, oz;
        backproject<kFast>(dt, gx, y + 1, K, F, dx, dy, dz);
        backproject<kFast>(de, ex, y, K, F, ox, oy, oz);
        const bool inner = (gx > 0) & (y > 0) & (gx < W - 1) & (y < H - 1);
        const float4 rec =
            prep_record(cx, cy, cz, from_left(cx, ox), from_left(cy, oy), from_left(cz, oz),
                        from_right(cx, ox), from_right(cy, oy), from_right(cz, oz), ux, uy, uz, dx,
                        dy, dz, inner);
        // non-temporal, through the frame's descriptor (as prep_tile's)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, rec), rrec,
                                               rcol + y * W * (int)sizeof(float4), 0, 2);
        float sx, sy, sz;
        backproject<kFast>(dsr, gx, y, K, F, sx, sy, sz);
        const f4v t = {rec.x, rec.y, rec.z, rec.w};
        const LaneMask okm = ident_accumulate_xy<kSp, true>(sx, sy, sz, cx, cy, t, ia.thr2, acc);
        cnt += lane_in(okm) ? 1 : 0;
        ux = cx, uy = cy, uz = cz;
        cx = dx, cy = dy, cz = dz;
    };
    // Everything requested so far has landed before the loop is entered
    // (vmcnt(0), once per unit): with requests still in flight on entry the
    // compiler sizes the loop's waits for the entry edge, where no store
    // stands between the requests, and every iteration would wait for the
    // previous row's store.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    int y = y0;
    for (; y + 1 < y1; y += 2) {
        row(y, in0);
        row(y + 1, in1);
    }
    if (y < y1) row(y, in0);  // the last row of a band of odd length
    if (!paired) return;
    acc[28] = (double)cnt;
    double tot;
    wave_reduce_scatter<kNeq>(acc, lane, tot);
    // lanes 2q and 2q + 1 hold the sum of value q: lane q takes it
    const double s = __shfl(tot, (2 * lane) & 63, 64);
    PoseState ps{};
    ps.arrivals = ia.arrivals;
    if (!handoff_publish<kNeq>(ia.partials + ((size_t)p * per + unit) * kPartStride, ps, p, per, lane,
                               s))
        return;
    double neq[kNeq];
    handoff_sum<kNeq, kPartStride>(ia.partials, p, per, lane, neq);
    double* sh_T64 = sh_neq + 32;  // [16]
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kNeq; ++q) sh_neq[q] = neq[q];
    }
    if (lane < 16) sh_T64[lane] = (lane % 5) == 0 ? 1.0 : 0.0;
    if (lane < 12) sh_T32[lane] = (lane % 5) == 0 ? 1.0f : 0.0f;
    const int st = solve_update_wave_call(sh_neq, sh_T64, sh_T32, lane);
    if (lane < 16) ia.T64[(size_t)p * 16 + lane] = sh_T64[lane];
    if (lane < 12) ia.T32[(size_t)p * 12 + lane] = sh_T32[lane];
    if (ia.iters == 1 && ia.T_out && lane < 16)
        ia.T_out[(size_t)p * 16 + lane] = lane < 12 ? sh_T32[lane] : (lane == 15 ? 1.0f : 0.0f);
    for (int k = lane; k < ia.iters; k += 64) ia.arr_it[(size_t)p * ia.iters + k] = 0u;
    if (lane == 0) {
        ia.status[p] = st;
        ia.epoch[p] = 1u;
        ia.arrivals[p] = 0u;  // re-armed for the next launch (stream order)
        if (ia.stats) {
            ia.stats[(size_t)p * ia.iters * 2 + 0] = neq[28];
            ia.stats[(size_t)p * ia.iters * 2 + 1] = neq[27];
        }
    }
}

// -------------------------------------------------------------- k_icp_coop --
// Small batches: C2's single pair and the SLAM tracker's frame-to-frame align
// (youth_icp_track_frame).  One pair cannot fill the chip, so k_icp's cost
// there is the chain of memory round trips per iteration (dequeue, pose poll,
// pose load, cold depth and record loads, ticket, last-arriver solve, pose
// publish: ~17 us).  This kernel shortens that chain:
//   * ONE cooperative launch of n_pairs x G co-resident workgroups replaces
//     k_init + k_icp + k_finish; workgroup b owns chunk c = b % G of pair
//     p = b / G for every iteration (no queue);
//   * its source pixels (npx per lane) are loaded and back-projected ONCE
//     into LDS; its record gathers hit the same lines every iteration
//     (L1/L2-warm);
//   * per iteration ONE hand-off, and no counter in it: each workgroup
//     stores its partial row (sc1, 8-byte stores) over a row that holds the
//     EMPTY pattern, and every workgroup loads ALL the pair's rows, loading
//     again every 16-byte piece that still holds EMPTY, then sums them in the
//     fixed column order of k_icp's last arriver and solves itself.
//     Identical inputs and code give every workgroup the identical fp64
//     pose, so no pose is handed off.  The wait is the data itself: one
//     memory round trip after the last row lands, where an arrival counter
//     costs three (store drain + atomic, counter poll, row loads; round 5:
//     publish + arrive 1.04, poll 0.80, row loads 1.16 us per iteration).
// EMPTY is a signalling NaN (high word kPartEmptyHi): fp64 arithmetic never
// yields one (NaN results are quiet), so a row value can never look empty;
// each value is one 8-byte store and is checked on its own, so no ordering
// between a row's values is needed.  Rows are triple-buffered by iteration
// (k % 3): once a workgroup has seen every row of iteration k, every
// workgroup of the pair has read iteration k-1's rows (it read them before it
// stored k), so it resets its OWN row of buffer (k+2) % 3 = (k-1) % 3 to
// EMPTY, drains, and only then stores iteration k+1: whoever loads
// iteration k+2's rows has seen that k+1 row first, so it sees EMPTY or the
// k+2 value, never the k-1 one.  Across calls the rows alternate between two
// arenas with the counter sets: a call resets the rows the previous call
// used in the other arena (stream order: the arena a call uses is never the
// one it resets).  Co-residency is NOT guaranteed: by default the grid is a
// plain launch sized to an idle device's capacity (coop_enqueue orders this
// process's cooperative launches per device; hipLaunchCooperativeKernel is
// opt-in, YOUTH_ICP_COOP_LAUNCH=runtime), so another process holding CUs
// can leave workgroups unscheduled.  Every spin is therefore bounded
// (timeout -> YOUTH_STATUS_TIMEOUT, no hang), every workgroup preps its
// tiles before it first waits (a timed-out launch still leaves complete
// records), and the tracker realigns a timed-out frame
// (youth_icp_track_realign: the same plan again, then the persistent k_icp).

struct CoopState {
    const double* T_init;  // [pair][16] or null (identity)
    double* T64;           // [pair][16]
    float* T32;            // [pair][12]
    int32_t* status;       // [pair]
    double* stats;         // [pair][iters][2]
    float* T_out;          // [pair][16] fp32 4x4, or null
    unsigned* set;         // this call's counters: timeout word + prep counters
    unsigned* set_next;    // the next call's: zeroed here
    unsigned* head_err;    // k_icp's queue words: error/telemetry cleared for get_poses
    int iters, n_pairs, G, npx;  // G workgroups per pair, npx source pixels per lane
    // fused target prep (null: none): pair p's workgroups turn depth frame
    // prep_src + p N into record frame prep_out0 + p; prep_wait: those are
    // the records this launch gathers (hand-off before iteration 0), else
    // they are for a later launch (the tracker's next reference frame)
    const int16_t* prep_src;
    int prep_out0, prep_wait, prep_wide;
    // pair 0's result straight into pinned host memory (the tracker): fp64
    // 4x4 pose [16], then the status word; null: none
    double* res_host;
    // 1: workgroup c's source pixels are target tile c (kTileW x kCoopTileH,
    // = npx x kThreads pixels), the tile it preps, so its iteration-0 gathers
    // (small motion) hit records it has just written; 0: a contiguous run
    int tile_src;
    // tracker micro-batch (chain = 1; youth_icp_track_submit_batch): pairs
    // (f_{p-1}, f_p) of consecutive frames.  Pair p preps its own source
    // frame f_p into record frame prep_slot[p]; its target records are record
    // frame tgt_slot[p]: pair 0 the reference, pair p >= 1 the frame pair p-1
    // preps in this launch, so pair p waits for pair p-1's prep counter.
    // Pair p's result goes to the pinned slot res_pair[p].
    int chain;
    int tgt_slot[kCoopMaxChain], prep_slot[kCoopMaxChain];
    double* res_pair[kCoopMaxChain];
    // partial rows: this call's arena [kCoopBufs][part_cap][kPartStride]
    // (row p G + c), every row EMPTY at launch; the other arena, whose first
    // part_reset rows of every buffer (the previous call's) are reset here
    double* part;
    double* part_next;
    int part_cap, part_reset;
    int poll_delay;  // x 64 clocks before the first pass over the rows
    unsigned spin_max;  // polls before a wait gives up (kCoopSpinMax; the test hook's less)
    int stall_chunk;    // test hook: this chunk of pair 0 never stores iteration stall_iter's row (-1: none)
    int stall_iter;
};

// Phase timestamps for tools/coopbench only (never in the product build):
// thread 0 of every workgroup records s_memrealtime (100 MHz) at 8 points of
// each iteration into coop_phase[block][iteration][16] (slots 8-10: solve).
#ifdef YOUTH_COOP_PHASES
__device__ unsigned long long* coop_phase;
#define COOP_MARK(k, slot)                                                           \
    do {                                                                             \
        if (threadIdx.x == 0 && coop_phase && (k) < 32)                              \
            coop_phase[((size_t)blockIdx.x * 32 + (k)) * 16 + (slot)] =              \
                __builtin_amdgcn_s_memrealtime();                                    \
    } while (0)
#define COOP_MARK_WAVE(k, slot)                                                      \
    do {                                                                             \
        if ((threadIdx.x & 63) == 0 && threadIdx.x && coop_phase && (k) < 32)       \
            coop_phase[((size_t)blockIdx.x * 32 + (k)) * 16 + (slot)] =              \
                __builtin_amdgcn_s_memrealtime();                                    \
    } while (0)
#else
#define COOP_MARK(k, slot) \
    do {                   \
    } while (0)
#define COOP_MARK_WAVE(k, slot) \
    do {                        \
    } while (0)
#endif

// sum_pair_rows for k_icp_coop's counter-free hand-off: the same loads, sums
// and order, but every 16-byte piece that still holds EMPTY (its row not
// stored yet) is loaded again until none does.  The sums are those of
// sum_pair_rows over the same rows, bit for bit.  Every spin is bounded: a
// thread that passes spin_max polls, or finds the timeout word set, sets
// it and `stop` comes back non-zero in every thread (the caller stops).
template <int kBatch>
__device__ __forceinline__ double sum_pair_rows_polled(__amdgpu_buffer_rsrc_t rpart, int nblk,
                                                       double (*colsum)[kPartStride],
                                                       unsigned* err, int* sh_stop, int delay,
                                                       unsigned spin_max, int& stop)
{
    // rows land about when this workgroup's own did: the first pass waits
    // `delay` x 64 clocks so that it finds most of them (a pass over EMPTY
    // rows is traffic every workgroup pays again)
    int d = delay;
    for (; d >= 8; d -= 8) __builtin_amdgcn_s_sleep(8);
    for (; d > 0; --d) __builtin_amdgcn_s_sleep(1);
    const int t = threadIdx.x;
    const int j = t / kPieces, q = t - j * kPieces;
    int mine = 0;
    if (j < kSumCols) {
        double s0 = 0.0, s1 = 0.0;
        for (int bb = j; bb < nblk; bb += kBatch * kSumCols) {
            u4v v[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                const int b = bb + i * kSumCols;
                // aux 16 = sc1 (bypass this CU's L1: written by other CUs)
                v[i] = b < nblk ? __builtin_bit_cast(
                                      u4v, __builtin_amdgcn_raw_buffer_load_b128(
                                               rpart, (b * kPartStride + 2 * q) * 8, 0, 16))
                                : u4v{0u, 0u, 0u, 0u};
            }
            unsigned spins = 0;
            for (;;) {
                bool miss = false;
#pragma unroll
                for (int i = 0; i < kBatch; ++i) {
                    if (v[i].y == kPartEmptyHi || v[i].w == kPartEmptyHi) {  // pad rows are 0
                        miss = true;
                        // volatile (aux bit 31; emitted as sc0 sc1): the
                        // optimiser must re-issue every re-poll (a non-volatile
                        // one was once left out of a loop: DESIGN.md §9 1b)
                        v[i] = __builtin_bit_cast(
                            u4v, __builtin_amdgcn_raw_buffer_load_b128(
                                     rpart, ((bb + i * kSumCols) * kPartStride + 2 * q) * 8, 0,
                                     (int)(16u | 0x80000000u)));
                    }
                }
                if (!miss) break;
                if (++spins > spin_max || ((spins & 63u) == 0u && ld_u32_sc1(err) != 0u)) {
                    __hip_atomic_fetch_or(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    mine = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            double a0[kBatch], a1[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                a0[i] = __hiloint2double((int)v[i].y, (int)v[i].x);
                a1[i] = __hiloint2double((int)v[i].w, (int)v[i].z);
            }
            s0 += tree_sum<kBatch>(a0);
            s1 += tree_sum<kBatch>(a1);
        }
        colsum[j][2 * q] = s0;
        colsum[j][2 * q + 1] = s1;
    }
    // stop: sh_stop is 0 while the loop runs and is only ever set to 1 (every
    // thread then leaves the loop), so no reset is needed
    if (mine) *sh_stop = 1;
    __syncthreads();
    stop = __builtin_amdgcn_readfirstlane(*sh_stop);
    double tsum = 0.0;
    if (t < kNeq) {
        double c[kSumCols];
#pragma unroll
        for (int jj = 0; jj < kSumCols; ++jj) c[jj] = colsum[jj][t];
        tsum = tree_sum<kSumCols>(c);
    }
    return tsum;
}

// Spec a7-a9 for Q source pixels already back-projected (px = pixel slots
// s0 .. s0+Q-1 of this lane in the LDS planes X/Y/Z [slot][256]): transform,
// project, Q record gathers back to back, residual, Jacobian, exact products
// into the fp64 accumulators.  Same expressions as accumulate_chunk.
template <int kSp, bool kFast, int Q, int kThreads, typename A>
__device__ __forceinline__ void coop_group(const float* __restrict__ X, const float* __restrict__ Y,
                                           const float* __restrict__ Z, int s0, const float* T,
                                           __amdgpu_buffer_rsrc_t rrec, int W, int H,
                                           const Intr& K, const FastK& F, float thr2,
                                           A* acc, int& nmatch)
{
    const int t = threadIdx.x;
    float qx[Q], qy[Q], qz[Q], fu[Q], fv[Q];
    LaneMask in[Q];
    int j[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float sx = X[(s0 + q) * kThreads + t];
        const float sy = Y[(s0 + q) * kThreads + t];
        const float sz = Z[(s0 + q) * kThreads + t];
        xform_project<kSp>(T, sx, sy, sz, K, W, H, qx[q], qy[q], qz[q], fu[q], fv[q], in[q], j[q]);
    }
    f4v rec[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q)
        // aux 16 = sc1: the records come from this launch's fused prep (sc1
        // stores, drained, sharded counter) and are read ONLY by sc1 loads, so
        // no agent acquire is needed after the prep wait (MI355X_MICROARCH.md
        // "Valid forms", table row 1; L1 hits were worth less than the
        // acquire: C2 15.9 -> 16.4 K, profiles/r05/c2ab_r5zc_sc1_gathers.txt)
        rec[q] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rrec, (int)((unsigned)j[q] * 16u), 0, 16));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        nmatch += __builtin_popcountll(match_accumulate<kSp, kFast, false>(
            qx[q], qy[q], qz[q], rec[q], fu[q], fv[q], in[q], K, F, thr2, acc));  // per wave
    }
}

// Pixels per lane cs.npx is a launch parameter: the host picks it so the
// n_pairs x G workgroups spread over every CU (the pixel phase of one wave
// is latency-bound, so it costs ~npx x the per-pixel chain: DESIGN.md §5);
// kThreads = 512 puts two waves on each SIMD to hide that latency.  Lane t
// of chunk c owns source pixels c kThreads npx + s kThreads + t, s < npx;
// their back-projected X/Y/Z live in dynamic LDS [3][npx][kThreads] for the
// whole launch.
template <int kSp, bool kFast, int kThreads, int kTH>
__global__ __launch_bounds__(kThreads, 2) void k_icp_coop(const int16_t* __restrict__ dsrc,
                                                             const float4* __restrict__ recs,
                                                             size_t P, PairMap pm, int W, int H,
                                                             Intr K, FastK F, float thr2,
                                                             CoopState cs)
{
    extern __shared__ float coop_src[];  // [3][npx][kThreads]
    __shared__ float sPX[(kTH + 2) * kLdsW];  // fused prep neighbourhood
    __shared__ float sPY[(kTH + 2) * kLdsW];
    __shared__ float sPZ[(kTH + 2) * kLdsW];
    __shared__ double red[kThreads / 64][kNeq];
    __shared__ double colsum[kSumCols][kPartStride];
    __shared__ double sh_neq[kNeq];
    __shared__ double sh_T64[12];
    __shared__ float sh_T[12];
    __shared__ int sh_stop;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int G = cs.G;
    const int npx = cs.npx;
    const int p = blockIdx.x / G;
    const int c = blockIdx.x - p * G;
    const int N = W * H;
    unsigned* err = cs.set + kCoopErrWord;
    unsigned* prep_cnt = cs.set + kCoopPrepWords + (size_t)p * kCoopPrepPair;
    // the prep counter this pair waits on: its own (prep_wait), or in a
    // tracker chain the previous pair's (whose prep is this pair's target)
    const bool prep_wait = cs.chain ? p > 0 : cs.prep_wait != 0;
    unsigned* wait_cnt = cs.chain ? prep_cnt - kCoopPrepPair : prep_cnt;
    const int tgt_frame = cs.chain ? cs.tgt_slot[p] : pm.tgt0 + p;
    float* X = coop_src;
    float* Y = coop_src + npx * kThreads;
    float* Z = coop_src + 2 * npx * kThreads;

    COOP_MARK(3, 15);  // prologue stamps: kernel entry (slot 15 of iterations 3, 0, 1, 2)
    if (blockIdx.x == 0) {
        // the next call's words: the timeout word and every prep shard word
        // (word 0 of each 128-B line; the rest of a line is never used)
        for (int i = threadIdx.x; i < 1 + kCoopMaxPairs * kCoopPrepShards; i += kThreads)
            st_u32_sc1(cs.set_next + (i == 0 ? kCoopErrWord
                                             : kCoopPrepWords + (i - 1) * kCoopShardStride),
                       0u);
        if (threadIdx.x == 0) {
            st_u32_sc1(cs.head_err + kQError, 0u);
            st_u32_sc1(cs.head_err + kQSpins, 0u);
            st_u32_sc1(cs.head_err + kQWaited, 0u);
        }
    }
    // the previous call's partial rows (the other arena) back to EMPTY, for
    // the next call; spread over the whole grid
    if (cs.part_reset > 0) {
        const unsigned per = (unsigned)cs.part_reset * kPartStride;  // doubles per buffer
        const unsigned stride = gridDim.x * kThreads;
        for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < kCoopBufs * per; i += stride) {
            const unsigned b = i / per;
            st_u64_sc1(cs.part_next + (size_t)b * cs.part_cap * kPartStride + (i - b * per),
                       kPartEmpty);
        }
    }
    if (threadIdx.x < 12) {
        const double v = cs.T_init ? cs.T_init[(size_t)p * 16 + threadIdx.x]
                                   : ((threadIdx.x % 5) == 0 ? 1.0 : 0.0);
        sh_T64[threadIdx.x] = v;
        sh_T[threadIdx.x] = (float)v;
    }
    // ---- fused target prep: tiles c, c + G, ... of pair p's target frame,
    // records stored write-through (sc1); every storing wave drains, then
    // one arrival on the pair's prep counter (R1 hand-off)
    if (cs.prep_src) {
        const int tiles_x = (W + kTileW - 1) / kTileW;
        const int tiles = tiles_x * ((H + kTH - 1) / kTH);
        const int16_t* tdep = cs.prep_src + (size_t)p * N;
        float4* R = const_cast<float4*>(recs) +
                    (size_t)(cs.chain ? cs.prep_slot[p] : cs.prep_out0 + p) * P;
        for (int t = c; t < tiles; t += G) {  // uniform per workgroup
            const int ty = t / tiles_x;
            const int x0 = (t - ty * tiles_x) * kTileW, y0 = ty * kTH;
            if (cs.prep_wide)
                prep_tile<kFast, true, true, kThreads, kTH>(tdep, R, W, H, P, K, F, nullptr,
                                                                   x0, y0, sPX, sPY, sPZ);
            else
                prep_tile<kFast, false, true, kThreads, kTH>(tdep, R, W, H, P, K, F,
                                                                    nullptr, x0, y0, sPX, sPY, sPZ);
            __syncthreads();  // LDS planes reused by the next tile
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
        __syncthreads();
        if ((cs.prep_wait || cs.chain) && threadIdx.x == 0)
            __hip_atomic_fetch_add(prep_cnt + (c & (kCoopPrepShards - 1)) * kCoopShardStride, 1u,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    COOP_MARK(0, 15);  // prep published
    // ---- this workgroup's source pixels, back-projected once (spec a2)
    {
        const int16_t* sD = dsrc + (size_t)(pm.src0 + p) * N;
        const int base = c * npx * kThreads + threadIdx.x;
        const int tiles_x = (W + kTileW - 1) / kTileW;
        const int tyc = c / tiles_x;
        const int tx0 = (c - tyc * tiles_x) * kTileW, ty0 = tyc * kTH;
        for (int s = 0; s < npx; ++s) {
            int u, v;
            bool inr;
            if (cs.tile_src) {
                const int k = s * kThreads + threadIdx.x;
                u = tx0 + (k & (kTileW - 1));
                v = ty0 + k / kTileW;
                inr = u < W && v < H;
            } else {
                const int i = base + s * kThreads;
                inr = i < N;
                v = inr ? i / W : 0;
                u = inr ? i - v * W : 0;
            }
            const int d = inr ? (int)sD[(size_t)v * W + u] : 0;
            float x, y, z;
            backproject<kFast>(d, inr ? u : 0, inr ? v : 0, K, F, x, y, z);
            X[s * kThreads + threadIdx.x] = x;
            Y[s * kThreads + threadIdx.x] = y;
            Z[s * kThreads + threadIdx.x] = z;
        }
    }
    const __amdgpu_buffer_rsrc_t rrec = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(recs + (size_t)tgt_frame * P), (short)0,
        (int)(P * sizeof(float4)), 0x00020000);
    const size_t buf_stride = (size_t)cs.part_cap * kPartStride;  // doubles per buffer
    double* const part0 = cs.part + (size_t)p * G * kPartStride;  // pair p's rows, buffer 0
    int32_t st_acc = 0;
    bool timeout = false;
    COOP_MARK(1, 15);  // source pixels staged
    if (cs.prep_src && prep_wait) {
        // every workgroup of pair p prepped its tiles: ONE relaxed poll (lane
        // s of wave 0 polls shard s, which counts the chunks c = s mod 8);
        // the other waves load after the barrier below, and every gather of
        // the records is an sc1 load (coop_group), so no acquire follows
        if (wave == 0) {
            const unsigned want = lane < kCoopPrepShards
                                      ? (unsigned)((G - lane + kCoopPrepShards - 1) / kCoopPrepShards)
                                      : 0u;
            unsigned spins = 0;
            int stop = 0;
            for (;;) {
                const unsigned have =
                    lane < kCoopPrepShards ? ld_u32_sc1(wait_cnt + lane * kCoopShardStride) : 0u;
                if (__ballot(have < want) == 0ull) break;
                __builtin_amdgcn_s_sleep(1);
                if (++spins > cs.spin_max || ld_u32_sc1(err) != 0u) {
                    if (lane == 0)
                        __hip_atomic_fetch_or(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    stop = 1;
                    break;
                }
            }
            if (lane == 0) sh_stop = stop;
        }
        __syncthreads();
        timeout = __builtin_amdgcn_readfirstlane(sh_stop) != 0;
    } else {
        if (threadIdx.x == 0) sh_stop = 0;
        __syncthreads();
    }

    COOP_MARK(2, 15);  // every record of the pair visible
    for (int k = 0; k < cs.iters && !timeout; ++k) {
        COOP_MARK(k, 0);
        float T[12];
#pragma unroll
        for (int q = 0; q < 12; ++q)
            T[q] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh_T[q])));
        double acc[kNeq];
        // lane32: the lane's fp32 sums over its npx pixels, converted once
        typedef std::conditional_t<sp_lane32(kSp), float, double> A;
        A la[28];
#pragma unroll
        for (int q = 0; q < 28; ++q) la[q] = A(0);
        int nmatch = 0;
        int s0 = 0;
        for (; s0 + 4 <= npx; s0 += 4)
            coop_group<kSp, kFast, 4, kThreads>(X, Y, Z, s0, T, rrec, W, H, K, F, thr2, la, nmatch);
        switch (npx - s0) {  // wave-uniform tail
        case 3: coop_group<kSp, kFast, 3, kThreads>(X, Y, Z, s0, T, rrec, W, H, K, F, thr2, la, nmatch); break;
        case 2: coop_group<kSp, kFast, 2, kThreads>(X, Y, Z, s0, T, rrec, W, H, K, F, thr2, la, nmatch); break;
        case 1: coop_group<kSp, kFast, 1, kThreads>(X, Y, Z, s0, T, rrec, W, H, K, F, thr2, la, nmatch); break;
        default: break;
        }
#pragma unroll
        for (int q = 0; q < 28; ++q) acc[q] = (double)la[q];
        acc[28] = lane == 0 ? (double)nmatch : 0.0;  // the wave's count, lane 0
        COOP_MARK(k, 1);
        if (wave < 4) COOP_MARK_WAVE(k, 11 + wave);  // slots 12-14: waves 1-3 pixel loop done
        {
            double tot;
            wave_reduce_scatter<kNeq>(acc, lane, tot);
            COOP_MARK(k, 11);
            if (!(lane & 1) && (lane >> 1) < kNeq) red[wave][lane >> 1] = tot;
        }
        __syncthreads();
        double* part = part0 + (size_t)(k % kCoopBufs) * buf_stride;
        COOP_MARK(k, 2);
        if (wave == 0) {
            // ---- store this chunk's partial row (sc1) over its EMPTY row.
            // The drain first: this wave's reset of its row of buffer
            // (k+1) % 3 (stored at iteration k-1) must be visible before any
            // value of iteration k is (see the hand-off above)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            double sum = 0.0;
            if (lane < kPartStride && !(k == cs.stall_iter && p == 0 && c == cs.stall_chunk)) {
                if (lane < kNeq) {  // the waves' sums as a pairwise tree (3 dependent adds)
                    double r[kThreads / 64];
#pragma unroll
                    for (int w = 0; w < kThreads / 64; ++w) r[w] = red[w][lane];
                    sum = tree_sum<kThreads / 64>(r);
                }
                st_u64_sc1(part + (size_t)c * kPartStride + lane,
                           (unsigned long long)__double_as_longlong(sum));
            }
            COOP_MARK(k, 3);
            COOP_MARK(k, 4);
        }
        COOP_MARK(k, 5);
        // ---- every workgroup sums the pair's partials in the same fixed
        // order, as soon as each row has landed (no counter, no barrier)
        const __amdgpu_buffer_rsrc_t rpart = __builtin_amdgcn_make_buffer_rsrc(
            part, (short)0, G * kPartStride * (int)sizeof(double), 0x00020000);
        int stop = 0;
        const double tsum = sum_pair_rows_polled<16>(rpart, G, colsum, err, &sh_stop,
                                                      cs.poll_delay, cs.spin_max, stop);
        COOP_MARK(k, 6);
        if (stop) {
            timeout = true;
            break;
        }
        if (wave == 0) {
            if (lane < kNeq) sh_neq[lane] = tsum;
            if (c == 0 && cs.stats && lane == 0) {
                cs.stats[((size_t)p * cs.iters + k) * 2 + 0] = readlane64(tsum, 28);
                cs.stats[((size_t)p * cs.iters + k) * 2 + 1] = readlane64(tsum, 27);
            }
            COOP_MARK(k, 8);
            st_acc |= solve_update_wave(sh_neq, sh_T64, sh_T, lane);
            COOP_MARK(k, 9);
            // every row of iteration k seen: every workgroup of the pair has
            // read iteration k-1's, so this row of that buffer ((k+2) % 3,
            // written next at iteration k+2) goes back to EMPTY now
            if (k + 2 < cs.iters && lane < kPartStride)
                st_u64_sc1(part0 + (size_t)((k + 2) % kCoopBufs) * buf_stride +
                               (size_t)c * kPartStride + lane,
                           kPartEmpty);
            COOP_MARK(k, 10);
        }
        __syncthreads();
        COOP_MARK(k, 7);
    }

    // ---- pair p's results, from its chunk-0 workgroup (replaces k_finish)
    if (c == 0 && threadIdx.x < 16) {
        const int i = threadIdx.x;
        const double v = i < 12 ? sh_T64[i]
                                : (cs.T_init ? cs.T_init[(size_t)p * 16 + i] : (i == 15 ? 1.0 : 0.0));
        cs.T64[(size_t)p * 16 + i] = v;
        if (i < 12) cs.T32[(size_t)p * 12 + i] = (float)v;
        if (cs.T_out) cs.T_out[(size_t)p * 16 + i] = i < 12 ? (float)v : (i == 15 ? 1.0f : 0.0f);
        const int32_t st = st_acc | (timeout ? YOUTH_STATUS_TIMEOUT : 0);
        if (i == 0) cs.status[p] = st;
        double* res = cs.chain ? cs.res_pair[p] : (p == 0 ? cs.res_host : nullptr);
        if (res) {
            // fine-grained pinned slot: system-scope stores go to host memory
            // past the L2, and the wave waits for them before it ends, so the
            // tracker's completion event needs no system-scope L2 writeback
            __hip_atomic_store(res + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (i == 0)
                __hip_atomic_store(reinterpret_cast<int32_t*>(res + 16), st,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __builtin_amdgcn_s_waitcnt(0);
        }
    }
}

// Copy out fp32 4x4 poses (optional) and fold a persistent-kernel timeout
// into every pair's status.
__global__ void k_finish(const double* __restrict__ T64, int n, float* __restrict__ out,
                         int32_t* __restrict__ status, const unsigned* __restrict__ error)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 16) return;
    const int i = t & 15;
    if (out) out[t] = i < 12 ? (float)T64[(size_t)(t >> 4) * 16 + i] : (i == 15 ? 1.0f : 0.0f);
    if (i == 0 && error && *error) status[t >> 4] |= YOUTH_STATUS_TIMEOUT;
}

// The tracker's H2D of m page-locked host frames, pulled by the GPU itself
// (the default; YOUTH_ICP_TRACK_COPY=sdma uses hipMemcpyAsync on the copy
// engine instead).  On the shared GPU hosts the SDMA path ran at 36-41 K
// frames/s in quiet passes but stalled the submitting thread inside
// hipMemcpyAsync for 8-18 ms about once in ten backlogged passes and fell to
// ~9 K frames/s while the host was loaded; this kernel's passes stayed within
// a few per cent of each other under the same conditions (DESIGN.md §6,
// profiles/r05/).  Few 64-lane workgroups (a total of ~32 per launch), four
// 16-byte loads in flight per lane, so its waves sit beside the resident
// cooperative grid of the launch before it without slowing it much.
struct FramePtrs {
    const int16_t* src[kCoopMaxChain];
};
__global__ __launch_bounds__(64) void k_pull_frames(FramePtrs fp, int16_t* __restrict__ dst, int N,
                                                    int m)
{
    const int f = blockIdx.y;
    if (f >= m) return;
    const int16_t* __restrict__ s16 = fp.src[f];
    int16_t* __restrict__ d16 = dst + (size_t)f * N;
    const int stride = gridDim.x * 64;
    const int t0 = blockIdx.x * 64 + threadIdx.x;
    // 16-byte body when both ends are 16-byte aligned (page-locked buffers
    // and W*H % 8 == 0 frames), else element by element
    const bool vec = (((uintptr_t)s16 | (uintptr_t)d16) & 15) == 0;
    int done = 0;
    if (vec) {
        typedef int v4i __attribute__((ext_vector_type(4)));
        const v4i* __restrict__ s = reinterpret_cast<const v4i*>(s16);
        v4i* __restrict__ d = reinterpret_cast<v4i*>(d16);
        const int nv = N / 8;
        int i = t0;
        for (; i + 3 * stride < nv; i += 4 * stride) {
            const v4i a = __builtin_nontemporal_load(s + i);
            const v4i b = __builtin_nontemporal_load(s + i + stride);
            const v4i c = __builtin_nontemporal_load(s + i + 2 * stride);
            const v4i e = __builtin_nontemporal_load(s + i + 3 * stride);
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

// Per-pair status of one chunk of the host batch API, the launch's timeout
// flag folded in (as youth_icp_get_poses does).
__global__ void k_status_out(const int32_t* __restrict__ status, int n,
                             const unsigned* __restrict__ error, int32_t* __restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = status[t] | (*error ? YOUTH_STATUS_TIMEOUT : 0);
}

}  // namespace

// ============================================================ launch layer ==
// Declared in icp_host.h; `static` what only this unit uses.

namespace youth_icp {

int reduce_geometry(const youth_icp_ctx* c, int n_pairs, int* chunk_out)
{
    // work chunks per iteration: fewer chunks make items wait for their
    // pair's pose, more pay the per-item hand-off.  Measured
    // best (tools/chunk_sweep.sh, profiles/r02/chunk_sweep.txt): ~2048 up to
    // 256 pairs per launch (64 pairs: +2.4 %, 128: +3.4 % over 3072), ~3072
    // above.  At least 8 pixels per lane.
    static const int knob = [] {
        const char* e = getenv("YOUTH_ICP_TARGET_CHUNKS");  // tuning knob
        const int v = e ? atoi(e) : 0;
        return v > 0 ? v : 0;
    }();
    // a context that shares the device with share - 1 concurrent ones runs on
    // 1/share of the workgroup slots, so it takes 1/share of the chunks: the
    // same items per workgroup and iteration (youth_icp_set_concurrency).
    // Shared, <= 96 pairs: 1536 / share (64 pairs, share 2: 768 chunks 81.6 K
    // aligns/s, 1024 81.1 K, 1280 79.9 K; profiles/r03/ab_share.txt)
    const int base = c->share > 1 && n_pairs <= 96 ? 1536 : (n_pairs <= 256 ? 2048 : 3072);
    const int target_blocks = (knob ? knob : base) / c->share;
    int nb = (target_blocks + n_pairs - 1) / n_pairs;
    const int max_nb = (c->N + 2 * kRedStep - 1) / (2 * kRedStep);
    if (nb > max_nb) nb = max_nb;
    if (nb < 1) nb = 1;
    return round_chunks(c->N, nb, chunk_out);
}

// k_icp_coop's partial-row arenas, every row EMPTY (k_icp_coop comment).  A
// call needing more rows than there are reallocates (hipFree waits for the
// device, so no launch still uses the old rows).  The EMPTY fill is enqueued
// on the launch's stream ahead of the launch; any later coop launch of this
// context is ordered after this one (coop_enqueue), so after the fill too.
static int ensure_coop_part(youth_icp_ctx* c, hipStream_t s, int rows)
{
    if (rows <= c->coop_part_cap) return YOUTH_OK;
    const int cap = std::max(rows, c->n_cu * 2);
    if (c->d_coop_part) HIP_TRY(hipFree(c->d_coop_part));
    c->d_coop_part = nullptr;
    c->coop_part_cap = 0;
    const size_t doubles = (size_t)2 * kCoopBufs * cap * kPartStride;
    HIP_TRY(hipMalloc(&c->d_coop_part, doubles * sizeof(double)));
    static_assert((unsigned)(kPartEmpty >> 32) == (unsigned)kPartEmpty, "EMPTY fills by words");
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->d_coop_part, (int)kPartEmptyHi, doubles * 2, s));
    c->coop_part_cap = cap;
    c->coop_part_rows[0] = c->coop_part_rows[1] = 0;
    return YOUTH_OK;
}

int ensure_partials(youth_icp_ctx* c, size_t doubles)
{
    return grow_device_buffer(g_icp_err, &c->d_partials, &c->partials_cap, doubles);
}

int ensure_stats(youth_icp_ctx* c, int iters)
{
    // two buffers of one capacity, stats_iters: the tickets grow on a copy of
    // it, and it is zero unless both hold that many iterations
    int arr_iters = c->stats_iters;
    const int rc = grow_device_buffer(g_icp_err, &c->d_arr_it, &arr_iters, iters, (size_t)c->max_frames);
    if (rc == YOUTH_OK)
        return grow_device_buffer(g_icp_err, &c->d_stats, &c->stats_iters, iters, (size_t)c->max_frames * 2);
    c->stats_iters = 0;
    return rc;
}

static int ensure_assoc(youth_icp_ctx* c)
{
    if (c->d_assoc) return YOUTH_OK;
    HIP_TRY(hipMalloc(&c->d_assoc, (size_t)c->max_frames * c->N * sizeof(int32_t)));
    return YOUTH_OK;
}

static int ensure_xyz(youth_icp_ctx* c)
{
    if (c->d_xyz) return YOUTH_OK;
    const size_t bytes = 3 * c->P * sizeof(float) * (size_t)c->max_frames;
    HIP_TRY(hipMalloc(&c->d_xyz, bytes));
    HIP_TRY(hipMemset(c->d_xyz, 0, bytes));
    return YOUTH_OK;
}

static int ev_begin(youth_icp_ctx* c, hipStream_t s, EventPair* ep, int kind)
{
    ep->a = nullptr;
    if (!c->timing || (c->timing_iter_only && kind != 0)) return YOUTH_OK;
    if (c->ev_free.empty()) {
        EventPair e{};
        HIP_TRY(hipEventCreate(&e.a));
        HIP_TRY(hipEventCreate(&e.b));
        c->ev_free.push_back(e);
    }
    *ep = c->ev_free.back();
    c->ev_free.pop_back();
    ep->kind = kind;
    HIP_TRY(hipEventRecord(ep->a, s));
    return YOUTH_OK;
}

static int ev_end(youth_icp_ctx* c, hipStream_t s, EventPair* ep)
{
    if (!c->timing || !ep->a) return YOUTH_OK;
    HIP_TRY(hipEventRecord(ep->b, s));
    c->ev_live.push_back(*ep);
    return YOUTH_OK;
}

int ev_harvest(youth_icp_ctx* c)
{
    for (auto& e : c->ev_live) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        c->t_ms[e.kind] += ms;
        c->t_n[e.kind] += 1;
        c->ev_free.push_back(e);
    }
    c->ev_live.clear();
    return YOUTH_OK;
}

// init (nullable): the persistent path's per-call state, set by the same launch.
static int launch_prep_with(youth_icp_ctx* c, hipStream_t s, const int16_t* depth, int n_frames,
                            int out0, bool want_xyz, const InitArgs* init)
{
    if (n_frames <= 0) return YOUTH_OK;
    if (want_xyz) {
        int rc = ensure_xyz(c);
        if (rc) return rc;
    }
    const int tiles_x = (c->W + kPrepTW - 1) / kPrepTW, tiles_y = (c->H + kPrepTH - 1) / kPrepTH;
    const long long rows = (long long)tiles_y * n_frames;
    const long long blocks = (long long)tiles_x * (c->prep_xcd_map == 2 ? (rows + 7) / 8 * 8 : rows);
    if (blocks > 0x7fffffffLL) return g_icp_err.set(YOUTH_EINVAL, "launch_prep: %lld tiles", blocks);
    EventPair ep{};
    int rc = ev_begin(c, s, &ep, 2);
    if (rc) return rc;
    float* xyz = want_xyz ? c->d_xyz : nullptr;
    const bool wide = (c->W % 4 == 0) && (reinterpret_cast<uintptr_t>(depth) % 8 == 0);
    auto kern = c->fast ? (wide ? k_prep<true, true> : k_prep<true, false>)
                        : (wide ? k_prep<false, true> : k_prep<false, false>);
    const InitArgs ia = init ? *init : InitArgs{};
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kPrepThreads), 0, s, depth, out0, c->W,
                       c->H, c->P, c->K, c->F, c->d_rec, xyz, ia, tiles_x, tiles_y, n_frames,
                       c->prep_xcd_map);
    HIP_TRY(hipGetLastError());
    return ev_end(c, s, &ep);
}

// k_prep_ident<spec, fast> by index spec 2 + fast
typedef void (*PrepIdentKernel)(const int16_t*, int, int, int, size_t, Intr, FastK, float4*,
                                IdentArgs, int, int, int);
static PrepIdentKernel prep_ident_kernel(int idx)
{
    static const PrepIdentKernel tab[4] = {k_prep_ident<0, false>, k_prep_ident<0, true>,
                                           k_prep_ident<1, false>, k_prep_ident<1, true>};
    return tab[idx & 3];
}

// The prep job with iteration 0 of every pair inside it (k_prep_ident); nb:
// k_icp's chunks per pair, which share the partial rows.
static int launch_prep_ident(youth_icp_ctx* c, hipStream_t s, const PrepJob* job,
                             const int16_t* dsrc, PairMap pm, int n_pairs, int iters, float thr2,
                             int nb, float* d_T_out)
{
    const int blocks_x = (c->W + kPrepColW - 1) / kPrepColW;
    // Rows per unit: a longer band means fewer halo rows, unit starts (one
    // memory round trip before the first row), reductions and publishes, but
    // fewer waves to balance over the chip.  Measured at 640x480
    // (profiles/colprep/band_sweep.txt): at 512 pairs 24 rows 87.4 K aligns/s,
    // 48 88.3, 96 88.5, 120 88.4, 160 88.5, 240 88.2, 480 88.4; at 64, 128 and
    // 256 pairs the long bands win too (64 pairs: 24 rows 79.1, 48 81.4, 96
    // 81.5, 160 81.6, with 1,920 units on 4,096 wave slots), so a small batch
    // does not shorten its bands to fill the chip as the tile form shortened
    // its strips.  Below 64 pairs nothing is measured: there the band shortens
    // until the grid holds one wave per SIMD, but not below 24 rows.
    int band = c->prep_band;
    if (band <= 0) {
        const long long rows = (long long)c->H * blocks_x * job->n / (4LL * c->n_cu);
        band = (int)std::max<long long>(std::min<long long>(kPrepBand, rows), 24);
    }
    band = std::min(band, c->H);
    const int bands = (c->H + band - 1) / band;
    const int per = blocks_x * bands;  // units, and partial rows, per frame
    const long long blocks = (long long)per * job->n;
    if (blocks > 0x7fffffffLL) return g_icp_err.set(YOUTH_EINVAL, "launch_prep: %lld units", blocks);
    int rc = ensure_partials(c, (size_t)std::max(nb, per) * n_pairs * kPartStride);
    if (rc) return rc;
    EventPair ep{};
    rc = ev_begin(c, s, &ep, 2);
    if (rc) return rc;
    const IdentArgs ia{dsrc,      pm,        n_pairs,     iters,      thr2,
                       c->d_partials, c->d_T64, c->d_T32,  c->d_status, c->d_stats,
                       c->d_epoch, c->d_arr_it, c->d_arrivals, d_T_out,  c->d_head};
    auto kern = prep_ident_kernel(c->spec * 2 + (c->fast ? 1 : 0));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kPrepColW), 0, s, job->depth, job->out0,
                       c->W, c->H, c->P, c->K, c->F, c->d_rec, ia, blocks_x, bands, band);
    HIP_TRY(hipGetLastError());
    return ev_end(c, s, &ep);
}

int launch_prep(youth_icp_ctx* c, hipStream_t s, const int16_t* depth, int n_frames, int out0,
                bool want_xyz)
{
    return launch_prep_with(c, s, depth, n_frames, out0, want_xyz, nullptr);
}

template <int kSp, bool kAssoc, bool kFast, bool kAligned, bool kFuse>
static void launch_reduce_t(youth_icp_ctx* c, hipStream_t s, dim3 grid, const int16_t* dsrc,
                            PairMap pm, float thr2, int chunk, const PoseState& ps)
{
    hipLaunchKernelGGL((k_reduce<kSp, kAssoc, kFast, kAligned, kFuse>), grid, dim3(kRedThreads), 0,
                       s, dsrc, c->d_rec, c->P, pm, c->W, c->H, c->K, c->F, thr2, chunk,
                       c->d_partials, kAssoc ? c->d_assoc : (int32_t*)nullptr, ps);
}

// sel = assoc 8 | fuse 4 | fast 2 | aligned 1 (assoc with fuse excluded)
template <int kSp>
static void launch_reduce_sel(youth_icp_ctx* c, hipStream_t s, dim3 grid, const int16_t* dsrc,
                              PairMap pm, float thr2, int chunk, const PoseState& ps, int sel)
{
    switch (sel) {
    case 0: launch_reduce_t<kSp, false, false, false, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 1: launch_reduce_t<kSp, false, false, true, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 2: launch_reduce_t<kSp, false, true, false, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 3: launch_reduce_t<kSp, false, true, true, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 4: launch_reduce_t<kSp, false, false, false, true>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 5: launch_reduce_t<kSp, false, false, true, true>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 6: launch_reduce_t<kSp, false, true, false, true>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 7: launch_reduce_t<kSp, false, true, true, true>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 8: launch_reduce_t<kSp, true, false, false, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 9: launch_reduce_t<kSp, true, false, true, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    case 10: launch_reduce_t<kSp, true, true, false, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    default: launch_reduce_t<kSp, true, true, true, false>(c, s, grid, dsrc, pm, thr2, chunk, ps); break;
    }
}

int launch_reduce(youth_icp_ctx* c, hipStream_t s, const int16_t* dsrc, int src0, int tgt0,
                  int n_pairs, bool assoc, int* nblk_out, int fuse_it)
{
    const PairMap pm{src0, tgt0};
    int chunk = 0;
    const int nb = reduce_geometry(c, n_pairs, &chunk);
    int rc = ensure_partials(c, (size_t)nb * n_pairs * kNeq);
    if (rc) return rc;
    if (assoc) {
        rc = ensure_assoc(c);
        if (rc) return rc;
    }
    const float thr2 = c->prm.dist_thresh * c->prm.dist_thresh;
    const bool aligned = (reinterpret_cast<uintptr_t>(dsrc) % 8 == 0) && (c->W % 4 == 0) &&
                           c->centred_exact;
    dim3 grid(nb, n_pairs);
    EventPair ep{};
    rc = ev_begin(c, s, &ep, 0);
    if (rc) return rc;
    const PoseState ps{c->d_T64, c->d_T32, c->d_status, c->d_stats, c->d_arrivals,
                       fuse_it < 0 ? 0 : fuse_it, c->prm.iters};
    const bool fuse = fuse_it >= 0;
    if (assoc && fuse) return g_icp_err.set(YOUTH_EINVAL, "launch_reduce: assoc with fused solve");
    const int sel = (assoc ? 8 : 0) | (fuse ? 4 : 0) | (c->fast ? 2 : 0) | (aligned ? 1 : 0);
    switch (variant(c)) {
    case 0: launch_reduce_sel<0>(c, s, grid, dsrc, pm, thr2, chunk, ps, sel); break;
    case 1: launch_reduce_sel<1>(c, s, grid, dsrc, pm, thr2, chunk, ps, sel); break;
    case 2: launch_reduce_sel<2>(c, s, grid, dsrc, pm, thr2, chunk, ps, sel); break;
    default: launch_reduce_sel<3>(c, s, grid, dsrc, pm, thr2, chunk, ps, sel); break;
    }
    HIP_TRY(hipGetLastError());
    c->lanes = youth_lanes{YOUTH_LANES_STRIDED, chunk, kRedThreads, 0};
    c->has_lanes = true;
    c->lanes_mixed = false;
    *nblk_out = nb;
    return ev_end(c, s, &ep);
}

// Small-batch plan.  One wave per SIMD issues a wave64 instruction in >= 4
// cycles, so a pair's pixel phase costs ~ npx x (workgroups per CU): pick
// the npx (source pixels per lane) minimising npx x ceil(n_pairs G / CUs)
// among those whose n_pairs x G workgroups fit the co-resident capacity with
// one block per CU to spare (cooperative launch admission,
// MI355X_MICROARCH.md); ties go to the larger npx (fewer partials to sum).
static size_t coop_lds(int npx, int threads) { return (size_t)3 * npx * threads * sizeof(float); }

bool coop_plan(const youth_icp_ctx* c, int n_pairs, int* npx_out, int* G_out)
{
    if (!c->coop || n_pairs > c->coop_max_pairs || n_pairs > kCoopMaxPairs) return false;
    const int v = variant(c) * 2 + (c->fast ? 1 : 0);
    long long best = -1;
    for (int npx = 1; npx <= kCoopMaxPx; ++npx) {
        if (c->coop_px && npx != c->coop_px) continue;
        const int chunk = npx * c->coop_threads;
        const int G = (c->N + chunk - 1) / chunk;
        const long long wgs = (long long)G * n_pairs;
        // VGPR-limited occupancy: k_icp_coop's SGPR count (106) admits 6
        // 256-thread blocks per CU (MI355X_MICROARCH.md residency formula),
        // more than the API's VGPR answer, so the API count is exact here
        const int bpc = c->coop_bpc[c->coop_threads == 256][v][npx];
        if (bpc < 1 || wgs > (long long)c->n_cu * bpc) continue;
        const long long cost = (long long)npx * ((wgs + c->n_cu - 1) / c->n_cu);
        if (best < 0 || cost <= best) {
            best = cost;
            *npx_out = npx;
            *G_out = G;
        }
    }
    return best >= 0;
}

template <int kSp>
static const void* coop_kernel_t(bool fast, int threads, bool tall)
{
    if (threads == 256)
        return fast ? (const void*)k_icp_coop<kSp, true, 256, kCoopTileH>
                    : (const void*)k_icp_coop<kSp, false, 256, kCoopTileH>;
    if (tall)
        return fast ? (const void*)k_icp_coop<kSp, true, 512, kCoopTileHTall>
                    : (const void*)k_icp_coop<kSp, false, 512, kCoopTileHTall>;
    return fast ? (const void*)k_icp_coop<kSp, true, 512, kCoopTileH>
                : (const void*)k_icp_coop<kSp, false, 512, kCoopTileH>;
}

static const void* coop_kernel(int var, bool fast, int threads, bool tall = false)
{
    switch (var) {
    case 0: return coop_kernel_t<0>(fast, threads, tall);
    case 1: return coop_kernel_t<1>(fast, threads, tall);
    case 2: return coop_kernel_t<2>(fast, threads, tall);
    default: return coop_kernel_t<3>(fast, threads, tall);
    }
}


// k_icp_coop's workgroups poll each other, so all n_pairs x G of them must be
// resident together.  The planner sizes the grid to the co-resident capacity
// of an idle device; what remains is another spin-waiting grid occupying the
// CUs at the same time.  In this library that can only be another
// k_icp_coop (k_icp never waits on a workgroup that is not running), so the
// cooperative launches of a device are totally ordered instead, and launched
// as plain kernels: hipLaunchCooperativeKernel's runtime path costs ~20 us
// per launch on ROCm 7 (single-pair aligns/s 9.2 K against 11.3 K,
// profiles/r02/stream_probe.txt).
//   * While every coop launch of the device has come from ONE stream, stream
//     order is the total order: no extra packet.
//   * The first launch from a second stream switches the device to ordered
//     mode for good: the host waits once for the device to drain (the
//     previous stream's last coop grid included; that stream's handle is not
//     touched, the caller may have destroyed it), and from then on every
//     coop launch records the device's
//     completion event and waits on it when its stream differs from the
//     previous launch's (an event record costs ~2.7 us per launch: 10.9 K).
// YOUTH_ICP_COOP_LAUNCH=runtime restores hipLaunchCooperativeKernel.
struct CoopOrder {
    std::mutex mu;
    std::condition_variable cv;  // launches wait while the one-time drain runs
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;
    bool any = false;
    bool multi = false;     // launches seen from more than one stream
    bool draining = false;  // the first switch's device drain is in progress (mu released)
};
static CoopOrder g_coop_order[64];

static int coop_enqueue(youth_icp_ctx* c, hipStream_t s, void** args, int blocks, int npx,
                        bool tall)
{
    const void* kern = coop_kernel(variant(c), c->fast, c->coop_threads, tall);
    const dim3 grid((unsigned)blocks), block(c->coop_threads);
    const unsigned lds = (unsigned)coop_lds(npx, c->coop_threads);
    if (c->coop_refuse)  // test hook: the runtime's refusal, nothing enqueued
        return g_icp_err.set(YOUTH_EHIP, "coop_enqueue: cooperative launch refused (test hook)");
    if (c->coop_launch == 1) {
        HIP_TRY(hipLaunchCooperativeKernel(kern, grid, block, args, lds, s));
        return YOUTH_OK;
    }
    if (c->coop_launch == 2 || c->device < 0 || c->device >= 64) {  // unordered (probe only)
        HIP_TRY(hipLaunchKernel(kern, grid, block, args, lds, s));
        return YOUTH_OK;
    }
    CoopOrder& o = g_coop_order[c->device];
    std::unique_lock<std::mutex> lk(o.mu);
    o.cv.wait(lk, [&o] { return !o.draining; });
    if (o.any && o.last != s) {
        if (!o.done) HIP_TRY(hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
        if (!o.multi) {
            // first switch: the previous stream may be a caller's stream that
            // has been destroyed since, so its handle is not used again
            // (ADVICE r3); the host waits once for the device to drain, which
            // covers that stream's last coop grid.  The drain runs without
            // holding mu: other threads' coop launches on this
            // device wait on cv meanwhile (none may start before it ends),
            // nothing else is blocked.  From now on every launch records
            // `done` on its own stream right after it
            o.draining = true;
            lk.unlock();
            const hipError_t e = hipDeviceSynchronize();
            lk.lock();
            o.draining = false;
            o.cv.notify_all();
            if (e != hipSuccess)
                return g_icp_err.set(YOUTH_EHIP, "coop launch: device drain on the first stream "
                                     "switch: %s", hipGetErrorString(e));
            o.multi = true;
        } else {
            HIP_TRY(hipStreamWaitEvent(s, o.done, 0));
        }
    }
    HIP_TRY(hipLaunchKernel(kern, grid, block, args, lds, s));
    if (o.multi) HIP_TRY(hipEventRecord(o.done, s));
    o.last = s;
    o.any = true;
    return YOUTH_OK;
}

static int launch_coop(youth_icp_ctx* c, hipStream_t s, const int16_t* dsrc, PairMap pm,
                       int n_pairs, const double* dTi, float* d_T_out, int npx, int G,
                       const PrepJob* job)
{
    const int iters = c->prm.iters;
    int rc = ensure_coop_part(c, s, n_pairs * G);
    if (rc) return rc;
    const int par = c->coop_par;
    unsigned* set = c->d_coop + (size_t)par * kCoopSetWords;
    unsigned* set_next = c->d_coop + (size_t)(par ^ 1) * kCoopSetWords;
    c->coop_par ^= 1;
    const bool wide = job && (c->W % 4 == 0) && (reinterpret_cast<uintptr_t>(job->depth) % 8 == 0);
    // tile-shaped source chunks when one target tile is exactly one
    // workgroup's pixels and the pair has one workgroup per tile: 64 x 24
    // tiles at 3 px per lane (640x480), 64 x 80 at 10 (1280x960; that
    // kernel's larger prep LDS must still admit the planned grid)
    auto tiles_of = [&](int th) {
        return ((c->W + kTileW - 1) / kTileW) * ((c->H + th - 1) / th);
    };
    const bool tall = c->coop_tile_src && c->coop_threads == 512 &&
                      npx * 512 == kTileW * kCoopTileHTall && G == tiles_of(kCoopTileHTall) &&
                      (long long)n_pairs * G <= (long long)c->n_cu * c->coop_bpc_tall[variant(c) * 2 + (c->fast ? 1 : 0)];
    const bool tile_src = tall || (c->coop_tile_src && npx * c->coop_threads == kTileW * kCoopTileH &&
                                   G == tiles_of(kCoopTileH));
    CoopState cs{dTi,      c->d_T64, c->d_T32, c->d_status,          c->d_stats,
                 d_T_out,  set,      set_next, c->d_head,            iters,
                 n_pairs,  G,        npx,      job ? job->depth : nullptr,
                 job ? job->out0 : 0, job && job->wait ? 1 : 0, wide ? 1 : 0,
                 c->coop_res_host, tile_src ? 1 : 0};
    if (job && job->chain) {
        cs.chain = 1;
        for (int i = 0; i < kCoopMaxChain; ++i) {
            cs.tgt_slot[i] = job->tgt_slot[i];
            cs.prep_slot[i] = job->prep_slot[i];
            cs.res_pair[i] = job->res[i];
        }
    }
    const size_t arena = (size_t)kCoopBufs * c->coop_part_cap * kPartStride;
    cs.part = c->d_coop_part + (size_t)par * arena;
    cs.part_next = c->d_coop_part + (size_t)(par ^ 1) * arena;
    cs.part_cap = c->coop_part_cap;
    cs.part_reset = c->coop_part_rows[par ^ 1];  // the previous call's rows
    // the first pass over the rows waits G / 8 x 64 clocks by default: the
    // rows' landing spread grows with the rows every workgroup loads
    // (profiles/r05/delay_sweep_r5s.txt, _r5t.txt: 640x480 (G 200) best at
    // 20-24, 1280x960 (G 240) at 28-32; no wait 13.7 K / 4.93 K aligns/s,
    // 24: 15.7 K / 5.32 K, 32: 15.3 K / 5.41 K; the tracker within noise)
    cs.poll_delay = c->coop_poll_delay >= 0 ? c->coop_poll_delay : G / 8;
    // test hook (YOUTH_ICP_TEST_COOP_STALL=<chunk>[:<launches>]): the
    // context's first coop launches lose one row, so their waits time out
    // after ~20 ms
    cs.stall_chunk = c->coop_stall_once;
    cs.stall_iter = c->coop_stall_iter;
    // a lost iteration-0 row is ended by the product's bound itself (the
    // test of it); a later one by the hook's shorter bound
    cs.spin_max = c->coop_stall_once >= 0 && c->coop_stall_iter != 0 ? 20000u : kCoopSpinMax;
    if (c->coop_stall_once >= 0 && --c->coop_stall_left <= 0) c->coop_stall_once = -1;
    const float4* recs = c->d_rec;
    size_t P = c->P;
    int W = c->W, H = c->H;
    Intr K = c->K;
    FastK F = c->F;
    float thr2 = c->prm.dist_thresh * c->prm.dist_thresh;
    void* args[] = {(void*)&dsrc, (void*)&recs, (void*)&P, (void*)&pm, (void*)&W, (void*)&H,
                    (void*)&K, (void*)&F, (void*)&thr2, (void*)&cs};
    EventPair ep{};
    rc = ev_begin(c, s, &ep, 0);
    if (rc) return rc;
    rc = coop_enqueue(c, s, args, n_pairs * G, npx, tall);
    if (rc) {
        c->coop_par = par;  // nothing ran: the sets and arenas stay as they were
        return rc;
    }
    c->coop_part_rows[par ^ 1] = 0;          // reset by this launch
    c->coop_part_rows[par] = n_pairs * G;    // dirtied by it
    c->last_coop_G = G;
    c->last_coop_px = npx;
    c->lanes = youth_lanes{tile_src ? YOUTH_LANES_COOP_TILE : YOUTH_LANES_COOP, npx * c->coop_threads,
                           c->coop_threads, npx};
    c->has_lanes = true;
    c->lanes_mixed = false;
    return ev_end(c, s, &ep);
}

// k_icp<variant, fast, aligned> by index variant 4 + fast 2 + aligned
typedef void (*IcpKernel)(const int16_t*, const float4*, size_t, PairMap, int, int, Intr, FastK,
                          float, double*, IterState);
static IcpKernel icp_kernel(int var)
{
    static const IcpKernel tab[4 * kVariants] = {
        k_icp<0, false, false>, k_icp<0, false, true>, k_icp<0, true, false>, k_icp<0, true, true>,
        k_icp<1, false, false>, k_icp<1, false, true>, k_icp<1, true, false>, k_icp<1, true, true>,
        k_icp<2, false, false>, k_icp<2, false, true>, k_icp<2, true, false>, k_icp<2, true, true>,
        k_icp<3, false, false>, k_icp<3, false, true>, k_icp<3, true, false>, k_icp<3, true, true>};
    return tab[var & (4 * kVariants - 1)];
}

int launch_init(youth_icp_ctx* c, hipStream_t s, const double* dTi, int n_pairs, int iters,
                bool persistent)
{
    hipLaunchKernelGGL(k_init, dim3((n_pairs + 63) / 64), dim3(64), 0, s, dTi, n_pairs, c->d_T64,
                       c->d_T32, c->d_status, persistent ? c->d_epoch : (unsigned*)nullptr,
                       persistent ? c->d_arr_it : (unsigned*)nullptr, iters, c->d_head);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int upload_T_init(youth_icp_ctx* c, hipStream_t s, const double* T_init_host, int n_pairs,
                  const double** dTi)
{
    *dTi = nullptr;
    if (!T_init_host) return YOUTH_OK;
    for (size_t i = 0; i < (size_t)n_pairs * 16; ++i)
        if (!std::isfinite(T_init_host[i]))
            return g_icp_err.set(YOUTH_EINVAL, "T_init: non-finite entry in pair %d", (int)(i / 16));
    HIP_TRY(hipMemcpyAsync(c->d_Tinit, T_init_host, (size_t)n_pairs * 16 * sizeof(double),
                           hipMemcpyHostToDevice, s));
    *dTi = c->d_Tinit;
    return YOUTH_OK;
}

int run_iterations(youth_icp_ctx* c, hipStream_t s, const int16_t* dsrc, int src0, int tgt0,
                   int n_pairs, const double* T_init_host, float* d_T_out, bool* exported,
                   const PrepJob* job)
{
    const PairMap pm{src0, tgt0};
    const int iters = c->prm.iters;
    if (exported) *exported = false;
    // k_icp_coop fuses the prep job (one pair of workgroups per target);
    // every other path runs k_prep first
    int npx = 0, G = 0;
    bool coop;
    if (job && job->chain) {
        // a tracker micro-batch runs every pair on the single-pair plan, so
        // each pair's summation tree (and pose) is the one track_frame gives;
        // refused (EINVAL, nothing enqueued) when that grid is not co-resident
        if (iters <= 0 || job->n != n_pairs || n_pairs > kCoopMaxChain ||
            !coop_plan(c, 1, &npx, &G) ||
            (long long)n_pairs * G >
                (long long)c->n_cu *
                    c->coop_bpc[c->coop_threads == 256][variant(c) * 2 + (c->fast ? 1 : 0)][npx])
            return g_icp_err.set(YOUTH_EINVAL, "track batch: %d pairs do not fit one cooperative grid",
                                 n_pairs);
        coop = true;
    } else {
        coop = iters > 0 && (!job || job->n == n_pairs || (!job->wait && job->n == 1)) &&
               coop_plan(c, n_pairs, &npx, &G);
    }
    c->last_coop = coop;
    c->last_first_form = 0;
    int rc = ensure_stats(c, iters > 0 ? iters : 1);
    if (rc) return rc;
    const double* dTi = nullptr;
    rc = upload_T_init(c, s, T_init_host, n_pairs, &dTi);
    if (rc) return rc;
    if (coop) {
        rc = launch_coop(c, s, dsrc, pm, n_pairs, dTi, d_T_out, npx, G, job);
        if (rc == YOUTH_OK) {
            if (exported) *exported = d_T_out != nullptr;
            c->last_pairs = n_pairs;
            c->last_iters = iters;
            c->last_stream = s;
            return YOUTH_OK;
        }
        if (job && job->chain) return rc;  // a micro-batch has no other kernel path
        // the runtime refused the cooperative launch (nothing was enqueued): this
        // context takes the persistent path from now on
        fprintf(stderr, "youth_icp: cooperative launch refused (%s); using the persistent path\n",
                youth_icp_last_error());
        (void)hipGetLastError();
        c->coop = false;
        c->last_coop = false;
    }
    const bool persistent = c->persistent && iters > 0;
    int chunk = 0;
    const int nb = persistent ? reduce_geometry(c, n_pairs, &chunk) : 0;
    const float thr2 = c->prm.dist_thresh * c->prm.dist_thresh;
    // Every pose starts at identity (no T_init) and the sums are exact:
    // iteration 0 matches every pixel with the record at its own index.  It
    // runs inside the prep pass when that pass forms every pair's target
    // records (k_prep_ident), else as k_icp's identity form.
    const bool ident = persistent && !dTi && c->ident_first && c->reduce != YOUTH_REDUCE_LANE32;
    // Not inside the prep pass when contexts share the device (set_concurrency):
    // k_prep_ident holds its CUs about twice as long as k_prep, beside the
    // other context's k_icp; 64- and 128-pair shards two in flight then ran
    // anywhere from -3 % to +3 % of the parent (profiles/ident/shards.txt),
    // where k_icp's own identity form is a steady +0.5 to +2 %.
    const bool ident_prep = ident && c->ident_prep && c->share == 1 && job && job->wait &&
                            job->out0 <= tgt0 && tgt0 + n_pairs <= job->out0 + job->n;
    if (ident_prep) {
        rc = launch_prep_ident(c, s, job, dsrc, pm, n_pairs, iters, thr2, nb, d_T_out);
        if (rc) return rc;
    } else if (persistent && job) {
        // k_prep also sets the per-call state (k_init folded in)
        const InitArgs ia{dTi,         n_pairs,    c->d_T64, c->d_T32, c->d_status,
                          c->d_epoch,  c->d_arr_it, iters,   c->d_head};
        rc = launch_prep_with(c, s, job->depth, job->n, job->out0, false, &ia);
        if (rc) return rc;
    } else {
        if (job) {
            rc = launch_prep(c, s, job->depth, job->n, job->out0, false);
            if (rc) return rc;
        }
        rc = launch_init(c, s, dTi, n_pairs, iters, persistent);
        if (rc) return rc;
    }
    if (persistent) {
        rc = ensure_partials(c, (size_t)nb * n_pairs * kPartStride);
        if (rc) return rc;
        const bool aligned = (reinterpret_cast<uintptr_t>(dsrc) % 8 == 0) && (c->W % 4 == 0) &&
                           c->centred_exact;
        const int var = variant(c) * 4 + (c->fast ? 2 : 0) + (aligned ? 1 : 0);
        const int first = ident_prep ? 1 : 0;
        const long long items = (long long)(iters - first) * n_pairs * nb;
        long long grid = (long long)c->n_cu * c->icp_blocks_per_cu[var] / c->share;
        if (grid > items) grid = items;
        if (grid < 1) grid = 1;
        const IterState is{c->d_T64,  c->d_T32,  c->d_status, c->d_stats,
                           c->d_arr_it, c->d_epoch, c->d_head + kQHead, c->d_head + kQError,
                           d_T_out,   iters,      n_pairs,    nb,
                           chunk,
                           // 8 per-XCD heads from 128 pairs (+0.7 % there), one below (64
                           // pairs: -0.8 % with 8; profiles/r03/ab_queues.txt)
                           c->queues ? c->queues : (n_pairs >= 128 ? kMaxQueues : 1),
                           // no T_init: iteration 0 at the identity pose (exact sums only:
                           // the lane32 kernels have no such form)
                           ident && !ident_prep, first, c->issue_prio};
        c->last_first_form = ident_prep ? 2 : ident ? 1 : 0;
        if (exported) *exported = d_T_out != nullptr;  // k_icp's final solves write d_T_out
        EventPair ep{};
        rc = ev_begin(c, s, &ep, 0);
        if (rc) return rc;
        if (items > 0) {  // (iters == 1 after k_prep_ident: nothing is left)
            auto kern = icp_kernel(var);
            hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kRedThreads), 0, s, dsrc, c->d_rec,
                               c->P, pm, c->W, c->H, c->K, c->F, thr2, c->d_partials, is);
            HIP_TRY(hipGetLastError());
        }
        c->lanes = youth_lanes{YOUTH_LANES_STRIDED, chunk, kRedThreads, 0};
        c->has_lanes = true;
        c->lanes_mixed = false;
        rc = ev_end(c, s, &ep);
        if (rc) return rc;
    } else {
        // arrival counters of the per-iteration fused kernel, re-armed in-kernel
        HIP_TRY(hipMemsetAsync(c->d_arrivals, 0, (size_t)c->max_frames * sizeof(unsigned), s));
        for (int it = 0; it < iters; ++it) {
            int nb = 0;
            rc = launch_reduce(c, s, dsrc, src0, tgt0, n_pairs, false, &nb, it);  // + fused solve
            if (rc) return rc;
        }
    }
    c->last_pairs = n_pairs;
    c->last_iters = iters;
    c->last_stream = s;
    return YOUTH_OK;
}

int export_poses(youth_icp_ctx* c, hipStream_t s, int n_pairs, float* d_T_out, bool timeout)
{
    hipLaunchKernelGGL(k_finish, dim3((n_pairs * 16 + 255) / 256), dim3(256), 0, s, c->d_T64,
                       n_pairs, d_T_out, c->d_status,
                       timeout ? (const unsigned*)(c->d_head + kQError) : (const unsigned*)nullptr);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

// Decide the division path for these intrinsics (k_verify_fastdiv).
int verify_fastdiv(youth_icp_ctx* c)
{
    c->fast = false;
    const char* off = getenv("YOUTH_ICP_NO_FASTDIV");
    if (off && *off && *off != '0') return YOUTH_OK;
    HIP_TRY(hipMemsetAsync(c->d_flag, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_verify_fastdiv, dim3(128, 64), dim3(256), 0, c->stream, c->K, c->F, c->W,
                       c->H, c->d_flag);
    HIP_TRY(hipGetLastError());
    unsigned bad = 1;
    HIP_TRY(hipMemcpyAsync(&bad, c->d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->fast = bad == 0;
    return YOUTH_OK;
}

hipError_t fill_occupancy(youth_icp_ctx* c, const char** what)
{
    hipError_t e;
    *what = "occupancy";
    for (int v = 0; v < 4 * kVariants; ++v) {
        int nb = 0;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)icp_kernel(v),
                                                              kRedThreads, 0)) != hipSuccess)
            return e;
        c->icp_blocks_per_cu[v] = nb > 0 ? nb : 1;
    }
    *what = "occupancy coop";
    for (int ti = 0; ti < 2; ++ti)
        for (int v = 0; v < 2 * kVariants; ++v)
            for (int npx = 1; npx <= kCoopMaxPx; ++npx) {
                const int th = ti ? 256 : 512;
                int nb = 0;
                if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                         &nb, coop_kernel(v >> 1, (v & 1) != 0, th), th, coop_lds(npx, th))) !=
                    hipSuccess)
                    return e;
                c->coop_bpc[ti][v][npx] = nb;
            }
    *what = "occupancy coop tall";
    for (int v = 0; v < 2 * kVariants; ++v) {
        int nb = 0;
        const int npx = kTileW * kCoopTileHTall / 512;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                 &nb, coop_kernel(v >> 1, (v & 1) != 0, 512, true), 512, coop_lds(npx, 512))) !=
            hipSuccess)
            return e;
        c->coop_bpc_tall[v] = nb;
    }
    return hipSuccess;
}

void coop_forget_stream(youth_icp_ctx* c)
{
    if (c->device < 0 || c->device >= 64) return;
    // the device's coop ordering must not take a later stream that reuses
    // this handle for the same stream (its work is complete: synchronised
    // by the caller, and every earlier coop launch ran before it)
    CoopOrder& o = g_coop_order[c->device];
    std::lock_guard<std::mutex> lk(o.mu);
    if (o.any && o.last == c->stream) {
        o.any = false;
        o.last = nullptr;
    }
}

int launch_solve_sums(youth_icp_ctx* c, hipStream_t s, int nblk)
{
    hipLaunchKernelGGL(k_solve, dim3(1), dim3(64), 0, s, c->d_partials, nblk, 0, 1, c->d_T64,
                       c->d_T32, c->d_status, (double*)nullptr, c->d_neq);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

int launch_solve_neq(youth_icp_ctx* c, hipStream_t s)
{
    hipLaunchKernelGGL(k_solve_neq, dim3(1), dim3(64), 0, s, c->d_neq, c->d_T64, c->d_T32,
                       c->d_status);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

hipError_t launch_status_out(youth_icp_ctx* c, hipStream_t s, int n, int32_t* out)
{
    hipLaunchKernelGGL(k_status_out, dim3((n + 255) / 256), dim3(256), 0, s, c->d_status, n,
                       (const unsigned*)(c->d_head + kQError), out);
    return hipGetLastError();
}

int launch_pull_frames(youth_icp_ctx* c, hipStream_t s, const int16_t* const* src, int m,
                       int16_t* dst, int N, int wg)
{
    FramePtrs fp{};
    for (int i = 0; i < m; ++i) fp.src[i] = src[i];
    hipLaunchKernelGGL(k_pull_frames, dim3(wg, m), dim3(64), (unsigned)c->trk_pull_lds, s, fp, dst,
                       N, m);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

hipError_t launch_selftest(int which, unsigned long long n, unsigned long long seed,
                           unsigned long long* d_bad)
{
    if (which == 0)
        hipLaunchKernelGGL(k_selftest_projdiv, dim3(4096), dim3(256), 0, 0, n, seed, d_bad);
    else if (which == 1)
        hipLaunchKernelGGL(k_selftest_projquot, dim3(4096), dim3(256), 0, 0, n, seed, d_bad);
    else
        hipLaunchKernelGGL(k_selftest_normalize, dim3(8192), dim3(256), 0, 0, n, seed, d_bad);
    return hipGetLastError();
}

}  // namespace youth_icp
