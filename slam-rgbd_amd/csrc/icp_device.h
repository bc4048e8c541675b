// icp_device.h — the device code that the two kernel units share:
// icp_kernels.hip (the depth-only ICP kernels) and rgbd_align.hip (the RGB-D
// alignment).  Layout constants and the structs kernels take by value
// (PairMap, PoseState); the 64-bit lane helpers; fast / IEEE division, the
// projection quotient and the normalisation; back-projection, of one pixel
// and of a lane's four per loop step (backproject4); lane masks; spec a7-a9
// per pixel (survey_project, xform_project, match_accumulate over
// gate_accumulate; ident_accumulate, the identity-pose form); the wave
// reduce-scatter (wave_reduce_scatter<kN>); the fused solve's hand-off
// between a pair's workgroups (handoff_publish, handoff_sum); the a10 solve
// and pose update.  One text of the spec's arithmetic and of the summation
// order for both units.  The host units (icp_api.cpp, icp_batch.cpp,
// icp_track.cpp; rgbd_api.cpp, rgbd_track.cpp) include it through icp_host.h
// for the constants and structs alone.
//
// No __global__ function lives here: a kernel in a shared header would be
// emitted again by every unit that includes it.
#ifndef YOUTH_ICP_DEVICE_H
#define YOUTH_ICP_DEVICE_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "youth_icp.h"

// Internal linkage on purpose: every kernel keeps the name it had when all of
// this was one translation unit, and nothing here is visible outside a unit.
namespace {

// ----------------------------------------------------------------- layout --
// Workspace frame f:
//   recs + f*P            float4 {z, nx, ny, nz} per pixel (targets);
//   xyz  + f*3*P (+P, +2P) optional X, Y, Z planes (stage-level API only).
// P = plane stride = round_up(N + 4, 256); the pad is zeroed once, so a
// clamped fetch or a float4 load past N reads an invalid point (z = 0).
// Sources are read straight from the caller's int16 depth.
constexpr int kTileW = 64;
// k_prep tiles 128 x 24 by 512-thread workgroups: four per CU fill all 32
// wave slots (LDS 40.6 KB each).  A 128-px row touches 2 lines of its own
// and 2 of its neighbours' where a 64-px row touched 1 + 2, so the depth
// over-fetch drops from 2.8x to 1.9x: k_prep's PMC traffic 1.21 -> 1.105x of
// its 18 B/px, and 586 -> 582 us per 512 frames (profiles/r04/ab_r4c.txt,
// prep128x24_pmc.txt).  Also measured: 128 x 16 650 us (1.11x), 256 x 12
// 747 us (1.07x; three per CU, LDS-limited); earlier 64 x 48 593 us, 64 x 24 by
// 256 threads 617 us, 64 x 80 / 1024 625 us (profiles/r02/ab_s44.txt,
// ab_s45.txt); fewer workgroups per CU cost more (ab_s43.txt: 7 -> 6 per CU +8 %)
constexpr int kPrepThreads = 512;
// k_prep's own tile (k_icp_coop's fused prep keeps kTileW-wide tiles, whose
// shape its lane partition and prep counters assume); -D knobs for A/B
#ifndef YOUTH_PREP_TW
#define YOUTH_PREP_TW 128
#endif
#ifndef YOUTH_PREP_TH
#define YOUTH_PREP_TH 24
#endif
constexpr int kPrepTW = YOUTH_PREP_TW;
constexpr int kPrepTH = YOUTH_PREP_TH;
// k_prep_ident: one wave per unit of 64 columns (one per lane) x a band of rows
constexpr int kPrepColW = 64;
constexpr int kPrepBand = 96;  // rows per unit at large batches (launch_prep_ident)
constexpr int kLdsW = kTileW + 2;

constexpr int kRedThreads = 256;
constexpr int kRedStep = kRedThreads * 4;  // pixels per workgroup loop step
constexpr int kNeq = YOUTH_NEQ;
// k_icp's chunk partials: rows of 30 doubles (29 + a zero pad, 240 B) so the
// last arriver reads them as 16-byte pieces; kSumCols interleaved columns of
// chunks are summed in parallel, then the column sums in column order.
constexpr int kPartStride = 30;
constexpr int kPieces = kPartStride / 2;  // 16-byte pieces per row
constexpr int kSumCols = 16;              // kSumCols * kPieces <= kRedThreads
// Persistent-queue words (unsigned index into ctx->d_head), one 128-B line
// apart so the contended dequeue atomic shares no line with the polled flag.
// k_icp's work queues: up to kMaxQueues heads, kQHeads + 32 q (queue q holds
// the pairs p = q (mod n_queues)).
constexpr int kQHead = 0, kQError = 32, kQSpins = 64, kQWaited = 96, kQHeads = 128;
constexpr int kMaxQueues = 8, kQHeadStride = 32;
constexpr int kQWords = kQHeads + kMaxQueues * kQHeadStride;

typedef float f4v __attribute__((ext_vector_type(4)));  // a gathered {z, nx, ny, nz} record
typedef unsigned u4v __attribute__((ext_vector_type(4)));  // two doubles, raw bits

struct Intr {
    float fx, fy, cx, cy, ds;
};

// Division by the constants fx, fy, ds in two operations (Brisebarre,
// Muller & Raina, "Accelerating correctly rounded floating-point division
// when the divisor is known in advance", IEEE TC 2004): for each divisor y,
// h = RN(1/y) and l = RN((1 - y h) / y); then q = RN(n h + RN(n l)) =
// fma(n, h, n * l).  Used only where k_verify_fastdiv finds it equal to IEEE
// n / y on the whole domain the kernels divide.
struct FastK {
    float hfx, lfx, hfy, lfy, hds, lds;
};

// 64-bit lane helpers (two 32-bit halves)
__device__ __forceinline__ double join64(unsigned lo, unsigned hi)
{
    return __hiloint2double((int)hi, (int)lo);
}
__device__ __forceinline__ unsigned lo32(double x) { return (unsigned)__double2loint(x); }
__device__ __forceinline__ unsigned hi32(double x) { return (unsigned)__double2hiint(x); }

// lane `l`'s value in every lane (wave-uniform l: two v_readlane into SGPRs)
__device__ __forceinline__ double readlane64(double x, int l)
{
    return join64((unsigned)__builtin_amdgcn_readlane((int)lo32(x), l),
                  (unsigned)__builtin_amdgcn_readlane((int)hi32(x), l));
}

// fma(n, h, RN(n l)): equal to RN(n / d) wherever k_verify_fastdiv found
// no mismatch (h, l of the divisor d, FastK).
__device__ __forceinline__ float div_fast(float n, float h, float l)
{
    return fmaf(n, h, n * l);
}

template <bool kFast>
__device__ __forceinline__ float bp_div(float n, float d, float h, float l)
{
    return kFast ? div_fast(n, h, l) : n / d;
}

// Spec a7's two projection quotients nu/den and nv/den, IEEE correctly
// rounded, sharing one reciprocal.  hipcc expands an fp32 a/b (denormals on)
// to  s = div_scale(b,b,a); n = div_scale(a,b,a); r = rcp(s);
//     r = fma(fma(-s,r,1), r, r); q = n*r; q = fma(fma(-s,q,n), r, q);
//     q = div_fmas(fma(-s,q,n), r, q); result = div_fixup(q, b, a)   (`make asm`).
// For b in [2^-60, 2^60] div_scale rescales neither operand except when a is
// 0, |a/b| >= ~2^95, |a/b| < 2^-126 or |a| < 2^-103; otherwise div_fmas is a
// plain fma and div_fixup returns q unchanged, so q = RN(n r) with those two
// fma corrections equals a/b bit for bit, and its reciprocal part depends on
// b only (one correction suffices from a correctly rounded r: proj_quot).  In the excepted
// cases the results differ at most between 0 / tiny / huge / inf / NaN
// values, which the projection (+cx, +0.5, floor, range test) maps to the same
// pixel or to "outside".  Callers fall back to a/b when b is out of range.
// youth_icp_selftest_projdiv compares the two bitwise on random and edge
// cases (tests/test_gpu_parity.py).
__device__ __forceinline__ float proj_recip(float den)
{
    const float r0 = __builtin_amdgcn_rcpf(den);
    return fmaf(fmaf(-den, r0, 1.0f), r0, r0);
}
__device__ __forceinline__ bool proj_den_ok(float den)
{
    return (den >= 0x1p-60f) & (den <= 0x1p60f);
}
// Spec a7's projection reciprocal RN(1 / den): for den in [2^-60, 2^60] the
// hardware reciprocal refined by ONE Newton step, fma(fma(-den, r0, 1), r0,
// r0) (proj_recip), is already the correctly rounded 1.0f / den: measured
// for EVERY fp32 den in that range (tools/rcp_probe.hip,
// profiles/r02/rcp_probe.txt: 0 of 1,006,632,961 differ; the two further
// quotient corrections used before changed nothing), and re-checked by
// youth_icp_selftest_projdiv (tests/test_gpu_parity.py).  Outside: IEEE.
__device__ __forceinline__ float proj_rcp_rn(float den)
{
    if (proj_den_ok(den))  // always in practice (den is a depth in metres)
        return proj_recip(den);
    return 1.0f / den;
}

// Which arithmetic spec a7/a8 runs in (youth_icp_set_spec):
//   kSpecSurvey (default) SURVEY.md §8a a7/a8 + §7 literally: separately
//               rounded products and sums in a fixed order (no FMA) and the
//               projection quotient fx P'x / P'z as an IEEE division;
//   kSpecFma    opt-in: fma chains and one correctly rounded reciprocal.
// The oracle restates both (oracle_set_spec); every kernel of the iteration
// (k_icp, k_icp_coop, k_reduce) is instantiated for each.
constexpr int kSpecFma = YOUTH_SPEC_FMA;
constexpr int kSpecSurvey = YOUTH_SPEC_SURVEY;
// ... and for each reduction of spec a9 (youth_icp_set_reduce):
//   lane32 (default) SURVEY.md §8a a9 as worded, "fp32 lanes -> fp64
//          finalize": each lane sums its pixels' 28 products with v_fma_f32
//          over its whole share of a work item, then converts once;
//   exact  every product exact in fp64 (v_fmac_f64 per product).
// The kernels' template parameter kSp is the VARIANT: bit 0 the arithmetic
// (kSpecFma / kSpecSurvey), bit 1 (kRedLane32) the lane32 reduction.
constexpr int kRedLane32 = 2;
constexpr int kVariants = 4;
__host__ __device__ constexpr bool sp_survey(int v) { return (v & 1) == kSpecSurvey; }
__host__ __device__ constexpr bool sp_lane32(int v) { return (v & kRedLane32) != 0; }

// kSpecSurvey's projection quotient RN(n / den) from r = RN(1 / den)
// (proj_recip inside proj_den_ok: correctly rounded, checked exhaustively):
// q0 = RN(n r) is within one ulp of n / den, the remainder n - den q0 is
// exact in one fma, and one correction q0 + (n - den q0) r rounds to
// RN(n / den) (Markstein, IBM J. Res. Dev. 34(1), 1990, Theorem 1; barring
// under/overflow of the remainder, which only happens for quotients that
// project to the same pixel or off the frame).  hipcc's a/b applies two
// such corrections; youth_icp_selftest_projquot compares this one with
// IEEE a/b bitwise and through the projection (tests/test_gpu_parity.py).
__device__ __forceinline__ float proj_quot(float n, float den, float r)
{
    const float q0 = n * r;
    return fmaf(fmaf(-den, q0, n), r, q0);
}

// (int)floorf(x) in one instruction (v_cvt_flr_i32_f32; floorf + the int
// conversion are two 4-cycle VALU forms, profiles/r03/valu_cycles.txt).
// Equal to (int)floorf(x) for every normal or zero x with |x| < 2^30, and
// (unsigned) of it < 16384 exactly when 0 <= floorf(x) < 16384 for every
// non-NaN x but denormals (saturating conversion): youth_icp_selftest_projquot
// checks both over all 2^32 bit patterns.  kSpecSurvey's projected
// coordinate ((q + c) + 0.5) is never NaN (T finite, q finite or +-inf) and
// never denormal (it is 0 or at least 2^-25 in magnitude: s + 0.5 with s a
// float near -0.5 is exact by Sterbenz, |s| < 0.25 leaves it above 0.25).
__device__ __forceinline__ int floor_i32(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// Spec a6's normalisation n = c / sqrtf(|c|^2) on its common range, bit for
// bit.  hipcc's correctly rounded sqrtf is  x' = x < 2^-96 ? x 2^32 : x;
// s = v_sqrt(x'); s -= (fma(-(s-1ulp), s, x') <= 0); s += (fma(-(s+1ulp), s,
// x') > 0); unscale; return x for +-0 / +inf (`make asm`).  For x in
// [2^-96, 2^118] the scaling and the class fix-up are identities, leaving
// the sequence below.  The three quotients then share one reciprocal
// (norm_div): len = sqrt(x) is in [2^-48, 2^59] and |c_i| <= ~len, so
// div_scale rescales no operand when |c_i| >= 2^-64; c_i = 0
// is exact through the sign: RN(c/len) = copysign(RN(|c|/len), c).  Callers
// take the IEEE expressions when norm_fast_ok is false.
// youth_icp_selftest_normalize checks both against IEEE on device.
__device__ __forceinline__ float sqrt_rn_mid(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u);
    const float sup = __uint_as_float(__float_as_uint(s) + 1u);
    const float t = fmaf(-sdn, s, x) <= 0.0f ? sdn : s;
    return fmaf(-sup, s, x) > 0.0f ? sup : t;
}
__device__ __forceinline__ bool norm_comp_ok(float c)
{
    return !((fabsf(c) < 0x1p-64f) & (c != 0.0f));
}
__device__ __forceinline__ bool norm_fast_ok(float len2, float cx, float cy, float cz)
{
    return (len2 >= 0x1p-96f) && (len2 <= 0x1p118f) && norm_comp_ok(cx) && norm_comp_ok(cy) &&
           norm_comp_ok(cz);
}
// The three quotients take ONE correction from the correctly rounded
// reciprocal r = RN(1 / len) (proj_recip; len in [2^-48, 2^59]), as the
// projection's proj_quot (Markstein's theorem; youth_icp_selftest_normalize
// compares with IEEE c / sqrtf(len2) bitwise).
__device__ __forceinline__ float norm_div(float c, float len, float r)
{
    return copysignf(proj_quot(fabsf(c), len, r), c);
}
// norm_fast_ok on the bits, for k_prep: len2 (>= +0 or NaN) in [2^-96,
// 2^118] as one unsigned compare; a component c is "tiny" (0 < |c| < 2^-64)
// iff t = 2 bits(c) - 2 (sign shifted out, wrapping: +-0 -> 2^32 - 2) is
// below 2 bits(2^-64) - 2, so the three tests are one min3 and one compare.
// The self-test checks it equals norm_fast_ok on every random vector.
__device__ __forceinline__ bool norm_fast_ok_bits(float len2, float cx, float cy, float cz)
{
    constexpr unsigned kLo = 0x0F800000u, kHi = 0x7A800000u, kTiny = 2u * 0x1F800000u - 2u;
    const unsigned tx = (__float_as_uint(cx) << 1) - 2u, ty = (__float_as_uint(cy) << 1) - 2u,
                   tz = (__float_as_uint(cz) << 1) - 2u;
    return (int)((__float_as_uint(len2) - kLo) <= (kHi - kLo)) & (int)(min(min(tx, ty), tz) >= kTiny);
}

// viewerModule.c:341-345 with explicit intrinsics (bit-identical to the
// viewer for cx = W/2, cy = H/2, f = 570.3f, ds = 1000.0f):
//   valid iff d > 0;  z = d / ds;  x = ((u - cx) z) / fx;  y = ((v - cy) z) / fy
template <bool kFast>
__device__ __forceinline__ void backproject(int d, int u, int v, const Intr& K,
                                            const FastK& F, float& x, float& y, float& z)
{
    const float zz = bp_div<kFast>((float)max(d, 0), K.ds, F.hds, F.lds);  // d <= 0: 0/ds = +0
    x = bp_div<kFast>(((float)u - K.cx) * zz, K.fx, F.hfx, F.lfx);
    y = bp_div<kFast>(((float)v - K.cy) * zz, K.fy, F.hfy, F.lfy);
    z = zz;
}
// The same with the centred pixel coordinates uc = (float)u - cx and
// vc = (float)v - cy supplied (exact: integers below 2^24), so a caller
// walking a row forms them by additions.
template <bool kFast>
__device__ __forceinline__ void backproject_c(int d, float uc, float vc, const Intr& K,
                                              const FastK& F, float& x, float& y, float& z)
{
    const float zz = bp_div<kFast>((float)max(d, 0), K.ds, F.hds, F.lds);
    x = bp_div<kFast>(uc * zz, K.fx, F.hfx, F.lfx);
    y = bp_div<kFast>(vc * zz, K.fy, F.hfy, F.lfy);
    z = zz;
}

// One pixel's target record {z, nx, ny, nz} (spec a6) from its back-projected
// point (px, py, pz) and its four neighbours' points: left (u - 1), right
// (u + 1), up (v - 1), down (v + 1); inner: the pixel is off the 1-px border.
// The one text for prep_tile (points read from its LDS planes) and
// k_prep_ident (points in registers), so their records are the same bits.
// Branch-free but for the rare fallback: every lane forms the normal (a caller
// has a point for every neighbour, 0 outside the image) and the record is
// selected at the end.  Every z is >= +0 (back-projection of max(d, 0), 0
// outside the image), so the five z > 0 tests are one test of their minimum,
// taken on the bits (the same order for non-negative floats; +0 is bits 0).
__device__ __forceinline__ float4 prep_record(float px, float py, float pz, float lx, float ly,
                                              float lz, float rx, float ry, float rz, float ux,
                                              float uy, float uz, float dx, float dy, float dz,
                                              bool inner)
{
    const unsigned zmin = min(min(min(__float_as_uint(pz), __float_as_uint(lz)),
                                  min(__float_as_uint(rz), __float_as_uint(uz))),
                              __float_as_uint(dz));
    const float ax = rx - lx;
    const float ay = ry - ly;
    const float az = rz - lz;
    const float bx = dx - ux;
    const float by = dy - uy;
    const float bz = dz - uz;
    const float cx = ay * bz - az * by;
    const float cy = az * bx - ax * bz;
    const float cz = ax * by - ay * bx;
    const float len2 = (cx * cx + cy * cy) + cz * cz;
    bool has_n = inner & (zmin != 0u) & (len2 > 0.0f);
    const float len = sqrt_rn_mid(len2);
    const float r = proj_recip(len);
    float nx = norm_div(cx, len, r);
    float ny = norm_div(cy, len, r);
    float nz = norm_div(cz, len, r);
    if (__builtin_expect(has_n & !norm_fast_ok_bits(len2, cx, cy, cz), 0)) {
        const float l = sqrtf(len2);  // correctly rounded (checked in .s)
        nx = cx / l;
        ny = cy / l;
        nz = cz / l;
        // |c|^2 overflowed (points of ~10^10 m under a corner camera): c /
        // inf is (0, 0, 0), and a zero normal is no normal (spec a6 / a7:
        // the oracle tests the stored normal).  A finite len2 > 0 leaves a
        // component of at least |c| / sqrt(3), so only this branch needs the test
        has_n = (nx != 0.0f) | (ny != 0.0f) | (nz != 0.0f);
    }
    // oriented so n.P <= 0
    if (((nx * px + ny * py) + nz * pz) > 0.0f) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    if (!has_n) nx = ny = nz = 0.0f;
    // a target without a normal is stored as z = 0 ("invalid target"): the
    // spec's two tests "target valid" and "normal valid" become the one
    // tz > 0 test in the pixel loop (a stored Z plane keeps pz)
    return make_float4(has_n ? pz : 0.0f, nx, ny, nz);
}

// ------------------------------------------------------------ solve (a10) --
// Spec a10 (round 5): A x = b by block elimination with 3x3 adjugates, xi =
// -x; the same correctly rounded operations in the same order as
// oracle_solve (oracle/icp_oracle.c), so xi and the status are bit-identical.
// With P = A[0..2][0..2] (rotation), Q = A[0..2][3..5], R = A[3..5][3..5],
// b = (b1, b2), C = adj(P):
//   detP = P00 C00 + P01 C01 + P02 C02, M = C Q, u = C b1
//   S' = detP R - Q^T M (detP times the Schur complement), y' = detP b2 - Q^T u
//   x2 = adj(S') y' * (1 / det S'),  x1 = C (b1 - Q x2) * (1 / detP)
// ONE division on the dependent chain (1 / detP runs beside it) and no value
// crosses lanes, against LDL^T's six dependent reciprocals and lane
// broadcasts (tools/solvebench).  The rotation block goes first,
// as LDL^T's pivot order does: eliminating the translation block first was
// faster on paper but 2-3x more sensitive to the sums' last bits on
// ill-conditioned frames.  DEGENERATE iff an LDL^T pivot is
// <= 1e-12 max diag, tested on the leading minors by products.
__device__ __forceinline__ double dd2(double a, double b, double c, double d)
{
    return fma(a, b, -(c * d));  // a b - c d
}
__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2,
                                       double b2)
{
    return fma(a2, b2, fma(a1, b1, a0 * b0));
}
// symmetric 3x3 {m00, m01, m02, m11, m12, m22}: adjugate, matrix-vector
__device__ __forceinline__ void adj3(const double* p, double* c)
{
    c[0] = dd2(p[3], p[5], p[4], p[4]);
    c[1] = dd2(p[2], p[4], p[1], p[5]);
    c[2] = dd2(p[1], p[4], p[2], p[3]);
    c[3] = dd2(p[0], p[5], p[2], p[2]);
    c[4] = dd2(p[1], p[2], p[0], p[4]);
    c[5] = dd2(p[0], p[3], p[1], p[1]);
}
__device__ __forceinline__ void symv3(const double* c, const double* v, double* o)
{
    o[0] = dot3(c[0], v[0], c[1], v[1], c[2], v[2]);
    o[1] = dot3(c[1], v[0], c[3], v[1], c[4], v[2]);
    o[2] = dot3(c[2], v[0], c[4], v[1], c[5], v[2]);
}
// neq wave-uniform (LDS or registers); every lane computes everything, so no
// value crosses lanes.  xi is zeroed on a nonzero status.
__device__ __forceinline__ int solve_block6(const double* neq, double xi[6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = 0.0;
    if (!(neq[28] >= 6.0)) return YOUTH_STATUS_FEW_MATCHES;
    double maxd = 0.0;  // the diagonal, in order (a, a) = 0, 6, 11, 15, 18, 20
    maxd = neq[0] > maxd ? neq[0] : maxd;
    maxd = neq[6] > maxd ? neq[6] : maxd;
    maxd = neq[11] > maxd ? neq[11] : maxd;
    maxd = neq[15] > maxd ? neq[15] : maxd;
    maxd = neq[18] > maxd ? neq[18] : maxd;
    maxd = neq[20] > maxd ? neq[20] : maxd;
    if (!(maxd > 0.0)) return YOUTH_STATUS_DEGENERATE;
    const double eps = 1e-12 * maxd;
    const double P[6] = {neq[0], neq[1], neq[2], neq[6], neq[7], neq[11]};
    const double R[6] = {neq[15], neq[16], neq[17], neq[18], neq[19], neq[20]};
    const double Q[3][3] = {{neq[3], neq[4], neq[5]}, {neq[8], neq[9], neq[10]},
                            {neq[12], neq[13], neq[14]}};
    const double b1[3] = {neq[21], neq[22], neq[23]}, b2[3] = {neq[24], neq[25], neq[26]};
    double C[6], E[6], S[6], M[3][3], u[3], y[3], v[3], x2[3], w[3];
    adj3(P, C);
    const double detP = dot3(P[0], C[0], P[1], C[1], P[2], C[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // M = C Q, column by column
        const double q[3] = {Q[0][j], Q[1][j], Q[2][j]};
        double o[3];
        symv3(C, q, o);
        M[0][j] = o[0];
        M[1][j] = o[1];
        M[2][j] = o[2];
    }
    symv3(C, b1, u);
    // S' upper triangle (i <= j): detP R[i][j] - (Q^T M)[i][j]
    S[0] = fma(detP, R[0], -dot3(Q[0][0], M[0][0], Q[1][0], M[1][0], Q[2][0], M[2][0]));
    S[1] = fma(detP, R[1], -dot3(Q[0][0], M[0][1], Q[1][0], M[1][1], Q[2][0], M[2][1]));
    S[2] = fma(detP, R[2], -dot3(Q[0][0], M[0][2], Q[1][0], M[1][2], Q[2][0], M[2][2]));
    S[3] = fma(detP, R[3], -dot3(Q[0][1], M[0][1], Q[1][1], M[1][1], Q[2][1], M[2][1]));
    S[4] = fma(detP, R[4], -dot3(Q[0][1], M[0][2], Q[1][1], M[1][2], Q[2][1], M[2][2]));
    S[5] = fma(detP, R[5], -dot3(Q[0][2], M[0][2], Q[1][2], M[1][2], Q[2][2], M[2][2]));
#pragma unroll
    for (int j = 0; j < 3; ++j)
        y[j] = fma(detP, b2[j], -dot3(Q[0][j], u[0], Q[1][j], u[1], Q[2][j], u[2]));
    adj3(S, E);
    const double detS = dot3(S[0], E[0], S[1], E[1], S[2], E[2]);
    const double epsP = eps * detP;
    // pivots P00, C22/P00, detP/C22, S'00/detP, E22/(detP S'00), detS/(detP E22)
    const bool ok = (P[0] > eps) & (C[5] > eps * P[0]) & (detP > eps * C[5]) & (S[0] > epsP) &
                    (E[5] > epsP * S[0]) & (detS > epsP * E[5]);
    if (!ok) return YOUTH_STATUS_DEGENERATE;
    const double rS = 1.0 / detS, rP = 1.0 / detP;
    symv3(E, y, v);
#pragma unroll
    for (int i = 0; i < 3; ++i) x2[i] = v[i] * rS;
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = b1[i] - dot3(Q[i][0], x2[0], Q[i][1], x2[1], Q[i][2], x2[2]);
    symv3(C, w, v);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xi[i] = -(v[i] * rP);
        xi[3 + i] = -x2[i];
    }
    return 0;
}

__device__ void se3_exp_left(const double xi[6], double* T)
{
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a, b, c;
    if (th2 < 0x1p-7) {  // spec a10: Taylor in th2 (oracle_se3_exp: same fma chain)
        const double x = th2;
        a = fma(x, fma(x, fma(x, fma(x, fma(x, -0x1.ae64567f544e4p-26, 0x1.71de3a556c734p-19),
                                        -0x1.a01a01a01a01ap-13), 0x1.1111111111111p-7),
                       -0x1.5555555555555p-3), 0x1.0000000000000p+0);
        b = fma(x, fma(x, fma(x, fma(x, fma(x, -0x1.1eed8eff8d898p-29, 0x1.27e4fb7789f5cp-22),
                                        -0x1.a01a01a01a01ap-16), 0x1.6c16c16c16c17p-10),
                       -0x1.5555555555555p-5), 0x1.0000000000000p-1);
        c = fma(x, fma(x, fma(x, fma(x, fma(x, -0x1.6124613a86d09p-33, 0x1.ae64567f544e4p-26),
                                        -0x1.71de3a556c734p-19), 0x1.a01a01a01a01ap-13),
                       -0x1.1111111111111p-7), 0x1.5555555555555p-3);
    } else {
        const double th = sqrt(th2);
        double s, co;
        sincos(th, &s, &co);
        a = s / th;
        b = (1.0 - co) / th2;
        c = (th - s) / (th2 * th);
    }
    const double Km[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double K2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            K2[i][j] = (Km[i][0] * Km[0][j] + Km[i][1] * Km[1][j]) + Km[i][2] * Km[2][j];
    double E[3][4];
    for (int i = 0; i < 3; ++i) {
        double V[3];
        for (int j = 0; j < 3; ++j) {
            const double I = (i == j) ? 1.0 : 0.0;
            E[i][j] = (I + a * Km[i][j]) + b * K2[i][j];
            V[j] = (I + b * Km[i][j]) + c * K2[i][j];
        }
        E[i][3] = (V[0] * xi[3] + V[1] * xi[4]) + V[2] * xi[5];
    }
    double O[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = (E[i][0] * T[0 * 4 + j] + E[i][1] * T[1 * 4 + j]) + E[i][2] * T[2 * 4 + j];
            if (j == 3) s += E[i][3];
            O[i * 4 + j] = s;
        }
    for (int i = 0; i < 12; ++i) T[i] = O[i];
}

// Spec a10 by ONE wave (all 64 lanes call it): solve_block6 in every lane
// (wave-uniform, no cross-lane traffic), then se3_exp_left with its
// per-element operations and order, lane l < 12 computing output entry
// (l / 4, l % 4) of exp(xi^) T.  neq (LDS, kNeq): the pair's sums; T64 (LDS,
// 12): pose in/out; T32 (LDS, 12): fp32 copy out.  Returns the status bits;
// the pose is updated only when they are 0.
__device__ __forceinline__ int solve_update_wave(const double* neq, double* T64, float* T32, int lane)
{
    double xi[6];
    const int st = solve_block6(neq, xi);
    if (st) return st;

    // T <- exp(xi^) T (se3_exp_left), one output entry per lane
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a, b, c;
    if (th2 < 0x1p-7) {  // spec a10: Taylor in th2 (oracle_se3_exp: same fma chain)
        const double x2 = th2;
        a = fma(x2, fma(x2, fma(x2, fma(x2, fma(x2, -0x1.ae64567f544e4p-26, 0x1.71de3a556c734p-19),
                                          -0x1.a01a01a01a01ap-13), 0x1.1111111111111p-7),
                        -0x1.5555555555555p-3), 0x1.0000000000000p+0);
        b = fma(x2, fma(x2, fma(x2, fma(x2, fma(x2, -0x1.1eed8eff8d898p-29, 0x1.27e4fb7789f5cp-22),
                                          -0x1.a01a01a01a01ap-16), 0x1.6c16c16c16c17p-10),
                        -0x1.5555555555555p-5), 0x1.0000000000000p-1);
        c = fma(x2, fma(x2, fma(x2, fma(x2, fma(x2, -0x1.6124613a86d09p-33, 0x1.ae64567f544e4p-26),
                                          -0x1.71de3a556c734p-19), 0x1.a01a01a01a01ap-13),
                        -0x1.1111111111111p-7), 0x1.5555555555555p-3);
    } else {
        const double th = sqrt(th2);
        double sn, co;
        sincos(th, &sn, &co);
        a = sn / th;
        b = (1.0 - co) / th2;
        c = (th - sn) / (th2 * th);
    }
    const double Km[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    const int l = lane < 12 ? lane : 11;
    const int r = l >> 2, col = l & 3;
    double Kr[3];  // row r of Km
#pragma unroll
    for (int k = 0; k < 3; ++k) Kr[k] = r == 0 ? Km[0][k] : (r == 1 ? Km[1][k] : Km[2][k]);
    double Er[3], Vr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double K2 = (Kr[0] * Km[0][k] + Kr[1] * Km[1][k]) + Kr[2] * Km[2][k];
        const double I = (r == k) ? 1.0 : 0.0;
        Er[k] = (I + a * Kr[k]) + b * K2;
        Vr[k] = (I + b * Kr[k]) + c * K2;
    }
    const double Er3 = (Vr[0] * xi[3] + Vr[1] * xi[4]) + Vr[2] * xi[5];
    double o = (Er[0] * T64[0 * 4 + col] + Er[1] * T64[1 * 4 + col]) + Er[2] * T64[2 * 4 + col];
    if (col == 3) o += Er3;
    if (lane < 12) {
        T64[lane] = o;
        T32[lane] = (float)o;
    }
    return 0;
}

__device__ __forceinline__ void solve_update(const double* neq, double* T64, float* T32,
                                             int32_t* status)
{
    double xi[6];
    const int st = solve_block6(neq, xi);
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = T64[i];
    if (st == 0) se3_exp_left(xi, T);
    for (int i = 0; i < 12; ++i) {
        T64[i] = T[i];
        T32[i] = (float)T[i];
    }
    *status |= st;
}

// ------------------------------------------------------- the pixel loops --
struct PairMap {
    int src0, tgt0;  // pair p: source depth frame src0 + p, target record frame tgt0 + p
};

// Per-iteration pose state for the fused solve (k_reduce's kFuse;
// k_rgbd_reduce's RgbdState derives from it).  T32 is read by every workgroup
// of pair p at entry and rewritten only by p's LAST workgroup, after all of
// p's workgroups have arrived (so after they read it).
struct PoseState {
    double* T64;          // [pair][16]
    float* T32;           // [pair][12]
    int32_t* status;      // [pair]
    double* stats;        // [pair][iters][2] or null
    unsigned* arrivals;   // [pair], zero at launch; re-armed by the last arriver
    int it, iters;
};

template <bool kAligned>
__device__ __forceinline__ short4 load_depth4(const int16_t* __restrict__ sD, int i, int end)
{
    // i < end always here; kAligned => i % 4 == 0 and i + 3 < end
    short4 d;
    if (kAligned) {
        d = *reinterpret_cast<const short4*>(sD + i);
    } else {
        d.x = sD[i];
        d.y = (i + 1) < end ? sD[i + 1] : (short)0;
        d.z = (i + 2) < end ? sD[i + 2] : (short)0;
        d.w = (i + 3) < end ? sD[i + 3] : (short)0;
    }
    return d;
}

// Source points of a lane's four pixels i .. i + 3 of one loop step, depths
// dd[0..3], pixel i at column u0 of row v0 (accumulate_chunk, k_rgbd_reduce):
// point(q, x, y, z) takes each as it is formed (the callers project it at
// once; statement order matters to the scheduler, as does dd being the
// caller's array: HISTORY.md).  kAligned: the four share a row, centred
// coordinates by exact additions (uc0 + q == (float)(u0 + q) - cx, which the
// host checked for these intrinsics: centred_exact).  Else a pixel past the
// row's end wraps to the next row, and one at or past `end` back-projects
// depth 0, an invalid point.
template <bool kFast, bool kAligned, typename Fn>
__device__ __forceinline__ void backproject4(const int* dd, int i, int end, int u0, int v0,
                                             int W, const Intr& K, const FastK& F, Fn&& point)
{
    const float uc0 = (float)u0 - K.cx, vc0 = (float)v0 - K.cy;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float sx, sy, sz;
        if (kAligned) {
            backproject_c<kFast>(dd[q], uc0 + (float)q, vc0, K, F, sx, sy, sz);
        } else {
            int u = u0 + q, v = v0;
            const bool wrap = u >= W;
            u = wrap ? u - W : u;
            v = wrap ? v + 1 : v;
            backproject<kFast>((i + q) < end ? dd[q] : 0, u, v, K, F, sx, sy, sz);
        }
        point(q, sx, sy, sz);
    }
}

// Lane masks (one bit per lane of the wave, bit set only on active lanes):
// compares go straight to SGPR masks (v_cmp), combine on the scalar unit and
// feed selects through inverse_ballot, and a wave's match count is one
// s_bcnt1; a per-lane boolean would be rebuilt from a 0/1 select and a
// compare wherever it is counted (two 4-cycle VALU forms per pixel).
typedef unsigned long long LaneMask;
constexpr int kFcmpOgt = 2, kFcmpOlt = 4, kIcmpUlt = 36, kIcmpUle = 37;
__device__ __forceinline__ LaneMask mask_gt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOgt); }
__device__ __forceinline__ LaneMask mask_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOlt); }
__device__ __forceinline__ LaneMask mask_ult(unsigned a, unsigned b) { return __builtin_amdgcn_uicmp(a, b, kIcmpUlt); }
__device__ __forceinline__ LaneMask mask_ule(unsigned a, unsigned b) { return __builtin_amdgcn_uicmp(a, b, kIcmpUle); }
__device__ __forceinline__ bool lane_in(LaneMask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// ------------------------------------------------- spec a7-a9 per pixel --
// Shared by k_reduce / k_icp (accumulate_chunk), k_icp_coop (coop_group) and
// k_rgbd_reduce (survey_project and match_accumulate<kSpecSurvey>);
// oracle/icp_oracle.c assoc_one / oracle_reduce evaluate the same operations
// with the same roundings (fmaf = one rounding, -ffp-contract=off elsewhere).
//   a7  P' = R P + t:  P'_i = fma(R_i2, z, fma(R_i1, y, fma(R_i0, x, t_i)))
//       valid iff z > 0 and P'_z > 0;  rz = RN(1 / P'_z);
//       u' = floor(fma(fx P'_x, rz, cx + 0.5)), v' likewise; in range of the
//       target frame.  Unmatched pixels compute on safe values (branch-free)
//       and gather record 0.
//   kSpecSurvey: P'_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i and
//       u' = floor(((fx P'_x) / P'_z + cx) + 0.5), the
//       quotient IEEE (proj_quot on the shared correctly rounded reciprocal).

// kSpecSurvey's a7, handing out the sub-pixel coordinates uf = (fx P'x) / P'z
// + cx and vf as well: the RGB-D photometric term interpolates with them
// (DESIGN.md §13); xform_project drops them.  Statement order matters to the
// scheduler: uf, its floor, vf, its floor.
__device__ __forceinline__ void survey_project(const float* T, float sx, float sy, float sz,
                                               const Intr& K, int W, int H, float& qx, float& qy,
                                               float& qz, float& uf, float& vf, float& fu, float& fv,
                                               LaneMask& inm, int& j)
{
    qx = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3];
    qy = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7];
    qz = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11];
    const float nu = K.fx * qx, nv = K.fy * qy;
    // P'_z in [2^-60, 2^60] (proj_den_ok, which implies P'_z > 0) as ONE
    // unsigned compare on its bits (negative and NaN bit patterns lie
    // above 2^60's): every lane takes the fast quotient with den = P'_z;
    // a valid source whose P'_z is <= 0 or outside the range (never in
    // practice: tests/test_gpu_icp_hostile.py puts whole frames at P'_z <= 0,
    // which qpos rejects; P'_z in (0, 2^-60) or above 2^60 with the pixel
    // still in the frame no test reaches, profiles/hostile/mutant.txt)
    // redoes it below as the IEEE division of
    // the spec.  The
    // other lanes' quotients may be inf / NaN; the mask drops them.
    const LaneMask sok = mask_gt(sz, 0.0f);
    const LaneMask dok = mask_ule(__float_as_uint(qz) - 0x21800000u, 0x5d800000u - 0x21800000u);
    const float r = proj_recip(qz);
    float pu = proj_quot(nu, qz, r);
    float pv = proj_quot(nv, qz, r);
    LaneMask vz = sok & dok;
    const LaneMask slow = sok & ~dok;
    if (__builtin_expect(slow != 0, 0)) {  // wave-uniform
        const LaneMask qpos = mask_gt(qz, 0.0f);
        if (lane_in(slow)) {
            const float den = lane_in(qpos) ? qz : 1.0f;
            pu = nu / den;
            pv = nv / den;
        }
        vz |= slow & qpos;
    }
    // floor, in-range test and the pixel index without selects: the
    // coordinates stay finite on every lane (saturated integers), and an
    // unmatched lane's gather is masked after it (a raw buffer load past
    // the records returns 0, any index inside them is a real record).
    // The row test is the records' own: v' outside [0, H) is clamped to
    // H, whose index lies in the frame's zeroed pad (P >= N + 4) or past
    // the buffer (returns 0), a record with z = 0, which the match gate
    // (tz > 0) rejects as it rejects a target without a normal
    uf = pu + K.cx;
    const int iu = floor_i32(uf + 0.5f);
    vf = pv + K.cy;
    const int iv = floor_i32(vf + 0.5f);
    const unsigned ivc = min((unsigned)iv, (unsigned)H);
    inm = vz & mask_ult((unsigned)iu, (unsigned)W);
    fu = (float)iu;
    fv = (float)iv;
    j = (int)(__umul24(ivc, (unsigned)W) + (unsigned)iu);
}

template <int kSp>
__device__ __forceinline__ void xform_project(const float* T, float sx, float sy, float sz,
                                              const Intr& K, int W, int H, float& qx, float& qy,
                                              float& qz, float& fu, float& fv, LaneMask& inm, int& j)
{
    if (sp_survey(kSp)) {
        float uf, vf;
        survey_project(T, sx, sy, sz, K, W, H, qx, qy, qz, uf, vf, fu, fv, inm, j);
    } else {
        qx = fmaf(T[2], sz, fmaf(T[1], sy, fmaf(T[0], sx, T[3])));
        qy = fmaf(T[6], sz, fmaf(T[5], sy, fmaf(T[4], sx, T[7])));
        qz = fmaf(T[10], sz, fmaf(T[9], sy, fmaf(T[8], sx, T[11])));
        const LaneMask vz = mask_gt(sz, 0.0f) & mask_gt(qz, 0.0f);
        const float rz = proj_rcp_rn(lane_in(vz) ? qz : 1.0f);
        const float uu = floorf(fmaf(K.fx * qx, rz, K.cx + 0.5f));
        const float vv = floorf(fmaf(K.fy * qy, rz, K.cy + 0.5f));
        // 0 <= u' < W and 0 <= v' < H on the integer values: uu, vv are
        // finite integral floats (T finite, youth_icp.h), v_cvt_i32_f32
        // saturates outside the int range, and a negative one wraps to
        // >= 2^31 unsigned, so the unsigned compares equal the spec's four
        // float compares
        const int iu = (int)uu, iv = (int)vv;
        inm = vz & mask_ult((unsigned)iu, (unsigned)W) & mask_ult((unsigned)iv, (unsigned)H);
        const bool in = lane_in(inm);
        fu = in ? uu : 0.0f;
        fv = in ? vv : 0.0f;
        // 0 when !in; v', W <= 16384 (youth_icp_create): the 24-bit
        // multiply-add is exact and full rate
        j = in ? (int)__umul24((unsigned)iv, (unsigned)W) + iu : 0;
    }
}

//   a7  gate: target valid with a normal (k_prep stores z = 0 for a target
//       without one, so tz > 0 is both tests) and |P' - P_t|^2 < thr^2 with
//       d2 = fma(dz, dz, fma(dy, dy, dx dx));
//   a8  r = n.(P' - P_t) = fma(n2, dz, fma(n1, dy, n0 dx));
//       J = [P' x n, n], (P' x n)_0 = fma(qy, n2, -(qz n1)) etc.;
//   a9  lane32 (A = float): acc = fma(J_a, J_b, acc) in fp32, one rounding
//       per product-add; exact (A = double): the 28 products of fp32 values
//       are exact in fp64, one rounding per add.  Unmatched lanes skip the
//       update, or add J = 0 and r = +-0, which leaves every sum unchanged
//       (an accumulator is never -0: it starts at +0 and x + -x is +0).
//   kSpecSurvey: d2 = (dx dx + dy dy) + dz dz, r = (n0 dx + n1 dy) + n2 dz,
//       (P' x n)_0 = qy n2 - qz n1 etc. (no FMA).
// gate_accumulate takes the target's x, y as given: match_accumulate
// recomputes them from the record's z with k_prep's expression (bit-identical
// to the stored plane); the prep pass's identity iteration has them in its
// LDS planes.
template <int kSp, bool kSkip, typename A>
__device__ __forceinline__ LaneMask gate_accumulate(float qx, float qy, float qz, float tx, float ty,
                                                    f4v t, LaneMask inm, float thr2, A* acc)
{
    const float tz = t.x;
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    const float d2 = sp_survey(kSp) ? (dx * dx + dy * dy) + dz * dz
                                        : fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const LaneMask okm = inm & mask_gt(tz, 0.0f) & mask_lt(d2, thr2);
    // kSkip (the throughput kernels): unmatched lanes leave the sums
    // unchanged by not running the update (exec-masked; a wave without a
    // match skips it), k_icp 2 % faster than masking the normal.  Else
    // (k_icp_coop, latency-bound: the branches cost it 5 %,
    // profiles/r03/ab_exec_mask.txt) the normal is masked to 0, so J = 0 and
    // r = +-0 add +0 exactly: the same sums either way
    const bool ok = lane_in(okm);
    if (!kSkip || ok) {
        const float n0 = kSkip || ok ? t.y : 0.0f;
        const float n1 = kSkip || ok ? t.z : 0.0f;
        const float n2 = kSkip || ok ? t.w : 0.0f;
        float r, Jf[6];
        if (sp_survey(kSp)) {
            r = (n0 * dx + n1 * dy) + n2 * dz;
            Jf[0] = qy * n2 - qz * n1;
            Jf[1] = qz * n0 - qx * n2;
            Jf[2] = qx * n1 - qy * n0;
        } else {
            r = fmaf(n2, dz, fmaf(n1, dy, n0 * dx));
            Jf[0] = fmaf(qy, n2, -(qz * n1));
            Jf[1] = fmaf(qz, n0, -(qx * n2));
            Jf[2] = fmaf(qx, n1, -(qy * n0));
        }
        Jf[3] = n0;
        Jf[4] = n1;
        Jf[5] = n2;
        int k = 0;
        if constexpr (sizeof(A) == sizeof(float)) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int bb = a; bb < 6; ++bb) {
                    acc[k] = fmaf(Jf[a], Jf[bb], acc[k]);
                    ++k;
                }
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] = fmaf(Jf[a], r, acc[21 + a]);
            acc[27] = fmaf(r, r, acc[27]);
        } else {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int bb = a; bb < 6; ++bb) {
                    acc[k] = fma((double)Jf[a], (double)Jf[bb], acc[k]);
                    ++k;
                }
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] = fma((double)Jf[a], (double)r, acc[21 + a]);
            acc[27] = fma((double)r, (double)r, acc[27]);
        }
    }
    return okm;
}

template <int kSp, bool kFast, bool kSkip, typename A>
__device__ __forceinline__ LaneMask match_accumulate(float qx, float qy, float qz, f4v t, float fu,
                                                     float fv, LaneMask inm, const Intr& K,
                                                     const FastK& F, float thr2, A* acc)
{
    const float tz = t.x;
    const float tx = bp_div<kFast>((fu - K.cx) * tz, K.fx, F.hfx, F.lfx);
    const float ty = bp_div<kFast>((fv - K.cy) * tz, K.fy, F.hfy, F.lfy);
    return gate_accumulate<kSp, kSkip>(qx, qy, qz, tx, ty, t, inm, thr2, acc);
}

// Spec a7-a9 of one pixel at the IDENTITY pose (the first iteration of an
// align without T_init; DESIGN.md §2 "the identity lemma").  With R = I and
// t = 0 both arithmetics return P' = P bit for bit on every valid source
// pixel: 1 x is exact, 0 y and 0 z are zeros of either sign, and x + (+-0) =
// x for x != 0, (+0) + (+-0) = +0; a valid pixel (z > 0) never has x or y =
// -0 ((u - cx) z is +0 or a normal number, and so is its quotient by fx).
// The projection of P lands on the pixel it was back-projected from: uf =
// (fx x) / z + cx differs from u by at most 4 roundings of |u - cx| and one
// of u, under 0.03 px for |u - cx| < 2^17 (the host checks the intrinsics:
// ident_first_ok), so floor(uf + 0.5) = u and likewise v, in range by
// construction.  So the pixel is "in" iff its source is valid, the matched
// record is the record at its own index, and (fu, fv) are its own
// coordinates: no transform, reciprocal, quotients, floors, index or gather.
// (sx, sy, sz) as backproject4 forms them, t the target's record at pixel
// (u, v) = (fu, fv); the gate, r, J and the sums are match_accumulate's own.
template <int kSp, bool kFast, bool kSkip, typename A>
__device__ __forceinline__ LaneMask ident_accumulate(float sx, float sy, float sz, f4v t, float fu,
                                                     float fv, const Intr& K, const FastK& F,
                                                     float thr2, A* acc)
{
    return match_accumulate<kSp, kFast, kSkip>(sx, sy, sz, t, fu, fv, mask_gt(sz, 0.0f), K, F, thr2,
                                               acc);
}
// The same with the target's x, y at hand (k_prep_ident: the prep pass's LDS
// planes, which hold what match_accumulate recomputes from the record's z).
template <int kSp, bool kSkip, typename A>
__device__ __forceinline__ LaneMask ident_accumulate_xy(float sx, float sy, float sz, float tx,
                                                        float ty, f4v t, float thr2, A* acc)
{
    return gate_accumulate<kSp, kSkip>(sx, sy, sz, tx, ty, t, mask_gt(sz, 0.0f), thr2, acc);
}

// Wave sum of kN <= 32 per-lane accumulators by recursive halving: at lane
// mask m = 32, 16, 8, 4, 2 each lane keeps one half of its remaining values
// (the upper half iff lane & m) and sends the other half to lane ^ m, so the
// fp64 exchanges number 16 + 8 + 4 + 2 + 1 + 1 = 32 instead of 29 x 6 for a
// symmetric butterfly.  On exit lane 2q and 2q+1 both hold the wave total of
// value q (q < kN); the summation tree is fixed, so results are
// deterministic.  wave_reduce_scatter: k_reduce, k_icp and k_icp_coop sum
// kNeq values with it, k_rgbd_reduce the 31 of the joint record.
//   m = 32, 16: v_permlane32_swap / v_permlane16_swap exchange the upper
//     half-wave (odd rows) of one register with the lower half (even rows) of
//     another.  With vdst = v[q] and src = v[q+h], each lane is left holding
//     the value it keeps in one register and its partner's send in the other,
//     so v[q] = D + S with no select (keep + recv, commutative: bitwise the
//     same as the shuffle form).
//   m = 8, 2, 1: DPP (row_ror:8, quad_perm) moves; m = 4: ds_swizzle xor.
// No LDS bpermute; the partners (lane ^ m) and the add order are unchanged,
// so the sums are bit-identical to the shuffle form.
template <int kM>
__device__ __forceinline__ double xchg_small(double x)
{
    int lo = (int)lo32(x), hi = (int)hi32(x);
    if (kM == 8) {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x128, 0xf, 0xf, false);  // row_ror:8
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x128, 0xf, 0xf, false);
    } else if (kM == 4) {
        lo = __builtin_amdgcn_ds_swizzle(lo, 0x1F | (4 << 10));  // bit mode, xor 4
        hi = __builtin_amdgcn_ds_swizzle(hi, 0x1F | (4 << 10));
    } else if (kM == 2) {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, false);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
        hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, false);
    }
    return join64((unsigned)lo, (unsigned)hi);
}

template <int kM>
__device__ __forceinline__ void rs_stage_small(double* v, int lane)
{
    constexpr int h = kM / 2;
    const bool up = (lane & kM) != 0;
#pragma unroll
    for (int q = 0; q < h; ++q) {
        const double send = up ? v[q] : v[q + h];
        const double keep = up ? v[q + h] : v[q];
        v[q] = keep + xchg_small<kM>(send);
    }
}

template <int kN>
__device__ __forceinline__ void wave_reduce_scatter(const double* acc, int lane, double& total)
{
    static_assert(kN <= 32, "one value per lane pair");
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = q < kN ? acc[q] : 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {  // m = 32
        const auto l = __builtin_amdgcn_permlane32_swap(lo32(v[q]), lo32(v[q + 16]), false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi32(v[q]), hi32(v[q + 16]), false, false);
        v[q] = join64(l[0], h[0]) + join64(l[1], h[1]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // m = 16
        const auto l = __builtin_amdgcn_permlane16_swap(lo32(v[q]), lo32(v[q + 8]), false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi32(v[q]), hi32(v[q + 8]), false, false);
        v[q] = join64(l[0], h[0]) + join64(l[1], h[1]);
    }
    rs_stage_small<8>(v, lane);
    rs_stage_small<4>(v, lane);
    rs_stage_small<2>(v, lane);
    total = v[0] + xchg_small<1>(v[0]);
}

// ------------------------------------------- the fused solve's hand-off --
// The in-launch hand-off of k_reduce<..., kFuse> and k_rgbd_reduce
// (cdna_hip_programming.md G16, MI355X_MICROARCH.md "Valid forms" row 1), in
// two steps that wave 0 of every workgroup of pair p runs back to back, lane
// < kN holding the workgroup's sum s of value `lane`:
//   handoff_publish  write-through (sc1) stores of the workgroup's row
//                    `mine`, drained by the storing wave, then ONE agent-scope
//                    atomic per workgroup on ps.arrivals[p].  True only in the
//                    workgroup whose add returns nblk - 1, the pair's last:
//                    every other returns from the kernel.
//   handoff_sum      the last arriver adds the pair's nblk rows (kStride
//                    doubles apart) in a fixed order (k_solve's: lanes
//                    0..kN-1 the first half of the rows, lanes 32.. the second
//                    half, then one add; loads in batches of 8) and leaves the
//                    kN pair totals in neq, in every lane.
// No acquire fence between them: every load of the handed-off rows is an sc1
// load and every store of them was an sc1 store drained before the add (G16:
// the fence may then be dropped).  What a kernel does with the totals, and
// re-arming ps.arrivals[p], stays in the kernel.  Two functions and not one
// so that each kernel keeps the code shape it had with the text written out
// (the early return and neq in the kernel's own body): as one function the
// fused k_reduce measured 0.5 % slower at one pair (profiles/share/ab.txt).
template <int kN>
__device__ __forceinline__ bool handoff_publish(double* mine, const PoseState& ps, int p, int nblk,
                                                int lane, double s)
{
    if (lane < kN)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(mine) + lane,
                           (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned ticket = 0;
    if (lane == 0)
        ticket = __hip_atomic_fetch_add(ps.arrivals + p, 1u, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    return ticket == (unsigned)nblk - 1;
}

template <int kN, int kStride>
__device__ __forceinline__ void handoff_sum(const double* partials, int p, int nblk, int lane,
                                            double* neq)
{
    static_assert(kN <= 32 && kN <= kStride, "one value per lane of a half-wave");
    const unsigned long long* base =
        reinterpret_cast<const unsigned long long*>(partials + (size_t)p * nblk * kStride);
    const int half = (nblk + 1) >> 1;
    const int k = lane & 31;
    double t = 0.0;
    if (k < kN) {
        const int b0 = lane < 32 ? 0 : half;
        const int b1 = lane < 32 ? half : nblk;
        for (int bb = b0; bb < b1; bb += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                v[q] = bb + q < b1 ? __longlong_as_double((long long)__hip_atomic_load(
                                         base + (size_t)(bb + q) * kStride + k, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT))
                                   : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) t += v[q];
        }
    }
    t += __shfl_down(t, 32, 64);
#pragma unroll
    for (int q = 0; q < kN; ++q) neq[q] = __shfl(t, q, 64);
}

// ------------------------------------------------------- k_icp_coop layout --
// k_icp_coop's constants (icp_kernels.hip describes the kernel); the context
// and the launch layer size their buffers by them.
constexpr int kCoopShardStride = 32;  // words: one 128-B line per counter
constexpr int kCoopMaxPx = 32;       // source pixels per lane (LDS: 3 x 32 KB)
constexpr int kCoopMaxPairs = 16;
constexpr int kCoopBufs = 3;         // partial-row buffers per arena (iteration k % 3)
constexpr unsigned kPartEmptyHi = 0x7FF7A5A5u;  // EMPTY = 0x7FF7A5A5'7FF7A5A5 (a signalling NaN)
constexpr unsigned long long kPartEmpty = 0x7FF7A5A57FF7A5A5ull;
// counter set layout (words): timeout word (one line) | [pair][shard][32]
// prep-done counters: workgroup c of a pair arrives on shard c % 8 (one
// 128-B line each), so no line takes more than ~G/8 of the pair's arrivals
// (MI355X_MICROARCH.md "fanin": 255 arrivals on one word take 3.2 us)
constexpr int kCoopPrepShards = 8;
constexpr int kCoopErrWord = 0;
constexpr int kCoopPrepWords = kCoopErrWord + kCoopShardStride;
constexpr int kCoopPrepPair = kCoopPrepShards * kCoopShardStride;  // words per pair
constexpr int kCoopSetWords = kCoopPrepWords + kCoopMaxPairs * kCoopPrepPair;
constexpr int kCoopTileH = 24;  // fused prep tiles: 64 x 24 pixels (one per workgroup of a 640x480 pair: 200 tiles, G = 200)
constexpr int kCoopTileHTall = 80;  // 64 x 80 (= 10 px per lane x 512: one per workgroup of a 1280x960 pair, G = 240)
// Polls before a wait gives up (~0.5-1 us each: ~35-65 ms).  A wait of a
// co-resident grid ends within microseconds; one that reaches the bound has
// a workgroup that never started (the grid is not co-resident: another
// process holds CUs), and the tracker's realign then runs after one stalled
// frame instead of a stall of seconds (round 6; 2^22 polls, ~4 s, before).
// The bound counts polls, not time: a wave that is preempted does not poll.
// (A bound chosen per iteration, short for iteration 0 only, cost C2 1.9 %:
// profiles/r06/coop_spin_bound_ab_r6j.txt.)
constexpr unsigned kCoopSpinMax = 1u << 16;
constexpr int kCoopMaxChain = YOUTH_TRACK_MAX_BATCH;  // frames per tracker micro-batch

}  // namespace

#endif  // YOUTH_ICP_DEVICE_H
