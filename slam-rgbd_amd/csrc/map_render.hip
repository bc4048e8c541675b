// Rendering the voxel map on gfx950 (C-ABI: include/youth_map_render.h; spec:
// DESIGN.md §12): int16 depth and uint8 RGB frames of the map seen from any
// pose.  The render is a z-buffer over the stored voxels.  A pixel's result is
// the MINIMUM of a packed 64-bit (depth, colour) value over the voxels that
// cover it, and every step up to that value is fp32 evaluated as written, so
// the output is one bit pattern for any launch shape, slot order or kernel
// variant.
//
//   k_map_render_splat    the grid runs over the table's slots (1024 per
//                         workgroup, keys loaded coalesced), views on
//                         gridDim.y.  An occupied slot's 32-B record gives the
//                         centroid, the camera point, the cull, the footprint
//                         and the value; every covered pixel takes one 64-bit
//                         unsigned atomic min into the view's z-buffer, skipped
//                         when a relaxed load already shows a value <= the
//                         candidate (the minimum only falls).
//                         kQueue = false: a lane walks the footprints of its
//                         own voxels.  kQueue = true: the surviving voxels are
//                         compacted into an LDS queue (ballot + prefix), an
//                         exclusive scan of their pixel counts follows, and all
//                         256 threads drain (voxel, pixel) items one per lane,
//                         so consecutive lanes hit consecutive pixels of a row.
//   k_map_render_resolve  z-buffer -> depth and colour, and all ones stored
//                         back: the next render needs no memset.
//
// The table is only read.  Few slots are occupied (2.7 % at 2^22 slots in
// tools/map_bench.py's run) and a near voxel covers up to 16 x 16 pixels, which
// is what the queue is for; which path is faster is measured by
// tools/map_render_bench.py, not assumed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "map_table.h"
#include "youth_map.h"

namespace {

constexpr int kRThreads = 256;
constexpr int kRSlots = 4;                       // slots per thread
constexpr int kRTile = kRThreads * kRSlots;      // slots per workgroup = queue capacity
constexpr int kRPx = 8;                          // pixels per thread of the resolve
constexpr unsigned long long kFar = ~0ull;       // an uncovered pixel of the z-buffer

struct RenderP {
    float fx, fy, cx, cy, ds, vpm;
    float ulim, vlim;    // (float)(W + 32), (float)(H + 32)
    float max_splat;
    int W, H;
    uint32_t min_count;
};

// A voxel's footprint clipped to the frame (w, h >= 1) and its value.
struct Splat {
    unsigned long long val;
    int x0, y0, w, h;
};

__device__ __forceinline__ float centroid_axis(int32_t i, uint32_t sum_q, float fc, float vpm)
{
    const float c = (float)sum_q / fc;
    return ((float)i + (c + 0.5f) * 0.00390625f) / vpm;
}

// DESIGN.md §12 for the voxel in `slot`; false: empty, culled or wholly
// outside the frame.
__device__ __forceinline__ bool project(const MapTable& t, uint32_t slot, const RenderP& P,
                                        const float* V, Splat& sp)
{
    const unsigned long long key = t.keys[slot];
    if (key == kEmpty) return false;
    const uint4* rec = reinterpret_cast<const uint4*>(t.vals + (size_t)slot * kValWords);
    const uint4 a = rec[0];   // count, sum_q
    const uint4 b = rec[1];   // sum_c, pad
    const uint32_t count = a.x;
    // min_count >= 1: no division by 0, and a slot vacated by a removal (its key
    // kept, count 0: youth_map_remove.h) is no voxel here either
    if (count < P.min_count) return false;
    int32_t ix, iy, iz;
    key_cell(key, ix, iy, iz);
    const float fc = (float)count;
    const float px = centroid_axis(ix, a.y, fc, P.vpm);
    const float py = centroid_axis(iy, a.z, fc, P.vpm);
    const float pz = centroid_axis(iz, a.w, fc, P.vpm);
    const float xc = ((V[0] * px + V[1] * py) + V[2] * pz) + V[3];
    const float yc = ((V[4] * px + V[5] * py) + V[6] * pz) + V[7];
    const float zc = ((V[8] * px + V[9] * py) + V[10] * pz) + V[11];
    if (!(zc > 0.0f)) return false;
    const float df = rintf(zc * P.ds);
    if (!(df >= 1.0f && df <= 32767.0f)) return false;
    const float uf = (xc * P.fx) / zc + P.cx;
    const float vf = (yc * P.fy) / zc + P.cy;
    if (!(uf > -32.0f && uf < P.ulim && vf > -32.0f && vf < P.vlim)) return false;
    // fx > 0 and vpm * zc >= 0: the quotient is never NaN; clamped in float
    const float sf = fminf(fmaxf(ceilf(P.fx / (P.vpm * zc)), 1.0f), P.max_splat);
    const int s = (int)sf;
    const float h = 0.5f * (float)(s - 1);
    const int u0 = (int)floorf((uf - h) + 0.5f);
    const int v0 = (int)floorf((vf - h) + 0.5f);
    const int x0 = max(u0, 0), x1 = min(u0 + s, P.W);
    const int y0 = max(v0, 0), y1 = min(v0 + s, P.H);
    if (x1 <= x0 || y1 <= y0) return false;
    const uint32_t half = count >> 1;
    const uint32_t R = (b.x + half) / count, G = (b.y + half) / count, B = (b.z + half) / count;
    sp.val = ((unsigned long long)(uint32_t)(int)df << 24) | (unsigned long long)(R << 16) |
             (unsigned long long)(G << 8) | (unsigned long long)B;
    sp.x0 = x0;
    sp.y0 = y0;
    sp.w = x1 - x0;
    sp.h = y1 - y0;
    return true;
}

__device__ __forceinline__ void splat_px(unsigned long long* p, unsigned long long val)
{
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > val) atomicMin(p, val);
}

struct SplatQueue {
    unsigned long long val[kRTile];
    uint32_t xy[kRTile];    // x0 | y0 << 16
    uint32_t wh[kRTile];    // w | h << 8
    uint32_t pre[kRTile];   // pixels of the entries before this one
    uint32_t wave_tot[kRThreads / 64];
    uint32_t n;
};

template <bool kQueue>
__global__ __launch_bounds__(kRThreads) void k_map_render_splat(MapTable t, RenderP P,
                                                                const float* __restrict__ d_V,
                                                                unsigned long long* __restrict__ zbuf)
{
    __shared__ __align__(8) unsigned char lds_raw[kQueue ? sizeof(SplatQueue) : 8];
    SplatQueue* q = reinterpret_cast<SplatQueue*>(lds_raw);   // unused without kQueue
    const int view = blockIdx.y;
    float V[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) V[k] = d_V[(size_t)view * 12 + k];
    unsigned long long* z = zbuf + (size_t)view * ((size_t)P.W * P.H);
    const uint32_t base = blockIdx.x * (uint32_t)kRTile + threadIdx.x;
    if (!kQueue) {
        for (int j = 0; j < kRSlots; ++j) {
            const uint32_t slot = base + (uint32_t)j * kRThreads;
            Splat sp;
            if (slot > t.mask || !project(t, slot, P, V, sp)) continue;
            for (int y = 0; y < sp.h; ++y) {
                unsigned long long* row = z + (size_t)(sp.y0 + y) * P.W + sp.x0;
                for (int x = 0; x < sp.w; ++x) splat_px(row + x, sp.val);
            }
        }
        return;
    }
    if (threadIdx.x == 0) q->n = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < kRSlots; ++j) {
        const uint32_t slot = base + (uint32_t)j * kRThreads;
        Splat sp;
        const bool ok = slot <= t.mask && project(t, slot, P, V, sp);
        const unsigned long long m = __ballot(ok);
        if (m == 0) continue;   // wave-uniform
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&q->n, (uint32_t)__popcll(m));
        at = __shfl(at, 0, 64);
        if (ok) {
            const uint32_t e = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            q->val[e] = sp.val;
            q->xy[e] = (uint32_t)sp.x0 | ((uint32_t)sp.y0 << 16);
            q->wh[e] = (uint32_t)sp.w | ((uint32_t)sp.h << 8);
        }
    }
    __syncthreads();
    const uint32_t n = q->n;
    if (n == 0) return;
    // exclusive scan of the entries' pixel counts: kRSlots entries per thread,
    // a shuffle scan per wave, the waves' totals through LDS
    uint32_t cnt[kRSlots], mine = 0;
#pragma unroll
    for (int k = 0; k < kRSlots; ++k) {
        const uint32_t e = threadIdx.x * kRSlots + k;
        const uint32_t wh = e < n ? q->wh[e] : 0u;
        cnt[k] = (wh & 0xffu) * (wh >> 8);
        mine += cnt[k];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) q->wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < kRThreads / 64; ++w) {
        const uint32_t wt = q->wave_tot[w];
        if (w < (int)(threadIdx.x >> 6)) before += wt;
        total += wt;
    }
#pragma unroll
    for (int k = 0; k < kRSlots; ++k) {
        const uint32_t e = threadIdx.x * kRSlots + k;
        if (e < n) q->pre[e] = before;
        before += cnt[k];
    }
    __syncthreads();
    // item `it` belongs to the last entry whose prefix is <= it (every entry
    // has at least one pixel, so the prefixes rise strictly)
    for (uint32_t it = threadIdx.x; it < total; it += kRThreads) {
        uint32_t lo = 0, hi = n - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (q->pre[mid] <= it)
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint32_t r = it - q->pre[lo];
        const uint32_t w = q->wh[lo] & 0xffu;
        const uint32_t y = r / w, x = r - y * w;
        const uint32_t xy = q->xy[lo];
        splat_px(z + (size_t)((xy >> 16) + y) * P.W + (xy & 0xffffu) + x, q->val[lo]);
    }
}

// Pixels [i, i + kRPx) of view blockIdx.y.  kVec: N % kRPx == 0 and the output
// bases aligned for the 16-byte depth word and the 8-byte colour words.
template <bool kVec, bool kRgb>
__global__ __launch_bounds__(kRThreads) void k_map_render_resolve(
    unsigned long long* __restrict__ zbuf, int16_t* __restrict__ depth, uint8_t* __restrict__ rgb,
    int N)
{
    const int i = (blockIdx.x * kRThreads + threadIdx.x) * kRPx;
    if (i >= N) return;
    const size_t at = (size_t)blockIdx.y * N + i;
    unsigned long long* z = zbuf + at;
    unsigned long long v[kRPx];
    if (kVec) {
        ulonglong2* z2 = reinterpret_cast<ulonglong2*>(z);
#pragma unroll
        for (int k = 0; k < kRPx / 2; ++k) {
            const ulonglong2 w = z2[k];
            v[2 * k] = w.x;
            v[2 * k + 1] = w.y;
        }
#pragma unroll
        for (int k = 0; k < kRPx / 2; ++k) z2[k] = ulonglong2{kFar, kFar};
    } else {
#pragma unroll
        for (int k = 0; k < kRPx; ++k) {
            v[k] = kFar;
            if (i + k < N) {
                v[k] = z[k];
                z[k] = kFar;
            }
        }
    }
    uint32_t dd[kRPx], cc[kRPx];   // depth, packed R << 16 | G << 8 | B
#pragma unroll
    for (int k = 0; k < kRPx; ++k) {
        const bool hit = v[k] != kFar;
        dd[k] = hit ? (uint32_t)(v[k] >> 24) : 0u;
        cc[k] = hit ? (uint32_t)v[k] & 0xffffffu : 0u;
    }
    if (kVec) {
        uint4 w;
        w.x = dd[0] | (dd[1] << 16);
        w.y = dd[2] | (dd[3] << 16);
        w.z = dd[4] | (dd[5] << 16);
        w.w = dd[6] | (dd[7] << 16);
        *reinterpret_cast<uint4*>(depth + at) = w;
        if (kRgb) {
            unsigned char by[kRPx * 3];
#pragma unroll
            for (int k = 0; k < kRPx; ++k) {
                by[3 * k] = (unsigned char)(cc[k] >> 16);
                by[3 * k + 1] = (unsigned char)(cc[k] >> 8);
                by[3 * k + 2] = (unsigned char)cc[k];
            }
            uint2* out = reinterpret_cast<uint2*>(rgb + at * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint2 o;
                o.x = by[8 * k] | (by[8 * k + 1] << 8) | (by[8 * k + 2] << 16) |
                      ((uint32_t)by[8 * k + 3] << 24);
                o.y = by[8 * k + 4] | (by[8 * k + 5] << 8) | (by[8 * k + 6] << 16) |
                      ((uint32_t)by[8 * k + 7] << 24);
                out[k] = o;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRPx; ++k) {
            if (i + k < N) {
                depth[at + k] = (int16_t)dd[k];
                if (kRgb) {
                    rgb[(at + k) * 3] = (unsigned char)(cc[k] >> 16);
                    rgb[(at + k) * 3 + 1] = (unsigned char)(cc[k] >> 8);
                    rgb[(at + k) * 3 + 2] = (unsigned char)cc[k];
                }
            }
        }
    }
}

// The limits of a view (youth_map_render.h); on success the defaults are filled in.
int check_view(const char* who, const struct youth_map_view* view, const youth_intrinsics* K,
               struct youth_map_view& v)
{
    if (!view) return g_map_err.set(YOUTH_EINVAL, "%s: null view", who);
    v = *view;
    if (!youth::frame_size_ok(v.W, v.H, 1))
        return g_map_err.set(YOUTH_EINVAL,
                             "%s: %dx%d view (need 1 <= W,H <= 16384, W*H <= 2^26)", who, v.W,
                             v.H);
    if (v.max_splat < 0 || v.max_splat > 16)
        return g_map_err.set(YOUTH_EINVAL, "%s: max_splat %d (need 0 or 1..16)", who,
                             v.max_splat);
    if (v.max_splat == 0) v.max_splat = 16;
    if (v.min_count == 0) v.min_count = 1;
    if (K && !(std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) &&
               std::isfinite(K->cy) && std::isfinite(K->depth_scale) && K->fx > 0.0f &&
               K->fy > 0.0f && K->depth_scale > 0.0f))
        return g_map_err.set(YOUTH_EINVAL,
                             "%s: intrinsics must be finite with fx, fy, depth_scale > 0", who);
    return YOUTH_OK;
}

int render_launch(const youth_map_render_res& r, int n_views, const struct youth_map_view& v,
                  const youth_intrinsics* K, const float* d_V, int16_t* d_depth, uint8_t* d_rgb,
                  hipStream_t s)
{
    // the viewer's default: 570.3, 570.3, (float)(W / 2), (float)(H / 2), 1000
    const youth_intrinsics Kd = K ? *K : youth_default_intrinsics(v.W, v.H);
    RenderP P;
    P.fx = Kd.fx;
    P.fy = Kd.fy;
    P.cx = Kd.cx;
    P.cy = Kd.cy;
    P.ds = Kd.depth_scale;
    P.vpm = r.vpm;
    P.ulim = (float)(v.W + 32);
    P.vlim = (float)(v.H + 32);
    P.max_splat = (float)v.max_splat;
    P.W = v.W;
    P.H = v.H;
    P.min_count = v.min_count;
    MapTable t{const_cast<unsigned long long*>(r.keys), const_cast<uint32_t*>(r.vals), nullptr,
               r.mask};
    const unsigned tiles = (unsigned)(((unsigned long long)r.mask + kRTile) / kRTile);
    if (r.queue)
        k_map_render_splat<true><<<dim3(tiles, n_views), kRThreads, 0, s>>>(t, P, d_V, r.zbuf);
    else
        k_map_render_splat<false><<<dim3(tiles, n_views), kRThreads, 0, s>>>(t, P, d_V, r.zbuf);
    HIP_TRY(hipGetLastError());
    const int N = v.W * v.H;
    const bool vec = (N % kRPx) == 0 && ((uintptr_t)d_depth % 16) == 0 &&
                     (!d_rgb || ((uintptr_t)d_rgb % 8) == 0);
    using Fn = void (*)(unsigned long long*, int16_t*, uint8_t*, int);
    static const Fn fn[2][2] = {
        {k_map_render_resolve<false, false>, k_map_render_resolve<false, true>},
        {k_map_render_resolve<true, false>, k_map_render_resolve<true, true>}};
    const int px = kRThreads * kRPx;
    hipLaunchKernelGGL(fn[vec][d_rgb != nullptr], dim3((N + px - 1) / px, n_views),
                       dim3(kRThreads), 0, s, r.zbuf, d_depth, d_rgb, N);
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

}  // namespace

extern "C" {

int youth_map_view_from_pose(const double T_world[16], float V[12])
{
    if (!T_world || !V) return g_map_err.set(YOUTH_EINVAL, "youth_map_view_from_pose: null argument");
    for (int q = 0; q < 12; ++q)
        if (!std::isfinite(T_world[q]))
            return g_map_err.set(YOUTH_EINVAL,
                                 "youth_map_view_from_pose: pose entry %d is not finite", q);
    const double* T = T_world;
    float out[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (float)T[4 * c + r];
        // every product and sum rounded to fp64 (the build contracts nothing)
        out[4 * r + 3] = (float)-((T[0 + r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
    }
    for (int q = 0; q < 12; ++q)
        if (!std::isfinite(out[q]))
            return g_map_err.set(YOUTH_EINVAL,
                                 "youth_map_view_from_pose: entry %d of the view is not finite", q);
    memcpy(V, out, sizeof(out));
    return YOUTH_OK;
}

int youth_map_render_device(youth_map* m, int n_views, const struct youth_map_view* view,
                            const youth_intrinsics* K, const float* d_V, int16_t* d_depth,
                            uint8_t* d_rgb, void* stream)
{
    if (!m || !d_V || !d_depth)
        return g_map_err.set(YOUTH_EINVAL, "youth_map_render_device: null argument");
    if (n_views < 1 || n_views > youth::kMaxFrames)
        return g_map_err.set(YOUTH_EINVAL, "youth_map_render_device: %d views (need 1..65535)",
                             n_views);
    struct youth_map_view v;
    int rc = check_view("youth_map_render_device", view, K, v);
    if (rc < 0) return rc;
    youth_map_render_res r;
    rc = youth_map_render_acquire(m, (size_t)n_views * v.W * v.H, 0, false, (hipStream_t)stream,
                                  &r);
    if (rc < 0) return rc;
    return render_launch(r, n_views, v, K, d_V, d_depth, d_rgb,
                         stream ? (hipStream_t)stream : r.stream);
}

int youth_map_render_host(youth_map* m, const struct youth_map_view* view, const youth_intrinsics* K,
                          const double* T_world, int16_t* depth, uint8_t* rgb)
{
    if (!m || !depth) return g_map_err.set(YOUTH_EINVAL, "youth_map_render_host: null argument");
    struct youth_map_view v;
    int rc = check_view("youth_map_render_host", view, K, v);
    if (rc < 0) return rc;
    float V[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    if (T_world && (rc = youth_map_view_from_pose(T_world, V)) < 0) return rc;
    const size_t N = (size_t)v.W * v.H;
    youth_map_render_res r;
    rc = youth_map_render_acquire(m, N, N, rgb != nullptr, nullptr, &r);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(r.V, V, sizeof(V), hipMemcpyHostToDevice, r.stream));
    rc = render_launch(r, 1, v, K, r.V, r.depth, rgb ? r.rgb : nullptr, r.stream);
    if (rc < 0) return rc;
    HIP_TRY(hipMemcpyAsync(depth, r.depth, N * sizeof(int16_t), hipMemcpyDeviceToHost, r.stream));
    if (rgb) HIP_TRY(hipMemcpyAsync(rgb, r.rgb, N * 3, hipMemcpyDeviceToHost, r.stream));
    HIP_TRY(hipStreamSynchronize(r.stream));
    return YOUTH_OK;
}

}  // extern "C"
