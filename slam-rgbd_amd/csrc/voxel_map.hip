// Voxel map on gfx950 (C-ABI: include/youth_map.h; spec: DESIGN.md §10).
//
// World-frame point fusion: every contributing pixel of every integrated
// frame lands in one voxel of a sparse grid kept as an open-addressing hash
// table in HBM.  A record is integers only (count, sum of the in-voxel
// position q per axis, sum of R, G, B) and every accumulation is an unsigned
// integer atomic add, so the table's CONTENT does not depend on the launch
// shape, the frame order or thread timing; only the slot a voxel sits in
// does, and extraction sorts that away.
//
//   k_map_integrate  one 2048-pixel raster tile per workgroup (the viewer's
//                    tiling: 8 consecutive pixels per thread, 16-B depth and
//                    8-B colour loads).  A thread first merges runs of equal
//                    keys among its own 8 pixels in registers, then adds each
//                    run to the workgroup's LDS hash table (64-bit LDS CAS on
//                    the key, LDS integer adds).  After a barrier each occupied
//                    LDS slot goes to the global table as ONE insert (64-bit
//                    CAS on the key, only when a relaxed load does not find
//                    the key already) and one set of integer atomic adds.
//                    A run that finds no room in the LDS table within its
//                    probe bound goes straight to the global table; with
//                    YOUTH_MAP_LDS=0 every run does (no LDS is allocated).
//   k_map_update     the same tile code (voxel_map_tile.inc) taking frames out
//                    again (youth_map_remove.h): the LDS table sums a tile's runs
//                    as before, and each of its slots is then looked up in the
//                    global table without claiming anything and subtracted, the
//                    count with a returning atomic (an old value below the
//                    subtrahend is an underflow), the sums without.  A voxel
//                    emptied this way keeps its slot and key (count 0) for the
//                    next integration of the voxel.  Also both legs of a move.
//   k_map_extract    compacts the live slots (count > 0) into youth_voxel
//                    records (slot order; the host sorts).
//   k_map_scan       counts live, vacant and stale slots, on request.
//   k_map_rehash     compaction: every live slot into a fresh table.
//
// The table's layout is shared with map_render.hip (map_table.h), which renders
// the map from a pose and reaches a youth_map through youth_map_render_acquire.
//
// Atomics execute at the memory side and a hashed scatter is the one-lane-
// per-row shape, the slowest there is; the rate known for this chip was
// measured for float adds, the integer rate is not known.  The LDS table is
// there to send one insert per (tile, voxel) instead of one per pixel; what it
// buys is measured by tools/map_bench.py, not assumed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cloud_backproject.h"
#include "map_table.h"
#include "youth_map.h"

namespace {

using youth_cloud::CloudK;

constexpr int kMapThreads = 256;
constexpr int kMapPx = 8;                       // pixels per thread
constexpr int kLdsSlots = kMapThreads * kMapPx / 2;   // per-workgroup table: half the tile
constexpr int kLdsProbe = 8;                    // LDS probe bound
constexpr int kProbe = 128;                     // global probe bound
enum { kStIntegrated, kStOutOfRange, kStDropped, kStOccupied, kStDirect, kStExtracted,
       // removal (k_map_update), the scan and the rehash: beside the above, so that
       // struct youth_map_stats keeps its size
       kStRemoved, kStMissing, kStUnderflow, kStLive, kStVacant, kStStale, kStRehashFail, kStN };

struct Acc {
    unsigned long long key;
    uint32_t cnt, q[3], c[3];
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long h)
{
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// One axis of the key: false = out of range.
__device__ __forceinline__ bool axis_key(float a, float vpm, uint32_t& cell, uint32_t& q)
{
    const float s = a * vpm;
    const float fl = floorf(s);
    if (!(-1048576.0f <= fl && fl < 1048576.0f)) return false;   // NaN fails too
    const int i = (int)fl;
    const float f = s - fl;   // may round up to 1.0f for tiny negative s
    q = min(255u, (uint32_t)(f * 256.0f));
    cell = (uint32_t)(i + (1 << 20));
    return true;
}

// The slot of `key` in the global table, claiming an empty one if it is new;
// false when the probe bound is exhausted (the caller drops the point).  A
// stale relaxed load can only show "empty" for a slot that is taken, and the
// CAS then returns the slot's real key.
__device__ __forceinline__ bool global_slot(const MapTable& t, unsigned long long key,
                                            uint32_t& slot, uint32_t& claimed)
{
    const uint32_t h = (uint32_t)mix64(key);
    for (int p = 0; p < kProbe; ++p) {
        const uint32_t s = (h + (uint32_t)p) & t.mask;
        unsigned long long k =
            __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmpty) {
            k = atomicCAS(&t.keys[s], kEmpty, key);
            if (k == kEmpty) {
                ++claimed;
                slot = s;
                return true;
            }
        }
        if (k == key) {
            slot = s;
            return true;
        }
    }
    return false;
}

// The slot of `key`, never claiming one: false when an empty slot or the probe
// bound is reached first (the key is absent).  Removal runs after the
// integrations it undoes, in stream order, so every key it looks for is visible.
__device__ __forceinline__ bool global_find(const MapTable& t, unsigned long long key, uint32_t& slot)
{
    const uint32_t h = (uint32_t)mix64(key);
    for (int p = 0; p < kProbe; ++p) {
        const uint32_t s = (h + (uint32_t)p) & t.mask;
        const unsigned long long k =
            __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == key) {
            slot = s;
            return true;
        }
        if (k == kEmpty) return false;
    }
    return false;
}

// A removing launch counts removed / missing / underflow where an adding one
// counts integrated / dropped / occupied; out_of_range and direct it leaves alone.
struct Tally {
    uint32_t integrated = 0, out_of_range = 0, dropped = 0, occupied = 0, direct = 0;
};

// A run (or an LDS slot's sum) out of the global table.  The slot keeps its key
// (open addressing cannot hand it back): a vacated slot has count 0.  The count
// is subtracted with a returning atomic, which is what detects an underflow; the
// sums need no answer.
template <bool kRgb>
__device__ __forceinline__ void global_sub(const MapTable& t, const Acc& a, Tally& n)
{
    uint32_t slot;
    if (!global_find(t, a.key, slot)) {
        n.dropped += a.cnt;   // missing
        return;
    }
    uint32_t* v = t.vals + (size_t)slot * kValWords;
    const uint32_t old = atomicSub(v + 0, a.cnt);
    if (old < a.cnt) ++n.occupied;   // one underflow event
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicSub(v + 1 + j, a.q[j]);
    if (kRgb) {
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicSub(v + 4 + j, a.c[j]);
    }
    n.integrated += a.cnt;   // removed
}

// A run (or an LDS slot's sum) into the global table, or with kRemove out of it.
template <bool kRgb, bool kRemove = false>
__device__ __forceinline__ void global_add(const MapTable& t, const Acc& a, Tally& n)
{
    if (kRemove) {
        global_sub<kRgb>(t, a, n);
        return;
    }
    uint32_t slot;
    if (!global_slot(t, a.key, slot, n.occupied)) {
        n.dropped += a.cnt;
        return;
    }
    uint32_t* v = t.vals + (size_t)slot * kValWords;
    atomicAdd(v + 0, a.cnt);
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(v + 1 + j, a.q[j]);
    if (kRgb) {
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicAdd(v + 4 + j, a.c[j]);
    }
    n.integrated += a.cnt;
}

struct LdsTable {
    unsigned long long keys[kLdsSlots];
    uint32_t vals[7][kLdsSlots];   // [word][slot]: a flush reads consecutive banks
};

template <bool kLds, bool kRgb, bool kRemove = false>
__device__ __forceinline__ void emit_run(const MapTable& t, LdsTable* lt, const Acc& a, Tally& n)
{
    if (kLds) {
        const uint32_t h = (uint32_t)(mix64(a.key) >> 32);
        for (int p = 0; p < kLdsProbe; ++p) {
            const uint32_t s = (h + (uint32_t)p) & (kLdsSlots - 1);
            const unsigned long long k = atomicCAS(&lt->keys[s], kEmpty, a.key);
            if (k == kEmpty || k == a.key) {
                atomicAdd(&lt->vals[0][s], a.cnt);
#pragma unroll
                for (int j = 0; j < 3; ++j) atomicAdd(&lt->vals[1 + j][s], a.q[j]);
                if (kRgb) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) atomicAdd(&lt->vals[4 + j][s], a.c[j]);
                }
                return;
            }
        }
    }
    if (!kRemove) n.direct += a.cnt;   // the LDS table has no room for this key (or there is none)
    global_add<kRgb, kRemove>(t, a, n);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <bool kVec, bool kLds, bool kRgb>
__global__ __launch_bounds__(kMapThreads) void k_map_integrate(
    const int16_t* __restrict__ depth, const uint8_t* __restrict__ rgb, int W, int N, CloudK K,
    const float* __restrict__ T_world, float vpm, int max_depth, MapTable t)
{
    constexpr bool kRemove = false;
#include "voxel_map_tile.inc"
}

// k_map_integrate's removing form (kRemove) and the two legs of a move: the
// same tile code.  T_other, when given, is the move's other pose array: a frame
// whose twelve floats are bitwise equal in both stays where it is and is
// skipped by both legs.  The test is uniform over the workgroup, so the early
// return is taken before any barrier by all of its threads or by none.
template <bool kVec, bool kLds, bool kRgb, bool kRemove>
__global__ __launch_bounds__(kMapThreads) void k_map_update(
    const int16_t* __restrict__ depth, const uint8_t* __restrict__ rgb, int W, int N, CloudK K,
    const float* __restrict__ T_world, const float* __restrict__ T_other, float vpm, int max_depth,
    MapTable t)
{
    if (T_other) {
        const size_t at = (size_t)blockIdx.y * 12;
        bool same = true;
#pragma unroll
        for (int q = 0; q < 12; ++q)
            same = same && __float_as_uint(T_world[at + q]) == __float_as_uint(T_other[at + q]);
        if (same) return;
    }
#include "voxel_map_tile.inc"
}

// Live slots -> records, in slot order of arrival (the host sorts).  A slot
// vacated by a removal (count 0) holds no record; a map that was only ever
// added to has none, because a claimed slot receives its add in the same launch.
__global__ __launch_bounds__(kMapThreads) void k_map_extract(MapTable t, youth_voxel* __restrict__ out,
                                                             uint32_t cap)
{
    const uint32_t s = blockIdx.x * kMapThreads + threadIdx.x;
    if (s > t.mask) return;
    const unsigned long long key = t.keys[s];
    if (key == kEmpty) return;
    const uint32_t* v = t.vals + (size_t)s * kValWords;
    if (v[0] == 0) return;
    const uint32_t at = (uint32_t)atomicAdd(&t.stats[kStExtracted], 1ull);
    if (at >= cap) return;
    youth_voxel r;
    key_cell(key, r.ix, r.iy, r.iz);
    r.count = v[0];
    for (int j = 0; j < 3; ++j) {
        r.sum_q[j] = v[1 + j];
        r.sum_c[j] = v[4 + j];
    }
    out[at] = r;
}

// One pass over the table: live (key, count > 0), vacant (key, count 0) and
// stale (vacant with a sum left over) slots, exact whatever was interleaved
// before it.  The host zeroes the three counters first.
__global__ __launch_bounds__(kMapThreads) void k_map_scan(MapTable t)
{
    const uint32_t s = blockIdx.x * kMapThreads + threadIdx.x;
    uint32_t live = 0, vacant = 0, stale = 0;
    if (s <= t.mask && t.keys[s] != kEmpty) {
        const uint4* v = reinterpret_cast<const uint4*>(t.vals + (size_t)s * kValWords);
        const uint4 a = v[0], b = v[1];   // count q q q | c c c pad
        live = a.x != 0;
        vacant = a.x == 0;
        stale = vacant && (a.y | a.z | a.w | b.x | b.y | b.z) != 0;
    }
    const uint32_t sums[3] = {wave_sum_u32(live), wave_sum_u32(vacant), wave_sum_u32(stale)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (sums[j]) atomicAdd(&t.stats[kStLive + j], (unsigned long long)sums[j]);
    }
}

// Every live slot of `t` into the fresh table (keys, vals) of the same
// capacity.  Keys are unique, so a claim is one CAS on an empty slot and the
// eight value words are plain stores.  A key that finds no slot within the
// probe bound is counted (kStRehashFail, in the old table's stats) and the host
// keeps the old table; the moved slots are counted as live.
__global__ __launch_bounds__(kMapThreads) void k_map_rehash(MapTable t, unsigned long long* keys,
                                                            uint32_t* vals)
{
    const uint32_t s = blockIdx.x * kMapThreads + threadIdx.x;
    if (s > t.mask) return;
    const unsigned long long key = t.keys[s];
    if (key == kEmpty) return;
    const uint4* v = reinterpret_cast<const uint4*>(t.vals + (size_t)s * kValWords);
    if (t.vals[(size_t)s * kValWords] == 0) return;   // vacated: nothing to move
    const uint32_t h = (uint32_t)mix64(key);
    for (int p = 0; p < kProbe; ++p) {
        const uint32_t d = (h + (uint32_t)p) & t.mask;
        if (__hip_atomic_load(&keys[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kEmpty) continue;
        if (atomicCAS(&keys[d], kEmpty, key) != kEmpty) continue;
        uint4* o = reinterpret_cast<uint4*>(vals + (size_t)d * kValWords);
        o[0] = v[0];   // count q q q
        o[1] = v[1];   // c c c pad
        atomicAdd(&t.stats[kStLive], 1ull);
        return;
    }
    atomicAdd(&t.stats[kStRehashFail], 1ull);
}

}  // namespace

// =============================================================== host side ==

thread_local youth::ErrorText g_map_err;   // map_table.h

struct youth_map {
    int device = 0;
    float vpm = 0.0f;
    long long cap = 0;
    bool lds = true;      // YOUTH_MAP_LDS
    int max_depth = 0;
    hipStream_t stream = nullptr;
    MapTable t{};
    // host API staging (one frame) and the extraction buffer, grown on demand
    int16_t* d_depth = nullptr;
    uint8_t* d_rgb = nullptr;
    size_t depth_cap = 0, rgb_cap = 0;
    float* d_T = nullptr;   // [12]
    youth_voxel* d_rec = nullptr;
    size_t rec_cap = 0;
    // rendering (map_render.hip): the z-buffer, all ones between renders
    bool render_queue = true;   // YOUTH_MAP_RENDER_QUEUE
    unsigned long long* d_zbuf = nullptr;
    size_t zbuf_cap = 0;        // 64-bit values
};

static void map_free(youth_map* m)
{
    if (!m) return;
    if (hipSetDevice(m->device) == hipSuccess) {
        if (m->stream) (void)hipStreamSynchronize(m->stream);
        (void)hipFree(m->t.keys);
        (void)hipFree(m->t.vals);
        (void)hipFree(m->t.stats);
        (void)hipFree(m->d_depth);
        (void)hipFree(m->d_rgb);
        (void)hipFree(m->d_T);
        (void)hipFree(m->d_rec);
        (void)hipFree(m->d_zbuf);
        if (m->stream) (void)hipStreamDestroy(m->stream);
    }
    delete m;
}

// stats (host order) after the map's stream has drained
static int map_read_stats(youth_map* m, unsigned long long* st)
{
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(st, m->t.stats, kStN * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return YOUTH_OK;
}

// the host API's staging buffers, grown to N pixels
static int map_stage(youth_map* m, size_t N, bool rgb)
{
    if (m->depth_cap >= N && (!rgb || m->rgb_cap >= N)) return YOUTH_OK;
    // no copy of an earlier call may still be in flight on the old buffers
    HIP_TRY(hipStreamSynchronize(m->stream));
    const int rc = grow_device_buffer(g_map_err, &m->d_depth, &m->depth_cap, N);
    if (rc < 0 || !rgb) return rc;
    return grow_device_buffer(g_map_err, &m->d_rgb, &m->rgb_cap, N, 3);
}

// map_table.h: the renderer's door to a map
int youth_map_render_acquire(youth_map* m, size_t zbuf_px, size_t stage_px, bool stage_rgb,
                             hipStream_t stream, youth_map_render_res* out)
{
    HIP_TRY(hipSetDevice(m->device));
    if (m->zbuf_cap < zbuf_px) {
        const int rc = grow_device_buffer(g_map_err, &m->d_zbuf, &m->zbuf_cap, zbuf_px);
        if (rc < 0) return rc;
        HIP_TRY(hipMemsetAsync(m->d_zbuf, 0xff, zbuf_px * sizeof(unsigned long long),
                               stream ? stream : m->stream));
    }
    if (stage_px) {
        const int rs = map_stage(m, stage_px, stage_rgb);
        if (rs < 0) return rs;
    }
    out->device = m->device;
    out->vpm = m->vpm;
    out->queue = m->render_queue;
    out->stream = m->stream;
    out->keys = m->t.keys;
    out->vals = m->t.vals;
    out->mask = m->t.mask;
    out->zbuf = m->d_zbuf;
    out->depth = m->d_depth;
    out->rgb = m->d_rgb;
    out->V = m->d_T;
    return YOUTH_OK;
}

static double voxel_axis(int32_t i, uint32_t sum_q, uint32_t count, float vpm)
{
    return ((double)i + ((double)sum_q / (double)count + 0.5) / 256.0) / (double)vpm;
}

extern "C" {

const char* youth_map_last_error(void) { return g_map_err.c_str(); }

youth_map* youth_map_create(int device, float vpm, long long capacity_slots)
{
    if (!std::isfinite(vpm) || !(vpm > 0.0f) || capacity_slots < 1 ||
        capacity_slots > (1LL << 28)) {
        g_map_err.set(YOUTH_EINVAL,
                      "youth_map_create: vpm %g, %lld slots (need finite vpm > 0, 1 <= slots <= 2^28)",
                      (double)vpm, capacity_slots);
        return nullptr;
    }
    if (youth::check_device(g_map_err, "youth_map_create", device) < 0) return nullptr;
    auto* m = new youth_map;
    m->device = device;
    m->vpm = vpm;
    m->cap = 64;
    while (m->cap < capacity_slots) m->cap <<= 1;
    if (const char* e = getenv("YOUTH_MAP_LDS")) m->lds = atoi(e) != 0;
    if (const char* e = getenv("YOUTH_MAP_RENDER_QUEUE")) m->render_queue = atoi(e) != 0;
    m->t.mask = (uint32_t)(m->cap - 1);
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&m->t.keys, (size_t)m->cap * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&m->t.vals, (size_t)m->cap * kValWords * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&m->t.stats, kStN * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&m->d_T, 12 * sizeof(float)) != hipSuccess) {
        g_map_err.set(YOUTH_ENOMEM, "youth_map_create: device allocation failed (%lld slots)", m->cap);
        map_free(m);
        return nullptr;
    }
    if (youth_map_clear(m) < 0) {
        map_free(m);
        return nullptr;
    }
    return m;
}

void youth_map_destroy(youth_map* m) { map_free(m); }

int youth_map_clear(youth_map* m)
{
    if (!m) return g_map_err.set(YOUTH_EINVAL, "youth_map_clear: null map");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemsetAsync(m->t.keys, 0xff, (size_t)m->cap * sizeof(unsigned long long), m->stream));
    HIP_TRY(hipMemsetAsync(m->t.vals, 0, (size_t)m->cap * kValWords * sizeof(uint32_t), m->stream));
    HIP_TRY(hipMemsetAsync(m->t.stats, 0, kStN * sizeof(unsigned long long), m->stream));
    return YOUTH_OK;
}

int youth_map_set_max_depth(youth_map* m, int max_depth)
{
    if (!m || max_depth < 0)
        return g_map_err.set(YOUTH_EINVAL, "youth_map_set_max_depth: null map or negative depth");
    m->max_depth = max_depth;
    return YOUTH_OK;
}

// Shared by the integrate, remove and move entry points (`who` names the one
// reporting): the checks, the launch shape and the launch of one kernel over
// n_frames frames.  kAdd runs k_map_integrate; kRemoveLeg / kAddLeg run
// k_map_update, which also takes the other pose array of a move (or NULL).
enum MapLeg { kAdd, kRemoveLeg, kAddLeg };

static int map_launch(youth_map* m, const char* who, MapLeg leg, const int16_t* d_depth,
                      const uint8_t* d_rgb, int n_frames, int W, int H, const youth_intrinsics* K,
                      const float* d_T_world, const float* d_T_other, void* stream)
{
    if (!m || !d_depth) return g_map_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if (n_frames < 0 || n_frames > youth::kMaxFrames || !youth::frame_size_ok(W, H, 1))
        return g_map_err.set(YOUTH_EINVAL,
                             "%s: %d frames of %dx%d (need 0 <= frames <= 65535, "
                             "1 <= W,H <= 16384, W*H <= 2^26)",
                             who, n_frames, W, H);
    if (n_frames == 0) return YOUTH_OK;
    HIP_TRY(hipSetDevice(m->device));
    const int N = W * H;
    const int tile_px = kMapThreads * kMapPx;
    const int tiles = (N + tile_px - 1) / tile_px;
    // the viewer's default: 570.3, 570.3, (float)(W / 2), (float)(H / 2), 1000
    const youth_intrinsics Kd = K ? *K : youth_default_intrinsics(W, H);
    const CloudK k{Kd.fx, Kd.fy, Kd.cx, Kd.cy, Kd.depth_scale};
    hipStream_t s = stream ? (hipStream_t)stream : m->stream;
    // vector loads: every frame base and thread offset aligned for the 16-byte
    // depth word and the 8-byte colour words (as k_cloud_emit)
    const bool vec = (N % kMapPx) == 0 && ((uintptr_t)d_depth % 16) == 0 &&
                     (!d_rgb || ((uintptr_t)d_rgb % 8) == 0);
    const dim3 grid(tiles, n_frames), block(kMapThreads);
    if (leg == kAdd) {
        using Fn = void (*)(const int16_t*, const uint8_t*, int, int, CloudK, const float*, float, int,
                            MapTable);
        static const Fn fn[2][2][2] = {
            {{k_map_integrate<false, false, false>, k_map_integrate<false, false, true>},
             {k_map_integrate<false, true, false>, k_map_integrate<false, true, true>}},
            {{k_map_integrate<true, false, false>, k_map_integrate<true, false, true>},
             {k_map_integrate<true, true, false>, k_map_integrate<true, true, true>}}};
        hipLaunchKernelGGL(fn[vec][m->lds][d_rgb != nullptr], grid, block, 0, s, d_depth, d_rgb, W, N,
                           k, d_T_world, m->vpm, m->max_depth, m->t);
    } else {
        using Fn = void (*)(const int16_t*, const uint8_t*, int, int, CloudK, const float*,
                            const float*, float, int, MapTable);
#define YOUTH_MAP_UPDATE_FNS(R)                                                                  \
    {{{k_map_update<false, false, false, R>, k_map_update<false, false, true, R>},               \
      {k_map_update<false, true, false, R>, k_map_update<false, true, true, R>}},                \
     {{k_map_update<true, false, false, R>, k_map_update<true, false, true, R>},                 \
      {k_map_update<true, true, false, R>, k_map_update<true, true, true, R>}}}
        static const Fn fn[2][2][2][2] = {YOUTH_MAP_UPDATE_FNS(false), YOUTH_MAP_UPDATE_FNS(true)};
#undef YOUTH_MAP_UPDATE_FNS
        hipLaunchKernelGGL(fn[leg == kRemoveLeg][vec][m->lds][d_rgb != nullptr], grid, block, 0, s,
                           d_depth, d_rgb, W, N, k, d_T_world, d_T_other, m->vpm, m->max_depth, m->t);
    }
    HIP_TRY(hipGetLastError());
    return YOUTH_OK;
}

// One host frame in (kAdd) or out (kRemoveLeg) through the staging buffers.
static int map_host_frame(youth_map* m, const char* who, MapLeg leg, const int16_t* depth,
                          const uint8_t* rgb, int W, int H, const youth_intrinsics* K,
                          const double* T_world)
{
    if (!m || !depth) return g_map_err.set(YOUTH_EINVAL, "%s: null argument", who);
    if (!youth::frame_size_ok(W, H, 1))
        return g_map_err.set(YOUTH_EINVAL, "%s: %dx%d frame", who, W, H);
    float T32[12];
    if (T_world) {
        for (int q = 0; q < 12; ++q) {
            T32[q] = (float)T_world[q];
            if (!std::isfinite(T_world[q]) || !std::isfinite(T32[q]))
                return g_map_err.set(YOUTH_EINVAL, "%s: pose entry %d is not finite", who, q);
        }
    }
    HIP_TRY(hipSetDevice(m->device));
    const size_t N = (size_t)W * H;
    const int rs = map_stage(m, N, rgb != nullptr);
    if (rs < 0) return rs;
    HIP_TRY(hipMemcpyAsync(m->d_depth, depth, N * sizeof(int16_t), hipMemcpyHostToDevice, m->stream));
    if (rgb) HIP_TRY(hipMemcpyAsync(m->d_rgb, rgb, N * 3, hipMemcpyHostToDevice, m->stream));
    if (T_world)
        HIP_TRY(hipMemcpyAsync(m->d_T, T32, sizeof(T32), hipMemcpyHostToDevice, m->stream));
    const int rc = map_launch(m, who, leg, m->d_depth, rgb ? m->d_rgb : nullptr, 1, W, H, K,
                              T_world ? m->d_T : nullptr, nullptr, m->stream);
    if (rc < 0) return rc;
    // the staging buffers and the caller's frame are free again on return
    HIP_TRY(hipStreamSynchronize(m->stream));
    return YOUTH_OK;
}

int youth_map_integrate_device(youth_map* m, const int16_t* d_depth, const uint8_t* d_rgb,
                               int n_frames, int W, int H, const youth_intrinsics* K,
                               const float* d_T_world, void* stream)
{
    return map_launch(m, "youth_map_integrate_device", kAdd, d_depth, d_rgb, n_frames, W, H, K,
                      d_T_world, nullptr, stream);
}

int youth_map_integrate_host(youth_map* m, const int16_t* depth, const uint8_t* rgb, int W, int H,
                             const youth_intrinsics* K, const double* T_world)
{
    return map_host_frame(m, "youth_map_integrate_host", kAdd, depth, rgb, W, H, K, T_world);
}

int youth_map_remove_device(youth_map* m, const int16_t* d_depth, const uint8_t* d_rgb, int n_frames,
                            int W, int H, const youth_intrinsics* K, const float* d_T_world,
                            void* stream)
{
    return map_launch(m, "youth_map_remove_device", kRemoveLeg, d_depth, d_rgb, n_frames, W, H, K,
                      d_T_world, nullptr, stream);
}

int youth_map_remove_host(youth_map* m, const int16_t* depth, const uint8_t* rgb, int W, int H,
                          const youth_intrinsics* K, const double* T_world)
{
    return map_host_frame(m, "youth_map_remove_host", kRemoveLeg, depth, rgb, W, H, K, T_world);
}

int youth_map_move_device(youth_map* m, const int16_t* d_depth, const uint8_t* d_rgb, int n_frames,
                          int W, int H, const youth_intrinsics* K, const float* d_T_old,
                          const float* d_T_new, void* stream)
{
    if (!d_T_old || !d_T_new)
        return g_map_err.set(YOUTH_EINVAL, "youth_map_move_device: null argument");
    // removal first: a voxel's count never passes through a value it did not
    // have, so an underflow still means a frame that was not in the map
    const int rc = map_launch(m, "youth_map_move_device", kRemoveLeg, d_depth, d_rgb, n_frames, W, H,
                              K, d_T_old, d_T_new, stream);
    if (rc < 0) return rc;
    return map_launch(m, "youth_map_move_device", kAddLeg, d_depth, d_rgb, n_frames, W, H, K, d_T_new,
                      d_T_old, stream);
}

int youth_map_compact(youth_map* m)
{
    if (!m) return g_map_err.set(YOUTH_EINVAL, "youth_map_compact: null map");
    HIP_TRY(hipSetDevice(m->device));
    unsigned long long* keys = nullptr;
    uint32_t* vals = nullptr;
    if (hipMalloc(&keys, (size_t)m->cap * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&vals, (size_t)m->cap * kValWords * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(keys);
        return g_map_err.set(YOUTH_ENOMEM, "youth_map_compact: device allocation failed (%lld slots)",
                             m->cap);
    }
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(m->stream);
        (void)hipFree(keys);
        (void)hipFree(vals);
        return rc;
    };
    const unsigned blocks = (unsigned)((m->cap + kMapThreads - 1) / kMapThreads);
    unsigned long long st[kStN];
    if (hipMemsetAsync(keys, 0xff, (size_t)m->cap * sizeof(unsigned long long), m->stream) != hipSuccess ||
        hipMemsetAsync(vals, 0, (size_t)m->cap * kValWords * sizeof(uint32_t), m->stream) != hipSuccess ||
        hipMemsetAsync(m->t.stats + kStLive, 0, (kStN - kStLive) * sizeof(unsigned long long),
                       m->stream) != hipSuccess)
        return fail(youth::hip_failed(g_map_err, hipGetLastError(), __FILE_NAME__, __LINE__));
    k_map_rehash<<<blocks, kMapThreads, 0, m->stream>>>(m->t, keys, vals);
    if (hipGetLastError() != hipSuccess || map_read_stats(m, st) < 0)
        return fail(g_map_err.set(YOUTH_EHIP, "youth_map_compact: the rehash did not run"));
    if (st[kStRehashFail] != 0)   // all or nothing: the old table was only read
        return fail(g_map_err.set(YOUTH_ENOMEM,
                                  "youth_map_compact: %llu voxels found no slot within the probe "
                                  "bound; the map is unchanged",
                                  st[kStRehashFail]));
    std::swap(m->t.keys, keys);
    std::swap(m->t.vals, vals);
    (void)hipFree(keys);
    (void)hipFree(vals);
    // occupied becomes live; nothing is vacant in the fresh table
    HIP_TRY(hipMemcpyAsync(m->t.stats + kStOccupied, &st[kStLive], sizeof(unsigned long long),
                           hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return YOUTH_OK;
}

int youth_map_remove_stats(youth_map* m, struct youth_map_remove_stats* out)
{
    if (!m || !out) return g_map_err.set(YOUTH_EINVAL, "youth_map_remove_stats: null argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemsetAsync(m->t.stats + kStLive, 0, 3 * sizeof(unsigned long long), m->stream));
    const unsigned blocks = (unsigned)((m->cap + kMapThreads - 1) / kMapThreads);
    k_map_scan<<<blocks, kMapThreads, 0, m->stream>>>(m->t);
    HIP_TRY(hipGetLastError());
    unsigned long long st[kStN];
    const int rc = map_read_stats(m, st);
    if (rc < 0) return rc;
    out->removed = st[kStRemoved];
    out->missing = st[kStMissing];
    out->underflow = st[kStUnderflow];
    out->live = st[kStLive];
    out->vacant = st[kStVacant];
    out->stale = st[kStStale];
    return YOUTH_OK;
}

long long youth_map_voxels(youth_map* m)
{
    if (!m) return g_map_err.set(YOUTH_EINVAL, "youth_map_voxels: null map");
    unsigned long long st[kStN];
    const int rc = map_read_stats(m, st);
    return rc < 0 ? rc : (long long)st[kStOccupied];
}

int youth_map_stats(youth_map* m, struct youth_map_stats* out)
{
    if (!m || !out) return g_map_err.set(YOUTH_EINVAL, "youth_map_stats: null argument");
    unsigned long long st[kStN];
    const int rc = map_read_stats(m, st);
    if (rc < 0) return rc;
    out->integrated = st[kStIntegrated];
    out->out_of_range = st[kStOutOfRange];
    out->dropped = st[kStDropped];
    out->occupied = st[kStOccupied];
    out->direct = st[kStDirect];
    out->capacity = (uint64_t)m->cap;
    return YOUTH_OK;
}

int youth_map_extract(youth_map* m, youth_voxel* out, int cap)
{
    if (!m || cap < 0 || (!out && cap > 0))
        return g_map_err.set(YOUTH_EINVAL, "youth_map_extract: null argument");
    unsigned long long st[kStN];
    int rc = map_read_stats(m, st);
    if (rc < 0) return rc;
    size_t n = (size_t)st[kStOccupied];
    if (n > (size_t)cap)
        return g_map_err.set(YOUTH_EINVAL, "youth_map_extract: %zu voxels, room for %d", n, cap);
    if (n == 0) return 0;
    rc = grow_device_buffer(g_map_err, &m->d_rec, &m->rec_cap, n);
    if (rc < 0) return rc;
    HIP_TRY(hipMemsetAsync(m->t.stats + kStExtracted, 0, sizeof(unsigned long long), m->stream));
    const unsigned blocks = (unsigned)((m->cap + kMapThreads - 1) / kMapThreads);
    k_map_extract<<<blocks, kMapThreads, 0, m->stream>>>(m->t, m->d_rec, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    // n bounds the records; their exact number (slots vacated by a removal hold
    // none) is what the kernel counted
    unsigned long long live = 0;
    HIP_TRY(hipMemcpyAsync(&live, m->t.stats + kStExtracted, sizeof(live), hipMemcpyDeviceToHost,
                           m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (live > n) return g_map_err.set(YOUTH_EHIP, "youth_map_extract: %llu records of %zu slots", live, n);
    n = (size_t)live;
    if (n == 0) return 0;
    HIP_TRY(hipMemcpyAsync(out, m->d_rec, n * sizeof(youth_voxel), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    // the slot order depends on which wave won an insert: never leaves here
    std::sort(out, out + n, [](const youth_voxel& a, const youth_voxel& b) {
        if (a.iz != b.iz) return a.iz < b.iz;
        if (a.iy != b.iy) return a.iy < b.iy;
        return a.ix < b.ix;
    });
    return (int)n;
}

int youth_map_sync(youth_map* m, void* stream)
{
    if (!m) return g_map_err.set(YOUTH_EINVAL, "youth_map_sync: null map");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(stream ? (hipStream_t)stream : m->stream));
    return YOUTH_OK;
}

int youth_map_points(const youth_voxel* vox, int n, float vpm, float* xyzrgb)
{
    if (n < 0 || (n > 0 && (!vox || !xyzrgb)) || !std::isfinite(vpm) || !(vpm > 0.0f))
        return g_map_err.set(YOUTH_EINVAL, "youth_map_points: bad argument");
    for (int k = 0; k < n; ++k) {
        const youth_voxel& r = vox[k];
        if (r.count == 0) return g_map_err.set(YOUTH_EINVAL, "youth_map_points: record %d is empty", k);
        float* o = xyzrgb + (size_t)k * 6;
        o[0] = (float)voxel_axis(r.ix, r.sum_q[0], r.count, vpm);
        o[1] = (float)voxel_axis(r.iy, r.sum_q[1], r.count, vpm);
        o[2] = (float)voxel_axis(r.iz, r.sum_q[2], r.count, vpm);
        for (int j = 0; j < 3; ++j) o[3 + j] = (float)((double)r.sum_c[j] / (double)r.count / 255.0);
    }
    return YOUTH_OK;
}

int youth_map_write_ply(const char* path, const youth_voxel* vox, int n, float vpm)
{
    if (!path || n < 0 || (n > 0 && !vox) || !std::isfinite(vpm) || !(vpm > 0.0f))
        return g_map_err.set(YOUTH_EINVAL, "youth_map_write_ply: bad argument");
    for (int k = 0; k < n; ++k)
        if (vox[k].count == 0)
            return g_map_err.set(YOUTH_EINVAL, "youth_map_write_ply: record %d is empty", k);
    FILE* f = fopen(path, "w");
    if (!f) return g_map_err.set(YOUTH_EINVAL, "youth_map_write_ply: cannot open %s", path);
    fprintf(f,
            "ply\nformat ascii 1.0\ncomment youth_map voxels_per_metre %.9g\n"
            "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property uint count\nend_header\n",
            (double)vpm, n);
    for (int k = 0; k < n; ++k) {
        const youth_voxel& r = vox[k];
        unsigned c[3];
        for (int j = 0; j < 3; ++j)   // the mean colour, rounded to nearest
            c[j] = (unsigned)((2ull * r.sum_c[j] + r.count) / (2ull * r.count));
        fprintf(f, "%.9g %.9g %.9g %u %u %u %u\n",
                (double)(float)voxel_axis(r.ix, r.sum_q[0], r.count, vpm),
                (double)(float)voxel_axis(r.iy, r.sum_q[1], r.count, vpm),
                (double)(float)voxel_axis(r.iz, r.sum_q[2], r.count, vpm), c[0], c[1], c[2],
                r.count);
    }
    const int ok = ferror(f) == 0;
    if (fclose(f) != 0 || !ok) return g_map_err.set(YOUTH_EINVAL, "youth_map_write_ply: write to %s failed", path);
    return YOUTH_OK;
}

}  // extern "C"
