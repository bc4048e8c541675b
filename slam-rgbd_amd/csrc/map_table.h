// The voxel map's hash table as its kernels see it, shared by
// voxel_map.hip (integrate, extract) and map_render.hip (render), and the door
// through which the renderer reaches a youth_map, whose layout stays private
// to voxel_map.hip.
#ifndef YOUTH_MAP_TABLE_H
#define YOUTH_MAP_TABLE_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "hip_host.h"
#include "youth_map.h"

// Internal linkage on purpose: the table travels to the kernels by value, and
// each translation unit's kernels keep the names they had before the table
// was shared.
namespace {

constexpr unsigned long long kEmpty = ~0ull;    // a key is 63 bits: never all ones
constexpr int kValWords = 8;                    // count, q[3], c[3], pad: 32 B per slot

struct MapTable {
    unsigned long long* keys;   // [cap]
    uint32_t* vals;             // [cap][kValWords]
    unsigned long long* stats;  // [kStN]
    uint32_t mask;              // cap - 1
};

// A key is (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20).
__device__ __forceinline__ void key_cell(unsigned long long key, int32_t& ix, int32_t& iy,
                                         int32_t& iz)
{
    ix = (int32_t)(key & 0x1fffff) - (1 << 20);
    iy = (int32_t)((key >> 21) & 0x1fffff) - (1 << 20);
    iz = (int32_t)((key >> 42) & 0x1fffff) - (1 << 20);
}

}  // namespace

// What a render needs of a map.  The z-buffer and the staging buffers belong
// to the map and live until it is destroyed.
struct youth_map_render_res {
    int device;
    float vpm;
    bool queue;                 // YOUTH_MAP_RENDER_QUEUE
    hipStream_t stream;         // the map's own stream
    const unsigned long long* keys;
    const uint32_t* vals;
    uint32_t mask;
    unsigned long long* zbuf;   // >= zbuf_px values, all ones between renders
    int16_t* depth;             // staging of the host API: stage_px pixels
    uint8_t* rgb;               //   stage_px * 3 bytes when asked for
    float* V;                   //   [12]
};

// Fills `out`; grows the z-buffer to zbuf_px 64-bit values (a grown buffer is
// filled with all ones on `stream`, NULL = the map's) and the staging buffers
// to stage_px pixels.  YOUTH_OK or a negative code with the error text set.
__attribute__((visibility("hidden"))) int youth_map_render_acquire(
    youth_map* m, size_t zbuf_px, size_t stage_px, bool stage_rgb, hipStream_t stream,
    youth_map_render_res* out);

// The map's channel (hip_host.h), defined in voxel_map.hip: youth_map_last_error
// reads it, and map_render.hip reports through it too.
__attribute__((visibility("hidden"))) extern thread_local youth::ErrorText g_map_err;
#define HIP_ERR g_map_err

#endif  // YOUTH_MAP_TABLE_H
