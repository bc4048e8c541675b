// Device helpers shared by the viewer point list (viewer_cloud.hip) and the
// voxel map (voxel_map.hip): a thread's run of depth / colour values and the
// fp32 expressions of one pixel's camera- and world-frame point.  Both kernels
// must form the same bit patterns, so the expressions live
// here once; -ffp-contract=off keeps them as written (only the fmaf calls fuse).
#ifndef YOUTH_CLOUD_BACKPROJECT_H
#define YOUTH_CLOUD_BACKPROJECT_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace youth_cloud {

struct CloudK {
    float fx, fy, cx, cy, ds;
};

// kPx depth values of pixels [i, i+kPx) of one frame.  kVec: one 8-/16-byte
// load (frame base aligned, N % kPx == 0, so i + kPx <= N whenever i < N).
template <bool kVec, int kPx>
__device__ __forceinline__ void load_depth(const int16_t* __restrict__ d, int i, int N, int* dd)
{
    if (kVec) {
        int v[kPx / 2];
        if (i < N) {
            if constexpr (kPx == 8) {
                const int4 w = *reinterpret_cast<const int4*>(d + i);
                v[0] = w.x;
                v[1] = w.y;
                v[2] = w.z;
                v[3] = w.w;
            } else {
                const int2 w = *reinterpret_cast<const int2*>(d + i);
                v[0] = w.x; v[1] = w.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPx / 2; ++k) v[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < kPx / 2; ++k) {
            dd[2 * k] = (int)(short)(v[k] & 0xffff);   // little-endian: low half first
            dd[2 * k + 1] = v[k] >> 16;                // arithmetic shift: sign kept
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPx; ++k) dd[k] = (i + k) < N ? (int)d[i + k] : 0;
    }
}

// kPx * 3 colour bytes of pixels [i, i+kPx) (viewerModule.c:348-352): kVec
// loads 8-byte (kPx 8) or 4-byte (kPx 4) words, the offset (fN + i) * 3
// being a multiple of 24 / 12.
template <bool kVec, int kPx>
__device__ __forceinline__ void load_rgb(const uint8_t* __restrict__ c, int i, int N,
                                         unsigned char* cc)
{
    if (kVec && i < N) {
        unsigned wds[kPx * 3 / 4];
        if constexpr (kPx == 8) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint2 w = *reinterpret_cast<const uint2*>(c + 8 * k);
                wds[2 * k] = w.x;
                wds[2 * k + 1] = w.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) wds[k] = *reinterpret_cast<const unsigned*>(c + 4 * k);
        }
#pragma unroll
        for (int k = 0; k < kPx * 3; ++k) cc[k] = (unsigned char)(wds[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < kPx * 3; ++k) cc[k] = (i + k / 3) < N ? c[k] : (unsigned char)0;
    }
}

// viewerModule.c:343-345, evaluated as written (IEEE quotients)
__device__ __forceinline__ void camera_point(int d, int u, int v, const CloudK& K, float& x,
                                             float& y, float& z)
{
    z = (float)d / K.ds;
    x = (((float)u - K.cx) * z) / K.fx;
    y = (((float)v - K.cy) * z) / K.fy;
}

// world frame (youth_cloud_build_device_posed): P_w = R P + t, one fma chain
// per axis in the ICP transform's order (spec a7); row = that axis's row of
// the row-major 3x4 pose
__device__ __forceinline__ float world_axis(const float* row, float x, float y, float z)
{
    return fmaf(row[2], z, fmaf(row[1], y, fmaf(row[0], x, row[3])));
}

}  // namespace youth_cloud

#endif  // YOUTH_CLOUD_BACKPROJECT_H
