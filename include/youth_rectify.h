/*
 * youth_rectify.h — C-ABI of the lens rectifier on MI355X.
 *
 * Every other unit assumes an ideal pinhole camera.  The rectifier resamples a
 * sensor's depth and colour frames, distorted by the Brown-Conrady model with
 * OpenCV's coefficients D = (k1, k2, p1, p2, k3), into the frames an ideal
 * pinhole camera Ko would have taken.  Lens distortion does not change Z, so
 * depth is resampled, not recomputed.  Opt-in: nothing else in the library
 * calls it except the SLAM drop-in under YOUTH_SLAM_RECTIFY=1 (below).
 *
 * Definition.  K = (fx, fy, cx, cy, ds) is the sensor's camera, Ko the output
 * camera (NULL: K; its depth scale must equal K's), frames are W x H in and
 * out.  The map of output pixel (u, v), all fp32, every operation rounded as
 * written, no FMA, IEEE division:
 *   x = ((float)u - cxo) / fxo          y = ((float)v - cyo) / fyo
 *   r2 = x x + y y                      rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *   xy = x y
 *   tx = (2 p1) xy + p2 (r2 + 2 (x x))  ty = p1 (r2 + 2 (y y)) + (2 p2) xy
 *   us = fx (x rad + tx) + cx           vs = fy (y rad + ty) + cy
 * The pixel is covered iff 0 <= us <= W-1 and 0 <= vs <= H-1 (false for NaN).
 * Covered: U = (int)floorf(us 32 + 0.5f), ix = min(U >> 5, W-2),
 * a = U - 32 ix in 0..32 (1/32 px); likewise V, iy, b.
 * Map words (youth_rectify_map_device), two uint32 per output pixel:
 *   word 0: bits 0-5 a, bits 6-11 b, bit 31 covered;  word 1: iy W + ix;
 *   both 0 where the pixel is not covered.
 * Taps t00 = (ix, iy), t10 = (ix+1, iy), t01 = (ix, iy+1), t11 = (ix+1, iy+1)
 * with weights w00 = (32-a)(32-b), w10 = a(32-b), w01 = (32-a)b, w11 = ab
 * (sum 1024).
 * Colour (uint8, 1 or 3 interleaved channels), per channel:
 *   out = (sum w c + 512) >> 10; an uncovered pixel gives 0.
 * Depth (int16, valid iff > 0): an uncovered pixel gives 0.  Otherwise n is
 * the nearest tap, column ix + (a >= 16), row iy + (b >= 16).  n <= 0 is
 * copied (a hole never shrinks, no surface is invented across one).  Else the
 * gate is youth_filter.h's with its defaults,
 *   T = min(255, 8 + ((96 (n >> 4)^2) >> 16)),
 * a tap of value d joins iff d > 0 and |d - n| < T (the nearest always does,
 * and its weight is never 0), den = sum w, num = sum w (d - n + T),
 *   out = n - T + (num + (den >> 1)) / den           (unsigned 32-bit)
 * so a depth edge is never averaged across and out > 0 iff n > 0.
 * With D = 0 and Ko = K the output equals the input bit for bit.
 *
 * Plain C99, no HIP or torch types (streams travel as void*).  Entry points
 * return YOUTH_OK (0) or a negative YOUTH_E* code (youth_icp.h); the text of
 * the calling thread's last error is youth_rectify_last_error().  A rectifier
 * is used from one thread at a time.
 */
#ifndef YOUTH_RECTIFY_H
#define YOUTH_RECTIFY_H

#include <stddef.h>
#include <stdint.h>

#include "youth_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef YOUTH_DISTORTION_DEFINED
#define YOUTH_DISTORTION_DEFINED
/* OpenCV order and meaning. */
typedef struct youth_distortion {
    float k1, k2, p1, p2, k3;
} youth_distortion;
#endif

typedef struct youth_rectify youth_rectify;

/* Camera.k1, Camera.k2, Camera.p1, Camera.p2, Camera.k3 of an ORB-SLAM3-style
 * YAML (the file youth_parse_camera_yaml reads); a missing key is 0.
 * 1 = read, 0 = unreadable file or NULL argument (*D untouched). */
int youth_parse_camera_yaml_distortion(const char* path, youth_distortion* D);

/* A rectifier for W x H frames (2 <= W, H <= 16384, W*H <= 2^26) on HIP device
 * `device`.  YOUTH_EINVAL (with a text) for NULL K, D or out, a bad size, a
 * non-finite coefficient or camera value, a focal length <= 0, or a Ko whose
 * depth scale differs from K's; YOUTH_ENODEV without a device.  Argument
 * errors are reported before the device is looked at. */
int youth_rectify_create(int device, int W, int H, const youth_intrinsics* K,
                         const youth_distortion* D, const youth_intrinsics* Ko,
                         youth_rectify** out);
void youth_rectify_destroy(youth_rectify* r);

/* The number of covered output pixels (0 for NULL). */
long long youth_rectify_covered(const youth_rectify* r);

/* The map as data: d_map uint32 [H][W][2] on the rectifier's device.
 * Asynchronous on `stream` (NULL: the default stream). */
int youth_rectify_map_device(youth_rectify* r, uint32_t* d_map, void* stream);

/* Device-resident batch: depth int16 [n][H][W], colour uint8
 * [n][H][W][channels], channels 1 or 3, n_frames <= 65535.  Either plane pair
 * may be NULL (depth only, colour only; `channels` is ignored without colour);
 * a pair with one NULL, both pairs NULL, or an output that overlaps an input
 * is YOUTH_EINVAL.  Asynchronous on `stream`.  Any base alignment and width
 * work; frames whose width is a multiple of 4, on a depth output aligned to 8
 * bytes and a colour output aligned to 4, take the kernel's vector stores. */
int youth_rectify_device(youth_rectify* r, const int16_t* d_depth_in, int16_t* d_depth_out,
                         const uint8_t* d_rgb_in, uint8_t* d_rgb_out, int channels, int n_frames,
                         void* stream);

/* Host frames: upload to device staging the rectifier owns, one launch,
 * download; synchronous.  An output may be its input. */
int youth_rectify_host(youth_rectify* r, const int16_t* depth_in, int16_t* depth_out,
                       const uint8_t* rgb_in, uint8_t* rgb_out, int channels, int n_frames);

/* n separate host frames (page-locked or pageable), rectified in place:
 * depth[i] int16 [H][W], rgb[i] uint8 [H][W][3] (rgb NULL: depth only).  One
 * upload per buffer, one launch, one download per buffer; synchronous. */
int youth_rectify_host_frames(youth_rectify* r, int16_t* const* depth, uint8_t* const* rgb, int n);

const char* youth_rectify_last_error(void);

/* The SLAM.h drop-in: 1 while the module rectifies the frames it tracks.
 * That needs YOUTH_SLAM_RECTIFY=1 at initSlamModule and a YAML whose
 * coefficients are not all zero; frames of the YAML's size are then rectified
 * in place (Ko = K) before they are tracked, so the tracker, the map and the
 * loop closer see ideal-pinhole frames.  Without the variable nothing is
 * created or launched, and a YAML with non-zero coefficients earns one stderr
 * line saying they are ignored. */
int youth_slam_rectify_active(void);

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_RECTIFY_H */
