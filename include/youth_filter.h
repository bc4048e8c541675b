/*
 * youth_filter.h — C-ABI of the edge-preserving depth filter on MI355X
 * (DESIGN.md §11).
 *
 * A KinectFusion-style tracker smooths the raw depth with an edge-preserving
 * filter before it takes normals: at the sensor noise SURVEY §8d defines
 * (sigma = 1.5 mm * Z^2) 1-px central-difference normals are unusable beyond
 * ~2 m (youth_synth.h).  The filter is opt-in: the tracker family of
 * youth_icp.h applies it to every frame it uploads once
 * youth_icp_set_depth_filter (or YOUTH_ICP_DEPTH_FILTER) turns it on; callers
 * of the device APIs filter their own buffers with youth_depth_filter_device.
 *
 * Definition, all integer.  Two parameters, 1 <= t0 <= 255 and
 * 0 <= t2 <= 1000 (defaults 8 and 96, meant for millimetre depth); a fixed
 * 5x5 window with spatial weights ws[] = {1, 2, 4, 2, 1} per axis.  For pixel
 * (u, v) with centre c = d[v][u]:
 *   c <= 0:  out = c (copied, negatives included).
 *   gate:    T = min(255, t0 + ((t2 * (c >> 4)^2) >> 16))      (unsigned 32-bit;
 *            for mm depth and the defaults T ~ 8 mm + 5.7 mm * Z^2)
 *   a tap (dx, dy) in [-2, 2]^2 contributes iff its pixel is inside the frame,
 *            n = d[v+dy][u+dx] > 0 and |delta| < T, delta = n - c;
 *   weight:  w = (T^2 - delta^2) * ws[dy+2] * ws[dx+2]  (the centre always contributes)
 *   sums:    den = sum w, num = sum w * (delta + T)      (both fit unsigned 32-bit)
 *   out = c - T + floor((num + (den >> 1)) / den)
 * out lies in [c - T + 1, c + T - 1] and out > 0 iff c > 0: the filter never
 * changes which pixels are valid.  The output does not depend on the launch
 * shape; with t0 = 1, t2 = 0 the filter is the identity.
 *
 * Plain C99, no HIP or torch types (streams travel as void*).  Entry points
 * return YOUTH_OK (0) or a negative YOUTH_E* code (youth_icp.h); the text of
 * the calling thread's last error is youth_depth_filter_last_error().
 */
#ifndef YOUTH_FILTER_H
#define YOUTH_FILTER_H

#include <stddef.h>
#include <stdint.h>

#include "youth_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef YOUTH_FILTER_PARAMS_DEFINED
#define YOUTH_FILTER_PARAMS_DEFINED
typedef struct youth_filter_params {
    int t0, t2;
} youth_filter_params;
#endif

/* t0 = 8, t2 = 96. */
youth_filter_params youth_depth_filter_default_params(void);

/* Device-resident batch: d_in, d_out int16 [n_frames][H][W] on HIP device
 * `device`, n_frames <= 65535, W and H within youth_icp_create's limits
 * (3 <= W, H <= 16384, W*H <= 2^26).  d_out must not overlap d_in.  P == NULL:
 * the defaults.  Asynchronous on `stream` (NULL: the default stream).
 * Frames whose width is a multiple of 4 and whose buffers are 8-byte aligned
 * take the kernel's vector path; any other width or base works too.
 * YOUTH_EINVAL (with a text) for bad sizes, parameters out of range, NULL or
 * overlapping buffers; YOUTH_ENODEV without a device.  Argument errors are
 * reported before the device is looked at. */
int youth_depth_filter_device(int device, const int16_t* d_in, int16_t* d_out, int n_frames, int W,
                              int H, const youth_filter_params* P, void* stream);

/* Host frames: upload, filter, download; synchronous.  `out` may be `in`. */
int youth_depth_filter_host(int device, const int16_t* in, int16_t* out, int n_frames, int W, int H,
                            const youth_filter_params* P);

const char* youth_depth_filter_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* YOUTH_FILTER_H */
