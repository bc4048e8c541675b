// hip_host.h — host support shared by every unit of libyouth_icp.so (not
// installed): the error text behind the youth_*_last_error functions, the HIP
// check macro, the frame limits, the device check and the growing device
// buffer.  Header-only and hidden: nothing here is exported or needs linking.
#ifndef YOUTH_HIP_HOST_H
#define YOUTH_HIP_HOST_H

#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include <string>

#include "youth_icp.h"

namespace youth __attribute__((visibility("hidden"))) {

// The last error of one module: its text and its code.  The library keeps four
// channels, one thread_local instance each, because which function reports
// which module's text is public (youth_icp.h, youth_viewer.h, youth_map.h,
// youth_filter.h): ICP with RGB-D (icp_host.h), the viewer cloud, the map with
// its render (map_table.h), the depth filter.
class ErrorText {
public:
    // Sets the text (at most 511 bytes) and the code; returns code.
    __attribute__((format(printf, 3, 4))) int set(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        text_ = buf;
        code_ = code;
        return code;
    }
    const char* c_str() const { return text_.c_str(); }
    int code() const { return code_; }

private:
    std::string text_;
    int code_ = YOUTH_OK;
};

inline int hip_failed(ErrorText& err, hipError_t e, const char* file, int line)
{
    return err.set(YOUTH_EHIP, "%s (line %d of %s)", hipGetErrorString(e), line, file);
}

// Frame limits of every entry point.  W, H <= 16384 and W*H <= 2^26: pixel
// indices fit the kernels' 24-bit multiplies and a frame's 16 B/px records
// their 32-bit buffer offsets.  Frames (or views) of one call <= 65535: they
// travel on gridDim.y.
constexpr int kMaxSide = 16384;
constexpr long long kMaxPixels = 1LL << 26;
constexpr int kMaxFrames = 65535;

inline bool frame_size_ok(int W, int H, int min_side)
{
    return W >= min_side && H >= min_side && W <= kMaxSide && H <= kMaxSide &&
           (long long)W * H <= kMaxPixels;
}

// `device` names a visible HIP device, or the text says why not.  A failed
// count leaves its error in the runtime; it is cleared here so that the next
// hipGetLastError of this thread does not report it.
inline int check_device(ErrorText& err, const char* who, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return err.set(YOUTH_ENODEV, "%s: no HIP device visible", who);
    }
    if (device < 0 || device >= ndev)
        return err.set(YOUTH_EINVAL, "%s: device %d of %d", who, device, ndev);
    return YOUTH_OK;
}

// Grow the device buffer *buf to hold at least `want` units of `per` elements;
// *cap is its capacity in units.  A failure leaves it empty: the pointer is
// nulled and the capacity zeroed before the new allocation.  hipFree waits for
// the device, so no kernel still reads the old buffer.
template <typename T, typename N>
int grow_device_buffer(ErrorText& err, T** buf, N* cap, N want, size_t per = 1)
{
    if (want <= *cap) return YOUTH_OK;
    hipError_t e = *buf ? hipFree(*buf) : hipSuccess;
    *buf = nullptr;
    *cap = 0;
    if (e == hipSuccess) e = hipMalloc(buf, (size_t)want * per * sizeof(T));
    if (e != hipSuccess) return hip_failed(err, e, __FILE_NAME__, __LINE__);
    *cap = want;
    return YOUTH_OK;
}

}  // namespace youth

// The HIP check of every unit: a failed call sets the unit's channel and
// returns YOUTH_EHIP from the enclosing function.  A unit names its channel
// before its first use: #define HIP_ERR g_cloud_error.
#define HIP_TRY(expr)                                                             \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) return youth::hip_failed(HIP_ERR, e_, __FILE_NAME__, __LINE__); \
    } while (0)

#endif  // YOUTH_HIP_HOST_H
