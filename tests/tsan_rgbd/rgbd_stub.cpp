// rgbd_stub.cpp — TEST INFRASTRUCTURE ONLY: a CPU stand-in for the RGB-D
// tracker behind slam_api.cpp's hook table (slam_rgbd_hooks.h), registered from
// a static initialiser as slam_rgbd.cpp registers the real one, so the RGB-D
// worker runs under ThreadSanitizer / AddressSanitizer on a machine without a
// GPU.  Linked only into tests/tsan_rgbd's driver.  It computes no alignment:
// a frame's "relative pose" is a translation by the difference of the frames'
// byte sums (depth and colour), so the composed pose telescopes to
// (sum of the last frame - sum of the first) * 1e-6 and the driver can check
// that every frame, colour included, reached the trajectory in order.  Frames
// are read in place: a buffer changed between submit and collect aborts.
// YOUTH_STUB_RGBD_REFUSE_AT=k (read at create) makes the tracker refuse its
// k-th submission whole, as the real one does (all or nothing);
// youth_rgbd_stub_refused_frames counts the frames refused so.
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "slam_rgbd_hooks.h"

namespace {

struct Frame {
    const int16_t* d;
    const uint8_t* c;
    long long sum;
    int has_ref;
    double dx;
};

struct Stub {
    int W, H, batch;
    int has_ref;
    long long ref_sum;
    Frame f[2 * YOUTH_TRACK_MAX_BATCH];  // submitted, not collected (oldest first)
    int sub_m[2];                        // frames left of the submissions in flight
    int n, subs;
    int refuse_at, submits;  // YOUTH_STUB_RGBD_REFUSE_AT; submissions asked for so far
};

// frames of the submissions the stub refused (all trackers)
long long g_refused = 0;

long long frame_sum(const Stub* s, const int16_t* d, const uint8_t* c)
{
    long long v = 0;
    const int N = s->W * s->H;
    for (int i = 0; i < N; ++i) v += d[i];
    for (int i = 0; i < 3 * N; ++i) v += c[i];
    return v;
}

void stub_start(void) {}

void* stub_create(int device, int w, int h, int batch, const youth_intrinsics* K)
{
    (void)device, (void)K;
    Stub* s = static_cast<Stub*>(calloc(1, sizeof(Stub)));
    if (s) s->W = w, s->H = h, s->batch = batch;
    const char* e = getenv("YOUTH_STUB_RGBD_REFUSE_AT");
    if (s && e) s->refuse_at = atoi(e);
    return s;
}

void stub_destroy(void* t)
{
    if (t && static_cast<Stub*>(t)->n != 0) abort();  // the worker drains before it destroys
    free(t);
}

int stub_submit(void* t, const int16_t* const* depth, const uint8_t* const* rgb, int n)
{
    Stub* s = static_cast<Stub*>(t);
    if (!s || !depth || !rgb || n < 1 || n > s->batch || s->subs >= 2) return YOUTH_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!depth[i] || !rgb[i]) return YOUTH_EINVAL;
    if (s->refuse_at > 0 && ++s->submits == s->refuse_at) {  // all or nothing: no frame taken
        __atomic_fetch_add(&g_refused, (long long)n, __ATOMIC_SEQ_CST);
        return YOUTH_EINVAL;
    }
    for (int i = 0; i < n; ++i) {
        Frame& f = s->f[s->n++];
        f.d = depth[i];
        f.c = rgb[i];
        f.sum = frame_sum(s, f.d, f.c);
        f.has_ref = s->has_ref;
        f.dx = s->has_ref ? (double)(f.sum - s->ref_sum) * 1e-6 : 0.0;
        s->has_ref = 1;
        s->ref_sum = f.sum;
    }
    s->sub_m[s->subs++] = n;
    return 0;
}

int stub_collect(void* t, double* T_rel, int* has_ref)
{
    Stub* s = static_cast<Stub*>(t);
    if (!s || !T_rel || s->n == 0) return YOUTH_EINVAL;
    struct timespec ts = {0, 200 * 1000};  // an align takes a while
    nanosleep(&ts, nullptr);
    const Frame f = s->f[0];
    if (frame_sum(s, f.d, f.c) != f.sum) abort();  // reused while in flight
    memmove(s->f, s->f + 1, (size_t)(s->n - 1) * sizeof(Frame));
    --s->n;
    if (--s->sub_m[0] == 0) {
        s->sub_m[0] = s->sub_m[1];
        --s->subs;
    }
    memset(T_rel, 0, 16 * sizeof(double));
    T_rel[0] = T_rel[5] = T_rel[10] = T_rel[15] = 1.0;
    T_rel[3] = f.dx;
    if (has_ref) *has_ref = f.has_ref;
    return 0;
}

int stub_reset(void* t)
{
    Stub* s = static_cast<Stub*>(t);
    if (!s || s->n != 0) return YOUTH_EINVAL;
    s->has_ref = 0;
    return 0;
}

const char* stub_error(void) { return "rgbd stub"; }

const youth_slam_rgbd_hooks g_hooks = {stub_start,   stub_create, stub_destroy, stub_submit,
                                       stub_collect, stub_reset,  stub_error};

struct Registrar {
    Registrar() { youth_slam_set_rgbd_hooks(&g_hooks); }
} g_registrar;

}  // namespace

// stub only (declared in rgbd_driver.cpp): frames of refused submissions
extern "C" long long youth_rgbd_stub_refused_frames(void)
{
    return __atomic_load_n(&g_refused, __ATOMIC_SEQ_CST);
}
