// rgbd_driver.cpp — sanitizer driver for the SLAM module's RGB-D worker
// (slam_api.cpp, YOUTH_SLAM_RGBD=1; built by tests/tsan_rgbd/Makefile with
// -fsanitize=thread and with -fsanitize=address,undefined, linked with
// tests/tsan/icp_stub.c and rgbd_stub.cpp).  The product's real entry points,
// from several threads at once:
//   1. several producers pushing depth + colour while readers poll the
//      trajectory, the map points and the status;
//   2. one producer whose composed pose is checked against the frames' bytes,
//      colour included; a push without colour; resets and a size change in
//      mid-stream;
//   3. stopSlamModule with a backlog, then a restart;
//   4. a submission the tracker refuses (the stub's YOUTH_STUB_RGBD_REFUSE_AT):
//      none of its frames is recorded, the stream goes on;
//   5. a change to a larger frame size with a backlog of the old size, seen
//      through a map hook table of the driver's own: every frame of both sizes
//      is handed on with its colour, and no page-locked buffer of the old size
//      outlives the change.
// Exit 0 when every check holds; the sanitizers abort (non-zero) on a report,
// LeakSanitizer on a colour or depth buffer that left the pools for good.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "slam_map_hooks.h"
#include "youth_icp.h"

static void check(bool ok, const char* what)
{
    if (!ok) {
        fprintf(stderr, "FAIL: %s\n", what);
        exit(1);
    }
}

struct Frame {
    std::vector<int16_t> d;
    std::vector<uint8_t> c;
    long long sum() const
    {
        long long s = 0;
        for (int16_t v : d) s += v;
        for (uint8_t v : c) s += v;
        return s;
    }
};

static Frame frame(int w, int h, int value)
{
    Frame f;
    f.d.assign((size_t)w * h, (int16_t)(1000 + value));
    f.c.assign((size_t)w * h * 3, (uint8_t)(value * 7));
    f.c[0] = (uint8_t)value;
    return f;
}

// a producer that must not lose frames waits while the queue is long
static void push(const Frame& f, int w, int h, uint32_t ts)
{
    while (youth_slam_queue_size() >= 6) std::this_thread::sleep_for(std::chrono::microseconds(100));
    check(processSlamFrame(f.d.data(), f.c.data(), w, h, ts) == 1, "processSlamFrame accepted");
}

static const int W = 32, H = 24;

static void scenario_producers()
{
    initSlamModule(nullptr, nullptr);
    check(isSlamModuleRunning() == 1 && youth_slam_rgbd_active() == 1, "module runs in RGB-D mode");
    std::atomic<bool> done{false};
    std::vector<std::thread> prod;
    for (int t = 0; t < 4; ++t)
        prod.emplace_back([t] {
            for (int k = 0; k < 40; ++k) push(frame(W, H, 10 * t + k), W, H, (uint32_t)(t * 1000 + k));
        });
    std::thread reader([&] {
        while (!done.load()) {
            (void)getSlamMapPoints();
            const int len = youth_slam_trajectory_length();
            std::vector<uint32_t> ts(len > 0 ? len : 1);
            std::vector<double> T((size_t)(len > 0 ? len : 1) * 16);
            std::vector<int32_t> st(len > 0 ? len : 1);
            (void)youth_slam_get_trajectory(len, ts.data(), T.data());
            (void)youth_slam_get_status(len, st.data(), nullptr, nullptr);
            (void)youth_slam_rgbd_active();
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    });
    for (auto& p : prod) p.join();
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    done.store(true);
    reader.join();
    check(youth_slam_trajectory_length() == 160, "every frame of four producers recorded");
    if (const char* b = getenv("YOUTH_SLAM_TRACK_BATCH"))
        if (atoi(b) > 1) check(youth_slam_batched_frames() > 0, "backlogged frames travelled together");
    stopSlamModule();
}

static double last_x()
{
    const int len = youth_slam_trajectory_length();
    double T[16];
    check(youth_slam_get_pose(len - 1, nullptr, T) == 1, "last pose readable");
    return T[3];
}

static void scenario_stream_reset_resize()
{
    initSlamModule(nullptr, nullptr);
    check(youth_slam_rgbd_active() == 1, "RGB-D mode");
    std::vector<Frame> fr;
    for (int k = 0; k < 20; ++k) fr.push_back(frame(W, H, 3 * k + 1));
    for (int k = 0; k < 20; ++k) push(fr[k], W, H, (uint32_t)k);
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    check(youth_slam_trajectory_length() == 20, "20 frames recorded");
    // the composed pose telescopes over the frames' bytes, colour included
    check(fabs(last_x() - (double)(fr[19].sum() - fr[0].sum()) * 1e-6) < 1e-9, "pose follows depth and colour");
    // without colour a frame is refused and nothing changes
    check(processSlamFrame(fr[0].d.data(), nullptr, W, H, 500) == 0, "frame without colour refused");
    check(youth_slam_wait_idle(20000) == 1 && youth_slam_trajectory_length() == 20, "refusal left the trajectory");
    // a reset: the next frame is the new origin
    resetSlam();
    for (int k = 5; k < 15; ++k) push(fr[k], W, H, (uint32_t)(100 + k));
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    check(youth_slam_trajectory_length() == 10, "10 frames since the reset");
    check(fabs(last_x() - (double)(fr[14].sum() - fr[5].sum()) * 1e-6) < 1e-9, "pose restarted at the reset");
    // resets from another thread in mid-stream: no length is promised, only
    // that nothing races and the stream goes on
    std::thread resetter([] {
        for (int i = 0; i < 5; ++i) {
            std::this_thread::sleep_for(std::chrono::microseconds(700));
            resetSlam();
        }
    });
    for (int k = 0; k < 20; ++k) push(fr[k], W, H, (uint32_t)(200 + k));
    resetter.join();
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    check(youth_slam_trajectory_length() <= 20, "at most the pushed frames");
    // a size change with frames of the old size still queued: drain, new context
    const int w2 = 16, h2 = 12;
    std::vector<Frame> small;
    for (int k = 0; k < 7; ++k) small.push_back(frame(w2, h2, 5 * k + 2));
    resetSlam();
    for (int k = 0; k < 4; ++k) push(fr[k], W, H, (uint32_t)(300 + k));
    for (int k = 0; k < 7; ++k) push(small[k], w2, h2, (uint32_t)(400 + k));
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    check(youth_slam_trajectory_length() == 7, "the new size starts a new sequence");
    check(fabs(last_x() - (double)(small[6].sum() - small[0].sum()) * 1e-6) < 1e-9, "pose of the new size");
    stopSlamModule();
}

static void scenario_stop_with_backlog()
{
    initSlamModule(nullptr, nullptr);
    std::vector<Frame> fr;
    for (int k = 0; k < 10; ++k) fr.push_back(frame(W, H, k));
    for (int k = 0; k < 10; ++k)
        check(processSlamFrame(fr[k].d.data(), fr[k].c.data(), W, H, (uint32_t)k) == 1, "push");
    stopSlamModule();
    check(isSlamModuleRunning() == 0 && youth_slam_rgbd_active() == 0, "stopped");
    check(youth_slam_trajectory_length() <= 10, "at most the pushed frames");
    // producers racing the stop
    initSlamModule(nullptr, nullptr);
    std::thread p([&] {
        for (int k = 0; k < 200; ++k) (void)processSlamFrame(fr[k % 10].d.data(), fr[k % 10].c.data(), W, H, (uint32_t)k);
    });
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
    stopSlamModule();
    p.join();
    // and a restart works
    initSlamModule(nullptr, nullptr);
    for (int k = 0; k < 3; ++k) push(fr[k], W, H, (uint32_t)k);
    check(youth_slam_wait_idle(20000) == 1 && youth_slam_trajectory_length() == 3, "restart tracks");
    stopSlamModule();
}

// stubs only: frames of the submissions rgbd_stub.cpp refused; the smallest
// page-locked buffer icp_stub.c has alive (in int16 values) and their number
extern "C" long long youth_rgbd_stub_refused_frames(void);
extern "C" size_t youth_stub_host_min_values(int* count);

// A refused submission (the stub's YOUTH_STUB_RGBD_REFUSE_AT) is all or
// nothing: none of its frames is pending or recorded, its buffers go back, and
// the frames after it are tracked.
static void scenario_refused_submission()
{
    setenv("YOUTH_STUB_RGBD_REFUSE_AT", "3", 1);
    initSlamModule(nullptr, nullptr);
    check(youth_slam_rgbd_active() == 1, "RGB-D mode");
    const long long refused0 = youth_rgbd_stub_refused_frames();
    const int F = 30, burst = 5;
    std::vector<Frame> fr;
    for (int k = 0; k < F; ++k) fr.push_back(frame(W, H, 2 * k + 1));
    for (int k = 0; k < F; ++k) {
        if (k % burst == 0)
            while (youth_slam_queue_size() > 0) std::this_thread::yield();
        check(processSlamFrame(fr[k].d.data(), fr[k].c.data(), W, H, (uint32_t)(k + 1)) == 1, "push");
    }
    // wait_idle succeeds only with nothing in flight: no refused frame is pending
    check(youth_slam_wait_idle(20000) == 1, "worker idle after a refused submission");
    const long long refused = youth_rgbd_stub_refused_frames() - refused0;
    check(refused > 0, "a submission was refused");
    check(youth_slam_trajectory_length() == F - (int)refused, "every frame but the refused ones recorded");
    Frame tail = frame(W, H, 99);
    check(processSlamFrame(tail.d.data(), tail.c.data(), W, H, (uint32_t)(F + 1)) == 1, "push");
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    const int len = youth_slam_trajectory_length();
    check(len == F + 1 - (int)refused, "the frame after the refusal recorded");
    std::vector<uint32_t> ts(len);
    check(youth_slam_get_trajectory(len, ts.data(), nullptr) == len, "trajectory");
    for (int i = 1; i < len; ++i) check(ts[i] > ts[i - 1], "timestamps strictly increase");
    check(ts[len - 1] == (uint32_t)(F + 1), "the last frame pushed is the last recorded");
    // the refused frames are a gap of `refused` consecutive timestamps
    int gaps = 0;
    for (int i = 1; i < len; ++i)
        if (ts[i] != ts[i - 1] + 1) {
            ++gaps;
            check(ts[i] == ts[i - 1] + 1 + (uint32_t)refused, "the refused frames are one submission");
        }
    check(gaps == 1 && ts[0] == 1, "one gap in the recorded frames");
    // the pose telescopes over the recorded frames: none of the refused ones took part
    check(fabs(last_x() - (double)(tail.sum() - fr[ts[0] - 1].sum()) * 1e-6) < 1e-9, "pose skips the refused frames");
    stopSlamModule();
    unsetenv("YOUTH_STUB_RGBD_REFUSE_AT");
}

// What the map is handed: every recorded frame, by size, colour read in place.
static std::atomic<int> g_seen_big{0}, g_seen_small{0}, g_seen_bad{0};
static const int W2 = 48, H2 = 36;  // W2 H2 > 1.5 W H: above the old size's colour buffers too
static void map_integrate(const int16_t* depth, const uint8_t* rgb, int w, int h, const youth_intrinsics*,
                          const double*)
{
    if (!depth || !rgb) {
        g_seen_bad.fetch_add(1);
        return;
    }
    long long s = 0;
    for (int i = 0; i < w * h; ++i) s += depth[i];
    for (int i = 0; i < 3 * w * h; ++i) s += rgb[i];  // the sanitizer sees every byte
    if (s <= 0) g_seen_bad.fetch_add(1);
    (w == W2 && h == H2 ? g_seen_big : g_seen_small).fetch_add(1);
}
static void map_nop_start(int) {}
static void map_nop(void) {}
static int map_save(const char*) { return 1; }
static int map_render(const struct youth_map_view*, const youth_intrinsics*, const double*, int16_t*, uint8_t*)
{
    return 0;
}
static const youth_slam_map_hooks g_map_stub = {map_nop_start, map_nop, map_integrate, map_nop, map_save, map_render};

// Colour buffers across a size change with a backlog: the module is set up for
// W x H (so its pools hold buffers of exactly that size), frames of W x H are
// still queued and in flight when larger ones arrive.  Every frame of both
// sizes is recorded and handed on with its colour, and once the worker has
// settled on the new size no page-locked buffer of the old one is left.
static void scenario_resize_backlog()
{
    char path[64];
    snprintf(path, sizeof(path), "/tmp/youth_rgbd_cam_%d.yaml", (int)getpid());
    FILE* f = fopen(path, "w");
    check(f != nullptr, "camera file");
    fprintf(f, "Camera.fx: 30.0\nCamera.fy: 30.0\nCamera.cx: 16.0\nCamera.cy: 12.0\nCamera.width: %d\nCamera.height: %d\n", W, H);
    fclose(f);
    youth_slam_set_map_hooks(&g_map_stub);
    initSlamModule(path, nullptr);
    unlink(path);
    int count = 0;
    check(youth_stub_host_min_values(&count) == (size_t)W * H && count > 0, "pools set up for W x H");
    const int n1 = 5, n2 = 5;  // 10 queued at most: nothing is dropped
    std::vector<Frame> a, b;
    for (int k = 0; k < n1; ++k) a.push_back(frame(W, H, 4 * k + 1));
    for (int k = 0; k < n2; ++k) b.push_back(frame(W2, H2, 6 * k + 3));
    for (int k = 0; k < n1; ++k) check(processSlamFrame(a[k].d.data(), a[k].c.data(), W, H, (uint32_t)k) == 1, "push");
    for (int k = 0; k < n2; ++k)
        check(processSlamFrame(b[k].d.data(), b[k].c.data(), W2, H2, (uint32_t)(100 + k)) == 1, "push");
    check(youth_slam_wait_idle(20000) == 1, "worker idle");
    check(g_seen_small.load() == n1 && g_seen_big.load() == n2 && g_seen_bad.load() == 0,
          "every frame of both sizes recorded, colour with it");
    check(youth_slam_trajectory_length() == n2, "the new size is a new sequence");
    check(fabs(last_x() - (double)(b[n2 - 1].sum() - b[0].sum()) * 1e-6) < 1e-9, "pose of the new size");
    stopSlamModule();
    check(youth_stub_host_min_values(&count) >= (size_t)W2 * H2 && count > 0,
          "no page-locked buffer of the old size left behind");
    youth_slam_set_map_hooks(nullptr);
}

int main()
{
    setenv("YOUTH_SLAM_RGBD", "1", 1);
    scenario_resize_backlog();  // first: the pools hold no larger buffer of an earlier scenario yet
    scenario_producers();
    scenario_stream_reset_resize();
    scenario_stop_with_backlog();
    scenario_refused_submission();
    printf("rgbd worker: all scenarios passed\n");
    return 0;
}
