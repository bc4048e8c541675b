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
//   3. stopSlamModule with a backlog, then a restart.
// Exit 0 when every check holds; the sanitizers abort (non-zero) on a report,
// LeakSanitizer on a colour or depth buffer that left the pools for good.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

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

int main()
{
    setenv("YOUTH_SLAM_RGBD", "1", 1);
    scenario_producers();
    scenario_stream_reset_resize();
    scenario_stop_with_backlog();
    printf("rgbd worker: all scenarios passed\n");
    return 0;
}
