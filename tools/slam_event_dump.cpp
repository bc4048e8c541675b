// slam_event_dump.cpp — the SLAM worker's event sequence and trajectory for a
// fixed lock-step feed, as text: evidence that a change of slam_api.cpp's
// worker or buffer pools leaves both as they were (profiles/slam_worker/).
// Host only, linked like the sanitizer drivers with the CPU stand-ins:
//   gcc -std=gnu99 -O1 -Iinclude -c tests/tsan/icp_stub.c -o icp_stub.o
//   g++ -std=c++17 -O1 -Iinclude -Islam-rgbd_amd/csrc tools/slam_event_dump.cpp \
//       slam-rgbd_amd/csrc/slam_api.cpp tests/tsan_rgbd/rgbd_stub.cpp icp_stub.o \
//       -o slam_event_dump -lpthread
//   ./slam_event_dump depth > depth.txt ; ./slam_event_dump rgbd > rgbd.txt
// The feed pushes one frame and waits for the worker to go idle, so every
// event's place is fixed; it holds a resetSlam, a change to a larger frame size
// and one back, and in depth mode timed-out aligns (the stub's
// YOUTH_STUB_TIMEOUT_EVERY).  IDLE_BEGIN / IDLE_END are left out: the idle
// wait wakes every 20 ms, so their number depends on the machine's timing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <vector>

#include "youth_icp.h"

static void dump_trajectory(const char* when)
{
    const int len = youth_slam_trajectory_length();
    std::vector<uint32_t> ts(len + 1);
    std::vector<int32_t> st(len + 1);
    std::vector<double> T((size_t)(len + 1) * 16);
    youth_slam_get_trajectory(len, ts.data(), T.data());
    youth_slam_get_status(len, st.data(), nullptr, nullptr);
    printf("trajectory %s: %d poses, map points %d\n", when, len, getSlamMapPoints());
    for (int i = 0; i < len; ++i) {
        printf("  ts %u status %d T", ts[i], st[i]);
        for (int k = 0; k < 16; ++k) printf(" %a", T[(size_t)i * 16 + k]);
        printf("\n");
    }
}

static int g_ts = 0;

static void feed(int w, int h, int frames, bool color)
{
    for (int k = 0; k < frames; ++k, ++g_ts) {
        std::vector<int16_t> d((size_t)w * h, (int16_t)(900 + 11 * g_ts));
        std::vector<uint8_t> c((size_t)w * h * 3, (uint8_t)(5 * g_ts + 1));
        d[g_ts % d.size()] = 0;  // one invalid pixel
        if (processSlamFrame(d.data(), color ? c.data() : nullptr, w, h, (uint32_t)(1000 + g_ts)) != 1 ||
            youth_slam_wait_idle(20000) != 1) {
            fprintf(stderr, "feed failed at frame %d\n", g_ts);
            exit(1);
        }
    }
}

int main(int argc, char** argv)
{
    const bool rgbd = argc > 1 && strcmp(argv[1], "rgbd") == 0;
    if (rgbd)
        setenv("YOUTH_SLAM_RGBD", "1", 1);
    else
        setenv("YOUTH_STUB_TIMEOUT_EVERY", "4", 1);
    // the module set up for 32 x 24: its pools hold buffers of exactly that size
    char path[64];
    snprintf(path, sizeof(path), "/tmp/youth_event_dump_%d.yaml", (int)getpid());
    FILE* f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "Camera.fx: 30.0\nCamera.fy: 30.0\nCamera.cx: 16.0\nCamera.cy: 12.0\n"
               "Camera.width: 32\nCamera.height: 24\n");
    fclose(f);
    youth_slam_trace_enable(4096);
    initSlamModule(path, nullptr);
    unlink(path);
    if (youth_slam_rgbd_active() != (rgbd ? 1 : 0)) return 1;
    feed(32, 24, 6, rgbd);
    dump_trajectory("before the reset");
    resetSlam();
    feed(32, 24, 5, rgbd);
    dump_trajectory("before the larger size");
    feed(48, 36, 5, rgbd);
    dump_trajectory("before the smaller size");
    feed(32, 24, 4, rgbd);
    dump_trajectory("at the end");
    stopSlamModule();
    std::vector<double> t(4096);
    std::vector<int> kind(4096), arg(4096);
    const int n = youth_slam_trace_read(4096, t.data(), kind.data(), arg.data());
    // the producer's events and the worker's as two sequences: the worker's
    // timed wake-up may take a frame before the producer has traced PUSH_END
    int shown = 0;
    for (int who = 0; who < 2; ++who)
        for (int i = 0; i < n && i < 4096; ++i) {
            if (kind[i] == YOUTH_SLAM_EV_IDLE_BEGIN || kind[i] == YOUTH_SLAM_EV_IDLE_END) continue;
            const bool producer = kind[i] == YOUTH_SLAM_EV_PUSH_BEGIN || kind[i] == YOUTH_SLAM_EV_PUSH_END ||
                                  kind[i] == YOUTH_SLAM_EV_DROP;
            if (producer != (who == 0)) continue;
            printf("%s event %d %d\n", who == 0 ? "producer" : "worker", kind[i], arg[i]);
            ++shown;
        }
    printf("events %d (idle waits left out)\n", shown);
    long long persistent = 0, lost = 0;
    const long long re = youth_slam_realigned(&persistent, &lost);
    printf("batched %lld realigned %lld %lld %lld\n", youth_slam_batched_frames(), re, persistent, lost);
    youth_slam_trace_enable(0);
    return 0;
}
