// rgbd_host.h — the RGB-D host side's internal interface (not installed; the
// public one is include/youth_rgbd.h), on the ICP context and launch layer of
// icp_host.h: the context every youth_rgbd_* entry point works on, the structs
// the host fills for the kernels, the launch layer through which the host
// units reach them, and the few functions that cross the two host units.
//
//   rgbd_align.hip  the RGB-D kernels and the launch layer declared here
//   rgbd_api.cpp    create / destroy, pair and sequence align, the level
//                   schedule, device and stage-level entries
//   rgbd_track.cpp  the streaming tracker
#ifndef YOUTH_RGBD_HOST_H
#define YOUTH_RGBD_HOST_H

#include "icp_host.h"
#include "youth_filter.h"
#include "youth_rgbd.h"

// Cross-unit names are hidden: libyouth_icp.so exports the C API only.
namespace youth_rgbd __attribute__((visibility("hidden"))) {

constexpr int kRgbdNeq = YOUTH_RGBD_NEQ;
constexpr int kRgbdStride = 32;  // doubles per partial row (31 + a pad)

// The structs below are kernel arguments by value (k_rgbd_reduce,
// k_rgbd_decimate): every unit sees the same layout.

// host constants of §13: w = lambda / 255, kx = (0.5 w) fx, ky = (0.5 w) fy
struct PhotoK {
    float w, kx, ky;
};

// One k_rgbd_decimate launch: two frame sets (a pair call's sources and
// targets), every coarse level of a schedule.
struct DecimJob {
    const int16_t* depth[2];  // set k: [n[k]][H][W]
    const uint8_t* gray[2];
    int n[2];
    int n_lv;                              // levels to emit, strides decreasing
    int stride[YOUTH_RGBD_MAX_LEVELS];     // each of 2, 4, 8, 16
    int16_t* dout[2][YOUTH_RGBD_MAX_LEVELS];  // [set][level]: [n[set]][H_s][W_s]
    uint8_t* gout[2][YOUTH_RGBD_MAX_LEVELS];
};

}  // namespace youth_rgbd

struct youth_rgbd_ctx {
    youth_icp_ctx* icp = nullptr;  // records, poses, status, arrival counters, staging depth
    youth_rgbd_params prm{};
    youth_rgbd::PhotoK pk{};
    int frames = 0;                // frames the workspace holds: max_frames + 1
    int chunks = 0;                // YOUTH_RGBD_CHUNKS (0: planned)
    unsigned* d_photo = nullptr;   // [frames][N] packed words of the targets
    uint8_t* d_gray = nullptr;     // [frames][N] staging for the host entry points
    uint8_t* d_rgb = nullptr;      // [frames][N][3] (lazy: youth_rgbd_track_host_sequence)
    double* d_part = nullptr;      // [pair][chunk][kRgbdStride]
    size_t part_cap = 0;           // doubles
    double* d_stats = nullptr;     // [frames][stats_iters][4]
    int stats_iters = 0;
    double* d_neq = nullptr;       // [kRgbdNeq]
    int last_pairs = 0, last_iters = 0;
    hipStream_t last_stream = nullptr;

    // level schedule (youth_rgbd_set_levels).  A level's
    // workspace is a context of its own, W_s x H_s under K_s (this one for
    // stride 1); a coarse level's frames are decimated into depth / gray: the
    // call's sources (or its sequence) from element 0, its targets from
    // element off.
    struct Level {
        youth_rgbd_level lv{};
        youth_rgbd_ctx* ctx = nullptr;
        int16_t* depth = nullptr;
        uint8_t* gray = nullptr;
        size_t off = 0;  // elements, a multiple of 16
    };
    struct Schedule {
        int n = 0;
        Level at[YOUTH_RGBD_MAX_LEVELS];
    } sched;
    // the streaming tracker's own schedule (youth_rgbd_track_set_levels): the
    // same workspaces, without the decimated frames: a coarse level's banks
    // and slots are its context's own, at the parent's bank and slot indices
    Schedule trk_sched;
    // of the frame youth_rgbd_track_collect returned last
    int last_lv_n = 0;
    double last_lv_T[YOUTH_RGBD_MAX_LEVELS][16] = {};
    int32_t last_lv_st[YOUTH_RGBD_MAX_LEVELS] = {};

    // streaming tracker (youth_rgbd_track_*).  Depth and
    // intensity: two banks of trk_b frame slots, a submission's frames in the
    // bank the one before it did not use.  Records and words: slot 0 the
    // reference, slots 1 .. m the submission's frames (one bank: preps and
    // iterations of all submissions are ordered on the context's stream).
    int trk_b = 1;            // frames per submission at most; fixes the reduce geometry
    int trk_ref = -1;         // record / word slot of the reference (-1: none yet)
    int trk_bank = 0;         // bank of the next submission
    bool flt_on = false;
    youth_filter_params flt{8, 96};
    int16_t* d_raw = nullptr;  // [trk_raw_cap][N] unfiltered frames of one submission
    int trk_raw_cap = 0;
    int pull_wg = 0;           // YOUTH_RGBD_PULL_WG: k_rgbd_pull workgroups per frame (0: auto)
    hipEvent_t pull_ev = nullptr;  // youth_rgbd_pull_host: staging -> device done
    int16_t* pull_stage_d = nullptr;  // its pinned staging of pageable frames
    uint8_t* pull_stage_c = nullptr;
    int pull_stage_cap = 0;
    struct Sub {
        int m = 0, next = 0;      // frames of the submission, the next to collect
        int first_has_ref = 0;
        double* res = nullptr;    // pinned: [res_lv][res_cap][16] poses, then [res_lv][res_cap]
                                  // status words; without a schedule one level
        int res_cap = 0;          // frames `res` holds per level
        int res_lv = 0;           // levels `res` holds
        int n_lv = 0;             // levels of the submission (0: no schedule)
        int16_t* stage_d = nullptr;  // pinned staging of pageable frames [stage_cap][N]
        uint8_t* stage_c = nullptr;  //                                   [stage_cap][N][3]
        int stage_cap = 0;
        hipEvent_t h2d = nullptr, done = nullptr;
    } sub[2];
    int sub_head = 0, sub_n = 0;  // oldest submission in flight, submissions in flight
};

namespace youth_rgbd __attribute__((visibility("hidden"))) {

// -------------------------------------- rgbd_align.hip: the launch layer --
// A pair map travels as its two frame offsets, as in icp_host.h.

// k_rgbd_prep over n frames of `channels` channels; gray / photo nullable
int rgbd_launch_prep(hipStream_t s, const uint8_t* in, int channels, int n, int W, int H,
                     uint8_t* gray, unsigned* photo);
// One k_rgbd_reduce launch over n_pairs pairs: iteration `it` of `iters` with
// its fused solve, or (neq_out) the sums alone.
// geo_pairs: the pair count the chunks are planned for (0: n_pairs).
int rgbd_launch_reduce(youth_rgbd_ctx* r, hipStream_t s, const int16_t* dsrc, const uint8_t* gsrc,
                       int src0, int tgt0, int n_pairs, int it, int iters, double* neq_out,
                       int geo_pairs = 0);
// k_rgbd_decimate over the job's frames, W x H each
int rgbd_launch_decimate(hipStream_t s, const DecimJob& job, int W, int H);
// k_rgbd_pull: m page-locked host frames -> d_depth, d_gray and (nullable) d_rgb
int rgbd_launch_pull(youth_rgbd_ctx* r, hipStream_t s, const int16_t* const* depth,
                     const uint8_t* const* rgb, int m, int16_t* d_depth, uint8_t* d_gray,
                     uint8_t* d_rgb);

// ---------------------------------------------------------- rgbd_api.cpp --
int rgbd_ensure_stats(youth_rgbd_ctx* r, int iters);
// The rules of a schedule for context r (`who` speaks); full_last: the last
// level has stride 1 (the tracker's).
int rgbd_check_levels(const char* who, const youth_rgbd_ctx* r, const youth_rgbd_level* levels,
                      int n, bool full_last);
// A checked schedule's workspaces into `next` (emptied again on failure): per
// coarse level a context of W_s x H_s under K_s for r's max_frames and, with
// `frames`, room for the decimated frames of a call.
int rgbd_build_schedule(const char* who, youth_rgbd_ctx* r, const youth_rgbd_level* levels, int n,
                        bool frames, youth_rgbd_ctx::Schedule& next);
// A schedule of `owner` emptied: its child workspaces (which wait for their
// streams) and its frames released.
void rgbd_drop_schedule(youth_rgbd_ctx::Schedule& S, const youth_rgbd_ctx* owner);

// -------------------------------------------------------- rgbd_track.cpp --
// frames submitted to the streaming tracker and not collected yet
int rgbd_track_pending(const youth_rgbd_ctx* r);

}  // namespace youth_rgbd

#endif  // YOUTH_RGBD_HOST_H
