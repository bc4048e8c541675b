// icp_host.h — the host side's internal interface (not installed; the public
// one is include/youth_icp.h): the context every youth_icp_* entry point works
// on, the error text they share, and the launch layer through which the host
// units reach the kernels.
//
//   icp_kernels.hip  the depth-only kernels and the launch layer declared here
//   icp_api.cpp      create / destroy, setters, device and stage-level entries
//   icp_batch.cpp    the host batch and multi-GPU batch API
//   icp_track.cpp    the pipelined tracker
//   rgbd_host.h      the RGB-D alignment's own interface, on this context:
//                    rgbd_align.hip, rgbd_api.cpp, rgbd_track.cpp
#ifndef YOUTH_ICP_HOST_H
#define YOUTH_ICP_HOST_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "hip_host.h"
#include "host_copy.h"
#include "icp_device.h"
#include "youth_icp.h"

// Cross-unit functions are hidden: libyouth_icp.so exports the C API only.
namespace youth_icp __attribute__((visibility("hidden"))) {

// The ICP channel (hip_host.h), one per thread: youth_icp_last_error and
// youth_rgbd_last_error read it.
extern thread_local youth::ErrorText g_icp_err;

}  // namespace youth_icp

// the channel HIP_TRY (hip_host.h) reports to in every unit on this header
#define HIP_ERR youth_icp::g_icp_err

struct EventPair {
    hipEvent_t a, b;
    int kind;
};

// frames in flight through youth_icp_track_submit (YOUTH_TRACK_MAX_IN_FLIGHT):
// two one at a time, or two micro-batches of two, so the next submission's
// host copy and H2D overlap the launch before it
constexpr int kTrackDepth = YOUTH_TRACK_MAX_IN_FLIGHT;

// K and F are of icp_device.h's unnamed-namespace types (the kernels take them
// by value under those names): every unit sees the same layout.
struct youth_icp_ctx {
    int device = 0;
    int W = 0, H = 0, N = 0;
    size_t P = 0;
    int max_frames = 0;
    Intr K{};
    FastK F{};
    bool fast = false;  // verified 2-op back-projection division
    bool centred_exact = true;  // aligned loop's centred columns exact (centred_exact)
    int spec = kSpecSurvey;  // spec a7/a8 arithmetic (youth_icp_set_spec, YOUTH_ICP_SPEC)
    youth_icp_params prm{};
    hipStream_t stream = nullptr;

    int16_t* d_depth = nullptr;  // [max_frames][N] staging for host-side APIs
    float4* d_rec = nullptr;     // [max_frames][P] target records {z, nx, ny, nz}
    float* d_xyz = nullptr;      // [max_frames][3][P] (lazy: stage-level API only)
    double* d_T64 = nullptr;     // [max_frames][16]
    float* d_T32 = nullptr;      // [max_frames][12]
    int32_t* d_status = nullptr; // [max_frames]
    double* d_Tinit = nullptr;   // [max_frames][16]
    double* d_stats = nullptr;   // [max_frames][stats_iters][2]
    int stats_iters = 0;
    double* d_partials = nullptr;
    size_t partials_cap = 0;  // doubles
    double* d_neq = nullptr;  // [max_frames][29]
    int32_t* d_assoc = nullptr;
    float* d_Tout = nullptr;  // [max_frames][16]
    unsigned* d_flag = nullptr;
    unsigned* d_arrivals = nullptr;  // [max_frames] fused-solve arrival counters
    unsigned* d_arr_it = nullptr;    // [max_frames][stats_iters] persistent arrival tickets
    unsigned* d_epoch = nullptr;     // [max_frames] persistent pose epochs
    unsigned* d_head = nullptr;      // queue words kQHead / kQError / kQSpins / kQWaited
    bool persistent = true;          // one k_icp launch per align (else per-iteration k_reduce)
    // Iteration 0 of a persistent align without T_init takes the identity form
    // (ident_accumulate): the intrinsics keep the identity lemma's bound
    // (ident_first_ok) and YOUTH_ICP_NO_IDENT_FIRST=1 is not set.  It runs
    // inside the prep pass (k_prep_ident) where that pass forms the pairs'
    // targets, unless YOUTH_ICP_IDENT_FIRST=icp keeps it in k_icp.
    bool ident_first = true;
    bool ident_prep = true;
    int prep_band = 0;               // rows per k_prep_ident unit (YOUTH_ICP_PREP_BAND; 0: by batch size)
    int last_first_form = 0;         // the last align's (youth_icp_get_first_iter)
    int reduce = YOUTH_REDUCE_EXACT; // spec a9 (youth_icp_set_reduce, YOUTH_ICP_REDUCE)
    youth_lanes lanes{};             // lane partition of the last align's iterations
    bool has_lanes = false;
    bool lanes_mixed = false;        // the last host batch call ran more than one partition
    int icp_blocks_per_cu[4 * kVariants] = {};  // occupancy of k_icp<variant, fast, aligned> [variant 4 + fast 2 + aligned]
    int n_cu = 0;
    // small batches: k_icp_coop (youth_icp_create reads the knobs)
    bool coop = true;                // YOUTH_ICP_NO_COOP=1 disables
    int coop_px = 0;                 // YOUTH_ICP_COOP_PX: force pixels per lane (0: plan)
    int coop_px_env = 0;             // coop_px outside the tracker's batch mode
    int coop_threads = 512;          // YOUTH_ICP_COOP_THREADS=256: one wave per SIMD
    int coop_max_pairs = kCoopMaxPairs;  // YOUTH_ICP_COOP_MAX_PAIRS (<= kCoopMaxPairs)
    int coop_launch = 0;             // YOUTH_ICP_COOP_LAUNCH: 0 serial (default), 1 runtime, 2 plain
    bool trk_copy_compute = false;   // YOUTH_ICP_TRACK_COPY=compute: tracker H2D on the launch stream
    bool trk_copy_sdma = false;      // YOUTH_ICP_TRACK_COPY=sdma: hipMemcpyAsync, not k_pull_frames
    int trk_pull_wg = 0;             // YOUTH_ICP_PULL_WG: k_pull_frames workgroups per frame (0: auto)
    int trk_pull_lds = 48 << 10;     // YOUTH_ICP_PULL_LDS: LDS bytes a k_pull_frames workgroup reserves
    int trk_pull_reserve = 32;       // YOUTH_ICP_PULL_RESERVE_CU: CUs a micro-batch plan leaves free
    // staging copies of host frames (track_submit_batch / track_host_sequence):
    // split over the submitting thread and trk_copy_helpers persistent threads
    // once a submission holds trk_copy_min bytes (host_copy.h); the pool starts
    // with the first such submission
    int trk_copy_helpers = 3;        // YOUTH_ICP_COPY_THREADS: helper threads (0: one thread copies)
    size_t trk_copy_min = 1u << 20;  // bytes per submission from which the copy is split
    std::unique_ptr<youth::HostCopyPool> copy_pool;
    bool coop_refuse = false;       // YOUTH_ICP_TEST_REFUSE_COOP=1 (test hook)
    // occupancy of k_icp_coop<variant, fast, threads> [threads 256?][variant 2 + fast] at npx (LDS)
    int coop_bpc[2][2 * kVariants][kCoopMaxPx + 1] = {};
    int coop_bpc_tall[2 * kVariants] = {};  // the 64 x 80 prep-tile kernel at 10 px per lane
    unsigned* d_coop = nullptr;      // 2 counter sets of kCoopSetWords
    int32_t* d_status_out = nullptr; // [max_frames] host batch API: status per pair of the call
    int coop_par = 0;                // set (and partial-row arena) used by the next coop call
    double* d_coop_part = nullptr;   // 2 arenas x kCoopBufs x coop_part_cap rows (EMPTY when idle)
    int coop_part_cap = 0;           // rows per buffer
    int coop_part_rows[2] = {0, 0};  // rows per buffer the last call on each arena used
    int coop_poll_delay = -1;        // YOUTH_ICP_COOP_POLL_DELAY (x 64 clocks); -1: G / 8
    int coop_stall_once = -1;        // YOUTH_ICP_TEST_COOP_STALL (test hook): chunk that stalls
    int coop_stall_left = 0;         // coop launches the hook still stalls
    int coop_stall_iter = 1;         // YOUTH_ICP_TEST_COOP_STALL_ITER: the iteration whose row is lost
    bool realign_stall = false;      // YOUTH_ICP_TEST_REALIGN_STALL=1 (test hook): realigns' coop launches stall
    int last_coop_G = 0, last_coop_px = 0;
    bool last_coop = false;          // the last align ran k_icp_coop

    int last_pairs = 0;
    int last_iters = 0;
    hipStream_t last_stream = nullptr;

    int track_ref = -1;  // ring slot (0/1) of the tracker's reference frame
    double* coop_res_host = nullptr;  // set around a tracker align: k_icp_coop writes its result there
    bool coop_tile_src = true;        // YOUTH_ICP_COOP_TILE_SRC=0: contiguous source chunks
    int trk_batch = 1;                // frames per submission in youth_icp_track_host_sequence
    long long trk_chained = 0;        // micro-batch launches so far (youth_icp_track_chained)
    long long trk_chained_frames = 0; // frames those launches aligned (youth_icp_track_chained_frames)
    long long trk_realigned[3] = {};  // youth_icp_track_realign: coop / persistent / still failed
    long long batch_realigned = 0;    // host batch API chunks realigned after a coop timeout
    // depth filter in front of the tracker (youth_icp_set_depth_filter,
    // YOUTH_ICP_DEPTH_FILTER): off = nothing allocated, nothing launched
    bool flt_on = false;
    youth_filter_params flt{8, 96};
    int16_t* d_raw = nullptr;        // [trk_raw_slots][N] raw frames of one launch, filtered into d_depth
    int queues = 0;                  // k_icp work queues (YOUTH_ICP_QUEUES=1..8; 0: by batch size)
    int issue_prio = 1;              // k_icp's projection phase at wave priority 1 (YOUTH_ICP_PRIO=0: off)
    int share = 1;                   // contexts launching k_icp concurrently (set_concurrency)
    int prep_xcd_map = 0;             // YOUTH_ICP_PREP_XCD_MAP=1: k_prep tiles contiguous per XCD (slower)
    // pipelined tracking (youth_icp_track_submit / _collect): up to
    // kTrackDepth frames in flight, each with a pinned staging buffer, pinned
    // results and events
    struct TrackSlot {
        int16_t* pinned = nullptr;     // host depth copy, H2D source
        double* res = nullptr;         // pinned: T64 [16], then the status word
        hipEvent_t h2d = nullptr;      // staging -> device depth done (xfer)
        hipEvent_t done = nullptr;     // align + result D2H done (stream)
        hipEvent_t done_nf = nullptr;  // the same without the system-scope fence (the
                                       // kernel stored the result to host memory itself)
        hipEvent_t ev = nullptr;       // the one of the two recorded for this submission
        int has_ref = 0;
    } trk[kTrackDepth];
    int trk_dslot_last[2 * YOUTH_TRACK_MAX_BATCH];  // trk[] entry of the last launch that read depth slot d (-1: none)
    int trk_prev_d0 = -1;                       // first depth slot of the last launch
    int trk_head = 0, trk_n = 0;       // oldest in-flight submission, count in flight
    int trk_cap = 2;                   // ring entries in use (grows to kTrackDepth on demand)

    // host-buffer batch API: H2D of chunk k+1 on xfer overlaps the align of chunk k
    hipStream_t xfer = nullptr;
    std::vector<hipEvent_t> xfer_ev;

    bool timing = false;
    bool timing_iter_only = false;  // set_timing(2): events around the iteration kernel only
    std::vector<EventPair> ev_live;
    std::vector<EventPair> ev_free;
    double t_ms[3] = {0, 0, 0};
    int t_n[3] = {0, 0, 0};
};

// Target frames to turn into records before (or, for the tracker, beside)
// the iterations: depth frames [depth, depth + n N) -> record frames
// [out0, out0 + n); wait: the iterations gather exactly these records.
struct PrepJob {
    const int16_t* depth;
    int n, out0;
    bool wait;
    // tracker micro-batch (k_icp_coop only; CoopState.chain): pair p preps
    // its source frame into record frame prep_slot[p] and gathers record
    // frame tgt_slot[p]; results to the pinned slots res[p]
    bool chain = false;
    int tgt_slot[kCoopMaxChain] = {}, prep_slot[kCoopMaxChain] = {};
    double* res[kCoopMaxChain] = {};
};

inline bool filter_params_ok(const youth_filter_params* p)
{
    return p->t0 >= 1 && p->t0 <= 255 && p->t2 >= 0 && p->t2 <= 1000;
}

namespace youth_icp __attribute__((visibility("hidden"))) {

// The kernels' template variant of a context: spec a7/a8 arithmetic in bit
// 0, the lane32 reduction of spec a9 in bit 1.
inline int variant(const youth_icp_ctx* c)
{
    return c->spec | (c->reduce == YOUTH_REDUCE_LANE32 ? kRedLane32 : 0);
}

// ------------------------------------------ icp_api.cpp: context helpers --
hipStream_t pick_stream(youth_icp_ctx* c, void* stream);
int bind_device(youth_icp_ctx* c);

// ------------------------------------- icp_kernels.hip: the launch layer --
// A pair map travels as its two frame offsets (PairMap{src0, tgt0}): a type of
// the kernels' unnamed namespace cannot cross units.

// youth_icp_create's part that names kernels: the occupancy tables of k_icp
// and k_icp_coop.  On failure *what names the step for the error text.
hipError_t fill_occupancy(youth_icp_ctx* c, const char** what);
// Decide the division path for the context's intrinsics (k_verify_fastdiv).
int verify_fastdiv(youth_icp_ctx* c);
// youth_icp_destroy's part: the device's coop ordering forgets c->stream.
void coop_forget_stream(youth_icp_ctx* c);

int ensure_stats(youth_icp_ctx* c, int iters);
int ensure_partials(youth_icp_ctx* c, size_t doubles);
int ev_harvest(youth_icp_ctx* c);
// chunks per pair and pixels per chunk of one iteration's launch
int reduce_geometry(const youth_icp_ctx* c, int n_pairs, int* chunk_out);
// N pixels in about nb chunks: the chunk rounded up to whole workgroup steps
// (kRedStep), the chunk count recomputed from it.
inline int round_chunks(int N, int nb, int* chunk_out)
{
    const int chunk = ((N + nb - 1) / nb + kRedStep - 1) / kRedStep * kRedStep;
    *chunk_out = chunk;
    return (N + chunk - 1) / chunk;
}
// Caller-given initial poses [n_pairs][16], checked finite (which keeps every
// projected coordinate finite: the kernels' integer in-range test relies on
// it, xform_project), on their way to d_Tinit; *dTi: d_Tinit, or null when
// T_init_host is (identity).
int upload_T_init(youth_icp_ctx* c, hipStream_t s, const double* T_init_host, int n_pairs,
                  const double** dTi);
// Whether n_pairs pairs run as one k_icp_coop grid, and its plan.
bool coop_plan(const youth_icp_ctx* c, int n_pairs, int* npx_out, int* G_out);

// Target records (and optionally XYZ planes) for n_frames depth frames at
// `depth`, into workspace frames [out0, out0 + n_frames).
int launch_prep(youth_icp_ctx* c, hipStream_t s, const int16_t* depth, int n_frames, int out0,
                bool want_xyz);
// fuse_it >= 0: fused solve of iteration fuse_it (k_reduce's last workgroup
// per pair updates the pose); fuse_it < 0: partials only (launch_solve follows).
int launch_reduce(youth_icp_ctx* c, hipStream_t s, const int16_t* dsrc, int src0, int tgt0,
                  int n_pairs, bool assoc, int* nblk_out, int fuse_it = -1);
// All ICP iterations of n_pairs pairs.  *exported is set when the kernel
// also wrote the fp32 4x4 poses to d_T_out (k_icp_coop); otherwise the
// caller runs export_poses.
int run_iterations(youth_icp_ctx* c, hipStream_t s, const int16_t* dsrc, int src0, int tgt0,
                   int n_pairs, const double* T_init_host, float* d_T_out = nullptr,
                   bool* exported = nullptr, const PrepJob* job = nullptr);
// k_finish: fp32 4x4 poses to d_T_out; timeout: the launch's timeout flag is
// folded into every pair's status.
int export_poses(youth_icp_ctx* c, hipStream_t s, int n_pairs, float* d_T_out,
                 bool timeout);
// k_init: poses from dTi (device, or null: identity), status 0, the queue
// words zeroed; persistent: k_icp's epochs and arrival tickets as well.
int launch_init(youth_icp_ctx* c, hipStream_t s, const double* dTi, int n_pairs, int iters,
                bool persistent);
// k_solve on pair 0's nblk partials: the sums to d_neq, no pose update.
int launch_solve_sums(youth_icp_ctx* c, hipStream_t s, int nblk);
// k_solve_neq: one solve and update from d_neq on d_T64 / d_T32 / d_status.
int launch_solve_neq(youth_icp_ctx* c, hipStream_t s);
// k_status_out: d_status[0 .. n) with the timeout flag folded in -> out.
hipError_t launch_status_out(youth_icp_ctx* c, hipStream_t s, int n, int32_t* out);
// k_pull_frames: m page-locked host frames of N values -> dst[0 .. m N).
int launch_pull_frames(youth_icp_ctx* c, hipStream_t s, const int16_t* const* src, int m,
                       int16_t* dst, int N, int wg);
// icp_track.cpp: whether [p, p + bytes) lies inside one buffer of
// youth_icp_host_alloc (page-locked: a kernel may read it in place).
bool host_alloc_covers_bytes(const void* p, size_t bytes);
// icp_track.cpp: a collect's wait for its frame: with poll, up to 2 ms of
// hipEventQuery first; then hipEventSynchronize.
hipError_t wait_event_polled(hipEvent_t ev, bool poll);
// The self-test kernels (0 projdiv, 1 projquot, 2 normalize) on the null
// stream; returns hipGetLastError().
hipError_t launch_selftest(int which, unsigned long long n, unsigned long long seed,
                           unsigned long long* d_bad);

}  // namespace youth_icp

#endif  // YOUTH_ICP_HOST_H
