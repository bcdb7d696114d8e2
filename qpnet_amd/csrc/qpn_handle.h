// qpn_handle.h -- the library handle (shared by decode.hip and train_host.hip)
#pragma once
#include "qpn_common.h"
#include "decode_plan.h"
#include "adam_groups.h"
#include "train_stats_plan.h"

struct TrainState;
void qpn_train_destroy(TrainState* t);

// decode launch-plan knobs, parsed once in qpn_create (all optional; tests / tools build a fresh handle per setting)
struct DecodeKnobs {
    bool generic;          // QPN_DECODE_GENERIC: the interpreter kernel k_decode instead of the straight-line k_decode_fast
    bool no_resl;          // QPN_DECODE_NO_RESL: no LDS-resident residual tiles in the one-CU kernel
    int coop;              // QPN_DECODE_COOP=<G>: cooperative decode with up to G workgroups per utterance (0: only where one CU cannot hold the state)
    int coopb;             // QPN_DECODE_COOPB: smallest batch that takes the utterance-batched cooperative kernel (decode_coopb.hip) where it applies (default 1: always; 0 = never -- the per-utterance kernel decode_coop.hip)
    int coopb_delay[3];    // QPN_COOPB_DELAY_G / _X / _T (dev): first poll of the gate / block-output / post-net gathers of that kernel, x 128 clocks after the exchange waves reach it (8 / 4 / 0)
    int pipe;              // QPN_DECODE_PIPE: 0 = one-CU kernels, 1 / unset = the five-role pipelined kernel where it applies
    bool stamps;           // QPN_STAMPS (dev, -DQPN_ENABLE_STAMPS builds)
    bool test_pipe_gives_up;   // -DQPN_TESTING builds only (QPN_TEST_PIPE_GIVES_UP=1)
};

struct qpn_handle {      // every member has an initialiser: qpn_create sets only what it computes, qpn_destroy may meet a handle at any stage of it
    Geom g = {};
    int device = -1;
    DecodeKnobs dk = {};
    // decode program (decode_program.h), decided in qpn_create; its lists are uploaded by the first qpn_set_weights, which then drops the host copies
    DecodeProgram prog;
    DecodeParams dp = {};            // template (pointers filled per call)
    int* d_map = nullptr; float* d_wpk = nullptr; Task* d_tasks = nullptr; float* d_qb = nullptr; BiasDesc* d_bd = nullptr; int* d_status = nullptr; int* d_bias_src = nullptr;
    const float* d_flat = nullptr; bool have_weights = false;
    // per-call workspaces (grow only)
    float* d_pproj = nullptr; size_t pproj_cap = 0;
    float* d_ring = nullptr; size_t ring_cap = 0;
    int* d_known = nullptr; size_t known_cap = 0;
    UttDesc* d_utts = nullptr; size_t utts_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr; float last_ms = 0;
    bool pending = false;
    // device facts queried at qpn_create (nothing assumes a 256-CU chip that is all ours)
    int n_cus = 0;                   // hipDeviceAttributeMultiprocessorCount
    int pipe_rows = 0;               // five-role groups one pipelined launch can hold resident (5 workgroups each), a multiple of 8
    int pipe_nu = 3;                 // utterances per group when the batch exceeds them (QPN_PIPE_NU: 2..3)
    // pinned staging of the utterance descriptors (enqueue does not synchronise)
    UttDesc* h_utts_pinned = nullptr; size_t h_utts_cap = 0;
    // live output (qpn_decode_live / qpn_decode_poll): host-coherent pinned memory the running kernel writes and the host reads
    int live_every = 0;              // 0: not armed
    bool live_call = false;          // the decode in flight was enqueued armed
    int32_t* h_live = nullptr; int32_t* d_live = nullptr; size_t live_cap = 0;                     // mirror of d_out, [B][max_n] (host address / the device's address of it)
    long long* h_live_done = nullptr; long long* d_live_done = nullptr; size_t live_done_cap = 0;   // [B] published counts
    int64_t live_stride = 0;         // max_n of the call in flight
    int* h_cancel = nullptr; int* d_cancel = nullptr; size_t cancel_cap = 0;   // the stop request of qpn_decode_cancel: one host-coherent word, zeroed at every armed enqueue, read by the kernels at their publish points
    float samp_top_p = 1.0f, samp_min_p = 0.0f;      // ... and top_p / min_p (qpn_decode_sampling_ex; 1.0f / 0.0f: off)
    float samp_inv_temp = 1.0f; int samp_top_k = 0;  // sampling controls of the decode calls enqueued from now on (qpn_decode_sampling): 1 / temperature, top-k cut (0: off; k == n_quantize is stored as 0)
    std::vector<RowDraw> samp_rows;  // per-row records of the QPN_MODE_SAMPLING calls enqueued from now on (qpn_decode_row_sampling), input order, checked and converted; empty: off
    RowDraw* h_rows_pinned = nullptr; size_t h_rows_cap = 0;      // pinned staging of the call's records (copied on the call's stream with the descriptors) ...
    RowDraw* d_rows = nullptr; size_t rows_cap = 0;               // ... and the device table the kernels index by UttDesc.row
    // draw track of the QPN_MODE_SAMPLING calls enqueued from now on (qpn_decode_frame_sampling): [track_rows][track_frames], input order, checked and converted; track_rows == 0: off.
    // The table lives in h_track_pinned, allocated and filled by the setter (never by the enqueue; a handle without a device keeps the shape only).  The setter is refused while a
    // decode is in flight, so the staging holds the table of the call in flight until qpn_decode_finish has run: the re-run after a give-up copies it again
    int track_rows = 0; int64_t track_frames = 0;
    FrameDraw* h_track_pinned = nullptr; size_t h_track_cap = 0;
    FrameDraw* d_track = nullptr; size_t track_cap = 0;           // ... and the device table the kernels index by (UttDesc.row, frame)
    bool live_final = false;         // the last decode was armed and has been finished: qpn_decode_final_counts reads its counts (until the next enqueue)
    std::vector<int64_t> live_seen;  // per-row high-water mark of what qpn_decode_poll has reported.  The counts restart only while qpn_decode_finish re-runs a launch that gave up,
                                     // and a handle is not thread-safe: only a caller that polls from a second thread under its own lock around finish could ever see the restart
    struct DecodeCall {              // arguments of the decode in flight: qpn_decode_finish re-runs it with the plan of decode_plan_retry when a
        int B = 0, n_x = 0; int64_t F = 0, Td = 0;   // multi-workgroup launch gave up (peers not co-resident: masked / shared GPU)
        const int64_t* d_x = nullptr; const float* d_h = nullptr; const void* d_dfac = nullptr; int d_is_f32 = 0;
        std::vector<int64_t> n_samples; int maxd = 0, mode = 0; uint64_t seed = 0;
        float inv_temp = 1.0f; int top_k = 0;      // the handle's sampling controls at the enqueue: a re-run draws with the same ones
        float top_p = 1.0f, min_p = 0.0f;
        std::vector<RowDraw> rows;                 // ... and the per-row records in force at the enqueue (empty: none): the re-run draws with the same ones
        bool track = false;                        // ... and whether the handle's draw track was in force (it cannot change before qpn_decode_finish: see h_track_pinned)
        const int64_t* d_teacher = nullptr; int64_t* d_out = nullptr; float* d_logits = nullptr;
        DecodePlanIn in = {}; DecodePlan plan = {};   // what was planned from, and what the launches followed
    } call;
    std::string plan;                // human-readable launch plan of the last decode (qpn_last_decode_plan)
    unsigned long long* d_xch = nullptr; size_t xch_cap = 0;   // exchange granules of the cooperative kernels
    struct TrainState* train = nullptr;        // lazily created by the training entry points (train_host.hip)
    float* in_grad = nullptr; int64_t in_grad_n = 0;      // qpn_train_input_grad: where the next backward writes dL/dh (one shot; on the handle: armed before any training state exists)
    const float* distill_t = nullptr; int64_t distill_n = 0; float distill_alpha = 0.f, distill_temp = 1.f;      // qpn_train_distill: the teacher logits of the next forward-with-loss (one shot; on the handle for the same reason)
    qpn_loss_opts loss_opts = {}; bool loss_opts_armed = false;      // qpn_train_loss_opts: the loss options of the next forward-with-loss (one shot; on the handle for the same reason)
    // parameter groups of the Adam launches (qpn_adam_groups, train_host.hip): on the handle, not in the training state -- qpn_adam_step works on a handle that never trained
    int adam_n_groups = 0;                     // 0: off (the table below may stay: the same table set again costs no upload)
    float adam_lr[QPN_ADAM_MAX_GROUPS] = {}, adam_wd[QPN_ADAM_MAX_GROUPS] = {};
    AdamGroupTable adam_table;                 // the normalised table the device holds (adam_groups.h)
    char* d_adam_table = nullptr;              // [seg_end int64 | block pairs 2 x int32 | seg_group int32]
    // per-tensor statistics (qpn_tensor_stats, train_stats.hip): the plan of the caller's tensor table and its device copy, for the same reason on the handle
    StatsPlan stats_plan;                      // train_stats_plan.h
    char* d_stats = nullptr;                   // [items | partial records, one per item | records, one per tensor | first_item int32]
};
// what the launch plan needs to know of the kernels' own limits (decode_pipe.hip, decode_coopb.hip)
bool qpn_pipe_supported(const Geom& g);
bool qpn_coopb_supported(const Geom& g);
int qpn_pipe_rows_resident(int n_cus);
// the launchers of a plan's launches: rows [l.first, l.first + l.rows) of the descriptors behind p.utts, grouped as the plan says
int qpn_launch_decode_pipe(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream);
int qpn_launch_decode_coop(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, int G, hipStream_t stream);
int qpn_launch_decode_coopb(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream);
int grow_xch(qpn_handle* h, size_t words);      // the exchange buffer of those kernels holds >= words granules (grow only)
