// qpn_handle.h -- the library handle (shared by decode.hip and train_host.hip)
#pragma once
#include "qpn_common.h"
#include "decode_plan.h"

struct BiasDesc { int64_t auxb[2], convb[2], convPb[2]; int adaptive; int pad; };
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

struct qpn_handle {
    Geom g;
    int device;
    DecodeKnobs dk;
    // decode program
    std::vector<int> h_map;          // gather map of the packed tile buffer
    std::vector<Task> h_tasks;
    int n_slots;
    int aux_woff4, aux_tiles, logRa;
    DecodeParams dp;                 // template (pointers filled per call)
    FastParams fp;                   // tile map of the specialised kernel
    int* d_map; float* d_wpk; Task* d_tasks; float* d_qb; BiasDesc* d_bd; int* d_status; int* d_bias_src;
    std::vector<int> h_bias_src;
    const float* d_flat; bool have_weights;
    // per-call workspaces (grow only)
    float* d_pproj; size_t pproj_cap;
    float* d_ring; size_t ring_cap;
    int* d_known; size_t known_cap;
    UttDesc* d_utts; size_t utts_cap;
    hipEvent_t ev0, ev1; float last_ms;
    bool pending;
    // device facts queried at qpn_create (nothing assumes a 256-CU chip that is all ours)
    int n_cus;                       // hipDeviceAttributeMultiprocessorCount
    int pipe_rows;                   // five-role groups one pipelined launch can hold resident (5 workgroups each), a multiple of 8
    int pipe_nu;                     // utterances per group when the batch exceeds them (1..3)
    // pinned staging of the utterance descriptors (enqueue does not synchronise)
    UttDesc* h_utts_pinned; size_t h_utts_cap;
    // live output (qpn_decode_live / qpn_decode_poll): host-coherent pinned memory the running kernel writes and the host reads
    int live_every;                  // 0: not armed
    bool live_call;                  // the decode in flight was enqueued armed
    int32_t* h_live; int32_t* d_live; size_t live_cap;                 // mirror of d_out, [B][max_n] (host address / the device's address of it)
    long long* h_live_done; long long* d_live_done; size_t live_done_cap;   // [B] published counts
    int64_t live_stride;             // max_n of the call in flight
    int* h_cancel; int* d_cancel; size_t cancel_cap;   // the stop request of qpn_decode_cancel: one host-coherent word, zeroed at every armed enqueue, read by the kernels at their publish points
    float samp_top_p, samp_min_p;          // ... and top_p / min_p (qpn_decode_sampling_ex; 1.0f / 0.0f: off)
    float samp_inv_temp; int samp_top_k;   // sampling controls of the decode calls enqueued from now on (qpn_decode_sampling): 1 / temperature, top-k cut (0: off; k == n_quantize is stored as 0)
    bool live_final;                 // the last decode was armed and has been finished: qpn_decode_final_counts reads its counts (until the next enqueue)
    std::vector<int64_t> live_seen;  // per-row high-water mark of what qpn_decode_poll has reported.  The counts restart only while qpn_decode_finish re-runs a launch that gave up,
                                     // and a handle is not thread-safe: only a caller that polls from a second thread under its own lock around finish could ever see the restart
    struct DecodeCall {              // arguments of the decode in flight: qpn_decode_finish re-runs it with the plan of decode_plan_retry when a
        int B, n_x; int64_t F, Td;   // multi-workgroup launch gave up (peers not co-resident: masked / shared GPU)
        const int64_t* d_x; const float* d_h; const void* d_dfac; int d_is_f32;
        std::vector<int64_t> n_samples; int maxd, mode; uint64_t seed;
        float inv_temp; int top_k;      // the handle's sampling controls at the enqueue: a re-run draws with the same ones
        float top_p, min_p;
        const int64_t* d_teacher; int64_t* d_out; float* d_logits;
        DecodePlanIn in; DecodePlan plan;   // what was planned from, and what the launches followed
    } call;
    std::string plan;                // human-readable launch plan of the last decode (qpn_last_decode_plan)
    bool single_cu_ok;               // the step state fits one CU's LDS (decode.hip kernels); otherwise decode_coop.hip only
    int w_past_il[QPN_MAX_LAYERS];   // channel-interleaved past-tap tiles (cooperative kernel)
    unsigned long long* d_xch; size_t xch_cap;   // exchange granules of the cooperative kernels
    // batched cooperative kernel (decode_coopb.hip): workgroup w's A-operand fragments are the cb_per_w float4 from cb_base4 + w * cb_per_w of the packed weights;
    // cb_zc.. = float4 offsets of the tiles inside that block; or cb_ok = false
    bool cb_ok; int cb_zc[QPN_MAX_LAYERS], cb_zp[QPN_MAX_LAYERS], cb_rs[QPN_MAX_LAYERS], cb_p1, cb_p2; long long cb_base4; int cb_per_w;
    bool decode_ok; std::string decode_err;   // geometries the decode kernels do not cover still train (and report why on decode calls)
    struct TrainState* train;        // lazily created by the training entry points (train_host.hip)
};
// the launchers of a plan's launches: rows [l.first, l.first + l.rows) of the descriptors behind p.utts, grouped as the plan says
int qpn_launch_decode_pipe(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream);
int qpn_launch_decode_coop(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, int G, hipStream_t stream);
int qpn_launch_decode_coopb(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream);
int grow_xch(qpn_handle* h, size_t words);      // the exchange buffer of those kernels holds >= words granules (grow only)
