// train_state.h -- the training state behind a handle: shared by train_host.hip (the step) and train_report.hip (how the step's reports come back)
#pragma once
#include "train_common.h"
#include "qpn_handle.h"
#include "train_report.h"
#include <string>

// The executor of train_report.h's ledger: the pinned slots, their events, and the stream a collected status word is cleared on (train_report.hip)
struct TrainReport {       // every member has a default
    ReportLedger ledger;
    hipStream_t last_stream = nullptr;        // the stream of the latest training call
    int* h_status = nullptr; hipEvent_t ev_status[2] = {};        // two slots of one word
    double* h_loss = nullptr; hipEvent_t ev_loss[2] = {};         // two slots of LOSS_SLOT doubles
    int init();
    void destroy();
    // every training call says where it runs, and what it ended in where that decides whose the device's norm word is
    void call_on(hipStream_t s) { last_stream = s; }
    void call_on(hipStream_t s, StepEnd e) { last_stream = s; ledger.step_ended(e); }
    bool stack_given_up() const { return ledger.stack_disabled; }
};
// The one-call step in loss modes 0 / 1: its last kernel (Adam, or the accumulate kernel of a micro-step in front of the closing one) writes the reports into the
// pinned slots itself -- what qpn_train_status_enqueue / qpn_train_loss_enqueue do with a copy each, without the two copy-engine launches behind the step.
// qpn_report_open in front of that launch: the slots, free for a writer (null: the step sends no such report); qpn_report_close behind it: the events, and the slots pending
struct ReportSlots { int* h_status; double* h_loss; double* h_norm; int sslot, lslot; };
struct TrainState;
int qpn_report_open(TrainState* t, bool lagged_loss, StepEnd end, hipStream_t stream, ReportSlots* s);
int qpn_report_close(TrainState* t, const ReportSlots& s, hipStream_t stream);

// Every member has a default: a state under construction is destroyable at any point (qpn_train_destroy frees what is there)
struct TrainState {
    TrainLayout lay;                          // what train_plan decided (train_plan.h): the path, hoist, block / bias / slab offsets (bw.sl points at lay.slabs), early_first
    int* d_wmap = nullptr; float* d_wp = nullptr; int* d_bstart = nullptr; int* d_blist = nullptr; float* d_bp = nullptr;
    int* d_gdst = nullptr; int* d_gdst_list = nullptr; int* d_gzero = nullptr;
    TrainParams tp = {};                      // template with block offsets filled in
    TrainBwd bw = {};
    TrainKnobs knobs = {};                    // launch-plan knobs, parsed once (qpn_train_knobs_parse)
    TrainShape shape; TrainFwdPlan fplan; TrainBwdPlan bplan;      // what the latest forward / backward launched (train_launch_plan.h)
    std::string plan_text;                    // qpn_train_last_plan: built when asked for
    AuxGeom ag = {};                          // aux hoist: per-layer offsets for k_aux_proj / k_aux_tail (s_out refreshed per forward)
    // workspaces (grow only)
    float* d_ws = nullptr; size_t ws_cap = 0; // one arena, carved per call (train_arena)
    int* d_tap = nullptr; size_t tap_cap = 0;
    double* d_loss3 = nullptr;                // qpn_distill_loss(h_loss3): 2 x 64 slots for the loss's two components, allocated by the first call that asks for them
    double* d_mass = nullptr;                 // loss options: 64 slots for the effective sum of weights + [64] the word k_weight_mass writes, allocated by the first call that needs them
    int* d_status = nullptr; double* d_loss = nullptr;   // d_status: 16 words -- [0] the sticky status word, [2..3] the count of Adam updates applied (k_adam); d_loss: one LOSS_SLOT
    TrainReport report;                       // how the status word, the loss and the norm come back (train_report.h, train_report.hip)
    // gradient-norm clipping (qpn_adam_step_clip): d_gnorm = TR_GN_BLOCKS partial sums of squares; the norm word a clipping k_adam leaves is d_loss[LOSS_NORM_AT] (one copy takes both out)
    double* d_gnorm = nullptr;
    bool fwd_valid = false;
    bool loss_clear = false;                  // the loss accumulator is zero (cleared by the forward's refresh kernel, consumed by one CE call)
    int* d_ctmap = nullptr; float* d_ct = nullptr;           // causal conv table [tap][class][C] and its gather map
    int* d_gmap = nullptr; float* d_gwp = nullptr;           // GEMM path (lay.use_gemm: n_resch > 128, or QPN_TRAIN_GEMM=1): the K-major weight blocks of train_gemm.hip and their map
    TrainGemm gm = {};
    int64_t generation = 0;                   // bumped by every qpn_train_forward: identifies whose activations the workspace holds
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr;   // side stream for the weight gradients that overlap the layer backward
    hipEvent_t ev_early = nullptr; int early_recorded = 0;   // qpn_train_early_bucket: the flat-gradient tail (from lay.early_first) that is final before the layer backward ends
    int64_t bwd_generation = -1;                             // generation of the forward the last backward belonged to
    const float* post_bwd_dlogits = nullptr;                 // ... on this dL/dlogits buffer
    unsigned* d_sq = nullptr; size_t sq_pos_cap = 0, sq_per_dir = 0;         // stack work queues (train_stack.hip): [16 control words | forward flags | backward flags]
    StackQ sqf = {}, sqb = {};
};

static inline int need_dev(qpn_handle* h) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (h->device < 0) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    return QPN_OK;
}
