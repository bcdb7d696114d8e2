// train_report.h -- how a training step's reports come back without draining the stream: the bookkeeping, as a record and the decisions on it.
// No HIP: train_report.hip executes what these functions return (copies, event waits, the clear), tests/train_report_sweep.cpp runs them against a fake device.
//
// The reports of a step are the STICKY status word (kernels OR into it; it is cleared when it is read: every flag is reported exactly once), the loss (64 partial
// sums) and, behind a clipping Adam launch, the gradient norm that step clipped by.  Each travels to pinned host memory behind the step's kernels -- by a copy
// (qpn_train_status_enqueue / qpn_train_loss_enqueue) or written by the step's last kernel itself (the one-call step) -- into one of TWO slots, with an event behind it.
// Two slots, because the report of two steps ago is long done when its slot is reused: a loop that looks at every report EXCEPT the newest at the start of step i + 1
// never waits for step i (whose kernels the device still has queued while the host enqueues the next step), and learns of a bad chunk two steps late at most.
// Both writers share the one pair of slots.  A slot is never handed to a writer while its previous report is pending and unwaited.
#pragma once
#include "../../include/qpnet_hip.h"

// a pinned loss slot: the 64 partial sums, then the gradient norm of the same step
constexpr int LOSS_PARTS = 64, LOSS_NORM_AT = 64, LOSS_SLOT = 72;
inline double loss_sum(const double* parts) { double sum = 0.0; for (int i = 0; i < LOSS_PARTS; ++i) sum += parts[i]; return sum; }      // the loss of a step: its 64 partial sums, in order

// the status word as a return code and its message (a constant: nothing is formatted)
struct StatusRc { int rc; const char* msg; };
inline StatusRc status_to_rc(int st) {
    if (st & 1) return {QPN_ERANGE, "pitch-dependent tap outside the layer input (dilated factor > maxd or < 0; reference assert qpnet.py:294)"};
    if (st & 4) return {QPN_ENODEV, "the one-launch residual stack gave up waiting for a peer workgroup: the flagged step's results are invalid (its Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step); the handle runs a launch per layer from here on (QPN_STACK_QUEUE=0 selects that from the start)"};
    if (st & 2) return {QPN_ERANGE, "target class outside [0, n_quantize) (reference assert qpnet_train.py:525)"};
    if (st & 32) return {QPN_ERANGE, "a NaN or an infinity in the teacher logits of a distillation loss (qpn_distill_loss / qpn_train_distill): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"};
    if (st & 64) return {QPN_ERANGE, "a NaN, infinite or negative value among the sample weights of a loss with options (qpn_ce_loss_opts / qpn_distill_loss_opts / qpn_train_loss_opts; it counted as 0): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"};
    if (st & (1 << 16)) return {QPN_ERANGE, "non-finite gradient norm (an inf or NaN in the gradient): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"};
    if (st & 8) return {QPN_ERANGE, "a peer rank flagged its chunk of this data-parallel step, or an earlier micro-step of this accumulation window was flagged (a tap or target out of range, or an abandoned stack launch there): every rank skipped the update, the replicas are unchanged"};
    return {QPN_OK, ""};
}

// what happened on the handle: the norm word on the device is the latest Adam launch's, and only a launch that clipped wrote it
enum class StepEnd { AdamClipped, AdamPlain, NoAdam };      // NoAdam: a step or accumulate call that ended without an Adam launch (a micro-step in front of the closing one)

// a status slot has landed with word w: what its collector does, in this order
struct StatusLanded {
    StatusRc rc;           // what the collector returns
    bool clear;            // w != 0: clear the device word -- sticky until read, reported once.  ON the stream of the latest training call, i.e. behind every step
                           // enqueued so far (their Adam kernels all see the word set and skip) and in front of the next one: a null-stream memset is not ordered against
                           // a non-blocking stream and could land in the middle of a k_adam launch, whose blocks each read the word; and the stream of the call BEFORE
                           // the latest may be another one, busy with work of the caller's own -- a clear queued behind that lands after the next step has read the word
    bool mask_other;       // the other slot is pending and may have copied the same sticky bits before this clear: wait for it, take w's bits out of it, tell other_masked()
    int other;
};
struct LossNext { int slot; bool wait_drop; };                // wait_drop: an uncollected report of two calls ago sits there -- wait for it, it is dropped
struct LossCollect { int slot; bool valid; };                 // valid: a report is pending there (wait for it, then loss_landed)
struct SlotOrder { int n; int slot[2]; };

struct ReportLedger {      // every member has a default
    bool status_pending[2] = {}; int status_newest = 0;      // the deferred status check, two slots of one word
    bool loss_pending[2] = {}; int loss_newest = 0;          // the loss read one step late, two slots of LOSS_SLOT doubles
    bool gnorm_last = false;                                 // the latest Adam launch on this handle clipped (the device's norm word is that launch's)
    bool gnorm_slot[2] = {};                                 // loss slot i carries a norm
    double gnorm_collected = 0.0; bool gnorm_collected_valid = false;      // the norm that came with the loss the last loss_collect returned
    bool stack_disabled = false;                             // a stack-queue launch gave up once (status bit 4): this handle keeps to a launch per layer

    void step_ended(StepEnd e) { gnorm_last = e == StepEnd::AdamClipped; }
    bool norm_live() const { return gnorm_last; }            // qpn_train_grad_norm has a norm to read
    int loss_doubles() const { return gnorm_last ? LOSS_NORM_AT + 1 : LOSS_PARTS; }      // what a loss copy takes out: behind a clipping Adam launch the norm leaves with the partial sums

    // the next status report goes to the slot that is not the newest; the report that slot still holds (two reports old: long done) is collected FIRST
    int status_next() const { return status_newest ^ 1; }
    void status_sent(int slot) { status_pending[slot] = true; status_newest = slot; }
    // the next lagged loss likewise; the slot carries a norm when the step's Adam launch clipped
    LossNext loss_next() const { const int slot = loss_newest ^ 1; return {slot, loss_pending[slot]}; }
    void loss_sent(int slot) { loss_pending[slot] = true; loss_newest = slot; gnorm_slot[slot] = gnorm_last; }

    // which status slots a call looks at (a slot that is not pending is skipped), older first.  collect_lagged leaves the newest alone; poll looks at both, but a slot
    // whose event has not fired counts as pending and is left alone: poll does not wait for a report it looks at.  (Known exception, behaviour kept from before the
    // ledger: a landed report that is FLAGGED makes its collector wait for the other slot's event to mask it -- mask_other above --, in a poll too.  MEASUREMENTS.md)
    SlotOrder status_order(bool newest_too) const { return {newest_too ? 2 : 1, {status_newest ^ 1, status_newest}}; }
    StatusLanded status_landed(int slot, int w) {
        status_pending[slot] = false;
        if (w & 4) stack_disabled = true;
        return {status_to_rc(w), w != 0, w != 0 && status_pending[slot ^ 1], slot ^ 1};
    }
    void other_masked(int other, int left) { if (!left) status_pending[other] = false; }      // nothing left in it: it stops pending
    // the draining qpn_train_status has read word w off the device itself, behind everything: both slots stop pending.  (What they hold is at most w -- unless an
    // earlier report's clear took a bit out of the word that a still-pending slot holds: that flag is dropped here.  Known, behaviour kept from before the ledger;
    // the step that raised it was skipped on the device like every step behind a flagged one.  MEASUREMENTS.md)
    StatusLanded status_drained(int w) {
        status_pending[0] = status_pending[1] = false;
        if (w & 4) stack_disabled = true;
        return {status_to_rc(w), w != 0, false, 0};
    }

    // loss collect: newest = 0 the report sent one call EARLIER (complete by the time the host has enqueued another step), 1 the last one.  Whatever it finds,
    // the norm of the previous collect is forgotten: qpn_train_grad_norm_lagged answers for the loss THIS collect returned
    LossCollect loss_collect(int newest) {
        const int slot = newest ? loss_newest : loss_newest ^ 1;
        gnorm_collected_valid = false;
        return {slot, loss_pending[slot]};
    }
    void loss_landed(int slot, double norm) {      // norm: the slot's word LOSS_NORM_AT (looked at only where the slot carries one)
        loss_pending[slot] = false;
        if (gnorm_slot[slot]) { gnorm_collected = norm; gnorm_collected_valid = true; }
    }
};
