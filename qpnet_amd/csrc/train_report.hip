// train_report.hip -- the executor of train_report.h: the entry points that bring a step's status word, loss and gradient norm to the host, each as
// "ask the ledger, do what it says", and the two calls by which the one-call step (train_host.hip) sends the same reports from its last kernel
// (tests/train_report_sweep.cpp cannot include this file: its namespace `now` repeats these functions line for line over a fake device.  A change to the order of
//  the calls here -- call_on against the collect, the poll loop -- is made there too, or the CPU comparison with the old bookkeeping no longer covers what ships.)
#include "train_state.h"

int TrainReport::init() {
    QPN_HIP(hipHostMalloc((void**)&h_status, 64, hipHostMallocDefault));
    QPN_HIP(hipHostMalloc((void**)&h_loss, 2 * LOSS_SLOT * sizeof(double), hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) {
        QPN_HIP(hipEventCreateWithFlags(&ev_loss[i], hipEventDisableTiming));
        QPN_HIP(hipEventCreateWithFlags(&ev_status[i], hipEventDisableTiming));
    }
    return QPN_OK;
}
void TrainReport::destroy() {
    if (h_status) (void)hipHostFree(h_status);
    if (h_loss) (void)hipHostFree(h_loss);
    for (int i = 0; i < 2; ++i) if (ev_loss[i]) (void)hipEventDestroy(ev_loss[i]);
    for (int i = 0; i < 2; ++i) if (ev_status[i]) (void)hipEventDestroy(ev_status[i]);
}

static int report_rc(const StatusRc& r) { if (r.rc) qpn_set_error("%s", r.msg); return r.rc; }

// the report in a status slot, if one is pending there: waits for that slot's event only
static int status_collect_slot(TrainState* t, int slot) {
    TrainReport& r = t->report;
    if (!r.ledger.status_pending[slot]) return QPN_OK;
    QPN_HIP(hipEventSynchronize(r.ev_status[slot]));
    const int st = r.h_status[slot];
    const StatusLanded d = r.ledger.status_landed(slot, st);
    if (d.clear) QPN_HIP(hipMemsetAsync(t->d_status, 0, sizeof(int), r.last_stream));
    if (d.mask_other) {
        QPN_HIP(hipEventSynchronize(r.ev_status[d.other]));
        r.h_status[d.other] &= ~st;
        r.ledger.other_masked(d.other, r.h_status[d.other]);
    }
    return report_rc(d.rc);
}

int qpn_report_open(TrainState* t, bool lagged_loss, StepEnd end, hipStream_t stream, ReportSlots* s) {
    TrainReport& r = t->report;
    s->sslot = r.ledger.status_next();
    int rc = status_collect_slot(t, s->sslot); if (rc) return rc;
    const LossNext ln = r.ledger.loss_next();
    s->lslot = ln.slot;
    if (lagged_loss && ln.wait_drop) QPN_HIP(hipEventSynchronize(r.ev_loss[ln.slot]));
    r.call_on(stream, end);
    s->h_status = r.h_status + s->sslot;
    s->h_loss = lagged_loss ? r.h_loss + LOSS_SLOT * ln.slot : nullptr;
    s->h_norm = lagged_loss ? s->h_loss + LOSS_NORM_AT : nullptr;
    return QPN_OK;
}
int qpn_report_close(TrainState* t, const ReportSlots& s, hipStream_t stream) {
    TrainReport& r = t->report;
    QPN_HIP(hipEventRecord(r.ev_status[s.sslot], stream));
    r.ledger.status_sent(s.sslot);
    if (s.h_loss) {
        QPN_HIP(hipEventRecord(r.ev_loss[s.lslot], stream));
        r.ledger.loss_sent(s.lslot);
    }
    return QPN_OK;
}

extern "C" int qpn_train_loss(qpn_handle* h, double* h_loss, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train || !h_loss) { qpn_set_error("qpn_train_loss needs a preceding qpn_train_forward_loss / qpn_ce_loss"); return QPN_ESTATE; }
    hipStream_t stream = (hipStream_t)stream_;
    double parts[LOSS_PARTS];
    QPN_HIP(hipMemcpyAsync(parts, h->train->d_loss, sizeof(parts), hipMemcpyDeviceToHost, stream));
    QPN_HIP(hipStreamSynchronize(stream));
    *h_loss = loss_sum(parts);
    return QPN_OK;
}

// The loss without draining the stream every step: _enqueue copies this step's partial sums to a pinned slot behind the step's kernels; _collect(newest = 0)
// returns the sum enqueued one call EARLIER -- it does not wait in practice --, newest = 1 the last one (waits for it).  *h_valid = 0: no such copy.
extern "C" int qpn_train_loss_enqueue(qpn_handle* h, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train) { qpn_set_error("qpn_train_loss_enqueue needs a preceding qpn_train_forward_loss / qpn_ce_loss"); return QPN_ESTATE; }
    TrainState* t = h->train; TrainReport& r = t->report;
    const LossNext ln = r.ledger.loss_next();
    if (ln.wait_drop) QPN_HIP(hipEventSynchronize(r.ev_loss[ln.slot]));
    QPN_HIP(hipMemcpyAsync(r.h_loss + LOSS_SLOT * ln.slot, t->d_loss, r.ledger.loss_doubles() * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    QPN_HIP(hipEventRecord(r.ev_loss[ln.slot], (hipStream_t)stream_));
    r.ledger.loss_sent(ln.slot);
    return QPN_OK;
}
extern "C" int qpn_train_loss_collect(qpn_handle* h, int newest, double* h_loss, int* h_valid) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h_loss || !h_valid) { qpn_set_error("bad loss_collect arguments"); return QPN_EINVAL; }
    *h_valid = 0; *h_loss = 0.0;
    if (!h->train) return QPN_OK;
    TrainReport& r = h->train->report;
    const LossCollect c = r.ledger.loss_collect(newest);
    if (!c.valid) return QPN_OK;
    QPN_HIP(hipEventSynchronize(r.ev_loss[c.slot]));
    const double* slot = r.h_loss + LOSS_SLOT * c.slot;
    r.ledger.loss_landed(c.slot, slot[LOSS_NORM_AT]);
    *h_loss = loss_sum(slot); *h_valid = 1;
    return QPN_OK;
}

// The status word, draining the stream ...
extern "C" int qpn_train_status(qpn_handle* h, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train) { qpn_set_error("no training call yet"); return QPN_ESTATE; }
    TrainState* t = h->train;
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    int st = 0;
    QPN_HIP(hipMemcpy(&st, t->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) QPN_HIP(hipMemsetAsync(t->d_status, 0, sizeof(int), (hipStream_t)stream_));
    t->report.call_on((hipStream_t)stream_);
    return report_rc(t->report.ledger.status_drained(st).rc);
}
// ... and without draining it: _enqueue copies the word to a pinned slot behind the work enqueued so far and returns; _collect waits for the copies only and
// reports them; _collect_lagged leaves the newest alone
extern "C" int qpn_train_status_enqueue(qpn_handle* h, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train) { qpn_set_error("no training call yet"); return QPN_ESTATE; }
    TrainState* t = h->train; TrainReport& r = t->report;
    const int slot = r.ledger.status_next();
    r.call_on((hipStream_t)stream_);
    rc = status_collect_slot(t, slot); if (rc) return rc;
    QPN_HIP(hipMemcpyAsync(r.h_status + slot, t->d_status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    QPN_HIP(hipEventRecord(r.ev_status[slot], (hipStream_t)stream_));
    r.ledger.status_sent(slot);
    return QPN_OK;
}
static int status_collect(qpn_handle* h, bool newest_too) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train) return QPN_OK;
    const SlotOrder o = h->train->report.ledger.status_order(newest_too);
    for (int k = 0; k < o.n; ++k) { rc = status_collect_slot(h->train, o.slot[k]); if (rc) return rc; }
    return QPN_OK;
}
extern "C" int qpn_train_status_collect(qpn_handle* h) { return status_collect(h, true); }
extern "C" int qpn_train_status_collect_lagged(qpn_handle* h) { return status_collect(h, false); }
// ... and without waiting at all: only the checks whose reports have already landed are looked at (hipEventQuery); *pending = checks still in flight
// (a landed report that is flagged still waits for the OTHER slot's event to mask it, as status_collect_slot always does: train_report.h, status_order)
extern "C" int qpn_train_status_poll(qpn_handle* h, int* pending) {
    int rc = need_dev(h); if (rc) return rc;
    if (pending) *pending = 0;
    if (!h->train) return QPN_OK;
    TrainReport& r = h->train->report;
    const SlotOrder o = r.ledger.status_order(true);
    for (int k = 0; k < o.n; ++k) {
        const int slot = o.slot[k];
        if (!r.ledger.status_pending[slot]) continue;
        if (hipEventQuery(r.ev_status[slot]) != hipSuccess) { (void)hipGetLastError(); if (pending) ++*pending; continue; }
        rc = status_collect_slot(h->train, slot); if (rc) return rc;
    }
    return QPN_OK;
}

// Adam updates APPLIED on this handle so far (k_adam counts on the device: a launch that found the status word set -- its own rank's or, data-parallel, a peer's --
// applies nothing).  Drains `stream`.  A caller that counts steps on the host (the bias correction's step number) re-bases its count on this after a status error.
extern "C" int qpn_train_applied_updates(qpn_handle* h, int64_t* applied, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!applied) { qpn_set_error("bad applied_updates arguments"); return QPN_EINVAL; }
    *applied = 0;
    if (!h->train) return QPN_OK;
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    unsigned long long v = 0;
    QPN_HIP(hipMemcpy(&v, h->train->d_status + 2, sizeof(v), hipMemcpyDeviceToHost));
    *applied = (int64_t)v;
    return QPN_OK;
}

// The norm the latest Adam launch on this handle clipped by (drains `stream`); *h_valid = 0 when that launch did not clip, or there was none
extern "C" int qpn_train_grad_norm(qpn_handle* h, double* h_norm, int* h_valid, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h_norm || !h_valid) { qpn_set_error("bad grad_norm arguments"); return QPN_EINVAL; }
    *h_norm = 0.0; *h_valid = 0;
    if (!h->train || !h->train->report.ledger.norm_live()) return QPN_OK;
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    QPN_HIP(hipMemcpy(h_norm, h->train->d_loss + LOSS_NORM_AT, sizeof(double), hipMemcpyDeviceToHost));
    *h_valid = 1;
    return QPN_OK;
}
// ... and without a wait of its own: the norm of the step whose loss the last qpn_train_loss_collect returned (it left the device in that loss's slot)
extern "C" int qpn_train_grad_norm_lagged(qpn_handle* h, double* h_norm, int* h_valid) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h_norm || !h_valid) { qpn_set_error("bad grad_norm arguments"); return QPN_EINVAL; }
    *h_norm = 0.0; *h_valid = 0;
    if (!h->train || !h->train->report.ledger.gnorm_collected_valid) return QPN_OK;
    *h_norm = h->train->report.ledger.gnorm_collected; *h_valid = 1;
    return QPN_OK;
}
