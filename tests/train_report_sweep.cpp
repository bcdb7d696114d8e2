// Stand-alone sweep over the training reports' ledger (qpnet_amd/csrc/train_report.h): seeded random sequences of the calls that send and fetch a step's status word,
// loss and gradient norm run twice in lockstep on a small fake device -- once through the ledger, executed as train_report.hip executes it, once through a verbatim
// transcription of the bookkeeping the ledger replaced (the loose TrainState members, as train_host.hip updated them before the ledger existed).  After every operation
// both must agree on the return code and message, every output, every device action (waits, copies, the clear and its stream, event records, in order), the pinned
// status slots (i.e. the mask applied to the other slot) and all bookkeeping members.  On the ledger's run the invariants (a)-(f) of sequence() are asserted.
// Built with the host sanitizers and run as a child process (tests/test_train_report_cpu.py).
#include "../qpnet_amd/csrc/train_report.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

static long n_ops = 0; static unsigned g_seed = 0; static bool g_trace = false;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s (line %d) -- seed %u, operation %ld\n", #cond, __LINE__, g_seed, n_ops); exit(1); } } while (0)

// ---------------------------------------------------------------- the fake device
// One queue in enqueue order with a stream label per entry: the caller orders its two streams against each other, as a caller that moves a handle between streams
// must.  Entries land when the driver lets time pass (land) or when a wait forces them (everything up to the awaited entry).  The status word is sticky: faults OR
// into it.  A step's last kernel writes the reports of train_adam.hip: the status word, the 64 loss partials, the norm where it clipped.
typedef int hipStream_t; typedef int hipEvent_t; typedef int hipError_t;
enum { hipSuccess = 0, hipErrorNotReady = 600, hipMemcpyDeviceToHost = 2 };
struct Dev {
    enum Kind { COPY, SET, EVENT, KERNEL };
    struct Op { Kind k; int stream; void* dst; const void* src; size_t n; int ev; int raise; double id; bool clip; int* h_status; double* h_loss; double* h_norm; long serial, step; };
    int d_status[16] = {}; double d_loss[LOSS_SLOT] = {};
    int h_status[16] = {}; double h_loss[2 * LOSS_SLOT] = {};      // this run's pinned slots
    std::deque<Op> q; long serial = 0, landed = 0;                 // landed: serial of the last entry that has run
    long ev_serial[4] = {-1, -1, -1, -1};                          // the entry an event was last recorded as (-1: never)
    std::vector<long> log;                                         // every device action of the current operation
    // invariants
    int unreported = 0;                                            // (a) bits raised on the device and not yet returned by a call
    long raised_at[32] = {};                                       // (b) the step that first raised a bit still unreported
    int latest_call_stream = 0;                                    // (c) the stream of the latest training call, told by the driver
    long writer[4] = {-1, -1, -1, -1}; long known_done = 0;        // (e) the last entry that writes pinned slot i (status 0, 1; loss 2, 3); the host knows everything <= known_done has run
    long n_lost_to_drain = 0;                                      //     (a) ... except a flag the draining status call drops with the slot that alone still holds it (behaviour kept: MEASUREMENTS.md)
    bool in_poll = false; long n_poll_waits = 0;                   // (f)
    long last_on[2] = {}, moved_at[2] = {};                       // the last entry of a stream; what was enqueued when the handle moved to it
    long step_now = 0, launches = 0; int copy_raise = 0;           // copy_raise: the fault of a call-by-call step, raised right in front of the status copy that follows it

    int slot_of(const void* p) const {
        if (p >= (const void*)h_status && p < (const void*)(h_status + 2)) return (int)((const int*)p - h_status);
        if (p >= (const void*)h_loss && p < (const void*)(h_loss + 2 * LOSS_SLOT)) return 2 + (int)(((const double*)p - h_loss) / LOSS_SLOT);
        return -1;
    }
    void hand_to_writer(const void* p) {                           // (e): no pinned slot goes to a writer while its previous write is pending and unwaited
        const int s = slot_of(p); if (s < 0) return;
        CHECK(writer[s] <= known_done);
        writer[s] = serial + 1;
    }
    void push(Op o) { o.serial = ++serial; o.step = step_now; last_on[o.stream] = serial; q.push_back(o); }
    void raise(int bits, long step) {
        for (int b = 0; b < 32; ++b) if ((bits >> b & 1) && !(unreported >> b & 1)) raised_at[b] = step;
        d_status[0] |= bits; unreported |= bits;
    }
    void run_one() {
        const Op o = q.front(); q.pop_front(); landed = o.serial;
        switch (o.k) {
        case COPY: raise(o.raise, o.step); memcpy(o.dst, o.src, o.n); break;
        case SET: memset(o.dst, 0, o.n); break;
        case EVENT: break;
        case KERNEL:
            raise(o.raise, o.step);
            if (o.id >= 0.0) d_loss[0] = o.id;                     // (a stand-alone Adam launch, id < 0, leaves the loss alone: its norm goes with the loss the device holds)
            if (o.clip) d_loss[LOSS_NORM_AT] = d_loss[0] + 0.5;
            if (o.h_loss) memcpy(o.h_loss, d_loss, LOSS_PARTS * sizeof(double));
            if (o.clip && o.h_norm) *o.h_norm = d_loss[LOSS_NORM_AT];
            if (o.h_status) *o.h_status = d_status[0];
            break;
        }
    }
    void run_to(long s) { while (!q.empty() && q.front().serial <= s) run_one(); if (s > known_done) known_done = s; }
    void land(int n) { while (n-- > 0 && !q.empty()) run_one(); }
    // a call returned word w as its report: every bit of it was raised and not yet returned (a); -> the step that raised the oldest of them (b)
    long reported(int w) {
        CHECK((w & ~unreported) == 0);
        long oldest = step_now;
        for (int b = 0; b < 32; ++b) if (w >> b & 1) oldest = raised_at[b] < oldest ? raised_at[b] : oldest;
        unreported &= ~w;
        return oldest;
    }
};
static Dev* D = nullptr;      // the device of the run that is executing

static hipError_t hipEventSynchronize(hipEvent_t e) {
    if (D->in_poll && D->ev_serial[e] > D->landed) {               // (f) poll never waits for the event of a report it looks at ...
        CHECK(!D->log.empty() && D->log.back() / 100 == 7);        //     ... but it DOES wait for the other slot's, right behind a clear, to mask it: the known exception, counted (behaviour kept: MEASUREMENTS.md)
        ++D->n_poll_waits;
    }
    D->log.push_back(100 + e);
    if (D->ev_serial[e] >= 0) D->run_to(D->ev_serial[e]);
    return hipSuccess;
}
static hipError_t hipEventQuery(hipEvent_t e) {
    const bool done = D->ev_serial[e] <= D->landed;
    D->log.push_back(200 + e * 2 + done);
    if (done && D->ev_serial[e] > D->known_done) D->known_done = D->ev_serial[e];      // (in one queue: everything in front of it has run too)
    return done ? hipSuccess : hipErrorNotReady;
}
static hipError_t hipGetLastError() { return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    D->log.push_back(300 + e * 2 + s);
    Dev::Op o = {}; o.k = Dev::EVENT; o.stream = s; o.ev = e; D->push(o); D->ev_serial[e] = D->serial;
    return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
    CHECK(!D->in_poll);
    D->log.push_back(400 + s);
    D->run_to(D->last_on[s] > D->moved_at[s] ? D->last_on[s] : D->moved_at[s]);      // (the stream waits for what the other one held when the handle moved to it)
    return hipSuccess;
}
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, int, hipStream_t s) {
    D->log.push_back(500 + s); D->log.push_back((long)n); D->log.push_back(D->slot_of(dst));
    D->hand_to_writer(dst);
    Dev::Op o = {}; o.k = Dev::COPY; o.stream = s; o.dst = dst; o.src = src; o.n = n;
    if (src == (const void*)D->d_status) { o.raise = D->copy_raise; D->copy_raise = 0; }
    D->push(o);
    return hipSuccess;
}
static hipError_t hipMemcpy(void* dst, const void* src, size_t n, int) {      // (behind a hipStreamSynchronize in every use: reads what has landed)
    CHECK(!D->in_poll);
    D->log.push_back(600); D->log.push_back((long)n);
    // the draining status call reads the word itself and drops both slots: (a) cannot hold for a flag that by now only a pinned slot holds (an earlier report's clear took it out of the word)
    if (src == (const void*)D->d_status) { const int lost = D->unreported & ~D->d_status[0]; if (lost) { ++D->n_lost_to_drain; D->unreported &= ~lost; } }
    memcpy(dst, src, n);
    return hipSuccess;
}
static hipError_t hipMemsetAsync(void* dst, int, size_t n, hipStream_t s) {
    D->log.push_back(700 + s);
    CHECK(dst == (void*)D->d_status && n == sizeof(int));
    CHECK(s == D->latest_call_stream);                             // (c) a clear is only ever issued on the stream of the latest training call
    Dev::Op o = {}; o.k = Dev::SET; o.stream = s; o.dst = dst; o.n = n; D->push(o);
    return hipSuccess;
}
// the step's last launch (k_adam, or k_grad_accum in a micro-step in front of the closing one) with the report addresses it was handed
static void fake_launch(int raise, double id, bool clip, int* h_status, double* h_loss, double* h_norm, hipStream_t s) {
    D->log.push_back(800 + s); D->log.push_back(D->slot_of(h_status)); D->log.push_back(D->slot_of(h_loss)); D->log.push_back(D->slot_of(h_norm)); D->log.push_back(clip);
    if (h_status) D->hand_to_writer(h_status);
    if (h_loss) D->hand_to_writer(h_loss);
    if (h_norm) CHECK(h_loss && h_norm == h_loss + LOSS_NORM_AT);
    Dev::Op o = {}; o.k = Dev::KERNEL; o.stream = s; o.raise = raise; o.id = id; o.clip = clip; o.h_status = h_status; o.h_loss = h_loss; o.h_norm = h_norm; D->push(o);
    ++D->launches;
}

#define QPN_HIP(call) do { if ((call) != hipSuccess) { fprintf(stderr, "fake HIP call failed (line %d)\n", __LINE__); exit(1); } } while (0)
static const char* g_msg = "";      // qpn_last_error of the run that is executing
static void qpn_set_error(const char* m) { g_msg = m; }

// what one operation of the driver asks for, and what it gives back
struct Call { int loss_mode; bool clip, closing; int raise; double id; hipStream_t stream; };
struct Out {
    int rc = 0; const char* msg = ""; double loss = 0.0; int valid = 0; double norm = 0.0; int nvalid = 0; int pending = 0; int word = 0; bool reported = false;
    bool same(const Out& o) const { return rc == o.rc && !strcmp(msg, o.msg) && loss == o.loss && valid == o.valid && norm == o.norm && nvalid == o.nvalid && pending == o.pending && word == o.word && reported == o.reported; }
};
static Out* g_out = nullptr;        // ... of the run that is executing

// ---------------------------------------------------------------- the transcription: the bookkeeping as train_host.hip did it before the ledger
// (the functions' member updates and HIP calls as they stood; argument checks, need_dev and the `h->train` tests are left out, the kernels' launches are fake_launch)
namespace old {
struct TrainState {
    int* d_status = nullptr; double* d_loss = nullptr;
    hipStream_t last_stream = 0;
    int* h_status_pinned = nullptr; hipEvent_t ev_status[2] = {0, 1}; bool status_pending[2] = {}; int status_newest = 0;
    double* h_loss_pinned = nullptr; hipEvent_t ev_loss[2] = {2, 3}; bool loss_pending[2] = {}; int loss_newest = 0;
    bool gnorm_last = false;
    bool gnorm_slot[2] = {};
    double gnorm_collected = 0.0; bool gnorm_collected_valid = false;
    bool stack_disabled = false;
};
static int status_to_rc(int st) {
    g_out->word = st; g_out->reported = st != 0;      // (the driver's: which word the call reported)
    if (st & 1) { qpn_set_error("pitch-dependent tap outside the layer input (dilated factor > maxd or < 0; reference assert qpnet.py:294)"); return QPN_ERANGE; }
    if (st & 4) { qpn_set_error("the one-launch residual stack gave up waiting for a peer workgroup: the flagged step's results are invalid (its Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step); the handle runs a launch per layer from here on (QPN_STACK_QUEUE=0 selects that from the start)"); return QPN_ENODEV; }
    if (st & 2) { qpn_set_error("target class outside [0, n_quantize) (reference assert qpnet_train.py:525)"); return QPN_ERANGE; }
    if (st & 32) { qpn_set_error("a NaN or an infinity in the teacher logits of a distillation loss (qpn_distill_loss / qpn_train_distill): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"); return QPN_ERANGE; }
    if (st & 64) { qpn_set_error("a NaN, infinite or negative value among the sample weights of a loss with options (qpn_ce_loss_opts / qpn_distill_loss_opts / qpn_train_loss_opts; it counted as 0): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"); return QPN_ERANGE; }
    if (st & (1 << 16)) { qpn_set_error("non-finite gradient norm (an inf or NaN in the gradient): the step's Adam update, and that of the steps enqueued behind it until this report, were skipped on the device: parameters and moments are those of the last clean step"); return QPN_ERANGE; }
    if (st & 8) { qpn_set_error("a peer rank flagged its chunk of this data-parallel step, or an earlier micro-step of this accumulation window was flagged (a tap or target out of range, or an abandoned stack launch there): every rank skipped the update, the replicas are unchanged"); return QPN_ERANGE; }
    return QPN_OK;
}
static int qpn_train_loss(TrainState* t, double* h_loss, hipStream_t stream) {
    double parts[64];
    QPN_HIP(hipMemcpyAsync(parts, t->d_loss, sizeof(parts), hipMemcpyDeviceToHost, stream));
    QPN_HIP(hipStreamSynchronize(stream));
    *h_loss = loss_sum(parts);
    return QPN_OK;
}
static int qpn_train_loss_enqueue(TrainState* t, hipStream_t stream_) {
    const int slot = t->loss_newest ^ 1;
    if (t->loss_pending[slot]) QPN_HIP(hipEventSynchronize(t->ev_loss[slot]));      // (an uncollected copy of two calls ago: dropped)
    // (behind a clipping Adam launch the step's gradient norm, d_loss[64], leaves in the same copy)
    QPN_HIP(hipMemcpyAsync(t->h_loss_pinned + LOSS_SLOT * slot, t->d_loss, (t->gnorm_last ? 65 : 64) * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    t->gnorm_slot[slot] = t->gnorm_last;
    QPN_HIP(hipEventRecord(t->ev_loss[slot], (hipStream_t)stream_));
    t->loss_pending[slot] = true; t->loss_newest = slot;
    return QPN_OK;
}
static int qpn_train_loss_collect(TrainState* t, int newest, double* h_loss, int* h_valid) {
    *h_valid = 0; *h_loss = 0.0;
    const int slot = newest ? t->loss_newest : t->loss_newest ^ 1;
    t->gnorm_collected_valid = false;
    if (!t->loss_pending[slot]) return QPN_OK;
    QPN_HIP(hipEventSynchronize(t->ev_loss[slot]));
    t->loss_pending[slot] = false;
    *h_loss = loss_sum(t->h_loss_pinned + LOSS_SLOT * slot); *h_valid = 1;
    if (t->gnorm_slot[slot]) { t->gnorm_collected = t->h_loss_pinned[LOSS_SLOT * slot + 64]; t->gnorm_collected_valid = true; }
    return QPN_OK;
}
static int qpn_train_status(TrainState* t, hipStream_t stream_) {
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    int st = 0;
    QPN_HIP(hipMemcpy(&st, t->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) QPN_HIP(hipMemsetAsync(t->d_status, 0, sizeof(int), (hipStream_t)stream_));          // sticky until read: reported once
    t->last_stream = (hipStream_t)stream_;
    if (st & 4) t->stack_disabled = true;
    t->status_pending[0] = t->status_pending[1] = false;
    return status_to_rc(st);
}
static int status_collect_slot(TrainState* t, int slot) {
    if (!t->status_pending[slot]) return QPN_OK;
    QPN_HIP(hipEventSynchronize(t->ev_status[slot]));
    t->status_pending[slot] = false;
    const int st = t->h_status_pinned[slot];
    if (st & 4) t->stack_disabled = true;
    if (st) {
        QPN_HIP(hipMemsetAsync(t->d_status, 0, sizeof(int), t->last_stream));
        const int other = slot ^ 1;                                   // ... also where the other slot copied the same sticky bits before this clear
        if (t->status_pending[other]) {
            QPN_HIP(hipEventSynchronize(t->ev_status[other]));
            t->h_status_pinned[other] &= ~st;
            if (!t->h_status_pinned[other]) t->status_pending[other] = false;
        }
    }
    return status_to_rc(st);
}
static int qpn_train_status_enqueue(TrainState* t, hipStream_t stream_) {
    int rc;
    const int slot = t->status_newest ^ 1;
    t->last_stream = (hipStream_t)stream_;
    rc = status_collect_slot(t, slot); if (rc) return rc;            // (two enqueues old: long done)
    QPN_HIP(hipMemcpyAsync(t->h_status_pinned + slot, t->d_status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream_));
    QPN_HIP(hipEventRecord(t->ev_status[slot], (hipStream_t)stream_));
    t->status_pending[slot] = true; t->status_newest = slot;
    return QPN_OK;
}
static int qpn_train_status_collect(TrainState* t) {
    int rc;
    rc = status_collect_slot(t, t->status_newest ^ 1); if (rc) return rc;
    return status_collect_slot(t, t->status_newest);
}
static int qpn_train_status_poll(TrainState* t, int* pending) {
    int rc;
    if (pending) *pending = 0;
    for (int k = 0; k < 2; ++k) {
        const int slot = k == 0 ? t->status_newest ^ 1 : t->status_newest;      // older first
        if (!t->status_pending[slot]) continue;
        if (hipEventQuery(t->ev_status[slot]) != hipSuccess) { (void)hipGetLastError(); if (pending) ++*pending; continue; }
        rc = status_collect_slot(t, slot); if (rc) return rc;
    }
    return QPN_OK;
}
static int qpn_train_status_collect_lagged(TrainState* t) {
    return status_collect_slot(t, t->status_newest ^ 1);
}
static int qpn_adam_step_avg(TrainState* t, const Call& a, bool clip) {
    if (t) { t->last_stream = (hipStream_t)a.stream; t->gnorm_last = clip; }
    fake_launch(a.raise, a.id, clip, nullptr, nullptr, nullptr, a.stream);
    return QPN_OK;
}
static int qpn_grad_accumulate(TrainState* t, const Call& a) {
    if (t) { t->last_stream = (hipStream_t)a.stream; t->gnorm_last = false; }
    return QPN_OK;
}
static int qpn_train_grad_norm(TrainState* t, double* h_norm, int* h_valid, hipStream_t stream_) {
    *h_norm = 0.0; *h_valid = 0;
    if (!t->gnorm_last) return QPN_OK;
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    QPN_HIP(hipMemcpy(h_norm, t->d_loss + 64, sizeof(double), hipMemcpyDeviceToHost));
    *h_valid = 1;
    return QPN_OK;
}
static int qpn_train_grad_norm_lagged(TrainState* t, double* h_norm, int* h_valid) {
    *h_norm = 0.0; *h_valid = 0;
    if (!t->gnorm_collected_valid) return QPN_OK;
    *h_norm = t->gnorm_collected; *h_valid = 1;
    return QPN_OK;
}
static int train_step_body(TrainState* t, const Call& a, Out& o) {
    int rc;
    const int loss_mode = a.loss_mode;
    const bool closing = a.closing;
    const bool clip = closing && a.clip;
    const hipStream_t stream = (hipStream_t)a.stream;
    t->last_stream = stream;
    rc = qpn_train_status_collect_lagged(t); if (rc) return rc;          // the check of the step before the previous one (never waits for queued work)
    t->last_stream = stream;                                             // (train_forward_impl)
    if (loss_mode == 2) {
        if (closing) { rc = qpn_adam_step_avg(t, a, clip); if (rc) return rc; }
        else { t->last_stream = stream; t->gnorm_last = false; fake_launch(a.raise, a.id, false, nullptr, nullptr, nullptr, stream); }      // (no Adam launch: this micro-step has no norm)
        rc = qpn_train_loss(t, &o.loss, a.stream); if (rc) return rc;
        o.valid = 1;
        if (clip) { int nv = 0; rc = qpn_train_grad_norm(t, &o.norm, &nv, a.stream); if (rc) return rc; }      // (the stream has just been drained)
        return qpn_train_status(t, a.stream);
    }
    const int sslot = t->status_newest ^ 1;
    rc = status_collect_slot(t, sslot); if (rc) return rc;               // (two enqueues old: long done)
    const int lslot = t->loss_newest ^ 1;
    if (loss_mode == 1 && t->loss_pending[lslot]) QPN_HIP(hipEventSynchronize(t->ev_loss[lslot]));      // (an uncollected copy of two calls ago: dropped)
    double* const hl = loss_mode == 1 ? t->h_loss_pinned + LOSS_SLOT * lslot : nullptr;
    t->gnorm_last = clip;
    t->last_stream = stream;
    fake_launch(a.raise, a.id, clip, t->h_status_pinned + sslot, hl, hl ? hl + 64 : nullptr, stream);
    QPN_HIP(hipEventRecord(t->ev_status[sslot], stream));
    t->status_pending[sslot] = true; t->status_newest = sslot;
    if (loss_mode == 1) {
        QPN_HIP(hipEventRecord(t->ev_loss[lslot], stream));
        t->loss_pending[lslot] = true; t->loss_newest = lslot; t->gnorm_slot[lslot] = clip;
        rc = qpn_train_loss_collect(t, 0, &o.loss, &o.valid); if (rc) return rc;
        if (t->gnorm_collected_valid) o.norm = t->gnorm_collected;
    }
    return QPN_OK;
}
}      // namespace old

// ---------------------------------------------------------------- the ledger, executed as train_report.hip executes it
// (line for line train_report.hip's functions: a change there is made here too)
namespace now {
struct Report {
    ReportLedger ledger; hipStream_t last_stream = 0; int* h_status = nullptr; hipEvent_t ev_status[2] = {0, 1}; double* h_loss = nullptr; hipEvent_t ev_loss[2] = {2, 3};
    int* d_status = nullptr; double* d_loss = nullptr;
    void call_on(hipStream_t s) { last_stream = s; }
    void call_on(hipStream_t s, StepEnd e) { last_stream = s; ledger.step_ended(e); }
};
static int report_rc(const StatusRc& r, int w) { g_out->word = w; g_out->reported = w != 0; if (r.rc) qpn_set_error(r.msg); return r.rc; }
static int status_collect_slot(Report& r, int slot) {
    if (!r.ledger.status_pending[slot]) return QPN_OK;
    QPN_HIP(hipEventSynchronize(r.ev_status[slot]));
    const int st = r.h_status[slot];
    const StatusLanded d = r.ledger.status_landed(slot, st);
    if (d.clear) QPN_HIP(hipMemsetAsync(r.d_status, 0, sizeof(int), r.last_stream));
    if (d.mask_other) {
        QPN_HIP(hipEventSynchronize(r.ev_status[d.other]));
        r.h_status[d.other] &= ~st;
        r.ledger.other_masked(d.other, r.h_status[d.other]);
    }
    return report_rc(d.rc, st);
}
struct Slots { int* h_status; double* h_loss; double* h_norm; int sslot, lslot; };
static int report_open(Report& r, bool lagged_loss, StepEnd end, hipStream_t stream, Slots* s) {
    s->sslot = r.ledger.status_next();
    int rc = status_collect_slot(r, s->sslot); if (rc) return rc;
    const LossNext ln = r.ledger.loss_next();
    s->lslot = ln.slot;
    if (lagged_loss && ln.wait_drop) QPN_HIP(hipEventSynchronize(r.ev_loss[ln.slot]));
    r.call_on(stream, end);
    s->h_status = r.h_status + s->sslot;
    s->h_loss = lagged_loss ? r.h_loss + LOSS_SLOT * ln.slot : nullptr;
    s->h_norm = lagged_loss ? s->h_loss + LOSS_NORM_AT : nullptr;
    return QPN_OK;
}
static int report_close(Report& r, const Slots& s, hipStream_t stream) {
    QPN_HIP(hipEventRecord(r.ev_status[s.sslot], stream));
    r.ledger.status_sent(s.sslot);
    if (s.h_loss) { QPN_HIP(hipEventRecord(r.ev_loss[s.lslot], stream)); r.ledger.loss_sent(s.lslot); }
    return QPN_OK;
}
static int train_loss(Report& r, double* h_loss, hipStream_t stream) {
    double parts[LOSS_PARTS];
    QPN_HIP(hipMemcpyAsync(parts, r.d_loss, sizeof(parts), hipMemcpyDeviceToHost, stream));
    QPN_HIP(hipStreamSynchronize(stream));
    *h_loss = loss_sum(parts);
    return QPN_OK;
}
static int loss_enqueue(Report& r, hipStream_t stream) {
    const LossNext ln = r.ledger.loss_next();
    if (ln.wait_drop) QPN_HIP(hipEventSynchronize(r.ev_loss[ln.slot]));
    QPN_HIP(hipMemcpyAsync(r.h_loss + LOSS_SLOT * ln.slot, r.d_loss, r.ledger.loss_doubles() * sizeof(double), hipMemcpyDeviceToHost, stream));
    QPN_HIP(hipEventRecord(r.ev_loss[ln.slot], stream));
    r.ledger.loss_sent(ln.slot);
    return QPN_OK;
}
static int loss_collect(Report& r, int newest, double* h_loss, int* h_valid) {
    *h_valid = 0; *h_loss = 0.0;
    const LossCollect c = r.ledger.loss_collect(newest);
    if (!c.valid) return QPN_OK;
    QPN_HIP(hipEventSynchronize(r.ev_loss[c.slot]));
    const double* slot = r.h_loss + LOSS_SLOT * c.slot;
    r.ledger.loss_landed(c.slot, slot[LOSS_NORM_AT]);
    *h_loss = loss_sum(slot); *h_valid = 1;
    return QPN_OK;
}
static int train_status(Report& r, hipStream_t stream) {
    QPN_HIP(hipStreamSynchronize(stream));
    int st = 0;
    QPN_HIP(hipMemcpy(&st, r.d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) QPN_HIP(hipMemsetAsync(r.d_status, 0, sizeof(int), stream));
    r.call_on(stream);
    return report_rc(r.ledger.status_drained(st).rc, st);
}
static int status_enqueue(Report& r, hipStream_t stream) {
    const int slot = r.ledger.status_next();
    r.call_on(stream);
    int rc = status_collect_slot(r, slot); if (rc) return rc;
    QPN_HIP(hipMemcpyAsync(r.h_status + slot, r.d_status, sizeof(int), hipMemcpyDeviceToHost, stream));
    QPN_HIP(hipEventRecord(r.ev_status[slot], stream));
    r.ledger.status_sent(slot);
    return QPN_OK;
}
static int status_collect(Report& r, bool newest_too) {
    const SlotOrder o = r.ledger.status_order(newest_too);
    for (int k = 0; k < o.n; ++k) { int rc = status_collect_slot(r, o.slot[k]); if (rc) return rc; }
    return QPN_OK;
}
static int status_poll(Report& r, int* pending) {
    *pending = 0;
    const SlotOrder o = r.ledger.status_order(true);
    for (int k = 0; k < o.n; ++k) {
        const int slot = o.slot[k];
        if (!r.ledger.status_pending[slot]) continue;
        if (hipEventQuery(r.ev_status[slot]) != hipSuccess) { (void)hipGetLastError(); ++*pending; continue; }
        int rc = status_collect_slot(r, slot); if (rc) return rc;
    }
    return QPN_OK;
}
static int grad_norm(Report& r, double* h_norm, int* h_valid, hipStream_t stream) {
    *h_norm = 0.0; *h_valid = 0;
    if (!r.ledger.norm_live()) return QPN_OK;
    QPN_HIP(hipStreamSynchronize(stream));
    QPN_HIP(hipMemcpy(h_norm, r.d_loss + LOSS_NORM_AT, sizeof(double), hipMemcpyDeviceToHost));
    *h_valid = 1;
    return QPN_OK;
}
static int grad_norm_lagged(Report& r, double* h_norm, int* h_valid) {
    *h_norm = 0.0; *h_valid = 0;
    if (!r.ledger.gnorm_collected_valid) return QPN_OK;
    *h_norm = r.ledger.gnorm_collected; *h_valid = 1;
    return QPN_OK;
}
static int train_step_body(Report& r, const Call& a, Out& o) {      // train_host.hip's, with the forward, the backward and the launches' arguments left out
    const bool clip = a.closing && a.clip;
    const StepEnd end = clip ? StepEnd::AdamClipped : a.closing ? StepEnd::AdamPlain : StepEnd::NoAdam;
    r.call_on(a.stream);
    int rc = status_collect(r, false); if (rc) return rc;
    r.call_on(a.stream);                                             // (train_forward_impl)
    if (a.loss_mode == 2) {
        r.call_on(a.stream, end);                                    // (qpn_adam_step_avg, or the micro-step that has none)
        fake_launch(a.raise, a.id, clip, nullptr, nullptr, nullptr, a.stream);
        rc = train_loss(r, &o.loss, a.stream); if (rc) return rc;
        o.valid = 1;
        if (clip) { int nv = 0; rc = grad_norm(r, &o.norm, &nv, a.stream); if (rc) return rc; }
        return train_status(r, a.stream);
    }
    Slots rs;
    rc = report_open(r, a.loss_mode == 1, end, a.stream, &rs); if (rc) return rc;
    fake_launch(a.raise, a.id, clip, rs.h_status, rs.h_loss, rs.h_norm, a.stream);
    rc = report_close(r, rs, a.stream); if (rc) return rc;
    if (a.loss_mode == 1) {
        rc = loss_collect(r, 0, &o.loss, &o.valid); if (rc) return rc;
        int nv = 0; rc = grad_norm_lagged(r, &o.norm, &nv); if (rc) return rc;
    }
    return QPN_OK;
}
}      // namespace now

// ---------------------------------------------------------------- the driver
// A fault is raised by the kernels of a step, and a report follows them: the one-call step's last kernel carries the armed bits, the call-by-call step's status copy
// has them right in front of it.  A step whose report was refused (its call returned an older flag instead) raised nothing: its bits stay armed.
// "Switch stream" moves the handle: the next TRAINING call (one that tells the library its stream and runs kernels or the status copy there) is on the other stream.
enum OpKind { STEP, STATUS_ENQUEUE, COLLECT, COLLECT_LAGGED, POLL, STATUS, LOSS_ENQUEUE, LOSS_COLLECT0, LOSS_COLLECT1, GRAD_NORM, GRAD_NORM_LAGGED, ADAM, ACCUMULATE, INJECT, SWITCH, CATCH_UP, N_OPS };
static const char* const OP_NAMES[N_OPS] = {"step", "status_enqueue", "collect", "collect_lagged", "poll", "status", "loss_enqueue", "loss_collect(0)", "loss_collect(1)", "grad_norm", "grad_norm_lagged", "adam_step_avg", "grad_accumulate", "inject", "switch_stream", "catch_up"};
static const int FLAG_BITS[7] = {1, 2, 4, 8, 32, 64, 1 << 16};
static long g_poll_waits = 0, g_lost_to_drain = 0, g_reports = 0, g_norms = 0;

static unsigned rnd_state;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void sequence(unsigned seed, int length, bool steps_only) {
    g_seed = seed; rnd_state = seed * 2654435761u + 12345u;
    Dev* devs = new Dev[2];      // [0]: the transcription's, [1]: the ledger's
    old::TrainState ot; now::Report nr;
    ot.d_status = devs[0].d_status; ot.d_loss = devs[0].d_loss; ot.h_status_pinned = devs[0].h_status; ot.h_loss_pinned = devs[0].h_loss;
    nr.d_status = devs[1].d_status; nr.d_loss = devs[1].d_loss; nr.h_status = devs[1].h_status; nr.h_loss = devs[1].h_loss;
    hipStream_t cur = 0; bool move = false; int armed = 0; double next_id = 1.0, dev_id = 0.0; long steps_done = 0;
    // (d) what the driver knows of the losses on their way, kept by the rules of the C ABI's documentation, not by the ledger: the newest report and the one before it;
    // the loss each must return; whether the latest of {an Adam launch that clipped, one that did not, a step or accumulate call without one} in front of it clipped
    bool last_clipped = false; int newest = 0; bool sent_[2] = {}, clipped_[2] = {}; double id_[2] = {};
    static const int tail[8] = {CATCH_UP, COLLECT, COLLECT, STATUS_ENQUEUE, CATCH_UP, COLLECT, COLLECT, STATUS};
    static const int steps[8] = {STEP, STEP, STEP, STEP, STEP, INJECT, CATCH_UP, STEP};
    for (int i = 0; i < length + 8; ++i, ++n_ops) {
        const bool flushing = i >= length;      // the tail: everything lands and every report is fetched, so that (a) can be closed
        const int op = flushing ? tail[i - length] : steps_only ? steps[rnd() % 8] : (rnd() % 4 == 0) ? (int)STEP : (int)(rnd() % N_OPS);
        Call c = {};
        if (op == STEP) { const unsigned m = rnd() % 8; c.loss_mode = steps_only ? (m < 7 ? (int)(m & 1) : 2) : (int)(rnd() % 3); c.clip = rnd() & 1; c.closing = rnd() % 4 != 0; }
        if (op == ADAM) { c.clip = rnd() & 1; c.closing = true; }
        if (g_trace) printf("op %d: %s mode %d clip %d closing %d armed %#x stream %d%s\n", i, OP_NAMES[op], c.loss_mode, (int)c.clip, (int)c.closing, armed, cur, move ? " (moving)" : "");
        if (op == INJECT) { armed |= FLAG_BITS[rnd() % 7]; if (rnd() % 4 == 0) armed |= FLAG_BITS[rnd() % 7]; continue; }
        if (op == SWITCH) { move = !move; continue; }
        const int land = (int)(rnd() % 6);
        if (op == CATCH_UP) { for (int w = 0; w < 2; ++w) devs[w].land(flushing ? 1 << 20 : land); continue; }
        const bool training_call = op == STEP || op == STATUS_ENQUEUE || op == STATUS || op == ADAM || op == ACCUMULATE;
        if (training_call && move) { cur ^= 1; move = false; for (int w = 0; w < 2; ++w) devs[w].moved_at[cur] = devs[w].serial; }
        const bool carries = op == STEP || op == STATUS_ENQUEUE;
        c.stream = cur; c.raise = op == STEP ? armed : 0; c.id = op == STEP ? next_id : -1.0;
        Out out[2]; long launched[2];
        for (int w = 0; w < 2; ++w) {
            D = &devs[w]; D->log.clear(); D->step_now = steps_done; g_msg = ""; g_out = &out[w];
            if (training_call) D->latest_call_stream = cur;
            D->copy_raise = op == STATUS_ENQUEUE ? armed : 0;
            const long launches = D->launches;
            Out& o = out[w];
            int rc = 0;
            switch (op) {
            case STEP: rc = w ? now::train_step_body(nr, c, o) : old::train_step_body(&ot, c, o); break;
            case STATUS_ENQUEUE: rc = w ? now::status_enqueue(nr, cur) : old::qpn_train_status_enqueue(&ot, cur); break;
            case COLLECT: rc = w ? now::status_collect(nr, true) : old::qpn_train_status_collect(&ot); break;
            case COLLECT_LAGGED: rc = w ? now::status_collect(nr, false) : old::qpn_train_status_collect_lagged(&ot); break;
            case POLL: D->in_poll = true; rc = w ? now::status_poll(nr, &o.pending) : old::qpn_train_status_poll(&ot, &o.pending); D->in_poll = false; break;
            case STATUS: rc = w ? now::train_status(nr, cur) : old::qpn_train_status(&ot, cur); break;
            case LOSS_ENQUEUE: rc = w ? now::loss_enqueue(nr, cur) : old::qpn_train_loss_enqueue(&ot, cur); break;
            case LOSS_COLLECT0: case LOSS_COLLECT1:
                rc = w ? now::loss_collect(nr, op == LOSS_COLLECT1, &o.loss, &o.valid) : old::qpn_train_loss_collect(&ot, op == LOSS_COLLECT1, &o.loss, &o.valid);
                if (!rc) rc = w ? now::grad_norm_lagged(nr, &o.norm, &o.nvalid) : old::qpn_train_grad_norm_lagged(&ot, &o.norm, &o.nvalid);      // what _lagged answers after the call
                break;
            case GRAD_NORM: rc = w ? now::grad_norm(nr, &o.norm, &o.nvalid, cur) : old::qpn_train_grad_norm(&ot, &o.norm, &o.nvalid, cur); break;
            case GRAD_NORM_LAGGED: rc = w ? now::grad_norm_lagged(nr, &o.norm, &o.nvalid) : old::qpn_train_grad_norm_lagged(&ot, &o.norm, &o.nvalid); break;
            case ADAM:
                if (w) { nr.call_on(cur, c.clip ? StepEnd::AdamClipped : StepEnd::AdamPlain); fake_launch(0, c.id, c.clip, nullptr, nullptr, nullptr, cur); }
                else rc = old::qpn_adam_step_avg(&ot, c, c.clip);
                break;
            case ACCUMULATE:
                if (w) nr.call_on(cur, StepEnd::NoAdam); else rc = old::qpn_grad_accumulate(&ot, c);
                break;
            }
            o.rc = rc; o.msg = rc ? g_msg : "";
            launched[w] = D->launches - launches;
            D->copy_raise = 0;
            if (!flushing && land > 3) D->land(land - 3);      // (time passes between calls, too)
        }
        if (g_trace) { printf("    -> rc %d word %#x loss %g valid %d norm %g nvalid %d pending %d | device word %#x, unreported %#x, in flight %zu, exceptions %ld %ld | actions", out[1].rc, out[1].word, out[1].loss, out[1].valid, out[1].norm, out[1].nvalid, out[1].pending, devs[1].d_status[0], devs[1].unreported, devs[1].q.size(), devs[1].n_poll_waits, devs[1].n_lost_to_drain); for (long v : devs[1].log) printf(" %ld", v); printf("\n"); }
        // ---- both runs agree
        CHECK(out[0].same(out[1]) && launched[0] == launched[1]);
        CHECK(devs[0].log == devs[1].log);
        CHECK(!memcmp(devs[0].h_status, devs[1].h_status, 2 * sizeof(int)) && devs[0].d_status[0] == devs[1].d_status[0]);
        CHECK(devs[0].q.size() == devs[1].q.size() && devs[0].landed == devs[1].landed);
        const ReportLedger& L = nr.ledger;
        CHECK(ot.last_stream == nr.last_stream && ot.stack_disabled == L.stack_disabled && ot.gnorm_last == L.gnorm_last && ot.status_newest == L.status_newest && ot.loss_newest == L.loss_newest);
        CHECK(ot.gnorm_collected_valid == L.gnorm_collected_valid && (!L.gnorm_collected_valid || ot.gnorm_collected == L.gnorm_collected));
        for (int s = 0; s < 2; ++s) CHECK(ot.status_pending[s] == L.status_pending[s] && ot.loss_pending[s] == L.loss_pending[s] && (!L.loss_pending[s] || ot.gnorm_slot[s] == L.gnorm_slot[s]));
        // ---- the invariants, on the ledger's run ((c), (e) and (f) are checked by the fake device as the calls are made)
        const Out& o = out[1];
        const StatusRc want = status_to_rc(o.word);
        CHECK(o.rc == want.rc && !strcmp(o.msg, want.msg) && (o.rc != 0) == o.reported);      // (a) ... as the code status_to_rc gives for the set of bits then set
        if (o.reported) {
            const long oldest = devs[1].reported(o.word); devs[0].reported(o.word);           // (a) ... raised, and not returned before
            if (steps_only) CHECK(steps_done - oldest <= 2);                                  // (b) no later than the second step after the one that raised it
            ++g_reports;
        }
        if (o.word & 4) CHECK(L.stack_disabled);
        const bool sent = op == STEP ? launched[1] == 1 : o.rc == 0;      // the call got as far as its launch / copy
        if (carries && sent) armed = 0;
        if (sent && (op == STEP || op == ADAM)) last_clipped = c.closing && c.clip;
        if (sent && op == ACCUMULATE) last_clipped = false;
        if (sent && op == STEP) { dev_id = c.id; next_id += 1.0; ++steps_done; }
        if (sent && ((op == STEP && c.loss_mode == 1) || op == LOSS_ENQUEUE)) { newest ^= 1; sent_[newest] = true; clipped_[newest] = last_clipped; id_[newest] = dev_id; }
        // (d) a norm returned with a loss comes from the same slot write as that loss; absent when that step did not clip or did not close a window
        if (op == LOSS_COLLECT0 || op == LOSS_COLLECT1 || (op == STEP && c.loss_mode == 1 && sent)) {
            const int slot = op == LOSS_COLLECT1 ? newest : newest ^ 1;
            const bool norm = op == STEP ? o.norm != 0.0 : o.nvalid != 0;
            CHECK(o.valid == (int)sent_[slot]);
            if (o.valid) { CHECK(o.loss == id_[slot] && norm == clipped_[slot]); if (norm) { CHECK(o.norm == o.loss + 0.5); ++g_norms; } }
            else CHECK(!norm && o.loss == 0.0 && o.norm == 0.0);
            sent_[slot] = false;
        }
        if (op == STEP && c.loss_mode == 2 && sent) CHECK(o.valid && o.loss == c.id && o.norm == (c.closing && c.clip ? c.id + 0.5 : 0.0));
        if (op == GRAD_NORM) { CHECK(o.nvalid == (int)last_clipped); if (o.nvalid) CHECK(o.norm == dev_id + 0.5); }
    }
    CHECK(devs[1].unreported == 0);      // (a) every injected flag was returned
    g_poll_waits += devs[1].n_poll_waits; g_lost_to_drain += devs[1].n_lost_to_drain;
    delete[] devs;
}

int main(int argc, char** argv) {
    if (argc == 4) { g_trace = true; sequence((unsigned)strtoul(argv[1], nullptr, 10), atoi(argv[2]), atoi(argv[3]) != 0); return 0; }      // dev: <seed> <length> <steps only>, printed operation by operation
    // status_to_rc's table, one line per bit the kernels set
    for (int b = 0; b < 7; ++b) { const StatusRc r = status_to_rc(FLAG_BITS[b]); printf("STATUS %d %d %s\n", FLAG_BITS[b], r.rc, r.msg); }
    CHECK(status_to_rc(0).rc == QPN_OK && status_to_rc(1 | 4).rc == QPN_ERANGE && status_to_rc(4 | 2).rc == QPN_ENODEV);
    printf("GEOMETRY %d %d %d\n", LOSS_SLOT, LOSS_PARTS, LOSS_NORM_AT);
    for (unsigned seed = 1; seed <= 1500; ++seed) sequence(seed, 200, false);
    for (unsigned seed = 1; seed <= 1500; ++seed) sequence(100000 + seed, 100, true);
    printf("REPORTS %ld NORMS %ld POLL_WAITED_FOR_OTHER %ld LOST_TO_DRAIN %ld\n", g_reports, g_norms, g_poll_waits, g_lost_to_drain);
    printf("TRAIN_REPORT_SWEEP_OK %ld\n", n_ops);
    return 0;
}
