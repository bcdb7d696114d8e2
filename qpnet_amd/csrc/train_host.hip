// train_host.hip -- host orchestration of the training step behind the C ABI:
//   qpn_train_forward / qpn_train_backward  (QPNet.forward + autograd, reference qpnet.py:239-312)
//   qpn_ce_loss                              (CrossEntropyLoss mean, reference qpnet_train.py:430,526-528)
//   qpn_adam_step                            (torch.optim.Adam, reference qpnet_train.py:426-429,531)
#include "train_state.h"
#include <algorithm>
#include <memory>
#include <string.h>

int qpn_launch_fwd(const TrainParams& p, const TrainFwdPlan& pl, const AuxGeom& ag, const StackQ& sq, hipStream_t stream, const TrainBwd& fuse_post_bwd, const RefreshArgs& rf);
static CeOpts ce_opts_of(const qpn_loss_opts& o, double* mass, double* d_mass);
int qpn_launch_bwd(const TrainParams& p, const TrainBwd& bw, const TrainBwdPlan& pl, const AuxGeom& ag, const StackQ& sq, hipStream_t stream);
int qpn_launch_fwd_gemm(const TrainParams& p, const TrainGemm& w, hipStream_t stream);
int qpn_launch_bwd_gemm(const TrainParams& p, const TrainBwd& bw, const TrainGemm& w, hipStream_t stream);

// The environment is read HERE, once per handle: the launch path of a step never calls getenv().
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return (e && *e) ? atoi(e) : dflt; }
void qpn_train_knobs_parse(TrainKnobs& k) {
    k.serial = env_int("QPN_TRAIN_SERIAL", 0) != 0;
    k.stack_q_fwd = env_int("QPN_STACK_QUEUE", 1) != 0;
    k.stack_q_bwd = k.stack_q_fwd && env_int("QPN_STACK_QUEUE_BWD", 1) != 0;
    k.stack_wgs = env_int("QPN_STACK_WGS", 0); if (k.stack_wgs < 0 || k.stack_wgs > 4096) k.stack_wgs = 0;
    k.stack_wgs_bwd = env_int("QPN_STACK_WGS_BWD", 0); if (k.stack_wgs_bwd < 0 || k.stack_wgs_bwd > 4096) k.stack_wgs_bwd = 0;
    k.persist_fwd = env_int("QPN_LAYER_PERSIST", 1) != 0;
    k.persist_bwd = env_int("QPN_LAYER_BWD_PERSIST", 1) != 0;
    k.wgrad_generic = getenv("QPN_WGRAD_GENERIC") != nullptr;
    k.wgrad_chunks = env_int("QPN_WGRAD_CHUNKS", 0); if (k.wgrad_chunks < 1 || k.wgrad_chunks > 512) k.wgrad_chunks = 0;
    k.wgrad_chunks_side = env_int("QPN_WGRAD_CHUNKS_SIDE", 0); if (k.wgrad_chunks_side < 1 || k.wgrad_chunks_side > 512) k.wgrad_chunks_side = 0;
    k.up_side = env_int("QPN_UP_SIDE", 1) != 0;
    k.reduce_early = env_int("QPN_REDUCE_EARLY", 1) != 0;
    k.wr_side = env_int("QPN_WR_SIDE", 1) != 0;
    k.post_fuse = env_int("QPN_POST_FUSE", 1) != 0;
    k.post_pair = env_int("QPN_POST_WGRAD_PAIR", 1) != 0;
    k.zero_in_post = env_int("QPN_ZERO_IN_POST", 1) != 0;
    k.post_wide = env_int("QPN_POST_WIDE", 1) != 0;
    k.xcd_swizzle = getenv("QPN_NO_XCD_SWIZZLE") == nullptr;
    k.ce_separate = getenv("QPN_CE_SEPARATE") != nullptr;
    k.event_fence = env_int("QPN_EVENT_FENCE", 0) == 1;
    k.aux_hoist = env_int("QPN_AUX_HOIST", 1) != 0;
    k.prep_fuse = env_int("QPN_PREP_FUSE", 1) != 0;
    k.test_stack_gives_up = false;
#ifdef QPN_TESTING
    k.test_stack_gives_up = env_int("QPN_TEST_STACK_GIVES_UP", 0) == 1;
#endif
}

int qpn_num_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256; cached[dev] = n; }
    return cached[dev];
}

// ---- per-group timing
// Marks are HIP events on the stream a launch went to; a group's time is the sum, over its marks, of the time since the PREVIOUS mark on the same stream
// (group -1: a baseline only -- behind a cross-stream wait, so that the wait is nobody's time).  Serial mode (qpn_train_profile_begin) puts the whole
// step on one stream: a kernel's time alone.  Overlapped mode (qpn_train_profile_begin_overlapped) leaves the step as the timed loop runs it -- the skip /
// post-net weight gradients, the early reduction, the aux tail and dWr on the side stream next to the stack backward and dW1 -- and times every launch
// where it runs: what a kernel costs in the step, which is what the bench line's roofline.kernel is chosen by.
struct Prof { bool on = false; bool overlapped = false; std::vector<hipEvent_t> ev; std::vector<int> grp; std::vector<hipStream_t> st; size_t used = 0; };
static thread_local Prof g_prof;
bool qpn_prof_active() { return g_prof.on; }
bool qpn_prof_serial() { return g_prof.on && !g_prof.overlapped; }
void qpn_prof_mark(int group, hipStream_t stream) {
    Prof& P = g_prof;
    if (!P.on) return;
    if (P.used == P.ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; P.ev.push_back(e); P.grp.push_back(0); P.st.push_back(nullptr); }
    P.grp[P.used] = group; P.st[P.used] = stream;
    (void)hipEventRecord(P.ev[P.used++], stream);
}
extern "C" int qpn_train_profile_begin(qpn_handle* h, void* stream) {
    (void)h; g_prof.on = true; g_prof.overlapped = false; g_prof.used = 0;
    qpn_prof_mark(-1, (hipStream_t)stream);
    return QPN_OK;
}
extern "C" int qpn_train_profile_begin_overlapped(qpn_handle* h, void* stream) {
    (void)h; g_prof.on = true; g_prof.overlapped = true; g_prof.used = 0;
    qpn_prof_mark(-1, (hipStream_t)stream);
    return QPN_OK;
}
extern "C" int qpn_train_profile_mark(qpn_handle* h, int group, void* stream) {
    (void)h; qpn_prof_mark(group, (hipStream_t)stream); return QPN_OK;
}
extern "C" int qpn_train_profile_end(qpn_handle* h, float* h_ms, int n, void* stream) {
    Prof& P = g_prof;
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (h && h->train && h->train->side) QPN_HIP(hipStreamSynchronize(h->train->side));
    for (int i = 0; i < n; ++i) h_ms[i] = 0.f;
    for (size_t i = 1; i < P.used; ++i) {
        if (P.grp[i] < 0 || P.grp[i] >= n) continue;
        size_t j = i;
        while (j > 0 && P.st[j - 1] != P.st[i]) --j;              // the previous mark on the same stream
        if (j == 0) continue;
        float ms = 0.f;
        QPN_HIP(hipEventElapsedTime(&ms, P.ev[j - 1], P.ev[i]));
        h_ms[P.grp[i]] += ms;
    }
    P.on = false;
    return QPN_OK;
}

__global__ void k_gather_f(const float* __restrict__ flat, const int* __restrict__ map, float* __restrict__ out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { int m = map[i]; out[i] = m >= 0 ? flat[m] : 0.0f; }
}
// the per-step refresh of everything derived from the parameters, in ONE launch: weight blocks (fragment order or K-major), the
// transposed causal table, the packed bias sums; also clears the loss accumulator of the coming step
__global__ void k_refresh(const float* __restrict__ flat, const int* __restrict__ wmap, float* __restrict__ wout, int64_t nw,
                          const int* __restrict__ ctmap, float* __restrict__ ct, int64_t nct,
                          const int* __restrict__ bstart, const int* __restrict__ blist, float* __restrict__ bp, int nb,
                          int* __restrict__ status, double* __restrict__ loss) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nw) { const int m = wmap[i]; wout[i] = m >= 0 ? flat[m] : 0.0f; return; }
    i -= nw;
    if (i < nct) { ct[i] = flat[ctmap[i]]; return; }
    i -= nct;
    if (i < nb) { float a = 0.f; for (int j = bstart[i]; j < bstart[i + 1]; ++j) a += flat[blist[j]]; bp[i] = a; return; }
    i -= nb;
    // (the status word is STICKY: kernels OR into it, only qpn_train_status clears it when it reads it -- a check every N steps
    //  then still sees an out-of-range tap / target of any step in between; the reference asserts on every step)
    (void)status;
    if (i >= 16 && i < 16 + 64) loss[i - 16] = 0.0;
}
// device copy of a host map, with `spare` more entries behind it (never read); the buffer is the state's at once: whatever fails later, the guard of train_init frees it
static int upload(int** d, const std::vector<int>& v, size_t spare = 0) {
    QPN_HIP(hipMalloc(d, (v.size() + spare) * sizeof(int)));
    if (!v.empty()) QPN_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return QPN_OK;
}

// Per-handle training setup: plan the layout (train_plan.h -- all of the arithmetic, CPU-tested), upload its maps, create the events and streams.
// The state under construction is the guard's: every early return destroys it with what it had allocated
static int train_init(qpn_handle* h) {
    if (h->train) return QPN_OK;
    const Geom& g = h->g;
    std::unique_ptr<TrainState, void (*)(TrainState*)> t(new TrainState(), qpn_train_destroy);
    qpn_train_knobs_parse(t->knobs);
    const TrainPlan pl = train_plan(g, t->knobs, (g.C > 128 || getenv("QPN_TRAIN_GEMM")) && !getenv("QPN_TRAIN_TILES"));
    if (pl.rc) return pl.rc;
    t->lay = pl; t->ag = pl.ag; t->gm = pl.gm;
    TrainParams& p = t->tp;
    p.hoist = pl.hoist ? 1 : 0;
    p.C = g.C; p.S = g.S; p.Q = g.Q; p.A = g.A; p.Ap = pl.Ap; p.L = g.L; p.U = g.U;
    p.Kt = pl.Kt; p.Ktp = pl.Ktp; p.LC = pl.LC;
    p.causal_w = g.causal_w; p.causal_b = g.causal_b; p.up_w = g.up_w; p.up_b = g.up_b;
    for (int l = 0; l < g.L; ++l) {
        const TrainPlanLayer& s = pl.layers[l];
        TrLayer& ly = p.layers[l];
        ly.adaptive = s.adaptive; ly.dilation = s.dilation; ly.tap_off = -1;      // (tap_off, s_in, s_out: per call)
        ly.w1_f4 = s.w1_f4; ly.w1t_f4 = s.w1t_f4; ly.wr_f4 = s.wr_f4; ly.wrt_f4 = s.wrt_f4; ly.bias1 = s.bias1; ly.biasr = s.biasr;
    }
    p.ws_f4 = pl.ws_f4; p.wst_f4 = pl.wst_f4; p.p1_f4 = pl.p1_f4; p.p1t_f4 = pl.p1t_f4; p.p2_f4 = pl.p2_f4; p.p2t_f4 = pl.p2t_f4;
    p.bias_s = pl.bias_s; p.bias_p1 = pl.bias_p1; p.bias_p2 = pl.bias_p2;
    t->bw.sl = &t->lay.slabs; t->bw.gstage = pl.gstage; t->bw.nch = pl.nch; t->bw.n_params = g.n_params;

    int rc;
    const std::vector<int>& wmap = pl.use_gemm ? pl.h_gmap : pl.h_wmap;
    if (pl.use_gemm) {
        rc = upload(&t->d_gmap, wmap); if (rc) return rc;
        QPN_HIP(hipMalloc(&t->d_gwp, wmap.size() * sizeof(float)));
        t->gm.wp = t->d_gwp;
    }
    const size_t nfrag = pl.use_gemm ? 4 : wmap.size();      // (the GEMM path keeps its own K-major blocks: a token buffer stands in for the fragment-ordered ones)
    rc = upload(&t->d_wmap, pl.h_wmap, nfrag - pl.h_wmap.size()); if (rc) return rc;
    QPN_HIP(hipMalloc(&t->d_wp, nfrag * sizeof(float)));
    rc = upload(&t->d_bstart, pl.h_bstart); if (rc) return rc;
    rc = upload(&t->d_blist, pl.h_blist); if (rc) return rc;
    QPN_HIP(hipMalloc(&t->d_bp, (size_t)pl.n_bias * sizeof(float)));
    rc = upload(&t->d_gdst, pl.gdst_start); if (rc) return rc;
    rc = upload(&t->d_gdst_list, pl.gdst_list); if (rc) return rc;
    rc = upload(&t->d_gzero, pl.gzero, 1); if (rc) return rc;
    rc = upload(&t->d_ctmap, pl.h_ctmap); if (rc) return rc;
    QPN_HIP(hipMalloc(&t->d_ct, pl.h_ctmap.size() * sizeof(float)));
    QPN_HIP(hipMalloc(&t->d_status, 64));
    QPN_HIP(hipMemset(t->d_status, 0, 64));
    QPN_HIP(hipMalloc(&t->d_gnorm, TR_GN_BLOCKS * sizeof(double)));
    QPN_HIP(hipMemset(t->d_gnorm, 0, TR_GN_BLOCKS * sizeof(double)));
    QPN_HIP(hipMalloc(&t->d_loss, LOSS_SLOT * sizeof(double)));
    QPN_HIP(hipMemset(t->d_loss, 0, LOSS_SLOT * sizeof(double)));
    rc = t->report.init(); if (rc) return rc;
    QPN_HIP(hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking));          // on the handle's device (current at this call)
    // the fork / join events only order kernels of THIS device's streams: no system-scope fence (cache write-back for the host) at each record
    // (QPN_EVENT_FENCE=1 restores it)
    const unsigned evf = hipEventDisableTiming | (t->knobs.event_fence ? 0u : (unsigned)hipEventDisableSystemFence);
    QPN_HIP(hipEventCreateWithFlags(&t->ev_fork, evf));
    QPN_HIP(hipEventCreateWithFlags(&t->ev_join, evf));
    QPN_HIP(hipEventCreateWithFlags(&t->ev_mid, evf));
    QPN_HIP(hipEventCreateWithFlags(&t->ev_early, evf));
    h->train = t.release();
    return QPN_OK;
}

void qpn_train_destroy(TrainState* t) {
    if (!t) return;
    void* bufs[] = {t->d_wmap, t->d_wp, t->d_bstart, t->d_blist, t->d_bp, t->d_gdst, t->d_gdst_list, t->d_gzero, t->d_ws, t->d_tap, t->d_status, t->d_loss, t->d_gmap, t->d_gwp, t->d_ctmap, t->d_ct, t->d_sq, t->d_gnorm, t->d_loss3, t->d_mass};
    for (void* b : bufs) if (b) (void)hipFree(b);
    t->report.destroy();
    if (t->side) (void)hipStreamDestroy(t->side);
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    if (t->ev_mid) (void)hipEventDestroy(t->ev_mid);
    if (t->ev_early) (void)hipEventDestroy(t->ev_early);
    delete t;
}

// targets == nullptr: plain forward.  Otherwise the mean cross entropy (and d_dlogits) is computed too: inside the post-net kernel
// when the tile path can hold a row of logits in LDS, by a k_ce_hard launch (train_loss.hip) behind the forward otherwise.
// fuse_bwd: the caller runs this forward's backward next, with the same d_dlogits, whatever the loss is (qpn_train_step): the post-net's backward may run inside the forward's launch
static int train_forward_impl(qpn_handle* h, const float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                              const int64_t* d_x, const float* d_h, const float* d_dfac, float* d_logits,
                              const int64_t* d_targets, int64_t tgt_stride, float* d_dlogits, int want_logits, void* stream_, bool fuse_bwd = false) {
    // the soft-target arm (qpn_train_distill) belongs to the next forward that computes a loss: one shot, consumed here, also by a forward that fails below
    const float* d_teacher = nullptr; int64_t teacher_n = 0; float ds_alpha = 0.f, ds_temp = 1.f;
    if (h && d_targets && h->distill_t) { d_teacher = h->distill_t; teacher_n = h->distill_n; ds_alpha = h->distill_alpha; ds_temp = h->distill_temp; h->distill_t = nullptr; h->distill_n = 0; }
    // the loss-options arm (qpn_train_loss_opts): the same rules
    qpn_loss_opts lo = {}; bool lo_armed = false;
    if (h && d_targets && h->loss_opts_armed) { lo = h->loss_opts; lo_armed = true; h->loss_opts_armed = false; }
    int rc = need_dev(h); if (rc) return rc;
    rc = train_init(h); if (rc) return rc;
    TrainState* t = h->train;
    hipStream_t stream = (hipStream_t)stream_;
    const Geom& g = h->g;
    if (!d_flat || !d_x || !d_h || !d_dfac || !d_logits || B < 1 || BL < 1 || maxd < 1) { qpn_set_error("bad train_forward arguments"); return QPN_EINVAL; }
    if (d_targets && tgt_stride < BL) { qpn_set_error("bad train_forward_loss arguments: target rows shorter than batch_length"); return QPN_EINVAL; }
    if (d_teacher) {
        const int64_t want = (int64_t)B * BL * g.Q;
        if (teacher_n != want) {
            qpn_set_error("qpn_train_distill: n = %lld, this forward has B * BL * n_quantize = %d * %d * %d = %lld", (long long)teacher_n, B, BL, g.Q, (long long)want);
            return QPN_EINVAL;
        }
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cap_st);
        if (cap_st != hipStreamCaptureStatusNone) { qpn_set_error("qpn_train_distill: an armed forward cannot be captured (the arm is host state a replay would not renew)"); return QPN_ESTATE; }
    }
    if (lo_armed) {
        if (lo.d_weights && lo.n_weights != (int64_t)B * BL) {
            qpn_set_error("qpn_train_loss_opts: n_weights = %lld, this forward has B * BL = %d * %d = %lld rows", (long long)lo.n_weights, B, BL, (long long)B * BL);
            return QPN_EINVAL;
        }
        if (d_teacher && lo.label_smoothing > 0.f) { qpn_set_error("qpn_train_loss_opts: label_smoothing cannot be combined with a distillation teacher (the soft targets already smooth)"); return QPN_EINVAL; }
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cap_st);
        if (cap_st != hipStreamCaptureStatusNone) { qpn_set_error("qpn_train_loss_opts: an armed forward cannot be captured (the arm is host state a replay would not renew)"); return QPN_ESTATE; }
        if (lo.norm == 1 && !t->d_mass) QPN_HIP(hipMalloc(&t->d_mass, 72 * sizeof(double)));
    }
    // ---- the call's shape (train_launch_plan.h): rows, the layers' first valid rows and tap tables, the frames the rows touch, the queue positions -- or a refusal
    {
        const TrainShape shape = train_shape(g, t->lay, B, T, F, Td, BL, maxd);
        if (shape.rc) return shape.rc;      // (the state still describes the previous forward)
        t->shape = shape;
    }
    const TrainShape& sh = t->shape;
    TrainParams& p = t->tp;
    p.B = B; p.T = sh.T; p.F = sh.F; p.Td = sh.Td; p.BL = BL; p.N0 = sh.N0; p.N1 = sh.N1; p.maxd = maxd; p.ffirst = sh.ffirst; p.nfr = sh.nfr;
    const int L = g.L, N1 = p.N1;
    for (int l = 0; l < L; ++l) { TrLayer& ly = p.layers[l]; ly.s_in = sh.s_in[l]; ly.s_out = sh.s_out[l]; ly.tap_off = sh.tap_off[l]; t->ag.s_out[l] = sh.s_out[l]; p.qT[l] = sh.qT[l]; }
    for (int l = 0; l <= TR_MAXL; ++l) p.qP[l] = sh.qP[l];
    p.qtotal = sh.qtotal;
    // ---- carve the arena: ONE list (train_arena) gives its size and every buffer's place
    const TrainArena a = train_arena(t->lay, g, B, N1, BL, p.nfr);
    if (a.total > t->ws_cap) {
        if (t->d_ws) (void)hipFree(t->d_ws);
        t->d_ws = nullptr; t->ws_cap = 0;
        hipError_t e = hipMalloc(&t->d_ws, a.total * sizeof(float));
        if (e != hipSuccess) { qpn_set_error("hipMalloc(%zu MiB) for the training workspace failed", a.total * 4 >> 20); return QPN_ENOMEM; }
        t->ws_cap = a.total;
    }
    const size_t ntap = (size_t)std::max(L, 1) * B * N1;
    if (ntap > t->tap_cap) {
        if (t->d_tap) (void)hipFree(t->d_tap);
        t->d_tap = nullptr; t->tap_cap = 0;
        QPN_HIP(hipMalloc(&t->d_tap, ntap * sizeof(int)));
        t->tap_cap = ntap;
    }
    TrainBwd& bw = t->bw;
    float* const w = t->d_ws;
    p.X = a.at(w, TA_X); p.SG = a.at(w, TA_SG); p.TH = a.at(w, TA_TH); p.HUP = a.at(w, TA_HUP); p.S0 = a.at(w, TA_S0); p.Y0 = a.at(w, TA_Y0);
    bw.DXA[0] = a.at(w, TA_DXA); bw.DXB[0] = a.at(w, TA_DXB); bw.DXA[1] = bw.DXB[1] = nullptr;
    bw.DZ = a.at(w, TA_DZ); bw.DS0 = a.at(w, TA_DS0); bw.DY0 = a.at(w, TA_DY0); bw.DGS = a.at(w, TA_DGS); bw.DHUP = a.at(w, TA_DHUP); bw.slab = a.at(w, TA_SLAB);
    p.XC = (int*)a.at(w, TA_XC);
    p.scratch_rows = a.at(w, TA_SCRATCH);
    if (t->lay.use_gemm) t->gm.G = a.at(w, TA_G);
    p.PA = a.at(w, TA_PA); bw.DPA = a.at(w, TA_DPA); bw.EB = a.at(w, TA_EB); p.WJ = (float2*)a.at(w, TA_WJ); bw.GW = a.at(w, TA_GW);      // (null unless hoist)
    p.TAP = t->d_tap; p.status = t->d_status;
    t->report.call_on(stream);
    {   // stack work queues (train_stack.hip): a flag word per (layer, batch item, 16-row tile) and direction, compared with a per-forward epoch
        // (zeroed only when (re)allocated), and the tile tables k_train_prep writes.  The regions keep their places for the life of an
        // allocation (sized for 1.5x the positions that forced it): a table word of an earlier step must never be read as a flag
        if ((size_t)p.qtotal > t->sq_pos_cap) {
            if (t->d_sq) (void)hipFree(t->d_sq);
            t->d_sq = nullptr; t->sq_pos_cap = 0;
            const size_t cap = (size_t)p.qtotal + (size_t)p.qtotal / 2 + 64;
            const size_t per_dir = (cap / 32 + 2) * 1056;              // (sq_fidx: 32 flags per 128-byte line, lines 4224 bytes apart)
            const size_t nsq = TR_QHDR_WORDS + 2 * per_dir + 2 * (cap + 1) * 8;      // + two int4 per position and direction
            QPN_HIP(hipMalloc(&t->d_sq, nsq * sizeof(unsigned)));
            QPN_HIP(hipMemsetAsync(t->d_sq, 0, nsq * sizeof(unsigned), stream));
            t->sq_pos_cap = cap; t->sq_per_dir = per_dir;
        }
        // A step captured into a hipGraph replays its launches with the arguments of the capture: the queues' epoch -- a launch argument, a new one
        // per forward, which is what lets the flags go unzeroed -- would repeat, and every flag of the previous replay would read as published.
        // While the stream is capturing the stack therefore runs as a launch per layer.
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cap_st);
        const bool no_queue = t->report.stack_given_up() || cap_st != hipStreamCaptureStatusNone;
        p.qctl = no_queue ? nullptr : t->d_sq;                   // (nullptr: no queue launches, no tables)
        p.qtab = no_queue ? nullptr : (int4*)(t->d_sq + TR_QHDR_WORDS + 2 * t->sq_per_dir);
        p.qtab_b = no_queue ? nullptr : p.qtab + 2 * (t->sq_pos_cap + 1);
        const unsigned epoch = (unsigned)((t->generation + 1) % 0xFFFFFFFFll) + 1u;      // (generation is bumped below; never 0)
        StackQ& f = t->sqf; StackQ& bq = t->sqb;
        f.flags = t->d_sq + TR_QHDR_WORDS; f.head = t->d_sq + 1024; f.abort = t->d_sq + 1; f.stats = t->d_sq + 4; f.epoch = epoch; f.total = p.qtotal; f.tab = p.qtab;
        bq.flags = f.flags + t->sq_per_dir; bq.head = f.head + 8 * TR_QHEAD_STRIDE; bq.abort = f.abort; bq.stats = t->d_sq + 8; bq.epoch = epoch; bq.total = p.qtotal; bq.tab = p.qtab_b;
    }
    p.flat = d_flat; p.wp = (const float4*)t->d_wp; p.bp = t->d_bp; p.x = d_x; p.h = d_h; p.d = d_dfac; p.logits = d_logits;
    // ---- what this forward launches (train_launch_plan.h): the facts of the call, then the plan -- or a refusal, before anything is launched
    TrainFwdFacts ff;
    ff.cus = qpn_num_cus(); ff.queues_usable = p.qctl != nullptr; ff.flat_aligned16 = ((uintptr_t)d_flat & 15) == 0;
    ff.targets = d_targets != nullptr; ff.want_logits = want_logits != 0; ff.dlogits = d_dlogits != nullptr; ff.fuse_bwd = fuse_bwd;
    ff.soft_targets = d_teacher != nullptr; ff.loss_opts = lo_armed;
    t->fwd_valid = false;
    t->fplan = train_fwd_plan(g, t->lay, t->knobs, sh, ff);
    const TrainFwdPlan& fp = t->fplan;
    if (fp.rc) return fp.rc;
    // ---- refresh the fragment-ordered weights / packed biases from the current parameters: a launch of its own, or (fp.fuse_prep: tile path, causal table
    //      slices that fit; QPN_PREP_FUSE=0 switches it off) roles of the prep launch -- then nothing is launched here
    RefreshArgs rf;
    {
        const int* wmap = t->lay.use_gemm ? t->d_gmap : t->d_wmap;
        float* wout = t->lay.use_gemm ? t->d_gwp : t->d_wp;
        const int64_t nw = t->lay.n_map, nct = (int64_t)2 * g.Q * g.C;
        rf.wmap = wmap; rf.wout = wout; rf.nw = nw; rf.bstart = t->d_bstart; rf.blist = t->d_blist; rf.nb = t->lay.n_bias; rf.loss = t->d_loss;
        if (!fp.fuse_prep)
            hipLaunchKernelGGL(k_refresh, dim3(fp.refresh.gx), dim3(fp.refresh.block), 0, stream, d_flat, wmap, wout, nw, t->d_ctmap, t->d_ct, nct,
                               t->d_bstart, t->d_blist, t->d_bp, t->lay.n_bias, t->d_status, t->d_loss);
        p.ct = t->d_ct;
    }
    qpn_prof_mark(PG_PREP, stream);
    t->loss_clear = true;
    ++t->generation;
    const bool fuse_ce = fp.fuse_ce;
    p.ce_tgt = fuse_ce ? d_targets : nullptr; p.ce_stride = tgt_stride; p.ce_dlogits = d_dlogits; p.ce_loss = t->d_loss;
    if (!fp.store_logits) p.logits = nullptr;
    rc = t->lay.use_gemm ? qpn_launch_fwd_gemm(p, t->gm, stream) : qpn_launch_fwd(p, fp, t->ag, t->sqf, stream, t->bw, rf);
    t->post_bwd_dlogits = d_dlogits;
    p.ce_tgt = nullptr; p.logits = d_logits;
    if (rc) return rc;
    t->fwd_valid = true;
    if (fuse_ce) { t->loss_clear = false; qpn_prof_mark(PG_CE, stream); }
    else if (d_targets) {
        const CeOpts co = ce_opts_of(lo, nullptr, t->d_mass);
        const LossCall lc = {d_logits, d_teacher, d_targets, tgt_stride, B, BL, g.Q, ds_alpha, ds_temp, lo_armed ? &co : nullptr, d_dlogits, t->d_loss, nullptr, t->d_status, t->loss_clear};
        rc = qpn_launch_loss(lc, stream);
        if (rc) return rc;
        t->loss_clear = false;
    }
    return QPN_OK;
}

extern "C" int qpn_train_forward(qpn_handle* h, const float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                                 const int64_t* d_x, const float* d_h, const float* d_dfac, float* d_logits, void* stream_) {
    return train_forward_impl(h, d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_logits, nullptr, 0, nullptr, 1, stream_);
}

extern "C" int qpn_train_forward_loss(qpn_handle* h, const float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                                      const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                                      float* d_logits, int want_logits, float* d_dlogits, void* stream_) {
    if (!d_targets) { qpn_set_error("bad train_forward_loss arguments: no targets"); return QPN_EINVAL; }
    return train_forward_impl(h, d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_logits, d_targets, tgt_stride, d_dlogits, want_logits & 1, stream_, (want_logits & QPN_FWD_BACKWARD_FOLLOWS) != 0);
}

// alpha in (0, 1], temperature finite and > 0: the rules of both distillation entry points (checked without a device)
static int check_distill_args(const char* fn, float alpha, float temperature) {
    if (!(alpha > 0.f && alpha <= 1.f)) { qpn_set_error("%s: alpha must lie in (0, 1] (got %g)", fn, (double)alpha); return QPN_EINVAL; }
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e+38f)) { qpn_set_error("%s: temperature must be finite and > 0 (got %g)", fn, (double)temperature); return QPN_EINVAL; }
    return QPN_OK;
}

// The arm is host state on the handle (no device is needed to set it); the next forward that computes a loss takes it -- whatever that forward then returns
extern "C" int qpn_train_distill(qpn_handle* h, const float* d_teacher, int64_t n, float alpha, float temperature) {
    if (!h) { qpn_set_error("qpn_train_distill: null handle"); return QPN_EINVAL; }
    h->distill_t = nullptr; h->distill_n = 0;
    if (!d_teacher) return QPN_OK;
    if (n < 1) { qpn_set_error("qpn_train_distill: n must be >= 1 with teacher logits (got %lld)", (long long)n); return QPN_EINVAL; }
    int rc = check_distill_args("qpn_train_distill", alpha, temperature); if (rc) return rc;
    if ((uintptr_t)d_teacher & 15) { qpn_set_error("qpn_train_distill: d_teacher must be 16-byte aligned"); return QPN_EINVAL; }
    if (h->loss_opts_armed && h->loss_opts.label_smoothing > 0.f) { qpn_set_error("qpn_train_distill: a teacher cannot be combined with the armed label_smoothing (qpn_train_loss_opts; the soft targets already smooth)"); return QPN_EINVAL; }
    h->distill_t = d_teacher; h->distill_n = n; h->distill_alpha = alpha; h->distill_temp = temperature;
    return QPN_OK;
}

// ---- loss options (include/qpnet_hip.h: qpn_loss_opts).  The argument rules of all three entry points, checked without a device
static bool loss_opts_default(const qpn_loss_opts& o) { return !o.d_weights && !o.use_ignore && o.label_smoothing == 0.f && o.norm == 0; }
static int check_loss_opts(const char* fn, const qpn_loss_opts* o, bool with_teacher) {
    if (!o) { qpn_set_error("%s: opts is NULL", fn); return QPN_EINVAL; }
    if (o->d_weights && o->n_weights < 1) { qpn_set_error("%s: n_weights must be >= 1 with d_weights (got %lld)", fn, (long long)o->n_weights); return QPN_EINVAL; }
    if (!(o->label_smoothing >= 0.f && o->label_smoothing < 1.f)) { qpn_set_error("%s: label_smoothing must lie in [0, 1) (got %g)", fn, (double)o->label_smoothing); return QPN_EINVAL; }
    if (o->norm != 0 && o->norm != 1) { qpn_set_error("%s: norm must be 0 (rows) or 1 (weights) (got %d)", fn, o->norm); return QPN_EINVAL; }
    if ((uintptr_t)o->d_weights & 3) { qpn_set_error("%s: d_weights must be 4-byte aligned", fn); return QPN_EINVAL; }
    if (with_teacher && o->label_smoothing > 0.f) { qpn_set_error("%s: label_smoothing cannot be combined with a distillation teacher (the soft targets already smooth)", fn); return QPN_EINVAL; }
    return QPN_OK;
}
// the kernels' view of checked options: mass -- 64 slots (or nullptr); word -- where k_weight_mass writes what norm = 1 divides by (d_mass + 64)
static CeOpts ce_opts_of(const qpn_loss_opts& o, double* mass, double* d_mass) {
    return CeOpts{o.d_weights, (long long)o.ignore_index, o.use_ignore ? 1 : 0, o.label_smoothing, o.norm == 1 ? d_mass + 64 : nullptr, mass};
}
// The four stand-alone loss entry points below are this one function.  fn: the entry's name for its messages (nullptr: qpn_ce_loss, which has made its one
// terse check, behind need_dev / train_init); soft / with_opts: the entry takes a teacher / options.  Argument errors are reported before any device is needed.
// h_out (may be NULL: nothing is read back and the call does not synchronise): [0] the loss; soft: then the hard CE mean and T^2 KL; with_opts: then the
// effective sum of weights
static int loss_entry(const char* fn, qpn_handle* h, const float* d_logits, bool soft, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                      float alpha, float temperature, bool with_opts, const qpn_loss_opts* opts, float* d_dlogits, double* h_out, void* stream_) {
    int rc;
    if (fn) {
        if (!h) { qpn_set_error("%s: null handle", fn); return QPN_EINVAL; }
        if (!d_logits) { qpn_set_error("%s: d_logits is NULL", fn); return QPN_EINVAL; }
        if (soft && !d_teacher) { qpn_set_error("%s: d_teacher is NULL", fn); return QPN_EINVAL; }
        if (!d_targets) { qpn_set_error("%s: d_targets is NULL", fn); return QPN_EINVAL; }
        if (B < 1) { qpn_set_error("%s: B must be >= 1 (got %d)", fn, B); return QPN_EINVAL; }
        if (BL < 1) { qpn_set_error("%s: BL must be >= 1 (got %d)", fn, BL); return QPN_EINVAL; }
        if (tgt_stride < BL) { qpn_set_error("%s: tgt_stride (%lld) is shorter than BL (%d)", fn, (long long)tgt_stride, BL); return QPN_EINVAL; }
        if (soft) { rc = check_distill_args(fn, alpha, temperature); if (rc) return rc; }
        if (with_opts) {
            rc = check_loss_opts(fn, opts, soft); if (rc) return rc;
            if (opts->d_weights && opts->n_weights != (int64_t)B * BL) { qpn_set_error("%s: n_weights = %lld, the call has B * BL = %d * %d = %lld rows", fn, (long long)opts->n_weights, B, BL, (long long)B * BL); return QPN_EINVAL; }
        }
        if (h->g.Q % 256 == 0 && ((((uintptr_t)d_logits) | (soft ? (uintptr_t)d_teacher : 0) | ((uintptr_t)d_dlogits)) & 15)) {
            qpn_set_error(soft ? "%s: d_logits, d_teacher and d_dlogits must be 16-byte aligned" : "%s: d_logits and d_dlogits must be 16-byte aligned", fn); return QPN_EINVAL;
        }
    }
    rc = need_dev(h); if (rc) return rc;
    rc = train_init(h); if (rc) return rc;
    TrainState* t = h->train;
    hipStream_t stream = (hipStream_t)stream_;
    if (with_opts && !t->d_mass) QPN_HIP(hipMalloc(&t->d_mass, 72 * sizeof(double)));
    if (soft && h_out && !t->d_loss3) QPN_HIP(hipMalloc(&t->d_loss3, 128 * sizeof(double)));
    const CeOpts co = with_opts ? ce_opts_of(*opts, h_out ? t->d_mass : nullptr, t->d_mass) : CeOpts{};
    const LossCall lc = {d_logits, soft ? d_teacher : nullptr, d_targets, tgt_stride, B, BL, h->g.Q, alpha, temperature, with_opts ? &co : nullptr,
                         d_dlogits, t->d_loss, soft && h_out ? t->d_loss3 : nullptr, t->d_status, t->loss_clear};
    rc = qpn_launch_loss(lc, stream); if (rc) return rc;
    t->loss_clear = false;
    if (h_out) {
        double parts[64], comp[128], mass[64];
        QPN_HIP(hipMemcpyAsync(parts, t->d_loss, sizeof(parts), hipMemcpyDeviceToHost, stream));
        if (soft) QPN_HIP(hipMemcpyAsync(comp, t->d_loss3, sizeof(comp), hipMemcpyDeviceToHost, stream));
        if (with_opts) QPN_HIP(hipMemcpyAsync(mass, t->d_mass, sizeof(mass), hipMemcpyDeviceToHost, stream));
        QPN_HIP(hipStreamSynchronize(stream));
        *h_out++ = loss_sum(parts);
        if (soft) { *h_out++ = loss_sum(comp); *h_out++ = (double)temperature * (double)temperature * loss_sum(comp + 64); }
        if (with_opts) *h_out++ = loss_sum(mass);
    }
    return QPN_OK;
}

extern "C" int qpn_ce_loss(qpn_handle* h, const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                           float* d_dlogits, double* h_loss, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    rc = train_init(h); if (rc) return rc;
    if (!d_logits || !d_targets || B < 1 || BL < 1 || tgt_stride < BL) { qpn_set_error("bad ce_loss arguments"); return QPN_EINVAL; }
    return loss_entry(nullptr, h, d_logits, false, nullptr, d_targets, tgt_stride, B, BL, 0.f, 0.f, false, nullptr, d_dlogits, h_loss, stream_);
}
extern "C" int qpn_distill_loss(qpn_handle* h, const float* d_logits, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                                float alpha, float temperature, float* d_dlogits, double* h_loss3, void* stream_) {
    return loss_entry("qpn_distill_loss", h, d_logits, true, d_teacher, d_targets, tgt_stride, B, BL, alpha, temperature, false, nullptr, d_dlogits, h_loss3, stream_);
}
extern "C" int qpn_ce_loss_opts(qpn_handle* h, const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                                const qpn_loss_opts* opts, float* d_dlogits, double* h_loss2, void* stream_) {
    return loss_entry("qpn_ce_loss_opts", h, d_logits, false, nullptr, d_targets, tgt_stride, B, BL, 0.f, 0.f, true, opts, d_dlogits, h_loss2, stream_);
}
extern "C" int qpn_distill_loss_opts(qpn_handle* h, const float* d_logits, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                                     float alpha, float temperature, const qpn_loss_opts* opts, float* d_dlogits, double* h_loss4, void* stream_) {
    return loss_entry("qpn_distill_loss_opts", h, d_logits, true, d_teacher, d_targets, tgt_stride, B, BL, alpha, temperature, true, opts, d_dlogits, h_loss4, stream_);
}

// The arm is host state on the handle, as qpn_train_distill's is.  An options struct that is entirely default arms nothing: the next forward launches what it always launched
extern "C" int qpn_train_loss_opts(qpn_handle* h, const qpn_loss_opts* opts) {
    if (!h) { qpn_set_error("qpn_train_loss_opts: null handle"); return QPN_EINVAL; }
    h->loss_opts_armed = false;
    if (!opts) return QPN_OK;
    int rc = check_loss_opts("qpn_train_loss_opts", opts, h->distill_t != nullptr); if (rc) return rc;
    if (loss_opts_default(*opts)) return QPN_OK;
    h->loss_opts = *opts; h->loss_opts_armed = true;
    return QPN_OK;
}

// dev / diagnostics: the control words of the stack work queues as the last step left them (synchronises the stream)
extern "C" int qpn_train_stack_stats(qpn_handle* h, unsigned* h_out, int n, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train || !h->train->d_sq || !h_out || n < 1) { qpn_set_error("no stack-queue launch yet"); return QPN_ESTATE; }
    QPN_HIP(hipStreamSynchronize((hipStream_t)stream_));
    QPN_HIP(hipMemcpy(h_out, h->train->d_sq, sizeof(unsigned) * (size_t)(n < 1024 ? n : 1024), hipMemcpyDeviceToHost));      // (words 600.. : stamps of a -DQPN_STACK_STAMPS build)
    return QPN_OK;
}

#ifdef QPN_TESTING
// test hook (a -DQPN_TESTING build only; tests/f64_child.py): the rectified post-net activations relu(s0), relu(y0) of the last forward ([B][BL][S] floats each) --
// their signs are the ReLU sides this forward took, which a float64 yardstick of the gradient must be given (a unit within rounding of zero falls on either side)
extern "C" int qpn_test_postnet_activations(qpn_handle* h, float* d_s0, float* d_y0, int64_t n, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train || !h->train->fwd_valid || !d_s0 || !d_y0) { qpn_set_error("no forward to read"); return QPN_ESTATE; }
    const TrainParams& p = h->train->tp;
    if (n != (int64_t)p.B * p.BL * p.S) { qpn_set_error("postnet_activations: n != B * BL * S"); return QPN_EINVAL; }
    QPN_HIP(hipMemcpyAsync(d_s0, p.S0, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    QPN_HIP(hipMemcpyAsync(d_y0, p.Y0, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    return QPN_OK;
}
#endif

extern "C" int64_t qpn_train_generation(qpn_handle* h) { return (h && h->train) ? h->train->generation : 0; }

extern "C" int qpn_train_backward(qpn_handle* h, const float* d_dlogits, float* d_flatgrad, void* stream_) {
    return qpn_train_backward_ex(h, d_dlogits, d_flatgrad, 1.0f, 0, stream_);
}

// The arm is host state on the handle (no device is needed to set it); the next backward takes it -- whatever that backward then returns
extern "C" int qpn_train_input_grad(qpn_handle* h, float* d_dh, int64_t n) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (d_dh && n < 1) { qpn_set_error("qpn_train_input_grad: n must be >= 1 with a destination (got %lld)", (long long)n); h->in_grad = nullptr; h->in_grad_n = 0; return QPN_EINVAL; }
    h->in_grad = d_dh; h->in_grad_n = d_dh ? n : 0;
    return QPN_OK;
}

extern "C" int qpn_train_backward_ex(qpn_handle* h, const float* d_dlogits, float* d_flatgrad, float grad_scale, int append_scale, void* stream_) {
    float* d_dh = nullptr; int64_t dh_n = 0;
    if (h) { d_dh = h->in_grad; dh_n = h->in_grad_n; h->in_grad = nullptr; h->in_grad_n = 0; }      // one shot: consumed here, also by a backward that fails below
    int rc = need_dev(h); if (rc) return rc;
    if (!h->train || !h->train->fwd_valid) { qpn_set_error("qpn_train_backward needs a preceding qpn_train_forward"); return QPN_ESTATE; }
    if (!d_dlogits || !d_flatgrad) { qpn_set_error("bad train_backward arguments"); return QPN_EINVAL; }
    TrainState* t = h->train;
    TrainBwd& bw = t->bw;
    bw.dh = nullptr;
    if (d_dh) {
        const int64_t want = (int64_t)t->tp.B * h->g.A * t->tp.F;
        if (dh_n != want) {
            qpn_set_error("qpn_train_input_grad: n = %lld, the forward of this backward has B * n_aux * F = %d * %d * %d = %lld", (long long)dh_n, t->tp.B, h->g.A, t->tp.F, (long long)want);
            return QPN_EINVAL;
        }
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing((hipStream_t)stream_, &cap_st);
        if (cap_st != hipStreamCaptureStatusNone) { qpn_set_error("qpn_train_input_grad: an armed backward cannot be captured (the arm is host state a replay would not renew)"); return QPN_ESTATE; }
        bw.dh = d_dh;
    }
    bw.dlogits = d_dlogits; bw.gflat = d_flatgrad; bw.gdst = t->d_gdst; bw.gdst_list = t->d_gdst_list; bw.gzero = t->d_gzero; bw.n_gzero = t->lay.n_gzero;
    bw.gscale = grad_scale; bw.append_scale = append_scale; bw.status = h->train->d_status;
    bw.side = t->side; bw.ev_fork = t->ev_fork; bw.ev_join = t->ev_join; bw.ev_mid = t->ev_mid;
    t->early_recorded = 0; bw.ev_early = t->ev_early; bw.early_recorded = (append_scale && t->lay.early_first >= 0) ? &t->early_recorded : nullptr;
    // ---- what this backward launches (train_launch_plan.h).  The backward queue's heads and flags belong to ONE backward per forward: a repeated backward of
    //      the same forward runs a launch per layer, and its own post-net backward
    TrainBwdFacts bf;
    bf.cus = qpn_num_cus(); bf.side_stream = t->side != nullptr; bf.prof_serial = qpn_prof_serial(); bf.gdst = t->d_gdst != nullptr; bf.append_scale = append_scale;
    bf.feature_grad = bw.dh != nullptr; bf.first_bwd = t->bwd_generation != t->generation; bf.same_dlogits = d_dlogits == t->post_bwd_dlogits;
    t->bwd_generation = t->generation;
    t->bplan = train_bwd_plan(h->g, t->lay, t->knobs, t->shape, t->fplan, bf);
    if (t->bplan.rc) return t->bplan.rc;
    return t->lay.use_gemm ? qpn_launch_bwd_gemm(t->tp, bw, t->gm, (hipStream_t)stream_) : qpn_launch_bwd(t->tp, bw, t->bplan, t->ag, t->sqb, (hipStream_t)stream_);
}

// The forward's and the backward's plan of the handle's latest training calls as one line of text each (train_launch_plan.h: plan_text), "fwd[...] ... | bwd[...] ...".
// Formatted here, on request: a step formats nothing.  The handle owns the text; it is valid until the next training call
extern "C" const char* qpn_train_last_plan(qpn_handle* h) {
    if (!h || !h->train) return "";
    TrainState* t = h->train;
    t->plan_text = t->generation > 0 ? plan_text(h->g, t->lay, t->shape, t->fplan) : std::string();
    if (t->bwd_generation == t->generation && t->generation > 0) t->plan_text += " | " + plan_text(h->g, t->lay, t->shape, t->bplan);
    return t->plan_text.c_str();
}

extern "C" int qpn_train_early_bucket(qpn_handle* h, int64_t* first, int64_t* count, void* stream_) {
    int rc = need_dev(h); if (rc) return rc;
    if (!first || !count) { qpn_set_error("bad early_bucket arguments"); return QPN_EINVAL; }
    *first = 0; *count = 0;
    TrainState* t = h->train;
    if (!t || !t->early_recorded) return QPN_OK;            // this backward finished nothing early (one stream, no upsampling kernel, a plain backward): one exchange
    *first = t->lay.early_first; *count = t->bw.n_params - t->lay.early_first + 4;
    QPN_HIP(hipStreamWaitEvent((hipStream_t)stream_, t->ev_early, 0));
    return QPN_OK;
}

// first element of the flat-gradient tail that a backward finishes early (the post-net blocks; the 4-float trailer follows them), or -1: a
// property of the model's parameter layout, known once the handle has trained a step -- what data-parallel ranks agree on before they split the exchange
extern "C" int64_t qpn_train_early_first(qpn_handle* h) { return (h && h->train && h->device >= 0) ? h->train->lay.early_first : -1; }

extern "C" int qpn_adam_step(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                             int step, float lr, float beta1, float beta2, float eps, float weight_decay, void* stream_) {
    return qpn_adam_step_ex(h, d_flat, d_grad, d_m, d_v, n, step, lr, beta1, beta2, eps, weight_decay, nullptr, stream_);
}

extern "C" int qpn_adam_step_ex(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                                int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                const float* d_grad_denominator, void* stream_) {
    return qpn_adam_step_clip(h, d_flat, d_grad, d_m, d_v, n, step, lr, beta1, beta2, eps, weight_decay, d_grad_denominator, 0.0f, stream_);
}

extern "C" int qpn_adam_step_clip(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                                  int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  const float* d_grad_denominator, float max_grad_norm, void* stream_) {
    return qpn_adam_step_avg(h, d_flat, d_grad, d_m, d_v, n, step, lr, beta1, beta2, eps, weight_decay, d_grad_denominator, max_grad_norm, nullptr, 0.0f, stream_);
}

// the averaged-weights arguments of the _avg calls: both absent (NULL, 0: averaging off), or n caller-owned floats and 0 < decay < 1.  Checked before anything
// about the device or the handle's state.  *omd = 1 - decay, formed once, in fp32: the factor every thread multiplies by
static int check_ema_args(const float* d_ema, float ema_decay, float* omd) {
    *omd = 0.0f;
    if (ema_decay != ema_decay) { qpn_set_error("ema_decay is NaN"); return QPN_EINVAL; }
    if (!d_ema && ema_decay == 0.0f) return QPN_OK;
    if (!d_ema) { qpn_set_error("ema_decay is set but d_ema is NULL (averaging off is d_ema = NULL with ema_decay = 0)"); return QPN_EINVAL; }
    if (!(ema_decay > 0.0f && ema_decay < 1.0f)) { qpn_set_error("ema_decay must lie in (0, 1) when d_ema is given (averaging off is d_ema = NULL with ema_decay = 0)"); return QPN_EINVAL; }
    *omd = 1.0f - ema_decay;
    return QPN_OK;
}

// ---- parameter groups (adam_groups.h).  Sticky on the handle, like qpn_decode_sampling: from the call on EVERY Adam launch of the handle (qpn_adam_step*, qpn_train_step*,
// the closing micro-step of qpn_train_step_acc) takes lr / weight_decay per element from the table and leaves frozen elements alone; the launch's own two values
// are ignored.  The caller's arrays are not referenced after return.  A table equal (after merging neighbours of one group) to the one the handle holds only
// replaces the group values -- no device work: the per-step path of a learning-rate schedule.  A new table is a set-up call: it waits for `stream` (the launches
// that read the old table) and uploads; not while that stream is capturing.  n_groups = 0: off, nothing else is looked at, no device is needed.
extern "C" int qpn_adam_groups(qpn_handle* h, int n_groups, const float* h_lr, const float* h_weight_decay,
                               int64_t n_seg, const int64_t* h_seg_end, const int32_t* h_seg_group, void* stream_) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (n_groups < 0 || n_groups > QPN_ADAM_MAX_GROUPS) { qpn_set_error("bad adam_groups arguments: n_groups must lie in [0, %d] (got %d)", QPN_ADAM_MAX_GROUPS, n_groups); return QPN_EINVAL; }
    if (n_groups == 0) { h->adam_n_groups = 0; return QPN_OK; }
    char why[256];
    if (!adam_groups_check(n_groups, h_lr, h_weight_decay, n_seg, h_seg_end, h_seg_group, why, sizeof(why))) { qpn_set_error("bad adam_groups arguments: %s", why); return QPN_EINVAL; }
    int rc = need_dev(h); if (rc) return rc;
    if (!h->d_adam_table || !adam_groups_normalise(n_seg, h_seg_end, h_seg_group).same_segments(h->adam_table)) {
        AdamGroupTable t = adam_groups_build(n_seg, h_seg_end, h_seg_group);
        hipStream_t stream = (hipStream_t)stream_;
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cap_st);
        if (cap_st != hipStreamCaptureStatusNone) { qpn_set_error("qpn_adam_groups with a new segment table while the stream is capturing (set the table before the capture)"); return QPN_ESTATE; }
        const size_t ns = t.seg_end.size(), nb = t.block.size();                  // [seg_end | block pairs | seg_group]: the 8-byte entries first
        const size_t bytes = ns * sizeof(int64_t) + (ns + nb) * sizeof(int32_t);
        char* d_new = nullptr;
        QPN_HIP(hipStreamSynchronize(stream));
        QPN_HIP(hipMalloc(&d_new, bytes));
        hipError_t e = hipMemcpy(d_new, t.seg_end.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_new + ns * sizeof(int64_t), t.block.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_new + ns * sizeof(int64_t) + nb * sizeof(int32_t), t.seg_group.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d_new); QPN_HIP(e); }
        h->adam_n_groups = 0;                                    // (between the two tables the handle has none)
        if (h->d_adam_table) (void)hipFree(h->d_adam_table);
        h->d_adam_table = d_new;
        h->adam_table = std::move(t);
    }
    for (int q = 0; q < QPN_ADAM_MAX_GROUPS; ++q) { h->adam_lr[q] = q < n_groups ? h_lr[q] : 0.0f; h->adam_wd[q] = q < n_groups ? h_weight_decay[q] : 0.0f; }
    h->adam_n_groups = n_groups;
    return QPN_OK;
}

// the groups of an Adam launch over n elements: *use = false with groups off; QPN_EINVAL when the table covers another n
static int adam_groups_arg(const qpn_handle* h, int64_t n, AdamGroupsArg* a, bool* use) {
    *use = h->adam_n_groups > 0;
    if (!*use) return QPN_OK;
    const AdamGroupTable& t = h->adam_table;
    if (n != t.n) { qpn_set_error("bad adam_step arguments: n = %lld, the handle's parameter groups (qpn_adam_groups) cover %lld elements", (long long)n, (long long)t.n); return QPN_EINVAL; }
    const size_t ns = t.seg_end.size();
    a->seg_end = reinterpret_cast<const long long*>(h->d_adam_table);
    a->block = reinterpret_cast<const int*>(h->d_adam_table + ns * sizeof(int64_t));
    a->seg_group = a->block + t.block.size();
    for (int q = 0; q < QPN_ADAM_MAX_GROUPS; ++q) { a->lr[q] = h->adam_lr[q]; a->wd[q] = h->adam_wd[q]; }
    return QPN_OK;
}

// max_grad_norm > 0: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) in front of the update (k_grad_sumsq + k_adam<true, ..>); otherwise exactly the launch qpn_adam_step_ex always made.
// d_ema: the averaged weights move with every APPLIED update, inside the same launch (k_adam<.., true, ..>); NULL with ema_decay 0: the instances without it
extern "C" int qpn_adam_step_avg(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                                 int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 const float* d_grad_denominator, float max_grad_norm, float* d_ema, float ema_decay, void* stream_) {
    float omd;
    int rc = check_ema_args(d_ema, ema_decay, &omd); if (rc) return rc;
    rc = need_dev(h); if (rc) return rc;
    if (!d_flat || !d_grad || !d_m || !d_v || n < 1 || step < 1 || max_grad_norm != max_grad_norm) { qpn_set_error("bad adam_step arguments"); return QPN_EINVAL; }
    AdamGroupsArg ga; bool grouped;
    rc = adam_groups_arg(h, n, &ga, &grouped); if (rc) return rc;
    const bool clip = max_grad_norm > 0.f;
    if (clip) { rc = train_init(h); if (rc) return rc; }                 // (the partial sums and the norm word live in the training state)
    TrainState* const t = h->train;
    if (t) t->report.call_on((hipStream_t)stream_, clip ? StepEnd::AdamClipped : StepEnd::AdamPlain);
    const AdamCall c = {d_flat, d_grad, d_m, d_v, n, step, lr, beta1, beta2, eps, weight_decay, d_grad_denominator, t ? t->d_status : nullptr, nullptr, nullptr, nullptr,
                        max_grad_norm, clip ? t->d_gnorm : nullptr, clip ? t->d_loss + LOSS_NORM_AT : nullptr, nullptr, d_ema, omd, grouped ? &ga : nullptr};
    return qpn_launch_adam(c, (hipStream_t)stream_);
}

// Gradient accumulation: d_acc <- first ? d_grad : d_acc + d_grad over cnt floats (k_grad_accum; callers pass n + 4: the row-weighted gradient qpn_train_backward_ex
// left and its trailer).  first overwrites: d_acc needs no clearing.  The arguments are checked before anything about the device
extern "C" int qpn_grad_accumulate(qpn_handle* h, float* d_acc, const float* d_grad, int64_t cnt, int first, void* stream_) {
    if (!d_acc) { qpn_set_error("bad grad_accumulate arguments: d_acc is NULL"); return QPN_EINVAL; }
    if (!d_grad) { qpn_set_error("bad grad_accumulate arguments: d_grad is NULL"); return QPN_EINVAL; }
    if (cnt < 1) { qpn_set_error("bad grad_accumulate arguments: cnt must be >= 1"); return QPN_EINVAL; }
    if (d_acc == d_grad) { qpn_set_error("bad grad_accumulate arguments: d_acc is d_grad (the accumulator must be a buffer of its own)"); return QPN_EINVAL; }
    int rc = need_dev(h); if (rc) return rc;
    // (a step that ends here ran no Adam launch: the norm word is not this step's -- qpn_train_loss_enqueue / qpn_train_grad_norm report "did not clip")
    if (h->train) h->train->report.call_on((hipStream_t)stream_, StepEnd::NoAdam);
    return qpn_launch_grad_accum(d_acc, d_grad, cnt, first, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

// One optimisation step behind ONE call -- what a training loop's body is (reference src/bin/qpnet_train.py:517-531: forward, CrossEntropyLoss, backward,
// Adam.step, loss.item()): the calls FusedTrainer.step used to make one by one, in their order.  The host side of a step is then a single foreign call
// (a Python caller's other threads -- the loader -- run while it is in progress) instead of seven with interpreter work between them.
//   loss_mode 0: no loss;  1 "lagged": this step's loss is copied out behind its kernels and *h_loss receives the PREVIOUS step's (*h_valid = 0 at the first
//   step or right behind a flush: qpn_train_loss_collect(newest = 1) fetches the last one), the stream is never drained;  2: this step's loss, read in the call
//   (drains the stream, as the reference's loss.item() does).
// The device-side status word is handled as FusedTrainer.step documents: collected two steps late at most (mode 0 / 1), in the call (mode 2).
// The arguments of a step, in the order of the widest entry point (qpn_train_step_acc); the narrower ones leave the tail at "off":
// max_grad_norm > 0: the step clips (qpn_adam_step_clip), and *h_grad_norm (may be NULL) receives the norm of the step whose loss *h_loss is -- mode 1: the previous
// step's, out of the same pinned slot as its loss; mode 2: this step's; mode 0: none.  0 where that step did not clip.
// d_ema / ema_decay: qpn_adam_step_avg's (every loss mode moves the average: it is the Adam launch's own work).
// d_acc != NULL: micro-step `micro` of a window of micro_count > 1 chunks (qpn_train_step_acc); NULL: the plain step, launch for launch what it always was
struct TrainStepArgs {
    float* d_flat; int B; int64_t T, F, Td; int BL, maxd;
    const int64_t* d_x; const float* d_h; const float* d_dfac; const int64_t* d_targets; int64_t tgt_stride;
    float* d_logits; float* d_dlogits; float* d_grad; float* d_m; float* d_v; int64_t n;
    int step; float lr, beta1, beta2, eps, weight_decay;
    int loss_mode; double* h_loss; int* h_valid; float max_grad_norm; double* h_grad_norm;
    float* d_ema; float ema_decay; float* d_acc; int micro, micro_count; void* stream;
};

static int train_step_body(qpn_handle* h, const TrainStepArgs& a) {
    if (a.h_valid) *a.h_valid = 0;
    if (a.h_loss) *a.h_loss = 0.0;
    if (a.h_grad_norm) *a.h_grad_norm = 0.0;
    float omd;
    int rc = check_ema_args(a.d_ema, a.ema_decay, &omd); if (rc) return rc;
    const int loss_mode = a.loss_mode;
    if (loss_mode < 0 || loss_mode > 2 || (loss_mode && (!a.h_loss || !a.h_valid)) || a.max_grad_norm != a.max_grad_norm) { qpn_set_error("bad train_step arguments"); return QPN_EINVAL; }
    const bool accum = a.d_acc != nullptr;                               // a window of several chunks: the gradient goes through the accumulator ...
    const bool closing = a.micro == a.micro_count - 1;                   // ... and only its last micro-step has an Adam launch
    const bool clip = closing && a.max_grad_norm > 0.f;
    rc = need_dev(h); if (rc) return rc;
    AdamGroupsArg ga; bool grouped = false;
    if (closing) { rc = adam_groups_arg(h, a.n, &ga, &grouped); if (rc) return rc; }      // (before anything is enqueued: a table for another n fails the whole step)
    const hipStream_t stream = (hipStream_t)a.stream;
    if (h->train) h->train->report.call_on(stream);                      // (a flagged word found here is cleared on THIS call's stream: train_report.h)
    rc = qpn_train_status_collect_lagged(h); if (rc) return rc;          // the check of the step before the previous one (never waits for queued work)
    if (!a.d_targets || !a.d_dlogits) { qpn_set_error("qpn_train_forward_loss needs targets and a dlogits buffer"); return QPN_EINVAL; }
    if (accum && (!a.d_grad || a.n < 1)) { qpn_set_error("bad train_step arguments: d_grad / n"); return QPN_EINVAL; }
    rc = train_forward_impl(h, a.d_flat, a.B, a.T, a.F, a.Td, a.BL, a.maxd, a.d_x, a.d_h, a.d_dfac, a.d_logits, a.d_targets, a.tgt_stride, a.d_dlogits, 0, a.stream, true); if (rc) return rc;
    // accumulating: d_grad <- n_r * g_r with the trailer {n_r, flagged_r, 0, 0} behind it, exactly what a data-parallel rank hands to the exchange -- the window is that
    // sum taken over time; Adam then reads the accumulator and divides by its trailer (a flag in it skips the update, as a peer rank's does)
    rc = accum ? qpn_train_backward_ex(h, a.d_dlogits, a.d_grad, (float)((int64_t)a.B * a.BL), 1, a.stream) : qpn_train_backward(h, a.d_dlogits, a.d_grad, a.stream); if (rc) return rc;
    TrainState* t = h->train;
    const float* const g_adam = accum ? a.d_acc : a.d_grad;
    const float* const den = accum ? a.d_acc + a.n : nullptr;
    if (loss_mode == 2) {
        if (accum) { rc = qpn_launch_grad_accum(a.d_acc, a.d_grad, a.n + 4, a.micro == 0, nullptr, nullptr, nullptr, nullptr, stream); if (rc) return rc; }
        if (closing) { rc = qpn_adam_step_avg(h, a.d_flat, g_adam, a.d_m, a.d_v, a.n, a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, den, a.max_grad_norm, a.d_ema, a.ema_decay, a.stream); if (rc) return rc; }
        else t->report.call_on(stream, StepEnd::NoAdam);                                              // (this micro-step has no norm)
        rc = qpn_train_loss(h, a.h_loss, a.stream); if (rc) return rc;
        *a.h_valid = 1;
        if (clip && a.h_grad_norm) { int nv = 0; rc = qpn_train_grad_norm(h, a.h_grad_norm, &nv, a.stream); if (rc) return rc; }      // (the stream has just been drained)
        return qpn_train_status(h, a.stream);
    }
    // modes 0 / 1: the step's last kernel writes the status word (and the loss partials, and the norm) into the pinned report slots itself (train_state.h)
    if (!a.d_flat || !a.d_grad || !a.d_m || !a.d_v || a.n < 1 || a.step < 1) { qpn_set_error("bad adam_step arguments"); return QPN_EINVAL; }
    ReportSlots rs;
    rc = qpn_report_open(t, loss_mode == 1, clip ? StepEnd::AdamClipped : closing ? StepEnd::AdamPlain : StepEnd::NoAdam, stream, &rs); if (rc) return rc;
    // (the micro-steps in front of the closing one end in the accumulate kernel: it carries the reports; in the closing one the Adam launch does, as ever)
    if (accum) { rc = qpn_launch_grad_accum(a.d_acc, a.d_grad, a.n + 4, a.micro == 0, closing ? nullptr : t->d_status, rs.h_status,
                                            rs.h_loss, (!closing && loss_mode == 1) ? t->d_loss : nullptr, stream); if (rc) return rc; }
    if (closing) {
        const AdamCall c = {a.d_flat, g_adam, a.d_m, a.d_v, a.n, a.step, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, den, t->d_status,
                            rs.h_status, rs.h_loss, loss_mode == 1 ? t->d_loss : nullptr,
                            a.max_grad_norm, t->d_gnorm, t->d_loss + LOSS_NORM_AT, rs.h_norm, a.d_ema, omd, grouped ? &ga : nullptr};
        rc = qpn_launch_adam(c, stream); if (rc) return rc;
    }
    rc = qpn_report_close(t, rs, stream); if (rc) return rc;
    if (loss_mode == 1) {
        rc = qpn_train_loss_collect(h, 0, a.h_loss, a.h_valid); if (rc) return rc;
        if (a.h_grad_norm) { int nv = 0; rc = qpn_train_grad_norm_lagged(h, a.h_grad_norm, &nv); if (rc) return rc; }      // (the norm that left the device in that loss's slot)
    }
    return QPN_OK;
}

// (a step that fails in front of its backward has no backward to consume an armed feature gradient: the arm is dropped with it)
static int train_step_impl(qpn_handle* h, const TrainStepArgs& a) {
    const int rc = train_step_body(h, a);
    if (rc && h) { h->in_grad = nullptr; h->in_grad_n = 0; h->distill_t = nullptr; h->distill_n = 0; h->loss_opts_armed = false; }      // (... and no forward to consume a soft-target or loss-options arm)
    return rc;
}

extern "C" int qpn_train_step(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                              const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                              float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                              int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                              int loss_mode, double* h_loss, int* h_valid, void* stream) {
    return train_step_impl(h, {d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_targets, tgt_stride, d_logits, d_dlogits, d_grad, d_m, d_v, n,
                               step, lr, beta1, beta2, eps, weight_decay, loss_mode, h_loss, h_valid, 0.0f, nullptr, nullptr, 0.0f, nullptr, 0, 1, stream});
}

extern "C" int qpn_train_step_clip(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                                   const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                                   float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                                   int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm, void* stream) {
    return train_step_impl(h, {d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_targets, tgt_stride, d_logits, d_dlogits, d_grad, d_m, d_v, n,
                               step, lr, beta1, beta2, eps, weight_decay, loss_mode, h_loss, h_valid, max_grad_norm, h_grad_norm, nullptr, 0.0f, nullptr, 0, 1, stream});
}

extern "C" int qpn_train_step_avg(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                                  const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                                  float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                                  int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm,
                                  float* d_ema, float ema_decay, void* stream) {
    return train_step_impl(h, {d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_targets, tgt_stride, d_logits, d_dlogits, d_grad, d_m, d_v, n,
                               step, lr, beta1, beta2, eps, weight_decay, loss_mode, h_loss, h_valid, max_grad_norm, h_grad_norm, d_ema, ema_decay, nullptr, 0, 1, stream});
}

// Gradient accumulation: the step above as micro-step `micro` of a window of micro_count chunks.  Every micro-step runs forward + loss, the row-weighted backward
// (qpn_train_backward_ex(B * BL, 1) into d_grad) and k_grad_accum into d_acc (micro 0 overwrites it); the last one also runs the Adam launch on d_acc, divided by the summed
// row count in its trailer.  The host side of a micro-step stays ONE foreign call, and a micro-step in front of the last ends in the accumulate kernel, whose block 0
// carries the status word and the loss partials to pinned memory as the Adam kernel does elsewhere: no copy-engine launch is added.
// The window's own arguments are checked first, then the averaged-weights ones, then the rest -- all before the device or the handle's state is looked at.
extern "C" int qpn_train_step_acc(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                                  const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                                  float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                                  int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm,
                                  float* d_ema, float ema_decay, float* d_acc, int micro, int micro_count, void* stream) {
    if (h_valid) *h_valid = 0;
    if (h_loss) *h_loss = 0.0;
    if (h_grad_norm) *h_grad_norm = 0.0;
    if (micro_count < 1) { qpn_set_error("bad train_step_acc arguments: micro_count must be >= 1"); return QPN_EINVAL; }
    if (micro < 0 || micro >= micro_count) { qpn_set_error("bad train_step_acc arguments: micro must lie in [0, micro_count)"); return QPN_EINVAL; }
    if (!d_acc && micro_count > 1) { qpn_set_error("bad train_step_acc arguments: d_acc is NULL with micro_count > 1"); return QPN_EINVAL; }
    if (d_acc && d_acc == d_grad) { qpn_set_error("bad train_step_acc arguments: d_acc is d_grad (the accumulator must be a buffer of its own)"); return QPN_EINVAL; }
    return train_step_impl(h, {d_flat, B, T, F, Td, BL, maxd, d_x, d_h, d_dfac, d_targets, tgt_stride, d_logits, d_dlogits, d_grad, d_m, d_v, n,
                               step, lr, beta1, beta2, eps, weight_decay, loss_mode, h_loss, h_valid, max_grad_norm, h_grad_norm, d_ema, ema_decay,
                               micro_count > 1 ? d_acc : nullptr, micro, micro_count, stream});
}
