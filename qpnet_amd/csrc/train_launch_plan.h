// train_launch_plan.h -- what a training step launches: the shape of a call, the forward's plan and the backward's plan.
// Pure host arithmetic (plain C++: no HIP, no handle, no globals, no getenv): train_host.hip gathers the facts of a call, asks here and hands the plans to the
// launchers of train_fwd.hip / train_bwd.hip / train_stack.hip, which carry them out in order and decide nothing.  tests/train_launch_plan_sweep.cpp checks the
// invariants on a CPU.  Every condition is stated ONCE: the forward and the backward read the same tlp_persist_* / tlp_stack_*_fits / tlp_post_wide_* here.
// (The GEMM step, lay.use_gemm, is only reported: train_gemm.hip keeps its own launchers.)
#pragma once
#include "qpn_geom.h"
#include "train_plan.h"
#include <stdio.h>
#include <string>

#ifdef __HIPCC__
#define TLP_HD __host__ __device__
#else
#define TLP_HD
#endif

// ---- the constants the arithmetic needs (the kernels read them from here)
#ifndef X0_CS
#define X0_CS 16          // k_step_prep: channels of a causal-table slice
#define X0_ST 17          //              row stride of the slice's table in LDS
#endif
#define X0_RPG 512        //              rows of a table workgroup at most
#define AUXP_FPB 8        // k_aux_proj / the aux roles: frames per workgroup
#define SQ_NQ 8           // stack work queues: sub-queues (head words 128 bytes apart)
#define TLP_LDS_MAX (160 * 1024)      // LDS of a CU: no tile may ask for more
#define TLP_LDS_OPTIN (48 * 1024)     // dynamic LDS above this needs hipFuncAttributeMaxDynamicSharedMemorySize
#define TLP_LDS_PREP (40 * 1024)      // the fused prep launch: four workgroups per CU must stay resident (its gather roles live on occupancy)
#define TLP_POST_MT 5                 // wide post-net tiles: 16 * 5 = 80 rows per workgroup
// leading dimension for an LDS A-tile read "row = lane&15, k = lane>>4" with ds_read_b32: ld == 2 (mod 32) makes the 32-lane groups conflict free
TLP_HD static inline int tr_lda(int K) { return ((K + 29) / 32) * 32 + 2; }

// per-kernel-group timing (HIP events on the launch stream; bench.py roofline): one group per LAUNCH of the heavy kernels, so that bench.py can name the
// single longest kernel (PG_WGRAD = the gate contraction's weight gradient dW1, then the residual 1x1's, the skip 1x1's, the post-net pair's and the causal table's)
enum { PG_PREP = 0, PG_LAYER_FWD, PG_POST_FWD, PG_CE, PG_POST_BWD, PG_WGRAD, PG_LAYER_BWD, PG_GRAD_TAIL, PG_ADAM, PG_ALLREDUCE,
       PG_WGRAD_WR, PG_WGRAD_SKIP, PG_WGRAD_POST, PG_WGRAD_CAUSAL, PG_COUNT };

struct StepPrepPlan { int nx0, rpg, naux, nbias, nwt, nprep; };     // k_step_prep: workgroups per role (items: per batch item); rpg: rows of a table workgroup
struct TlpLaunch { unsigned gx = 0, gy = 1, gz = 1, block = 0; size_t lds = 0; };

// ---------------------------------------------------------------- the call's shape
struct TrainShape {
    int rc = QPN_OK;                                   // QPN_EINVAL (and the error text set): nothing else is valid then
    int B = 0, T = 0, F = 0, Td = 0, BL = 0, maxd = 0, N0 = 0, N1 = 0;
    int s_in[TR_MAXL] = {}, s_out[TR_MAXL] = {}, tap_off[TR_MAXL] = {};      // first valid local row of a layer's input / output; its tap table (every layer has one)
    int ntap_layers = 0;
    int ffirst = 0, nfr = 0;                           // hoist: first frame the N1 rows touch, frames they touch
    int qT[TR_MAXL] = {}, qP[TR_MAXL + 1] = {}, qtotal = 0;      // stack queues: 16-row tiles per batch item in layer l (= the tiles of a per-layer launch), first position of layer l, positions
};
inline TrainShape train_shape(const Geom& g, const TrainLayout& lay, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd) {
    TrainShape s;
    const int64_t N0 = (int64_t)g.recA * maxd + g.recF + 1 + BL;           // qpnet.py:254-262
    const int64_t hup = g.U > 0 ? F * g.U : F;
    if (N0 > T || N0 - 1 > Td || N0 - 1 > hup) {
        qpn_set_error("chunk too short: need receptive field (%lld) + batch_length (%d) = %lld samples, have x:%lld d:%lld h_up:%lld",
                      (long long)(N0 - BL), BL, (long long)N0, (long long)T, (long long)Td, (long long)hup);
        s.rc = QPN_EINVAL; return s;
    }
    if (T >= ((int64_t)1 << 31) || Td >= ((int64_t)1 << 31) || F * (g.U > 0 ? g.U : 1) >= ((int64_t)1 << 31) || (int64_t)B * N0 >= ((int64_t)1 << 31)) {
        qpn_set_error("chunk too long: the training kernels index rows with 32 bits"); s.rc = QPN_EINVAL; return s;
    }
    s.B = B; s.T = (int)T; s.F = (int)F; s.Td = (int)Td; s.BL = BL; s.maxd = maxd; s.N0 = (int)N0; s.N1 = (int)N0 - 1;
    const int N1 = s.N1;
    int row = 0, pos = 0;
    for (int l = 0; l < g.L; ++l) {
        const TrainPlanLayer& ly = lay.layers[l];
        s.s_in[l] = row; row += ly.adaptive ? ly.dilation * maxd : ly.dilation; s.s_out[l] = row;
        s.tap_off[l] = l * B * N1;             // every layer gets a tap table (fixed layers: n - dilation), so the kernels load taps unconditionally
        s.qT[l] = (N1 - s.s_out[l] + 15) / 16;
        s.qP[l] = pos; pos += B * s.qT[l];     // positions of a queue: layer-major, batch item, tile (rows ascending)
    }
    s.ntap_layers = g.L;
    for (int l = g.L; l <= TR_MAXL; ++l) s.qP[l] = pos;
    s.qtotal = pos;
    if (lay.hoist) {
        if (N1 >= (1 << 24)) {
            qpn_set_error("chunk too long for the register-resident layer kernels (%d rows; QPN_AUX_HOIST=0 QPN_LAYER_PERSIST=0 QPN_LAYER_BWD_PERSIST=0 selects the tile-per-workgroup kernels)", N1);
            s.rc = QPN_EINVAL; return s;
        }
        s.ffirst = (int)(((int64_t)F * g.U - N1) / g.U); s.nfr = (int)F - s.ffirst;
    }
    return s;
}

// ---------------------------------------------------------------- conditions shared by both directions
// the register-resident layer kernels (n_resch 64, K = 176 or the hoisted K = 128): 32-bit element offsets of one batch item
inline bool tlp_persist_fwd(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s) {
    return g.C == 64 && (lay.Ktp == 176 || lay.hoist) && s.N1 < (1 << 24) && k.persist_fwd;
}
inline bool tlp_off32_bwd(const Geom& g, const TrainLayout& lay, const TrainShape& s) {
    return (int64_t)s.N1 * (lay.LC > 2 * g.C ? lay.LC : 2 * g.C) < (1ll << 32);
}
inline bool tlp_persist_bwd(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s) {
    return g.C == 64 && (lay.Ktp == 176 || lay.hoist) && lay.Ap <= 64 && s.N1 < (1 << 24) && tlp_off32_bwd(g, lay, s) && k.persist_bwd;
}
// the whole stack as ONE launch over a (layer, tile) work queue (train_stack.hip)
inline bool tlp_stack_fwd_fits(const Geom& g, const TrainLayout& lay, const TrainShape& s) {
    return g.C == 64 && (lay.hoist ? lay.Ktp == 128 : lay.Ktp == 176) && g.L >= 1 && g.L <= TR_MAXL && s.B < 65536 && (int64_t)s.N1 * g.C * 4 <= (1ll << 30) &&
           (int64_t)(g.L + 1) * s.B * s.N1 < (1ll << 31);
}
inline bool tlp_stack_bwd_fits(const Geom& g, const TrainLayout& lay, const TrainShape& s) {
    return tlp_stack_fwd_fits(g, lay, s) && lay.Ap <= 64 && (int64_t)s.B * s.BL * lay.LC < (1ll << 31) && tlp_off32_bwd(g, lay, s);
}
// wide post-net tiles (S = Q = 256, n_resch 64).  k_post_fwd_w contracts the skip path one layer (64 gate columns) at a time, so L * C does not matter to it;
// k_post_bwd_w produces the L * C columns of the skip-path gate gradients in passes of 256 (its eight waves' column tiles), so L * C must be a multiple of 256,
// and 256 and 512 are what it is admitted for: the two conditions differ on purpose
inline bool tlp_post_wide_fwd(const Geom& g, const TrainKnobs& k) { return g.S == 256 && g.Q == 256 && g.C == 64 && k.post_wide; }
inline bool tlp_post_wide_bwd(const Geom& g, const TrainLayout& lay, const TrainKnobs& k) { return tlp_post_wide_fwd(g, k) && (lay.LC == 256 || lay.LC == 512); }
inline bool tlp_zero_in_post(const Geom& g, const TrainLayout& lay, const TrainKnobs& k) { return tlp_post_wide_bwd(g, lay, k) && k.zero_in_post; }

inline unsigned tlp_nq(unsigned G) { return G / 8 < 1 ? 1 : (G / 8 < SQ_NQ ? G / 8 : SQ_NQ); }      // every sub-queue needs a puller (a workgroup's home: (blockIdx / 8) % nq)
inline TlpLaunch tlp_launch(unsigned gx, unsigned gy, unsigned gz, unsigned block, size_t lds) { TlpLaunch l; l.gx = gx; l.gy = gy; l.gz = gz; l.block = block; l.lds = lds; return l; }
inline size_t tlp_lds_aux(const Geom& g, bool hoist) { return hoist ? (size_t)(2 * g.C * g.A + g.A * AUXP_FPB + 8) * sizeof(float) : 0; }
// k_train_prep: `blocks` item workgroups per batch item (the launch's third argument), then the frame-rate projections' workgroups
inline TlpLaunch tlp_prep_launch(int C, int Ap, int L, int A, int B, int N1, bool hoist, int nfr, int* blocks) {
    const long items = (long)N1 * (C / 4 + (hoist ? 0 : Ap / 4) + L);
    *blocks = (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
    const int naux = hoist ? (nfr + 1 + AUXP_FPB - 1) / AUXP_FPB * L : 0;
    return tlp_launch((unsigned)(*blocks + naux), (unsigned)B, 1, 256, hoist ? (size_t)(2 * C * A + A * AUXP_FPB + 8) * sizeof(float) : 0);
}

// ---------------------------------------------------------------- the forward
enum { TLP_GENERIC = 0, TLP_PERSIST, TLP_STACK };      // the layer path of a direction: a tile per workgroup / register-resident, a launch per layer / one work-queue launch
enum { TLP_POST_TILE = 0, TLP_POST_WIDE, TLP_POST_FB };                // the post-net form: 16-row tiles / 80-row tiles / (forward only) forward and backward in one launch
struct TrainFwdFacts {
    int cus = 0;                       // compute units of the device
    bool queues_usable = false;        // the stack queues are allocated, the stream is not capturing, no queue launch of this handle has given up
    bool flat_aligned16 = false;       // the flat parameter pointer
    bool targets = false, want_logits = false, dlogits = false;
    bool fuse_bwd = false;             // the one-call step: this forward's backward follows with the same dL/dlogits
    bool soft_targets = false, loss_opts = false;      // the armed loss forms (k_ce_soft / k_ce_hard<NV, true> behind the forward)
};
struct TrainFwdPlan {
    int rc = QPN_OK;
    bool gemm = false;                 // the GEMM step: nothing below but fuse_prep (false), fuse_ce (false) and the refresh launch is used
    bool queues_usable = false;        // (the backward of this forward may use its queue)
    bool fuse_prep = false; TlpLaunch refresh, prep; int prep_blocks = 0; StepPrepPlan roles = {};
    int path = TLP_GENERIC, form = 11; // form: template argument of the persistent / queue kernels (K = 16 * form: 8 hoisted, 11 with the aux columns)
    int flags0 = 0;                    // 2: XCD-aware tile order
    TlpLaunch layer[TR_MAXL], stack; unsigned nq = 0;
    bool test_stack_gives_up = false;
    int post = TLP_POST_TILE; TlpLaunch post_l;
    bool fuse_ce = false, fuse_post = false, store_logits = true;
};
inline TrainFwdPlan train_fwd_plan(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s, const TrainFwdFacts& f) {
    TrainFwdPlan p;
    const int C = g.C, S = g.S, Q = g.Q, L = g.L, B = s.B, N1 = s.N1, BL = s.BL;
    p.gemm = lay.use_gemm; p.queues_usable = f.queues_usable; p.test_stack_gives_up = k.test_stack_gives_up;
    p.refresh = tlp_launch((unsigned)((lay.n_map + (int64_t)2 * Q * C + lay.n_bias + 16 + 64 + 255) / 256), 1, 1, 256, 0);
    if (p.gemm) return p;
    // ---- the first launch: k_step_prep (refresh roles + the chunk's preparation) where the causal table slices fit, else k_refresh + k_train_prep
    const auto lds_x0 = [&](int rpg) { return ((size_t)2 * Q * X0_ST + 2 * (size_t)rpg) * sizeof(float); };
    p.fuse_prep = k.prep_fuse && !(C % X0_CS || Q % 2 || g.causal_w % 4 || !f.flat_aligned16 || (lay.hoist && g.A > 64)) && lds_x0(X0_RPG) <= TLP_LDS_PREP;
    if (p.fuse_prep) {
        StepPrepPlan& r = p.roles;
        const int64_t R = (int64_t)B * N1, rpg = (R + 127) / 128;      // ~128 row groups: 128 x (C / 16) workgroups x 32 KB of L2 reads = 16 MB
        r.rpg = (int)(rpg < 16 ? 16 : rpg > X0_RPG ? X0_RPG : rpg);
        r.nx0 = (int)((R + r.rpg - 1) / r.rpg) * (C / X0_CS);
        r.naux = lay.hoist ? (s.nfr + 1 + AUXP_FPB - 1) / AUXP_FPB * L * B : 0;
        r.nbias = (lay.n_bias + 64 + 255) / 256;
        r.nwt = (int)((lay.n_map + 1023) / 1024);
        const long items = (long)N1 * ((lay.hoist ? 0 : lay.Ap / 4) + L);
        r.nprep = (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
        if (r.nprep < 1) r.nprep = 1;
        const size_t la = tlp_lds_aux(g, lay.hoist), lx = lds_x0(r.rpg);
        p.prep = tlp_launch((unsigned)(r.nx0 + r.naux + r.nbias + r.nwt + r.nprep * B), 1, 1, 256, la > lx ? la : lx);
    } else p.prep = tlp_prep_launch(C, lay.Ap, L, g.A, B, N1, lay.hoist, s.nfr, &p.prep_blocks);
    // ---- the layers.  16-row tiles everywhere (twice the workgroups of 32-row tiles, all co-resident: measured 8-15 % faster for the layer and post-net kernels)
    const size_t lds_layer = (size_t)16 * (tr_lda(lay.Ktp) + tr_lda(C)) * sizeof(float);
    const size_t lds_post = (size_t)16 * (tr_lda(S) + (tr_lda(S) > 2 * tr_lda(C) ? tr_lda(S) : 2 * tr_lda(C))) * sizeof(float);
    if (lds_layer > TLP_LDS_MAX || lds_post > TLP_LDS_MAX) {
        qpn_set_error("training kernels: tiles do not fit the 160 KiB LDS for n_resch=%d n_skipch=%d (n_resch <= 128 supported)", C, S);
        p.rc = QPN_EINVAL; return p;
    }
    p.flags0 = k.xcd_swizzle ? 2 : 0; p.form = lay.hoist ? 8 : 11;
    const bool persist = tlp_persist_fwd(g, lay, k, s);
    if (lay.hoist && !persist) { qpn_set_error("internal: the frame-rate aux term needs the register-resident layer kernels"); p.rc = QPN_EINVAL; return p; }
    p.path = !persist ? TLP_GENERIC : (k.stack_q_fwd && f.queues_usable && tlp_stack_fwd_fits(g, lay, s)) ? TLP_STACK : TLP_PERSIST;
    if (p.path == TLP_STACK) {
        unsigned G = k.stack_wgs > 0 ? (unsigned)k.stack_wgs : (unsigned)f.cus * 2;      // 2 workgroups per CU
        if (G > (unsigned)s.qtotal) G = (unsigned)s.qtotal;
        if (G > 1024) G = 1024;                                                            // (scratch rows: one pair per workgroup)
        p.stack = tlp_launch(G, 1, 1, 256, (size_t)(32 * tr_lda(16 * p.form) + 4 * 16 * tr_lda(64)) * sizeof(float) + 64);
        p.nq = tlp_nq(G);
    } else for (int l = 0; l < L; ++l) {
        const int tiles = s.qT[l];
        if (persist) {
            int G = f.cus * 2; if (G > tiles) G = tiles;
            if (G > 1024) G = 1024;                                                        // (scratch_rows holds a pair of rows for 1024 workgroups per batch item)
            p.layer[l] = tlp_launch((unsigned)G, (unsigned)B, 1, 256, (size_t)(32 * tr_lda(lay.Ktp) + 4 * 16 * tr_lda(64)) * sizeof(float));
        } else p.layer[l] = tlp_launch((unsigned)tiles, (unsigned)B, 1, 256, lds_layer);
    }
    // ---- the loss and the post-net
    p.fuse_ce = f.targets && Q <= S && Q % 256 == 0 && !k.ce_separate && !f.soft_targets && !f.loss_opts;      // (armed: QPN_CE_SEPARATE's route)
    p.store_logits = !(p.fuse_ce && !f.want_logits);
    // (the post-net's backward inside the forward's launch, k_post_fb_w: where the backward would have run k_post_bwd_w with the zeroing inside)
    p.fuse_post = f.fuse_bwd && p.fuse_ce && f.dlogits && k.post_fuse && tlp_zero_in_post(g, lay, k);
    const size_t ldsw = (size_t)16 * TLP_POST_MT * (tr_lda(256) + 2 * tr_lda(64)) * sizeof(float);
    p.post = !tlp_post_wide_fwd(g, k) ? TLP_POST_TILE : p.fuse_post ? TLP_POST_FB : TLP_POST_WIDE;
    p.post_l = p.post == TLP_POST_TILE ? tlp_launch((unsigned)(BL + 15) / 16, (unsigned)B, 1, 512, lds_post)
                                       : tlp_launch((unsigned)(BL + 16 * TLP_POST_MT - 1) / (16 * TLP_POST_MT), (unsigned)B, 1, 512, ldsw);
    return p;
}

// ---------------------------------------------------------------- the final reduction and what follows it (also the GEMM step's tail)
struct TrainTailPlan {
    int rc = QPN_OK;
    bool early_done = false;           // the [g_early0, g_early1) slab range has been reduced already
    bool up_done = false;              // ... and so have the zeroing / trailer and, on top of the zeros, the upsampling kernel's gradient (or the aux tail) and the feature gradient
    TlpLaunch reduce;
    bool causal_hist = false; int CB = 0, rpw = 0; TlpLaunch causal;       // k_causal_bwd: no contraction owns the causal table
    bool up_bwd = false, aux_tail = false, input_grad = false; TlpLaunch up, aux;
};
struct TrainTailIn { int C, Q, U, L, A, B, N1, F, gstage, n_gzero, g_cw; bool hoist; };      // (the GEMM step fills it from its kernel arguments)
inline TrainTailIn tlp_tail_in(const Geom& g, const TrainLayout& lay, const TrainShape& s) {
    return TrainTailIn{g.C, g.Q, g.U, g.L, g.A, s.B, s.N1, s.F, lay.gstage, lay.n_gzero, lay.slabs.g_cw, lay.hoist};
}
inline TrainTailPlan train_tail_plan(const TrainTailIn& in, bool feature_grad, bool early_done, bool up_done) {
    TrainTailPlan t;
    t.early_done = early_done; t.up_done = up_done;
    t.reduce = tlp_launch((unsigned)(((int64_t)in.gstage + (up_done ? 0 : in.n_gzero + 4) + 255) / 256), 1, 1, 256, 0);
    if (in.g_cw < 0) {
        int CB = in.C < 64 ? in.C : 64;
        while (CB > 1 && (size_t)2 * in.Q * CB * sizeof(float) > 128 * 1024) CB /= 2;
        const size_t lds_c = (size_t)2 * in.Q * CB * sizeof(float);
        if (lds_c > TLP_LDS_MAX) { qpn_set_error("causal-table gradient: n_quantize too large for the LDS histogram"); t.rc = QPN_EINVAL; return t; }
        t.causal_hist = true; t.CB = CB; t.rpw = (int)(((int64_t)in.B * in.N1 + 127) / 128); t.causal = tlp_launch(128, 1, 1, 256, lds_c);
    }
    t.up_bwd = in.U > 0 && !up_done && !in.hoist;
    t.aux_tail = in.hoist && !up_done;      // (behind the reduction's zeroing: it adds onto the upsampling-bias entry)
    t.input_grad = feature_grad && !up_done;
    if (in.U > 0) t.up = tlp_launch((unsigned)(in.F - (int)(((int64_t)in.F * in.U - in.N1) / in.U)), (unsigned)in.B, 1, 128, 0);      // a workgroup per (frame the N1 rows touch, batch item)
    t.aux = tlp_launch((unsigned)(in.L * in.A + in.U), 1, 1, 128, 0);
    return t;
}

// ---------------------------------------------------------------- the backward
// One job = one launch (or one event edge) of the backward, in the order the host enqueues them
enum { TJ_MARK = 0,        // nothing but its profile mark
       TJ_ZERO,            // k_zero_dx
       TJ_POST_BWD,        // k_post_bwd_w / k_post_bwd
       TJ_FORK,            // record ev_fork on main, the side stream waits for it
       TJ_SKIP, TJ_POST,   // the skip / post-net weight gradients (arg: chunks; TJ_POST's n: one paired launch, or two)
       TJ_REDUCE_EARLY,    // the early range of the slab reduction (n = 1: with the zeroing and the trailer)
       TJ_EARLY_EVENT,     // record ev_early: the post-net bucket is final (qpn_train_early_bucket)
       TJ_LAYERS,          // the layer backward: the queue launch, or a launch per layer
       TJ_MID,             // record ev_mid on main behind the layer backward, the side stream waits for it
       TJ_UP, TJ_AUX_TAIL, // k_up_bwd / k_aux_tail
       TJ_INPUT_GRAD,      // the feature gradient (armed only)
       TJ_W1, TJ_WR, TJ_CAUSAL,      // dW1, dWr, the causal table's contraction (arg: chunks)
       TJ_JOIN,            // record ev_join on the side stream
       TJ_WAIT,            // main waits for ev_join
       TJ_REDUCE,          // the final reduction
       TJ_CAUSAL_HIST };   // k_causal_bwd
struct TrainJob { signed char kind, side, mark, n; short arg; };      // side: 0 main, 1 side stream; mark: profile group marked behind it on its stream (-1: baseline, -2: none)
#define TLP_MAX_JOBS 40
struct TrainBwdFacts {
    int cus = 0;
    bool side_stream = false, prof_serial = false;
    bool gdst = false;                 // the slab reduction's map is there
    int append_scale = 0;
    bool feature_grad = false;         // qpn_train_input_grad armed
    bool first_bwd = false;            // the first backward of its forward (the queue's heads and flags belong to ONE backward per forward)
    bool same_dlogits = false;         // dL/dlogits is the buffer the forward was given
};
struct TrainBwdPlan {
    int rc = QPN_OK;
    bool gemm = false;
    bool post_done = false;            // the forward's launch has run the zeroing and the post-net's backward already
    int path = TLP_GENERIC, form = 11, swz = 0;
    TlpLaunch layer[TR_MAXL], stack; unsigned nq = 0;
    bool test_stack_gives_up = false;
    int post = TLP_POST_TILE; TlpLaunch post_l, zero;
    bool zero_in_post = false, overlap = false, early_reduce = false, up_side = false, wr_side = false, wr_summed = false, post_pair = false, wgrad_generic = false;
    int nch = 0, nch_side = 0;
    TlpLaunch reduce_early;
    TrainTailPlan tail;                // (tail.early_done, tail.up_done: the two flags the final reduction receives)
    TrainJob jobs[TLP_MAX_JOBS]; int njobs = 0;
};
inline TrainBwdPlan train_bwd_plan(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s, const TrainFwdPlan& fwd, const TrainBwdFacts& f) {
    TrainBwdPlan p;
    const int C = g.C, S = g.S, Q = g.Q, L = g.L, B = s.B, BL = s.BL;
    p.gemm = lay.use_gemm;
    if (p.gemm) return p;
    p.post_done = fwd.fuse_post && f.first_bwd && f.same_dlogits;      // (a repeated backward, or another dL/dlogits: the separate kernel)
    p.test_stack_gives_up = k.test_stack_gives_up;
    // 16-row tiles (measured 11-15 % faster than 32 rows: twice the workgroups, a shorter last round)
    const size_t lds_post = (size_t)16 * (tr_lda(Q > S ? Q : S) + tr_lda(S)) * sizeof(float);
    const size_t lds_layer = (size_t)16 * (4 * tr_lda(C) + tr_lda(2 * C)) * sizeof(float);
    if (lds_post > TLP_LDS_MAX || lds_layer > TLP_LDS_MAX) { qpn_set_error("backward tiles do not fit LDS"); p.rc = QPN_EINVAL; return p; }
    const bool persist = tlp_persist_bwd(g, lay, k, s);
    if (lay.hoist && !persist) { qpn_set_error("internal: the frame-rate aux term needs the register-resident layer kernels"); p.rc = QPN_EINVAL; return p; }
    p.path = !persist ? TLP_GENERIC : (k.stack_q_bwd && f.first_bwd && fwd.queues_usable && tlp_stack_bwd_fits(g, lay, s)) ? TLP_STACK : TLP_PERSIST;
    p.form = lay.hoist ? 8 : 11; p.swz = k.xcd_swizzle ? 1 : 0;
    p.wr_summed = p.path == TLP_STACK;      // the stack queue's tiles have replaced the own-row part of dXout by the sum of both parts (store_dx in k_stack_bwd)
    p.post_pair = k.post_pair; p.wgrad_generic = k.wgrad_generic;
    if (p.path == TLP_STACK) {
        // 1.5 workgroups per CU: the skip / post-net weight gradients run on the side stream while this launch is resident, and a launch that fills every
        // CU twice over leaves them no room -- measured on the overlapped step: 0.846 ms with 2 per CU, 0.776 with 1.5, 0.778 with 1, 0.790 for the eight
        // per-layer launches.  The K = 128 form: 1.25 per CU -- 320 -- measured 1411-1415 steps/s against 1375 at 384 and 1365 at 256; counts whose groups
        // of eight do not divide evenly over the eight sub-queues -- 304, 336, 352 -- are 3-4 % slower
        unsigned G = k.stack_wgs_bwd > 0 ? (unsigned)k.stack_wgs_bwd : (unsigned)(p.form == 8 ? f.cus * 5 / 4 / 64 * 64 : f.cus * 3 / 2);
        if (G < 8) G = (unsigned)f.cus;
        if (G > (unsigned)s.qtotal) G = (unsigned)s.qtotal;
        if (G > 1024) G = 1024;
        p.stack = tlp_launch(G, 1, 1, 256, (size_t)(8 * 16 * tr_lda(64) + 16 * tr_lda(128) + 16 * tr_lda(16 * p.form)) * sizeof(float) + 128 + 256);      // + control words, + the hoist form's G partials
        p.nq = tlp_nq(G);
    } else for (int l = 0; l < L; ++l) {
        const int tiles = s.qT[l];
        if (persist) {      // register-resident weights, 2 workgroups per CU over contiguous tile ranges (k_layer_bwd_p)
            int G = f.cus * 2; if (G > tiles) G = tiles;
            if (G > 1024) G = 1024;
            p.layer[l] = tlp_launch((unsigned)G, (unsigned)B, 1, 256, (size_t)(8 * 16 * tr_lda(C) + 16 * tr_lda(2 * C) + 16 * tr_lda(lay.Ktp) + 64) * sizeof(float));
        } else p.layer[l] = tlp_launch((unsigned)tiles, (unsigned)B, 1, 256, lds_layer);
    }
    p.overlap = f.side_stream && !f.prof_serial && !k.serial;
    p.post = tlp_post_wide_bwd(g, lay, k) ? TLP_POST_WIDE : TLP_POST_TILE;
    p.zero_in_post = tlp_zero_in_post(g, lay, k);
    p.zero = tlp_launch(64, (unsigned)L, (unsigned)B, 256, 0);
    p.post_l = p.post == TLP_POST_WIDE ? tlp_launch((unsigned)(BL + 16 * TLP_POST_MT - 1) / (16 * TLP_POST_MT), (unsigned)B, 1, 512, (size_t)16 * TLP_POST_MT * tr_lda(256) * sizeof(float))
                                       : tlp_launch((unsigned)(BL + 15) / 16, (unsigned)B, 1, 512, lds_post);
    const TrainSlabs& sl = lay.slabs;
    // the memory-bound reduction of the skip / post-net slabs runs on the side stream under the matrix-bound layer backward instead of at the end of the step
    p.early_reduce = p.overlap && f.gdst && sl.g_early1 > sl.g_early0 && k.reduce_early;
    // with the early reduction doing the zeroing / trailer too, the upsampling kernel's gradient (hoist: the aux tail) runs on the side stream next to dW1
    p.up_side = p.early_reduce && g.U > 0 && k.up_side;
    p.wr_side = p.overlap && k.wr_side;
    p.nch = p.nch_side = lay.nch;
    // (only with the early reduction: otherwise ONE launch reduces every block with one slab count.  64 -> 48 chunks makes each of these launches slower alone and the step faster)
    if (p.early_reduce) p.nch_side = k.wgrad_chunks_side > 0 && k.wgrad_chunks_side <= p.nch ? k.wgrad_chunks_side : (p.nch <= 48 ? p.nch : 48);
    p.reduce_early = tlp_launch((unsigned)(((int64_t)(sl.g_early1 - sl.g_early0) + (p.up_side ? lay.n_gzero + 4 : 0) + 255) / 256), 1, 1, 256, 0);
    p.tail = train_tail_plan(tlp_tail_in(g, lay, s), f.feature_grad, p.early_reduce, p.up_side);
    if (p.tail.rc) { p.rc = p.tail.rc; return p; }

    // ---- the jobs, in launch order
    auto job = [&](int kind, int side, int mark, int arg = 0, int n = 0) {
        TrainJob& j = p.jobs[p.njobs++]; j.kind = (signed char)kind; j.side = (signed char)side; j.mark = (signed char)mark; j.arg = (short)arg; j.n = (signed char)n;
    };
    const int post_parts = (Q == S && k.post_pair) ? 1 : 2;          // (wgrad_post_paired, train_wgrad_plan.h)
    auto skip_post = [&](int side) { job(TJ_SKIP, side, PG_WGRAD_SKIP, p.nch_side); job(TJ_POST, side, PG_WGRAD_POST, p.nch_side, post_parts); };
    if (!p.post_done && !p.zero_in_post) job(TJ_ZERO, 0, -2);
    if (!p.post_done) job(TJ_POST_BWD, 0, PG_POST_BWD); else job(TJ_MARK, 0, PG_POST_BWD);
    if (p.overlap) {
        // the skip 1x1 and post-net weight gradients only need what the post-net's backward has just produced: on a side stream UNDER the layer backward
        job(TJ_FORK, 1, -1);
        skip_post(1);
        if (p.early_reduce) job(TJ_REDUCE_EARLY, 1, PG_GRAD_TAIL, 0, p.up_side ? 1 : 0);
        if (p.up_side && f.append_scale && lay.early_first >= 0) job(TJ_EARLY_EVENT, 1, -2);
    }
    job(TJ_LAYERS, 0, -2);
    if (p.wr_side || p.up_side) {
        job(TJ_MID, 1, -1);
        if (p.up_side) {      // behind the early reduction's zeroing, on the same stream; the feature gradient, when armed, next to it
            job(lay.hoist ? TJ_AUX_TAIL : TJ_UP, 1, f.feature_grad ? -2 : PG_GRAD_TAIL);
            if (f.feature_grad) job(TJ_INPUT_GRAD, 1, PG_GRAD_TAIL);
        }
        if (p.wr_side) job(TJ_WR, 1, PG_WGRAD_WR, p.nch);
    }
    if (p.overlap) job(TJ_JOIN, 1, -2);
    job(TJ_MARK, 0, PG_LAYER_BWD);
    job(TJ_W1, 0, PG_WGRAD, p.nch);
    if (!p.wr_side) job(TJ_WR, 0, PG_WGRAD_WR, p.nch);
    if (!p.overlap) skip_post(0);
    if (sl.g_cw >= 0) job(TJ_CAUSAL, 0, PG_WGRAD_CAUSAL, p.nch); else job(TJ_MARK, 0, PG_WGRAD_CAUSAL);
    if (p.overlap) job(TJ_WAIT, 0, -1);      // joined BEFORE the final reduction (and before any early return: the caller's stream must own everything enqueued here)
    job(TJ_REDUCE, 0, -2);
    if (p.tail.causal_hist) job(TJ_CAUSAL_HIST, 0, -2);
    if (p.tail.up_bwd) job(TJ_UP, 0, -2);
    if (p.tail.aux_tail) job(TJ_AUX_TAIL, 0, -2);
    if (p.tail.input_grad) job(TJ_INPUT_GRAD, 0, -2);
    job(TJ_MARK, 0, PG_GRAD_TAIL);
    return p;
}

// ---------------------------------------------------------------- the plans as text (qpn_train_last_plan; built on request only)
inline void tlp_put(std::string& o, const char* name, const TlpLaunch& l) {
    char b[160]; snprintf(b, sizeof(b), " %s(%u,%u,%u;%u;%zu)", name, l.gx, l.gy, l.gz, l.block, l.lds); o += b;
}
inline const char* tlp_path_name(int path) { return path == TLP_STACK ? "stack" : path == TLP_PERSIST ? "persist" : "generic"; }
inline std::string tlp_kname(const char* base, int form, int last) {
    char b[64]; if (last < 0) snprintf(b, sizeof(b), "%s<%d>", base, form); else snprintf(b, sizeof(b), "%s<%d,%d>", base, form, last); return b;
}
inline std::string plan_text(const Geom& g, const TrainLayout& lay, const TrainShape& s, const TrainFwdPlan& p) {
    char b[256];
    if (p.gemm) return "fwd[path=gemm]";
    snprintf(b, sizeof(b), "fwd[path=%s hoist=%d fuse_prep=%d fuse_ce=%d fuse_post=%d logits=%d N1=%d qtotal=%d]", tlp_path_name(p.path), lay.hoist ? 1 : 0, p.fuse_prep ? 1 : 0,
             p.fuse_ce ? 1 : 0, p.fuse_post ? 1 : 0, p.store_logits ? 1 : 0, s.N1, s.qtotal);
    std::string o = b;
    if (p.fuse_prep) {
        snprintf(b, sizeof(b), " roles=%d,%d,%d,%d,%d,%d", p.roles.nx0, p.roles.rpg, p.roles.naux, p.roles.nbias, p.roles.nwt, p.roles.nprep); o += b;
        tlp_put(o, "k_step_prep", p.prep);
    } else { tlp_put(o, "k_refresh", p.refresh); tlp_put(o, "k_train_prep", p.prep); }
    if (p.path == TLP_STACK) { tlp_put(o, tlp_kname("k_stack_fwd", p.form, -1).c_str(), p.stack); snprintf(b, sizeof(b), " nq=%u", p.nq); o += b; }
    else for (int l = 0; l < g.L; ++l)
        tlp_put(o, p.path == TLP_PERSIST ? tlp_kname("k_layer_fwd_p", p.form, l == g.L - 1).c_str() : "k_layer_fwd<1>", p.layer[l]);
    tlp_put(o, p.post == TLP_POST_FB ? "k_post_fb_w<5>" : p.post == TLP_POST_WIDE ? "k_post_fwd_w<5>" : "k_post_fwd<1>", p.post_l);
    return o;
}
inline std::string plan_text(const Geom& g, const TrainLayout& lay, const TrainShape& s, const TrainBwdPlan& p) {
    char b[320];
    if (p.gemm) return "bwd[path=gemm]";
    snprintf(b, sizeof(b), "bwd[path=%s hoist=%d post_done=%d zero_in_post=%d overlap=%d early_reduce=%d up_side=%d wr_side=%d nch=%d nch_side=%d tail=%d,%d]", tlp_path_name(p.path),
             lay.hoist ? 1 : 0, p.post_done ? 1 : 0, p.zero_in_post ? 1 : 0, p.overlap ? 1 : 0, p.early_reduce ? 1 : 0, p.up_side ? 1 : 0, p.wr_side ? 1 : 0, p.nch, p.nch_side,
             p.tail.early_done ? 1 : 0, p.tail.up_done ? 1 : 0);
    std::string o = b;
    (void)s;
    for (int i = 0; i < p.njobs; ++i) {
        const TrainJob& j = p.jobs[i];
        const char* st = j.side ? " side:" : " main:";
        auto named = [&](const char* name, const TlpLaunch& l) { o += st; std::string t; tlp_put(t, name, l); o += t.c_str() + 1; };
        auto wg = [&](const char* name) { snprintf(b, sizeof(b), "%s%s(%d)", st, name, (int)j.arg); o += b; };
        switch (j.kind) {
        case TJ_MARK: break;
        case TJ_ZERO: named("k_zero_dx", p.zero); break;
        case TJ_POST_BWD: named(p.post == TLP_POST_WIDE ? "k_post_bwd_w<5>" : "k_post_bwd<1>", p.post_l); break;
        case TJ_FORK: o += " fork"; break;
        case TJ_SKIP: wg("skip"); break;
        case TJ_POST: wg("post"); snprintf(b, sizeof(b), "x%d", (int)j.n); o += b; break;
        case TJ_REDUCE_EARLY: named(j.n ? "k_reduce_grad_s+tail" : "k_reduce_grad_s", p.reduce_early); break;
        case TJ_EARLY_EVENT: o += " early"; break;
        case TJ_LAYERS:
            if (p.path == TLP_STACK) { named(tlp_kname("k_stack_bwd", p.form, -1).c_str(), p.stack); snprintf(b, sizeof(b), " nq=%u", p.nq); o += b; }
            else for (int l = g.L - 1; l >= 0; --l) named(p.path == TLP_PERSIST ? tlp_kname("k_layer_bwd_p", p.form, l == g.L - 1).c_str() : "k_layer_bwd<1>", p.layer[l]);
            break;
        case TJ_MID: o += " mid"; break;
        case TJ_UP: named("k_up_bwd", p.tail.up); break;
        case TJ_AUX_TAIL: named("k_aux_tail", p.tail.aux); break;
        case TJ_INPUT_GRAD: o += st; o += "input_grad"; break;
        case TJ_W1: wg("w1"); break;
        case TJ_WR: wg("wr"); break;
        case TJ_CAUSAL: wg("causal"); break;
        case TJ_JOIN: o += " join"; break;
        case TJ_WAIT: o += " wait"; break;
        case TJ_REDUCE: named("k_reduce_grad_s", p.tail.reduce); break;
        case TJ_CAUSAL_HIST: named("k_causal_bwd", p.tail.causal); break;
        }
    }
    return o;
}
