// train_plan.h -- the layout of a training handle: where every weight, bias and gradient lives in the packed blocks, the gradient slabs and the per-call arena.
// Pure host arithmetic (plain C++: no HIP, no handle, no globals): train_host.hip uploads what train_plan() returns and carves the arena where train_arena()
// says; tests/train_plan_sweep.cpp checks the invariants of both on a CPU.  Every index expression of a tensor is stated ONCE (the tp_*_src functions of qpn_geom.h):
// the forward packs, their transposes and the gradient map all go through it, so a gradient cannot land on another parameter than the forward read.
#pragma once
#include "qpn_geom.h"
#include <vector>

#define TR_MAXL QPN_MAX_LAYERS   // layers supported by the training kernels (the reference's deepest shipped stack, Rd10Rr3Ed4Er1, has 34: src/utils/param_model.py:66-72)
#define TR_EB_SLOTS 32           // the gate-bias accumulators E are spread over this many slabs per layer (workgroup index mod): ~40 float atomics per address and layer

// slab offsets (floats) of every weight-grad block; host side only
struct TrainSlabs {
    int g_w1[TR_MAXL], g_b1[TR_MAXL], g_wr[TR_MAXL], g_br[TR_MAXL], g_ws[TR_MAXL], g_bs;
    int g_p1, g_bp1, g_p2, g_bp2;
    int g_early0, g_early1;           // slab range [g_early0, g_early1): skip 1x1 / skip bias / post-net blocks, complete before the layer backward ends
    int g_cw, g_cb;                   // causal conv table [tap][C][Q] and bias, or -1: histogram kernel (k_causal_bwd)
};

// aux hoist: what k_aux_proj / k_aux_tail need of every layer (flat offsets of the aux 1x1 weights, offset of the packed gate bias, first valid row of the call)
struct AuxGeom { int auxS[TR_MAXL], auxT[TR_MAXL], bias1[TR_MAXL], s_out[TR_MAXL]; };

// K-major, zero-padded weight blocks of the GEMM path (train_gemm.hip; n_resch > 128): float offsets into `wp`
struct TrainGemm {
    const float* wp;                  // packed weights (refreshed from the flat parameters every step)
    float* G;                         // [L][B][N1][C] gate outputs sigma*tanh (A operand of the residual / skip contractions)
    int K1;                           // 2C + n_aux padded to 32: K of the gate GEMM
    int N1g, Cg, Sg, Qg, LCg, Ktg;    // column counts padded to 128: gate tiles, C, S, Q, L*C, 2C + n_aux
    long w1[TR_MAXL], w1t[TR_MAXL], wr[TR_MAXL], wrt[TR_MAXL];
    long ws, wst, p1, p1t, p2, p2t;
};

// Launch-plan knobs, parsed ONCE per handle from the environment (train_init): nothing in the per-step launch path calls getenv().
// All optional; the defaults are the measured best.  tests/test_train_gpu.py builds a fresh model (= a fresh handle) per arrangement.
struct TrainKnobs {
    bool serial;                      // QPN_TRAIN_SERIAL=1: every launch of a step on the caller's stream (also forced while a profile is taken)
    bool stack_q_fwd, stack_q_bwd;    // QPN_STACK_QUEUE=0 / QPN_STACK_QUEUE_BWD=0: a launch per layer instead of the work-queue launches (train_stack.hip)
    int stack_wgs, stack_wgs_bwd;     // QPN_STACK_WGS / QPN_STACK_WGS_BWD: grid sizes of the queue launches (0: 2 / 1.5 workgroups per CU)
    bool persist_fwd, persist_bwd;    // QPN_LAYER_PERSIST=0 / QPN_LAYER_BWD_PERSIST=0: the tile-per-workgroup layer kernels at n_resch 64
    bool wgrad_generic;               // QPN_WGRAD_GENERIC=1: the run-time-tiled weight-gradient kernel (k_wgrad2)
    int wgrad_chunks, wgrad_chunks_side;   // QPN_WGRAD_CHUNKS / QPN_WGRAD_CHUNKS_SIDE: time chunks (= partial slabs) of the weight gradients
    bool post_fuse;                        // QPN_POST_FUSE=0: qpn_train_step runs the post-net's forward and backward as two kernels (k_post_fwd_w, k_post_bwd_w) instead of k_post_fb_w
    bool up_side, reduce_early, wr_side;   // QPN_UP_SIDE=0 / QPN_REDUCE_EARLY=0 / QPN_WR_SIDE=0: where the backward's small launches run
    bool post_pair, zero_in_post, post_wide;   // QPN_POST_WGRAD_PAIR=0 / QPN_ZERO_IN_POST=0 / QPN_POST_WIDE=0
    bool xcd_swizzle;                 // QPN_NO_XCD_SWIZZLE=1 clears it
    bool ce_separate;                 // QPN_CE_SEPARATE=1: cross entropy as its own kernel behind the forward
    bool event_fence;                 // QPN_EVENT_FENCE=1: system-scope fence at the fork / join events
    bool prep_fuse;                   // QPN_PREP_FUSE=0: the per-step refresh (k_refresh) and the chunk's preparation (k_train_prep) as two launches instead of k_step_prep's one
    bool aux_hoist;                   // QPN_AUX_HOIST=0: the auxiliary 1x1 contracted at sample rate (K = 176) even where the frame-rate form applies
    bool test_stack_gives_up;         // -DQPN_TESTING builds only (QPN_TEST_STACK_GIVES_UP=1): the queue launches' published flags are made unrecognisable
};

// (where a tensor element lives in the flat parameter vector -- tp_gate_src .. tp_post2_src, tp_gate_bias, tp_idx: qpn_geom.h, shared with the decode planner)
// causal conv weight (C, Q, 2)
inline int64_t tp_causal_src(const Geom& g, int c, int q, int tap) { return g.causal_w + ((int64_t)c * g.Q + q) * 2 + tap; }
inline int tp_pad_to(int v, int q) { return (v + q - 1) / q * q; }

// ---------------------------------------------------------------- the two packed orders of a weight block
// position of B[k][n] in a fragment-ordered block (K x N, both multiples of 16), the operand order of wave_gemm (train_common.h):
// [(ks4 * NT + nt) * 64 + lane] float4, element e of it = B[16 ks4 + 4 e + (lane >> 4)][16 nt + (lane & 15)]
inline size_t tp_frag_pos(int N, int k, int n) {
    const int ks4 = k / 16, e = (k % 16) / 4, lane = ((k % 4) << 4) | (n % 16);
    return (((size_t)ks4 * (N / 16) + n / 16) * 64 + lane) * 4 + e;
}
// B[k][n] (K x N, both multiples of 16) -> fragment order; returns the float4 offset.  transposed: the block holds B^T, i.e. element (k, n) comes from src(n, k)
template <class F>
inline int tp_frag_pack(std::vector<int>& map, int K, int N, bool transposed, F src) {
    const int off4 = (int)(map.size() / 4);
    map.resize(map.size() + (size_t)K * N);
    int* m = map.data() + (size_t)off4 * 4;
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) m[tp_frag_pos(N, k, n)] = tp_idx(transposed ? src(n, k) : src(k, n));
    return off4;
}
// B[k][n] (K x N valid) -> K-major block [Kp][Np], zero padded (-1); returns the float offset
template <class F>
inline long tp_kmajor_pack(std::vector<int>& map, int K, int Kp, int N, int Np, bool transposed, F src) {
    const long off = (long)map.size();
    map.resize(map.size() + (size_t)Kp * Np, -1);
    int* m = map.data() + off;
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) m[(size_t)k * Np + n] = tp_idx(transposed ? src(n, k) : src(k, n));
    return off;
}
// column q of the GEMM path's gate block -> z column (natural: half * C + c), or -1 (padding): 128-wide tiles [sigma c0..c0+63 | tanh c0..c0+63]
inline int tp_gemm_gate_col(int C, int q) {
    const int tile = q / 128, w = q % 128, half = w / 64, c = 64 * tile + w % 64;
    return c < C ? half * C + c : -1;
}

// ---------------------------------------------------------------- the plan
struct TrainPlanLayer { int adaptive, dilation, w1_f4, wr_f4, w1t_f4, wrt_f4, bias1, biasr; };      // the constant fields of TrLayer
// the small part of a plan, which a handle keeps: the path and every offset ...
struct TrainLayout {
    bool use_gemm = false, hoist = false;      // hoist: the auxiliary 1x1 runs at frame rate (TrainParams::hoist)
    int Ap = 0, Kt = 0, Ktp = 0, LC = 0;
    TrainPlanLayer layers[TR_MAXL] = {};
    int ws_f4 = 0, p1_f4 = 0, p2_f4 = 0, wst_f4 = 0, p1t_f4 = 0, p2t_f4 = 0, bias_s = 0, bias_p1 = 0, bias_p2 = 0;
    int n_bias = 0;
    int64_t n_map = 0;                         // entries of the uploaded gather map (fragment-ordered blocks, or the GEMM path's K-major ones): what the refresh gathers
    int n_gzero = 0;                           // flat-grad entries no slab element feeds (TrainPlan::gzero)
    TrainSlabs slabs = {};                     // weight-grad staging space ("slab")
    int gstage = 0, nch = 0;                   // floats of one slab; time chunks (= partial slabs)
    int64_t early_first = -1;                  // first flat index of the tail that is final before the layer backward ends (the post-net blocks), or -1
};
// ... and what the handle copies or uploads once
struct TrainPlan : TrainLayout {
    int rc = QPN_OK;                           // QPN_EINVAL (and the error text set): a geometry the training kernels refuse; nothing else is valid then
    AuxGeom ag = {};                           // (s_out unset: a property of the call)
    TrainGemm gm = {};                         // GEMM path: offsets into h_gmap's blocks (pointers unset)
    std::vector<int> h_wmap;                   // gather map of the fragment-ordered weights (empty on the GEMM path, which keeps its own K-major blocks)
    std::vector<int> h_gmap;                   // ... of the K-major blocks (GEMM path only)
    std::vector<int> h_bstart, h_blist;        // CSR of the packed biases: packed bias i = sum of flat[h_blist[h_bstart[i] .. h_bstart[i + 1])]
    std::vector<int> h_gsrc;                   // flat-grad entry <- slab element; -1: no slab feeds it (zeroed, then written by a kernel of its own); -2: k_aux_tail stores it
    std::vector<int> gdst_start, gdst_list;    // its inverse, CSR: slab element s feeds gdst_list[gdst_start[s] .. gdst_start[s + 1]) (one spare entry at the end of the list)
    std::vector<int> gzero;                    // the -1 entries: listed for zeroing
    std::vector<int> h_ctmap;                  // causal conv table [tap][class][C] <- flat
};

inline TrainPlan train_plan(const Geom& g, const TrainKnobs& knobs, bool use_gemm) {
    TrainPlan t;
    const int C = g.C, S = g.S, Q = g.Q, A = g.A, L = g.L;
    auto refuse = [&](const char* msg) { qpn_set_error("%s", msg); t.rc = QPN_EINVAL; return t; };
    if (L > TR_MAXL) { qpn_set_error("training kernels support up to %d residual layers", TR_MAXL); t.rc = QPN_EINVAL; return t; }
    if (C % 16 || S % 16 || Q % 16) return refuse("training kernels need n_resch, n_skipch, n_quantize multiples of 16");
    if (use_gemm && (C % 32 || S % 32 || Q % 32)) return refuse("the GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32");
    if (g.n_params >= ((int64_t)1 << 31)) return refuse("the training maps index the parameters with 32 bits: this geometry has 2^31 or more");
    t.use_gemm = use_gemm;
    const int Ap = t.Ap = (A + 3) / 4 * 4;               // aux columns padded to the MFMA k-step
    // the auxiliary 1x1 at frame rate (TrainParams::hoist): the n_resch-64 register-resident kernels, at most two frames per 16-row tile
    t.hoist = !use_gemm && C == 64 && g.U >= 16 && A <= 64 && knobs.aux_hoist && knobs.persist_fwd && knobs.persist_bwd;
    t.Kt = t.hoist ? 2 * C : 2 * C + Ap; t.Ktp = (t.Kt + 15) / 16 * 16; t.LC = L * C;
    const int Ktp = t.Ktp, Kgate = t.hoist ? 2 * C : 2 * C + A;      // gate input columns with a weight (and a gradient) of their own in the block
    std::vector<int>& map = t.h_wmap;
    std::vector<std::vector<int>> biases;      // packed bias i <- list of flat indices
    auto add_bias = [&](int n, auto f) { int off = (int)biases.size(); for (int i = 0; i < n; ++i) biases.push_back(f(i)); return off; };
    auto one = [](int64_t flat) { return std::vector<int>{tp_idx(flat)}; };
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        TrainPlanLayer& ly = t.layers[l];
        ly.adaptive = y.adaptive; ly.dilation = y.dilation;
        auto gate = [&](int k, int n) { return tp_gate_src(y, C, A, k, n); };
        auto res = [&](int k, int n) { return tp_res_src(y, C, k, n); };
        ly.w1_f4 = tp_frag_pack(map, Ktp, 2 * C, false, gate);
        ly.w1t_f4 = tp_frag_pack(map, 2 * C, Ktp, true, gate);
        ly.wr_f4 = tp_frag_pack(map, C, C, false, res);
        ly.wrt_f4 = tp_frag_pack(map, C, C, true, res);
        ly.bias1 = add_bias(2 * C, [&](int n) { int64_t b[3]; const int nb = tp_gate_bias(y, C, n, b); std::vector<int> v; for (int i = 0; i < nb; ++i) v.push_back(tp_idx(b[i])); return v; });
        ly.biasr = add_bias(C, [&](int n) { return one(y.resb + n); });
    }
    auto skip = [&](int k, int n) { return tp_skip_src(g, k, n); };
    auto post1 = [&](int k, int n) { return tp_post1_src(g, k, n); };
    auto post2 = [&](int k, int n) { return tp_post2_src(g, k, n); };
    t.ws_f4 = tp_frag_pack(map, L * C, S, false, skip);
    t.wst_f4 = tp_frag_pack(map, S, L * C, true, skip);
    t.p1_f4 = tp_frag_pack(map, S, S, false, post1);
    t.p1t_f4 = tp_frag_pack(map, S, S, true, post1);
    t.p2_f4 = tp_frag_pack(map, S, Q, false, post2);
    t.p2t_f4 = tp_frag_pack(map, Q, S, true, post2);
    t.bias_s = add_bias(S, [&](int n) { std::vector<int> v; for (int l = 0; l < L; ++l) v.push_back(tp_idx(g.layers[l].skipb + n)); return v; });
    t.bias_p1 = add_bias(S, [&](int n) { return one(g.post1_b + n); });
    t.bias_p2 = add_bias(Q, [&](int n) { return one(g.post2_b + n); });
    if (use_gemm) {
        TrainGemm& gm = t.gm;
        std::vector<int>& gmap = t.h_gmap;
        const int Apad = tp_pad_to(Ap, 32);
        gm.K1 = 2 * C + Apad; gm.N1g = tp_pad_to(C, 64) * 2; gm.Cg = tp_pad_to(C, 128); gm.Sg = tp_pad_to(S, 128); gm.Qg = tp_pad_to(Q, 128);
        gm.LCg = tp_pad_to(L * C, 128); gm.Ktg = tp_pad_to(2 * C + Ap, 128);
        for (int l = 0; l < L; ++l) {
            const LayerGeom& y = g.layers[l];
            auto gate = [&](int k, int n) { return tp_gate_src(y, C, A, k, n); };
            auto res = [&](int k, int n) { return tp_res_src(y, C, k, n); };
            // gate GEMM: rows k = [x_cur C | x_past C | aux (n_aux, padded to 32)], columns in 128-wide tiles (tp_gemm_gate_col)
            gm.w1[l] = tp_kmajor_pack(gmap, 2 * C + A, gm.K1, gm.N1g, gm.N1g, false, [&](int k, int q) -> int64_t { const int n = tp_gemm_gate_col(C, q); return n >= 0 ? gate(k, n) : -1; });
            gm.w1t[l] = tp_kmajor_pack(gmap, 2 * C, 2 * C, 2 * C + A, gm.Ktg, true, gate);
            gm.wr[l] = tp_kmajor_pack(gmap, C, C, C, gm.Cg, false, res);
            gm.wrt[l] = tp_kmajor_pack(gmap, C, C, C, gm.Cg, true, res);
        }
        gm.ws = tp_kmajor_pack(gmap, L * C, L * C, S, gm.Sg, false, skip);
        gm.wst = tp_kmajor_pack(gmap, S, S, L * C, gm.LCg, true, skip);
        gm.p1 = tp_kmajor_pack(gmap, S, S, S, gm.Sg, false, post1);
        gm.p1t = tp_kmajor_pack(gmap, S, S, S, gm.Sg, true, post1);
        gm.p2 = tp_kmajor_pack(gmap, S, S, Q, gm.Qg, false, post2);
        gm.p2t = tp_kmajor_pack(gmap, Q, Q, S, gm.Sg, true, post2);
        std::vector<int>().swap(map);                        // the fragment-ordered blocks of the tile kernels are not used on this path
    }
    for (int l = 0; l < L; ++l) { t.ag.auxS[l] = tp_idx(g.layers[l].auxS); t.ag.auxT[l] = tp_idx(g.layers[l].auxT); t.ag.bias1[l] = t.layers[l].bias1; }
    t.n_bias = (int)biases.size();
    t.h_bstart.assign(1, 0);
    for (auto& v : biases) { for (int x : v) t.h_blist.push_back(x); t.h_bstart.push_back((int)t.h_blist.size()); }

    // ---- weight-grad staging space ("slab") and the flat-grad gather map
    // (slab order: first the blocks that need the layer backward -- dW1, dWr of every layer -- then, contiguous, the ones the side
    //  stream finishes early: skip 1x1 of every layer, skip bias, post-net; that range is reduced early as well, under the layer backward)
    TrainSlabs& sl = t.slabs;
    int go = 0;
    auto gtake = [&](int n) { int r = go; go += (n + 63) & ~63; return r; };
    std::vector<int>& gs = t.h_gsrc;
    gs.assign((size_t)g.n_params, -1);
    auto bias_grads = [&](int packed, int n, int slab) { for (int i = 0; i < n; ++i) for (int flat : biases[(size_t)packed + i]) gs[flat] = slab + i; };      // the biases of a packed sum share its gradient
    for (int l = 0; l < L; ++l) {
        sl.g_w1[l] = gtake(2 * C * Ktp);   // dW1[n][k] (n = z row, k = A-tile column), row-major [2C][Ktp]
        sl.g_b1[l] = gtake(2 * C);
        sl.g_wr[l] = gtake(C * C);         // dWr[o][c]
        sl.g_br[l] = gtake(C);
    }
    sl.g_early0 = go;
    for (int l = 0; l < L; ++l) sl.g_ws[l] = gtake(S * C);         // dWs_l[s][c]
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        for (int n = 0; n < 2 * C; ++n)
            for (int k = 0; k < 2 * C + A; ++k) gs[tp_gate_src(y, C, A, k, n)] = k < Kgate ? sl.g_w1[l] + n * Ktp + k : -2;      // (hoist: the aux columns are k_aux_tail's)
        bias_grads(t.layers[l].bias1, 2 * C, sl.g_b1[l]);
        for (int n = 0; n < C; ++n) for (int k = 0; k < C; ++k) gs[tp_res_src(y, C, k, n)] = sl.g_wr[l] + n * C + k;
        bias_grads(t.layers[l].biasr, C, sl.g_br[l]);
        for (int n = 0; n < S; ++n) for (int c = 0; c < C; ++c) gs[tp_skip_src(g, l * C + c, n)] = sl.g_ws[l] + n * C + c;
    }
    sl.g_bs = gtake(S);
    bias_grads(t.bias_s, S, sl.g_bs);
    sl.g_p1 = gtake(S * S); sl.g_bp1 = gtake(S); sl.g_p2 = gtake(Q * S); sl.g_bp2 = gtake(Q);
    sl.g_early1 = go;
    // the post-net blocks close the flat parameter order (state_dict order, qpnet.py): with the trailer behind them one contiguous early bucket
    t.early_first = (g.post1_b == g.post1_w + (int64_t)S * S && g.post2_w == g.post1_b + S && g.post2_b == g.post2_w + (int64_t)Q * S && g.post2_b + Q == g.n_params) ? g.post1_w : -1;
    for (int n = 0; n < S; ++n) for (int k = 0; k < S; ++k) gs[tp_post1_src(g, k, n)] = sl.g_p1 + n * S + k;
    bias_grads(t.bias_p1, S, sl.g_bp1);
    for (int n = 0; n < Q; ++n) for (int k = 0; k < S; ++k) gs[tp_post2_src(g, k, n)] = sl.g_p2 + n * S + k;
    bias_grads(t.bias_p2, Q, sl.g_bp2);
    // causal conv table: dW[c][q][tap] = sum_t dX0[t][c] * onehot(x[t-1+tap])[q] is one more time contraction (k_wgrad3 mode 4, train_wgrad.hip; its record: wgrad_rec_causal)
    // when its tiles fit (C = 64, Q a multiple of 128); otherwise the LDS-histogram kernel owns it (gs stays -1)
    sl.g_cw = sl.g_cb = -1;
    if (C == 64 && Q % 128 == 0 && !use_gemm) {
        sl.g_cw = gtake(2 * C * Q); sl.g_cb = gtake(C);
        for (int c = 0; c < C; ++c) {
            for (int q = 0; q < Q; ++q) for (int tp = 0; tp < 2; ++tp) gs[tp_causal_src(g, c, q, tp)] = sl.g_cw + tp * C * Q + c * Q + q;
            gs[g.causal_b + c] = sl.g_cb + c;
        }
    }
    t.gstage = go; t.nch = use_gemm ? 4 : 64;
    if (knobs.wgrad_chunks > 0) t.nch = knobs.wgrad_chunks;      // tuning knob: time chunks (= partial slabs)
    // the upsampling kernel's gradient is written by a dedicated kernel (gs stays -1: k_up_bwd adds onto the zeroed entries; hoist: k_aux_tail stores them)
    if (t.hoist) for (int j = 0; j < g.U; ++j) gs[g.up_w + j] = -2;      // (the upsampling bias stays -1: zeroed by the reduction, k_aux_tail adds onto it)

    {   // inverse of gsrc for the slab-order reduction, CSR: a slab element feeds one parameter, or several (a gate's conv / aux /
        // past-tap conv biases share one gradient, every layer's skip bias shares one); entries nothing feeds are listed for zeroing
        std::vector<int>& start = t.gdst_start; std::vector<int>& list = t.gdst_list;
        start.assign((size_t)go + 1, 0);
        for (int64_t i = 0; i < g.n_params; ++i) { if (gs[i] >= 0) ++start[(size_t)gs[i] + 1]; else if (gs[i] == -1) t.gzero.push_back(tp_idx(i)); }
        for (int k = 0; k < go; ++k) start[(size_t)k + 1] += start[k];
        list.resize((size_t)start[go] + 1);
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < g.n_params; ++i) if (gs[i] >= 0) list[(size_t)fill[gs[i]]++] = tp_idx(i);
    }
    t.h_ctmap.resize((size_t)2 * Q * C);
    for (int tp = 0; tp < 2; ++tp) for (int q = 0; q < Q; ++q) for (int c = 0; c < C; ++c) t.h_ctmap[((size_t)tp * Q + q) * C + c] = tp_idx(tp_causal_src(g, c, q, tp));
    t.n_map = (int64_t)(use_gemm ? t.h_gmap.size() : t.h_wmap.size()); t.n_gzero = (int)t.gzero.size();
    return t;
}

// ---------------------------------------------------------------- the per-call arena
// ONE carve list: the regions in carve order, each rounded up to 64 floats; `total` is where the list ends, so the size of the workspace and the place of
// every buffer cannot disagree.  Layout facts the kernels rely on (checked by the sweep): DXB starts where DXA's rounded (L + 1) nDX floats end (one memset
// clears both); EB lies directly behind DPA's nPA floats, inside the same carve (zeroed with it); S0 / Y0 carry a tail of one 80-row tile (96 S floats:
// the post-net backward prefetches its masks unclamped).
enum { TA_X, TA_SG, TA_TH, TA_HUP, TA_S0, TA_Y0, TA_DXA, TA_DXB, TA_DZ, TA_DS0, TA_DY0, TA_DGS, TA_DHUP, TA_SLAB, TA_XC, TA_SCRATCH, TA_G, TA_PA, TA_DPA, TA_EB, TA_WJ, TA_GW, TA_COUNT };
struct TrainArena {
    struct Region { size_t off, n; bool on; } r[TA_COUNT];      // floats; on == false: not carved on this path (its pointer is null)
    size_t total;                                               // floats
    float* at(float* base, int i) const { return r[i].on ? base + r[i].off : nullptr; }
};
inline TrainArena train_arena(const TrainLayout& t, const Geom& g, int B, int N1, int BL, int nfr) {
    TrainArena a = {};
    const int C = g.C, S = g.S, L = g.L;
    size_t w = 0;
    auto carve = [&](int i, size_t n) { a.r[i].off = w; a.r[i].n = n; a.r[i].on = true; w += (n + 63) & ~(size_t)63; };
    const size_t nX = (size_t)(L + 1) * B * N1 * C, nG = (size_t)L * B * N1 * C, nH = t.hoist ? 64 : (size_t)B * N1 * t.Ap, nS = (size_t)B * BL * S;
    const size_t nDX = (size_t)B * N1 * C, nDZ = (size_t)B * N1 * 2 * C;
    carve(TA_X, nX); carve(TA_SG, nG); carve(TA_TH, nG); carve(TA_HUP, nH); carve(TA_S0, nS + 96 * (size_t)S); carve(TA_Y0, nS + 96 * (size_t)S);
    carve(TA_DXA, (size_t)(L + 1) * nDX); carve(TA_DXB, (size_t)(L + 1) * nDX);
    carve(TA_DZ, (size_t)L * nDZ); carve(TA_DS0, nS); carve(TA_DY0, nS); carve(TA_DGS, (size_t)B * BL * L * C); carve(TA_DHUP, nH); carve(TA_SLAB, (size_t)t.nch * t.gstage);
    carve(TA_XC, (size_t)B * (N1 + 1));
    carve(TA_SCRATCH, (size_t)B * 1024 * 2 * 128);
    if (t.use_gemm) carve(TA_G, nG);
    if (t.hoist) {
        const size_t nPA = (size_t)L * B * (nfr + 1) * 2 * C, nEB = (size_t)L * TR_EB_SLOTS * 2 * C;
        carve(TA_PA, nPA);
        carve(TA_DPA, nPA + nEB); a.r[TA_DPA].n = nPA; a.r[TA_EB].off = a.r[TA_DPA].off + nPA; a.r[TA_EB].n = nEB; a.r[TA_EB].on = true;
        carve(TA_WJ, (size_t)2 * (N1 + 16)); carve(TA_GW, (size_t)L * B * N1);
    }
    a.total = w;
    return a;
}
