// qpn_geom.h -- the model geometry: where every tensor lives in the flat, state_dict-ordered parameter vector.  Plain C++ (no HIP): qpn_common.h
// includes it for the kernels' translation units, and the pure planners (train_plan.h, decode_program.h) and their stand-alone CPU tests include it alone.
// It also states, once, the flat index of every weight element (tp_*_src at the end).
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/qpnet_hip.h"

#define QPN_MAX_LAYERS 48

void qpn_set_error(const char* fmt, ...);      // (defined in decode.hip; a stand-alone test supplies its own)

#ifdef __HIPCC__
#define QPN_HOST_DEVICE __host__ __device__
#else
#define QPN_HOST_DEVICE
#endif

struct LayerGeom {
    int adaptive;      // 0 fixed, 1 pitch-adaptive
    int dilation;      // 2^k
    // flat offsets (floats) into the state_dict-ordered parameter vector
    // fixed:    convS/convT = (C,C,2) weights (tap0 older), biasS/biasT
    // adaptive: convC/convP per half
    int64_t wS, bS, wT, bT;            // fixed: dil*_sigmoid/tanh .conv.weight/.bias ; adaptive: convC
    int64_t wSP, bSP, wTP, bTP;        // adaptive only: convP
    int64_t auxS, auxSb, auxT, auxTb;  // (C,A,1), (C)
    int64_t skip, skipb, res, resb;    // (S,C,1),(S),(C,C,1),(C)
};

struct Geom {
    qpn_config cfg;
    int C, S, Q, A, U, LF, LA, L;
    int Cp, Sp, Ap;            // K paddings (16 * power of two)
    int recF, recA;
    int64_t causal_w, causal_b, up_w, up_b, post1_w, post1_b, post2_w, post2_b;
    int64_t n_params;
    LayerGeom layers[QPN_MAX_LAYERS];
};

QPN_HOST_DEVICE static inline int qpn_pad_k(int K) { int R = 1; while (16 * R < K) R *= 2; return 16 * R; }

inline int qpn_build_geom(const qpn_config* c, Geom* g) {
    memset(g, 0, sizeof(*g));
    if (!c) { qpn_set_error("null config"); return QPN_EINVAL; }
    g->cfg = *c;
    if (c->kernel_size != 2) { qpn_set_error("kernel_size must be 2 (reference runQP.py always uses 2)"); return QPN_EINVAL; }
    if (c->n_quantize < 2 || c->n_aux < 1 || c->n_resch < 1 || c->n_skipch < 1 || c->upsampling_factor < 0 ||
        c->dilationF_depth < 0 || c->dilationA_depth < 0 || c->dilationF_repeat < 0 || c->dilationA_repeat < 0) {
        qpn_set_error("bad geometry"); return QPN_EINVAL;
    }
    int C = g->C = c->n_resch, S = g->S = c->n_skipch, Q = g->Q = c->n_quantize, A = g->A = c->n_aux;
    g->U = c->upsampling_factor;
    g->LF = c->dilationF_depth * c->dilationF_repeat; g->LA = c->dilationA_depth * c->dilationA_repeat; g->L = g->LF + g->LA;
    if (g->L < 1 || g->L > QPN_MAX_LAYERS) { qpn_set_error("1..%d residual layers supported", QPN_MAX_LAYERS); return QPN_EINVAL; }
    g->Cp = qpn_pad_k(C); g->Sp = qpn_pad_k(S); g->Ap = qpn_pad_k(A);
    int64_t o = 0;
    g->causal_w = o; o += (int64_t)C * Q * 2; g->causal_b = o; o += C;
    if (g->U > 0) { g->up_w = o; o += g->U; g->up_b = o; o += 1; } else { g->up_w = g->up_b = -1; }
    const int64_t convsz = (int64_t)C * C * 2 + C, auxsz = (int64_t)C * A + C, sksz = (int64_t)S * C + S, rssz = (int64_t)C * C + C;
    const int64_t dconv = 2 * ((int64_t)C * C + C);
    int64_t Fs = o; o += g->LF * convsz; int64_t Ft = o; o += g->LF * convsz;
    int64_t Fas = o; o += g->LF * auxsz; int64_t Fat = o; o += g->LF * auxsz;
    int64_t Fsk = o; o += g->LF * sksz; int64_t Frs = o; o += g->LF * rssz;
    int64_t As = o; o += g->LA * dconv; int64_t At = o; o += g->LA * dconv;
    int64_t Aas = o; o += g->LA * auxsz; int64_t Aat = o; o += g->LA * auxsz;
    int64_t Ask = o; o += g->LA * sksz; int64_t Ars = o; o += g->LA * rssz;
    g->post1_w = o; o += (int64_t)S * S; g->post1_b = o; o += S;
    g->post2_w = o; o += (int64_t)Q * S; g->post2_b = o; o += Q;
    g->n_params = o;
    for (int l = 0; l < g->L; ++l) {
        LayerGeom& y = g->layers[l];
        y.adaptive = l >= g->LF;
        int i = y.adaptive ? l - g->LF : l;
        int depth = y.adaptive ? c->dilationA_depth : c->dilationF_depth;
        y.dilation = 1 << (i % depth);
        if (!y.adaptive) {
            y.wS = Fs + i * convsz; y.bS = y.wS + (int64_t)C * C * 2;
            y.wT = Ft + i * convsz; y.bT = y.wT + (int64_t)C * C * 2;
            y.auxS = Fas + i * auxsz; y.auxSb = y.auxS + (int64_t)C * A;
            y.auxT = Fat + i * auxsz; y.auxTb = y.auxT + (int64_t)C * A;
            y.skip = Fsk + i * sksz; y.skipb = y.skip + (int64_t)S * C;
            y.res = Frs + i * rssz; y.resb = y.res + (int64_t)C * C;
        } else {
            y.wS = As + i * dconv; y.bS = y.wS + (int64_t)C * C; y.wSP = y.bS + C; y.bSP = y.wSP + (int64_t)C * C;
            y.wT = At + i * dconv; y.bT = y.wT + (int64_t)C * C; y.wTP = y.bT + C; y.bTP = y.wTP + (int64_t)C * C;
            y.auxS = Aas + i * auxsz; y.auxSb = y.auxS + (int64_t)C * A;
            y.auxT = Aat + i * auxsz; y.auxTb = y.auxT + (int64_t)C * A;
            y.skip = Ask + i * sksz; y.skipb = y.skip + (int64_t)S * C;
            y.res = Ars + i * rssz; y.resb = y.res + (int64_t)C * C;
        }
    }
    g->recF = 0; g->recA = 0;
    for (int l = 0; l < g->L; ++l) (g->layers[l].adaptive ? g->recA : g->recF) += g->layers[l].dilation;
    return QPN_OK;
}

// ---------------------------------------------------------------- where a tensor element lives in the flat parameter vector
// Every index expression of a tensor is stated ONCE, here: the training planner (train_plan.h: forward packs, transposes, gradient map) and the decode planner
// (decode_program.h: every kernel family's gather map) both go through it, so decode reads the parameter training packs and reduces its gradient into.
// gate operand B[k][n] of z = [x_cur | x_past | aux] . W1: input column k, z column n = half * C + r (half 0 sigmoid, 1 tanh); -1 behind the aux columns.
// A fixed layer keeps both taps in one (C, C, 2) tensor (tap 1 current, tap 0 past); an adaptive one has convC / convP
inline int64_t tp_gate_src(const LayerGeom& y, int C, int A, int k, int n) {
    const int half = n / C, r = n % C;
    if (k < C) return y.adaptive ? (half ? y.wT : y.wS) + (int64_t)r * C + k : (half ? y.wT : y.wS) + ((int64_t)r * C + k) * 2 + 1;
    if (k < 2 * C) { const int kk = k - C; return y.adaptive ? (half ? y.wTP : y.wSP) + (int64_t)r * C + kk : (half ? y.wT : y.wS) + ((int64_t)r * C + kk) * 2; }
    if (k < 2 * C + A) return (half ? y.auxT : y.auxS) + (int64_t)r * A + (k - 2 * C);
    return -1;
}
// residual 1x1 B[k][n] = Wr[n][k]; skip 1x1 of all layers stacked along k (k = l * C + c); the two post-net 1x1
inline int64_t tp_res_src(const LayerGeom& y, int C, int k, int n) { return y.res + (int64_t)n * C + k; }
inline int64_t tp_skip_src(const Geom& g, int k, int n) { return g.layers[k / g.C].skip + (int64_t)n * g.C + (k % g.C); }
inline int64_t tp_post1_src(const Geom& g, int k, int n) { return g.post1_w + (int64_t)n * g.S + k; }
inline int64_t tp_post2_src(const Geom& g, int k, int n) { return g.post2_w + (int64_t)n * g.S + k; }
// the biases that add up on gate column n (conv, aux 1x1, and the past-tap conv of an adaptive layer): they share one packed bias and one gradient
inline int tp_gate_bias(const LayerGeom& y, int C, int n, int64_t (&out)[3]) {
    const int half = n / C, r = n % C;
    out[0] = (half ? y.bT : y.bS) + r; out[1] = (half ? y.auxTb : y.auxSb) + r;
    if (!y.adaptive) return 2;
    out[2] = (half ? y.bTP : y.bSP) + r;
    return 3;
}
// THE narrowing of a flat index to the 32 bits the device maps hold (both planners refuse a geometry whose indices do not fit)
inline int tp_idx(int64_t flat) { return (int)flat; }
