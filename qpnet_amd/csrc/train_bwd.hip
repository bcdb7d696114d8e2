// train_bwd.hip -- hand-written backward of QPNet.forward on gfx950 (what torch autograd does for the
// reference at src/bin/qpnet_train.py:529-530), fp32 MFMA.
//
//   k_post_bwd   : dlogits -> dY0 -> dS0 (skip-sum grad) -> per-layer gate grads DGS = dS0 . Ws_l
//   k_layer_bwd  : dXout, DGS -> dg -> (dzs, dzt) -> d[x_cur | x_past | aux] = dZ . W1
//                  x_cur part (+ residual) is stored at its own row; the x_past part is the backward of
//                  the pitch-dependent gather = scatter-add to row tap[n] (float atomics only for the
//                  adaptive blocks; fixed blocks have a unique writer per row)
//   (the weight gradients -- every one a time contraction dW[m][n] = sum_t A[t][m] B[t][n] into partial slabs -- are train_wgrad.hip;
//    their records and which kernel instance each gets: train_wgrad_plan.h.  qpn_launch_bwd below places their launches.)
//   k_causal_bwd : the one-hot causal conv's weight grad is a histogram over sample classes -> LDS table
//   k_up_bwd     : gradient of the (1,1,1,U) upsampling kernel and its bias
//   k_reduce_grad: slabs -> flat gradient in state_dict order
// (the optimiser step that consumes that gradient -- k_adam, k_grad_sumsq, k_grad_accum and their launchers -- is train_adam.hip)
#include "train_common.h"
#include "train_post.h"
#include "qpn_handle.h"
#include <string.h>
#include <stdlib.h>
#include <math.h>

// ------------------------------------------------------------------------------------------ post-net backward
// dynamic LDS: P[TM][lda(max(Q,S))] | R[TM][lda(S)]
template <int MT>
__global__ __launch_bounds__(512) void k_post_bwd(TrainParams p, TrainBwd bw) {
    constexpr int TM = 16 * MT;
    extern __shared__ float sm[];
    const int S = p.S, Q = p.Q, LC = p.LC;
    const int ldp = tr_lda(Q > S ? Q : S), ldr = tr_lda(S);
    float* P = sm; float* R = sm + TM * ldp;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NTS = S / 16;
    // The ReLU masks of the two epilogues (saved pre-activations Y0, S0 at this wave's output positions) are requested AHEAD of the
    // contraction they follow -- Y0 before the staging, S0 before the first contraction -- and pinned with an empty asm in front of
    // it: as plain epilogue loads each of the 8 sat behind its own s_waitcnt (a per-row `if` around load and store), 16 exposed L2
    // round trips per workgroup.  Rows past the chunk end read the arena's padding rows and are masked at the store.
    const int npairs = (NTS + 1) / 2;
    const int np0 = wave < npairs ? wave : 0;
    const int pnt[2] = {2 * np0, (2 * np0 + 1 < NTS) ? 2 * np0 + 1 : 2 * np0};
    float my[2][MT][4], ms[2][MT][4];
    auto mask_load = [&](const float* src, float (&m)[2][MT][4]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = t0 + 16 * mt + 4 * (lane >> 4) + i;      // rows past the chunk end: readable padding (see the arena), masked below
                    m[j][mt][i] = src[((size_t)b * p.BL + r) * S + 16 * pnt[j] + (lane & 15)];
                }
    };
#define PIN8(m) asm volatile("" :: "v"(m[0][0][0]), "v"(m[0][0][1]), "v"(m[0][0][2]), "v"(m[0][0][3]), "v"(m[1][0][0]), "v"(m[1][0][1]), "v"(m[1][0][2]), "v"(m[1][0][3]))
    mask_load(p.Y0, my);
    // stage dlogits rows
    for (int idx = tid; idx < TM * (Q / 2); idx += 512) {
        const int r = idx / (Q / 2), k = (idx - r * (Q / 2)) * 2;
        float2 v = make_float2(0.f, 0.f);
        if (t0 + r < p.BL) v = *(const float2*)(bw.dlogits + ((size_t)b * p.BL + t0 + r) * Q + k);
        *(float2*)(P + (size_t)r * ldp + k) = v;
    }
    __syncthreads();
    mask_load(p.S0, ms);
    PIN8(my);
    if (MT > 1) {
#pragma unroll
        for (int mt = 1; mt < MT; ++mt) asm volatile("" :: "v"(my[0][mt][0]), "v"(my[0][mt][1]), "v"(my[0][mt][2]), "v"(my[0][mt][3]), "v"(my[1][mt][0]), "v"(my[1][mt][1]), "v"(my[1][mt][2]), "v"(my[1][mt][3]));
    }
    // dY0 = (dlogits . W2) * (Y0 > 0)
    for (int pb = 0; pb < npairs; pb += 8) {
        const int np = pb + wave;
        if (np < npairs) {
            const int nt0 = 2 * np, nt1 = (2 * np + 1 < NTS) ? 2 * np + 1 : 2 * np;
            f32x4 acc[MT][2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { acc[mt][0] = (f32x4){0, 0, 0, 0}; acc[mt][1] = (f32x4){0, 0, 0, 0}; }
            const int nts[2] = {nt0, nt1};
            wave_gemm<MT, 2>(acc, P, ldp, p.wp + p.p2t_f4, NTS, nts, Q, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j && nt1 == nt0) break;
                const int c = 16 * (j ? nt1 : nt0) + (lane & 15);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 16 * mt + 4 * (lane >> 4) + i;
                        const bool in = t0 + r < p.BL;
                        const size_t o = ((size_t)b * p.BL + t0 + r) * S + c;
                        const float pre = pb == 0 ? my[j][mt][i] : (in ? p.Y0[o] : 0.f);
                        const float v = (in && pre > 0.f) ? acc[mt][j][i] : 0.f;
                        if (in) bw.DY0[o] = v;
                        R[(size_t)r * ldr + c] = v;
                    }
            }
        }
    }
    __syncthreads();
    PIN8(ms);
    if (MT > 1) {
#pragma unroll
        for (int mt = 1; mt < MT; ++mt) asm volatile("" :: "v"(ms[0][mt][0]), "v"(ms[0][mt][1]), "v"(ms[0][mt][2]), "v"(ms[0][mt][3]), "v"(ms[1][mt][0]), "v"(ms[1][mt][1]), "v"(ms[1][mt][2]), "v"(ms[1][mt][3]));
    }
#undef PIN8
    // dS0 = (dY0 . W1post) * (S0 > 0)   -> P (dlogits are dead)
    for (int pb = 0; pb < npairs; pb += 8) {
        const int np = pb + wave;
        if (np < npairs) {
            const int nt0 = 2 * np, nt1 = (2 * np + 1 < NTS) ? 2 * np + 1 : 2 * np;
            f32x4 acc[MT][2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { acc[mt][0] = (f32x4){0, 0, 0, 0}; acc[mt][1] = (f32x4){0, 0, 0, 0}; }
            const int nts[2] = {nt0, nt1};
            wave_gemm<MT, 2>(acc, R, ldr, p.wp + p.p1t_f4, NTS, nts, S, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j && nt1 == nt0) break;
                const int c = 16 * (j ? nt1 : nt0) + (lane & 15);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 16 * mt + 4 * (lane >> 4) + i;
                        const bool in = t0 + r < p.BL;
                        const size_t o = ((size_t)b * p.BL + t0 + r) * S + c;
                        const float pre = pb == 0 ? ms[j][mt][i] : (in ? p.S0[o] : 0.f);
                        const float v = (in && pre > 0.f) ? acc[mt][j][i] : 0.f;
                        if (in) bw.DS0[o] = v;
                        P[(size_t)r * ldp + c] = v;
                    }
            }
        }
    }
    __syncthreads();
    // DGS[t][l*C + c] = sum_s dS0[t][s] Ws_l[s][c]
    const int NTL = LC / 16, lpairs = (NTL + 1) / 2;
    for (int pb = 0; pb < lpairs; pb += 8) {
        const int np = pb + wave;
        if (np < lpairs) {
            const int nt0 = 2 * np, nt1 = (2 * np + 1 < NTL) ? 2 * np + 1 : 2 * np;
            f32x4 acc[MT][2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { acc[mt][0] = (f32x4){0, 0, 0, 0}; acc[mt][1] = (f32x4){0, 0, 0, 0}; }
            const int nts[2] = {nt0, nt1};
            wave_gemm<MT, 2>(acc, P, ldp, p.wp + p.wst_f4, NTL, nts, S, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j && nt1 == nt0) break;
                const int c = 16 * (j ? nt1 : nt0) + (lane & 15);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 16 * mt + 4 * (lane >> 4) + i;
                        if (t0 + r < p.BL) bw.DGS[((size_t)b * p.BL + t0 + r) * LC + c] = acc[mt][j][i];
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ post-net backward, wide tiles (S = Q = 256, n_resch 64)
// Counterpart of k_post_fwd_w (train_fwd.hip): 16 * MT rows per workgroup (MT = 5: a 20 000-row chunk is one round of 250
// workgroups), the transposed post-net weights stream from L2 once per 80 rows instead of once per 16, one [16 MT][256] LDS
// tile reused in place by the stages, every output array written as whole rows.  The ReLU masks are the signs of the rectified
// activations the forward stored (p.Y0, p.S0), requested ahead of the contraction they follow.
__device__ __forceinline__ void zero_dx_slice(const TrainParams& p, const TrainBwd& bw, int j, int b, size_t part, size_t nparts, int t, int nthr);
// zero_dx: this launch also does k_zero_dx's zeroing (fire-and-forget stores ahead of the first contraction; nothing here touches those
// arrays, the layer backward that does starts after this kernel) -- one launch and two stream events fewer per step
template <int MT>
__global__ __launch_bounds__(512) void k_post_bwd_w(TrainParams p, TrainBwd bw, int zero_dx) {
    if (zero_dx) for (int j = 0; j < p.L; ++j) zero_dx_slice(p, bw, j, blockIdx.y, blockIdx.x, gridDim.x, threadIdx.x, 512);
    extern __shared__ float sm[];
    float4 bq[2];
    post_bwd_w_tile<MT, false>(p, bw, sm, 0ull, 0ull, bq);
}
// Forward (skip sum, post-net, cross entropy) AND backward of a row tile in one kernel, for callers that run both anyway (qpn_train_step): dL/dlogits goes from the cross entropy
// to the first backward contraction through the LDS tile it is already in, the two ReLU masks are 40 sign bits a lane instead of 160 scattered loads, one launch, one prologue
// and the gap between two kernels less (the separate backward alone: 116 -> 104 us without its staging and mask loads).
template <int MT>
__global__ __launch_bounds__(512) void k_post_fb_w(TrainParams p, TrainBwd bw, int zero_dx) {
    if (zero_dx) for (int j = 0; j < p.L; ++j) zero_dx_slice(p, bw, j, blockIdx.y, blockIdx.x, gridDim.x, threadIdx.x, 512);
    extern __shared__ float sm[];
    unsigned long long mS = 0ull, mY = 0ull; float4 bq[2];
    post_fwd_w_tile<MT, true>(p, sm, mS, mY, bq);
    post_bwd_w_tile<MT, true>(p, bw, sm, mS, mY, bq);
}

// ------------------------------------------------------------------------------------------ layer backward
// dynamic LDS: Dx[TM][lda(C)] | Dz[TM][lda(2C)] | Sg, Th, Dg [TM][lda(C)] each
// DXin = grads w.r.t. this layer's OUTPUT (A: own-row part, B: scattered part, both zero-filled where unwritten);
// DXout = grads w.r.t. this layer's INPUT (same two-part form), consumed by layer l-1 / the causal backward.
template <int MT>
__global__ __launch_bounds__(256) void k_layer_bwd(TrainParams p, TrainBwd bw, int l, int last, int pp) {
    constexpr int TM = 16 * MT;
    extern __shared__ float sm[];
    const TrLayer ly = p.layers[l];
    const int C = p.C, Ktp = p.Ktp, Ap = p.Ap;
    const int ldx = tr_lda(C), ldz = tr_lda(2 * C);
    float* Dx = sm; float* Dz = sm + TM * ldx;
    const int b = blockIdx.y, n0 = ly.s_out + tr_xcd_tile(blockIdx.x, gridDim.x, pp & 1) * TM;      // pp: bit 0 XCD swizzle
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t rb = (size_t)b * p.N1;
    const size_t nDX = (size_t)p.B * p.N1 * C;     // grads wrt X[j] live at DXA/DXB[0] + j*nDX
    const float* DAin = bw.DXA[0] + (size_t)(l + 1) * nDX + rb * C; const float* DBin = bw.DXB[0] + (size_t)(l + 1) * nDX + rb * C;
    float* DAout = bw.DXA[0] + (size_t)l * nDX + rb * C; float* DBout = bw.DXB[0] + (size_t)l * nDX + rb * C;
    const int NCG = C / 16;
    // ---- stage dXout (= own-row part + scattered part), the saved gate halves and the skip-path gate grads: 16-byte loads
    float* Sg = Dz + TM * ldz; float* Th = Sg + TM * ldx; float* Dg = Th + TM * ldx;
    const float* SG = p.SG + ((size_t)(l * p.B + b) * p.N1) * C;
    const float* TH = p.TH + ((size_t)(l * p.B + b) * p.N1) * C;
    const int win0 = p.N1 - p.BL;
    // the residual-1x1 fragments of this wave's first n-tile do not depend on the tile: requested before the staging loads, consumed
    // behind the barrier (requested there, their L2 round trip was exposed in front of the first contraction)
    float4 bqr[4][1];
    if (!last) { const int ntr[1] = {wave < NCG ? wave : 0}; wave_b_preload<1, 4>(bqr, p.wp + ly.wrt_f4, NCG, ntr, C, lane); }
    {
        const int C4 = C / 4, tpr = C4 < 64 ? C4 : 64, rpp = 256 / tpr;
        const int tr = tid / tpr, tc = tid - tr * tpr;
        if (tr < rpp)
            for (int r = tr; r < TM; r += rpp) {
                const int n = n0 + r;
                for (int c4 = tc; c4 < C4; c4 += tpr) {
                    const int c = c4 * 4;
                    float4 dx = make_float4(0.f, 0.f, 0.f, 0.f), sg = dx, th = dx, dgs = dx;
                    if (n < p.N1) {
                        if (!last) {
                            const float4 a = *(const float4*)(DAin + (size_t)n * C + c), bb = *(const float4*)(DBin + (size_t)n * C + c);
                            dx = make_float4(a.x + bb.x, a.y + bb.y, a.z + bb.z, a.w + bb.w);
                        }
                        sg = *(const float4*)(SG + (size_t)n * C + c); th = *(const float4*)(TH + (size_t)n * C + c);
                        if (n >= win0) dgs = *(const float4*)(bw.DGS + ((size_t)b * p.BL + (n - win0)) * p.LC + (size_t)l * C + c);
                    }
                    float* d0 = Dx + (size_t)r * ldx + c; *(float2*)d0 = make_float2(dx.x, dx.y); *(float2*)(d0 + 2) = make_float2(dx.z, dx.w);
                    float* d1 = Sg + (size_t)r * ldx + c; *(float2*)d1 = make_float2(sg.x, sg.y); *(float2*)(d1 + 2) = make_float2(sg.z, sg.w);
                    float* d2 = Th + (size_t)r * ldx + c; *(float2*)d2 = make_float2(th.x, th.y); *(float2*)(d2 + 2) = make_float2(th.z, th.w);
                    float* d3 = Dg + (size_t)r * ldx + c; *(float2*)d3 = make_float2(dgs.x, dgs.y); *(float2*)(d3 + 2) = make_float2(dgs.z, dgs.w);
                }
            }
    }
    __syncthreads();
    // ---- dg = dXout . Wr + DGS ; dz = dg * gate'
    float* DZg = bw.DZ + ((size_t)l * p.B * p.N1 + rb) * 2 * C;
    for (int nt = wave; nt < NCG; nt += 4) {
        f32x4 acc[MT][1];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][0] = (f32x4){0, 0, 0, 0};
        if (!last) {
            const int nts[1] = {nt};
            if (nt == wave) wave_gemm_run<MT, 1, 4>(acc, Dx, ldx, bqr, p.wp + ly.wrt_f4, NCG, nts, C, lane);
            else wave_gemm_deep<MT, 1, 4>(acc, Dx, ldx, p.wp + ly.wrt_f4, NCG, nts, C, lane);
        }
        const int c = 16 * nt + (lane & 15);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * mt + 4 * (lane >> 4) + i, n = n0 + r;
                const float dg = acc[mt][0][i] + Dg[(size_t)r * ldx + c];
                const float sg = Sg[(size_t)r * ldx + c], th = Th[(size_t)r * ldx + c];
                float dzs, dzt; tr_gate_bwd(dg, sg, th, dzs, dzt);      // (th: the gate product the Th tile holds)
                if (n < p.N1) { DZg[(size_t)n * 2 * C + c] = dzs; DZg[(size_t)n * 2 * C + C + c] = dzt; }
                Dz[(size_t)r * ldz + c] = dzs; Dz[(size_t)r * ldz + C + c] = dzt;
            }
    }
    // ---- d[x_cur | x_past | aux] = dZ . W1.  A wave's n-tiles run back to back; the weight fragments of the NEXT n-tile and the
    //      scatter rows are requested before the barrier / under the previous tile's epilogue (K = 2C <= 128: all 8 steps fit the ring)
    const int NTK = Ktp / 16;
    const int* taps = p.TAP + ly.tap_off + (size_t)b * p.N1;      // a table for every layer (k_train_prep)
    float* DH = bw.DHUP + rb * Ap;
    constexpr int PD3 = 8;
    const float4* W1t = p.wp + ly.w1t_f4;
    float4 bq[PD3][1];
    int tprow[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 16 * mt + 4 * (lane >> 4) + i;
            tprow[mt][i] = taps[n < p.N1 ? n : p.N1 - 1];
        }
    if (wave < NTK) { const int nts0[1] = {wave}; wave_b_preload<1, PD3>(bq, W1t, NTK, nts0, 2 * C, lane); }
    __syncthreads();
    for (int nt = wave; nt < NTK; nt += 4) {
        f32x4 acc[MT][1];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][0] = (f32x4){0, 0, 0, 0};
        const int nts[1] = {nt};
        wave_gemm_run<MT, 1, PD3>(acc, Dz, ldz, bq, W1t, NTK, nts, 2 * C, lane);
        if (2 * C <= 16 * PD3 && nt + 4 < NTK) { const int ntn[1] = {nt + 4}; wave_b_preload<1, PD3>(bq, W1t, NTK, ntn, 2 * C, lane); }
        const int k = 16 * nt + (lane & 15);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * mt + 4 * (lane >> 4) + i, n = n0 + r;
                if (n >= p.N1) continue;
                const float v = acc[mt][0][i];
                if (k < C) DAout[(size_t)n * C + k] = v + Dx[(size_t)r * ldx + k];              // + residual path
                else if (k < 2 * C) {
                    if (ly.adaptive) atomicAdd(&DBout[(size_t)tprow[mt][i] * C + (k - C)], v);          // gather backward (collisions)
                    else DBout[(size_t)tprow[mt][i] * C + (k - C)] = v;                           // unique writer
                } else if (k < 2 * C + Ap) atomicAdd(&DH[(size_t)n * Ap + (k - 2 * C)], v);      // unique writer per layer, layers in order: fire-and-forget add
            }
        if (!(2 * C <= 16 * PD3) && nt + 4 < NTK) { const int ntn[1] = {nt + 4}; wave_b_preload<1, PD3>(bq, W1t, NTK, ntn, 2 * C, lane); }
    }
}

// ------------------------------------------------------------------------------------------ layer backward, persistent form (n_resch = 64)
// Same arithmetic as k_layer_bwd, organised like k_layer_fwd_p (train_fwd.hip): 2 workgroups per CU walk contiguous ranges of
// 16-row tiles with the layer's TRANSPOSED weights resident in registers -- wave w owns column tile w of dg = dXout . Wr and
// column tiles {w, w + 4, w + 8} of d[x_cur | x_past | aux] = dZ . W1 (4 + 3 x 8 fragment float4s per lane) -- the next tile's
// rows (dXout parts, saved gate halves, skip-path gate grads) and scatter targets in flight under the current tile, a branch-free
// tile loop (clamped loads, out-of-range stores redirected to a scratch row: exact s_waitcnt vmcnt counts), LDS-only barriers,
// all fragment reads ahead of their MFMAs.  Both results leave through LDS as whole rows: dZ (512 B rows), the own-row input
// gradient (+ residual path), the pitch-tap part as one 256-byte row per tap row -- a plain store for the fixed blocks (unique
// writer), ONE full-row float-atomic instruction per row for the adaptive blocks (the accumulator layout gave 64-byte strips
// of four different rows per instruction) -- and the aux columns as row-contiguous atomics.
template <int NTK, bool LAST>      // NTK = Ktp / 16 column tiles of the input gradient (11 for n_resch 64, n_aux 39)
__global__ __launch_bounds__(256, 2) void k_layer_bwd_p(TrainParams p, TrainBwd bw, int l, int flags, int tiles, float* dummy) {     // flags: bit 1 XCD swizzle
    constexpr int C = 64;
    constexpr int ldx = ((C + 29) / 32) * 32 + 2, ldz = ((2 * C + 29) / 32) * 32 + 2, ldo = ((16 * NTK + 29) / 32) * 32 + 2;
    constexpr int NJ = (NTK + 3) / 4;                              // column tiles of the second contraction per wave
    constexpr bool HOIST = NTK == 8;                               // the auxiliary 1x1 at frame rate (TrainParams::hoist): D / G instead of the aux columns (train_common.h, tr_aux_bwd)
    extern __shared__ float sm[];
    // two staging buffers {Dx | Sg | Th | Dg}, [16][ldx] each; Dz [16][ldz]; Os [16][ldo] (the second contraction's outputs); hoist: Gp [4][16]
    float* Dz = sm + 8 * 16 * ldx;
    float* Os = Dz + 16 * ldz;
    float* Gp = Os + 16 * ldo;
    const TrLayer ly = p.layers[l];
    const int Ap = p.Ap, N1 = p.N1;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    int t_first, t_count;
    tr_tile_range(blockIdx.x, gridDim.x, tiles, flags & 2, t_first, t_count);
    if (t_count <= 0) return;
    const int t_last = t_first + t_count - 1;
    const size_t rb = (size_t)b * N1;
    const size_t nDX = (size_t)p.B * N1 * C;
    const float* DAin = bw.DXA[0] + (size_t)(l + 1) * nDX + rb * C; const float* DBin = bw.DXB[0] + (size_t)(l + 1) * nDX + rb * C;
    float* DAout = bw.DXA[0] + (size_t)l * nDX + rb * C; float* DBout = bw.DXB[0] + (size_t)l * nDX + rb * C;
    const float* SG = p.SG + ((size_t)(l * p.B + b) * N1) * C;
    const float* TH = p.TH + ((size_t)(l * p.B + b) * N1) * C;
    const int win0 = N1 - p.BL;
    const float* DGS = bw.DGS + (size_t)b * p.BL * p.LC + (size_t)l * C;
    float* DZg = bw.DZ + ((size_t)l * p.B * N1 + rb) * 2 * C;
    float* DH = HOIST ? nullptr : bw.DHUP + rb * Ap;
    float* GWl = HOIST ? bw.GW + (size_t)(l * p.B + b) * N1 : nullptr;
    const int* taps = p.TAP + ly.tap_off + rb;
    // ---- resident weight fragments
    const float4* Wrt = p.wp + ly.wrt_f4; const float4* W1t = p.wp + ly.w1t_f4;
    float4 wr[4], w1[NJ][8];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) wr[ks] = LAST ? make_float4(0.f, 0.f, 0.f, 0.f) : Wrt[((size_t)ks * 4 + wave) * 64 + lane];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int nt = wave + 4 * j < NTK ? wave + 4 * j : NTK - 1;          // (a wave without a j-th tile keeps a copy it never uses)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w1[j][ks] = W1t[((size_t)ks * NTK + nt) * 64 + lane];
    }
    // ---- staging in: thread -> (row srow, 16-byte piece sc4) of the four [16][C] arrays
    const int srow = tid >> 4, sc4 = tid & 15;
    float4 ra, rb2, rsg, rth, rdg;
    auto load_rows = [&](int t) {
        const int n = ly.s_out + t * 16 + srow;
        const int nn = n < N1 ? n : N1 - 1;
        // 32-bit element offsets (one batch item's rows x channels fit easily; the batch part is in the bases): one full-rate multiply and
        // the SAME offset register behind four uniform bases, instead of a 64-bit multiply-add and a 64-bit add per load
        const unsigned o = __umul24((unsigned)nn, (unsigned)C) + 4u * sc4;
        ra = *(const float4*)(DAin + o); rb2 = *(const float4*)(DBin + o);          // (rows of the last layer: finite garbage, not used)
        rsg = *(const float4*)(SG + o); rth = *(const float4*)(TH + o);
        const int nw = nn >= win0 ? nn - win0 : 0;
        rdg = *(const float4*)(DGS + (__umul24((unsigned)nw, (unsigned)p.LC) + 4u * sc4));
    };
    auto store_rows = [&](int t, float* B) {
        const int n = ly.s_out + t * 16 + srow;
        const bool in = n < N1;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 dx = (in && !LAST) ? make_float4(ra.x + rb2.x, ra.y + rb2.y, ra.z + rb2.z, ra.w + rb2.w) : z;
        const float4 sg = in ? rsg : z, th = in ? rth : z, dg = (in && n >= win0) ? rdg : z;
        float* d0 = B + (size_t)srow * ldx + 4 * sc4;
        *(float2*)d0 = make_float2(dx.x, dx.y); *(float2*)(d0 + 2) = make_float2(dx.z, dx.w);
        float* d1 = d0 + 16 * ldx; *(float2*)d1 = make_float2(sg.x, sg.y); *(float2*)(d1 + 2) = make_float2(sg.z, sg.w);
        float* d2 = d1 + 16 * ldx; *(float2*)d2 = make_float2(th.x, th.y); *(float2*)(d2 + 2) = make_float2(th.z, th.w);
        float* d3 = d2 + 16 * ldx; *(float2*)d3 = make_float2(dg.x, dg.y); *(float2*)(d3 + 2) = make_float2(dg.z, dg.w);
    };
    // ---- staging out.  dZ: thread -> 8-byte pieces (rows zrow, zrow + 4, + 8, + 12; column zc2) of the [16][128] tile;
    //      input gradient: wave w owns rows 4w .. 4w+3, lane = channel: one 256-byte row per instruction
    const int zrow = tid >> 6, zc2 = (tid & 63) * 2;
    float* const dmy = dummy + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 2 * 128;       // two 512-byte scratch rows per workgroup
    int tprow[4], tpnext[4];
    auto load_taps = [&](int t, int (&tp)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int n = ly.s_out + t * 16 + 4 * wave + i; tp[i] = taps[n < N1 ? n : N1 - 1]; }
    };
    // aux hoist: the WJ entries of this lane's four dZ rows and its four PA values -- c*: the tile in hand, n*: the next tile's, in flight
    float2 cwj[4], nwj[4]; float cpa[4], npa[4]; int cpoff = 0, npoff = 0;
    auto load_aux = [&](int t, float2 (&wj)[4], float (&pa)[4], int& poff) {
        const int n0 = ly.s_out + t * 16;
        poff = tr_pa_off(p, l, b, n0);
        const float2* w = p.WJ + n0 + 4 * (lane >> 4);             // (16 rows of padding behind row N1 - 1)
        const float* q4 = p.PA + poff + 16 * wave + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) wj[i] = w[i];
        pa[0] = q4[0]; pa[1] = q4[C]; pa[2] = q4[2 * C]; pa[3] = q4[3 * C];
    };
    load_rows(t_first);
    if constexpr (HOIST) load_aux(t_first, cwj, cpa, cpoff);
    load_taps(t_first, tprow);
    store_rows(t_first, sm);
    const int arow = lane & 15, ak = lane >> 4;
    const int c = 16 * wave + (lane & 15);
    for (int ti = 0; ti < t_count; ++ti) {
        const int t = t_first + ti, n0 = ly.s_out + t * 16;
        float* Dx = sm + (ti & 1) * 4 * 16 * ldx; float* Sg = Dx + 16 * ldx; float* Th = Sg + 16 * ldx; float* Dg = Th + 16 * ldx;
        { const int tn = t + 1 < t_last ? t + 1 : t_last; load_rows(tn); load_taps(tn, tpnext); if constexpr (HOIST) load_aux(tn, nwj, npa, npoff); }      // (past the range: a harmless reload)
        TR_LDS_BARRIER();                                          // this tile's staged rows complete; Dz / Os free (readers: previous trip)
        // ---- dg = dXout . Wr + DGS ; dz = dg * gate'
        float xa[4][4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { const float* ap = Dx + (size_t)arow * ldx + 16 * ks + ak; xa[ks][0] = ap[0]; xa[ks][1] = ap[4]; xa[ks][2] = ap[8]; xa[ks][3] = ap[12]; }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 a0 = (f32x4){0, 0, 0, 0}, a1 = (f32x4){0, 0, 0, 0};
        if (!LAST) {
#pragma unroll
            for (int ks = 0; ks < 4; ks += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks][0], wr[ks].x, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks + 1][0], wr[ks + 1].x, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks][1], wr[ks].y, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks + 1][1], wr[ks + 1].y, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks][2], wr[ks].z, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks + 1][2], wr[ks + 1].z, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks][3], wr[ks].w, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks + 1][3], wr[ks + 1].w, a1, 0, 0, 0);
            }
        }
        float dzs[4], dzt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * (lane >> 4) + i;
            const float dg = (a0[i] + a1[i]) + Dg[(size_t)r * ldx + c];
            const float sg = Sg[(size_t)r * ldx + c], th = Th[(size_t)r * ldx + c];
            tr_gate_bwd(dg, sg, th, dzs[i], dzt[i]);              // (th: the gate product the Th tile holds)
            Dz[(size_t)r * ldz + c] = dzs[i];
            Dz[(size_t)r * ldz + C + c] = dzt[i];
        }
        float dacc[4] = {0.f, 0.f, 0.f, 0.f}, eacc[2] = {0.f, 0.f};
        if constexpr (HOIST) {      // the frame-rate aux term's backward (same arithmetic as k_stack_bwd)
            const TrAuxBwd ab = tr_aux_bwd(cwj, cpa, dzs, dzt, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) dacc[k] = ab.d[k];
            eacc[0] = ab.e[0]; eacc[1] = ab.e[1];
            if ((lane & 15) == 0) { float* gq = Gp + 16 * wave + 4 * (lane >> 4); gq[0] = ab.gp[0]; gq[1] = ab.gp[1]; gq[2] = ab.gp[2]; gq[3] = ab.gp[3]; }
        }
        TR_LDS_BARRIER();
        // ---- d[x_cur | x_past | aux] = dZ . W1
        float za[8][4];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) { const float* zp = Dz + (size_t)arow * ldz + 16 * ks + ak; za[ks][0] = zp[0]; za[ks][1] = zp[4]; za[ks][2] = zp[8]; za[ks][3] = zp[12]; }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[ks][0], w1[j][ks].x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[ks][1], w1[j][ks].y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[ks][2], w1[j][ks].z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[ks][3], w1[j][ks].w, acc[j], 0, 0, 0);
        }
        {   // dZ rows to global (512 B each), under the contraction: thread -> rows zrow + 4k, 8-byte piece zc2
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = zrow + 4 * k;
                float* d = DZg + (__umul24((unsigned)(n0 + r), 2u * C) + zc2);
                d = n0 + r < N1 ? d : dmy + zc2;
                *(float2*)d = *(const float2*)(Dz + (size_t)r * ldz + zc2);
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int nt = wave + 4 * j;
            if (nt >= NTK) continue;                               // wave-uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) Os[(size_t)(4 * (lane >> 4) + i) * ldo + 16 * nt + (lane & 15)] = acc[j][i];
        }
        TR_LDS_BARRIER();
        // ---- outputs as whole rows: wave w owns rows 4w .. 4w+3, lane = channel
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * wave + i, n = n0 + r;
            const bool in = n < N1;
            const float own = Os[(size_t)r * ldo + lane] + Dx[(size_t)r * ldx + lane];                 // + residual path
            float* da = DAout + (__umul24((unsigned)n, (unsigned)C) + lane);
            *(in ? da : dmy + lane) = own;
            const float past = Os[(size_t)r * ldo + C + lane];
            float* db = DBout + (__umul24((unsigned)tprow[i], (unsigned)C) + lane);
            db = in ? db : dmy + 128 + lane;
            if (ly.adaptive) atomicAdd(db, past);                                                       // gather backward (collisions)
            else *db = past;                                                                            // unique writer
            if constexpr (!HOIST) if (lane < Ap) {                                                      // (Ap <= 64)
                float* dh = DH + (__umul24((unsigned)n, (unsigned)Ap) + lane);
                atomicAdd(in ? dh : dmy + 192 + lane, Os[(size_t)r * ldo + 2 * C + lane]);               // unique writer per layer, layers in order
            }
        }
        if constexpr (HOIST) {      // D_l[frame][gate row] += this tile's share; the tile's 16 G values
            if (lane < 16) {
                float* dp = bw.DPA + cpoff + 16 * wave + lane;
                atomicAdd(dp, dacc[0]); atomicAdd(dp + C, dacc[1]); atomicAdd(dp + 2 * C, dacc[2]); atomicAdd(dp + 3 * C, dacc[3]);
                float* ep = bw.EB + (size_t)(l * TR_EB_SLOTS + (blockIdx.x & (TR_EB_SLOTS - 1))) * 2 * C + 16 * wave + lane;
                atomicAdd(ep, eacc[0]); atomicAdd(ep + C, eacc[1]);
            }
            if (tid < 16 && n0 + tid < N1) GWl[n0 + tid] = (Gp[tid] + Gp[16 + tid]) + (Gp[32 + tid] + Gp[48 + tid]);
        }
        store_rows(t + 1 < t_last ? t + 1 : t_last, sm + ((ti + 1) & 1) * 4 * 16 * ldx);
#pragma unroll
        for (int i = 0; i < 4; ++i) tprow[i] = tpnext[i];
        if constexpr (HOIST) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { cwj[i] = nwj[i]; cpa[i] = npa[i]; }
            cpoff = npoff;
        }
    }
}

// ------------------------------------------------------------------------------------------ upsampling kernel
// upsampling kernel grad: dw[j] = sum_{a,f} dH[a, U f + j] h[a,f];  db = sum dH   (qpnet.py:134-158)
// One workgroup per (frame, batch item): thread j < U owns sample U f + j of the frame, reads its dH row (Ap contiguous floats: the
// workgroup's reads are one contiguous U*Ap*4-byte block) and dots it with the frame's feature column held in LDS; one global atomic per
// (j, frame) instead of an LDS atomic per element (the element-wise version was 20 us for 3.8 MB: contended LDS atomics on 110 bins).
struct UpArgs { const float* h; const float* DHUP; float* gflat; int64_t up_w, up_b; float gscale; int U, Ap, A, F, N1, nfr, B; };
static UpArgs up_args(const TrainParams& p, const TrainBwd& bw) {
    UpArgs u; u.h = p.h; u.DHUP = bw.DHUP; u.gflat = bw.gflat; u.gscale = bw.gscale; u.U = p.U; u.Ap = p.Ap; u.A = p.A; u.F = p.F; u.N1 = p.N1;
    u.up_w = p.up_w; u.up_b = p.up_b; u.B = p.B;
    const int64_t q0 = (int64_t)p.F * p.U - p.N1;
    u.nfr = p.U > 0 ? (int)(((int64_t)p.F * p.U - 1) / p.U - q0 / p.U + 1) : 0;       // frames that the N1 rows touch
    return u;
}
// fx: frame (counted from the first one the rows touch), b: batch item; nthr threads (a multiple of 64, <= 256), all of which call this
__device__ __forceinline__ void up_bwd_body(const UpArgs& p, int fx, int b, int tid, int nthr) {
    __shared__ float hcol[64];
    __shared__ float red[4];
    const int U = p.U, Ap = p.Ap, A = p.A;
    const int64_t q0 = (int64_t)p.F * U - p.N1;           // h_up sample index of row 0
    const int f = (int)(q0 / U) + fx;                     // frames touched: f0 .. f0 + nfr - 1
    float dsum = 0.f;
    for (int a0 = 0; a0 < A; a0 += 64) {                  // (one pass for the usual 39 features)
        __syncthreads();
        if (tid < 64) hcol[tid] = (a0 + tid < A && f < p.F) ? p.h[((size_t)b * A + a0 + tid) * p.F + f] : 0.f;
        __syncthreads();
        for (int j = tid; j < U; j += nthr) {
            const int64_t n = (int64_t)f * U + j - q0;    // local row
            if (n < 0 || n >= p.N1 || f >= p.F) continue;
            const float* row = p.DHUP + ((size_t)b * p.N1 + n) * Ap + a0;
            float acc = 0.f;
            const int na = A - a0 < 64 ? A - a0 : 64;
            // the row's (up to 16) float4 words requested TOGETHER, then summed: with a run-time trip count the loop was load -> wait -> add
            // per word, ten memory latencies in a row -- 73 us beside the memory-bound dW1 launch (11 us alone)
            const int nq = na >> 2;
            float4 v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = *(const float4*)(row + 4 * (q < nq ? q : 0));
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < nq) { acc += v[q].x * hcol[4 * q] + v[q].y * hcol[4 * q + 1] + v[q].z * hcol[4 * q + 2] + v[q].w * hcol[4 * q + 3]; dsum += (v[q].x + v[q].y) + (v[q].z + v[q].w); }
            for (int a = 4 * nq; a < na; ++a) { const float v1 = row[a]; acc += v1 * hcol[a]; dsum += v1; }
            atomicAdd(&p.gflat[p.up_w + j], acc * p.gscale);
        }
    }
    for (int s = 32; s >= 1; s >>= 1) dsum += __shfl_xor(dsum, s);
    if ((tid & 63) == 0) red[tid >> 6] = dsum;
    __syncthreads();
    if (tid == 0) { float a = 0.f; for (int k = 0; k < nthr / 64; ++k) a += red[k]; atomicAdd(&p.gflat[p.up_b], a * p.gscale); }
}


// ------------------------------------------------------------------------------------------ small backward kernels
// Slabs -> flat gradient, walked in SLAB order: a wave reads 64 consecutive floats of each partial slab (the flat order is a
// permutation of it -- transposed blocks, interleaved taps -- so a gather in flat order touches scattered 4-byte words of 64 slabs),
// and the sum goes to the parameter(s) it feeds; entries nothing feeds are zeroed, the trailer appended.
// [s0, s1): the slab elements this launch reduces (the early range runs on the side stream under the layer backward); `tail`: this launch
// also zeroes the unfed entries and appends the trailer
__global__ void k_reduce_grad_s(const float* __restrict__ slab, const int* __restrict__ gdst, const int* __restrict__ gdst_list, const int* __restrict__ gzero, int n_gzero,
                                int nch, int gstage, int64_t n, float* __restrict__ g, float scale, int append_scale, int s0, int s1, int skip0, int skip1, int tail,
                                const int* __restrict__ status, int flag_again) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + s0;
    // trailer word 1 = "this rank's step is flagged" (the sticky status word, as a float): summed by the gradient exchange, so that EVERY rank's Adam kernel
    // skips the update of a step one rank flagged (k_adam).  flag_again: the backward's LAST launch writes it once more -- the trailer itself may have been appended
    // by the early launch on the side stream, before the stack backward could set its own bit -- unless the trailer has left with an early exchange bucket already
    if (flag_again && append_scale && i == s0) g[n + 1] = (status && *status) ? 1.f : 0.f;
    if (i < s1) {
        if (i >= skip0 && i < skip1) return;                 // (already reduced by the early launch)
        const int k0 = gdst[i], k1 = gdst[i + 1];
        if (k0 == k1) return;                                // padding of the slab layout
        // eight slabs' words requested together (the one-at-a-time sum kept ~4 loads in flight per lane: 29 us for 61 MB)
        float a = 0.f;
        const float* sp = slab + i;
        int c = 0;
        for (; c + 8 <= nch; c += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = sp[(size_t)(c + k) * gstage];
            a += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
        for (; c < nch; ++c) a += sp[(size_t)c * gstage];
        a *= scale;
        for (int k = k0; k < k1; ++k) g[gdst_list[k]] = a;
        return;
    }
    if (!tail) return;
    const int64_t j = i - s1;
    if (j < n_gzero) g[gzero[j]] = 0.f;
    else if (append_scale && j < n_gzero + 4 && !(flag_again && j == n_gzero + 1)) g[n + (j - n_gzero)] = j == n_gzero ? scale : (j == n_gzero + 1 && status && *status) ? 1.f : 0.f;
}

// causal conv weight grad: dW[c][q][tap] = sum over rows whose sample == q; LDS table per channel block
__global__ __launch_bounds__(256) void k_causal_bwd(TrainParams p, TrainBwd bw, int rows_per_wg, int CB) {
    extern __shared__ float tab[];                 // [2][Q][CB]; CB: channels per pass (64, fewer when the class count is large: the table stays within 128 KB)
    const int C = p.C, Q = p.Q;
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)p.B * p.N1;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < total ? r0 + rows_per_wg : total;
    for (int cb = 0; cb < C; cb += CB) {
        const int cbv = C - cb < CB ? C - cb : CB;          // channels of this block (the last one is partial when C % 64 != 0)
        for (int i = tid; i < 2 * Q * CB; i += 256) tab[i] = 0.f;
        __syncthreads();
        const int cpr = cbv;                         // channels per row handled by consecutive threads
        for (int64_t idx = r0 * cpr + tid; idx < r1 * cpr; idx += 256) {
            const int64_t rr = idx / cpr; const int c = (int)(idx - rr * cpr);
            const int b = (int)(rr / p.N1), n = (int)(rr - (int64_t)b * p.N1);
            const size_t o = ((size_t)b * p.N1 + n) * C + cb + c;
            const float v = bw.DXA[0][o] + bw.DXB[0][o];   // after the layer-0 backward the result sits in parity 0 (see launcher)
            const int64_t xo = (int64_t)p.T - p.N0 + n;
            int64_t s0 = p.x[(size_t)b * p.T + xo] % Q, s1 = p.x[(size_t)b * p.T + xo + 1] % Q;
            if (s0 < 0) s0 += Q;
            if (s1 < 0) s1 += Q;
            atomicAdd(&tab[(0 * Q + s0) * CB + c], v);
            atomicAdd(&tab[(1 * Q + s1) * CB + c], v);
        }
        __syncthreads();
        // flush: flat index ((c*Q + q)*2 + tap); iterate (q,tap) fastest for contiguous atomics
        for (int i = tid; i < 2 * Q * cbv; i += 256) {
            const int c = i / (2 * Q), qt = i - c * 2 * Q, q = qt >> 1, tp = qt & 1;
            const float v = tab[(tp * Q + q) * CB + c];
            if (v != 0.f) atomicAdd(&bw.gflat[p.causal_w + ((size_t)(cb + c) * Q + q) * 2 + tp], v * bw.gscale);
        }
        // bias grad = sum over all rows = sum over q of the tap-0 table
        for (int c = tid; c < cbv; c += 256) {
            float s = 0.f;
            for (int q = 0; q < Q; ++q) s += tab[(0 * Q + q) * CB + c];
            atomicAdd(&bw.gflat[p.causal_b + cb + c], s * bw.gscale);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(128) void k_up_bwd(UpArgs u) { up_bwd_body(u, blockIdx.x, blockIdx.y, threadIdx.x, 128); }

// Aux hoist: the gradients the frame-rate form leaves to a kernel of its own, from what the layer backward accumulated: D (DPA), G (GW) and
// the gate-bias gradient E_l[n] = colsum(dZ_l) (EB).  With h_up[a][U f + j] = h[a][f] w_up[j] + b_up (reference src/nets/qpnet.py:134-158) and
// z_l[t] += Va_l . h_up[:, t] + ba_l (qpnet.py:215-216, 663-664):
//   role A, blocks [0, L A):        dVa_l[n][a] = sum_{b, f} D_l[b][f][n] h[b][a][f] + b_up E_l[n]          (D_l[b][f][n] = sum_{t in f} w_up[j(t)] dZ_l[t][n])
//                                   db_up      += sum_n Va_l[n][a] E_l[n]                                    (one atomic per block onto the entry the reduction zeroed)
//   role B, blocks [L A, L A + U):  dw_up[j]    = sum_{l, b, t: j(t) = j, t >= s_out(l)} G_l[b][t]          (G_l[b][t] = sum_n dZ_l[t][n] (Va_l . h[b][:, f(t)])[n])
// It needs nothing of the weight-gradient launches: it runs on the side stream next to them.
__global__ __launch_bounds__(128) void k_aux_tail(AuxArgs p) {
    __shared__ float hrow[1024];
    __shared__ float red[2];
    const AuxGeom& ag = p.g;
    const int C = p.C, A = p.A, L = p.L, tid = threadIdx.x;
    const int bx = blockIdx.x;
    float v = 0.f;
    const bool role_a = bx < L * A;
    if (role_a) {
        const int l = bx / A, a = bx - l * A, n = tid;    // (128 threads = 2C gate rows)
        const size_t wi = (n < C ? ag.auxS[l] + (size_t)n * A : ag.auxT[l] + (size_t)(n - C) * A) + a;
        const float va = p.flat[wi];
        float e = 0.f;
        {
            float ev[TR_EB_SLOTS];
#pragma unroll
            for (int k = 0; k < TR_EB_SLOTS; ++k) ev[k] = p.EB[(size_t)(l * TR_EB_SLOTS + k) * 2 * C + n];
#pragma unroll
            for (int k = 0; k < TR_EB_SLOTS; ++k) e += ev[k];
        }
        float acc = 0.f;
        for (int b = 0; b < p.B; ++b) {
            const float* hb = p.h + ((size_t)b * A + a) * p.F + p.ffirst;
            const float* D = p.DPA + (size_t)(l * p.B + b) * (p.nfr + 1) * 2 * C + n;
            for (int f0 = 0; f0 < p.nfr; f0 += 1024) {
                const int nf = p.nfr - f0 < 1024 ? p.nfr - f0 : 1024;
                __syncthreads();
                for (int i = tid; i < nf; i += 128) hrow[i] = hb[f0 + i];
                __syncthreads();
                int f = 0;
                for (; f + 64 <= nf; f += 64) {           // 64 rows requested together (the loop is a chain of memory round trips otherwise)
                    float d[64];
#pragma unroll
                    for (int k = 0; k < 64; ++k) d[k] = D[(size_t)(f0 + f + k) * 2 * C];
#pragma unroll
                    for (int k = 0; k < 64; ++k) acc += d[k] * hrow[f + k];
                }
                for (; f + 16 <= nf; f += 16) {
                    float d[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) d[k] = D[(size_t)(f0 + f + k) * 2 * C];
#pragma unroll
                    for (int k = 0; k < 16; ++k) acc += d[k] * hrow[f + k];
                }
                for (; f < nf; ++f) acc += D[(size_t)(f0 + f) * 2 * C] * hrow[f];
            }
        }
        p.gflat[wi] = (acc + p.flat[p.up_b] * e) * p.gscale;
        v = va * e;
    } else {
        const int j = bx - L * A;
        const int q0 = p.F * p.U - p.N1;                 // h_up sample index of row 0
        const int items = L * p.B * p.nfr;
        for (int it = tid; it < items; it += 128) {
            const int fx = it % p.nfr, lb = it / p.nfr, l = lb / p.B;
            const int n = (p.ffirst + fx) * p.U + j - q0;
            if (n >= ag.s_out[l] && n < p.N1) v += p.GW[(size_t)lb * p.N1 + n];
        }
    }
    for (int sft = 32; sft >= 1; sft >>= 1) v += __shfl_xor(v, sft);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        if (role_a) atomicAdd(p.gflat + p.up_b, (red[0] + red[1]) * p.gscale);
        else p.gflat[p.up_w + (bx - L * A)] = (red[0] + red[1]) * p.gscale;
    }
}

// Zero exactly what the backward reads without having written it.  Grad wrt X[j] has two parts:
//   DXA[j] (own-row part): layer j writes rows [s_out(j), N1); layer j-1 (or the causal backward for j = 0) reads from
//           row s_in(j) (0 for j = 0) -> rows [s_in(j) or 0, s_out(j)) must read as zero;
//   DXB[j] (pitch-tap scatter part): a fixed layer is the unique writer of rows [s_in(j), N1 - dilation), so only the last
//           `dilation` rows (and, for j = 0, nothing in front) need zeros; an adaptive layer adds with atomics -> all rows.
// X[L]'s gradient is never read (the last block's residual output is unused, qpnet.py:306-309).
// part / nparts: the slice of (layer j, batch item b)'s zeroing this caller does, with nthr threads of which this is thread t
__device__ __forceinline__ void zero_dx_slice(const TrainParams& p, const TrainBwd& bw, int j, int b, size_t part, size_t nparts, int t, int nthr) {
    const int C = p.C;
    const TrLayer ly = p.layers[j];
    const size_t nDX = (size_t)p.B * p.N1 * C;
    float* A = bw.DXA[0] + (size_t)j * nDX + (size_t)b * p.N1 * C;
    float* Bq = bw.DXB[0] + (size_t)j * nDX + (size_t)b * p.N1 * C;
    const int a0 = j == 0 ? 0 : ly.s_in, a1 = ly.s_out;
    const int b0 = ly.adaptive ? 0 : p.N1 - ly.dilation, b1 = p.N1;
    const size_t na = (size_t)(a1 - a0) * C / 4, nb = (size_t)(b1 > b0 ? b1 - b0 : 0) * C / 4;      // C % 16 == 0
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    // layer 0's blocks also clear the aux-feature gradient [N1][Ap] of this batch item (every layer adds to it); aux hoist: every layer's
    // blocks clear the layer's frame-rate accumulators D_l[b] instead
    const size_t nh = p.hoist ? (size_t)(p.nfr + 1) * 2 * C / 4 : (j == 0 ? (size_t)p.N1 * p.Ap / 4 : 0);
    const size_t ne = (p.hoist && b == 0) ? (size_t)TR_EB_SLOTS * 2 * C / 4 : 0;            // ... and (batch item 0's blocks) the layer's gate-bias accumulators E_l
    float* H = p.hoist ? bw.DPA + (size_t)(j * p.B + b) * (p.nfr + 1) * 2 * C : bw.DHUP + (size_t)b * p.N1 * p.Ap;
    for (size_t i = part * nthr + t; i < na + nb + nh + ne; i += nparts * nthr) {
        if (i < na) ((float4*)(A + (size_t)a0 * C))[i] = z;
        else if (i < na + nb) ((float4*)(Bq + (size_t)(b0 > 0 ? b0 : 0) * C))[i - na] = z;
        else if (i < na + nb + nh) ((float4*)H)[i - na - nb] = z;
        else ((float4*)(bw.EB + (size_t)j * TR_EB_SLOTS * 2 * C))[i - na - nb - nh] = z;
    }
}
__global__ void k_zero_dx(TrainParams p, TrainBwd bw) {
    zero_dx_slice(p, bw, blockIdx.y, blockIdx.z, blockIdx.x, gridDim.x, threadIdx.x, blockDim.x);
}

// ------------------------------------------------------------------------------------------ launchers
void qpn_launch_zero_dx(const TrainParams& p, const TrainBwd& bw, hipStream_t stream) {
    hipLaunchKernelGGL(k_zero_dx, dim3(64, p.L, p.B), dim3(256), 0, stream, p, bw);
}

// the skip / post-net part of the slab reduction, launched on the side stream right behind those weight gradients
// tail: this launch also zeroes the entries no slab feeds and appends the trailer (then the final reduction must not: the upsampling
// kernel's gradient is added onto those zeros in between)
static void launch_reduce_early(const TrainBwd& bw, const TlpLaunch& l, hipStream_t st, int tail, int nch_side) {
    const TrainSlabs& sl = *bw.sl;
    hipLaunchKernelGGL(k_reduce_grad_s, dim3(l.gx), dim3(l.block), 0, st, bw.slab, bw.gdst, bw.gdst_list, bw.gzero, bw.n_gzero,
                       nch_side, bw.gstage, bw.n_params, bw.gflat, bw.gscale, bw.append_scale, sl.g_early0, sl.g_early1, 0, 0, tail, bw.status, 0);
}
// slabs -> flat gradient (writes every entry); the histogram-style gradients follow on top (causal table when no contraction owns it, upsampling kernel)
static void launch_reduce(const TrainBwd& bw, const TrainTailPlan& t, hipStream_t st) {
    const TrainSlabs& sl = *bw.sl;
    hipLaunchKernelGGL(k_reduce_grad_s, dim3(t.reduce.gx), dim3(t.reduce.block), 0, st, bw.slab, bw.gdst, bw.gdst_list, bw.gzero, bw.n_gzero,
                       bw.nch, bw.gstage, bw.n_params, bw.gflat, bw.gscale, bw.append_scale, 0, bw.gstage, t.early_done ? sl.g_early0 : 0, t.early_done ? sl.g_early1 : 0, t.up_done ? 0 : 1, bw.status, bw.append_scale == 1 ? 1 : 0);
}
static int launch_causal_hist(const TrainParams& p, const TrainBwd& bw, const TrainTailPlan& t, hipStream_t st) {
    if (t.causal.lds > TLP_LDS_OPTIN) QPN_HIP(hipFuncSetAttribute((const void*)k_causal_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.causal.lds));
    hipLaunchKernelGGL(k_causal_bwd, dim3(t.causal.gx), dim3(t.causal.block), t.causal.lds, st, p, bw, t.rpw, t.CB);
    return QPN_OK;
}
static void launch_up_bwd(const TrainParams& p, const TrainBwd& bw, const TlpLaunch& l, hipStream_t st) {
    hipLaunchKernelGGL(k_up_bwd, dim3(l.gx, l.gy), dim3(l.block), 0, st, up_args(p, bw));
}
static void launch_aux_tail(const TrainParams& p, const TrainBwd& bw, const AuxGeom& ag, const TlpLaunch& l, hipStream_t st) {
    hipLaunchKernelGGL(k_aux_tail, dim3(l.gx), dim3(l.block), 0, st, tr_aux_args(p, &bw, ag));
}

// The GEMM step's tail (train_gemm.hip keeps its own launchers): the final reduction with nothing done early, and what follows it.  The tile step's tail is
// the last jobs of its plan (qpn_launch_bwd)
int qpn_launch_grad_tail(const TrainParams& p, const TrainBwd& bw, const AuxGeom* ag, hipStream_t stream, bool early_done, bool up_done) {
    const TrainTailIn in = {p.C, p.Q, p.U, p.L, p.A, p.B, p.N1, p.F, bw.gstage, bw.n_gzero, bw.sl->g_cw, p.hoist != 0};
    const TrainTailPlan t = train_tail_plan(in, bw.dh != nullptr, early_done, up_done);
    if (t.rc) return t.rc;
    launch_reduce(bw, t, stream);
    if (t.causal_hist) { const int rc = launch_causal_hist(p, bw, t, stream); if (rc) return rc; }
    if (t.up_bwd) launch_up_bwd(p, bw, t.up, stream);
    if (t.aux_tail && ag) launch_aux_tail(p, bw, *ag, t.aux, stream);
    if (t.input_grad) qpn_launch_input_grad(p, bw, ag, stream);
    qpn_prof_mark(PG_GRAD_TAIL, stream);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}

int qpn_launch_stack_bwd(const TrainParams& p, const TrainBwd& bw, const StackQ& q, const TrainBwdPlan& pl, hipStream_t stream);

void qpn_launch_post_fb(const TrainParams& p, const TrainBwd& bw, const TlpLaunch& l, hipStream_t stream) {
    (void)hipFuncSetAttribute((const void*)k_post_fb_w<TLP_POST_MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds);
    hipLaunchKernelGGL((k_post_fb_w<TLP_POST_MT>), dim3(l.gx, l.gy), dim3(l.block), l.lds, stream, p, bw, 1);
}

// the persistent layer kernel of a plan: <8 | 11, last layer>
typedef void (*LayerBwdP)(TrainParams, TrainBwd, int, int, int, float*);
static LayerBwdP layer_bwd_p(int form, bool last) {
    return form == 8 ? (last ? k_layer_bwd_p<8, true> : k_layer_bwd_p<8, false>) : (last ? k_layer_bwd_p<11, true> : k_layer_bwd_p<11, false>);
}
static int launch_layers_bwd(const TrainParams& p, const TrainBwd& bw, const TrainBwdPlan& pl, const StackQ& sq, hipStream_t stream) {
    if (pl.path == TLP_STACK) return qpn_launch_stack_bwd(p, bw, sq, pl, stream);
    for (int l = p.L - 1; l >= 0; --l) {
        const TlpLaunch& y = pl.layer[l];
        if (pl.path == TLP_PERSIST) {      // register-resident weights, 2 workgroups per CU over contiguous tile ranges (k_layer_bwd_p)
            const LayerBwdP kf = layer_bwd_p(pl.form, l == p.L - 1);
            (void)hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)y.lds);
            hipLaunchKernelGGL(kf, dim3(y.gx, y.gy), dim3(y.block), y.lds, stream, p, bw, l, pl.swz ? 2 : 0, p.qT[l], p.scratch_rows);
        } else {
            if (y.lds > TLP_LDS_OPTIN) (void)hipFuncSetAttribute((const void*)k_layer_bwd<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)y.lds);
            hipLaunchKernelGGL((k_layer_bwd<1>), dim3(y.gx, y.gy), dim3(y.block), y.lds, stream, p, bw, l, l == p.L - 1 ? 1 : 0, pl.swz);
        }
    }
    return QPN_OK;
}

// The backward of the tile step: the jobs of its plan (train_launch_plan.h), in order, each on the stream the plan names.  Why a job runs where it does: DESIGN 5.
// sq: the backward queue (used by a TLP_STACK plan only)
int qpn_launch_bwd(const TrainParams& p, const TrainBwd& bw, const TrainBwdPlan& pl, const AuxGeom& ag, const StackQ& sq, hipStream_t stream) {
    const TrainSlabs& sl = *bw.sl;
    // the five contraction records (train_wgrad_plan.h), from one view of the step; p.TH holds the gate product, as it is
    const WgradView wv = tr_wgrad_view(p);
    const WgradBufs wb = tr_wgrad_bufs(p, bw, p.TH);
    const WgradFlags wf = {pl.wr_summed, pl.post_pair, true, true};
    bool ok = true;
    auto wgrad = [&](const Wg2& w, int chunks, hipStream_t st) { ok = ok && qpn_launch_wgrad(w, chunks, pl.wgrad_generic, st) == QPN_OK; };
    for (int i = 0; i < pl.njobs; ++i) {
        const TrainJob& j = pl.jobs[i];
        const hipStream_t st = j.side ? bw.side : stream;
        switch (j.kind) {
        case TJ_MARK: break;
        case TJ_ZERO: hipLaunchKernelGGL(k_zero_dx, dim3(pl.zero.gx, pl.zero.gy, pl.zero.gz), dim3(pl.zero.block), 0, st, p, bw); break;
        case TJ_POST_BWD: {
            const TlpLaunch& w = pl.post_l;
            if (pl.post == TLP_POST_WIDE) {      // 80 rows per workgroup (k_post_bwd_w)
                QPN_HIP(hipFuncSetAttribute((const void*)k_post_bwd_w<TLP_POST_MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds));
                hipLaunchKernelGGL((k_post_bwd_w<TLP_POST_MT>), dim3(w.gx, w.gy), dim3(w.block), w.lds, st, p, bw, pl.zero_in_post ? 1 : 0);
            } else {
                if (w.lds > TLP_LDS_OPTIN) (void)hipFuncSetAttribute((const void*)k_post_bwd<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds);
                hipLaunchKernelGGL((k_post_bwd<1>), dim3(w.gx, w.gy), dim3(w.block), w.lds, st, p, bw);
            }
        } break;
        case TJ_FORK: QPN_HIP(hipEventRecord(bw.ev_fork, stream)); QPN_HIP(hipStreamWaitEvent(bw.side, bw.ev_fork, 0)); break;
        case TJ_SKIP: wgrad(wgrad_rec_skip(wv, sl, wb, wf), j.arg, st); break;
        case TJ_POST: for (int part = 0; part < j.n; ++part) wgrad(wgrad_rec_post(wv, sl, wb, wf, part), j.arg, st); break;
        case TJ_REDUCE_EARLY: launch_reduce_early(bw, pl.reduce_early, st, j.n, pl.nch_side); break;
        // the post-net block of the flat gradient (and the zeroing and the row-count trailer behind it) is final from here on: a data-parallel caller
        // exchanges that bucket while the layer backward still runs (qpn_train_early_bucket)
        case TJ_EARLY_EVENT: QPN_HIP(hipEventRecord(bw.ev_early, st)); *bw.early_recorded = 1; break;
        case TJ_LAYERS: { const int rc = launch_layers_bwd(p, bw, pl, sq, st); if (rc) return rc; } break;
        case TJ_MID: QPN_HIP(hipEventRecord(bw.ev_mid, stream)); QPN_HIP(hipStreamWaitEvent(bw.side, bw.ev_mid, 0)); break;
        case TJ_UP: launch_up_bwd(p, bw, pl.tail.up, st); break;
        case TJ_AUX_TAIL: launch_aux_tail(p, bw, ag, pl.tail.aux, st); break;
        case TJ_INPUT_GRAD: qpn_launch_input_grad(p, bw, &ag, st); break;
        case TJ_W1: wgrad(wgrad_rec_w1(wv, sl, wb, wf), j.arg, st); break;
        case TJ_WR: wgrad(wgrad_rec_wr(wv, sl, wb, wf), j.arg, st); break;
        case TJ_CAUSAL: wgrad(wgrad_rec_causal(wv, sl, wb), j.arg, st); break;
        case TJ_JOIN: QPN_HIP(hipEventRecord(bw.ev_join, bw.side)); break;
        case TJ_WAIT: QPN_HIP(hipStreamWaitEvent(stream, bw.ev_join, 0)); break;
        case TJ_REDUCE:
            if (!ok) return QPN_EINVAL;      // (qpn_launch_wgrad has set the error text: a geometry no tile kernel takes; the side stream has been joined)
            launch_reduce(bw, pl.tail, st); break;
        case TJ_CAUSAL_HIST: { const int rc = launch_causal_hist(p, bw, pl.tail, st); if (rc) return rc; } break;
        }
        if (j.mark > -2) qpn_prof_mark(j.mark, st);
    }
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
