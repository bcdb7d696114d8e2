// decode.hip -- persistent autoregressive decode of QPNet on gfx950 (MI355X).
//
// Replaces QPNet.batch_fast_generate (reference src/nets/qpnet.py:314-559) and the per-sample
// helpers it calls (_generate_fixed_residual_forward :672-685, _generate_adaptive_residual_forward
// :642-655, FDilatedConv1d :81-87, _generate_dilated_index :613-624, _preprocess :561-564,
// _postprocess :566-571).  The reference dispatches ~160 tiny torch ops per generated sample;
// here the whole utterance is ONE kernel launch: one 1024-thread workgroup per utterance walks a
// host-built micro-program ("tasks") once per sample.  A task is a 64-lane x 16-deep weight tile
// (4 KiB, streamed from L2 with coalesced 16-byte loads, prefetched one task ahead across the
// workgroup barrier) plus an epilogue (gate / residual / skip accumulate / post-net / argmax).
// All recurrent state of the current step lives in LDS; the per-layer input history ("ring
// buffers", up to maxd*2^k samples deep) lives in a small L2-resident global block because
// 15*maxd*C floats exceed one CU's LDS for low pitch (SURVEY.md §7 "Ring-buffer footprint").
//
// Arithmetic is the fixed-order fp32 "QPNet-f32" spec of DESIGN.md §3, so results are
// bit-identical to the CPU oracle; compile with -ffp-contract=off.
#include "qpn_common.h"
#include "qpn_handle.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>

#include "decode_dev.h"


// ================================================================== small setup kernels
__global__ void k_pack_gather(const float* __restrict__ flat, const int* __restrict__ map, float* __restrict__ out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { int m = map[i]; out[i] = m >= 0 ? flat[m] : 0.0f; }
}


// Qb[l][row] = ((b_up * dot(Va[row,:], 1) + ba) + b_conv) [+ b_convP]   
// one workgroup of 64*k lanes per layer; aux tiles packed natural-row, R = Ap/16.
__global__ void k_fold_bias(const float4* __restrict__ wpk, const float* __restrict__ flat, const BiasDesc* __restrict__ bd,
                            int aux_woff4_layer0, int aux_tiles_per_layer, int logRa, int A, int Ap, int C,
                            const float* __restrict__ up_b_ptr, float* __restrict__ qb) {
    const float up_b = up_b_ptr ? *up_b_ptr : 0.0f;      // read on the device: qpn_set_weights needs no read-back
    extern __shared__ float4 smem4[];
    float* sm = (float*)smem4;
    const int l = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < Ap; i += blockDim.x) sm[i] = i < A ? 1.0f : 0.0f;
    __syncthreads();
    const int R = 1 << logRa, rpt = 64 / R, q = lane & (R - 1);
    const BiasDesc b = bd[l];
    for (int t = wave; t < aux_tiles_per_layer; t += nw) {
        float4 w[4], x[4];
        load_tile(w, wpk, aux_woff4_layer0 + (l * aux_tiles_per_layer + t) * 256, lane);
        const float4* xv = (const float4*)(sm + 16 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = xv[j];
        float rs = tree_reduce(chunk16(w, x), logRa);
        int row = t * rpt + (lane >> logRa);
        if (q == 0) {
            int half = row / C, r = row - half * C;
            float v = up_b * rs;
            v = v + flat[b.auxb[half] + r];
            v = v + flat[b.convb[half] + r];
            if (b.adaptive) v = v + flat[b.convPb[half] + r];
            qb[(size_t)l * 2 * C + row] = v;
        }
    }
}

// P[b][f][l][row] = dot(Va_l[row,:], h[b,:,f])  -- aux 1x1 convs hoisted to FRAME rate.
// grid (F, B); h is (B, A, F).
__global__ void k_aux_project(const float4* __restrict__ wpk, const float* __restrict__ h, int64_t F,
                              int aux_woff4_layer0, int aux_tiles_per_layer, int logRa, int A, int Ap, int C, int L,
                              float* __restrict__ pproj) {
    extern __shared__ float4 smem4[];
    float* sm = (float*)smem4;
    const int64_t f = blockIdx.x; const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < Ap; i += blockDim.x) sm[i] = i < A ? h[((size_t)b * A + i) * F + f] : 0.0f;
    __syncthreads();
    const int R = 1 << logRa, rpt = 64 / R, q = lane & (R - 1);
    float4 x[4];
    const float4* xv = (const float4*)(sm + 16 * q);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = xv[j];
    float* out = pproj + ((size_t)b * F + f) * L * 2 * C;
    const int ntiles = L * aux_tiles_per_layer;
    for (int t = wave; t < ntiles; t += nw) {
        float4 w[4];
        load_tile(w, wpk, aux_woff4_layer0 + t * 256, lane);
        float v = tree_reduce(chunk16(w, x), logRa);
        int l = t / aux_tiles_per_layer, tt = t - l * aux_tiles_per_layer;
        int row = tt * rpt + (lane >> logRa);
        if (q == 0) out[(size_t)l * 2 * C + row] = v;
    }
}

// known[b][i]: n_pad copies of Q/2 (qpnet.py:358) then x % Q (OneHot, qpnet.py:76)
__global__ void k_known(const int64_t* __restrict__ x, int n_x, int n_pad, int Q, int* __restrict__ known) {
    const int b = blockIdx.y, n0 = n_pad + n_x;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n0) {
        int v;
        if (i < n_pad) v = Q / 2;
        else { int64_t s = x[(size_t)b * n_x + (i - n_pad)] % Q; v = (int)(s < 0 ? s + Q : s); }
        known[(size_t)b * n0 + i] = v;
    }
}



// ================================================================== the persistent decode kernel

// aux terms a[t1] of every layer -> LDS (needs only the frame-rate projections)
__device__ __forceinline__ void stage_aux(const DecodeParams& p, const UttView& u, int64_t t1, int tid, int nthreads) {
    float* sm = SM;
    const int n = p.L * 2 * p.C;
    const int ut = aux_time(u, (int)t1);             // 32-bit: n0 + n_samples < 2^31 is checked on the host
    int f, j;
    if (ut < 0) { f = 0; j = 0; }                    // replicate pad of the upsampled h (qpnet.py:359)
    else if (p.U > 0) { f = (int)((unsigned)ut / (unsigned)p.U); j = ut - f * p.U; }
    else { f = ut; j = 0; }
    const float wj = p.U > 0 ? p.flat[p.up_w + j] : 1.0f;
    const float* pf = u.pproj + (size_t)f * n;
    for (int i = tid; i < n; i += nthreads) sm[p.o_auxv + i] = __builtin_fmaf(wj, pf[i], p.qb[i]);
}
// gathered past rows x_l[t2 - off_l(t2)] of every layer -> LDS xp; sel[l] = 1 when off == 1 (the row is
// produced during step t2-1 itself and is read from xbuf instead)
__device__ __forceinline__ void stage_taps(const DecodeParams& p, const UttView& u, int64_t t2, int tid, int nthreads, int* status) {
    const int L = p.L, C = p.C;
    float* sm = SM; int* smi = SMI;
    const int ut = aux_time(u, (int)t2);
    const int widx = (int)t2 < u.n0 - 1 ? (int)t2 - (u.n0 - 1) : 0;
    for (int i = tid; i < L * C; i += nthreads) {
        const int l = i / C, c = i - l * C;
        const RingDesc r = p.rings[l];
        int off = tap_offset(r, u, ut, widx);
        if (off < 1 || off >= r.len) { if (c == 0) atomicOr(status, 1); off = off < 1 ? 1 : r.len - 1; }
        if (c == 0) smi[p.o_sel + l] = off == 1;
        if (off > 1) {
            const int tp = (int)t2 - off;             // time of the past tap; < 0 -> a never-written (zero) slot
            const int slot = tp >= 0 ? (int)((unsigned)tp % (unsigned)r.len) : tp + r.len;
            sm[p.o_xp + l * p.Cp + c] = ld_agent(u.ring + r.base + (size_t)slot * C + c);
        }
    }
}
// causal conv on the one-hot input = two table rows (qpnet.py:110-132): input of layer 0 at time t1
__device__ __forceinline__ void causal_rows(const DecodeParams& p, const UttView& u, int s_prev, int s_cur, int64_t t1, int lane) {
    float* sm = SM;
    const RingDesc r0 = p.rings[0];
    for (int ch = lane; ch < p.C; ch += 64) {
        float v = p.flat[p.causal_w + ((size_t)ch * p.Q + s_prev) * 2] + p.flat[p.causal_w + ((size_t)ch * p.Q + s_cur) * 2 + 1];
        v = v + p.flat[p.causal_b + ch];
        sm[p.o_xbuf + ch] = v;
        st_agent(u.ring + r0.base + (size_t)((unsigned)t1 % (unsigned)r0.len) * p.C + ch, v);
    }
}

struct Ctx {
    const DecodeParams* p; const UttView* u;
    int lane, wave; int64_t Ttot;
    int creq, stop;      // the host's stop request: the publishing lane's state (live_put); the workgroup's copy of the LDS stop word
};

// one slot of the per-step program for this wave; `w` holds the slot's weight tile and is refilled with
// the tile of slot+3 as soon as it has been consumed (three tiles in flight per wave).
// where the one-CU kernels of the calls with per-row records keep the row's record (stage_row_draw, decode_dev.h): eight LDS words behind everything else the launch
// uses, the dev stamps included (launch_one_cu sizes the launch's LDS to match)
__device__ __forceinline__ int one_cu_rowd(const DecodeParams& p) { return p.o_stamp + (p.stamps ? 120 * QPN_NW : 0); }
template <int ROW, bool WIDE>
__device__ __forceinline__ void run_slot(Ctx& c, int slot, int64_t t, float4 (&w)[4]) {
    const DecodeParams& p = *c.p; const UttView& u = *c.u;
    float* sm = SM; int* smi = SMI;
    const int lane = c.lane;
    const int4* tl = (const int4*)(smi + p.o_tasks + (slot * QPN_NW + c.wave) * 8);
    const int4 q0 = tl[0], q1 = tl[1];
    const int opf = __builtin_amdgcn_readfirstlane(q0.x);
    int xoff = __builtin_amdgcn_readfirstlane(q0.z);
    const int row0 = __builtin_amdgcn_readfirstlane(q0.w);
    const int ta = __builtin_amdgcn_readfirstlane(q1.x), tb = __builtin_amdgcn_readfirstlane(q1.y);
    const int tc = __builtin_amdgcn_readfirstlane(q1.z), td = __builtin_amdgcn_readfirstlane(q1.w);
    // descriptor of the task three slots ahead (same register set)
    int ns = slot + 3; if (ns >= p.n_slots) ns -= p.n_slots;
    const int2 nq = *(const int2*)(smi + p.o_tasks + (ns * QPN_NW + c.wave) * 8);
    const int nopf = __builtin_amdgcn_readfirstlane(nq.x), nwoff = __builtin_amdgcn_readfirstlane(nq.y);
    if (opf & TF_BARRIER) {
        if (opf & TF_DRAIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_barrier();
        // the stop word is written in the pick phase only (the phase behind the TF_DRAIN barrier): read behind any other barrier, every wave finds
        // what the previous step's pick left -- the same value in all of them
        if (p.cancel && !(opf & TF_DRAIN)) c.stop = smi[p.o_samp + 2];
    }
    const int op = opf & 0xff;
    const int C = p.C, Q = p.Q;
    if (opf & TF_HASW) {
        const int logR = (opf >> 16) & 0xf;
        const int R = 1 << logR, q = lane & (R - 1);
        if (op == OP_PAST && smi[p.o_sel + tc]) xoff = tb;        // tap distance 1: the row is this step's layer input
        float4 x[4];
        const float4* xv = (const float4*)(sm + xoff + 16 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = xv[j];
        float acc = chunk16(w, x);
        if (nopf & TF_HASW) load_tile(w, p.wpk, nwoff, lane);
        acc = tree_reduce(acc, logR);
        const int row = row0 + (lane >> logR);
        const bool lead = q == 0;
        const int par = (int)(t & 1) * p.L * 2 * C;
        switch (op) {
        case OP_PAST:      // a = layer*2C: past-tap dot of the NEXT step -> pd[(t+1)&1]
            if (lead) sm[p.o_pd + (p.L * 2 * C - par) + ta + row] = acc;
            break;
        case OP_Z: {       // rows interleaved (sigmoid_c, tanh_c); a = layer*2C, c = g
            const int ch = row >> 1, half = row & 1, nat = half * C + ch;
            const float z = (acc + sm[p.o_pd + par + ta + nat]) + sm[p.o_auxv + ta + nat];
            float zo;
            if (logR == 2) zo = dpp_f<0x104>(z);            // row_shl:4 -> lane i reads lane i+4 (the tanh group)
            else if (logR == 1) zo = dpp_f<0x102>(z);
            else if (logR == 3) zo = dpp_f<0x108>(z);
            else if (logR == 0) zo = dpp_f<0x101>(z);
            else zo = __shfl_xor(z, R);
            if (lead && !half) sm[tc + ch] = qgate(z, zo);
            break;
        }
        case OP_RES:       // a = x in (LDS), b = bias (LDS), c = x out (LDS), d = ring index of the consumer or -1
            if (lead) {
                const float v = (acc + sm[tb + row]) + sm[ta + row];
                sm[tc + row] = v;
                if (td >= 0) {
                    const RingDesc r = p.rings[td];
                    st_agent(u.ring + r.base + (size_t)(t % r.len) * C + row, v);
                }
            }
            break;
        case OP_SKIP:      // a = accumulator (LDS), b = bias (LDS), c = other accumulator, d = y1
            if (lead) {
                const float v = sm[ta + row] + (acc + sm[tb + row]);
                sm[ta + row] = v;
                if (opf & TF_LAST) {
                    const float tot = tc >= 0 ? sm[tc + row] + v : v;     // sumF + sumA (qpnet.py:505)
                    sm[td + row] = tot > 0.0f ? tot : 0.0f;
                }
            }
            break;
        case OP_POST1:     // b = bias, c = y2
            if (lead) { const float v = acc + sm[tb + row]; sm[tc + row] = v > 0.0f ? v : 0.0f; }
            break;
        case OP_POST2:     // b = bias, c = logits
            if (lead) sm[tc + row] = acc + sm[tb + row];
            break;
        default: break;
        }
        return;
    }
    if (op == OP_ARGMAX) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int i = lane; i < Q; i += 64) { const float v = sm[p.o_lg + i]; if (v > bv) { bv = v; bi = i; } }
        bi = wave_argmax(bv, bi);
        const int64_t i = t - (u.n0 - 1);
        if (i >= 0 && u.logits) for (int k = lane; k < Q; k += 64) u.logits[(size_t)i * Q + k] = sm[p.o_lg + k];
        int next;
        if (i >= 0) {
            if (p.mode != QPN_MODE_ARGMAX) bi = sample_pick<ROW, WIDE>(p, (unsigned)u.row, one_cu_rowd(p), p.o_lg, Q, (unsigned)i, lane);
            next = bi;
            if (u.teacher) { const int64_t sv = u.teacher[i] % Q; next = (int)(sv < 0 ? sv + Q : sv); }
            if (lane == 0) { u.out[i] = bi; if (live_put(p, u, (int)i, bi, c.creq)) smi[p.o_samp + 2] = 1; }      // stop on request: the workgroup leaves after the next step
        } else next = u.known[t + 1];
        const int cur = smi[p.o_samp + 1];
        if (t + 2 < c.Ttot) causal_rows(p, u, cur, next, t + 1, lane);     // layer-0 input of the next step
        if (lane == 0) { smi[p.o_samp] = cur; smi[p.o_samp + 1] = next; }
    } else if (op == OP_STAGE) {    // a = first wave of the staging group, b = waves in it
        const int stid = (c.wave - ta) * 64 + lane, nst = tb * 64;
        int fdw = 0;      // draw track: the next step's frame record, requested in front of the staging loads and stored behind them (its pick is a step away)
        if constexpr (ROW == 2) if (t + 2 < c.Ttot) fdw = frame_draw_load(p, u, (int)t + 1, stid);
        for (int i = stid; i < p.S; i += nst) { sm[p.o_skf + i] = 0.0f; sm[p.o_ska + i] = 0.0f; }
        if (t + 2 < c.Ttot) stage_aux(p, u, t + 1, stid, nst);
        if (t + 3 < c.Ttot) stage_taps(p, u, t + 2, stid, nst, p.status);
        if constexpr (ROW == 2) if (t + 2 < c.Ttot) frame_draw_store(u, (int)t + 1, one_cu_rowd(p), stid, fdw);
    }
    if (nopf & TF_HASW) load_tile(w, p.wpk, nwoff, lane);
}

#define QPN_KERNEL k_decode
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE false
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_r      // ... of the calls with per-row records
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE false
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_t      // ... of the calls with a draw track
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE false
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
// ... and the three again for the sampled calls at n_quantize > 256: their picks run the wide draw (sample_pick<ROW, true>, decode_dev.h)
#define QPN_KERNEL k_decode_w
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE true
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_wr
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE true
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_wt
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE true
#include "decode_slot_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE


// ================================================================== specialised straight-line decode kernel
// Same algorithm, state and bit-exact arithmetic as k_decode, but for geometries whose per-layer tiles fit one
// round of 16 waves (2*NZ <= 16: n_resch <= 64) the per-step program is compiled as straight-line code with a
// STATIC tile assignment instead of being interpreted from the task table: ~45 instructions per tile instead of
// ~170, addresses and LDS offsets folded, reductions chosen at compile time.  (In-kernel stamps showed the
// interpreter spends ~1500 cycles of pure instruction issue per slot; the memory system was idle half the time.)
//   Z phase (per layer)  waves [0,NZ): this step's z tiles + gate      waves [NZ,2NZ): next step's past-tap dots
//   R phase              residual 1x1 tiles first (-> next layer input), then the skip 1x1 tiles
//   tail                 skip total/relu -> post 1x1 #1 -> post 1x1 #2 -> argmax/causal/staging
// What bounds a step and why the kernel looks the way it does: DESIGN.md §4, profiles/r01_decode_fast_phase_timeline.txt.
template <int V> struct ILog2 { static constexpr int v = 1 + ILog2<V / 2>::v; };
template <> struct ILog2<1> { static constexpr int v = 0; };

template <int LOGR>
__device__ __forceinline__ float tree_reduce_c(float acc) {
    if constexpr (LOGR == 5) { acc = acc + __shfl_xor(acc, 16); }
    if constexpr (LOGR >= 4) { acc = acc + dpp_f<0x128>(acc); }
    if constexpr (LOGR >= 3) { if constexpr (LOGR == 3) acc = acc + __shfl_xor(acc, 4); else acc = acc + dpp_f<0x124>(acc); }
    if constexpr (LOGR >= 2) { acc = acc + dpp_f<0x4E>(acc); }
    if constexpr (LOGR >= 1) { acc = acc + dpp_f<0xB1>(acc); }
    return acc;
}
__device__ __forceinline__ void read_x(float4 (&x)[4], int xoff_plus_16q) {
    const float4* xv = (const float4*)(SM + xoff_plus_16q);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = xv[j];
}

// One tile's worth of work for the straight-line kernel: 4 coalesced 1 KiB loads / the spec dot product of a tile.
__device__ __forceinline__ void tile_load(float4 (&w)[4], const float4* tp) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = tp[j * 64];
}

// NWV waves per workgroup.  Per layer a wave owns ZT tiles of the Z phase (ids w, w+NWV, ..: z tiles first, then the
// next step's past-tap tiles) and RT tiles of the R phase (residual tiles first, then skip tiles); every tile is
// re-requested in place for the next layer right after it has been consumed (a full layer ahead of its use).
// What a wave does with its slots depends only on which interval of wave ids it falls in, so the step loop is
// instantiated once per interval ("role", W0 = its first wave): inside a role the code is straight-line with no
// wave-dependent branches around the tile requests, and hipcc's waitcnt pass can then count the outstanding loads
// (vmcnt(N)) instead of draining the queue (vmcnt(0)) in front of every tile.
template <int C, int S, int Q, int NWV>
struct FastGeo {
    static constexpr int R = C / 16, LOGR = ILog2<R>::v, RPT = 64 / R;
    static constexpr int NZ = 2 * C / RPT, NRES = C / RPT, NSK = S / RPT;
    static constexpr int ZT = (2 * NZ + NWV - 1) / NWV, RT = (NRES + NSK + NWV - 1) / NWV;
    static constexpr int RS = S / 16, LOGRS = ILog2<RS>::v, RPTS = 64 / RS;
    static constexpr int NP1 = S / RPTS, NP2 = Q / RPTS;
    static constexpr int T1 = (NP1 + NWV - 1) / NWV, T2 = (NP2 + NWV - 1) / NWV;
    static constexpr int zkind(int id) { return id < NZ ? 1 : id < 2 * NZ ? 2 : 0; }            // 1 z tile, 2 past-tap tile
    static constexpr int rkind(int id) { return id < NRES ? 1 : id < NRES + NSK ? 2 : 0; }      // 1 residual, 2 skip
    static constexpr int next_boundary(int w0) {
        int nb = NWV;
        for (int i = 0; i < 16; ++i) {
            const int th[6] = {NZ - i * NWV, 2 * NZ - i * NWV, NRES - i * NWV, NRES + NSK - i * NWV, NP1 - i * NWV, NP2 - i * NWV};
            for (int k = 0; k < 6; ++k) if (th[k] > w0 && th[k] < nb) nb = th[k];
        }
        return nb;
    }
};

template <int C, int S, int Q, int NWV, bool RESL, int ROW, int W0>
__device__ __forceinline__ void fast_steps(const DecodeParams& p, const FastParams& f, const UttView& u,
                                           const int wave, const int lane0, const int tid0, const int Ttot) {
    using G = FastGeo<C, S, Q, NWV>;
    constexpr int NTH = NWV * 64;
    constexpr int R = G::R, LOGR = G::LOGR, RPT = G::RPT, NZ = G::NZ, NRES = G::NRES, ZT = G::ZT, RT = G::RT;
    constexpr int RS = G::RS, LOGRS = G::LOGRS, RPTS = G::RPTS, T1 = G::T1, T2 = G::T2;
    static_assert(ZT <= 4 && RT <= 4 && T1 <= 4 && T2 <= 4, "slot macros are expanded four times");
    float* sm = SM; int* smi = SMI;
    const int L = p.L;
    int stamp_i = 0;
    int creq = 0;           // the host's stop request: the publishing lane's state (live_put)
#ifdef QPN_ENABLE_STAMPS   // dev aid (-DQPN_ENABLE_STAMPS + QPN_STAMPS=1): s_memtime at every phase boundary of step 3000,
                           // parked in LDS behind the kernel's own state (no global stores in the timed code), dumped after the step
#define QPN_STAMP() do { if (p.stamps && t == 3000 && lane == 0 && stamp_i < 120) smi[p.o_stamp + stamp_i * QPN_NW + (wave < QPN_NW ? wave : 0)] = (int)__builtin_amdgcn_s_memtime(); ++stamp_i; } while (0)
#define QPN_STAMP_DUMP() do { if (p.stamps && t == 3000 && lane == 0) for (int k = 0; k < stamp_i && k < 120; ++k) p.stamps[(size_t)k * QPN_NW + (wave < QPN_NW ? wave : 0)] = (long long)(unsigned)smi[p.o_stamp + k * QPN_NW + (wave < QPN_NW ? wave : 0)]; } while (0)
#else
#define QPN_STAMP() do { (void)stamp_i; } while (0)
#define QPN_STAMP_DUMP() do { } while (0)
#endif
    const float4* wl0 = p.wpk + lane0;
    const int C2 = 2 * C, LC2 = L * C2;
    float4 wz[ZT][4], wr[RT][4], wp[4];
#define QPN_ZPTR(wl, l, id) ((wl) + ((id) < NZ ? f.w_cur[l] + (id) * 256 : f.w_past[l] + ((id) - NZ) * 256))
#define QPN_RPTR(wl, l, id) ((wl) + ((id) < NRES ? f.w_res[l] + (id) * 256 : f.w_skip[l] + ((id) - NRES) * 256))
#define QPN_ZINIT(wl, i) if constexpr ((i) < ZT && G::zkind(W0 + (i) * NWV) != 0) tile_load(wz[(i) < ZT ? (i) : 0], QPN_ZPTR(wl, 0, wave + (i) * NWV));
#define QPN_RINIT(wl, i) if constexpr ((i) < RT && G::rkind(W0 + (i) * NWV) != 0 && !(RESL && G::rkind(W0 + (i) * NWV) == 1)) tile_load(wr[(i) < RT ? (i) : 0], QPN_RPTR(wl, 0, wave + (i) * NWV));
    QPN_ZINIT(wl0, 0) QPN_ZINIT(wl0, 1) QPN_ZINIT(wl0, 2) QPN_ZINIT(wl0, 3)
    QPN_RINIT(wl0, 0) QPN_RINIT(wl0, 1) QPN_RINIT(wl0, 2) QPN_RINIT(wl0, 3)

    // The post-net tiles of a wave form one sequence s = 0..T1+T2-1 (post 1x1 #1 tiles, then #2) that cycles through three
    // register sets: wp, and the layer sets wz[0] / wr[0] once the last layer has consumed them.  Tile s is requested as
    // soon as tile s-3 has been consumed, the first three during the last layer.
#define QPN_TB(s) ((s) % 3 == 0 ? wp : (s) % 3 == 1 ? wz[0] : wr[0])
#define QPN_TVALID(s) ((s) < T1 ? (W0 + (s) * NWV < G::NP1) : ((s) < T1 + T2 && W0 + ((s) - T1) * NWV < G::NP2))
#define QPN_TLOAD(s) if constexpr (QPN_TVALID(s)) tile_load(QPN_TB(s), wl + ((s) < T1 ? f.w_p1 + (wave + (s) * NWV) * 256 : f.w_p2 + (wave + ((s) - T1) * NWV) * 256));

    // ---- one layer; LAST = the final layer, which hands its tile registers to the post-net instead of re-requesting
#define QPN_ZSLOT(i, LAST)                                                                                        \
            if constexpr ((i) < ZT) {                                                                             \
                constexpr int zk = G::zkind(W0 + (i) * NWV);                                                      \
                const int id = wave + (i) * NWV;                                                                  \
                if constexpr (zk == 1) {                                                                          \
                    float4 x[4]; read_x(x, p.o_xbuf + l * p.Cp + 16 * q);                                         \
                    float acc;                                                                                    \
                    if constexpr (LAST) acc = chunk16(wz[(i) < ZT ? (i) : 0], x);                                 \
                    else acc = chunk16_reload(wz[(i) < ZT ? (i) : 0], x, QPN_ZPTR(wl, l + 1, id));                \
                    acc = tree_reduce_c<LOGR>(acc);                                                               \
                    const int row = id * RPT + grp, ch = row >> 1, half = row & 1, nat = half * C + ch;           \
                    const float z = (acc + sm[p.o_pd + par + l * C2 + nat]) + sm[p.o_auxv + l * C2 + nat];        \
                    const float zo = dpp_f<0x100 + R>(z);   /* row_shl:R -> the tanh group's pre-activation */    \
                    if (q == 0 && !half) sm[p.o_gl + l * p.Cp + ch] = qgate(z, zo);                               \
                } else if constexpr (zk == 2) {                                                                   \
                    const int xo = smi[p.o_sel + l] ? p.o_xbuf + l * p.Cp : p.o_xp + l * p.Cp;                    \
                    float4 x[4]; read_x(x, xo + 16 * q);                                                          \
                    float acc;                                                                                    \
                    if constexpr (LAST) acc = chunk16(wz[(i) < ZT ? (i) : 0], x);                                 \
                    else acc = chunk16_reload(wz[(i) < ZT ? (i) : 0], x, QPN_ZPTR(wl, l + 1, id));                \
                    acc = tree_reduce_c<LOGR>(acc);                                                               \
                    if (q == 0) sm[p.o_pd + (LC2 - par) + l * C2 + (id - NZ) * RPT + grp] = acc;  /* next parity */ \
                }                                                                                                 \
                if constexpr (LAST && (i) == 0) { QPN_TLOAD(1) }                                                     \
            }
#define QPN_RDOT(i, LAST)                                                                                         \
            if constexpr ((i) < RT) {                                                                             \
                constexpr int rk = G::rkind(W0 + (i) * NWV);                                                      \
                if constexpr (RESL && rk == 1) {                                                                  \
                    if constexpr (!(LAST)) {              /* resident tile: four 1 KiB LDS reads, no global request */ \
                        const float4* tp = (const float4*)(sm + p.o_wres) + (l * NRES + wave + (i) * NWV) * 256 + lane; \
                        /* the slot's register set is idle in this mode (the post-net borrows it later): use it as the landing zone */ \
                        _Pragma("unroll") for (int j = 0; j < 4; ++j) wr[(i) < RT ? (i) : 0][j] = tp[j * 64];       \
                        racc[(i) < RT ? (i) : 0] = tree_reduce_c<LOGR>(chunk16(wr[(i) < RT ? (i) : 0], xg));      \
                    }                                                                                             \
                } else if constexpr (rk != 0) {                                                                   \
                    if constexpr (LAST) racc[(i) < RT ? (i) : 0] = tree_reduce_c<LOGR>(chunk16(wr[(i) < RT ? (i) : 0], xg)); \
                    else racc[(i) < RT ? (i) : 0] = tree_reduce_c<LOGR>(chunk16_reload(wr[(i) < RT ? (i) : 0], xg, QPN_RPTR(wl, l + 1, wave + (i) * NWV))); \
                }                                                                                                 \
                if constexpr (LAST && (i) == 0) { QPN_TLOAD(2) }                                                  \
            }
#define QPN_RPUT(i, LASTL)                                                                                            \
            if constexpr ((i) < RT) {                                                                             \
                constexpr int rk = G::rkind(W0 + (i) * NWV);                                                      \
                const int id = wave + (i) * NWV;                                                                  \
                if constexpr (rk == 1 && !(RESL && LASTL)) {                                                      \
                    const int row = id * RPT + grp;                                                               \
                    /* x_{l+1}; its ring row is written once per step at the end (no stores in the load queue here) */ \
                    sm[p.o_xbuf + (l + 1) * p.Cp + row] = (racc[(i) < RT ? (i) : 0] + sm[f.b_res[l] + row]) + sm[p.o_xbuf + l * p.Cp + row]; \
                } else if constexpr (rk == 2) {                                                                   \
                    const int row = (id - NRES) * RPT + grp;                                                      \
                    const int a = (f.adaptive[l] ? p.o_ska : p.o_skf) + row;                                      \
                    sm[a] = sm[a] + (racc[(i) < RT ? (i) : 0] + sm[f.b_skip[l] + row]);                           \
                }                                                                                                 \
            }
#define QPN_LAYER(LAST)                                                                                           \
            if constexpr (LAST) { QPN_TLOAD(0) }                                                                  \
            wg_barrier();                                   /* layer input x_l, pd[par], aux terms are in LDS */  \
            QPN_STAMP();                                                                                          \
            QPN_ZSLOT(0, LAST) QPN_ZSLOT(1, LAST) QPN_ZSLOT(2, LAST) QPN_ZSLOT(3, LAST)                           \
            QPN_STAMP();                                                                                          \
            wg_barrier();                                   /* gate vector g_l is in LDS */                       \
            QPN_STAMP();                                                                                          \
            if constexpr (G::rkind(W0) != 0) {              /* every R tile of the wave reads the same g_l */     \
                float4 xg[4]; read_x(xg, p.o_gl + l * p.Cp + 16 * q);                                             \
                float racc[RT];                                                                                   \
                QPN_RDOT(0, LAST) QPN_RDOT(1, LAST) QPN_RDOT(2, LAST) QPN_RDOT(3, LAST)                           \
                if (q == 0) { QPN_RPUT(0, LAST) QPN_RPUT(1, LAST) QPN_RPUT(2, LAST) QPN_RPUT(3, LAST) }                                   \
            } else if constexpr (LAST) { QPN_TLOAD(2) }

    for (int t = 1; t + 1 < Ttot; ++t) {
        // hipcc hoists every lane-constant address out of the step loop and then spills them: an opaque zero
        // re-derives the lane ids per step instead, so nothing derived from them can be hoisted
        int zero = 0;
        asm volatile("" : "+s"(zero));
        const int lane = lane0 + zero, tid = tid0 + zero;
        const float4* wl = wl0 + zero;
        const int q = lane & (R - 1), grp = lane >> LOGR, qs = lane & (RS - 1), grps = lane >> LOGRS;
        const int par = (t & 1) * LC2;
        stamp_i = 0;
        for (int l = 0; l + 1 < L; ++l) { QPN_LAYER(false) }
        { const int l = L - 1; QPN_LAYER(true) }
        QPN_STAMP();
        // ---- tail: skip total / relu -> post 1x1 #1 -> post 1x1 #2
        wg_barrier();
        for (int row = tid; row < S; row += NTH) {
            const float tot = sm[p.o_skf + row] + sm[p.o_ska + row];      // sum(skip_F) + sum(skip_A)  (qpnet.py:505)
            sm[p.o_y1 + row] = tot > 0.0f ? tot : 0.0f;
        }
        wg_barrier();
#define QPN_PDOT(s, acc) if constexpr (QPN_TVALID(s)) { acc = tree_reduce_c<LOGRS>(chunk16(QPN_TB(s), xq)); } QPN_TLOAD((s) + 3)
        if constexpr (W0 < G::NP1) {
            float4 xq[4]; read_x(xq, p.o_y1 + 16 * qs);
            float pa[T1];
            if constexpr (0 < T1) { QPN_PDOT(0, pa[0]) } if constexpr (1 < T1) { QPN_PDOT(1, pa[1 < T1 ? 1 : 0]) }
            if constexpr (2 < T1) { QPN_PDOT(2, pa[2 < T1 ? 2 : 0]) } if constexpr (3 < T1) { QPN_PDOT(3, pa[3 < T1 ? 3 : 0]) }
            if (qs == 0) {
#pragma unroll
                for (int i = 0; i < T1; ++i) if (W0 + i * NWV < G::NP1) {
                    const int row = (wave + i * NWV) * RPTS + grps;
                    const float v = pa[i] + sm[f.b_p1 + row];
                    sm[p.o_y2 + row] = v > 0.0f ? v : 0.0f;
                }
            }
        } else {                                            // no post #1 tile here: its slots of the sequence are free at once
            if constexpr (0 < T1) { QPN_TLOAD(3) } if constexpr (1 < T1) { QPN_TLOAD(4) } if constexpr (2 < T1) { QPN_TLOAD(5) }
        }
        wg_barrier();
        if constexpr (W0 < G::NP2) {
            float4 xq[4]; read_x(xq, p.o_y2 + 16 * qs);
            float pa[T2];
            if constexpr (0 < T2) { QPN_PDOT(T1 + 0, pa[0]) } if constexpr (1 < T2) { QPN_PDOT(T1 + 1, pa[1 < T2 ? 1 : 0]) }
            if constexpr (2 < T2) { QPN_PDOT(T1 + 2, pa[2 < T2 ? 2 : 0]) } if constexpr (3 < T2) { QPN_PDOT(T1 + 3, pa[3 < T2 ? 3 : 0]) }
            if (qs == 0) {
#pragma unroll
                for (int i = 0; i < T2; ++i) if (W0 + i * NWV < G::NP2) sm[p.o_lg + (wave + i * NWV) * RPTS + grps] = pa[i] + sm[f.b_p2 + (wave + i * NWV) * RPTS + grps];
            }
        }
#undef QPN_PDOT
        QPN_STAMP();
        // ---- end of step: this step's layer inputs x_1..x_{L-1} go to their rings (one row each) ...
        for (int i = tid; i < (L - 1) * C; i += NTH) {
            const int l1 = 1 + i / C, row = i % C;
            const RingDesc r = p.rings[l1];
            st_agent(u.ring + r.base + (size_t)((unsigned)t % (unsigned)r.len) * C + row, sm[p.o_xbuf + l1 * p.Cp + row]);
        }
        QPN_STAMP();
        QPN_STAMP_DUMP();
        // the LDS stop word is written in the pick below only: read here, between two barriers of the step, every wave finds what the previous
        // step's pick left -- the same value in all of them -- and the workgroup leaves together once this step has drained
        const int stop = p.cancel ? __builtin_amdgcn_readfirstlane(smi[p.o_samp + 2]) : 0;
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): the ring rows have left the wave
        wg_barrier();
        // ... layer-0 tiles of the next step fly while the sample is picked, the next layer-0 input looked up and the
        // aux terms / past rows staged
        QPN_ZINIT(wl, 0) QPN_ZINIT(wl, 1) QPN_ZINIT(wl, 2) QPN_ZINIT(wl, 3)
        QPN_RINIT(wl, 0) QPN_RINIT(wl, 1) QPN_RINIT(wl, 2) QPN_RINIT(wl, 3)
        if (wave == 0) {
            float bv = -INFINITY; int bi = 0x7fffffff;
            for (int i = lane; i < Q; i += 64) { const float v = sm[p.o_lg + i]; if (v > bv) { bv = v; bi = i; } }
            bi = wave_argmax(bv, bi);
            const int i = t - (u.n0 - 1);
            if (i >= 0 && u.logits) for (int k = lane; k < Q; k += 64) u.logits[(size_t)i * Q + k] = sm[p.o_lg + k];
            int next;
            if (i >= 0) {
                if (p.mode != QPN_MODE_ARGMAX) bi = sample_pick<ROW>(p, (unsigned)u.row, one_cu_rowd(p), p.o_lg, Q, (unsigned)i, lane);
                next = bi;
                if (u.teacher) { const int64_t sv = u.teacher[i] % Q; next = (int)(sv < 0 ? sv + Q : sv); }
                if (lane == 0) u.out[i] = bi;
            } else next = u.known[t + 1];
            const int cur = smi[p.o_samp + 1];
            if (t + 2 < Ttot) causal_rows(p, u, cur, next, t + 1, lane);
            if (lane == 0) { smi[p.o_samp] = cur; smi[p.o_samp + 1] = next; }
            // live output BEHIND the causal rows: the load of the host's stop word, a round trip to host memory that later loads of this wave queue up
            // behind, is issued once the next step's layer-0 input is in LDS.  Stop on request: the workgroup leaves after the next step
            if (i >= 0 && lane == 0 && live_put(p, u, i, bi, creq)) smi[p.o_samp + 2] = 1;
        } else {
            const int stid = (wave - 1) * 64 + lane, nst = (NWV - 1) * 64;
            int fdw = 0;      // draw track: the next step's frame record, requested in front of the staging loads and stored behind them (its pick is a step away)
            if constexpr (ROW == 2) if (t + 2 < Ttot) fdw = frame_draw_load(p, u, t + 1, stid);
            for (int i = stid; i < S; i += nst) { sm[p.o_skf + i] = 0.0f; sm[p.o_ska + i] = 0.0f; }
            if (t + 2 < Ttot) stage_aux(p, u, t + 1, stid, nst);
            if (t + 3 < Ttot) stage_taps(p, u, t + 2, stid, nst, p.status);
            if constexpr (ROW == 2) if (t + 2 < Ttot) frame_draw_store(u, t + 1, one_cu_rowd(p), stid, fdw);
        }
        if (stop) break;    // stopped on request at the previous step's publish point (this step has drained: its pick published nothing)
    }
#undef QPN_STAMP
#undef QPN_STAMP_DUMP
#undef QPN_ZPTR
#undef QPN_RPTR
#undef QPN_ZINIT
#undef QPN_RINIT
#undef QPN_TB
#undef QPN_TVALID
#undef QPN_TLOAD
#undef QPN_ZSLOT
#undef QPN_RDOT
#undef QPN_RPUT
#undef QPN_LAYER
}

template <int C, int S, int Q, int NWV, bool RESL, int ROW, int W0>
__device__ __forceinline__ void fast_dispatch(const DecodeParams& p, const FastParams& f, const UttView& u,
                                              const int wave, const int lane, const int tid, const int Ttot) {
    constexpr int NB = FastGeo<C, S, Q, NWV>::next_boundary(W0);
    if constexpr (NB >= NWV) fast_steps<C, S, Q, NWV, RESL, ROW, W0>(p, f, u, wave, lane, tid, Ttot);
    else {
        if (wave < NB) fast_steps<C, S, Q, NWV, RESL, ROW, W0>(p, f, u, wave, lane, tid, Ttot);
        else fast_dispatch<C, S, Q, NWV, RESL, ROW, NB>(p, f, u, wave, lane, tid, Ttot);
    }
}

// RESL: the residual-1x1 tiles of layers 0..L-2 (the ones on the critical path of every R phase) live in LDS for the whole
// launch: 16 fewer 1 KiB requests per layer through the serial vector-memory front end, and the waves that own them never
// block on it.  The host picks RESL when the tiles fit beside the step state (paper-size: 112 KiB + 38 KiB).
#define QPN_KERNEL k_decode_fast
#define QPN_KERNEL_ROW false
#include "decode_fast_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#define QPN_KERNEL k_decode_fast_r      // ... of the calls with per-row records
#define QPN_KERNEL_ROW true
#include "decode_fast_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#define QPN_KERNEL k_decode_fast_t      // ... of the calls with a draw track
#define QPN_KERNEL_ROW 2
#include "decode_fast_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW

// ================================================================== host side
static thread_local char g_err[512] = "";
void qpn_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* qpn_last_error(void) { return g_err; }
extern "C" int qpn_version(void) { return 1006; }

extern "C" int64_t qpn_param_count(const qpn_config* cfg) {
    Geom g; if (qpn_build_geom(cfg, &g) != QPN_OK) return -1; return g.n_params;
}


// the DecodeParams every call starts from: the geometry and the program's LDS layout, member by member -- the one place the two structs meet (pointers and the
// members of a call stay null / 0)
static DecodeParams decode_params_template(const Geom& g, const DecodeProgram& d) {
    DecodeParams p = {};
    const DecodeLds& s = d.lds;
    p.n_slots = d.n_slots;
    p.C = g.C; p.Cp = g.Cp; p.S = g.S; p.Q = g.Q; p.L = g.L; p.U = g.U;
    p.causal_w = g.causal_w; p.causal_b = g.causal_b; p.up_w = g.up_w;
    p.o_xbuf = s.o_xbuf; p.o_xp = s.o_xp; p.o_pd = s.o_pd; p.o_auxv = s.o_auxv; p.o_g = s.o_g; p.o_skf = s.o_skf; p.o_ska = s.o_ska; p.o_y1 = s.o_y1; p.o_y2 = s.o_y2;
    p.o_lg = s.o_lg; p.o_samp = s.o_samp; p.o_sel = s.o_sel; p.o_gl = s.o_gl; p.state_floats = s.state_floats;
    p.o_bias = s.o_bias; p.n_bias = s.n_bias; p.o_tasks = s.o_tasks; p.lds_floats = s.lds_floats;
    return p;
}

// The handle under construction is the guard's: every early return destroys it
extern "C" int qpn_create(const qpn_config* cfg, qpn_handle** out) {
    if (!out) { qpn_set_error("null out"); return QPN_EINVAL; }
    *out = nullptr;
    std::unique_ptr<qpn_handle, void (*)(qpn_handle*)> h(new qpn_handle(), qpn_destroy);
    int rc = qpn_build_geom(cfg, &h->g);
    if (rc != QPN_OK) return rc;
    {   // the environment is read HERE, once per handle: no decode or training call looks at it again
        DecodeKnobs& k = h->dk;
        k.generic = getenv("QPN_DECODE_GENERIC") != nullptr;
        k.no_resl = getenv("QPN_DECODE_NO_RESL") != nullptr;
        k.coop = 0; if (const char* e = getenv("QPN_DECODE_COOP")) k.coop = atoi(e) > 0 ? atoi(e) : 0;
        // (measured on one MI355X, repo-default geometry, us per sample step of the whole batch, batched / per-utterance kernel: B = 1: 89 / 92, 2: 90 / 97, 4: 98 / 110,
        //  8: 115 / 123, 16: 137 / 143, 20: 147 / 200, 32: 165 / 204, 64: 216 / 357 -- profiles/r06_coopb_batches.txt)
        k.coopb = 1; if (const char* e = getenv("QPN_DECODE_COOPB")) k.coopb = atoi(e) > 0 ? atoi(e) : 0;
        k.coopb_delay[0] = 8; k.coopb_delay[1] = 4; k.coopb_delay[2] = 0;
        if (const char* e = getenv("QPN_COOPB_DELAY_G")) k.coopb_delay[0] = atoi(e);
        if (const char* e = getenv("QPN_COOPB_DELAY_X")) k.coopb_delay[1] = atoi(e);
        if (const char* e = getenv("QPN_COOPB_DELAY_T")) k.coopb_delay[2] = atoi(e);
        k.pipe = 1; if (const char* e = getenv("QPN_DECODE_PIPE")) k.pipe = atoi(e) != 0 ? 1 : 0;
        k.stamps = getenv("QPN_STAMPS") != nullptr;
        k.test_pipe_gives_up = false;
#ifdef QPN_TESTING
        k.test_pipe_gives_up = getenv("QPN_TEST_PIPE_GIVES_UP") != nullptr;
#endif
    }
    // the decode program is decided here, without a device (decode_program.h).  A geometry it refuses still trains: the decode entry points report prog.err
    h->prog = decode_program(h->g, qpn_coopb_supported(h->g));
    if (h->prog.rc == QPN_OK) h->dp = decode_params_template(h->g, h->prog);
    else qpn_set_error("%s", h->prog.err);
    if (const char* e = getenv("QPN_PIPE_NU")) { const int v = atoi(e); if (v >= 2 && v <= 3) h->pipe_nu = v; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        // geometry-only handle: usable for qpn_param_count-style queries, every compute call fails loudly
        *out = h.release(); return QPN_OK;
    }
    QPN_HIP(hipGetDevice(&h->device));
    QPN_HIP(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->device));
    if (h->n_cus < 1) h->n_cus = 1;
    h->pipe_rows = qpn_pipe_rows_resident(h->n_cus);
    *out = h.release();
    return QPN_OK;
}

extern "C" void qpn_destroy(qpn_handle* h) {      // (every member may still be null)
    if (!h) return;
    if (h->device >= 0) {
        void* bufs[] = {h->d_map, h->d_wpk, h->d_tasks, h->d_qb, h->d_bd, h->d_status, h->d_bias_src, h->d_pproj, h->d_ring, h->d_known, h->d_utts, h->d_xch, h->d_adam_table, h->d_stats, h->d_rows, h->d_track};
        for (void* b : bufs) if (b) (void)hipFree(b);
        qpn_train_destroy(h->train);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->h_utts_pinned) (void)hipHostFree(h->h_utts_pinned);
        if (h->h_rows_pinned) (void)hipHostFree(h->h_rows_pinned);
        if (h->h_track_pinned) (void)hipHostFree(h->h_track_pinned);
        if (h->h_live) (void)hipHostFree(h->h_live);
        if (h->h_live_done) (void)hipHostFree(h->h_live_done);
        if (h->h_cancel) (void)hipHostFree(h->h_cancel);
    }
    delete h;
}

static int need_device(qpn_handle* h) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (h->device < 0) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    return QPN_OK;
}

// What the first qpn_set_weights puts on the device.  It belongs to this guard until commit() hands all of it to the handle at once: a call that fails half-way
// frees what it had, and leaves a handle whose next call allocates again
struct DecodeUploads {
    int* map = nullptr; float* wpk = nullptr; Task* tasks = nullptr; float* qb = nullptr; BiasDesc* bd = nullptr; int* status = nullptr; int* bias_src = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void commit(qpn_handle* h) {
        h->d_map = map; h->d_wpk = wpk; h->d_tasks = tasks; h->d_qb = qb; h->d_bd = bd; h->d_status = status; h->d_bias_src = bias_src; h->ev0 = ev0; h->ev1 = ev1;
        *this = DecodeUploads();
    }
    ~DecodeUploads() {
        void* bufs[] = {map, wpk, tasks, qb, bd, status, bias_src};
        for (void* b : bufs) if (b) (void)hipFree(b);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};
// device buffer of n elements, a copy of src[0 .. n) where src is given
template <class T>
static int upload(T** d, size_t n, const T* src) {
    QPN_HIP(hipMalloc(d, n * sizeof(T)));
    if (src && n) QPN_HIP(hipMemcpy(*d, src, n * sizeof(T), hipMemcpyHostToDevice));
    return QPN_OK;
}

extern "C" int qpn_set_weights(qpn_handle* h, const float* d_flat, size_t n, void* stream_) {
    int rc = need_device(h); if (rc) return rc;
    DecodeProgram& d = h->prog;
    if (d.rc != QPN_OK) { qpn_set_error("%s", d.err); return QPN_EINVAL; }
    if (!d_flat || (int64_t)n != h->g.n_params) { qpn_set_error("flat parameter vector must have %lld floats, got %zu", (long long)h->g.n_params, n); return QPN_EINVAL; }
    hipStream_t stream = (hipStream_t)stream_;
    const Geom& g = h->g;
    if (!h->d_map) {
        DecodeUploads u;
        rc = upload(&u.map, d.n_map, d.map.data()); if (rc) return rc;
        rc = upload(&u.wpk, d.n_map, (const float*)nullptr); if (rc) return rc;
        rc = upload(&u.tasks, d.n_tasks, d.tasks.data()); if (rc) return rc;
        rc = upload(&u.qb, (size_t)g.L * 2 * g.C, (const float*)nullptr); if (rc) return rc;
        rc = upload(&u.bd, (size_t)g.L, d.bd); if (rc) return rc;
        rc = upload(&u.status, 16 + 128 * QPN_NW * sizeof(long long) / sizeof(int), (const int*)nullptr); if (rc) return rc;      // the status line, then the dev stamps
        rc = upload(&u.bias_src, d.bias_src.size(), d.bias_src.data()); if (rc) return rc;
        QPN_HIP(hipEventCreate(&u.ev0)); QPN_HIP(hipEventCreate(&u.ev1));
        u.commit(h);
        std::vector<int>().swap(d.map); std::vector<Task>().swap(d.tasks); std::vector<int>().swap(d.bias_src);      // on the device now: n_map, n_tasks and lds.n_bias are what is used from here on
    }
    h->d_flat = d_flat;
    hipLaunchKernelGGL(k_pack_gather, dim3((unsigned)((d.n_map + 255) / 256)), dim3(256), 0, stream, d_flat, h->d_map, h->d_wpk, (int64_t)d.n_map);
    hipLaunchKernelGGL(k_fold_bias, dim3(g.L), dim3(256), g.Ap * sizeof(float), stream, (const float4*)h->d_wpk, d_flat, h->d_bd,
                       d.aux_woff4, d.aux_tiles, d.logRa, g.A, g.Ap, g.C, g.U > 0 ? d_flat + g.up_b : (const float*)nullptr, h->d_qb);
    QPN_HIP(hipGetLastError());
    h->have_weights = true;                              // (stream-ordered: later decode calls on this stream see the packed tiles)
    return QPN_OK;
}


template <class T>
static int grow(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return QPN_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    hipError_t e = hipMalloc(p, need * sizeof(T));
    if (e != hipSuccess) { qpn_set_error("hipMalloc(%zu bytes) failed: %s", need * sizeof(T), hipGetErrorString(e)); return QPN_ENOMEM; }
    *cap = need;
    return QPN_OK;
}

// pinned staging buffer of >= need elements (grow only)
template <class T>
static int grow_pinned(T** hp, size_t* cap, size_t need) {
    if (need <= *cap) return QPN_OK;
    if (*hp) (void)hipHostFree(*hp);
    *hp = nullptr; *cap = 0;
    QPN_HIP(hipHostMalloc((void**)hp, need * sizeof(T), hipHostMallocDefault));
    *cap = need;
    return QPN_OK;
}

// host-coherent pinned buffer of >= need elements (grow only) and the address the device uses for it
template <class T>
static int grow_coherent(T** hp, T** dp, size_t* cap, size_t need) {
    if (need <= *cap) return QPN_OK;
    if (*hp) (void)hipHostFree(*hp);
    *hp = nullptr; *dp = nullptr; *cap = 0;
    hipError_t e = hipHostMalloc((void**)hp, need * sizeof(T), hipHostMallocCoherent);
    if (e != hipSuccess) { *hp = nullptr; qpn_set_error("hipHostMalloc(%zu bytes, coherent) failed: %s", need * sizeof(T), hipGetErrorString(e)); return QPN_ENOMEM; }
    e = hipHostGetDevicePointer((void**)dp, *hp, 0);
    if (e != hipSuccess) { (void)hipHostFree(*hp); *hp = nullptr; *dp = nullptr; qpn_set_error("hipHostGetDevicePointer failed: %s", hipGetErrorString(e)); return QPN_ENODEV; }
    *cap = need;
    return QPN_OK;
}

int grow_xch(qpn_handle* h, size_t words) { return grow(&h->d_xch, &h->xch_cap, words); }
// One launch of the one-CU kernels (one 1024-thread workgroup per utterance) over the descriptors p.utts[l.first .. l.first + l.rows)
static int launch_one_cu(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream) {
    const Geom& g = h->g;
    const int n = l.rows; p.utts += l.first;
    const bool generic = h->dk.generic;
    const bool fast64 = !generic && g.C == 64 && g.S == 256 && g.Q == 256, fast32 = !generic && g.C == 32 && g.S == 32 && g.Q == 256;
    // the specialised kernel does not use the task table: the residual-1x1 tiles of layers 0..L-2 take its place (and more) when they fit
    const int stamp_floats = p.stamps ? 120 * QPN_NW : 0;
    const int nres_tiles = (g.C * g.C / 1024) * (g.L - 1);
    p.o_wres = (p.o_tasks + 3) & ~3;
    const bool trackk = p.mode == QPN_MODE_SAMPLING_TRACK;      // a draw track: the kernels whose pick reads the step's frame record (sample_pick<2>)
    const int rowd_floats = trackk ? 16 : p.row_draw ? 8 : 0;      // a call with per-row records: the row's record, behind everything else (stage_row_draw, decode_dev.h); a draw track: two frame records behind that
    const bool resl = (fast64 || fast32) && g.L >= 2 && !h->dk.no_resl &&
                      ((size_t)p.o_wres + (size_t)nres_tiles * 1024 + stamp_floats + rowd_floats) * sizeof(float) <= 160 * 1024;
    const int use_floats = resl ? p.o_wres + nres_tiles * 1024 : p.lds_floats;
    p.o_stamp = use_floats;
    const size_t lds_bytes = ((size_t)use_floats + stamp_floats + rowd_floats) * sizeof(float);
    if (rowd_floats && lds_bytes > 160 * 1024) { qpn_set_error("per-row sampling records need 32 bytes of LDS behind the %d KiB of step state of this geometry", (int)(lds_bytes >> 10)); return QPN_EINVAL; }
    typedef void (*FastKernel)(DecodeParams, FastParams);      // the ONE choice: a straight-line kernel, or (null) the interpreter
    const bool rowk = p.mode == QPN_MODE_SAMPLING_ROW;      // per-row records: the kernels whose pick reads them (sample_pick<true>)
    const FastKernel fast = trackk ? (fast64 ? (resl ? k_decode_fast_t<64, 256, 256, 16, true> : k_decode_fast_t<64, 256, 256, 16, false>)
                                    : fast32 ? (resl ? k_decode_fast_t<32, 32, 256, 16, true> : k_decode_fast_t<32, 32, 256, 16, false>) : nullptr)
                          : rowk ? (fast64 ? (resl ? k_decode_fast_r<64, 256, 256, 16, true> : k_decode_fast_r<64, 256, 256, 16, false>)
                                  : fast32 ? (resl ? k_decode_fast_r<32, 32, 256, 16, true> : k_decode_fast_r<32, 32, 256, 16, false>) : nullptr)
                          : fast64 ? (resl ? k_decode_fast<64, 256, 256, 16, true> : k_decode_fast<64, 256, 256, 16, false>)
                          : fast32 ? (resl ? k_decode_fast<32, 32, 256, 16, true> : k_decode_fast<32, 32, 256, 16, false>) : nullptr;
    typedef void (*SlotKernel)(DecodeParams);
    const bool wide = p.mode != QPN_MODE_ARGMAX && g.Q > 256;      // a sampled call at n_quantize > 256: the kernels whose pick is the wide draw (sample_pick<ROW, true>; never a straight-line kernel: those have Q = 256)
    const SlotKernel interp = wide ? (trackk ? k_decode_wt : rowk ? k_decode_wr : k_decode_w) : trackk ? k_decode_t : rowk ? k_decode_r : k_decode;
    if (lds_bytes > 48 * 1024) QPN_HIP(hipFuncSetAttribute(fast ? (const void*)fast : (const void*)interp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    if (fast) hipLaunchKernelGGL(fast, dim3(n), dim3(QPN_NT), lds_bytes, stream, p, h->prog.fp);
    else hipLaunchKernelGGL(interp, dim3(n), dim3(QPN_NT), lds_bytes, stream, p);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}

// what the planner is told: the handle's geometry and knobs, the device facts given (the handle's own, or a query's), the batch and the floats of a row's rings
static DecodePlanIn plan_inputs(const qpn_handle* h, int n_cus, int pipe_rows, int B, size_t ring_floats) {
    const Geom& g = h->g;
    DecodePlanIn in = {};
    in.C = g.C; in.S = g.S; in.Q = g.Q; in.Cp = g.Cp; in.Sp = g.Sp; in.L = g.L;
    in.single_cu_ok = h->prog.single_cu_ok; in.pipe_supported = qpn_pipe_supported(g); in.coopb_supported = h->prog.cb_ok;
    in.coopb_fits = decode_coopb_fits(in, h->prog.n_map * sizeof(float), (long long)ring_floats);
    in.n_cus = n_cus; in.pipe_rows = pipe_rows; in.pipe_nu = h->pipe_nu; in.B = B;
    in.coop = h->dk.coop; in.coopb = h->dk.coopb; in.pipe = h->dk.pipe; in.generic = h->dk.generic;
    return in;
}

// Enqueues the call h->call describes, launch by launch of its plan.  retry: nullptr, or the inputs decode_plan_retry made (qpn_decode_finish)
static int decode_enqueue_impl(qpn_handle* h, hipStream_t stream, const DecodePlanIn* retry) {
    const Geom& g = h->g;
    qpn_handle::DecodeCall& c = h->call;
    const int B = c.B, n_x = c.n_x, maxd = c.maxd; const int64_t F = c.F, Td = c.Td;
    const int64_t* h_n_samples = c.n_samples.data(); const int64_t* d_teacher = c.d_teacher; float* d_logits = c.d_logits;
    int rc; int64_t max_n = 0;
    for (int b = 0; b < B; ++b) {
        int64_t n = h_n_samples[b];
        if (n < 0) { qpn_set_error("negative n_samples"); return QPN_EINVAL; }
        if (n_x - 1 + n > Td || (g.U > 0 ? (n_x - 1 + n > F * g.U) : (n_x - 1 + n > F))) {
            qpn_set_error("row %d: n_samples=%lld exceeds the features/dilated factors provided", b, (long long)n); return QPN_EINVAL;
        }
        max_n = std::max(max_n, n);
    }
    // receptive field and left padding (qpnet.py:351-357)
    const int64_t RF = (int64_t)g.recA * maxd + g.recF + 1;
    int64_t n_pad = RF - n_x + 1; if (n_pad < 0) n_pad = 0;
    const int64_t n0 = n_pad + n_x;
    if (n0 + max_n >= ((int64_t)1 << 31)) { qpn_set_error("sequence too long"); return QPN_EINVAL; }
    DecodeParams p = h->dp;
    size_t ring_floats = 0;
    for (int l = 0; l < g.L; ++l) {
        const LayerGeom& y = g.layers[l];
        int len = (y.adaptive ? y.dilation * maxd : y.dilation) + 1;
        p.rings[l].base = (int)ring_floats; p.rings[l].len = len; p.rings[l].mult = y.dilation; p.rings[l].adaptive = y.adaptive;
        ring_floats += (size_t)len * g.C;
    }
    c.in = retry ? *retry : plan_inputs(h, h->n_cus, h->pipe_rows, B, ring_floats); c.plan = decode_plan(c.in);
    ring_floats = (ring_floats + 63) & ~(size_t)63;
    // rows are handed to the kernels longest first (descriptors are a permutation of the batch)
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return h_n_samples[a] > h_n_samples[b2]; });
    if (c.plan.needs_ring) { rc = grow(&h->d_ring, &h->ring_cap, ring_floats * (size_t)B); if (rc) return rc; }      // pitch-tap histories (one-CU kernels; role S1 of the pipelined one)
    rc = grow(&h->d_pproj, &h->pproj_cap, (size_t)B * F * g.L * 2 * g.C); if (rc) return rc;
    rc = grow(&h->d_known, &h->known_cap, (size_t)B * n0); if (rc) return rc;
    rc = grow(&h->d_utts, &h->utts_cap, (size_t)B); if (rc) return rc;
    rc = grow_pinned(&h->h_utts_pinned, &h->h_utts_cap, (size_t)B); if (rc) return rc;
    if (h->live_call) {
        // live output: the mirror and the counts grow like the descriptors; the counts are zeroed from the host (no kernel of this handle is
        // running: one decode in flight, and the re-run of qpn_decode_finish comes after a stream synchronisation)
        rc = grow_coherent(&h->h_live, &h->d_live, &h->live_cap, (size_t)B * (size_t)std::max<int64_t>(max_n, 1)); if (rc) return rc;
        rc = grow_coherent(&h->h_live_done, &h->d_live_done, &h->live_done_cap, (size_t)B); if (rc) return rc;
        rc = grow_coherent(&h->h_cancel, &h->d_cancel, &h->cancel_cap, (size_t)16); if (rc) return rc;      // (the stop request of qpn_decode_cancel: a 64-byte line of its own)
        for (int b = 0; b < B; ++b) __atomic_store_n(&h->h_live_done[b], 0LL, __ATOMIC_RELEASE);
        __atomic_store_n(h->h_cancel, 0, __ATOMIC_RELEASE);
        h->live_stride = max_n;
        p.live = h->d_live; p.live_done = h->d_live_done; p.live_every = h->live_every; p.cancel = h->d_cancel;
    }
    UttDesc* utts = h->h_utts_pinned;      // pinned and owned by the handle (one decode in flight per handle): no host synchronisation here
    for (int k = 0; k < B; ++k) {
        const int b = order[k];
        UttDesc& u = utts[k];
        u.pproj = (int64_t)b * F * g.L * 2 * g.C;
        u.dfac = (int64_t)b * Td;
        u.known = (int64_t)b * n0;
        u.teacher = d_teacher ? (int64_t)b * max_n : -1;
        u.out = (int64_t)b * max_n;
        u.logits = d_logits ? (int64_t)b * max_n * g.Q : -1;
        u.ring = (int64_t)k * ring_floats;
        u.n_pad = (int)n_pad; u.n0 = (int)n0; u.n_samples = (int)h_n_samples[b]; u.d_is_f32 = c.d_is_f32; u.F = F;
        u.row = b; u.pad_ = 0;
    }
    QPN_HIP(hipMemcpyAsync(h->d_utts, utts, (size_t)B * sizeof(UttDesc), hipMemcpyHostToDevice, stream));
    const bool track = c.mode == QPN_MODE_SAMPLING && c.track;                 // a draw track (qpn_decode_frame_sampling): the table goes from the setter's pinned staging, no host wait
    const bool row_draw = c.mode == QPN_MODE_SAMPLING && (!c.rows.empty() || track);      // per-row records (qpn_decode_row_sampling): staged and copied like the descriptors, no host wait
    if (row_draw) {
        rc = grow(&h->d_rows, &h->rows_cap, (size_t)B); if (rc) return rc;
        rc = grow_pinned(&h->h_rows_pinned, &h->h_rows_cap, (size_t)B); if (rc) return rc;      // (a track call: the setter has sized it)
        if (!c.rows.empty()) memcpy(h->h_rows_pinned, c.rows.data(), (size_t)B * sizeof(RowDraw));
        else for (int b = 0; b < B; ++b) {      // a track without records: key and counter word of the uniform call, (call seed, batch row); the track kernels read nothing else of it
            RowDraw& o = h->h_rows_pinned[b];
            o.seed_lo = (unsigned)c.seed; o.seed_hi = (unsigned)(c.seed >> 32); o.stream = (unsigned)b;
            o.inv_temp = c.inv_temp; o.top_k = c.top_k; o.top_p = c.top_p; o.min_p = c.min_p; o.pad_ = 0;
        }
        QPN_HIP(hipMemcpyAsync(h->d_rows, h->h_rows_pinned, (size_t)B * sizeof(RowDraw), hipMemcpyHostToDevice, stream));
    }
    if (track) {
        const size_t n = (size_t)B * (size_t)F;      // (the enqueue has checked B and F against the table)
        rc = grow(&h->d_track, &h->track_cap, n); if (rc) return rc;
        QPN_HIP(hipMemcpyAsync(h->d_track, h->h_track_pinned, n * sizeof(FrameDraw), hipMemcpyHostToDevice, stream));
    }
    if (c.plan.needs_ring) QPN_HIP(hipMemsetAsync(h->d_ring, 0, ring_floats * (size_t)B * sizeof(float), stream));
    QPN_HIP(hipMemsetAsync(h->d_status, 0, 64, stream));
    hipLaunchKernelGGL(k_known, dim3((unsigned)((n0 + 255) / 256), B), dim3(256), 0, stream, c.d_x, n_x, (int)n_pad, g.Q, h->d_known);
    hipLaunchKernelGGL(k_aux_project, dim3((unsigned)F, B), dim3(256), g.Ap * sizeof(float), stream, (const float4*)h->d_wpk, c.d_h, F,
                       h->prog.aux_woff4, h->prog.aux_tiles, h->prog.logRa, g.A, g.Ap, g.C, g.L, h->d_pproj);
    p.wpk = (const float4*)h->d_wpk; p.flat = h->d_flat; p.qb = h->d_qb; p.tasks = h->d_tasks; p.utts = h->d_utts;
    p.status = h->d_status; p.mode = c.mode; p.seed = c.seed; p.bias_src = h->d_bias_src;
    p.inv_temp = c.inv_temp; p.top_k = c.top_k; p.top_p = c.top_p; p.min_p = c.min_p;
    if (c.mode == QPN_MODE_SAMPLING && (c.inv_temp != 1.0f || c.top_k != 0 || c.top_p != 1.0f || c.min_p != 0.0f)) p.mode = QPN_MODE_SAMPLING_CTL;
    if (row_draw) { p.mode = QPN_MODE_SAMPLING_ROW; p.row_draw = h->d_rows; }      // the records take the place of the call's seed and of the four uniform values
    if (track) { p.mode = QPN_MODE_SAMPLING_TRACK; p.frame_draw = h->d_track; p.n_frames = F; }      // ... and the track's frame records the place of the four values
    p.stamps = h->dk.stamps ? (long long*)(h->d_status + 16) : nullptr;
    p.pproj = h->d_pproj; p.dfac = c.d_dfac; p.known = h->d_known; p.teacher = d_teacher; p.out = c.d_out; p.logits = d_logits; p.ring = h->d_ring;
    QPN_HIP(hipEventRecord(h->ev0, stream));
    for (int i = 0; i < c.plan.launches; ++i) {
        const DecodeLaunch l = decode_plan_launch(c.in, c.plan, i);
        rc = c.plan.kind == DECODE_COOPB ? qpn_launch_decode_coopb(h, p, l, stream) : c.plan.kind == DECODE_COOP ? qpn_launch_decode_coop(h, p, l, c.plan.G, stream)
           : c.plan.kind == DECODE_PIPE ? qpn_launch_decode_pipe(h, p, l, stream) : launch_one_cu(h, p, l, stream);
        if (rc) return rc;
    }
    char text[160]; decode_plan_text(c.in, c.plan, text, sizeof(text)); h->plan = text;
    QPN_HIP(hipEventRecord(h->ev1, stream));
    h->pending = true;
    return QPN_OK;
}

extern "C" int qpn_decode_enqueue(qpn_handle* h, int B, int n_x, int64_t F, int64_t Td,
                                  const int64_t* d_x, const float* d_h, const void* d_dfac, int d_is_f32,
                                  const int64_t* h_n_samples, int maxd, int mode, uint64_t seed,
                                  const int64_t* d_teacher, int64_t* d_out, float* d_logits, void* stream_) {
    int rc = need_device(h); if (rc) return rc;
    if (!h->have_weights) { qpn_set_error("qpn_set_weights must be called before qpn_decode"); return QPN_ESTATE; }
    if (h->pending) { qpn_set_error("one decode in flight per handle: call qpn_decode_finish first"); return QPN_ESTATE; }
    if (B < 1 || n_x < 1 || F < 1 || !d_x || !d_h || !d_dfac || !h_n_samples || !d_out || maxd < 1) { qpn_set_error("bad decode arguments"); return QPN_EINVAL; }
    if (mode != QPN_MODE_ARGMAX && mode != QPN_MODE_SAMPLING) { qpn_set_error("mode must be QPN_MODE_ARGMAX or QPN_MODE_SAMPLING"); return QPN_EINVAL; }
    if (mode == QPN_MODE_SAMPLING && (h->g.Q < 64 || h->g.Q % 64 || h->g.Q > 1024)) { qpn_set_error("sampling needs n_quantize in {64,128,...,1024} (a multiple of 64)"); return QPN_EINVAL; }
    if (mode == QPN_MODE_SAMPLING && !h->samp_rows.empty() && (size_t)B != h->samp_rows.size()) {
        qpn_set_error("B = %d rows, but qpn_decode_row_sampling set n_rows = %zu records (one per batch row; n_rows = 0 switches them off)", B, h->samp_rows.size()); return QPN_EINVAL;
    }
    if (mode == QPN_MODE_SAMPLING && h->track_rows > 0) {
        if (B != h->track_rows) { qpn_set_error("B = %d rows, but qpn_decode_frame_sampling set n_rows = %d (one track per batch row; n_rows = 0 switches the track off)", B, h->track_rows); return QPN_EINVAL; }
        if (F != h->track_frames) { qpn_set_error("F = %lld frames, but qpn_decode_frame_sampling set n_frames = %lld (one record per feature frame of h)", (long long)F, (long long)h->track_frames); return QPN_EINVAL; }
    }
    qpn_handle::DecodeCall& c = h->call;
    c.B = B; c.n_x = n_x; c.F = F; c.Td = Td; c.d_x = d_x; c.d_h = d_h; c.d_dfac = d_dfac; c.d_is_f32 = d_is_f32;
    c.n_samples.assign(h_n_samples, h_n_samples + B); c.maxd = maxd; c.mode = mode; c.seed = seed;
    c.inv_temp = h->samp_inv_temp; c.top_k = h->samp_top_k; c.top_p = h->samp_top_p; c.min_p = h->samp_min_p;
    if (mode == QPN_MODE_SAMPLING) c.rows = h->samp_rows; else c.rows.clear();
    c.track = mode == QPN_MODE_SAMPLING && h->track_rows > 0;
    c.d_teacher = d_teacher; c.d_out = d_out; c.d_logits = d_logits;
    h->live_call = h->live_every > 0;
    h->live_final = false;
    if (h->live_call) {
        if (d_teacher || d_logits) { h->live_call = false; qpn_set_error("live output is not offered together with teacher forcing or the logits output"); return QPN_EINVAL; }
        h->live_seen.assign((size_t)B, 0);
    }
    return decode_enqueue_impl(h, (hipStream_t)stream_, nullptr);
}

extern "C" int qpn_decode_live(qpn_handle* h, int every) {
    int rc = need_device(h); if (rc) return rc;
    if (every < 0) { qpn_set_error("every must be >= 1 (arm) or 0 (disarm)"); return QPN_EINVAL; }
    if (h->pending) { qpn_set_error("a decode is in flight: call qpn_decode_finish first"); return QPN_ESTATE; }
    h->live_every = every;
    return QPN_OK;
}

// the argument checks qpn_decode_sampling(_ex) and qpn_sample_logits(_ex) share: -> 1 / temperature, and top_k with "every class" (0 or Q) as 0
static int sampling_controls(float temperature, int top_k, float top_p, float min_p, int Q, float* inv_temp, int* k) {
    if (!(temperature > 0.0f) || std::isinf(temperature)) { qpn_set_error("temperature must be a finite number > 0 (got %g)", (double)temperature); return QPN_EINVAL; }
    const float inv = 1.0f / temperature;
    if (!std::isfinite(inv)) { qpn_set_error("temperature %g is too small: 1 / temperature is not a finite float", (double)temperature); return QPN_EINVAL; }
    if (top_k < 0 || top_k > Q) { qpn_set_error("top_k must be 0 (off) or 1..n_quantize = %d (got %d)", Q, top_k); return QPN_EINVAL; }
    if (!(top_p > 0.0f) || top_p > 1.0f) { qpn_set_error("top_p must lie in (0, 1] (1: off; got %g)", (double)top_p); return QPN_EINVAL; }
    if (!(min_p >= 0.0f) || min_p > 1.0f) { qpn_set_error("min_p must lie in [0, 1] (0: off; got %g)", (double)min_p); return QPN_EINVAL; }
    *inv_temp = inv; *k = top_k == Q ? 0 : top_k;
    return QPN_OK;
}

extern "C" int qpn_decode_sampling_ex(qpn_handle* h, float temperature, int top_k, float top_p, float min_p) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    float inv; int k;
    int rc = sampling_controls(temperature, top_k, top_p, min_p, h->g.Q, &inv, &k); if (rc) return rc;
    if (h->pending) { qpn_set_error("a decode is in flight: call qpn_decode_finish first"); return QPN_ESTATE; }
    h->samp_inv_temp = inv; h->samp_top_k = k; h->samp_top_p = top_p; h->samp_min_p = min_p;
    return QPN_OK;
}
extern "C" int qpn_decode_sampling(qpn_handle* h, float temperature, int top_k) { return qpn_decode_sampling_ex(h, temperature, top_k, 1.0f, 0.0f); }

extern "C" int qpn_decode_row_sampling(qpn_handle* h, int n_rows, const qpn_row_draw* h_rows) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (n_rows < 0) { qpn_set_error("n_rows must be >= 0 (0: off; got %d)", n_rows); return QPN_EINVAL; }
    if (n_rows > 0 && !h_rows) { qpn_set_error("h_rows is NULL with n_rows = %d", n_rows); return QPN_EINVAL; }
    std::vector<RowDraw> rows((size_t)n_rows);
    for (int b = 0; b < n_rows; ++b) {
        const qpn_row_draw& r = h_rows[b];
        float inv; int k;
        if (sampling_controls(r.temperature, r.top_k, r.top_p, r.min_p, h->g.Q, &inv, &k)) {      // the rules and messages of qpn_decode_sampling_ex, with the row in front
            const std::string why = qpn_last_error();
            qpn_set_error("row %d: %s", b, why.c_str()); return QPN_EINVAL;
        }
        RowDraw& o = rows[(size_t)b];
        o.seed_lo = (unsigned)r.seed; o.seed_hi = (unsigned)(r.seed >> 32); o.stream = r.stream;
        o.inv_temp = inv; o.top_k = k; o.top_p = r.top_p; o.min_p = r.min_p; o.pad_ = 0;
    }
    if (h->pending) { qpn_set_error("a decode is in flight: call qpn_decode_finish first"); return QPN_ESTATE; }
    h->samp_rows.swap(rows);
    return QPN_OK;
}

extern "C" int qpn_decode_frame_sampling(qpn_handle* h, int n_rows, int64_t n_frames, const qpn_frame_draw* h_track) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (n_rows < 0) { qpn_set_error("n_rows must be >= 0 (0: off; got %d)", n_rows); return QPN_EINVAL; }
    if (n_rows > 0 && n_frames < 1) { qpn_set_error("n_frames must be >= 1 (got %lld)", (long long)n_frames); return QPN_EINVAL; }
    if (n_rows > 0 && !h_track) { qpn_set_error("h_track is NULL with n_rows = %d", n_rows); return QPN_EINVAL; }
    if (n_rows > 0 && n_frames > (int64_t)(((size_t)1 << 40) / (size_t)n_rows)) { qpn_set_error("a track of %d x %lld records is too large", n_rows, (long long)n_frames); return QPN_EINVAL; }
    const size_t n = n_rows > 0 ? (size_t)n_rows * (size_t)n_frames : 0;
    std::vector<FrameDraw> track(n);
    for (size_t i = 0; i < n; ++i) {
        const qpn_frame_draw& r = h_track[i];
        float inv; int k;
        if (sampling_controls(r.temperature, r.top_k, r.top_p, r.min_p, h->g.Q, &inv, &k)) {      // the rules and messages of qpn_decode_sampling_ex, with the row and the frame in front
            const std::string why = qpn_last_error();
            qpn_set_error("row %d frame %lld: %s", (int)(i / (size_t)n_frames), (long long)(i % (size_t)n_frames), why.c_str()); return QPN_EINVAL;
        }
        FrameDraw& o = track[i];
        o.inv_temp = inv; o.top_k = k; o.top_p = r.top_p; o.min_p = r.min_p;
    }
    if (h->pending) { qpn_set_error("a decode is in flight: call qpn_decode_finish first"); return QPN_ESTATE; }
    if (n && h->device >= 0) {      // the pinned staging the enqueue copies from (and that of the records it makes for a call without any): allocated here, so that the enqueue allocates nothing on the host
        int rc = grow_pinned(&h->h_track_pinned, &h->h_track_cap, n); if (rc) return rc;
        rc = grow_pinned(&h->h_rows_pinned, &h->h_rows_cap, (size_t)n_rows); if (rc) return rc;
        memcpy(h->h_track_pinned, track.data(), n * sizeof(FrameDraw));
    }
    h->track_rows = n_rows; h->track_frames = n_rows > 0 ? n_frames : 0;
    return QPN_OK;
}

extern "C" int qpn_decode_poll(qpn_handle* h, int64_t* h_done, const int32_t** h_samples, int64_t* row_stride, int* running) {
    int rc = need_device(h); if (rc) return rc;
    if (!h_done || !h_samples || !row_stride || !running) { qpn_set_error("null argument"); return QPN_EINVAL; }
    if (!h->pending) { qpn_set_error("no decode in flight"); return QPN_ESTATE; }
    if (!h->live_call) { qpn_set_error("the decode in flight was enqueued without live output (qpn_decode_live)"); return QPN_ESTATE; }
    // the event first: once it has completed, the counts read below are the launch's last ones
    const hipError_t q = hipEventQuery(h->ev1);
    if (q != hipSuccess && q != hipErrorNotReady) { qpn_set_error("hipEventQuery failed: %s", hipGetErrorString(q)); return QPN_ENODEV; }
    if (q == hipErrorNotReady) (void)hipGetLastError();      // (not an error: do not leave it for the next launch check to find)
    *running = q == hipErrorNotReady ? 1 : 0;
    for (int b = 0; b < h->call.B; ++b) {
        const int64_t v = (int64_t)__atomic_load_n(&h->h_live_done[b], __ATOMIC_ACQUIRE);
        if (v > h->live_seen[b]) h->live_seen[b] = v;
        h_done[b] = h->live_seen[b];
    }
    *h_samples = h->h_live; *row_stride = h->live_stride;
    return QPN_OK;
}

extern "C" int qpn_decode_cancel(qpn_handle* h) {
    int rc = need_device(h); if (rc) return rc;
    if (!h->pending) { qpn_set_error("no decode in flight"); return QPN_ESTATE; }
    if (!h->live_call) { qpn_set_error("the decode in flight was enqueued without live output (qpn_decode_live): it has no publish points to stop at"); return QPN_ESTATE; }
    __atomic_store_n(h->h_cancel, 1, __ATOMIC_RELEASE);      // one store to host-coherent memory: no stream work, no wait; the kernels find it at their next publish point
    return QPN_OK;
}

extern "C" int qpn_decode_final_counts(qpn_handle* h, int64_t* h_done, int* cancelled) {
    int rc = need_device(h); if (rc) return rc;
    if (!h_done || !cancelled) { qpn_set_error("null argument"); return QPN_EINVAL; }
    if (h->pending) { qpn_set_error("a decode is in flight: call qpn_decode_finish first"); return QPN_ESTATE; }
    if (!h->live_final) { qpn_set_error("the last decode was not enqueued with live output (qpn_decode_live) and finished"); return QPN_ESTATE; }
    bool any_short = false;
    for (int b = 0; b < h->call.B; ++b) {
        h_done[b] = (int64_t)__atomic_load_n(&h->h_live_done[b], __ATOMIC_ACQUIRE);
        any_short = any_short || h_done[b] < h->call.n_samples[(size_t)b];
    }
    *cancelled = (__atomic_load_n(h->h_cancel, __ATOMIC_ACQUIRE) != 0 && any_short) ? 1 : 0;
    return QPN_OK;
}

extern "C" const char* qpn_last_decode_plan(qpn_handle* h) { return h ? h->plan.c_str() : ""; }

extern "C" int qpn_decode_plan_query(qpn_handle* h, int n_cus, int B, int attempt, char* buf, size_t cap) {
    if (!h || !buf || cap < 1 || B < 1 || attempt < 0 || attempt > 1) { qpn_set_error("bad plan query arguments"); return QPN_EINVAL; }
    if (h->prog.rc != QPN_OK) { qpn_set_error("%s", h->prog.err); return QPN_EINVAL; }
    const int pipe_rows = n_cus > 0 ? (n_cus / 40) * 8 : h->pipe_rows;
    if (n_cus <= 0) n_cus = h->n_cus;
    if (n_cus < 1) { qpn_set_error("no HIP device: the query needs n_cus"); return QPN_ENODEV; }
    DecodePlanIn in = plan_inputs(h, n_cus, pipe_rows, B, 0);      // (no call, no rings: see the header)
    DecodePlan plan = decode_plan(in);
    if (attempt && !decode_plan_retry(in, plan)) { qpn_set_error("this plan has no retry: one workgroup per utterance already"); return QPN_ESTATE; }
    decode_plan_text(in, plan, buf, cap);
    return QPN_OK;
}

extern "C" int qpn_decode_finish(qpn_handle* h, void* stream_) {
    int rc = need_device(h); if (rc) return rc;
    if (!h->pending) { qpn_set_error("no decode in flight"); return QPN_ESTATE; }
    hipStream_t stream = (hipStream_t)stream_;
    QPN_HIP(hipStreamSynchronize(stream));
    h->pending = false;
    int status = 0;
    QPN_HIP(hipMemcpy(&status, h->d_status, sizeof(int), hipMemcpyDeviceToHost));
    QPN_HIP(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    // A stop request (qpn_decode_cancel) ends the call: a multi-workgroup launch that stopped on it has drained through the give-up path (its peers
    // set status bit 4 when they see the abort flag), and a launch that had given up before the request is not completed either -- no re-run, and the
    // drain is not reported as QPN_ENODEV.  The rows' final counts: qpn_decode_final_counts.
    const bool stop_requested = h->live_call && __atomic_load_n(h->h_cancel, __ATOMIC_ACQUIRE) != 0;
    h->live_final = h->live_call;
    if (stop_requested) status &= ~4;
    if (status & 4) {
        // A multi-workgroup launch gave up: its workgroups were not all resident together (CU-masked or shared GPU, another kernel holding CUs).  Every wait
        // in those kernels is bounded, the grid has drained; run the batch again with a smaller footprint where decode_plan_retry has one.
        DecodePlanIn in = h->call.in; DecodePlan again = h->call.plan;
        if (decode_plan_retry(in, again)) {
            const std::string first_plan = h->plan;
            rc = decode_enqueue_impl(h, stream, &in); if (rc) return rc;
            QPN_HIP(hipStreamSynchronize(stream));
            h->pending = false;
            h->plan = first_plan + " -> timed out, retried: " + h->plan;
            QPN_HIP(hipMemcpy(&status, h->d_status, sizeof(int), hipMemcpyDeviceToHost));
            float ms2 = 0.f; QPN_HIP(hipEventElapsedTime(&ms2, h->ev0, h->ev1)); h->last_ms += ms2;
        }
    }
    if (h->dk.stamps) {      // dev aid: stamp times (cycles, relative to the first stamp of wave 0) of step 3000
        std::vector<long long> st((size_t)120 * QPN_NW);
        QPN_HIP(hipMemcpy(st.data(), h->d_status + 16, st.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int s = 0; s < 40; ++s) {
            fprintf(stderr, "stamp %2d:", s);
            for (int w = 0; w < QPN_NW; w += 5) fprintf(stderr, " w%-2d %7lld", w, st[(size_t)s * QPN_NW + w] - st[0]);
            fprintf(stderr, "\n");
        }
    }
    if (status & 4) { qpn_set_error("decode: a workgroup timed out waiting for its peers (is another job holding CUs of this GPU?)"); return QPN_ENODEV; }
    if (status & 1) { qpn_set_error("pitch-dependent tap left its ring buffer (dilated factor <= 0.5 or > maxd)"); return QPN_ERANGE; }
    return QPN_OK;
}

extern "C" int qpn_decode(qpn_handle* h, int B, int n_x, int64_t F, int64_t Td,
                          const int64_t* d_x, const float* d_h, const void* d_dfac, int d_is_f32,
                          const int64_t* h_n_samples, int maxd, int mode, uint64_t seed,
                          const int64_t* d_teacher, int64_t* d_out, float* d_logits, void* stream) {
    int rc = qpn_decode_enqueue(h, B, n_x, F, Td, d_x, d_h, d_dfac, d_is_f32, h_n_samples, maxd, mode, seed, d_teacher, d_out, d_logits, stream);
    if (rc) return rc;
    return qpn_decode_finish(h, stream);
}

extern "C" float qpn_last_decode_kernel_ms(qpn_handle* h) { return h ? h->last_ms : 0.0f; }

// ---------------------------------------------------------------- dilated index builders
__global__ void k_didx_train(const float* __restrict__ d, int64_t L, int dilation, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; const int b = blockIdx.y;
    if (i < L) {
        float dil = -d[(size_t)b * L + i] * (float)dilation;
        float s = __fadd_rn(dil, (float)(i - L));
        out[(size_t)b * L + i] = (int64_t)rintf(s);
    }
}
__global__ void k_didx_gen32(const float* __restrict__ d, int64_t n, int dilation, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int64_t)rintf(-d[i] * (float)dilation);
}
__global__ void k_didx_gen64(const double* __restrict__ d, int64_t n, int dilation, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)rint(-d[i] * (double)dilation);
}
// ---------------------------------------------------------------- stand-alone draw from given logits
// one wave per row: the row goes to LDS where the decode kernels keep their logits, and the wave calls the device function their picks call
__global__ __launch_bounds__(64) void k_sample_logits(const float* __restrict__ lg, int Q, unsigned long long seed, unsigned row, unsigned step0,
                                                      float inv_temp, int top_k, float top_p, float min_p, int64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    const float* src = lg + (size_t)blockIdx.x * Q;
    for (int i = lane; i < Q; i += 64) SM[i] = src[i];
    __syncthreads();
    const unsigned step = step0 + blockIdx.x;
    const int bi = Q > 256 ? sample_wave_wide(0, Q, sample_uniform(seed, row, step), inv_temp, top_k, top_p, min_p, lane)      // (in place: the row's Q floats are all it needs)
                   : (inv_temp != 1.0f || top_k != 0 || top_p != 1.0f || min_p != 0.0f)
                       ? sample_wave_ctl<true>(0, Q, sample_uniform(seed, row, step), inv_temp, top_k, top_p, min_p, lane)
                       : sample_wave(0, Q, seed, row, step, lane);
    if (lane == 0) out[blockIdx.x] = bi;
}
static int dev_ok() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    return QPN_OK;
}
extern "C" int qpn_sample_logits_ex(const float* d_logits, int64_t n_rows, int Q, uint64_t seed, int row, int64_t step0, float temperature, int top_k,
                                    float top_p, float min_p, int64_t* d_out, void* stream) {
    if (Q < 64 || Q % 64 || Q > 1024) { qpn_set_error("sampling needs Q = n_quantize in {64,128,...,1024} (a multiple of 64)"); return QPN_EINVAL; }
    float inv; int k;
    int rc = sampling_controls(temperature, top_k, top_p, min_p, Q, &inv, &k); if (rc) return rc;
    if (!d_logits || !d_out || n_rows < 1 || row < 0 || step0 < 0 || step0 + n_rows > ((int64_t)1 << 31)) { qpn_set_error("bad arguments (n_rows >= 1, row >= 0, 0 <= step0, step0 + n_rows <= 2^31)"); return QPN_EINVAL; }
    rc = dev_ok(); if (rc) return rc;
    hipLaunchKernelGGL(k_sample_logits, dim3((unsigned)n_rows), dim3(64), (size_t)Q * sizeof(float), (hipStream_t)stream, d_logits, Q, (unsigned long long)seed,
                       (unsigned)row, (unsigned)step0, inv, k, top_p, min_p, d_out);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
extern "C" int qpn_sample_logits(const float* d_logits, int64_t n_rows, int Q, uint64_t seed, int row, int64_t step0, float temperature, int top_k,
                                 int64_t* d_out, void* stream) {
    return qpn_sample_logits_ex(d_logits, n_rows, Q, seed, row, step0, temperature, top_k, 1.0f, 0.0f, d_out, stream);
}
extern "C" int qpn_dilated_index_train(const float* d_d, int B, int64_t L, int dilation, int64_t* d_out, void* stream) {
    int rc = dev_ok(); if (rc) return rc;
    if (!d_d || !d_out || B < 1 || L < 1) { qpn_set_error("bad arguments"); return QPN_EINVAL; }
    hipLaunchKernelGGL(k_didx_train, dim3((unsigned)((L + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, d_d, L, dilation, d_out);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
extern "C" int qpn_dilated_index_gen_f32(const float* d_d, int64_t n, int dilation, int64_t* d_out, void* stream) {
    int rc = dev_ok(); if (rc) return rc;
    if (!d_d || !d_out || n < 1) { qpn_set_error("bad arguments"); return QPN_EINVAL; }
    hipLaunchKernelGGL(k_didx_gen32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_d, n, dilation, d_out);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
extern "C" int qpn_dilated_index_gen_f64(const double* d_d, int64_t n, int dilation, int32_t* d_out, void* stream) {
    int rc = dev_ok(); if (rc) return rc;
    if (!d_d || !d_out || n < 1) { qpn_set_error("bad arguments"); return QPN_EINVAL; }
    hipLaunchKernelGGL(k_didx_gen64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_d, n, dilation, d_out);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
