// decode_coop.hip -- autoregressive decode with SEVERAL cooperating workgroups per utterance (gfx950 / MI355X).
//
// Replaces QPNet.batch_fast_generate (reference src/nets/qpnet.py:314-559) for geometries whose per-sample state and
// weight stream are too large for the one-CU-per-utterance kernels of decode.hip: the repo-default QPNet (n_resch 512,
// 16 layers: src/utils/param_model.py:58-64) touches 96 MB of weights and 1 MB of state per generated sample.
//
// Partition: workgroup g of the G that serve an utterance owns rows [g/G, (g+1)/G) of EVERY matrix (1/G of the weight
// stream, so the G CUs stream their slices from L2 / Infinity Cache in parallel).  Each dependent stage therefore ends
// with an all-gather of a short vector (C or S floats) among the G workgroups: 2 per layer + 3 for the post-net.
// The exchange is the data-tagged granule of the CDNA4 guide (Guideline 16, R2): every float travels as ONE aligned
// 8-byte {tag = step + 1, value} agent-scope store; consumers re-read their granules until the tag matches -- no flag,
// no fence, correct for any placement of the workgroups on CUs / XCDs.  The layer-input history ("ring buffers") IS the
// exchange buffer of x_l: slot t % len of ring l receives step t's x_l and is re-read later as the pitch-dependent tap.
// Buffers are reused once per generated sample; the sample-to-sample dependency (every workgroup needs ALL logits of
// step t before it can produce anything of step t+1) is the barrier that makes the reuse safe.
// Every wait is bounded: a timeout raises the abort flag, all workgroups drain and the host reports an error.
//
// Arithmetic: the fixed-order "QPNet-f32" spec -- bit-identical to the CPU oracle and to decode.hip.
#include "decode_dev.h"
#include "qpn_handle.h"
#include <string.h>

typedef unsigned long long u64;
#ifndef COOP_NT
#define COOP_NT 768      // 12 waves: 1024 threads cap the kernel at 128 registers (29 spilled, 112 bytes of scratch per lane re-read inside the
#endif                   // per-sample loop); measured at C = 512: 8.98 / 52.9 / 81.5 k samples/s for 1 / 8 / 20 utterances vs 8.84 / 45.4 / 75.2 k (512 threads: 8.69 / 49.9 / 66.7 k)
#define COOP_NW (COOP_NT / 64)
#define COOP_SPIN_LIMIT (1u << 22)

__device__ __forceinline__ void gr_store(u64* g, unsigned tag, float v) {
    __hip_atomic_store(g, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 gr_load(const u64* g) {
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first ceil(n / 256) waves fetch n granules of step `tag` into LDS: four granules per lane per sweep, re-read until every tag
// matches (a few polling waves instead of one polling lane per granule: pollers next to a weight stream cost bandwidth)
__device__ __forceinline__ void gather_vec(const u64* src, int n, unsigned tag, float* dst, int tid, int* abort, int* status) {
    const int base = (tid >> 6) * 256 + (tid & 63);
    if ((tid >> 6) * 256 >= n) return;
    u64 v[4];
    unsigned spins = 0;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + 64 * k;
            v[k] = i < n ? gr_load(src + i) : ((u64)tag << 32);
            ok &= (unsigned)(v[k] >> 32) == tag;
        }
        if (__all(ok)) break;
        if (++spins > COOP_SPIN_LIMIT || ((spins & 255u) == 0 && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            __hip_atomic_store(abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicOr(status, 4);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int i = base + 64 * k; if (i < n) dst[i] = __uint_as_float((unsigned)v[k]); }
}

#define QPN_KERNEL k_decode_coop
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE false
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coop_r      // ... of the calls with per-row records
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE false
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coop_t      // ... of the calls with a draw track
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE false
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
// ... and the three again for the sampled calls at n_quantize > 256: their picks run the wide draw (sample_pick<ROW, true>, decode_dev.h)
#define QPN_KERNEL k_decode_coop_w
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE true
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coop_wr
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE true
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coop_wt
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE true
#include "decode_coop_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE

// ------------------------------------------------------------------------------------------ host side
// l.rows utterances from l.first on (the kernel's b0), G workgroups each: the caller's launches hold no more than are resident together (one workgroup per CU)
int qpn_launch_decode_coop(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, int G, hipStream_t stream) {
    const Geom& g = h->g; const DecodeProgram& d = h->prog;
    const int L = g.L, C = g.C, S = g.S, Q = g.Q;
    CoopParams c; memset(&c, 0, sizeof(c));
    c.G = G; c.CB = C / G; c.SB = S / G; c.QB = Q / G; c.Sp = g.Sp;
    c.logR = ilog2(g.Cp / 16); c.rpt = 64 / (g.Cp / 16); c.logRs = ilog2(g.Sp / 16); c.rpts = 64 / (g.Sp / 16);
    long o = 0;
    for (int l = 0; l < L; ++l) { c.o_ring[l] = (int)o; o += (long)p.rings[l].len * C; c.w_past_il[l] = d.w_past_il[l];
                                  c.f_resb[l] = d.f_resb[l]; c.f_skipb[l] = d.f_skipb[l]; }
    c.o_g = (int)o; o += (long)L * C; c.o_y1 = (int)o; o += S; c.o_y2 = (int)o; o += S; c.o_lg = (int)o; o += Q;
    o = (o + 15) & ~15L;
    if (o >= (1L << 31)) { qpn_set_error("cooperative decode: exchange block too large"); return QPN_EINVAL; }
    c.utt_stride = o; c.f_p1b = d.f_p1b; c.f_p2b = d.f_p2b;
    const size_t xwords = (size_t)o * l.rows + 16;
    int rc = grow_xch(h, xwords); if (rc) return rc;
    c.xch = h->d_xch + 16; c.abort = (int*)h->d_xch;          // first 128 bytes: the abort flag
    // LDS of the kernel
    int lds = 2 * g.Cp + L * g.Cp + g.Cp + 2 * g.Sp + ((Q + 3) & ~3) + ((2 * c.SB + 3) & ~3) + L * 2 * c.CB + 4 + L * (c.CB + c.SB) + c.SB + c.QB;
    if (p.mode == QPN_MODE_SAMPLING_ROW) lds += 8;      // a call with per-row records: the row's record, eight words behind the rest (o_rd of coop_body<true>)
    if (p.mode == QPN_MODE_SAMPLING_TRACK) lds += 16;   // a call with a draw track: the record and two frame records (sample_pick<2>, decode_dev.h)
    const size_t lds_bytes = (size_t)lds * sizeof(float);
    if (lds_bytes > 160 * 1024) { qpn_set_error("cooperative decode: %zu KiB of step state per workgroup exceed LDS (use more workgroups per utterance)", lds_bytes >> 10); return QPN_EINVAL; }
    typedef void (*CoopKernel)(DecodeParams, FastParams, CoopParams, int);
    const bool wide = p.mode != QPN_MODE_ARGMAX && Q > 256;      // a sampled call at n_quantize > 256: the kernels whose pick is the wide draw (sample_pick<ROW, true>)
    const CoopKernel kfn = wide ? (p.mode == QPN_MODE_SAMPLING_TRACK ? k_decode_coop_wt : p.mode == QPN_MODE_SAMPLING_ROW ? k_decode_coop_wr : k_decode_coop_w)
                         : p.mode == QPN_MODE_SAMPLING_TRACK ? k_decode_coop_t : p.mode == QPN_MODE_SAMPLING_ROW ? k_decode_coop_r : k_decode_coop;
    QPN_HIP(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    QPN_HIP(hipMemsetAsync(h->d_xch, 0, xwords * sizeof(unsigned long long), stream));      // tags, rings, abort flag
    hipLaunchKernelGGL(kfn, dim3(G, l.rows), dim3(COOP_NT), lds_bytes, stream, p, d.fp, c, l.first);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
