// decode_coopb.hip -- cooperative autoregressive decode of the wide geometries with the UTTERANCES BATCHED INTO THE CONTRACTIONS (round 6; gfx950 / MI355X).
//
// decode_coop.hip gives every utterance its own group of workgroups: at the reference's decode batch (20 utterances, src/runQP.py:66) twenty groups each
// stream the repo-default model's 96.6 MB of weights per generated sample (9.8 TB/s aggregate -- the Infinity Cache's rate), and a row's 16-term FMA chain +
// cross-lane tree is a ~350-cycle dependent chain per (row tile, utterance).  Here ONE group of G = n_resch / 8 workgroups serves up to 16 utterances: the
// utterances are the N dimension of v_mfma_f32_16x16x4_f32, a workgroup's 16 rows of a matrix the M dimension, and the weights are read ONCE per sample step
// for all of them.  Reference: QPNet.batch_fast_generate, src/nets/qpnet.py:314-559 (the per-sample loop :446-557).
//
// Arithmetic: the fixed-order "QPNet-f32" spec, bit for bit.  Four chained MFMAs (accumulator 0, k ascending) ARE the spec's 16-term
// chain p = w0 x0, fma, fma, ... (tools/mfma_chain_test.hip: 5.1 M outputs, no difference), so a chunk's accumulator tile holds chunk16 of 16 rows x 16
// utterances; the spec's stride-halving tree over the K / 16 chunks is elementwise adds of such tiles in the same association: the four waves of a dot
// product take the chunks c = j (mod 4) in the order j, j+16, j+8, j+24, j+4, j+20, j+12, j+28 (three live tiles), and (W0 + W2) + (W1 + W3) closes it.
//
// Partition and exchange as in decode_coop.hip: workgroup w owns 8 channels (gate rows sigma / tanh of them: one 16-row tile; their residual rows + its
// S / G skip rows: one tile), every dependent stage ends in an all-gather of {tag, value} granules (2 per layer + 3), the layer-input history IS the
// exchange buffer.  Vectors live in LDS as B-operand images: float4 ((chunk * 4 + k-slot) * 16 + utterance) = x[utterance][16 chunk + 4 e + k-slot], e = 0..3.
#include "decode_dev.h"
#include "qpn_handle.h"
#include <string.h>
#include <stdlib.h>

typedef unsigned long long u64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define CBB_NT 512
#define CBB_NW (CBB_NT / 64)
#define CBB_NU 16                     // utterance columns of a tile
static_assert(CBB_NU == DECODE_COOPB_NU, "the launch planner spreads a batch over groups of CBB_NU utterances");
#define CBB_SPIN_LIMIT (1u << 20)

struct CoopbParams {
    u64* xch; long utt_stride;
    int o_ring[QPN_MAX_LAYERS]; int o_g, o_y1, o_y2, o_lg;
    int* abort; unsigned wpk_bytes; long long base4; int per_w, dev_nostream, dev_nocheck, poll_delay_g, poll_delay_x, poll_delay_t;      // workgroup w's fragments: per_w float4 from base4 + w * per_w
    int G, SB, QB, NBper, B;          // workgroups of a group (8 channels each); skip / logit rows per workgroup; utterances per group; utterances of the call
    int RC, RS;                       // 16-deep chunks of K = n_resch / K = n_skipch
    int zc[QPN_MAX_LAYERS], zp[QPN_MAX_LAYERS], rs[QPN_MAX_LAYERS], p1, p2;      // float4 offsets of the A-operand tiles inside the workgroup's fragment block: word chunk * 64 + lane
    int f_resb[QPN_MAX_LAYERS], f_skipb[QPN_MAX_LAYERS], f_p1b, f_p2b, adaptive[QPN_MAX_LAYERS];
};


typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#define CBB_SC1 16                    // cache-policy bit of the buffer accesses: sc1 (agent scope -- what the atomic accesses of the granules compile to)
#define CBB_XT 256                    // threads of the exchange waves

#define CBB_LT 10                     // ints per layer of the LDS layer table: granule offset of the ring, its length, adaptive?, fragment blocks zc / zp / rs, the step's slot (either parity), dilation
// (CBB_FRESH: a thread index made opaque, so that the compiler recomputes what derives from it at every use instead of keeping dozens of
//  loop-invariant offsets alive across the whole step -- they spilled)
#define CBB_FRESH(x) asm volatile("" : "+v"(x))

__host__ __device__ static inline int cbb_lds_floats(int C, int L) {
    return 4 * C * CBB_NU + 4 * 256 + 2 * 4 * 256 + 2 * 256 + 2 * 8 * CBB_NU + 2 * L * 8 + 8 + 16 + 2 * L * CBB_NU + L * CBB_LT + 2 * CBB_NU + 4 * CBB_NU + 2 * CBB_NU + 2 * CBB_NU + 4 + 32 + 1 + CBB_NU * 22;
}
// float offset, inside a B-operand image, of element (channel ch, utterance n)
__device__ __forceinline__ int img_idx(int ch, int n) { return (((((ch >> 4) << 2) + (ch & 3)) * CBB_NU + n) << 2) + ((ch >> 2) & 3); }
// two granules (adjacent channels, one tag) with one 16-byte store; each half validates itself, so the halves may become visible apart
__device__ __forceinline__ void gb_store2(__amdgpu_buffer_rsrc_t rs, int goff, unsigned tag, float v0, float v1) {
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(v0), tag, __float_as_uint(v1), tag}, rs, goff * 8, 0, CBB_SC1);
}
__device__ __forceinline__ void gb_store1(__amdgpu_buffer_rsrc_t rs, int goff, unsigned tag, float v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64((u32x2){__float_as_uint(v), tag}, rs, goff * 8, 0, CBB_SC1);
}

// ---- all-gather of one vector of every utterance of the group, by the 256 threads of the exchange waves.  An item is a PAIR of granules (channels 2 pr,
// 2 pr + 1 of utterance n: one 16-byte load; each half carries its own tag, so a torn pair is simply read again); a thread owns the items (n0 + k * per, pr),
// k = 0 .. NK - 1 (NK compiled for the group's size), and has them all in flight.  tags[n] == 0: the utterance has nothing here (a tap before time 1, or finished) -- zeros, no load.
// IMG: into a B-operand image, else plain [n][count].
struct GSrc { int src0, stride; const int* soff; const unsigned* tags; int hshift; int nocheck; int nlo; };      // granule offset of utterance 0's vector, utterance stride, per-utterance slots, tags, log2(pairs), (dev) no tag check, first utterance of this call's share
template <int NK> struct GBatch { u32x4 v[NK]; unsigned want[NK]; int voff[NK]; };
template <int NK>
__device__ __forceinline__ void g_issue(GBatch<NK>& b, __amdgpu_buffer_rsrc_t rs, const GSrc& s, int nb, int xt, int kb) {
    CBB_FRESH(xt);
    const int per = CBB_XT >> s.hshift, n0 = xt >> s.hshift, pr = xt & ((1 << s.hshift) - 1);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int n = s.nlo + n0 + (kb + k) * per;
        const bool in = n < nb;
        b.want[k] = in ? s.tags[n] : 0u;
        b.voff[k] = (s.src0 + (in ? n * s.stride + (s.soff ? s.soff[n] : 0) : 0) + 2 * pr) * 8;
        b.v[k] = (u32x4){0u, 0u, 0u, 0u};
        if (b.want[k]) b.v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, b.voff[k], 0, CBB_SC1);
    }
}
template <int NK, bool IMG>
__device__ __forceinline__ void g_finish(GBatch<NK>& b, __amdgpu_buffer_rsrc_t rs, const GSrc& s, float* dstbase, int count, int nb, int xt, int kb, int* abort, int* status) {
    unsigned spins = 0;
    if (!s.nocheck)
    for (;;) {
        unsigned bad = 0u;      // (one test for the round that succeeds: no branch per item)
#pragma unroll
        for (int k = 0; k < NK; ++k) bad |= b.want[k] ? ((b.v[k].y ^ b.want[k]) | (b.v[k].w ^ b.want[k])) : 0u;
        if (!bad) break;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (b.want[k] && (b.v[k].y != b.want[k] || b.v[k].w != b.want[k])) b.v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, b.voff[k], 0, CBB_SC1);
        if (++spins > CBB_SPIN_LIMIT || ((spins & 255u) == 0 && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            __hip_atomic_store(abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicOr(status, 4);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    CBB_FRESH(xt);
    const int per = CBB_XT >> s.hshift, n0 = xt >> s.hshift, pr = xt & ((1 << s.hshift) - 1);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int n = s.nlo + n0 + (kb + k) * per;
        if (n < nb) {      // (an utterance without a tag loaded nothing: its registers are the zeros of g_issue)
            const float a = __uint_as_float(b.v[k].x), c = __uint_as_float(b.v[k].z);
            if (IMG) { const int d = img_idx(2 * pr, n); dstbase[d] = a; dstbase[d + 4 * CBB_NU] = c; }      // channel 2 pr + 1: the next k-slot
            else *(float2*)(dstbase + n * count + 2 * pr) = make_float2(a, c);
        }
    }
}
template <int NK, bool IMG>
__device__ __forceinline__ void gather1_n(__amdgpu_buffer_rsrc_t rs, const GSrc& sa, float* da, int count, int nb, int xt, int kb, int* abort, int* status) {
    GBatch<NK> a;
    g_issue(a, rs, sa, nb, xt, kb);
    g_finish<NK, IMG>(a, rs, sa, da, count, nb, xt, kb, abort, status);
}
template <int NK>
__device__ __forceinline__ void gather2_n(__amdgpu_buffer_rsrc_t rs, const GSrc& sa, float* da, const GSrc& sb, float* db, bool two, int count, int nb, int xt, int kb, int* abort, int* status) {
    GBatch<NK> a, b;
    g_issue(a, rs, sa, nb, xt, kb);
    if (two) g_issue(b, rs, sb, nb, xt, kb);
    g_finish<NK, true>(a, rs, sa, da, count, nb, xt, kb, abort, status);
    if (two) g_finish<NK, true>(b, rs, sb, db, count, nb, xt, kb, abort, status);
}
// (the poll loop's instruction count is on the critical path of every exchange: it is compiled for exactly 1 .. 8 items per thread, and for 10 and 12; 13 .. 16 take two rounds)
#define CBB_BY_ITEMS(n_, kb_, CALL) do { switch (n_) { case 1: CALL(1, kb_); break; case 2: CALL(2, kb_); break; case 3: CALL(3, kb_); break; case 4: CALL(4, kb_); break; \
    case 5: CALL(5, kb_); break; case 6: CALL(6, kb_); break; case 7: CALL(7, kb_); break; default: CALL(8, kb_); break; } } while (0)
template <bool IMG>
__device__ __forceinline__ void gather1(__amdgpu_buffer_rsrc_t rs, const GSrc& sa, float* da, int count, int nb, int xt, int* abort, int* status) {
    const int per = CBB_XT >> sa.hshift, iters = (nb - sa.nlo + per - 1) / per;
#define CBB_G1(NK, KB) gather1_n<NK, IMG>(rs, sa, da, count, nb, xt, KB, abort, status)
    if (iters <= 8) { CBB_BY_ITEMS(iters, 0, CBB_G1); }
    else if (iters <= 10) CBB_G1(10, 0);      // (groups of 9..16 utterances: still one round -- a second one costs a round trip per edge)
    else if (iters <= 12) CBB_G1(12, 0);
    else { CBB_G1(8, 0); const int m = iters - 8; CBB_BY_ITEMS(m, 8, CBB_G1); }      // (16 in flight spill)
#undef CBB_G1
}
// two vectors of the same length at once (the second only if `two`)
__device__ __forceinline__ void gather2(__amdgpu_buffer_rsrc_t rs, const GSrc& sa, float* da, const GSrc& sb, float* db, bool two, int count, int nb, int xt, int* abort, int* status) {
    const int per = CBB_XT >> sa.hshift, iters = (nb - sa.nlo + per - 1) / per;
#define CBB_G2(NK, KB) gather2_n<NK>(rs, sa, da, sb, db, two, count, nb, xt, KB, abort, status)
    for (int kb = 0; kb < iters; kb += 8) { const int m = iters - kb; CBB_BY_ITEMS(m, kb, CBB_G2); }
#undef CBB_G2
}

// ---- a compute wave's share of a dot product over R chunks: the chunks c = j + 4 i (i = 0 .. R / 4 - 1), their A fragments in registers, each a chain of
// four MFMAs from accumulator 0, combined in the spec's tree order
// (buffer loads: the block's offset is a scalar, the lane's a 32-bit register -- no 64-bit per-lane addresses to keep)
__device__ __forceinline__ void load_frags(float4 (&an)[8], __amdgpu_buffer_rsrc_t rw, unsigned blk4, int R, int j, int lane) {
    CBB_FRESH(lane);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (4 * i < R) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, lane * 16, (int)((blk4 + (unsigned)(j + 4 * i) * 64u) * 16u), 0);
            an[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
}
// (written step-major: the k-th MFMA of all the chunks, then the next -- eight independent accumulator chains in flight instead of one chain after another)
template <int NCH>
__device__ __forceinline__ void chunk_tiles(const float4 (&an)[8], const float* img, int j, int lane, f32x4 (&acc)[8]) {
    float4 b[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) b[i] = *(const float4*)(img + ((((j + 4 * i) << 2) + (lane >> 4)) * CBB_NU + (lane & 15)) * 4);
#pragma unroll
    for (int i = 0; i < NCH; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[i].x, b[i].x, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NCH; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[i].y, b[i].y, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NCH; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[i].z, b[i].z, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NCH; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[i].w, b[i].w, acc[i], 0, 0, 0);
}
__device__ __forceinline__ f32x4 wave_dot(const float4 (&an)[8], const float* img, int R, int j, int lane) {
    CBB_FRESH(lane);
    f32x4 t[8];
    if (R == 32) {      // fragment i = chunk j + 4 i; the tree pairs chunks 16 apart, then 8, then 4: (t0 + t4) + (t2 + t6), (t1 + t5) + (t3 + t7)
        chunk_tiles<8>(an, img, j, lane, t);
        return ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
    }
    // R == 16: chunks j, j+4, j+8, j+12: (t0 + t2) + (t1 + t3)
    chunk_tiles<4>(an, img, j, lane, t);
    return (t[0] + t[2]) + (t[1] + t[3]);
}
// element (row r, utterance n) of a dot product from the four waves' partial tiles (the tree's last two levels)
__device__ __forceinline__ float close_elem(const float* P, int r, int n) {
    const int o = (((r >> 2) * 16 + n) << 2) + (r & 3);
    return (P[o] + P[512 + o]) + (P[256 + o] + P[768 + o]);
}
// Waves 0..3 COMPUTE: every dot product, A fragments prefetched a layer ahead into three register sets (current tap / past tap / residual + skip) -- these
// waves issue no other global access, so the in-order return of their loads never holds up anything but the weight stream itself.
// Waves 4..7 EXCHANGE: tags and tap distances, layer 0's input, the aux terms, every publish and every gather.
#define QPN_KERNEL k_decode_coopb
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE false
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coopb_r      // ... of the calls with per-row records
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE false
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coopb_t      // ... of the calls with a draw track
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE false
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
// ... and the three again for the sampled calls at n_quantize > 256: their picks run the wide draw (sample_pick<ROW, true>, decode_dev.h)
#define QPN_KERNEL k_decode_coopb_w
#define QPN_KERNEL_ROW false
#define QPN_KERNEL_WIDE true
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coopb_wr
#define QPN_KERNEL_ROW true
#define QPN_KERNEL_WIDE true
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE
#define QPN_KERNEL k_decode_coopb_wt
#define QPN_KERNEL_ROW 2
#define QPN_KERNEL_WIDE true
#include "decode_coopb_kernel.h"
#undef QPN_KERNEL
#undef QPN_KERNEL_ROW
#undef QPN_KERNEL_WIDE

// ------------------------------------------------------------------------------------------ host side
// geometries this kernel takes: 8 channels per workgroup make the gate tile; S / G and Q / G rows fit their tiles; K = 256 or 512 chunks trees
bool qpn_coopb_supported(const Geom& g) {
    if (g.L < 2 || g.C % 8 || g.C < 128 || g.S > g.C || g.Q > g.C) return false;      // (the skip / logit vectors reuse the channel images)
    if ((g.C & (g.C - 1)) || (g.S & (g.S - 1)) || (g.Q & (g.Q - 1)) || g.Q < 64) return false;      // (the gathers split a vector's granule pairs over the threads by shifts)
    const int G = g.C / 8;
    if (g.S % G || g.Q % G || g.S / G < 1 || g.S / G > 8 || g.Q / G < 1 || g.Q / G > 16) return false;
    const int RC = g.Cp / 16, RS = g.Sp / 16;
    if ((RC != 16 && RC != 32) || (RS != 16 && RS != 32) || g.Cp != g.C || g.Sp != g.S) return false;
    return (size_t)cbb_lds_floats(g.C, g.L) * sizeof(float) <= 160 * 1024;
}

// l.rows utterances on l.groups groups of C / 8 workgroups, l.per_group each (the plan has checked that 32-bit byte offsets reach: decode_coopb_fits)
int qpn_launch_decode_coopb(qpn_handle* h, DecodeParams p, const DecodeLaunch& l, hipStream_t stream) {
    const Geom& g = h->g; const DecodeProgram& d = h->prog;
    const int B = l.rows; p.utts += l.first;
    const int L = g.L, C = g.C, S = g.S, Q = g.Q;
    CoopbParams c; memset(&c, 0, sizeof(c));
    c.G = C / 8; c.SB = S / c.G; c.QB = Q / c.G; c.RC = g.Cp / 16; c.RS = g.Sp / 16; c.B = B;
    long o = 0;
    for (int l = 0; l < L; ++l) {
        c.o_ring[l] = (int)o; o += (long)p.rings[l].len * C;
        c.zc[l] = d.cb_zc[l]; c.zp[l] = d.cb_zp[l]; c.rs[l] = d.cb_rs[l];
        c.f_resb[l] = d.f_resb[l]; c.f_skipb[l] = d.f_skipb[l]; c.adaptive[l] = d.fp.adaptive[l];
    }
    c.p1 = d.cb_p1; c.p2 = d.cb_p2; c.base4 = d.cb_base4; c.per_w = d.cb_per_w;
    c.wpk_bytes = (unsigned)(d.n_map * sizeof(float));
    c.o_g = (int)o; o += (long)L * C; c.o_y1 = (int)o; o += S; c.o_y2 = (int)o; o += S; c.o_lg = (int)o; o += Q;
    o = (o + 15) & ~15L;
    c.utt_stride = o; c.f_p1b = d.f_p1b; c.f_p2b = d.f_p2b;
    if (l.per_group < 1 || l.per_group > CBB_NU || l.groups * l.per_group < B) { qpn_set_error("internal: %d utterances do not fit %d batched groups of %d", B, l.groups, l.per_group); return QPN_EINVAL; }
    c.NBper = l.per_group;
    const size_t xwords = (size_t)o * B + 16;
    int rc = grow_xch(h, xwords); if (rc) return rc;
    c.xch = h->d_xch + 16; c.abort = (int*)h->d_xch;
    const bool rowk = p.mode == QPN_MODE_SAMPLING_ROW;      // per-row records: the kernel whose pick reads them (sample_pick<true>), and 16 records of LDS behind the rest
    const bool trackk = p.mode == QPN_MODE_SAMPLING_TRACK;  // a draw track: its kernel (sample_pick<2>), and two frame records more per utterance
    const size_t lds_bytes = ((size_t)cbb_lds_floats(C, L) + (trackk ? CBB_NU * 16 : rowk ? CBB_NU * 8 : 0)) * sizeof(float);
    if (lds_bytes > 160 * 1024) { qpn_set_error("per-row sampling records need 512 (a draw track: 1024) bytes of LDS behind the %d KiB of this geometry's batched cooperative kernel", (int)(lds_bytes >> 10)); return QPN_EINVAL; }
    // first poll of an edge's gather: 8 / 4 x 128 clocks after the exchange waves reach it (QPN_COOPB_DELAY_G / _X / _T, dev).  Polls sent before anything can have been
    // published return stale a round trip later and load the memory side the publishes go through: B = 20: 151 -> 113 us per step, B = 4: 98.6 -> 91.3, B = 64: 220 -> 189
    // (tools/coopb_delay_sweep.py, profiles/r06_coopb_poll_delay.txt)
    c.poll_delay_g = h->dk.coopb_delay[0]; c.poll_delay_x = h->dk.coopb_delay[1]; c.poll_delay_t = h->dk.coopb_delay[2];
#ifdef QPN_ENABLE_STAMPS
    c.dev_nostream = getenv("QPN_COOPB_NOSTREAM") ? 1 : 0; c.dev_nocheck = getenv("QPN_COOPB_NOCHECK") ? 1 : 0;
#endif
    typedef void (*CoopbKernel)(const DecodeParams, const CoopbParams);
    const bool wide = p.mode != QPN_MODE_ARGMAX && Q > 256;      // a sampled call at n_quantize > 256: the kernels whose pick is the wide draw (sample_pick<ROW, true>)
    const CoopbKernel kfn = wide ? (trackk ? k_decode_coopb_wt : rowk ? k_decode_coopb_wr : k_decode_coopb_w) : trackk ? k_decode_coopb_t : rowk ? k_decode_coopb_r : k_decode_coopb;
    QPN_HIP(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    QPN_HIP(hipMemsetAsync(h->d_xch, 0, xwords * sizeof(unsigned long long), stream));      // tags, rings, abort flag
#ifdef QPN_TESTING
    if (h->dk.test_pipe_gives_up) {
        // test hook (a -DQPN_TESTING build only): the launch behaves as if a wait had timed out at once (abort flag raised, status bit 4): exercises the
        // re-run on the per-utterance cooperative kernel without needing a CU-masked device (tests/test_decode_gpu.py)
        static const int one = 1, four = 4;
        QPN_HIP(hipMemcpyAsync(h->d_xch, &one, sizeof(int), hipMemcpyHostToDevice, stream));
        QPN_HIP(hipMemcpyAsync(h->d_status, &four, sizeof(int), hipMemcpyHostToDevice, stream));
    }
#endif
    hipLaunchKernelGGL(kfn, dim3(c.G, l.groups), dim3(CBB_NT), lds_bytes, stream, p, c);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
