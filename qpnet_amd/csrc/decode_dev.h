// decode_dev.h -- device-side pieces shared by the decode kernels (decode.hip: one workgroup per utterance;
// decode_coop.hip: several cooperating workgroups per utterance).  Arithmetic = the fixed-order "QPNet-f32" spec of
// DESIGN.md section 3 (bit-identical to oracle/qpnet_oracle.c); compile with -ffp-contract=off.
#pragma once
#include "qpn_common.h"

// ================================================================== device helpers
// File-scope LDS symbol: device functions index it directly, so the compiler keeps address space 3
// (a generic float* would turn every LDS access into a FLAT op that also waits on the global-load queue).
extern __shared__ float4 qpn_lds[];
#define SM ((float*)qpn_lds)
#define SMI ((int*)qpn_lds)
__device__ __forceinline__ float qexp(float x) {
    x = fminf(fmaxf(x, -87.0f), 88.0f);
    float n = rintf(x * 0x1.715476p+0f);
    float r = __builtin_fmaf(n, -0x1.63p-1f, x);
    r = __builtin_fmaf(n, 0x1.bd0106p-13f, r);
    float p = 0x1.a01a02p-13f;
    p = __builtin_fmaf(p, r, 0x1.6c16c2p-10f);
    p = __builtin_fmaf(p, r, 0x1.111112p-7f);
    p = __builtin_fmaf(p, r, 0x1.555556p-5f);
    p = __builtin_fmaf(p, r, 0x1.555556p-3f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return p * __int_as_float(((int)n + 127) << 23);
}
__device__ __forceinline__ float qgate(float zs, float zt) {
    float ea = qexp(-zs);
    float eb = qexp(-2.0f * fabsf(zt));
    float num = 1.0f - eb;
    float den = (1.0f + ea) * (1.0f + eb);
    return copysignf(num / den, zt);
}

// 16-deep chunk of the spec dot product: p = w0*x0, then 15 fma in k order.
__device__ __forceinline__ float chunk16(const float4 (&w)[4], const float4 (&x)[4]) {
    float acc = w[0].x * x[0].x;
    acc = __builtin_fmaf(w[0].y, x[0].y, acc);
    acc = __builtin_fmaf(w[0].z, x[0].z, acc);
    acc = __builtin_fmaf(w[0].w, x[0].w, acc);
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        acc = __builtin_fmaf(w[j].x, x[j].x, acc);
        acc = __builtin_fmaf(w[j].y, x[j].y, acc);
        acc = __builtin_fmaf(w[j].z, x[j].z, acc);
        acc = __builtin_fmaf(w[j].w, x[j].w, acc);
    }
    return acc;
}
// Same dot product, and each 1 KiB quarter of the tile is re-requested (from tp) as soon as its four FMAs have
// been issued: the tile's registers free up a quarter at a time, so the next request reaches the (serial, 16
// cycles per load) vector-memory front end ~150 cycles earlier than after the whole chain.  The scheduling
// barriers pin the loads where they are written; hipcc otherwise sinks them below the epilogue.
__device__ __forceinline__ float chunk16_reload(float4 (&w)[4], const float4 (&x)[4], const float4* __restrict__ tp) {
    float acc = w[0].x * x[0].x;
    acc = __builtin_fmaf(w[0].y, x[0].y, acc);
    acc = __builtin_fmaf(w[0].z, x[0].z, acc);
    acc = __builtin_fmaf(w[0].w, x[0].w, acc);
    __builtin_amdgcn_sched_barrier(0);
    w[0] = tp[0];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        acc = __builtin_fmaf(w[j].x, x[j].x, acc);
        acc = __builtin_fmaf(w[j].y, x[j].y, acc);
        acc = __builtin_fmaf(w[j].z, x[j].z, acc);
        acc = __builtin_fmaf(w[j].w, x[j].w, acc);
        __builtin_amdgcn_sched_barrier(0);
        w[j] = tp[j * 64];
        __builtin_amdgcn_sched_barrier(0);
    }
    return acc;
}
// stride-halving tree over the R lanes of a row group (R = 1 << logR, lanes contiguous).
// The spec order is "p_i += p_{i+s} for s = R/2 .. 1"; fp add is commutative, so every lane of the
// group ends with the same bits whether the partner is reached by xor, rotation or quad permute.
__device__ __forceinline__ float rl_f(float v, int lane_) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_)); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// (value, index) maximum over the 64 lanes, lowest index among equal values; every lane returns the winner's index.
// Four DPP steps inside the 16-lane rows, then four v_readlane pairs and uniform compares across the rows (a butterfly of
// six ds_bpermute pairs is a ~900-cycle dependent chain on the pick's critical path).
__device__ __forceinline__ int wave_argmax(float bv, int bi) {
#define QPN_AMAX(CTRL) { const float ov_ = dpp_f<CTRL>(bv); const int oi_ = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, true); \
                         if (ov_ > bv || (ov_ == bv && oi_ < bi)) { bv = ov_; bi = oi_; } }
    QPN_AMAX(0xB1) QPN_AMAX(0x4E) QPN_AMAX(0x124) QPN_AMAX(0x128)
#undef QPN_AMAX
    float rv = rl_f(bv, 0); int ri = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float ov = rl_f(bv, 16 * r); const int oi = __builtin_amdgcn_readlane(bi, 16 * r);
        if (ov > rv || (ov == rv && oi < ri)) { rv = ov; ri = oi; }
    }
    return ri;
}
__device__ __forceinline__ float tree_reduce(float acc, int logR) {
    if (logR == 2) {                       // K = 64: two quad permutes, no LDS crossbar
        acc = acc + dpp_f<0x4E>(acc);      // quad_perm [2,3,0,1]  (stride 2)
        acc = acc + dpp_f<0xB1>(acc);      // quad_perm [1,0,3,2]  (stride 1)
        return acc;
    }
    if (logR == 4) {                       // K = 256: row rotations by 8 and 4, then the quad permutes
        acc = acc + dpp_f<0x128>(acc);     // row_ror:8
        acc = acc + dpp_f<0x124>(acc);     // row_ror:4
        acc = acc + dpp_f<0x4E>(acc);
        acc = acc + dpp_f<0xB1>(acc);
        return acc;
    }
    if (logR == 1) return acc + dpp_f<0xB1>(acc);
    if (logR == 5) {                       // K = 512: the stride-16 partner through v_permlane16_swap_b32 (a VALU op of gfx950), then as K = 256.
        // swap(a, a) leaves {row0, row0, row2, row2} in the first result and {row1, row1, row3, row3} in the second: the lane's
        // partner (lane ^ 16) is the second on even rows, the first on odd rows -- no trip through the LDS crossbar (a ds_bpermute
        // per step was a 5-deep ~120-cycle chain in front of every row of the wide models' matvecs)
        const int a = __float_as_int(acc);
        const auto sw = __builtin_amdgcn_permlane16_swap(a, a, false, false);
        const float partner = __int_as_float((threadIdx.x & 16) ? (int)sw[0] : (int)sw[1]);
        acc = acc + partner;
        acc = acc + dpp_f<0x128>(acc);
        acc = acc + dpp_f<0x124>(acc);
        acc = acc + dpp_f<0x4E>(acc);
        acc = acc + dpp_f<0xB1>(acc);
        return acc;
    }
    for (int s = (1 << logR) >> 1; s >= 1; s >>= 1) acc = acc + __shfl_xor(acc, s);
    return acc;
}
__device__ __forceinline__ void load_tile(float4 (&w)[4], const float4* __restrict__ wpk, int woff4, int lane) {
    const float4* p = wpk + (size_t)woff4 + lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = p[j * 64];
}
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// Ring-buffer traffic stays inside ONE workgroup (= one CU): producer waves store, drain vmcnt and pass a workgroup
// barrier before any wave loads the row -- the visibility HIP guarantees for global memory across __syncthreads().
// Workgroup scope keeps the rows in the CU's L1 / the XCD's L2 (write-back).  Agent scope (sc1, write-through) was
// measured to push every 4-byte store to the fabric: 2.0 KB written + ~1.8 KB fetched per generated sample
// (profiles/r01_decode_traffic_pmc.txt) against 172 B of algorithmic HBM bytes.
__device__ __forceinline__ float ld_agent(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_agent(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---------------------------------------------------------------- sampling mode (reference qpnet.py:507-510)
// softmax + categorical draw by inverse CDF with a counter-based generator (Philox4x32-10, counter = (step, row),
// key = seed), in the fixed order of DESIGN.md §3 so that the CPU oracle reproduces every draw bit for bit.
// (Parity with the reference's torch.Generator stream is statistical only.)  One wave, Q = 64 * per: per <= 4 here, in registers; per = 5..16 in sample_wave_wide below, the same arithmetic on weights kept in LDS.
__device__ __forceinline__ unsigned philox_first(unsigned c0, unsigned c1, unsigned k0, unsigned k1) {
    unsigned c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned row, unsigned step) {
    return (float)(philox_first(step, row, (unsigned)seed, (unsigned)(seed >> 32)) >> 8) * 0x1p-24f;
}

// inverse-CDF draw over the Q logits at SM[o_lg..]; `u` is the step's uniform (sample_uniform), which does not depend on the
// logits and can be computed while the producer is still working
__device__ __forceinline__ int sample_wave_u(int o_lg, int Q, float u, int lane) {
    const float* lg = SM + o_lg;
    const int per = Q >> 6;
    float l[4], e[4];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) { l[j] = j < per ? lg[lane * per + j] : -INFINITY; m = fmaxf(m, l[j]); }
    m = fmaxf(m, dpp_f<0xB1>(m)); m = fmaxf(m, dpp_f<0x4E>(m)); m = fmaxf(m, dpp_f<0x124>(m)); m = fmaxf(m, dpp_f<0x128>(m));
    // (every lane of a 16-lane row now holds the row's maximum: four v_readlane instead of two ds_bpermute round trips; max and
    //  min are order-independent, so the bits are the spec's)
    m = fmaxf(fmaxf(rl_f(m, 0), rl_f(m, 16)), fmaxf(rl_f(m, 32), rl_f(m, 48)));
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = j < per ? qexp(l[j] - m) : 0.0f;
    float a = e[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) if (j < per) a = a + e[j];
    float v = a;
    {   // d = 1 through the wave-wide DPP shift (wave_shr:1, lane 0 reads 0), the wider strides through the LDS crossbar
        const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); if (lane >= 1) v = v + up;
    }
    for (int d = 2; d < 64; d <<= 1) { const float up = __shfl_up(v, d); if (lane >= d) v = v + up; }
    const float total = rl_f(v, 63);
    float c = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
    if (lane == 0) c = 0.0f;
    const float th = u * total;
    int idx = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < per) { c = c + e[j]; if (idx == 0x7fffffff && c > th) idx = lane * per + j; }
#define QPN_IMIN(CTRL) { const int o_ = __builtin_amdgcn_update_dpp(0x7fffffff, idx, CTRL, 0xf, 0xf, false); idx = o_ < idx ? o_ : idx; }
    QPN_IMIN(0xB1) QPN_IMIN(0x4E) QPN_IMIN(0x124) QPN_IMIN(0x128)            // within rows of 16 lanes
#undef QPN_IMIN
    {
        const int i0 = __builtin_amdgcn_readlane(idx, 0), i1 = __builtin_amdgcn_readlane(idx, 16), i2 = __builtin_amdgcn_readlane(idx, 32), i3 = __builtin_amdgcn_readlane(idx, 48);
        const int a01 = i0 < i1 ? i0 : i1, a23 = i2 < i3 ? i2 : i3;
        idx = a01 < a23 ? a01 : a23;
    }
    return idx == 0x7fffffff ? Q - 1 : idx;
}

__device__ __forceinline__ int sample_wave(int o_lg, int Q, unsigned long long seed, unsigned row, unsigned step, int lane) {
    return sample_wave_u(o_lg, Q, sample_uniform(seed, row, step), lane);
}

// ---------------------------------------------------------------- sampling controls (qpn_decode_sampling)
// The draw above with a temperature (invT = 1 / T, formed on the host) and a top-k cut: e_c = qexp((l_c - m) * invT) for the classes of the
// kept set K = { c : l_c >= k-th largest logit } (ties with the k-th are all kept; k == 0 or k >= Q: every class), 0 otherwise; the pick is the
// first class OF K whose running cumulative exceeds th, or the highest class of K when none does.  invT == 1 and k == 0 give sample_wave_u's
// bits, but the call sites take that function then (sample_pick below): this one is reached by calls that set a control.
//
// The k-th largest logit is selected in registers.  A logit maps to a 32-bit key whose unsigned order is the float order (-0.0 is made +0.0
// first; the lanes' padding slots hold key 0, below every finite or infinite float's); the threshold key is built from the top bit down:
// a candidate stays when at least k keys reach it -- `per` compares and `per` scalar pop-counts, every intermediate wave-uniform, no LDS and no
// cross-lane data movement.  A candidate that exactly k keys reach ends the search early: those k keys are the k largest, and nothing tied
// with the smallest of them lies outside (it would reach the candidate too), so { key >= candidate } is K.  Distinct logits end it after the
// bits that tell the k-th from the (k+1)-th largest apart; rows with ties at the k-th value run all 32.
__device__ __forceinline__ unsigned sample_key(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// top_p / min_p (qpn_decode_sampling_ex), on the weights e[] of the kept set, in registers.
// nucleus_mass is S(w) of the spec for the weight whose bit pattern is `cand`: weights below it count as 0.0f, a lane's `per` weights are summed left to
// right, and the 64 lane sums in a balanced pairwise tree -- lane ^ 1, lane ^ 2 (quad permutes), then the other quad of the half row (row_half_mirror: the
// quads are uniform by then), the other half of the row (row_mirror), and the four rows as (r0 + r1) + (r2 + r3).  fp32 addition is commutative, so both
// sides of every pair compute the same bits.  Weights are non-negative floats: their bit patterns order as unsigned integers.
__device__ __forceinline__ float nucleus_mass(const float (&e)[4], const unsigned (&eb)[4], unsigned cand, int per) {
    float a = eb[0] >= cand ? e[0] : 0.0f;
#pragma unroll
    for (int j = 1; j < 4; ++j) if (j < per) a = a + (eb[j] >= cand ? e[j] : 0.0f);
    a = a + dpp_f<0xB1>(a); a = a + dpp_f<0x4E>(a); a = a + dpp_f<0x141>(a); a = a + dpp_f<0x140>(a);
    return (rl_f(a, 0) + rl_f(a, 16)) + (rl_f(a, 32) + rl_f(a, 48));
}
// min_p: a class stays when its weight is >= min_p (the maximum's weight is exactly 1.0f: it always stays).  top_p: N = { e >= w* }, w* the largest weight
// of the row with S(w*) >= top_p * S(0).  The threshold key is built from bit 30 down like the top-k threshold, a candidate staying when its mass reaches
// the target; every intermediate is wave-uniform.  Sets { e >= cand } are nested, so a candidate that as many weights reach as the current threshold (or as
// the last rejected candidate) has that one's set and is decided by its ballot count; the search ends when exactly one weight separates the two, because
// every later candidate then has one set or the other.  The empty set counts as rejected (its mass 0 is below every target: top_p > 0, S(0) >= 1).
__device__ __forceinline__ void nucleus_cut(float (&e)[4], bool (&keep)[4], float top_p, float min_p, int per) {
    unsigned eb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { keep[j] = keep[j] && e[j] >= min_p; e[j] = keep[j] ? e[j] : 0.0f; eb[j] = __float_as_uint(e[j]); }
    if (!(top_p < 1.0f)) return;
    const float target = top_p * nucleus_mass(e, eb, 0u, per);
    unsigned thr = 0u;
    int c_thr = 0, c_rej = 0;       // how many weights reach thr (at thr == 0: the positive ones, which carry all of S(0)) / the last rejected candidate
#pragma unroll
    for (int j = 0; j < 4; ++j) c_thr += __builtin_popcountll(__builtin_amdgcn_ballot_w64(eb[j] != 0u));
    for (int bit = 30; bit >= 0 && c_thr - c_rej > 1; --bit) {
        const unsigned cand = thr | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(eb[j] >= cand));
        const bool stays = cnt == c_thr || (cnt != c_rej && nucleus_mass(e, eb, cand, per) >= target);
        if (stays) { thr = cand; c_thr = cnt; } else c_rej = cnt;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { keep[j] = keep[j] && eb[j] >= thr; e[j] = keep[j] ? e[j] : 0.0f; }
}
// NUC: this instantiation holds the top_p / min_p cut (behind one wave-uniform test of the two values); the pipelined kernels of the calls that set neither
// are compiled without it (k_decode_pipe_c<NU, false>), every other caller takes NUC = true
template <bool NUC>
__device__ __forceinline__ int sample_wave_ctl(int o_lg, int Q, float u, float invT, int k, float top_p, float min_p, int lane) {
    const float* lg = SM + o_lg;
    const int per = Q >> 6;
    float l[4], e[4];
    unsigned key[4];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) { l[j] = j < per ? lg[lane * per + j] : -INFINITY; m = fmaxf(m, l[j]); key[j] = j < per ? sample_key(l[j]) : 0u; }
    m = fmaxf(m, dpp_f<0xB1>(m)); m = fmaxf(m, dpp_f<0x4E>(m)); m = fmaxf(m, dpp_f<0x124>(m)); m = fmaxf(m, dpp_f<0x128>(m));
    m = fmaxf(fmaxf(rl_f(m, 0), rl_f(m, 16)), fmaxf(rl_f(m, 32), rl_f(m, 48)));
    unsigned thr = 0u;              // K = { key >= thr }: key 0 keeps every class
    if (k > 0 && k < Q) {
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = thr | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[j] >= cand));      // (padding slots: key 0 < cand)
            if (cnt >= k) thr = cand;
            if (cnt == k) break;
        }
    }
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { keep[j] = j < per && key[j] >= thr; e[j] = keep[j] ? qexp((l[j] - m) * invT) : 0.0f; }
    if constexpr (NUC) if (top_p < 1.0f || min_p > 0.0f) nucleus_cut(e, keep, top_p, min_p, per);       // the kept set becomes N, the rest of the draw is the same
    float a = e[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) if (j < per) a = a + e[j];
    float v = a;
    { const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); if (lane >= 1) v = v + up; }
    for (int d = 2; d < 64; d <<= 1) { const float up = __shfl_up(v, d); if (lane >= d) v = v + up; }
    const float total = rl_f(v, 63);
    float c = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
    if (lane == 0) c = 0.0f;
    const float th = u * total;
    int idx = 0x7fffffff, hi = -1;      // first class of K past the threshold / highest class of K, of this lane
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < per) {
        c = c + e[j];
        if (keep[j]) { hi = lane * per + j; if (idx == 0x7fffffff && c > th) idx = lane * per + j; }
    }
#define QPN_IMIN(CTRL) { const int o_ = __builtin_amdgcn_update_dpp(0x7fffffff, idx, CTRL, 0xf, 0xf, false); idx = o_ < idx ? o_ : idx; }
    QPN_IMIN(0xB1) QPN_IMIN(0x4E) QPN_IMIN(0x124) QPN_IMIN(0x128)
#undef QPN_IMIN
    {
        const int i0 = __builtin_amdgcn_readlane(idx, 0), i1 = __builtin_amdgcn_readlane(idx, 16), i2 = __builtin_amdgcn_readlane(idx, 32), i3 = __builtin_amdgcn_readlane(idx, 48);
        const int a01 = i0 < i1 ? i0 : i1, a23 = i2 < i3 ? i2 : i3;
        idx = a01 < a23 ? a01 : a23;
    }
    if (idx != 0x7fffffff) return idx;
    // no class fired (th rounded up to the scanned total, the lanes' running sums to less): the highest class of K.  Lanes hold ascending
    // class ranges, so that is the `hi` of the highest lane that kept anything
    const unsigned long long any = __builtin_amdgcn_ballot_w64(hi >= 0);
    return any ? __builtin_amdgcn_readlane(hi, 63 - __builtin_clzll(any)) : Q - 1;
}
// ---------------------------------------------------------------- the wide draw: Q = 64 * per with per in 5..16 (n_quantize 320..1024)
// The same arithmetic as sample_wave_u / sample_wave_ctl / nucleus_cut, in the same order, for the rows whose lanes own more classes than the register
// form above carries: `per` is a run-time count here and the lane's weights live in LDS -- IN PLACE of its logits.  Lane i reads and writes the slots per*i .. per*i+per-1
// only, so no other lane's data is touched and no barrier is needed; every caller has copied the logits out (u.logits) before it picks, and every producer rewrites all Q
// slots before the next pick.  No array is indexed at run time (that would be scratch memory): the draw holds a handful of registers whatever `per` is, and asks for
// no LDS beyond the Q floats of the logits (decode_program's layout, the cooperative kernels' sizes and k_sample_logits' Q * 4 bytes are what they were).
// A kept class always has a weight > 0 (qexp clamps its argument at -87: the smallest weight is about 2^-126, a normal float) and a class outside the kept set holds 0.0f,
// so "kept" is the weight's bit pattern being non-zero and no second array of flags is needed.
// The order-free passes (maximum, counts, forming the weights) visit a lane's slots rotated by rot = per * lane / 64: at per = 8 and 16 the 64 lanes then hit 64 different
// LDS banks (straight, lane * per + j puts them on 8 or 4).  The ordered passes (lane sums left to right, the running sum of the pick) cannot.
__device__ __forceinline__ int wide_rot(int j, int rot, int per) { const int r = j + rot; return r >= per ? r - per : r; }
__device__ __forceinline__ float wide_lane_tree(float a) {      // nucleus_mass's balanced tree over the 64 lane sums
    a = a + dpp_f<0xB1>(a); a = a + dpp_f<0x4E>(a); a = a + dpp_f<0x141>(a); a = a + dpp_f<0x140>(a);
    return (rl_f(a, 0) + rl_f(a, 16)) + (rl_f(a, 32) + rl_f(a, 48));
}
// S(w) for the weight whose bit pattern is `cand`, over the weights at w[0 .. per-1] of every lane
__device__ __forceinline__ float wide_mass(const float* w, int per, unsigned cand) {
    const float e0 = w[0];
    float a = __float_as_uint(e0) >= cand ? e0 : 0.0f;
    for (int j = 1; j < per; ++j) { const float e = w[j]; a = a + (__float_as_uint(e) >= cand ? e : 0.0f); }
    return wide_lane_tree(a);
}
// how many weights of the row reach `cand` (bit patterns; wave-uniform)
__device__ __forceinline__ int wide_count(const float* w, int per, int rot, unsigned cand) {
    int cnt = 0;
    for (int j = 0; j < per; ++j) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(__float_as_uint(w[wide_rot(j, rot, per)]) >= cand));
    return cnt;
}
// invT == 1, k == 0, top_p == 1, min_p == 0 is the default draw (sample_wave_u's bits: every class kept, the fall-back pick Q - 1)
__device__ __forceinline__ int sample_wave_wide(int o_lg, int Q, float u, float invT, int k, float top_p, float min_p, int lane) {
    const int per = Q >> 6;
    float* w = SM + o_lg + lane * per;
    const int rot = (lane * per) >> 6;
    float m = -INFINITY;
    for (int j = 0; j < per; ++j) m = fmaxf(m, w[wide_rot(j, rot, per)]);
    m = fmaxf(m, dpp_f<0xB1>(m)); m = fmaxf(m, dpp_f<0x4E>(m)); m = fmaxf(m, dpp_f<0x124>(m)); m = fmaxf(m, dpp_f<0x128>(m));
    m = fmaxf(fmaxf(rl_f(m, 0), rl_f(m, 16)), fmaxf(rl_f(m, 32), rl_f(m, 48)));
    unsigned thr = 0u;              // K = { key >= thr }: key 0 keeps every class
    if (k > 0 && k < Q) {
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = thr | (1u << bit);
            int cnt = 0;
            for (int j = 0; j < per; ++j) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(sample_key(w[wide_rot(j, rot, per)]) >= cand));
            if (cnt >= k) thr = cand;
            if (cnt == k) break;
        }
    }
    for (int j = 0; j < per; ++j) {     // logits -> weights, with the min_p cut (min_p == 0 cuts nothing: every weight is >= 0)
        const int s = wide_rot(j, rot, per);
        const float l = w[s];
        float e = sample_key(l) >= thr ? qexp((l - m) * invT) : 0.0f;
        e = e >= min_p ? e : 0.0f;
        w[s] = e;
    }
    if (top_p < 1.0f) {             // nucleus_cut's search, the weights read from LDS
        const float target = top_p * wide_mass(w, per, 0u);
        unsigned pthr = 0u;
        int c_thr = wide_count(w, per, rot, 1u), c_rej = 0;
        for (int bit = 30; bit >= 0 && c_thr - c_rej > 1; --bit) {
            const unsigned cand = pthr | (1u << bit);
            const int cnt = wide_count(w, per, rot, cand);
            const bool stays = cnt == c_thr || (cnt != c_rej && wide_mass(w, per, cand) >= target);
            if (stays) { pthr = cand; c_thr = cnt; } else c_rej = cnt;
        }
        for (int j = 0; j < per; ++j) { const int s = wide_rot(j, rot, per); const float e = w[s]; if (__float_as_uint(e) < pthr) w[s] = 0.0f; }
    }
    float a = w[0];
    for (int j = 1; j < per; ++j) a = a + w[j];
    float v = a;
    { const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); if (lane >= 1) v = v + up; }
    for (int d = 2; d < 64; d <<= 1) { const float up = __shfl_up(v, d); if (lane >= d) v = v + up; }
    const float total = rl_f(v, 63);
    float c = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
    if (lane == 0) c = 0.0f;
    const float th = u * total;
    int idx = 0x7fffffff, hi = -1;      // first kept class past the threshold / highest kept class, of this lane
    for (int j = 0; j < per; ++j) {
        const float e = w[j];
        c = c + e;
        if (__float_as_uint(e) != 0u) { hi = lane * per + j; if (idx == 0x7fffffff && c > th) idx = lane * per + j; }
    }
#define QPN_IMIN(CTRL) { const int o_ = __builtin_amdgcn_update_dpp(0x7fffffff, idx, CTRL, 0xf, 0xf, false); idx = o_ < idx ? o_ : idx; }
    QPN_IMIN(0xB1) QPN_IMIN(0x4E) QPN_IMIN(0x124) QPN_IMIN(0x128)
#undef QPN_IMIN
    {
        const int i0 = __builtin_amdgcn_readlane(idx, 0), i1 = __builtin_amdgcn_readlane(idx, 16), i2 = __builtin_amdgcn_readlane(idx, 32), i3 = __builtin_amdgcn_readlane(idx, 48);
        const int a01 = i0 < i1 ? i0 : i1, a23 = i2 < i3 ? i2 : i3;
        idx = a01 < a23 ? a01 : a23;
    }
    if (idx != 0x7fffffff) return idx;
    const unsigned long long any = __builtin_amdgcn_ballot_w64(hi >= 0);
    return any ? __builtin_amdgcn_readlane(hi, 63 - __builtin_clzll(any)) : Q - 1;
}
struct UttView {            // per-utterance pointers derived from kernel-argument bases (global address space)
    const float* pproj; const void* dfac; const int* known; const int64_t* teacher; int64_t* out; float* logits; float* ring;
    int n_pad, n0, n_samples, d_is_f32, row;
    RowDraw rd;             // the row's sampling record (qpn_decode_row_sampling), wave-uniform: filled by make_row_view only (the pipelined kernel), zeros otherwise
};
__device__ __forceinline__ UttView make_view(const DecodeParams& p, const UttDesc& d) {
    UttView u;
    u.pproj = p.pproj + d.pproj;
    u.dfac = d.d_is_f32 ? (const void*)((const float*)p.dfac + d.dfac) : (const void*)((const double*)p.dfac + d.dfac);
    u.known = p.known + d.known;
    u.teacher = d.teacher >= 0 ? p.teacher + d.teacher : nullptr;
    u.out = p.out + d.out;
    u.logits = d.logits >= 0 ? p.logits + d.logits : nullptr;
    u.ring = p.ring + d.ring;
    u.n_pad = d.n_pad; u.n0 = d.n0; u.n_samples = d.n_samples; u.d_is_f32 = d.d_is_f32; u.row = d.row;
    u.rd = RowDraw{};
    return u;
}
// ... and the view of the pipelined kernel's per-row instantiations (k_decode_pipe_r, decode_pipe.hip): with the row's record, one 32-byte load of the table behind
// p.row_draw when the group takes the utterance.  Their picks read the record from the view's registers: nothing is fetched per step
__device__ __forceinline__ UttView make_row_view(const DecodeParams& p, const UttDesc& d) {
    UttView u = make_view(p, d);
    if (p.row_draw) u.rd = p.row_draw[d.row];
    return u;
}
__device__ __forceinline__ unsigned long long row_seed(const RowDraw& r) { return (unsigned long long)r.seed_lo | ((unsigned long long)r.seed_hi << 32); }
// The kernels whose pick chooses its draw at run time (the one-CU kernels, decode_coop.hip, decode_coopb.hip) keep a row's record in LDS instead: eight words at SMI[o_rd],
// copied ONCE when the workgroup takes the row (the caller passes a barrier before its first pick) and read back by the picks of the ROW instantiations (sample_pick).  Held in
// registers for the whole launch, the seven values pushed the one-CU kernels' spilled scalars into scratch memory.
__device__ __forceinline__ void stage_row_draw(const DecodeParams& p, int row, int o_rd, int tid) {
    if (p.row_draw && tid < 8) SMI[o_rd + tid] = ((const int*)(p.row_draw + row))[tid];
}
// a record read from LDS (every lane reads the same words): back into scalar registers, so that the draw's loop bounds and compares stay wave-uniform
__device__ __forceinline__ RowDraw row_draw_lds(int o_rd) {
    const int* r = SMI + o_rd;
    RowDraw o;
    o.seed_lo = (unsigned)__builtin_amdgcn_readfirstlane(r[0]); o.seed_hi = (unsigned)__builtin_amdgcn_readfirstlane(r[1]); o.stream = (unsigned)__builtin_amdgcn_readfirstlane(r[2]);
    o.inv_temp = __int_as_float(__builtin_amdgcn_readfirstlane(r[3])); o.top_k = __builtin_amdgcn_readfirstlane(r[4]);
    o.top_p = __int_as_float(__builtin_amdgcn_readfirstlane(r[5])); o.min_p = __int_as_float(__builtin_amdgcn_readfirstlane(r[6]));
    o.pad_ = 0;
    return o;
}
// what the decode kernels' picks call when p.mode is not QPN_MODE_ARGMAX.  The host folds "a control is set" into the mode word the picks test anyway
// (QPN_MODE_SAMPLING_CTL, qpn_common.h): one wave-uniform compare of a kernel argument selects the draw, a default call runs sample_wave / sample_wave_u
// untouched, and the controls themselves (DecodeParams.inv_temp / top_k, kernel arguments too: a captured launch replays them) are read on the
// controlled path only (top_p / min_p of qpn_decode_sampling_ex as well).
// ROW: the kernels of the calls with per-row records (qpn_decode_row_sampling; p.mode == QPN_MODE_SAMPLING_ROW, which the launchers turn into the choice of the
// kernel: k_decode_r, k_decode_fast_r, k_decode_coop_r, k_decode_coopb_r): the same controlled draw with its key, its counter word and its four values taken from
// the row's record at SMI[o_rd] instead of DecodeParams and the batch row.  Kernels of their own, as k_decode_pipe_c is: compiled into the kernels of every call
// behind one more compare, the second draw cost calls WITHOUT records 1.8 % of the batched cooperative kernel's step time (repo-default model at B = 20) and, merged
// into one call behind selects, the one-CU kernels 68 bytes of scratch per lane.  Each kernel body is a file that its .hip includes twice (decode_*_kernel.h): with
// ROW = false the source is what it was, and the compiled kernels have the instruction counts, scratch sizes and register figures they had.
//
// ROW == 2: the kernels of the calls with a draw track (qpn_decode_frame_sampling; p.mode == QPN_MODE_SAMPLING_TRACK: k_decode_t, k_decode_fast_t, k_decode_coop_t, k_decode_coopb_t),
// the third inclusion of the same bodies.  Key and counter word come from the row's record as above; the four values are those of the feature frame the step reads,
//     f(i) = min(F - 1, (n_x - 1 + i) / U)        (U == 0: min(F - 1, n_x - 1 + i); the un-padded time aux_time() returns for generation step i, reference qpnet.py:450-451).
// A row's block at SMI[o_rd] is 16 words here: the RowDraw, then two frame records, of the even and of the odd generation steps.  The record's address depends on i only, so
// it is fetched where the kernel stages step i's aux features -- in the one-CU kernels that is during the pick of step i - 1, hence the two slots -- by four lanes, one word
// each, and a workgroup barrier lies between that store and the pick that reads it: the load is never on the pick's dependent chain.
__device__ __forceinline__ const int* frame_draw_record(const DecodeParams& p, int row, int ut) {      // ut: the un-padded time of a generation step (>= 0)
    int64_t f = p.U > 0 ? (int64_t)((unsigned)ut / (unsigned)p.U) : (int64_t)ut;
    f = f < p.n_frames - 1 ? f : p.n_frames - 1;
    return (const int*)(p.frame_draw + ((size_t)row * (size_t)p.n_frames + (size_t)(f > 0 ? f : 0)));
}
// step t's record, one word in each of the lanes that call with word = 0..3 (0 elsewhere, and for the steps of the warm-up, which draw nothing)
__device__ __forceinline__ int frame_draw_load(const DecodeParams& p, const UttView& u, int t, int word) {
    const int i = t - (u.n0 - 1);
    return (i >= 0 && word < 4) ? frame_draw_record(p, u.row, t - u.n_pad)[word] : 0;
}
__device__ __forceinline__ void frame_draw_store(const UttView& u, int t, int o_rd, int word, int v) {
    const int i = t - (u.n0 - 1);
    if (i >= 0 && word < 4) SMI[o_rd + 8 + 4 * (i & 1) + word] = v;
}
__device__ __forceinline__ void stage_frame_draw(const DecodeParams& p, const UttView& u, int t, int o_rd, int word) {
    frame_draw_store(u, t, o_rd, word, frame_draw_load(p, u, t, word));
}
// the frame record of generation step `step` read from LDS (every lane reads the same words): back into scalar registers, as row_draw_lds does
__device__ __forceinline__ FrameDraw frame_draw_lds(int o_rd, unsigned step) {
    const int* r = SMI + o_rd + 8 + 4 * (int)(step & 1u);
    FrameDraw o;
    o.inv_temp = __int_as_float(__builtin_amdgcn_readfirstlane(r[0])); o.top_k = __builtin_amdgcn_readfirstlane(r[1]);
    o.top_p = __int_as_float(__builtin_amdgcn_readfirstlane(r[2])); o.min_p = __int_as_float(__builtin_amdgcn_readfirstlane(r[3]));
    return o;
}
// WIDE: the kernels of the sampled calls at Q > 256 (k_decode_w*, k_decode_coop_w*, k_decode_coopb_w*: the same bodies included three more times).  The launchers test
// Q > 256 once, on the host, where they choose the kernel; those kernels' picks run sample_wave_wide and nothing else.  Kernels of their own for the reason given above for
// ROW: behind one more compare inside the existing kernels, even the LDS-walking draw cost them scratch memory (the interpreter 24 -> 76 bytes per lane, the batched
// cooperative kernel 12 -> 28) and the per-utterance cooperative kernel six registers; with WIDE = false the source is what it was.  A call that set no control
// carries the values that switch every control off (1.0f, 0, 1.0f, 0.0f), so the wide kernels read them whatever the mode.
template <int ROW, bool WIDE = false>
__device__ __forceinline__ int sample_pick(const DecodeParams& p, unsigned row, int o_rd, int o_lg, int Q, unsigned step, int lane) {
    if constexpr (WIDE) {
        if constexpr (ROW == 2) {
            const RowDraw r = row_draw_lds(o_rd);
            const FrameDraw d = frame_draw_lds(o_rd, step);
            return sample_wave_wide(o_lg, Q, sample_uniform(row_seed(r), r.stream, step), d.inv_temp, d.top_k, d.top_p, d.min_p, lane);
        } else if constexpr (ROW == 1) {
            const RowDraw r = row_draw_lds(o_rd);
            return sample_wave_wide(o_lg, Q, sample_uniform(row_seed(r), r.stream, step), r.inv_temp, r.top_k, r.top_p, r.min_p, lane);
        } else {
            return sample_wave_wide(o_lg, Q, sample_uniform(p.seed, row, step), p.inv_temp, p.top_k, p.top_p, p.min_p, lane);
        }
    } else if constexpr (ROW == 2) {
        const RowDraw r = row_draw_lds(o_rd);
        const FrameDraw d = frame_draw_lds(o_rd, step);
        return sample_wave_ctl<true>(o_lg, Q, sample_uniform(row_seed(r), r.stream, step), d.inv_temp, d.top_k, d.top_p, d.min_p, lane);
    } else if constexpr (ROW == 1) {
        const RowDraw r = row_draw_lds(o_rd);
        return sample_wave_ctl<true>(o_lg, Q, sample_uniform(row_seed(r), r.stream, step), r.inv_temp, r.top_k, r.top_p, r.min_p, lane);
    } else {
        if (p.mode == QPN_MODE_SAMPLING) return sample_wave(o_lg, Q, p.seed, row, step, lane);
        return sample_wave_ctl<true>(o_lg, Q, sample_uniform(p.seed, row, step), p.inv_temp, p.top_k, p.top_p, p.min_p, lane);
    }
}

// Live output: the lane that has just stored sample i of its row (bi) mirrors it into host memory and, every live_every samples and after the
// row's last one, publishes the row's count.  The mirror stores are system-scope (write-through) and the count is a system-scope release
// store, which waits for them: a host that reads the count with an acquire load finds every sample below it in the mirror.  Rows of one
// launch, of several launches and of one group all publish under their own row index, so the plan does not matter.  Not armed (live ==
// nullptr, a kernel argument): one wave-uniform branch.
// gave_up: the abort flag of a multi-workgroup launch.  A wait that ran out raises it and lets its step finish on whatever it holds, so the
// pick of that step may be wrong; nothing is published once the flag is seen up.  The host then finds the launch ended short of the row's
// length, and the re-run (qpn_decode_finish) produces the rest.  Where the wait that ran out is the picking workgroup's own, the flag is up
// before the pick in program order.  Where it is a peer's or an upstream role's, this rests on timing, not on the memory model: the flag store
// and the later stores that carry the step's values on are relaxed stores to different addresses, and the flag store leads them by the rest
// of that stage's work and every hand-off between there and the pick (microseconds).
//
// Cancel (qpn_decode_cancel): p.cancel is one word of the same kind of memory that the host sets; armed launches only (null together with
// p.live).  The lane that publishes reads it with a system-scope load, a round trip to host memory, so the load is issued at one publish
// point, right behind the count's store, and its value is looked at at the next one: nothing in the step waits for it.  `creq` is that
// lane's state between publish points: the word as the last publish point's load found it (0 at the start; the host sets 1), or -1 once the
// stop has been handed on.  Returns true once, at the publish point that finds the word set, AFTER that point's count has been stored: the
// caller then stops the row -- a multi-workgroup launch by raising its abort flag (every peer drains as after a timeout), a one-CU workgroup
// through its LDS stop word.  From then on this lane publishes nothing (creq < 0), so the count stored here is the row's last; steps that drain may still store picks
// behind it.  A row's first look at the word, at its start, is cancel_requested(): a launch that starts after the request publishes nothing.
__device__ __forceinline__ bool cancel_requested(const DecodeParams& p) {
    return p.cancel && __hip_atomic_load(p.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}
__device__ __forceinline__ bool live_put(const DecodeParams& p, const UttView& u, int i, int bi, int& creq, const int* gave_up = nullptr) {
    if (!p.live) return false;
    __hip_atomic_store(p.live + (u.out - p.out) + i, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((unsigned)(i + 1) % (unsigned)p.live_every == 0u || i + 1 == u.n_samples) {
        if (gave_up && __hip_atomic_load(gave_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
        if (creq < 0) return false;
        __hip_atomic_store(p.live_done + u.row, (long long)(i + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (creq != 0) { creq = -1; return true; }
        creq = __hip_atomic_load(p.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (the raw word: any use of it here would wait for it here)
    }
    return false;
}

// pitch-dependent tap distance of ring `r` at (padded) time t  (qpnet.py:613-624)
// `widx` != 0: warm-up step over the known prefix -- the reference takes those taps from _dilated_index (qpnet.py:416,
// 592-611: rint(-d*dil + idx), idx = position from the end of the prefix), not from _generate_dilated_index
__device__ __forceinline__ int tap_offset(const RingDesc& r, const UttView& u, int ut, int widx) {
    if (!r.adaptive) return r.mult;
    if (ut < 0) return r.mult;                       // d := 1.0 in the left padding (qpnet.py:361-364)
    if (u.d_is_f32) {
        float d = ((const float*)u.dfac)[ut];
        if (widx) return widx - (int)rintf(__fadd_rn(-d * (float)r.mult, (float)widx));
        return -(int)rintf(-d * (float)r.mult);
    }
    double d = ((const double*)u.dfac)[ut];
    if (widx) return widx - (int)rint(__dadd_rn(-d * (double)r.mult, (double)widx));
    return -(int)rint(-d * (double)r.mult);
}
// un-padded time whose aux features / dilated factor step t uses: the newest sample's own in the generation loop
// (qpnet.py:450-452); one EARLIER during the warm-up over the known prefix, where the reference pairs layer output p with
// h[p-1], d[p-1] (h_ = h[:, :, :causal_output.size(-1)], qpnet.py:366-368; visible only with seeds of >= 3 samples)
__device__ __forceinline__ int aux_time(const UttView& u, int t) { return t - u.n_pad - (t < u.n0 - 1 ? 1 : 0); }
