// score.hip -- teacher-forced scoring of given logits: per row the negative log likelihood of the target, the entropy of the distribution,
// the argmax and the target's rank (qpn_score_logits; reference src/bin/qpnet_validate.py:409-437 keeps only the mean of the first).
//
// One wave per row, four waves per workgroup, SC_RPW rows per wave (the row-to-wave map of k_ce_hard, train_loss.hip).  A row of up to 1024 classes is read
// from global memory ONCE into registers; larger rows are read twice.  The log-sum-exp is k_ce_hard's arithmetic for that Q, operation for operation: the
// lane that owns a class, the order in which a lane adds its terms, tr_wave_max / tr_wave_sum, logf(se) + m -- so the float64 sum of a chunk's nll
// over its row count is the loss qpn_ce_loss reports.  That fixes which lane holds which class:
//   Q % 256 == 0: lane owns classes 4 lane + 256 p .. + 3 of pass p (one float4 per pass), __expf, terms added as (e0 + e1) + (e2 + e3) per pass
//   otherwise:    lane owns classes lane + 64 j (one dword per slot, 256 contiguous bytes per wave instruction), expf, terms added in slot order
#include "train_common.h"
#include <type_traits>

#define SC_RPW 4              // rows per wave (16 rows per workgroup, as k_ce_hard)
#define SC_IDX_NONE 65536     // above every class index (Q <= 65536)
#define SC_FLT_MAX 3.402823466e38f

static_assert(sizeof(qpn_score_row) == 16, "one 16-byte record per row");

// the record of one row (lane 0 stores): m, lt, idx, cnt are wave-uniform; se and s2 the lanes' partial sums
__device__ __forceinline__ void score_store(qpn_score_row* __restrict__ out, int64_t row, int lane, float m, float se, float s2, int idx, int cnt, float lt, bool in_range, int Q) {
    se = tr_wave_sum(se);
    s2 = tr_wave_sum(s2);
    const float lg_se = logf(se);
    const float lse = lg_se + m;                                          // k_ce_hard: logf(se) + m
    qpn_score_row r;
    r.nll = in_range ? lse - lt : INFINITY;
    r.entropy = lg_se + s2 / se;                                          // -sum p log p = log se + sum (e / se)(m - l): every term >= 0
    r.argmax = idx;
    r.rank = in_range ? cnt : Q;
    if (lane == 0) *(int4*)(out + row) = *(const int4*)&r;
}
// e (m - l) with x = l - m <= 0: 0 for e == 0 also where x is -inf (0 * inf otherwise)
__device__ __forceinline__ float score_term(float e, float x) { return e * fminf(-x, SC_FLT_MAX); }
// What needs no arithmetic on the values leaves the vector unit: a comparison of one class slot over the wave is ONE v_cmp into a scalar mask, and
//   argmax = the lowest class whose logit equals the row's maximum: lowest set lane of the slot's mask -> class, minimum over the slots (lowest index among the maxima)
//   rank   = the population count of (logit > l[t]) over the slots
// are scalar instructions on those masks (no per-lane index tracking, no wave reduction of an index or a count).
__device__ __forceinline__ int score_first(unsigned long long mask, int per_lane, int base, int cur) {      // class of the lowest set lane: base + per_lane * lane
    const int c = mask ? base + per_lane * (int)__builtin_ctzll(mask) : SC_IDX_NONE;
    return c < cur ? c : cur;
}

// one row held in registers, vector form (Q == 256 NP): v[p] = classes 4 lane + 256 p .. + 3
template <int NP>
__device__ __forceinline__ void score_row_vec(const float4 (&v)[NP], qpn_score_row* __restrict__ out, int64_t row, int lane, float lt, bool in_range, int Q) {
    float best = -INFINITY;
#pragma unroll
    for (int p = 0; p < NP; ++p) best = fmaxf(fmaxf(best, fmaxf(v[p].x, v[p].y)), fmaxf(v[p].z, v[p].w));
    const float m = tr_wave_max(best);
    float se = 0.f, s2 = 0.f;
    int idx = SC_IDX_NONE, cnt = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float x0 = v[p].x - m, x1 = v[p].y - m, x2 = v[p].z - m, x3 = v[p].w - m;
        const float e0 = __expf(x0), e1 = __expf(x1), e2 = __expf(x2), e3 = __expf(x3);
        se += (e0 + e1) + (e2 + e3);
        s2 += (score_term(e0, x0) + score_term(e1, x1)) + (score_term(e2, x2) + score_term(e3, x3));
        idx = score_first(__ballot(v[p].x == m), 4, 256 * p, idx); idx = score_first(__ballot(v[p].y == m), 4, 256 * p + 1, idx);
        idx = score_first(__ballot(v[p].z == m), 4, 256 * p + 2, idx); idx = score_first(__ballot(v[p].w == m), 4, 256 * p + 3, idx);
        cnt += __builtin_popcountll(__ballot(v[p].x > lt)) + __builtin_popcountll(__ballot(v[p].y > lt)) +
               __builtin_popcountll(__ballot(v[p].z > lt)) + __builtin_popcountll(__ballot(v[p].w > lt));
    }
    score_store(out, row, lane, m, se, s2, idx, cnt, lt, in_range, Q);
}
// ... lane-strided form (Q <= 256 NP): v[j] = class lane + 64 j, -inf past Q (adds an exact 0 to the sums, never above a target, equal to the maximum in no specified row)
template <int NP>
__device__ __forceinline__ void score_row_str(const float (&v)[4 * NP], qpn_score_row* __restrict__ out, int64_t row, int lane, float lt, bool in_range, int Q) {
    float best = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4 * NP; ++j) best = fmaxf(best, v[j]);
    const float m = tr_wave_max(best);
    float se = 0.f, s2 = 0.f;
    int idx = SC_IDX_NONE, cnt = 0;
#pragma unroll
    for (int j = 0; j < 4 * NP; ++j) {
        const float x = v[j] - m;
        const float e = lane + 64 * j < Q ? expf(x) : 0.f;
        se += e;
        s2 += score_term(e, x);
        idx = score_first(__ballot(v[j] == m), 1, 64 * j, idx);
        cnt += __builtin_popcountll(__ballot(v[j] > lt));
    }
    score_store(out, row, lane, m, se, s2, idx, cnt, lt, in_range, Q);
}

// VEC: Q == 256 NP.  !VEC: Q <= 256 NP.  NP == 0: any Q, the row is re-read.
// The register forms request the logits and targets of ALL the wave's rows before they reduce the first one (one basic block, the rows past the end clamped to the last
// row and not stored): with a row after the other, a wave paid a memory round trip per row in sequence, and the five waves a SIMD holds did not cover it.
template <int NP, bool VEC>
__global__ __launch_bounds__(256) void k_score(const float* __restrict__ logits, const int64_t* __restrict__ tgt, int64_t tgt_stride, int BL, int Q, int64_t rows,
                                               qpn_score_row* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform: rows, targets and their addresses stay in scalar registers)
    if constexpr (NP > 0) {
        const int64_t first = (int64_t)blockIdx.x * SC_RPW * 4 + wave;   // the wave's rows: first + 4 it (k_ce_hard's map)
        if (first >= rows) return;
        typename std::conditional<VEC, float4, float>::type v[SC_RPW][VEC ? NP : 4 * NP];
        int64_t tg[SC_RPW]; float lt[SC_RPW];
#pragma unroll
        for (int it = 0; it < SC_RPW; ++it) {
            const int64_t row = first + 4 * it < rows ? first + 4 * it : rows - 1;
            const float* lg = logits + (size_t)row * Q;
            const unsigned b = (unsigned)row / (unsigned)BL, t = (unsigned)row - b * (unsigned)BL;      // (rows < 2^31, checked by the host: a 64-bit division is ~150 instructions in front of every load)
            tg[it] = tgt[(size_t)b * tgt_stride + (tgt_stride - BL) + t];
            if constexpr (VEC) {
#pragma unroll
                for (int p = 0; p < NP; ++p) v[it][p] = *(const float4*)(lg + 4 * lane + 256 * p);
            } else {
#pragma unroll
                for (int j = 0; j < 4 * NP; ++j) { const int q = lane + 64 * j; v[it][j] = q < Q ? lg[q] : -INFINITY; }
            }
        }
#pragma unroll
        for (int it = 0; it < SC_RPW; ++it) {
            const int64_t row = first + 4 * it < rows ? first + 4 * it : rows - 1;
            lt[it] = tg[it] >= 0 && tg[it] < Q ? logits[(size_t)row * Q + tg[it]] : INFINITY;      // (out of range: nothing is above +inf; the record gets rank = Q, nll = +inf)
        }
#pragma unroll
        for (int it = 0; it < SC_RPW; ++it) {
            const int64_t row = first + 4 * it;
            if (row < rows) {
                const bool in_range = tg[it] >= 0 && tg[it] < Q;
                if constexpr (VEC) score_row_vec<NP>(v[it], out, row, lane, lt[it], in_range, Q);
                else score_row_str<NP>(v[it], out, row, lane, lt[it], in_range, Q);
            }
        }
    } else {
        for (int it = 0; it < SC_RPW; ++it) {
            const int64_t row = ((int64_t)blockIdx.x * SC_RPW + it) * 4 + wave;
            if (row >= rows) break;
            const float* lg = logits + (size_t)row * Q;
            const int64_t b = row / BL, t = row - b * BL;
            const int64_t tg = tgt[(size_t)b * tgt_stride + (tgt_stride - BL) + t];
            const bool in_range = tg >= 0 && tg < Q;
            const float lt = in_range ? lg[tg] : INFINITY;
            const bool vec = (Q & 255) == 0;
            float best = -INFINITY, bidx = (float)SC_IDX_NONE;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 x = *(const float4*)(lg + q);
                if (x.x > best) { best = x.x; bidx = (float)q; }
                if (x.y > best) { best = x.y; bidx = (float)(q + 1); }
                if (x.z > best) { best = x.z; bidx = (float)(q + 2); }
                if (x.w > best) { best = x.w; bidx = (float)(q + 3); }
            } else for (int q = lane; q < Q; q += 64) { const float x = lg[q]; if (x > best) { best = x; bidx = (float)q; } }
            const float m = tr_wave_max(best);
            float se = 0.f, s2 = 0.f, cnt = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 x = *(const float4*)(lg + q);
                const float e0 = __expf(x.x - m), e1 = __expf(x.y - m), e2 = __expf(x.z - m), e3 = __expf(x.w - m);
                se += (e0 + e1) + (e2 + e3);
                s2 += ((e0 > 0.f ? e0 * (m - x.x) : 0.f) + (e1 > 0.f ? e1 * (m - x.y) : 0.f)) + ((e2 > 0.f ? e2 * (m - x.z) : 0.f) + (e3 > 0.f ? e3 * (m - x.w) : 0.f));
                cnt += (float)((x.x > lt ? 1 : 0) + (x.y > lt ? 1 : 0) + (x.z > lt ? 1 : 0) + (x.w > lt ? 1 : 0));
            } else for (int q = lane; q < Q; q += 64) {
                const float x = lg[q];
                const float e = expf(x - m);
                se += e;
                s2 += e > 0.f ? e * (m - x) : 0.f;
                cnt += x > lt ? 1.f : 0.f;
            }
            const int idx = (int)-tr_wave_max(best == m ? -bidx : -(float)SC_IDX_NONE);      // (indices and counts below 2^24: exact as floats)
            score_store(out, row, lane, m, se, s2, idx, (int)tr_wave_sum(cnt), lt, in_range, Q);
        }
    }
}

static int score_dev_ok() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    return QPN_OK;
}

extern "C" int qpn_score_logits(const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL, int Q, qpn_score_row* d_out, void* stream_) {
    if (!d_logits) { qpn_set_error("d_logits is NULL"); return QPN_EINVAL; }
    if (!d_targets) { qpn_set_error("d_targets is NULL"); return QPN_EINVAL; }
    if (!d_out) { qpn_set_error("d_out is NULL"); return QPN_EINVAL; }
    if (B < 1) { qpn_set_error("B must be >= 1 (got %d)", B); return QPN_EINVAL; }
    if (BL < 1) { qpn_set_error("BL must be >= 1 (got %d)", BL); return QPN_EINVAL; }
    if (Q < 1 || Q > 65536) { qpn_set_error("Q must lie in 1..65536 (got %d)", Q); return QPN_EINVAL; }
    if (tgt_stride < BL) { qpn_set_error("tgt_stride must be >= BL = %d (got %lld)", BL, (long long)tgt_stride); return QPN_EINVAL; }
    const int64_t rows = (int64_t)B * BL;
    if (rows >= ((int64_t)1 << 31)) { qpn_set_error("B * BL must be below 2^31 (got %lld)", (long long)rows); return QPN_EINVAL; }
    int rc = score_dev_ok(); if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)((rows + 4 * SC_RPW - 1) / (4 * SC_RPW))), block(256);
    const bool vec = Q % 256 == 0;
    const int np = Q > 1024 ? 0 : (Q + 255) / 256;
#define SC_LAUNCH(NP, VEC) hipLaunchKernelGGL((k_score<NP, VEC>), grid, block, 0, stream, d_logits, d_targets, tgt_stride, BL, Q, rows, d_out)
    switch (np) {
        case 1: if (vec) SC_LAUNCH(1, true); else SC_LAUNCH(1, false); break;
        case 2: if (vec) SC_LAUNCH(2, true); else SC_LAUNCH(2, false); break;
        case 3: if (vec) SC_LAUNCH(3, true); else SC_LAUNCH(3, false); break;
        case 4: if (vec) SC_LAUNCH(4, true); else SC_LAUNCH(4, false); break;
        default: SC_LAUNCH(0, false); break;
    }
#undef SC_LAUNCH
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
