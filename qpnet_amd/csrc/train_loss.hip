// train_loss.hip -- the stand-alone loss kernels of the training step on gfx950 (MI355X) and their one launcher:
//   k_ce_hard<NV, W> : mean cross entropy + its gradient (reference qpnet_train.py:430,526-528); W: with the loss options
//   k_ce_soft<NV, W> : the soft-target (distillation) loss + its gradient; W: with row weights and ignore_index
//   k_weight_mass    : the effective sum of weights that norm = "weights" divides by
//   qpn_launch_loss  : what qpn_ce_loss / qpn_distill_loss / their _opts forms and a forward-with-loss whose cross entropy is not fused launch
// (the default fused step keeps its cross entropy inside the post-net tile: train_post.h)
// Both kernel families share one layout: one wave per row, rpw rows per wave, 16 rows per workgroup, 64 double loss slots.
//   NV > 0: Q == 256 NV.  The lane's 4 NV values of a row are loaded with 16-byte loads, all in flight before the first reduction, and stay in registers:
//           a row is read once.  NV == 0: any Q, loops -- four classes per lane and pass when Q % 256 == 0, one otherwise.
//   W false: no weight fetch, no zero-row skip, no mass; the CeOpts argument is taken and discarded.
// The !W and W instances are kernels of their own (a kernel template is compiled as directly as included text: MEASUREMENTS.md, "Loss options").
#include "train_common.h"
#include <type_traits>

// ---- loss options ("Loss options"): row weights, ignore_index, label smoothing, the normaliser.  Per row r with logits z, target y:
//   w_r = weights[r] (1 without weights), 0 when y == ignore_index;   CE_r = lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q;
//   L = (1 / N) sum_r w_r CE_r,   dL/dz_r = (w_r / N) (softmax(z) - (1 - eps) onehot(y) - eps / Q),   N = the row count, or the effective sum of weights.
// The helpers below are shared by k_ce_hard, k_weight_mass and k_ce_soft, so that all three agree on a row's weight.
// A NaN, infinite or negative weight sets status value 64 (the Adam launch of the step skips: the sticky-status rule) and counts as 0.
__device__ __forceinline__ float ce_weight_value(const CeOpts& o, int64_t row, int64_t tg, bool& bad) {
    float w = 1.0f;
    bad = false;
    if (o.w) { w = o.w[row]; if (!(w >= 0.f && w <= 3.402823466e+38f)) { bad = true; w = 0.f; } }
    if (o.use_ign && tg == (int64_t)o.ign) w = 0.f;
    return w;
}
__device__ __forceinline__ float ce_row_weight(const CeOpts& o, int64_t row, int64_t tg, int lane, int* status) {
    bool bad;
    const float w = ce_weight_value(o, row, tg, bad);
    if (bad && lane == 0) atomicOr(status, 64);
    return w;
}
// the normaliser N as a double (1 where the effective mass is 0: every sum it divides is 0 then) and 1 / N as the fp32 factor of the gradient (0 there)
template <bool W> __device__ __forceinline__ double ce_opt_den(const CeOpts& o, int64_t rows) {
    if constexpr (W) { if (o.norm_mass) { const double m = *o.norm_mass; return m > 0.0 ? m : 1.0; } }
    return (double)rows;
}
template <bool W> __device__ __forceinline__ float ce_opt_inv(const CeOpts& o, int64_t rows) {
    if constexpr (W) { if (o.norm_mass) { const double m = *o.norm_mass; return m > 0.0 ? (float)(1.0 / m) : 0.f; } }
    return 1.0f / (float)rows;
}
// a zero-weight row of dL/dlogits: exact +0, by the lanes that would have written the row's gradient
template <int NV> __device__ __forceinline__ void ce_zero_row(float* __restrict__ dst, int Q, int lane) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) *(float4*)(dst + lane * 4 + 256 * k) = z4;
    } else if ((Q & 255) == 0) { for (int q = lane * 4; q < Q; q += 256) *(float4*)(dst + q) = z4; }
    else for (int q = lane; q < Q; q += 64) dst[q] = 0.f;
}

// ---- what the hard and the soft kernels, and their register and loop forms, do alike: values in, a scalar out; operand order and parentheses are part of
//      the contract (the outputs are specified bit for bit).  These are the helpers that leave every instance's instructions as they were; the target's range
//      check, the gradient float4 and anything else that returns a float4 did not (MEASUREMENTS.md, "Loss options") and stay written out in the kernels.
// the target of a row: the last BL entries of its batch item's tgt_stride
__device__ __forceinline__ int64_t ce_target(const int64_t* __restrict__ tgt, int64_t tgt_stride, int BL, int64_t row) {
    const int64_t b = row / BL, t = row - b * BL;
    return tgt[(size_t)b * tgt_stride + (tgt_stride - BL) + t];
}
__device__ __forceinline__ float ce_max4(float m, float4 v) { return fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float ce_sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ce_expsum4(float4 v, float m) { return (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m)); }
// the four waves' partial sums of a workgroup, in wave order
__device__ __forceinline__ double ce_part_sum(const double (&p)[4]) { return p[0] + p[1] + p[2] + p[3]; }

// The effective sum of weights for norm = "weights", in fp64 and in a FIXED order (one workgroup: strided partial sums, an LDS tree): the same bits from run to
// run.  Written to the word k_ce_hard / k_ce_soft read (CeOpts::norm_mass); enqueued in front of them on the same stream.
__global__ __launch_bounds__(1024) void k_weight_mass(const int64_t* __restrict__ tgt, int64_t tgt_stride, int BL, int64_t rows, CeOpts o, double* __restrict__ out) {
    __shared__ double s[1024];
    double a = 0.0;
    // a thread's rows are threadIdx.x + 1024 j, added in the order of j; eight of them are loaded before the first is added (one workgroup: the loop lives on loads in flight)
    for (int64_t base = threadIdx.x; base < rows; base += 8 * 1024) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t row = base + 1024 * j;
            v[j] = 0.f;
            if (row < rows) {
                int64_t tg = 0;
                if (o.use_ign) { const int64_t b = row / BL, t = row - b * BL; tg = tgt[(size_t)b * tgt_stride + (tgt_stride - BL) + t]; }
                bool bad;
                v[j] = ce_weight_value(o, row, tg, bad);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (double)v[j];
    }
    s[threadIdx.x] = a;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// mean cross entropy + its gradient (reference qpnet_train.py:430,526-528).  <0, false> is the plain criterion, launched at every Q.
// W: the row's scale w_r / N is formed once, in fp32, and multiplies the gradient: with w_r == 1, eps == 0 and N the row count the output is the plain
// kernel's bits, with a power-of-two weight exactly that weight times them.  The row loss is formed in fp32 as the plain kernel forms it, widened and
// multiplied by (double)w_r.  A row of weight 0 is decided from the weight and the target BEFORE any load of its logits is issued: its logits are not read,
// its target is not range-checked, its dL/dlogits row is exact +0.  Smoothing (eps > 0, wave-uniform) adds one tr_wave_sum of z.
template <int NV, bool W>
__global__ __launch_bounds__(256) void k_ce_hard(const float* __restrict__ logits, const int64_t* __restrict__ tgt, int64_t tgt_stride, int BL, int Q, int64_t rows,
                                                 float* __restrict__ dlogits, double* __restrict__ loss, int rpw, int* __restrict__ status, CeOpts o) {
    __shared__ double part[W ? 2 : 1][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv = ce_opt_inv<W>(o, rows);
    const bool smooth = W && o.eps > 0.f;
    const float ome = W ? 1.0f - o.eps : 1.0f, eq = W ? o.eps / (float)Q : 0.f;
    double lsum = 0.0;
    [[maybe_unused]] double msum = 0.0;
    for (int it = 0; it < rpw; ++it) {
        const int64_t row = ((int64_t)blockIdx.x * rpw + it) * 4 + wave;
        if (row >= rows) break;
        const float* lg = logits + (size_t)row * Q;
        int64_t tg = ce_target(tgt, tgt_stride, BL, row);
        [[maybe_unused]] float wr = 1.0f;
        if constexpr (W) {          // the row's weight, from the weight and the target alone: a zero-weight row loads no logits
            wr = ce_row_weight(o, row, tg, lane, status);
            if (wr == 0.f) { if (dlogits) ce_zero_row<NV>(dlogits + (size_t)row * Q, Q, lane); continue; }
            msum += (double)wr;
        }
        const float sc = W ? wr * inv : inv;          // the row's scale, formed once
        float ce;
        if constexpr (NV > 0) {
            float4 z[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) z[k] = *(const float4*)(lg + lane * 4 + 256 * k);
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }     // reference: assert max(batch_t) < n_quantize
            const float ztg = lg[tg];
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < NV; ++k) m = ce_max4(m, z[k]);
            m = tr_wave_max(m);
            float se = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) se += ce_expsum4(z[k], m);
            se = tr_wave_sum(se);
            const float lse = logf(se) + m;
            if (dlogits) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int q = lane * 4 + 256 * k;
                    float4 g = make_float4(__expf(z[k].x - lse), __expf(z[k].y - lse), __expf(z[k].z - lse), __expf(z[k].w - lse));
                    const int dq = (int)tg - q;
                    if (dq == 0) g.x -= ome; else if (dq == 1) g.y -= ome; else if (dq == 2) g.z -= ome; else if (dq == 3) g.w -= ome;
                    if (smooth) { g.x -= eq; g.y -= eq; g.z -= eq; g.w -= eq; }
                    *(float4*)(dlogits + (size_t)row * Q + q) = make_float4(g.x * sc, g.y * sc, g.z * sc, g.w * sc);
                }
            }
            ce = lse - ztg;
            if (smooth) {
                float sz = 0.f;
#pragma unroll
                for (int k = 0; k < NV; ++k) sz += ce_sum4(z[k]);
                sz = tr_wave_sum(sz);
                ce = (lse - ome * ztg) - eq * sz;
            }
        } else {
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }
            float m = -INFINITY;
            const bool vec = (Q & 255) == 0;             // 4 contiguous logits per lane per pass (16-byte accesses)
            if (vec) for (int q = lane * 4; q < Q; q += 256) m = ce_max4(m, *(const float4*)(lg + q));
            else for (int q = lane; q < Q; q += 64) m = fmaxf(m, lg[q]);
            m = tr_wave_max(m);
            float se = 0.f, sz = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) { const float4 v = *(const float4*)(lg + q); se += ce_expsum4(v, m); sz += ce_sum4(v); }
            else for (int q = lane; q < Q; q += 64) { se += expf(lg[q] - m); sz += lg[q]; }
            se = tr_wave_sum(se);
            const float lse = logf(se) + m;
            if (dlogits) {
                if (vec) for (int q = lane * 4; q < Q; q += 256) {
                    const float4 v = *(const float4*)(lg + q);
                    float4 g = make_float4(__expf(v.x - lse), __expf(v.y - lse), __expf(v.z - lse), __expf(v.w - lse));
                    const int dq = (int)tg - q;
                    if (dq == 0) g.x -= ome; else if (dq == 1) g.y -= ome; else if (dq == 2) g.z -= ome; else if (dq == 3) g.w -= ome;
                    if (smooth) { g.x -= eq; g.y -= eq; g.z -= eq; g.w -= eq; }
                    *(float4*)(dlogits + (size_t)row * Q + q) = make_float4(g.x * sc, g.y * sc, g.z * sc, g.w * sc);
                } else for (int q = lane; q < Q; q += 64) {
                    float g = expf(lg[q] - lse) - (q == tg ? ome : 0.0f);
                    if (smooth) g -= eq;
                    dlogits[(size_t)row * Q + q] = g * sc;
                }
            }
            ce = lse - lg[tg];
            if (smooth) { sz = tr_wave_sum(sz); ce = (lse - ome * lg[tg]) - eq * sz; }
        }
        if constexpr (W) lsum += (double)ce * (double)wr; else lsum += (double)ce;
    }
    if (lane == 0) { part[0][wave] = lsum; if constexpr (W) part[1][wave] = msum; }
    __syncthreads();
    // 64 accumulator slots (summed by the reader): one double atomic per workgroup on ONE address serialises at the memory side
    if (threadIdx.x == 0) {
        atomicAdd(loss + (blockIdx.x & 63), ce_part_sum(part[0]) / ce_opt_den<W>(o, rows));
        if constexpr (W) if (o.mass) atomicAdd(o.mass + (blockIdx.x & 63), ce_part_sum(part[1]));
    }
}

// knowledge distillation ("Soft-target loss"): per row  L = (1 - alpha) CE(z, y) + alpha T^2 KL(softmax(t / T) || softmax(z / T))  and
//   dL/dz = (1 - alpha) (softmax(z) - onehot(y)) + alpha T (softmax(z / T) - softmax(t / T)),  both over the row count, z = logits, t = teacher.
// For the CE term, k_ce_hard's arithmetic operation for operation; the wave reductions are tr_wave_max / tr_wave_sum in its order, so dL/dlogits is the same
// bits from run to run.
//   NV > 0: the lane's 4 NV student and 4 NV teacher values stay in registers with their tempered exponentials: a row is read once (2 x 1 KB at Q = 256),
//           nothing lives in scratch.  NV == 0: the loops run over rows that are L2-hot after the first pass.
// KL is formed from log-probabilities ((t_i - m_t) / T - log S_t minus the student's counterpart): a teacher bitwise equal to the student gives exact zeros.
// A NaN or an infinity in a row's teacher logits sets status bit 5 (the Adam launch of the step skips: the sticky-status rule); that row's outputs are unspecified.
// comp (may be nullptr): 2 x 64 more slots -- the hard CE mean, then the KL mean BEFORE its factor T^2 -- for qpn_distill_loss's h_loss3.
// W: w_r multiplies the whole row loss, CE and KL term alike; the row's scale w_r / N is formed once.
__device__ __forceinline__ bool dk_bad(float v) { return !(fabsf(v) <= 3.402823466e+38f); }      // NaN or +-inf
template <int NV, bool W>
__global__ __launch_bounds__(256) void k_ce_soft(const float* __restrict__ logits, const float* __restrict__ teacher, const int64_t* __restrict__ tgt, int64_t tgt_stride,
                                                 int BL, int Q, int64_t rows, float alpha, float temp, float* __restrict__ dlogits, double* __restrict__ loss,
                                                 double* __restrict__ comp, int rpw, int* __restrict__ status, CeOpts o) {
    __shared__ double part[W ? 3 : 2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float invT = 1.0f / temp, oma = 1.0f - alpha, aT = alpha * temp;
    const float inv = ce_opt_inv<W>(o, rows);
    double csum = 0.0, ksum = 0.0;
    [[maybe_unused]] double msum = 0.0;
    for (int it = 0; it < rpw; ++it) {
        const int64_t row = ((int64_t)blockIdx.x * rpw + it) * 4 + wave;
        if (row >= rows) break;
        const float* lg = logits + (size_t)row * Q;
        const float* tl = teacher + (size_t)row * Q;
        int64_t tg = ce_target(tgt, tgt_stride, BL, row);
        [[maybe_unused]] float wr = 1.0f;
        if constexpr (W) {          // the row's weight, from the weight and the target alone: a zero-weight row loads no logits
            wr = ce_row_weight(o, row, tg, lane, status);
            if (wr == 0.f) { if (dlogits) ce_zero_row<NV>(dlogits + (size_t)row * Q, Q, lane); continue; }
            msum += (double)wr;
        }
        const float sc = W ? wr * inv : inv;          // the row's scale, formed once
        float ce, kl;
        bool bad = false;
        if constexpr (NV > 0) {
            float4 z[NV], u[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) { z[k] = *(const float4*)(lg + lane * 4 + 256 * k); u[k] = *(const float4*)(tl + lane * 4 + 256 * k); }
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }
            const float ztg = lg[tg];
            float mz = -INFINITY, mt = -INFINITY;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                mz = ce_max4(mz, z[k]);
                mt = ce_max4(mt, u[k]);
                bad = bad || dk_bad(u[k].x) || dk_bad(u[k].y) || dk_bad(u[k].z) || dk_bad(u[k].w);
            }
            mz = tr_wave_max(mz); mt = tr_wave_max(mt);
            float se = 0.f, sz = 0.f, st = 0.f;
            float4 ez[NV], eu[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                se += ce_expsum4(z[k], mz);
                ez[k] = make_float4(__expf((z[k].x - mz) * invT), __expf((z[k].y - mz) * invT), __expf((z[k].z - mz) * invT), __expf((z[k].w - mz) * invT));
                eu[k] = make_float4(__expf((u[k].x - mt) * invT), __expf((u[k].y - mt) * invT), __expf((u[k].z - mt) * invT), __expf((u[k].w - mt) * invT));
                sz += ce_sum4(ez[k]);
                st += ce_sum4(eu[k]);
            }
            se = tr_wave_sum(se); sz = tr_wave_sum(sz); st = tr_wave_sum(st);
            const float lse = logf(se) + mz, lsz = logf(sz), lst = logf(st), rz = 1.0f / sz, rt = 1.0f / st;
            float kq = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const float4 pz = make_float4(ez[k].x * rz, ez[k].y * rz, ez[k].z * rz, ez[k].w * rz);
                const float4 pt = make_float4(eu[k].x * rt, eu[k].y * rt, eu[k].z * rt, eu[k].w * rt);
                kq += (pt.x * (((u[k].x - mt) * invT - lst) - ((z[k].x - mz) * invT - lsz)) + pt.y * (((u[k].y - mt) * invT - lst) - ((z[k].y - mz) * invT - lsz))) +
                      (pt.z * (((u[k].z - mt) * invT - lst) - ((z[k].z - mz) * invT - lsz)) + pt.w * (((u[k].w - mt) * invT - lst) - ((z[k].w - mz) * invT - lsz)));
                if (dlogits) {
                    const int q = lane * 4 + 256 * k;
                    float4 g = make_float4(__expf(z[k].x - lse), __expf(z[k].y - lse), __expf(z[k].z - lse), __expf(z[k].w - lse));
                    const int dq = (int)tg - q;
                    if (dq == 0) g.x -= 1.0f; else if (dq == 1) g.y -= 1.0f; else if (dq == 2) g.z -= 1.0f; else if (dq == 3) g.w -= 1.0f;
                    *(float4*)(dlogits + (size_t)row * Q + q) = make_float4((oma * g.x + aT * (pz.x - pt.x)) * sc, (oma * g.y + aT * (pz.y - pt.y)) * sc,
                                                                            (oma * g.z + aT * (pz.z - pt.z)) * sc, (oma * g.w + aT * (pz.w - pt.w)) * sc);
                }
            }
            kl = tr_wave_sum(kq);
            ce = lse - ztg;
        } else {
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }
            const bool vec = (Q & 255) == 0;
            float mz = -INFINITY, mt = -INFINITY;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                mz = ce_max4(mz, v); mt = ce_max4(mt, w);
                bad = bad || dk_bad(w.x) || dk_bad(w.y) || dk_bad(w.z) || dk_bad(w.w);
            } else for (int q = lane; q < Q; q += 64) { const float w = tl[q]; mz = fmaxf(mz, lg[q]); mt = fmaxf(mt, w); bad = bad || dk_bad(w); }
            mz = tr_wave_max(mz); mt = tr_wave_max(mt);
            float se = 0.f, sz = 0.f, st = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                se += ce_expsum4(v, mz);
                sz += (__expf((v.x - mz) * invT) + __expf((v.y - mz) * invT)) + (__expf((v.z - mz) * invT) + __expf((v.w - mz) * invT));
                st += (__expf((w.x - mt) * invT) + __expf((w.y - mt) * invT)) + (__expf((w.z - mt) * invT) + __expf((w.w - mt) * invT));
            } else for (int q = lane; q < Q; q += 64) { se += expf(lg[q] - mz); sz += expf((lg[q] - mz) * invT); st += expf((tl[q] - mt) * invT); }
            se = tr_wave_sum(se); sz = tr_wave_sum(sz); st = tr_wave_sum(st);
            const float lse = logf(se) + mz, lsz = logf(sz), lst = logf(st), rz = 1.0f / sz, rt = 1.0f / st;
            float kq = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                const float zv[4] = {v.x, v.y, v.z, v.w}, wv[4] = {w.x, w.y, w.z, w.w};
                float gv[4], kv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = (zv[i] - mz) * invT, c = (wv[i] - mt) * invT;
                    const float pz = __expf(a) * rz, pt = __expf(c) * rt;
                    kv[i] = pt * ((c - lst) - (a - lsz));
                    gv[i] = (oma * (__expf(zv[i] - lse) - (q + i == tg ? 1.0f : 0.0f)) + aT * (pz - pt)) * sc;
                }
                kq += (kv[0] + kv[1]) + (kv[2] + kv[3]);
                if (dlogits) *(float4*)(dlogits + (size_t)row * Q + q) = make_float4(gv[0], gv[1], gv[2], gv[3]);
            } else for (int q = lane; q < Q; q += 64) {
                const float a = (lg[q] - mz) * invT, c = (tl[q] - mt) * invT;
                const float pz = expf(a) * rz, pt = expf(c) * rt;
                kq += pt * ((c - lst) - (a - lsz));
                if (dlogits) dlogits[(size_t)row * Q + q] = (oma * (expf(lg[q] - lse) - (q == tg ? 1.0f : 0.0f)) + aT * (pz - pt)) * sc;
            }
            kl = tr_wave_sum(kq);
            ce = lse - lg[tg];
        }
        if (__any(bad) && lane == 0) atomicOr(status, 32);
        if constexpr (W) { csum += (double)ce * (double)wr; ksum += (double)kl * (double)wr; } else { csum += (double)ce; ksum += (double)kl; }
    }
    if (lane == 0) { part[0][wave] = csum; part[1][wave] = ksum; if constexpr (W) part[2][wave] = msum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double den = ce_opt_den<W>(o, rows);
        const double c = ce_part_sum(part[0]) / den, k = ce_part_sum(part[1]) / den;
        atomicAdd(loss + (blockIdx.x & 63), (double)oma * c + (double)alpha * ((double)temp * (double)temp) * k);
        if (comp) { atomicAdd(comp + (blockIdx.x & 63), c); atomicAdd(comp + 64 + (blockIdx.x & 63), k); }
        if constexpr (W) if (o.mass) atomicAdd(o.mass + (blockIdx.x & 63), ce_part_sum(part[2]));
    }
}

// ------------------------------------------------------------------ the host launcher (called from train_host.hip)
// f(std::integral_constant<int, NV>) for the register form that holds a row of Q classes (Q = 256 NV <= 1024; 16-byte loads: every base pointer must be
// 16-byte aligned, checked by the callers), NV = 0 -- the loops -- for anything else
template <class F> static void ce_with_nv(int Q, F&& f) {
    switch ((Q % 256 == 0 && Q <= 1024) ? Q / 256 : 0) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        default: f(std::integral_constant<int, 0>()); break;
    }
}

int qpn_launch_loss(const LossCall& c, hipStream_t stream) {
    const int64_t rows = (int64_t)c.B * c.BL;
    // (the loss accumulator was cleared by this step's refresh; a loss call without a forward in front clears it itself)
    if (!c.loss_cleared) QPN_HIP(hipMemsetAsync(c.loss, 0, 64 * sizeof(double), stream));
    if (c.comp) QPN_HIP(hipMemsetAsync(c.comp, 0, 128 * sizeof(double), stream));
    // opts (nullptr: none): the W instances, behind the clear of the 64 mass slots and, for norm = "weights", the word they divide by
    const CeOpts o = c.opts ? *c.opts : CeOpts{nullptr, 0, 0, 0.f, nullptr, nullptr};
    if (o.mass) QPN_HIP(hipMemsetAsync(o.mass, 0, 64 * sizeof(double), stream));
    if (o.norm_mass) hipLaunchKernelGGL(k_weight_mass, dim3(1), dim3(1024), 0, stream, c.targets, c.tgt_stride, c.BL, rows, o, const_cast<double*>(o.norm_mass));
    const int rpw = 4;                // 16 rows per workgroup: ~1250 workgroups for a 20 k-row chunk (64 rows per workgroup left most CUs with one)
    const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
    ce_with_nv(c.Q, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (c.teacher) {
            if (c.opts) hipLaunchKernelGGL((k_ce_soft<NV, true>), grid, dim3(256), 0, stream, c.logits, c.teacher, c.targets, c.tgt_stride, c.BL, c.Q, rows, c.alpha, c.temp, c.dlogits, c.loss, c.comp, rpw, c.status, o);
            else hipLaunchKernelGGL((k_ce_soft<NV, false>), grid, dim3(256), 0, stream, c.logits, c.teacher, c.targets, c.tgt_stride, c.BL, c.Q, rows, c.alpha, c.temp, c.dlogits, c.loss, c.comp, rpw, c.status, o);
        } else if (c.opts) hipLaunchKernelGGL((k_ce_hard<NV, true>), grid, dim3(256), 0, stream, c.logits, c.targets, c.tgt_stride, c.BL, c.Q, rows, c.dlogits, c.loss, rpw, c.status, o);
        else hipLaunchKernelGGL((k_ce_hard<0, false>), grid, dim3(256), 0, stream, c.logits, c.targets, c.tgt_stride, c.BL, c.Q, rows, c.dlogits, c.loss, rpw, c.status, o);      // the plain criterion: the loops at every Q
    });
    qpn_prof_mark(PG_CE, stream);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
