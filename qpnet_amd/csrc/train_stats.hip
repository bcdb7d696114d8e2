// train_stats.hip -- per-tensor training statistics (qpn_tensor_stats) on gfx950: which tensor's gradient, weight or update is out of line.  Two launches that only
// READ the buffers an optimiser step leaves behind -- nothing here is on the step's path, and no kernel of the step knows of it.
//
//   k_tensor_stats_items : pass 1, one workgroup per work item (train_stats_plan.h: at most QPN_STATS_ITEM elements of one tensor) -> one partial record per item
//   k_tensor_stats_fold  : pass 2, one thread per tensor adds its items' partials in item order, applies the gradient denominator -> one record per tensor
//   qpn_tensor_stats     : the checks, the plan on the handle, the two launches, the drain
//
// The update is not stored anywhere: k_adam (train_adam.hip) leaves the gradient buffer as it is, and m, v after a launch determine what that launch subtracted,
// (lr / bc1) * (m_i / (sqrtf(v_i) / bc2_sqrt + eps)).  Pass 1 forms the second factor in the fp32 expression of adam_update; the caller multiplies by lr / bc1 of the tensor's group.
#include "train_common.h"
#include "qpn_handle.h"
#include <math.h>

// what a thread has seen of its item so far
struct StatsAcc { double gs, ws, us; float gmax, wmax; int gnf; };

__device__ __forceinline__ void stats_add_grad(StatsAcc& a, float x) {
    if (isfinite(x)) { a.gs += (double)x * (double)x; a.gmax = fmaxf(a.gmax, fabsf(x)); }      // (an fp32 square is exact in fp64)
    else ++a.gnf;
}
__device__ __forceinline__ void stats_add_weight(StatsAcc& a, float x) {
    if (isfinite(x)) { a.ws += (double)x * (double)x; a.wmax = fmaxf(a.wmax, fabsf(x)); }
}
__device__ __forceinline__ void stats_add_update(StatsAcc& a, float mi, float vi, float bc2_sqrt, float eps) {
    const float denom = sqrtf(vi) / bc2_sqrt + eps;             // adam_update's denom and mi / denom, the same fp32 operations
    const float u = mi / denom;
    a.us += (double)u * (double)u;
}
// elements [i0, i1), one by one: the part of an item in front of its first whole quad, or behind its last
__device__ __forceinline__ void stats_add_range(StatsAcc& a, const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                                                int64_t i0, int64_t i1, float bc2_sqrt, float eps) {
    for (int64_t i = i0; i < i1; ++i) {
        if (g) stats_add_grad(a, g[i]);
        stats_add_weight(a, w[i]);
        if (m) stats_add_update(a, m[i], v[i], bc2_sqrt, eps);
    }
}
// quad q of a buffer (elements 4q .. 4q + 3 of it): one 16-byte load from a 16-byte aligned base, four loads from any other -- the same four values
__device__ __forceinline__ float4 stats_load_quad(const float* __restrict__ p, int64_t q, bool aligned) {
    if (aligned) return reinterpret_cast<const float4*>(p)[q];
    return make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
}

// Pass 1.  Item [begin, end) of the flat vector: its whole quads (quad q = elements 4q .. 4q + 3, counted from element 0 of the vector, as k_grad_sumsq counts them)
// go to thread (q - first whole quad) % 256, at most QPN_STATS_ITEM / 1024 to a thread; the up to three elements in front of the first whole quad and behind
// the last one are thread 0's, added before and after its quads.  A thread adds in index order; the 256 sums meet in block_sum_f64's order.  So every addition's
// place is a function of (begin, end) alone: the same bits from run to run and at any alignment of the four bases (each buffer is read with 16-byte loads when
// ITS base allows).  g, and the pair m / v, may be null: their fields stay 0.  Non-finite gradient elements are counted and left out of sum and maximum, non-finite
// weights are left out.  The sums are of the gradient as stored; pass 2 divides.
constexpr int STATS_ROUNDS = QPN_STATS_ITEM / 1024;
__global__ __launch_bounds__(256, 8) void k_tensor_stats_items(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                                                            const StatsItem* __restrict__ items, float bc2_sqrt, float eps, qpn_tensor_stat* __restrict__ part) {
    __shared__ double red[3][4];
    __shared__ float redf[2][4];
    __shared__ int redi[4];
    const StatsItem it = items[blockIdx.x];
    const int64_t qb = (it.begin + 3) >> 2, qe = it.end >> 2;             // whole quads [qb, qe); qb > qe: the item lies inside one quad
    const int64_t head_end = qb * 4 < it.end ? qb * 4 : it.end;
    const int64_t tail_begin = qe >= qb ? qe * 4 : it.end;
    StatsAcc a = {};
    if (threadIdx.x == 0) stats_add_range(a, g, w, m, v, it.begin, head_end, bc2_sqrt, eps);
    const bool ag = (reinterpret_cast<uintptr_t>(g) & 15) == 0, aw = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const bool am = (reinterpret_cast<uintptr_t>(m) & 15) == 0, av = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
    float4 xg[STATS_ROUNDS], xw[STATS_ROUNDS], xm[STATS_ROUNDS], xv[STATS_ROUNDS];
#pragma unroll
    for (int k = 0; k < STATS_ROUNDS; ++k) {                              // every load of the thread first, none waited for
        const int64_t q = qb + threadIdx.x + 256 * k;
        xg[k] = xw[k] = xm[k] = xv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < qe) {
            xw[k] = stats_load_quad(w, q, aw);
            if (g) xg[k] = stats_load_quad(g, q, ag);
            if (m) { xm[k] = stats_load_quad(m, q, am); xv[k] = stats_load_quad(v, q, av); }
        }
    }
#pragma unroll
    for (int k = 0; k < STATS_ROUNDS; ++k) {
        const int64_t q = qb + threadIdx.x + 256 * k;
        if (q >= qe) continue;
        if (g) { stats_add_grad(a, xg[k].x); stats_add_grad(a, xg[k].y); stats_add_grad(a, xg[k].z); stats_add_grad(a, xg[k].w); }
        stats_add_weight(a, xw[k].x); stats_add_weight(a, xw[k].y); stats_add_weight(a, xw[k].z); stats_add_weight(a, xw[k].w);
        if (m) {
            stats_add_update(a, xm[k].x, xv[k].x, bc2_sqrt, eps); stats_add_update(a, xm[k].y, xv[k].y, bc2_sqrt, eps);
            stats_add_update(a, xm[k].z, xv[k].z, bc2_sqrt, eps); stats_add_update(a, xm[k].w, xv[k].w, bc2_sqrt, eps);
        }
    }
    if (threadIdx.x == 0) stats_add_range(a, g, w, m, v, tail_begin, it.end, bc2_sqrt, eps);
    // maxima and the count: xor butterfly inside each wave, the four wave values through LDS (block_sum_f64's barrier is theirs too)
    float gmax = a.gmax, wmax = a.wmax; int gnf = a.gnf;
    for (int sft = 32; sft >= 1; sft >>= 1) { gmax = fmaxf(gmax, __shfl_xor(gmax, sft)); wmax = fmaxf(wmax, __shfl_xor(wmax, sft)); gnf += __shfl_xor(gnf, sft); }
    if ((threadIdx.x & 63) == 0) { redf[0][threadIdx.x >> 6] = gmax; redf[1][threadIdx.x >> 6] = wmax; redi[threadIdx.x >> 6] = gnf; }
    const double gs = block_sum_f64(a.gs, red[0]), ws = block_sum_f64(a.ws, red[1]), us = block_sum_f64(a.us, red[2]);
    if (threadIdx.x == 0) {
        qpn_tensor_stat r;
        r.grad_sumsq = gs; r.weight_sumsq = ws; r.update_sumsq = us;
        r.grad_absmax = fmaxf(fmaxf(redf[0][0], redf[0][1]), fmaxf(redf[0][2], redf[0][3]));
        r.weight_absmax = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
        r.grad_nonfinite = (int64_t)redi[0] + redi[1] + redi[2] + redi[3];
        part[blockIdx.x] = r;
    }
}

// Pass 2.  Thread t adds the partial records of tensor t's items, first_item[t] .. first_item[t + 1] - 1, in that order, then applies the denominator the Adam launch
// divides the gradient by (den[0]: the summed row count of a data-parallel or accumulated gradient; null: 1): the sum of squares in fp64 by den^2, the maximum in
// fp32 by den -- k_adam's own g / den[0] of the largest element, division by a positive number being monotonic.
__global__ __launch_bounds__(256) void k_tensor_stats_fold(const qpn_tensor_stat* __restrict__ part, const int* __restrict__ first_item, int n_tensors,
                                                           const float* __restrict__ den, qpn_tensor_stat* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tensors) return;
    qpn_tensor_stat r = {};
    for (int i = first_item[t]; i < first_item[t + 1]; ++i) {
        const qpn_tensor_stat p = part[i];
        r.grad_sumsq += p.grad_sumsq; r.weight_sumsq += p.weight_sumsq; r.update_sumsq += p.update_sumsq;
        r.grad_absmax = fmaxf(r.grad_absmax, p.grad_absmax); r.weight_absmax = fmaxf(r.weight_absmax, p.weight_absmax);
        r.grad_nonfinite += p.grad_nonfinite;
    }
    if (den) {
        const float d = den[0];
        r.grad_sumsq = r.grad_sumsq / ((double)d * (double)d);
        r.grad_absmax = r.grad_absmax / d;
    }
    out[t] = r;
}

// ------------------------------------------------------------------------------------------ host
// The plan lives on the handle with its device copy, one allocation: [items | partial records, one per item | records, one per tensor | first_item].  A call
// whose table is the one the handle holds uploads nothing (the qpn_adam_groups rule).
static int stats_plan_upload(qpn_handle* h, int n_tensors, const int64_t* h_tensor_end, hipStream_t stream) {
    if (h->d_stats && h->stats_plan.same_table(n_tensors, h_tensor_end)) return QPN_OK;
    StatsPlan p = stats_plan_build(n_tensors, h_tensor_end);
    const size_t ni = p.items.size(), nt = (size_t)n_tensors;
    const size_t bytes = ni * sizeof(StatsItem) + (ni + nt) * sizeof(qpn_tensor_stat) + (nt + 1) * sizeof(int32_t);
    char* d_new = nullptr;
    QPN_HIP(hipStreamSynchronize(stream));
    QPN_HIP(hipMalloc(&d_new, bytes));
    hipError_t e = hipMemcpy(d_new, p.items.data(), ni * sizeof(StatsItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_new + ni * sizeof(StatsItem) + (ni + nt) * sizeof(qpn_tensor_stat), p.first_item.data(), (nt + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_new); QPN_HIP(e); }
    if (h->d_stats) (void)hipFree(h->d_stats);
    h->d_stats = d_new;
    h->stats_plan = std::move(p);
    return QPN_OK;
}

extern "C" int qpn_tensor_stats(qpn_handle* h, const float* d_flat, const float* d_grad, const float* d_m, const float* d_v,
                                int64_t n, int step, float beta1, float beta2, float eps, const float* d_grad_denominator,
                                int n_tensors, const int64_t* h_tensor_end, qpn_tensor_stat* h_out, void* stream_) {
    if (!h) { qpn_set_error("null handle"); return QPN_EINVAL; }
    if (!d_flat) { qpn_set_error("bad tensor_stats arguments: d_flat is NULL"); return QPN_EINVAL; }
    if (!h_out) { qpn_set_error("bad tensor_stats arguments: h_out is NULL"); return QPN_EINVAL; }
    char why[256];
    if (!stats_table_check(n, n_tensors, h_tensor_end, why, sizeof(why))) { qpn_set_error("bad tensor_stats arguments: %s", why); return QPN_EINVAL; }
    if ((d_m == nullptr) != (d_v == nullptr)) { qpn_set_error("bad tensor_stats arguments: %s is NULL while %s is given (both moments, or neither)", d_m ? "d_v" : "d_m", d_m ? "d_m" : "d_v"); return QPN_EINVAL; }
    float bc2_sqrt = 1.0f;
    if (d_m) {
        if (step < 1) { qpn_set_error("bad tensor_stats arguments: step must be >= 1 with moments (got %d)", step); return QPN_EINVAL; }
        if (!(beta1 >= 0.0f && beta1 < 1.0f)) { qpn_set_error("bad tensor_stats arguments: beta1 must lie in [0, 1) (got %g)", (double)beta1); return QPN_EINVAL; }
        if (!(beta2 >= 0.0f && beta2 < 1.0f)) { qpn_set_error("bad tensor_stats arguments: beta2 must lie in [0, 1) (got %g)", (double)beta2); return QPN_EINVAL; }
        if (!(eps >= 0.0f) || isinf(eps)) { qpn_set_error("bad tensor_stats arguments: eps must be a finite number >= 0 (got %g)", (double)eps); return QPN_EINVAL; }
        bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, step));           // qpn_launch_adam's expression for update number `step`: fp64, rounded once
    }
    if (h->device < 0) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    const hipStream_t stream = (hipStream_t)stream_;
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap_st);
    if (cap_st != hipStreamCaptureStatusNone) { qpn_set_error("qpn_tensor_stats while the stream is capturing (the call drains the stream and reads the records back)"); return QPN_ESTATE; }
    int rc = stats_plan_upload(h, n_tensors, h_tensor_end, stream); if (rc) return rc;
    const size_t ni = h->stats_plan.items.size(), nt = (size_t)n_tensors;
    const StatsItem* d_items = reinterpret_cast<const StatsItem*>(h->d_stats);
    qpn_tensor_stat* d_part = reinterpret_cast<qpn_tensor_stat*>(h->d_stats + ni * sizeof(StatsItem));
    qpn_tensor_stat* d_out = d_part + ni;
    const int* d_first = reinterpret_cast<const int*>(d_out + nt);
    hipLaunchKernelGGL(k_tensor_stats_items, dim3((unsigned)ni), dim3(256), 0, stream, d_grad, d_flat, d_m, d_v, d_items, bc2_sqrt, eps, d_part);
    hipLaunchKernelGGL(k_tensor_stats_fold, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, (const qpn_tensor_stat*)d_part, d_first, n_tensors,
                       d_grad ? d_grad_denominator : nullptr, d_out);
    QPN_HIP(hipGetLastError());
    QPN_HIP(hipStreamSynchronize(stream));
    QPN_HIP(hipMemcpy(h_out, d_out, nt * sizeof(qpn_tensor_stat), hipMemcpyDeviceToHost));
    return QPN_OK;
}
