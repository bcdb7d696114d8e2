// train_adam.hip -- the optimiser step of the fused trainer on gfx950: torch.optim.Adam over the flat parameter buffer, with everything that was built around it.
//
//   k_adam<CLIP, EMA, GROUPED> : the update (single tensor semantics, fp32).  CLIP: behind k_grad_sumsq, torch.nn.utils.clip_grad_norm_ in the same launch;
//                                EMA: the averaged weights move with every applied update; GROUPED: per-element lr / weight decay and frozen ranges (adam_groups.h)
//   k_grad_sumsq[_grp]         : the squared gradient norm as at most TR_GN_BLOCKS fp64 partial sums, in one fixed order
//   k_grad_accum               : gradient accumulation, acc <- first ? g : acc + g
//   qpn_launch_adam            : the one launcher of an AdamCall (train_common.h);  qpn_launch_grad_accum
#include "train_common.h"
#include <math.h>

// rep: the step's reports, written straight into pinned host memory by the step's last kernel (a copy engine launch each -- 3-4 us on the stream -- otherwise):
// the status word and, when asked for, the 64 partial sums of the loss (qpn_train_step)
struct AdamReports { int* h_status; double* h_loss; const double* d_loss; };
// the update of element i from its (scaled, clipped) gradient gi; returns the new weight
__device__ __forceinline__ float adam_update(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, int64_t i, float gi,
                                             float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
    if (wd != 0.f) gi += wd * w[i];
    const float mi = m[i] + (gi - m[i]) * (1.0f - b1);          // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float wn = w[i] - (lr / bc1) * (mi / denom);
    w[i] = wn;
    return wn;
}
// Parameter groups (qpn_adam_groups).  The block reads its pair of the table's block index (adam_groups.h) -- ONE uniform 8-byte load, asked for at the top of the
// kernel, next to the status word's, so that it puts no latency of its own in front of the loads of w, m, v, g.  In nearly every block the pair IS the lookup: the
// group is the same for all 256 elements, the branch below is uniform and no segment is read.  Only a block that a segment boundary crosses walks: every thread
// forward from the block's first segment to its own element.  lr / weight_decay then come out of the kernel arguments (a chain of selects over constant indices:
// SGPRs, no scratch).
// -> false: the element is frozen (w, m, v, g are not touched; the caller still moves the average)
// A workgroup of a grouped launch updates QPN_ADAM_WG_BLOCKS consecutive blocks, 256 elements at a time: the fixed cost of a workgroup (its launch, the status
// word's and the pairs' latency, when clipping the sum of the partials) is paid once per 1024 elements, and its pairs -- the index is padded -- are one 32-byte uniform load.
struct AdamGroupPairs { int2 p[QPN_ADAM_WG_BLOCKS]; };
__device__ __forceinline__ AdamGroupPairs adam_group_block(const AdamGroupsArg* G) {
    AdamGroupPairs r;
    const int2* src = reinterpret_cast<const int2*>(G->block) + (size_t)blockIdx.x * QPN_ADAM_WG_BLOCKS;
#pragma unroll
    for (int k = 0; k < QPN_ADAM_WG_BLOCKS; ++k) r.p[k] = src[k];
    return r;
}
__device__ __forceinline__ bool adam_group_values(const AdamGroupsArg* G, int2 blk, int64_t i, float& lr, float& wd) {
    int q = blk.y;
    if (q == QPN_ADAM_MIXED) {
        int s = blk.x;
        while (G->seg_end[s] <= i) ++s;                         // (the last end is n > i: the walk stays inside the table)
        q = G->seg_group[s];
    }
    if (q < 0) return false;
#pragma unroll
    for (int k = 0; k < QPN_ADAM_MAX_GROUPS; ++k) if (q == k) { lr = G->lr[k]; wd = G->wd[k]; }
    return true;
}

// The three switches are compile-time: an instance with one off is the kernel as it was before that feature (its arguments are dead there).
// The device-side status word (sticky until the host reads it: a tap / target out of range, an abandoned stack launch) flags results that must not
// reach the parameters: the update of a flagged step -- and of the steps enqueued behind it until the host has collected the word, two steps later
// at most -- is skipped; weights and both moments stay what the last clean step left (the host raises; the caller may drop the chunk and go on).
// Data-parallel (den = the exchanged trailer {summed row count, summed flags}): a step ANY rank flagged is skipped by EVERY rank -- the replicas stay
// identical -- and a rank that was not flagged itself sets bit 8 of its own word, so that its host raises too.
// CLIP -- torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2) in front of the update, as ONE extra launch (k_grad_sumsq) and no host round trip.
// EVERY block adds the npart <= 256 partial sums itself, in block_sum_f64's order: all blocks of the launch (and all ranks) derive the same total, hence the
// same coefficient and the same decision to skip, with no finalising block, counter or fence.
//   total = sqrt(sum g^2) (/ den[0]: the norm of the AVERAGED gradient);  coef = min(1, max_norm / (total + 1e-6)) in fp64, rounded once;  g <- (g / den[0]) * coef, then weight decay.
// The gradient buffer is left as it is.  A non-finite total skips the update like a flagged step (bit 16 of the status word, set by block 0; the blocks decide by
// their own total, not by the word).  Block 0 leaves the total in *d_norm (and the step's pinned report slot).
// EMA -- averaged weights (qpn_adam_step_avg): the thread that has just computed element i's new weight moves the average towards it, e += (w_new - e) * omd with
// omd = 1 - decay formed once on the host.  A skipped update returns before it: the average is of APPLIED states.
// GROUPED -- lr / weight_decay come from G, per element (the two arguments are not looked at); behind k_grad_sumsq_grp the norm is that of the elements that are not frozen.
// (Positional arguments, G directly behind rep: with it the grouped instances keep the instruction and wait counts they had as kernels of their own; G at the end
// costs them 3-4 instructions, one argument struct up to 21 waits -- profiles/adam_step.txt.)
template <bool CLIP, bool EMA, bool GROUPED>
__global__ __launch_bounds__(CLIP ? 256 : 1024) void k_adam(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                            float lr_, float b1, float b2, float eps, float wd_, float bc1, float bc2_sqrt, const float* __restrict__ den, int* __restrict__ status, AdamReports rep, AdamGroupsArg G,
                                                            const double* __restrict__ part, int npart, float max_norm, double* __restrict__ d_norm, double* h_norm,
                                                            float* __restrict__ e, float omd) {
    constexpr int NB = GROUPED ? QPN_ADAM_WG_BLOCKS : 1;        // 256-element blocks per workgroup
    float lr = GROUPED ? 0.f : lr_, wd = GROUPED ? 0.f : wd_;
    int64_t i = (int64_t)blockIdx.x * NB * blockDim.x + threadIdx.x;
    AdamGroupPairs blk = {};
    if (GROUPED) blk = adam_group_block(&G);
    double total = 0.0;
    if constexpr (CLIP) {
        __shared__ double red[4];
        total = sqrt(block_sum_f64((int)threadIdx.x < npart ? part[threadIdx.x] : 0.0, red));
        if (den) total = total / (double)den[0];
    }
    const bool bad = CLIP && !isfinite(total);
    const bool peer = den && den[1] > 0.f;
    const bool skip = bad || peer || (status && *status);
    if (blockIdx.x == 0) {
        if (rep.h_loss && threadIdx.x < 64) rep.h_loss[threadIdx.x] = rep.d_loss[threadIdx.x];
        if (threadIdx.x == 0) {
            if (CLIP) {
                *d_norm = total;
                if (h_norm) *h_norm = total;
            }
            if (status) {
                int st = *status;
                if (peer && !st) { st = 8; atomicOr(status, 8); }
                if (bad) { st |= 1 << 16; atomicOr(status, 1 << 16); }
                if (rep.h_status) *rep.h_status = st;
                if (!skip) atomicAdd((unsigned long long*)(status + 2), 1ull);      // updates APPLIED on this handle (qpn_train_applied_updates)
            }
        }
    }
    if (skip) return;
    float coef = 1.0f;
    if (CLIP) {
        const double c = (double)max_norm / (total + 1e-6);
        coef = c < 1.0 ? (float)c : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k, i += blockDim.x) {
        if (i >= n) return;
        if (GROUPED && !adam_group_values(&G, blk.p[k], i, lr, wd)) {      // frozen: only the average moves, towards the weight that stays
            if (EMA) e[i] = e[i] + (w[i] - e[i]) * omd;
            continue;
        }
        float gi = g[i];
        if (den) gi = gi / den[0];                              // data-parallel: summed row-weighted gradients / summed row count
        if (CLIP) gi = __fmul_rn(gi, coef);                     // (a product of its own: never fused into the weight-decay term, so coef == 1 leaves the unclipped bits)
        const float wn = adam_update(w, m, v, i, gi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        if (EMA) e[i] = e[i] + (wn - e[i]) * omd;
    }
}

// part[block] = sum of g[i]^2 over the block's share of the first n floats, in fp64 (an fp32 square is exact in fp64: the sum is good to n * 2^-53).
// The order of every addition is a function of n alone: element i belongs to quad i / 4, quad q to thread q % (threads of the grid), a thread adds its quads
// in index order, the short last quad included; then block_sum_f64.  No atomics: the same bits from run to run, and on every data-parallel rank (they hold
// the same exchanged buffer) wherever its allocator put that buffer -- a 16-byte aligned base reads a quad as one float4, any other base as four floats.
__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double red[4];
    const int64_t nq = n >> 2, nthr = (int64_t)gridDim.x * 256, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 4
        for (int64_t q = t; q < nq; q += nthr) {
            const float4 x = g4[q];
            acc += (double)x.x * (double)x.x; acc += (double)x.y * (double)x.y; acc += (double)x.z * (double)x.z; acc += (double)x.w * (double)x.w;
        }
    } else {
#pragma unroll 4
        for (int64_t q = t; q < nq; q += nthr) {
            const float x0 = g[4 * q], x1 = g[4 * q + 1], x2 = g[4 * q + 2], x3 = g[4 * q + 3];
            acc += (double)x0 * (double)x0; acc += (double)x1 * (double)x1; acc += (double)x2 * (double)x2; acc += (double)x3 * (double)x3;
        }
    }
    if (t == nq % nthr) for (int64_t i = nq * 4; i < n; ++i) acc += (double)g[i] * (double)g[i];      // the last n % 4 floats: quad nq, read one by one
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// k_grad_sumsq over the elements that are not frozen (qpn_adam_groups): the same quads on the same threads, added in the same order, a frozen element left out --
// bit for bit the sum k_grad_sumsq forms of the gradient with its frozen elements set to +0 (the accumulator is never -0: adding +0 changes nothing), and a frozen
// element's gradient is not read at all.  A wave's 64 quads are the 256 elements of ONE block of the table: the lookup is one (wave-uniform) 8-byte load per quad.
// Four quads per round, as k_grad_sumsq's unroll has them: first the four pairs, then the four gradient loads (each under its pair's verdict, none waited for), then
// the sums in quad order -- the grid is at most TR_GN_BLOCKS blocks, so it is the loads in flight per thread that the rate lives on.  A quad of a mixed block
// (a segment boundary inside the block) is walked element by element, in its place in that order.
__device__ __forceinline__ void sumsq_mixed(const float* __restrict__ g, const AdamGroupsArg& G, int s, int64_t i0, int64_t i1, double& acc) {
    for (int64_t i = i0; i < i1; ++i) {
        while (G.seg_end[s] <= i) ++s;
        if (G.seg_group[s] >= 0) acc += (double)g[i] * (double)g[i];
    }
}
__global__ __launch_bounds__(256) void k_grad_sumsq_grp(const float* __restrict__ g, int64_t n, double* __restrict__ part, AdamGroupsArg G) {
    __shared__ double red[4];
    const int64_t nq = n >> 2, nthr = (int64_t)gridDim.x * 256, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    const int2* const blocks = reinterpret_cast<const int2*>(G.block);
    double acc = 0.0;
    for (int64_t q0 = t; q0 < nq; q0 += 4 * nthr) {
        int2 blk[4]; float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t q = q0 + k * nthr;
            blk[k] = q < nq ? blocks[q >> 6] : make_int2(0, QPN_ADAM_FROZEN);      // (quad q = elements 4q .. 4q + 3 of block 4q / 256; past the end: nothing to add)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t q = q0 + k * nthr;
            x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (blk[k].y >= 0) {
                if (aligned) x[k] = reinterpret_cast<const float4*>(g)[q];
                else { x[k].x = g[4 * q]; x[k].y = g[4 * q + 1]; x[k].z = g[4 * q + 2]; x[k].w = g[4 * q + 3]; }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t q = q0 + k * nthr;
            if (blk[k].y == QPN_ADAM_MIXED) sumsq_mixed(g, G, blk[k].x, 4 * q, 4 * q + 4, acc);
            else if (blk[k].y >= 0) {
                acc += (double)x[k].x * (double)x[k].x; acc += (double)x[k].y * (double)x[k].y; acc += (double)x[k].z * (double)x[k].z; acc += (double)x[k].w * (double)x[k].w;
            }
        }
    }
    if (t == nq % nthr && nq * 4 < n) {                           // the last n % 4 floats: quad nq, read one by one
        const int2 b = blocks[nq >> 6];
        if (b.y == QPN_ADAM_MIXED) sumsq_mixed(g, G, b.x, nq * 4, n, acc);
        else if (b.y >= 0) for (int64_t i = nq * 4; i < n; ++i) acc += (double)g[i] * (double)g[i];
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- gradient accumulation (qpn_grad_accumulate / qpn_train_step_acc): acc <- first ? g : acc + g over cnt floats -- the row-weighted gradient of one chunk and its
// {row count, flags, 0, 0} trailer added to the window's.  One fp32 add per element and nothing else: the result is a function of the two inputs alone (numpy's
// float32 acc + g), the same bits from run to run and on every rank.  first OVERWRITES -- acc is not read, so whatever an earlier (abandoned) window or the allocator
// left there, NaNs included, is gone without a memset in the step.  Access as k_grad_sumsq's: quad q belongs to thread q % (threads of the grid), one float4 per
// buffer when BOTH bases are 16-byte aligned, four floats otherwise (the caller's g may start one float into an allocation); the short last quad one by one.
// rep: a micro-step that does not close its window has no Adam launch behind it, and this is its last kernel: block 0 carries the step's reports (the status word,
// the loss partials) into pinned memory as k_adam's block 0 does -- it reports only: no flag is raised, nothing is counted
__global__ __launch_bounds__(256) void k_grad_accum(float* __restrict__ acc, const float* __restrict__ g, int64_t cnt, int first, const int* __restrict__ status, AdamReports rep) {
    if (blockIdx.x == 0) {
        if (rep.h_loss && threadIdx.x < 64) rep.h_loss[threadIdx.x] = rep.d_loss[threadIdx.x];
        if (threadIdx.x == 0 && status && rep.h_status) *rep.h_status = *status;
    }
    const int64_t nq = cnt >> 2, nthr = (int64_t)gridDim.x * 256, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 15) == 0) {
        float4* a4 = reinterpret_cast<float4*>(acc);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        if (first) {
#pragma unroll 4
            for (int64_t q = t; q < nq; q += nthr) a4[q] = g4[q];
        } else {
#pragma unroll 4
            for (int64_t q = t; q < nq; q += nthr) {
                const float4 x = g4[q];
                float4 a = a4[q];
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
                a4[q] = a;
            }
        }
    } else if (first) {
#pragma unroll 4
        for (int64_t q = t; q < nq; q += nthr) {
            const float x0 = g[4 * q], x1 = g[4 * q + 1], x2 = g[4 * q + 2], x3 = g[4 * q + 3];
            acc[4 * q] = x0; acc[4 * q + 1] = x1; acc[4 * q + 2] = x2; acc[4 * q + 3] = x3;
        }
    } else {
#pragma unroll 4
        for (int64_t q = t; q < nq; q += nthr) {
            const float x0 = g[4 * q], x1 = g[4 * q + 1], x2 = g[4 * q + 2], x3 = g[4 * q + 3];
            const float a0 = acc[4 * q], a1 = acc[4 * q + 1], a2 = acc[4 * q + 2], a3 = acc[4 * q + 3];
            acc[4 * q] = a0 + x0; acc[4 * q + 1] = a1 + x1; acc[4 * q + 2] = a2 + x2; acc[4 * q + 3] = a3 + x3;
        }
    }
    if (t == nq % nthr) for (int64_t i = nq * 4; i < cnt; ++i) acc[i] = first ? g[i] : acc[i] + g[i];      // the last cnt % 4 floats: quad nq, one by one
}

// ------------------------------------------------------------------------------------------ launchers
// a report is made only where its source exists: the status word for h_status, the device's loss partials for h_loss
static AdamReports adam_reports(const int* status, int* h_status, double* h_loss, const double* d_loss) {
    AdamReports rep; rep.h_status = status ? h_status : nullptr; rep.h_loss = d_loss ? h_loss : nullptr; rep.d_loss = d_loss;
    return rep;
}

// One Adam launch (AdamCall, train_common.h): max_norm > 0 puts k_grad_sumsq[_grp] in front and clips; ema != nullptr moves the averaged weights; grp != nullptr
// takes lr / wd per element from the table (the call's own two are not looked at).  An ungrouped launch is a block per 256 elements, a grouped one a workgroup per
// QPN_ADAM_WG_BLOCKS of them.
int qpn_launch_adam(const AdamCall& c, hipStream_t stream) {
    static constexpr decltype(&k_adam<false, false, false>) instance[8] = {
        k_adam<false, false, false>, k_adam<false, false, true>, k_adam<false, true, false>, k_adam<false, true, true>,
        k_adam<true, false, false>, k_adam<true, false, true>, k_adam<true, true, false>, k_adam<true, true, true>};
    const double bc1 = 1.0 - pow((double)c.b1, c.step), bc2 = 1.0 - pow((double)c.b2, c.step);
    const bool clip = c.max_norm > 0.f;
    int nb = 0;
    if (clip) {
        const int64_t want = ((c.n >> 2) + 1 + 255) / 256;     // a thread per quad (and one for the short last quad) until the grid is full
        nb = want < TR_GN_BLOCKS ? (int)want : TR_GN_BLOCKS;
        if (c.grp) hipLaunchKernelGGL(k_grad_sumsq_grp, dim3(nb), dim3(256), 0, stream, c.g, c.n, c.part, *c.grp);
        else hipLaunchKernelGGL(k_grad_sumsq, dim3(nb), dim3(256), 0, stream, c.g, c.n, c.part);
    }
    const int64_t per_wg = c.grp ? QPN_ADAM_WG_BLOCKS * 256 : 256;
    hipLaunchKernelGGL(instance[4 * clip + 2 * (c.ema != nullptr) + (c.grp != nullptr)], dim3((unsigned)((c.n + per_wg - 1) / per_wg)), dim3(256), 0, stream,
                       c.w, c.g, c.m, c.v, c.n, c.lr, c.b1, c.b2, c.eps, c.wd, (float)bc1, (float)sqrt(bc2), c.den, c.status, adam_reports(c.status, c.h_status, c.h_loss, c.d_loss),
                       c.grp ? *c.grp : AdamGroupsArg{}, (const double*)c.part, nb, c.max_norm, c.d_norm, c.h_norm, c.ema, c.omd);
    qpn_prof_mark(PG_ADAM, stream);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}

// acc <- first ? g : acc + g over cnt floats (k_grad_accum).  The grid comes from the device, not from cnt: at most 8 blocks of 256 threads per compute unit,
// fewer while a thread per quad (and one for the short last quad) does not fill them; the rest is the kernel's stride.  status / h_status / h_loss / d_loss: the reports
// of a micro-step whose last kernel this is (qpn_train_step_acc), all NULL otherwise
int qpn_launch_grad_accum(float* acc, const float* g, int64_t cnt, int first, const int* status, int* h_status, double* h_loss, const double* d_loss, hipStream_t stream) {
    const int64_t want = ((cnt >> 2) + 1 + 255) / 256, cap = (int64_t)qpn_num_cus() * 8;
    const int nb = (int)(want < cap ? want : cap);
    hipLaunchKernelGGL(k_grad_accum, dim3(nb), dim3(256), 0, stream, acc, g, cnt, first ? 1 : 0, status, adam_reports(status, h_status, h_loss, d_loss));
    qpn_prof_mark(PG_ADAM, stream);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
