// train_input_grad.hip -- gradient of the training loss with respect to the auxiliary features h (qpn_train_input_grad).
//
// The layer backward already leaves everything this needs in the workspace; three small kernels contract it, one per way the
// forward consumed h.  Each writes EVERY element of dh[B][A][F] (exact zeros where no row of the chunk reaches), sums in a fixed order and uses
// no atomics; padding columns a >= A of the sources are never read into a result.
//   k_dh_frames  aux hoist (frame-rate aux 1x1): dh[b][a][f] = sum_l sum_{n < 2C} Va_l[n][a] D_l[b][f - ffirst][n]      (D = TrainBwd::DPA)
//   k_dh_up      every other path, U > 0:        dh[b][a][f] = sum_j w_up[j] dH[b][U f + j - q0][a], rows in [0, N1)     (dH = TrainBwd::DHUP, q0 = F U - N1)
//   k_dh_copy    upsampling_factor = 0:          dh[b][a][f] = dH[b][f - (F - N1)][a], the leading F - N1 columns zero
#include <hip/hip_runtime.h>
#include "train_common.h"

#define DH_FT 4              // frames per workgroup of k_dh_frames: one per wave (the contraction is latency-bound: many short workgroups, see the kernel)
#define DH_LDD 132           // leading dimension of its D tile (128 gate rows + 4)

struct DhFramesArgs { AuxArgs a; float* dh; };

// One workgroup per (tile of DH_FT frames counted from frame 0, batch item); 256 threads: wave fs owns frame fs of the tile, lane a the feature a (A <= 64 on
// this path).  Per layer: Va_l ([2C][A], 2C = 128, in the parameters' own layout: the two halves are contiguous runs of C A floats) and the tile's D rows
// (contiguous 2C floats each: coalesced float4 loads) are staged in LDS, then 128 FMAs per thread, layers and gate rows in ascending order -- the D operand is a
// broadcast read, the Va operand a conflict-free row.  [16 frames x 4 features per thread gave 12 workgroups on the paper-size bench chunk: 38 us next to the
// weight-gradient launches that own the register file; four frames per workgroup spreads the same 15 MFLOP over four times as many CUs.]
// The NEXT layer's operands are requested into registers before a layer's FMAs and stored behind them: written as "load, store, compute" every layer exposed
// a chain of memory round trips (ten dependent load -> LDS store pairs: 55 us for 15 MFLOP).  The results leave through an LDS transpose: h is (B, A, F)
// with f fastest, so a feature's frames are one run.
#define DH_VK 16             // Va elements per thread and half: ceil(64 * 64 / 256)
__global__ __launch_bounds__(256) void k_dh_frames(DhFramesArgs q) {
    __shared__ float Vs[128 * 64];
    __shared__ float Ds[DH_FT * DH_LDD];
    const AuxArgs& p = q.a;
    const int A = p.A, F = p.F, C = p.C, tid = threadIdx.x;
    const int f0 = blockIdx.x * DH_FT, b = blockIdx.y;
    float* out = q.dh + (size_t)b * A * F;
    if (f0 + DH_FT <= p.ffirst) {                          // the whole tile lies in front of the chunk: zeros
        for (int i = tid; i < A * DH_FT; i += 256) { const int a = i / DH_FT, f = f0 + i % DH_FT; if (f < F) out[(size_t)a * F + f] = 0.f; }
        return;
    }
    const int fs = tid >> 6, a = tid & 63, CA = C * A;
    float rs[DH_VK], rt[DH_VK];
    float4 rd = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int l) {                            // layer l's operands -> registers (all loads issued together)
        const float* vs = p.flat + p.g.auxS[l];
        const float* vt = p.flat + p.g.auxT[l];
#pragma unroll
        for (int k = 0; k < DH_VK; ++k) { const int i = tid + 256 * k; rs[k] = i < CA ? vs[i] : 0.f; rt[k] = i < CA ? vt[i] : 0.f; }
        const float* D = p.DPA + (size_t)(l * p.B + b) * (p.nfr + 1) * 2 * C;
        if (tid < DH_FT * 32) {                            // 32 float4 per row of 2C = 128 floats, DH_FT rows
            const int r = tid >> 5, c4 = tid & 31, f = f0 + r;
            rd = (f >= p.ffirst && f < F) ? *(const float4*)(D + (size_t)(f - p.ffirst) * 2 * C + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float acc = 0.f;
    request(0);
    for (int l = 0; l < p.L; ++l) {
        __syncthreads();                                   // the previous layer's FMAs have read their operands
#pragma unroll
        for (int k = 0; k < DH_VK; ++k) { const int i = tid + 256 * k; if (i < CA) { Vs[i] = rs[k]; Vs[CA + i] = rt[k]; } }
        if (tid < DH_FT * 32) *(float4*)(Ds + (tid >> 5) * DH_LDD + 4 * (tid & 31)) = rd;
        __syncthreads();
        if (l + 1 < p.L) request(l + 1);
        const float* dr = Ds + fs * DH_LDD;
        const float* vb = Vs + a;                          // Vs[n * A + a]; lanes a >= A read the next row's (or stale) words: never stored
#pragma unroll 8
        for (int n = 0; n < 128; n += 4) {
            const float4 d = *(const float4*)(dr + n);
            const float* v = vb + n * A;
            acc = fmaf(d.x, v[0], acc);
            acc = fmaf(d.y, v[A], acc);
            acc = fmaf(d.z, v[2 * A], acc);
            acc = fmaf(d.w, v[3 * A], acc);
        }
    }
    __syncthreads();
    float* Os = Ds;                                        // [64][DH_FT + 1]
    Os[a * (DH_FT + 1) + fs] = acc;
    __syncthreads();
    for (int i = tid; i < A * DH_FT; i += 256) {
        const int a = i / DH_FT, r = i % DH_FT, f = f0 + r;
        if (f < F) out[(size_t)a * F + f] = f >= p.ffirst ? Os[a * (DH_FT + 1) + r] : 0.f;
    }
}

struct DhUpArgs { const float* flat; const float* DHUP; float* dh; int64_t up_w; int U, Ap, A, F, N1; };

// One workgroup per (frame, batch item), as k_up_bwd; 256 threads: lane = feature within a pass of 64, the four waves take the frame's samples j = w, w + 4, ...
// (a row's Ap floats are contiguous: a wave reads one run per sample, eight samples requested together).  The four partial sums meet in LDS and are added in
// wave order.  Any Ap: features in passes of 64, no second sweep over the rows is needed beyond that.
__global__ __launch_bounds__(256) void k_dh_up(DhUpArgs p) {
    __shared__ float part[4][64];
    const int U = p.U, Ap = p.Ap, A = p.A, F = p.F, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x, b = blockIdx.y;
    const int64_t q0 = (int64_t)F * U - p.N1;              // h_up sample index of row 0
    const int64_t nb = (int64_t)f * U - q0;                // local row of the frame's sample 0 (negative: in front of the chunk)
    const float* w = p.flat + p.up_w;
    const float* rows = p.DHUP + (size_t)b * p.N1 * Ap;
    for (int a0 = 0; a0 < A; a0 += 64) {
        const int a = a0 + lane;
        const bool live = a < A;
        float acc = 0.f;
        int jlo = nb < 0 ? (int)(-nb) : 0;                 // first sample of the frame inside the chunk (rows past N1 - 1 do not exist: U f + j < F U)
        jlo += (wave - jlo % 4 + 4) % 4;                   // ... that belongs to this wave
        int j = jlo;
        for (; j + 28 < U; j += 32) {
            float v[8], wj[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] = live ? rows[(size_t)(nb + j + 4 * k) * Ap + a] : 0.f; wj[k] = w[j + 4 * k]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fmaf(wj[k], v[k], acc);
        }
        for (; j < U; j += 4) acc = fmaf(w[j], live ? rows[(size_t)(nb + j) * Ap + a] : 0.f, acc);
        __syncthreads();
        part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && live) p.dh[((size_t)b * A + a) * F + f] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    }
}

struct DhCopyArgs { const float* DHUP; float* dh; int Ap, A, F, N1; };

// upsampling_factor = 0: dH is dh already, time-major and aligned at the end of h.  A 32 x 32 transpose through LDS: reads run along the features of a row,
// writes along the frames of a feature.  grid (frames / 32, features / 32, batch items), 32 x 8 threads.
__global__ __launch_bounds__(256) void k_dh_copy(DhCopyArgs p) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y, b = blockIdx.z;
    const int f0 = blockIdx.x * 32, a0 = blockIdx.y * 32, lead = p.F - p.N1;      // columns in front of the chunk's rows
    for (int k = ty; k < 32; k += 8) {
        const int f = f0 + k, a = a0 + tx;
        tile[k][tx] = (f >= lead && f < p.F && a < p.A) ? p.DHUP[((size_t)b * p.N1 + (f - lead)) * p.Ap + a] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int a = a0 + k, f = f0 + tx;
        if (a < p.A && f < p.F) p.dh[((size_t)b * p.A + a) * p.F + f] = tile[tx][k];
    }
}

// after the layer backward of `bw`, on a stream ordered behind it; ag: the hoist path's geometry (not looked at otherwise)
void qpn_launch_input_grad(const TrainParams& p, const TrainBwd& bw, const AuxGeom* ag, hipStream_t st) {
    if (!bw.dh) return;
    if (p.hoist && ag) {
        DhFramesArgs q; q.a = tr_aux_args(p, &bw, *ag); q.dh = bw.dh;
        hipLaunchKernelGGL(k_dh_frames, dim3((p.F + DH_FT - 1) / DH_FT, p.B), dim3(256), 0, st, q);
    } else if (p.U > 0) {
        DhUpArgs u; u.flat = p.flat; u.DHUP = bw.DHUP; u.dh = bw.dh; u.up_w = p.up_w; u.U = p.U; u.Ap = p.Ap; u.A = p.A; u.F = p.F; u.N1 = p.N1;
        hipLaunchKernelGGL(k_dh_up, dim3(p.F, p.B), dim3(256), 0, st, u);
    } else {
        DhCopyArgs c; c.DHUP = bw.DHUP; c.dh = bw.dh; c.Ap = p.Ap; c.A = p.A; c.F = p.F; c.N1 = p.N1;
        hipLaunchKernelGGL(k_dh_copy, dim3((p.F + 31) / 32, (p.A + 31) / 32, p.B), dim3(32, 8), 0, st, c);
    }
}
