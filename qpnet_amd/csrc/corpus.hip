// corpus.hip -- cut one training batch out of a device-resident corpus (qpn_cut_chunks; what the reference's generator, src/bin/qpnet_train.py:200-335,
// assembles on the host for every step).  The corpus never changes and a chunk is a window into it, so the encoded samples, the scaled features and the
// dilated factors live on the device and the host sends a few dozen bytes per chunk: the segment table (corpus_segs.h).
//
// ONE launch writes every output element exactly once; the grid is sized from the data and its blocks are of three kinds, told apart by blockIdx.x:
//   [0, n_seq)            x, t, d.  All three are contiguous (B x T), so a block walks the FLAT index g = b T + s: a thread owns four consecutive elements
//                         and writes them with 16-byte stores (x, t: two each; d: one), whatever T is.  The int16 loads behind them start at an arbitrary
//                         arena offset and cannot be aligned to the stores: they are 2-byte loads that the cache lines absorb.
//   [n_seq, n_seq + n_tr) h.  A 32-frame x 32-feature tile goes through LDS: the arena side is read along the feature axis (128 contiguous bytes per
//                         frame), the output side is written along the frame axis (128 contiguous bytes per feature): neither is a strided 4-byte access.
//   the rest              w (when asked for): flat over (B x bl), four elements and one 16-byte store per thread.
// The table was checked on the host (corpus_segs_check) before the launch: no index computed here can leave an arena, and there is no status word.
#include "qpn_common.h"
#include "corpus_segs.h"

#define CUT_THREADS 256
#define CUT_PER_THREAD 4
#define CUT_TILE 32

static_assert(sizeof(qpn_corpus_seg) == 32, "one 32-byte record per segment");

struct CutParams {
    const int16_t* samples; const float* feats; const float* factors;
    const qpn_corpus_seg* segs; const int32_t* row_first;
    int64_t* x; int64_t* t; float* h; float* d; float* w;
    int B, frames, U, n_aux, bl, T;
    float unvoiced_weight;
    unsigned n_seq, n_tr, tiles_f, tiles_a;      // blocks of the first two kinds; feature-tile grid of a row
};

// arena index of sample s (0 <= s <= T) of row b: the row's segments are few (one per utterance the chunk touches), a linear walk
__device__ __forceinline__ int64_t cut_sample_at(const CutParams& p, int b, int s, int64_t* factor_at) {
    int k = p.row_first[b];
    const int end = p.row_first[b + 1] - 1;          // (the last segment needs no test: the row's sums were checked)
    int n = p.segs[k].n_samples;
    while (k < end && s >= n) { s -= n; n = p.segs[++k].n_samples; }
    if (factor_at) *factor_at = p.segs[k].factor0 + s / p.U;
    return p.segs[k].sample0 + s;
}
// arena feature row of frame j (0 <= j < frames) of row b
__device__ __forceinline__ int64_t cut_frame_at(const CutParams& p, int b, int j) {
    int k = p.row_first[b];
    const int end = p.row_first[b + 1] - 1;
    int n = p.segs[k].n_frames;
    while (k < end && j >= n) { j -= n; n = p.segs[++k].n_frames; }
    return p.segs[k].frame0 + j;
}

__global__ __launch_bounds__(CUT_THREADS) void k_cut_chunks(const CutParams p) {
    __shared__ float tile[CUT_TILE][CUT_TILE + 1];
    const unsigned blk = blockIdx.x, tid = threadIdx.x;
    if (blk < p.n_seq) {
        const int64_t total = (int64_t)p.B * p.T;
        const int64_t g0 = ((int64_t)blk * CUT_THREADS + tid) * CUT_PER_THREAD;
        if (g0 >= total) return;
        const int b = (int)(g0 / p.T), s = (int)(g0 - (int64_t)b * p.T);
        if (total - g0 >= CUT_PER_THREAD && s + CUT_PER_THREAD <= p.T) {
            // the thread's four lie in one row: five samples (the row holds T + 1: s + 4 <= T is one of them), four factors, five 16-byte stores
            int64_t xs[CUT_PER_THREAD + 1]; float ds[CUT_PER_THREAD];
#pragma unroll
            for (int i = 0; i <= CUT_PER_THREAD; ++i) {
                int64_t fa;
                xs[i] = p.samples[cut_sample_at(p, b, s + i, &fa)];
                if (i < CUT_PER_THREAD) ds[i] = p.factors[fa];
            }
            *(longlong2*)(p.x + g0) = make_longlong2(xs[0], xs[1]); *(longlong2*)(p.x + g0 + 2) = make_longlong2(xs[2], xs[3]);
            *(longlong2*)(p.t + g0) = make_longlong2(xs[1], xs[2]); *(longlong2*)(p.t + g0 + 2) = make_longlong2(xs[3], xs[4]);
            *(float4*)(p.d + g0) = make_float4(ds[0], ds[1], ds[2], ds[3]);
        } else {
            // the four straddle two rows (at most B - 1 threads of a batch), or are the batch's tail: element by element
            for (int64_t g = g0; g < total && g < g0 + CUT_PER_THREAD; ++g) {
                const int bb = (int)(g / p.T), ss = (int)(g - (int64_t)bb * p.T);
                int64_t fa;
                p.x[g] = p.samples[cut_sample_at(p, bb, ss, &fa)];
                p.d[g] = p.factors[fa];
                p.t[g] = p.samples[cut_sample_at(p, bb, ss + 1, nullptr)];
            }
        }
    } else if (blk < p.n_seq + p.n_tr) {
        unsigned r = blk - p.n_seq;
        const unsigned ta = r % p.tiles_a; r /= p.tiles_a;
        const unsigned tf = r % p.tiles_f;
        const int b = (int)(r / p.tiles_f);
        const int tx = tid & (CUT_TILE - 1), ty = tid / CUT_TILE;      // 32 x 8
        const int j0 = (int)tf * CUT_TILE, a0 = (int)ta * CUT_TILE;
        for (int k = ty; k < CUT_TILE; k += CUT_THREADS / CUT_TILE) {
            const int j = j0 + k, a = a0 + tx;
            if (j < p.frames && a < p.n_aux) tile[k][tx] = p.feats[cut_frame_at(p, b, j) * p.n_aux + a];
        }
        __syncthreads();
        for (int k = ty; k < CUT_TILE; k += CUT_THREADS / CUT_TILE) {
            const int a = a0 + k, j = j0 + tx;
            if (a < p.n_aux && j < p.frames) p.h[((int64_t)b * p.n_aux + a) * p.frames + j] = tile[tx][k];
        }
    } else {
        const int64_t total = (int64_t)p.B * p.bl;
        const int64_t g0 = ((int64_t)(blk - p.n_seq - p.n_tr) * CUT_THREADS + tid) * CUT_PER_THREAD;
        if (g0 >= total) return;
        const int n = total - g0 < CUT_PER_THREAD ? (int)(total - g0) : CUT_PER_THREAD;
        int b = (int)(g0 / p.bl), i0 = (int)(g0 - (int64_t)b * p.bl);
        float ws[CUT_PER_THREAD];
        for (int i = 0; i < n; ++i) {
            const int pos = p.T - p.bl + i0;
            ws[i] = p.feats[cut_frame_at(p, b, pos / p.U) * p.n_aux] > 0.5f ? 1.0f : p.unvoiced_weight;
            if (++i0 == p.bl) { i0 = 0; ++b; }
        }
        if (n == CUT_PER_THREAD) *(float4*)(p.w + g0) = make_float4(ws[0], ws[1], ws[2], ws[3]);
        else for (int i = 0; i < n; ++i) p.w[g0 + i] = ws[i];
    }
}

extern "C" int qpn_cut_chunks(const int16_t* d_samples, int64_t n_samples, const float* d_feats, const float* d_factors, int64_t n_frames, int n_aux,
                              const qpn_corpus_seg* h_segs, const int32_t* h_row_first, const qpn_corpus_seg* d_segs, const int32_t* d_row_first, int64_t n_segs,
                              int B, int frames, int U, int bl, float unvoiced_weight,
                              int64_t* d_x, int64_t* d_t, float* d_h, float* d_d, float* d_w, void* stream_) {
    if (!d_samples) { qpn_set_error("d_samples is NULL"); return QPN_EINVAL; }
    if (!d_feats) { qpn_set_error("d_feats is NULL"); return QPN_EINVAL; }
    if (!d_factors) { qpn_set_error("d_factors is NULL"); return QPN_EINVAL; }
    if (!h_segs || !h_row_first) { qpn_set_error("the host copy of the segment table is NULL"); return QPN_EINVAL; }
    if (!d_segs || !d_row_first) { qpn_set_error("the device copy of the segment table is NULL"); return QPN_EINVAL; }
    if (!d_x || !d_t || !d_h || !d_d) { qpn_set_error("an output pointer (d_x, d_t, d_h, d_d) is NULL"); return QPN_EINVAL; }
    if (((uintptr_t)d_x | (uintptr_t)d_t | (uintptr_t)d_d | (uintptr_t)d_w) & 15) { qpn_set_error("d_x, d_t, d_d and d_w must be 16-byte aligned"); return QPN_EINVAL; }
    if (d_w && !(unvoiced_weight >= 0.0f && unvoiced_weight <= 3.402823466e38f)) { qpn_set_error("unvoiced_weight must be finite and >= 0 (got %g)", (double)unvoiced_weight); return QPN_EINVAL; }
    CorpusSegsIn in;
    in.n_samples = n_samples; in.n_frames = n_frames; in.n_segs = n_segs; in.B = B; in.frames = frames; in.U = U; in.n_aux = n_aux; in.bl = bl;
    char msg[256];
    int rc = corpus_segs_check(in, h_segs, h_row_first, msg, sizeof(msg));
    if (rc) { qpn_set_error("%s", msg); return rc; }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { qpn_set_error("no HIP device: libqpnet_hip has no CPU fallback"); return QPN_ENODEV; }
    CutParams p;
    p.samples = d_samples; p.feats = d_feats; p.factors = d_factors; p.segs = d_segs; p.row_first = d_row_first;
    p.x = d_x; p.t = d_t; p.h = d_h; p.d = d_d; p.w = d_w;
    p.B = B; p.frames = frames; p.U = U; p.n_aux = n_aux; p.bl = bl; p.T = frames * U; p.unvoiced_weight = unvoiced_weight;
    const int64_t per_block = (int64_t)CUT_THREADS * CUT_PER_THREAD;
    p.tiles_f = (unsigned)((frames + CUT_TILE - 1) / CUT_TILE); p.tiles_a = (unsigned)((n_aux + CUT_TILE - 1) / CUT_TILE);
    const int64_t n_seq = ((int64_t)B * p.T + per_block - 1) / per_block, n_tr = (int64_t)B * p.tiles_f * p.tiles_a;
    const int64_t n_w = d_w ? ((int64_t)B * bl + per_block - 1) / per_block : 0;
    if (n_seq + n_tr + n_w >= ((int64_t)1 << 31)) { qpn_set_error("the batch needs %lld workgroups, more than one launch holds", (long long)(n_seq + n_tr + n_w)); return QPN_EINVAL; }
    p.n_seq = (unsigned)n_seq; p.n_tr = (unsigned)n_tr;
    hipLaunchKernelGGL(k_cut_chunks, dim3((unsigned)(n_seq + n_tr + n_w)), dim3(CUT_THREADS), 0, (hipStream_t)stream_, p);
    QPN_HIP(hipGetLastError());
    return QPN_OK;
}
