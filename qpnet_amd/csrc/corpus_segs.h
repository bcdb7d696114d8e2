// corpus_segs.h -- the segment table of qpn_cut_chunks and its check.  Pure host arithmetic (plain C++: no HIP, no handle, no globals): corpus.hip runs the
// check on the host copy of a table before it launches anything, and tests/corpus_segs_sweep.cpp runs it on a CPU under the host sanitizers.
//
// A batch has B rows; row b is the concatenation of the segments row_first[b] .. row_first[b + 1] - 1, each a window into the corpus arenas.  A row covers
// T + 1 = frames * U + 1 samples (the inputs [0, T) and the targets [1, T + 1)) and exactly `frames` feature rows.  A segment may take samples and no
// feature row: the chunk's last sample is the first sample of the NEXT frame, often of the next utterance.
#pragma once
#include <cstdint>
#include <cstdio>
#include "../../include/qpnet_hip.h"      // qpn_corpus_seg, the QPN_E* codes (declarations only)

struct CorpusSegsIn {
    int64_t n_samples, n_frames;          // arena sizes: int16 samples; rows of the feature arena = entries of the factor arena
    int64_t n_segs;                       // entries of the table
    int B, frames, U, n_aux, bl;
};

// QPN_OK, or QPN_EINVAL / QPN_ERANGE with a message in msg[cap] that names the argument, or the row and the segment.  QPN_ERANGE is kept for the one thing the
// kernel could not survive: a segment that reaches outside an arena.  Everything else that is wrong with a table is QPN_EINVAL.
static inline int corpus_segs_check(const CorpusSegsIn& in, const qpn_corpus_seg* segs, const int32_t* row_first, char* msg, size_t cap) {
#define CS_FAIL(code, ...) do { if (msg && cap) snprintf(msg, cap, __VA_ARGS__); return (code); } while (0)
    if (in.B < 1) CS_FAIL(QPN_EINVAL, "B must be >= 1 (got %d)", in.B);
    if (in.U < 1) CS_FAIL(QPN_EINVAL, "U must be >= 1 (got %d)", in.U);
    if (in.n_aux < 1) CS_FAIL(QPN_EINVAL, "n_aux must be >= 1 (got %d)", in.n_aux);
    if (in.frames < 1) CS_FAIL(QPN_EINVAL, "frames must be >= 1 (got %d)", in.frames);
    const int64_t T = (int64_t)in.frames * in.U;
    if (T >= ((int64_t)1 << 31) - 1) CS_FAIL(QPN_EINVAL, "frames * U must be below 2^31 - 1 (got %lld)", (long long)T);
    if ((int64_t)in.B * T >= ((int64_t)1 << 40) || (int64_t)in.B * in.frames * in.n_aux >= ((int64_t)1 << 40))
        CS_FAIL(QPN_EINVAL, "the batch is too large (B = %d, frames * U = %lld, n_aux = %d)", in.B, (long long)T, in.n_aux);
    if (in.bl < 1 || in.bl > T) CS_FAIL(QPN_EINVAL, "bl must lie in 1..frames * U = %lld (got %d)", (long long)T, in.bl);
    if (in.n_samples < 0 || in.n_frames < 0) CS_FAIL(QPN_EINVAL, "arena sizes must be >= 0 (got %lld samples, %lld frames)", (long long)in.n_samples, (long long)in.n_frames);
    if (!segs || !row_first) CS_FAIL(QPN_EINVAL, "the segment table is NULL");
    if (in.n_segs < 1 || in.n_segs > INT32_MAX) CS_FAIL(QPN_EINVAL, "n_segs must lie in 1..2^31 - 1 (got %lld)", (long long)in.n_segs);
    if (row_first[0] != 0) CS_FAIL(QPN_EINVAL, "row_first[0] must be 0 (got %d)", (int)row_first[0]);
    for (int b = 0; b < in.B; ++b)
        if (row_first[b + 1] < row_first[b]) CS_FAIL(QPN_EINVAL, "row_first is not monotone at row %d (%d after %d)", b, (int)row_first[b + 1], (int)row_first[b]);
    if (row_first[in.B] != in.n_segs) CS_FAIL(QPN_EINVAL, "row_first[B] must equal n_segs = %lld (got %d)", (long long)in.n_segs, (int)row_first[in.B]);
    for (int b = 0; b < in.B; ++b) {
        int64_t ns = 0, nf = 0;
        for (int32_t k = row_first[b]; k < row_first[b + 1]; ++k) {
            const qpn_corpus_seg& s = segs[k];
            const int j = (int)(k - row_first[b]);
            if (s.n_samples < 0 || s.n_frames < 0) CS_FAIL(QPN_EINVAL, "row %d segment %d: counts must be >= 0 (got %d samples, %d frames)", b, j, (int)s.n_samples, (int)s.n_frames);
            // (the counts are below 2^31 and the arena sizes are int64: none of the sums below can wrap once the starts are known to be in range)
            if (s.sample0 < 0 || s.sample0 > in.n_samples || s.n_samples > in.n_samples - s.sample0)
                CS_FAIL(QPN_ERANGE, "row %d segment %d: samples [%lld, +%d) leave the arena of %lld", b, j, (long long)s.sample0, (int)s.n_samples, (long long)in.n_samples);
            if (s.frame0 < 0 || s.frame0 > in.n_frames || s.n_frames > in.n_frames - s.frame0)
                CS_FAIL(QPN_ERANGE, "row %d segment %d: feature rows [%lld, +%d) leave the arena of %lld", b, j, (long long)s.frame0, (int)s.n_frames, (long long)in.n_frames);
            const int64_t nfd = ((int64_t)s.n_samples + in.U - 1) / in.U;      // frames whose factors the segment's samples repeat
            if (s.factor0 < 0 || s.factor0 > in.n_frames || nfd > in.n_frames - s.factor0)
                CS_FAIL(QPN_ERANGE, "row %d segment %d: factors [%lld, +%lld) leave the arena of %lld", b, j, (long long)s.factor0, (long long)nfd, (long long)in.n_frames);
            ns += s.n_samples; nf += s.n_frames;
        }
        if (ns != T + 1) CS_FAIL(QPN_EINVAL, "row %d: its segments hold %lld samples, frames * U + 1 = %lld expected", b, (long long)ns, (long long)(T + 1));
        if (nf != in.frames) CS_FAIL(QPN_EINVAL, "row %d: its segments hold %lld feature rows, frames = %d expected", b, (long long)nf, in.frames);
    }
#undef CS_FAIL
    return QPN_OK;
}
