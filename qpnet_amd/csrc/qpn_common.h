// qpn_common.h -- internal definitions shared by the HIP translation units of libqpnet_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/qpnet_hip.h"
#include "qpn_geom.h"             // LayerGeom / Geom / QPN_MAX_LAYERS / qpn_build_geom / qpn_pad_k, and the declaration of qpn_set_error
#include "decode_program.h"       // QPN_NW / QPN_NT, the OP_ / TF_ constants, Task / RingDesc / FastParams / BiasDesc, and the planner of the decode program

// ---------------------------------------------------------------- error plumbing
#define QPN_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            qpn_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorOutOfMemory ? QPN_ENOMEM : QPN_ENODEV;                    \
        }                                                                                  \
    } while (0)

// ---------------------------------------------------------------- decode program
#define QPN_MODE_SAMPLING_CTL 2   // DecodeParams.mode only, never an ABI value: QPN_MODE_SAMPLING with a sampling control set (qpn_decode_sampling / _ex: any of the four)
#define QPN_MODE_SAMPLING_ROW 3   // DecodeParams.mode only, never an ABI value: QPN_MODE_SAMPLING with per-row records set (qpn_decode_row_sampling): the pick takes its key and its
                                  // five values from DecodeParams.row_draw[UttDesc.row] instead of from DecodeParams
#define QPN_MODE_SAMPLING_TRACK 4 // DecodeParams.mode only, never an ABI value: QPN_MODE_SAMPLING with a draw track set (qpn_decode_frame_sampling): key and counter word from
                                  // DecodeParams.row_draw[UttDesc.row] as above (the host fills in {call seed, row} where the call has no records), the four values from the
                                  // record of the step's feature frame, DecodeParams.frame_draw[UttDesc.row * n_frames + f]
struct FrameDraw {          // one (batch row, feature frame) record of a draw track as the kernels read it (16 bytes); the host forms 1 / temperature and folds top_k
    float inv_temp; int top_k; float top_p, min_p;
};
static_assert(sizeof(FrameDraw) == 16, "one 16-byte record per frame");
struct RowDraw {            // one batch row's record as the kernels read it (32 bytes: one scalar load), indexed by UttDesc.row; the host forms 1 / temperature and folds top_k
    unsigned seed_lo, seed_hi, stream;      // Philox key, and the counter word that a uniform call fills with the batch row
    float inv_temp; int top_k; float top_p, min_p;
    int pad_;
};
static_assert(sizeof(RowDraw) == 32, "one 32-byte record per row");
struct UttDesc {            // offsets into the base pointers of DecodeParams (kernel-argument pointers keep
                            // the GLOBAL address space; pointers loaded from memory would become FLAT accesses)
    int64_t pproj;          // floats: [F][L][2C] per-frame aux projections
    int64_t dfac;           // elements: dilated factors row (double or float)
    int64_t known;          // ints: [n0] padded known prefix (sample ids)
    int64_t teacher;        // int64s: optional [n_samples], -1 = none
    int64_t out;            // int64s: [n_samples]
    int64_t logits;         // floats: optional [n_samples][Q], -1 = none
    int64_t ring;           // floats: ring block of this utterance (zeroed before launch)
    int n_pad, n0, n_samples, d_is_f32;
    int64_t F;
    int row, pad_;          // row of the caller's batch (the descriptors of a launch are a permuted slice of the batch): Philox key
};

// cooperative decode (decode_coop.hip): G workgroups per utterance, each owning 1/G of every layer's output rows; full
// vectors are exchanged through 8-byte {tag, value} granules in global memory (tag = step + 1, zeroed before every launch)
struct CoopParams {
    unsigned long long* xch;          // exchange memory
    long utt_stride;                  // granules per utterance
    int o_ring[QPN_MAX_LAYERS];       // granule offsets inside an utterance block: layer-input history [len_l][C]
    int o_g, o_y1, o_y2, o_lg;        // gate vectors [L][C], relu(skip total) [S], post-1 output [S], logits [Q]
    int* abort;                       // set when a wait timed out: every workgroup drains instead of spinning on
    int G, CB, SB, QB, Sp;            // workgroups per utterance; channels / skip rows / logit rows per workgroup
    int logR, rpt, logRs, rpts;       // lanes per row (log2) and rows per 4 KiB tile for K = C and K = S
    int w_past_il[QPN_MAX_LAYERS];    // float4 offsets of the past-tap tiles with (sigma_c, tanh_c) rows interleaved
    int f_resb[QPN_MAX_LAYERS], f_skipb[QPN_MAX_LAYERS], f_p1b, f_p2b;   // flat offsets of the biases the epilogues add
};

struct DecodeParams {
    const float4* wpk;
    const float* flat;
    const float* qb;        // [L][2C]
    const Task* tasks;
    const UttDesc* utts;
    const float* pproj; const void* dfac; const int* known; const int64_t* teacher; int64_t* out; float* logits; float* ring;
    int* status;
    long long* stamps;      // dev aid (QPN_STAMPS=1): s_memtime stamps of one step, [stamp][wave]
    int n_slots;
    int C, Cp, S, Q, L, U, mode;
    int64_t causal_w, causal_b, up_w;
    int o_xbuf, o_xp, o_pd, o_auxv, o_g, o_skf, o_ska, o_y1, o_y2, o_lg, o_samp, o_sel, state_floats;
    int o_bias, n_bias, o_tasks, lds_floats;
    int o_gl;               // specialised kernel: per-layer gate vectors [L][Cp]
    int o_stamp;            // dev stamps: first LDS float behind everything the launched kernel uses
    int o_wres;             // specialised kernel: residual-1x1 tiles of layers 0..L-2 resident in LDS (float offset, 16-byte aligned)
    const int* bias_src;    // [n_bias] flat indices of the biases mirrored in LDS
    unsigned long long seed;
    float inv_temp; int top_k;   // sampling controls (qpn_decode_sampling): 1 / temperature and the top-k cut, 1.0f / 0 = off (sample_wave_ctl, decode_dev.h)
    float top_p, min_p;          // ... and the nucleus and relative-probability cuts (qpn_decode_sampling_ex), 1.0f / 0.0f = off (nucleus_cut, decode_dev.h)
    RingDesc rings[QPN_MAX_LAYERS];
    // live output (qpn_decode_live), all null / 0 when it is not armed.  Host-coherent pinned memory that the host reads WHILE the launch runs:
    int32_t* live;          // mirror of `out` ([B][max_n], the element offsets of UttDesc.out)
    long long* live_done;   // [B], indexed by UttDesc.row: samples of that row that are final in the mirror
    int live_every;         // a row publishes its count after every live_every samples, and after its last one
    const int* cancel;      // the host's stop request (qpn_decode_cancel): one word, non-zero once the caller asked; read at publish points and at a row's start
    const RowDraw* row_draw;   // per-row sampling records (qpn_decode_row_sampling), [B] indexed by UttDesc.row; null unless mode == QPN_MODE_SAMPLING_ROW.  Loaded once when a workgroup takes a row
    const FrameDraw* frame_draw;   // draw track (qpn_decode_frame_sampling), [B][n_frames] with rows indexed by UttDesc.row; null unless mode == QPN_MODE_SAMPLING_TRACK.  One record per step,
    int64_t n_frames;              // fetched a step ahead of the pick that uses it (stage_frame_draw / frame_draw_word, decode_dev.h)
};
static_assert(sizeof(DecodeParams) == 1104 && offsetof(DecodeParams, n_slots) == 112 && offsetof(DecodeParams, o_xbuf) == 168 && offsetof(DecodeParams, o_gl) == 236 &&
              offsetof(DecodeParams, bias_src) == 248 && offsetof(DecodeParams, rings) == 280 && offsetof(DecodeParams, live) == 1048, "kernel argument layout");
