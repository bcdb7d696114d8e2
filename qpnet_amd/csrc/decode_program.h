// decode_program.h -- the decode program of a handle: the LDS layout of the one-CU kernels, the gather map of the packed weights for every kernel family, the
// interpreter's task table, the tile map of the straight-line kernel and every offset the launchers hand to a kernel.  Pure host arithmetic (plain C++: no HIP,
// no handle, no globals): qpn_create keeps what decode_program() returns, qpn_set_weights uploads its lists; tests/decode_program_sweep.cpp decodes the map
// back through the packers' position formulas on a CPU.  Every flat index comes from the tp_*_src functions of qpn_geom.h, which the training planner packs
// and reduces gradients through as well.
#pragma once
#include "qpn_geom.h"
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#define QPN_NW 16                 // waves per decode workgroup
#define QPN_NT (QPN_NW * 64)

enum {
    OP_NOP = 0, OP_PAST, OP_Z, OP_RES, OP_SKIP, OP_POST1, OP_POST2, OP_CAUSAL, OP_ARGMAX, OP_STAGE
};
#define TF_BARRIER 0x100      // workgroup barrier before this task
#define TF_DRAIN   0x200      // ... and drain this wave's global stores first
#define TF_LAST    0x400      // OP_SKIP of the last layer: also emit relu(skip total)
#define TF_HASW    0x800      // task consumes a weight tile (prefetchable)

struct Task {          // 32 bytes, wave-uniform; the table is copied to LDS at kernel start
    int op;            // opcode | flags | (log2 R << 16)
    int woff4;         // float4 offset of the weight tile in the packed buffer
    int xoff;          // LDS float offset of the input vector
    int row0;          // first row of the tile (in the matrix' packed row order)
    int a, b, c, d;    // op specific
};

struct RingDesc { int base; int len; int mult; int adaptive; };   // base: float offset in the utterance's ring block

// per-layer tile / bias locations for the specialised straight-line decode kernel (k_decode_fast)
struct FastParams {
    int w_cur[QPN_MAX_LAYERS], w_past[QPN_MAX_LAYERS], w_res[QPN_MAX_LAYERS], w_skip[QPN_MAX_LAYERS];   // float4 offsets
    int b_res[QPN_MAX_LAYERS], b_skip[QPN_MAX_LAYERS];                                                   // LDS float offsets
    int adaptive[QPN_MAX_LAYERS];
    int w_p1, w_p2, b_p1, b_p2;
};

struct BiasDesc { int64_t auxb[2], convb[2], convPb[2]; int adaptive; int pad; };      // flat offsets of the biases k_fold_bias folds into a layer's gate bias, per half
static_assert(sizeof(Task) == 32 && sizeof(RingDesc) == 16 && sizeof(FastParams) == (7 * QPN_MAX_LAYERS + 4) * 4 && sizeof(BiasDesc) == 56, "kernel-visible structs");
static_assert(offsetof(FastParams, b_res) == 16 * QPN_MAX_LAYERS && offsetof(FastParams, w_p1) == 28 * QPN_MAX_LAYERS && offsetof(BiasDesc, adaptive) == 48, "kernel-visible structs");

// LDS layout of the one-CU kernels (float offsets, all multiples of 4), in the order the kernels assume: the step state [0, state_floats) (zeroed at start),
// the biases the epilogues add, the task table.  Copied member by member into the DecodeParams template (decode_params_template, decode.hip)
struct DecodeLds {
    int o_xbuf, o_xp, o_pd, o_auxv, o_g, o_skf, o_ska, o_y1, o_y2, o_lg, o_samp, o_sel, o_gl, state_floats;
    int o_bias, n_bias, o_tasks, lds_floats;
};

struct DecodeProgram {
    int rc = QPN_OK;                 // QPN_EINVAL (and err): a geometry the decode kernels refuse (it may still train); nothing else is set then
    char err[160] = "";
    DecodeLds lds = {};
    FastParams fp = {};              // tile map of the specialised kernel
    int n_slots = 0;
    bool single_cu_ok = true;        // the step state fits one CU's LDS (decode.hip kernels); otherwise decode_coop.hip only
    int aux_woff4 = 0, aux_tiles = 0, logRa = 0;      // aux matrices (natural rows) of the frame-rate projection kernels
    int w_past_il[QPN_MAX_LAYERS] = {};               // channel-interleaved past-tap tiles (cooperative and pipelined kernels)
    // batched cooperative kernel (decode_coopb.hip): workgroup w's A-operand fragments are the cb_per_w float4 from cb_base4 + w * cb_per_w of the packed weights;
    // cb_zc.. = float4 offsets of the tiles inside that block; or cb_ok = false
    bool cb_ok = false;
    int cb_zc[QPN_MAX_LAYERS] = {}, cb_zp[QPN_MAX_LAYERS] = {}, cb_rs[QPN_MAX_LAYERS] = {}, cb_p1 = 0, cb_p2 = 0; long long cb_base4 = 0; int cb_per_w = 0;
    BiasDesc bd[QPN_MAX_LAYERS] = {};
    int f_resb[QPN_MAX_LAYERS] = {}, f_skipb[QPN_MAX_LAYERS] = {}, f_p1b = 0, f_p2b = 0;   // flat offsets of the biases the multi-workgroup kernels' epilogues add
    size_t n_map = 0, n_tasks = 0;   // lengths of map and tasks: they outlive the host copies, which qpn_set_weights releases once they are on the device
    std::vector<int> map;            // gather map of the packed tile buffer: packed float i = flat[map[i]], or 0 where map[i] == -1
    std::vector<Task> tasks;         // [n_slots][QPN_NW]
    std::vector<int> bias_src;       // flat indices of the biases mirrored in LDS
};

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// append the tiles of one matrix to the gather map; returns the float4 offset of its first tile.
// src(row, k) -> flat index (k < K) ; rows in PACKED order.
template <class F>
inline int pack_matrix(std::vector<int>& map, int rows, int K, int Kp, F src) {
    const int R = Kp / 16, rpt = 64 / R, tiles = rows / rpt;
    const int off4 = (int)(map.size() / 4);
    map.resize(map.size() + (size_t)tiles * 1024);
    int* m = map.data() + (size_t)off4 * 4;
    for (int t = 0; t < tiles; ++t)
        for (int j = 0; j < 4; ++j)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    int row = t * rpt + lane / R, q = lane % R, k = 16 * q + 4 * j + e;
                    m[((size_t)(t * 4 + j) * 64 + lane) * 4 + e] = k < K ? tp_idx(src(row, k)) : -1;
                }
    return off4;
}

// 16-row tiles as the MFMA's A operand (decode_coopb.hip).  ALL the fragments of one workgroup are contiguous (blocks of `per_w` float4 from `base4`: the
// workgroup streams 1.5 MB per generated sample and should not walk a new page for every matrix); inside a block, the tile at `rel4` holds, per 16-deep
// chunk c, word c * 64 + lane: element e = M[row m = lane & 15][16 c + 4 e + (lane >> 4)].  src(w, m, k) -> flat index, or -1 (a zero: padding rows)
template <class F>
inline void fill_mtiles(std::vector<int>& map, size_t base4, size_t per_w, size_t rel4, int G, int R, F src) {
    for (int w = 0; w < G; ++w) {
        int* mm = map.data() + (base4 + (size_t)w * per_w + rel4) * 4;
        for (int c = 0; c < R; ++c)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e)
                    mm[((size_t)c * 64 + lane) * 4 + e] = tp_idx(src(w, lane & 15, 16 * c + 4 * e + (lane >> 4)));
    }
}

// coopb_supported: qpn_coopb_supported(g) (decode_coopb.hip: that kernel's own limits); the map then opens with its fragment blocks
inline DecodeProgram decode_program(const Geom& g, bool coopb_supported) {
    DecodeProgram d;
    const int C = g.C, S = g.S, Q = g.Q, A = g.A, L = g.L;
    const int Rc = g.Cp / 16, Rs = g.Sp / 16, Ra = g.Ap / 16;
    d.rc = QPN_EINVAL;
    if (Rc > 32 || Rs > 64 || Ra > 64) { snprintf(d.err, sizeof(d.err), "n_resch <= 512, n_skipch/n_aux <= 1024 supported by the decode kernel"); return d; }
    if ((2 * C) % (64 / Rc) || C % (64 / Rc) || S % (64 / Rc) || S % (64 / Rs) || Q % (64 / Rs) || (2 * C) % (64 / Ra)) {
        snprintf(d.err, sizeof(d.err), "channel counts must be multiples of the tile height (n_resch %% %d, n_skipch %% %d, n_quantize %% %d)",
                 64 / Rc, std::max(64 / Rc, 64 / Rs), 64 / Rs);
        return d;
    }
    if (g.n_params >= (int64_t)1 << 31) { snprintf(d.err, sizeof(d.err), "model too large for 32-bit gather map"); return d; }
    d.rc = QPN_OK;
    // ---- LDS layout: step state first ...
    DecodeLds& p = d.lds;
    int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
    p.o_xbuf = take((L + 1) * g.Cp); p.o_xp = take(L * g.Cp); p.o_pd = take(2 * L * 2 * C); p.o_auxv = take(L * 2 * C);
    p.o_g = take(g.Cp); p.o_skf = take(S); p.o_ska = take(S); p.o_y1 = take(g.Sp); p.o_y2 = take(g.Sp); p.o_lg = take(Q);
    p.o_samp = take(4); p.o_sel = take(L); p.o_gl = take(L * g.Cp); p.state_floats = o;
    // ... then the biases the epilogues add (so no global load sits behind the weight prefetch queue)
    std::vector<int>& bsrc = d.bias_src;
    auto bias_block = [&](int64_t flat_off, int n) { int r = p.o_bias + (int)bsrc.size(); for (int i = 0; i < n; ++i) bsrc.push_back(tp_idx(flat_off + i)); return r; };
    p.o_bias = o;
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        d.fp.b_res[l] = bias_block(y.resb, C); d.fp.b_skip[l] = bias_block(y.skipb, S); d.fp.adaptive[l] = y.adaptive;
        d.f_resb[l] = tp_idx(y.resb); d.f_skipb[l] = tp_idx(y.skipb);
        BiasDesc& b = d.bd[l];
        for (int half = 0; half < 2; ++half) {      // (a fixed layer has no past-tap conv of its own: convPb stays 0, and k_fold_bias does not read it)
            int64_t f[3] = {0, 0, 0}; tp_gate_bias(y, C, half * C, f);
            b.convb[half] = f[0]; b.auxb[half] = f[1]; b.convPb[half] = f[2];
        }
        b.adaptive = y.adaptive;
    }
    d.fp.b_p1 = bias_block(g.post1_b, S); d.fp.b_p2 = bias_block(g.post2_b, Q);
    d.f_p1b = tp_idx(g.post1_b); d.f_p2b = tp_idx(g.post2_b);
    p.n_bias = (int)bsrc.size();
    o += (p.n_bias + 3) & ~3;

    // ---- packed weight tiles + task list
    std::vector<int>& map = d.map;
    const bool cb_ok = d.cb_ok = coopb_supported;
    const int cbG = C / 8, cbRC = g.Cp / 16, cbRS = g.Sp / 16, SBc = S / cbG, QBc = Q / cbG;      // workgroup w = channels 8 w .. 8 w + 7, SBc skip rows, QBc logit rows
    const size_t cb_per_w = cb_ok ? ((size_t)3 * L * cbRC + 2 * cbRS) * 64 : 0;      // float4 per workgroup: three tiles per layer + the two post-net tiles
    const size_t cb_base4 = 0;
    map.reserve(cb_per_w * cbG * 4 + (size_t)L * ((7 * C + S) * g.Cp + 2 * C * g.Ap) + (size_t)(S + Q) * g.Sp);      // all of it, so that it is faulted in once (DEFAULT: 58 M ints)
    if (cb_ok) {
        map.resize(cb_per_w * cbG * 4, -1);
        d.cb_base4 = (long long)cb_base4; d.cb_per_w = (int)cb_per_w;
    }
    std::vector<std::vector<Task>> phases;
    auto tile_tasks = [&](std::vector<Task>& ph, int op, int off4, int rows, int Kp, int xoff, int a, int b, int c, int dd, int flags) {
        const int R = Kp / 16, rpt = 64 / R, tiles = rows / rpt;
        for (int t = 0; t < tiles; ++t) {
            Task k; k.op = op | TF_HASW | flags | (ilog2(R) << 16); k.woff4 = off4 + t * 256; k.xoff = xoff; k.row0 = t * rpt;
            k.a = a; k.b = b; k.c = c; k.d = dd; ph.push_back(k);
        }
    };
    for (int l = 0; l < L; ++l) {
        const LayerGeom y = g.layers[l];
        auto srcw = [&](int half, int r, int k, int past) { return tp_gate_src(y, C, A, past ? C + k : k, half * C + r); };      // row r of a half's current / past tap
        const int off_past = pack_matrix(map, 2 * C, C, g.Cp, [&](int row, int k) { return srcw(row / C, row % C, k, 1); });
        const int off_cur = pack_matrix(map, 2 * C, C, g.Cp, [&](int row, int k) { return srcw(row & 1, row >> 1, k, 0); });      // (sigma_c, tanh_c) rows together
        d.w_past_il[l] = pack_matrix(map, 2 * C, C, g.Cp, [&](int row, int k) { return srcw(row & 1, row >> 1, k, 1); });
        const int off_res = pack_matrix(map, C, C, g.Cp, [&](int row, int k) { return tp_res_src(y, C, k, row); });
        const int off_skip = pack_matrix(map, S, C, g.Cp, [&](int row, int k) { return tp_skip_src(g, l * C + k, row); });
        if (cb_ok) {      // the batched cooperative kernel's A-operand fragments (decode_coopb.hip): rows m = half * 8 + channel of the gate, 8 residual + SBc skip rows
            d.cb_zc[l] = (3 * l + 0) * cbRC * 64; d.cb_zp[l] = (3 * l + 1) * cbRC * 64; d.cb_rs[l] = (3 * l + 2) * cbRC * 64;      // (relative to the workgroup's block)
            fill_mtiles(map, cb_base4, cb_per_w, d.cb_zc[l], cbG, cbRC, [&](int w, int m, int k) -> int64_t { return k < C ? srcw(m >> 3, 8 * w + (m & 7), k, 0) : -1; });
            fill_mtiles(map, cb_base4, cb_per_w, d.cb_zp[l], cbG, cbRC, [&](int w, int m, int k) -> int64_t { return k < C ? srcw(m >> 3, 8 * w + (m & 7), k, 1) : -1; });
            fill_mtiles(map, cb_base4, cb_per_w, d.cb_rs[l], cbG, cbRC, [&](int w, int m, int k) -> int64_t {
                if (k >= C) return -1;
                if (m < 8) return tp_res_src(y, C, k, 8 * w + m);
                return m - 8 < SBc ? tp_skip_src(g, l * C + k, SBc * w + m - 8) : -1; });
        }
        // Z phase: this step's pre-activations + the NEXT step's past-tap dots of the same layer (the
        // past rows are known one step early, so these tiles fill the waves the z tiles leave idle)
        std::vector<Task> zp, rp;
        d.fp.w_cur[l] = off_cur; d.fp.w_past[l] = off_past; d.fp.w_res[l] = off_res; d.fp.w_skip[l] = off_skip;
        tile_tasks(zp, OP_Z, off_cur, 2 * C, g.Cp, p.o_xbuf + l * g.Cp, l * 2 * C, 0, p.o_g, 0, 0);
        tile_tasks(zp, OP_PAST, off_past, 2 * C, g.Cp, p.o_xp + l * g.Cp, l * 2 * C, p.o_xbuf + l * g.Cp, l, 0, 0);
        tile_tasks(rp, OP_RES, off_res, C, g.Cp, p.o_g, p.o_xbuf + l * g.Cp, d.fp.b_res[l], p.o_xbuf + (l + 1) * g.Cp, l + 1 < L ? l + 1 : -1, 0);
        const bool last = l == L - 1;
        int acc = y.adaptive ? p.o_ska : p.o_skf;
        int other = last ? (y.adaptive ? (g.LF > 0 ? p.o_skf : -1) : -1) : 0;
        tile_tasks(rp, OP_SKIP, off_skip, S, g.Cp, p.o_g, acc, d.fp.b_skip[l], other, p.o_y1, last ? TF_LAST : 0);
        phases.push_back(zp); phases.push_back(rp);
    }
    auto post1 = [&](int row, int k) { return tp_post1_src(g, k, row); };
    auto post2 = [&](int row, int k) { return tp_post2_src(g, k, row); };
    if (cb_ok) {
        d.cb_p1 = 3 * L * cbRC * 64; d.cb_p2 = d.cb_p1 + cbRS * 64;
        fill_mtiles(map, cb_base4, cb_per_w, d.cb_p1, cbG, cbRS, [&](int w, int m, int k) -> int64_t { return (m < SBc && k < S) ? post1(SBc * w + m, k) : -1; });
        fill_mtiles(map, cb_base4, cb_per_w, d.cb_p2, cbG, cbRS, [&](int w, int m, int k) -> int64_t { return (m < QBc && k < S) ? post2(QBc * w + m, k) : -1; });
    }
    d.fp.w_p1 = pack_matrix(map, S, S, g.Sp, post1);
    d.fp.w_p2 = pack_matrix(map, Q, S, g.Sp, post2);
    std::vector<Task> p1, p2, pa;
    tile_tasks(p1, OP_POST1, d.fp.w_p1, S, g.Sp, p.o_y1, 0, d.fp.b_p1, p.o_y2, 0, 0);
    tile_tasks(p2, OP_POST2, d.fp.w_p2, Q, g.Sp, p.o_y2, 0, d.fp.b_p2, p.o_lg, 0, 0);
    { Task k = {}; k.op = OP_ARGMAX; pa.push_back(k);
      for (int w = 1; w < QPN_NW; ++w) { Task s = {}; s.op = OP_STAGE; s.a = 1; s.b = QPN_NW - 1; pa.push_back(s); } }
    // aux matrices (natural rows) for the frame-rate projection kernels: the gate's columns behind the two taps
    d.logRa = ilog2(Ra); d.aux_tiles = 2 * C / (64 / Ra);
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        const int off = pack_matrix(map, 2 * C, A, g.Ap, [&](int row, int k) { return tp_gate_src(y, C, A, 2 * C + k, row); });
        if (l == 0) d.aux_woff4 = off;
    }
    phases.push_back(p1); phases.push_back(p2); phases.push_back(pa);
    // lay the phases out as slots x waves; the ARGMAX/STAGE phase keeps its fixed wave assignment
    int slot = 0;
    for (size_t pi = 0; pi < phases.size(); ++pi) {
        const std::vector<Task>& ph = phases[pi];
        const bool is_last = pi + 1 == phases.size();
        const int ns = (int)((ph.size() + QPN_NW - 1) / QPN_NW);
        d.tasks.resize((size_t)(slot + ns) * QPN_NW);
        for (int s = 0; s < ns; ++s)
            for (int w = 0; w < QPN_NW; ++w) {
                const size_t idx = (size_t)s * QPN_NW + w;
                Task k = {}; k.op = OP_NOP;
                if (idx < ph.size()) k = ph[idx];
                if (s == 0) k.op |= TF_BARRIER | (is_last ? TF_DRAIN : 0);
                d.tasks[(size_t)(slot + s) * QPN_NW + w] = k;
            }
        slot += ns;
    }
    while (slot % 3) d.tasks.resize((size_t)(++slot) * QPN_NW, Task{});      // the kernel unrolls the slot loop by 3 (three weight tiles in flight per wave)
    d.n_slots = slot;
    p.o_tasks = o; o += slot * QPN_NW * 8;
    p.lds_floats = o;
    d.single_cu_ok = (size_t)o * 4 <= 160 * 1024;        // otherwise: several workgroups per utterance (decode_coop.hip)
    d.n_map = map.size(); d.n_tasks = d.tasks.size();
    return d;
}
