// Stand-alone sweep over the decode program planner (qpnet_amd/csrc/decode_program.h): for a list of geometries, with and without the batched cooperative kernel's blocks,
// the gather map is decoded back through position formulas written out HERE (not the packers' loops): every 4 KiB-tile matrix and every fragment block must hold each
// element of its tensor exactly once, at the index tp_*_src gives (what training packs and reduces into), with -1 exactly on the padding; the two families must agree;
// the task table must cover every row of every matrix once per phase; the LDS regions must lie in the order the kernels assume.  Prints a hash of every list
// ("GOLDEN ..." lines, compared with tests/golden/decode_program.json by tests/test_decode_program_cpu.py) and the number of programs checked.  Widths that are multiples
// of 16 but not of 32 and an acceptance sweep over n_resch, n_skipch and n_quantize run the same checks without a hash ("CHECKED ..." lines, the counts of the last line).
// Built with the host sanitizers and run as a child process.
#include "../qpnet_amd/csrc/qpn_geom.h"
#include "../qpnet_amd/csrc/decode_program.h"
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

static thread_local char g_err[512] = "";      // (thread_local, atomic: the acceptance sweep checks its programs on several threads)
void qpn_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

static thread_local std::string g_ctx;
static std::atomic<long> n_programs(0);
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s (line %d) -- %s\n", #cond, __LINE__, g_ctx.c_str()); exit(1); } } while (0)

template <class T> static void golden(const char* name, const char* key, const T* p, size_t n) {      // 64-bit FNV-1a over the values widened to 64 bits, little endian
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { long long v = (long long)p[i]; for (int b = 0; b < 8; ++b) { h ^= (unsigned long long)((v >> (8 * b)) & 0xff); h *= 1099511628211ull; } }
    printf("GOLDEN %s %s %zu %016llx\n", name, key, n, h);
}

struct Range { int64_t lo, n; bool has(int64_t v) const { return v >= lo && v < lo + n; } };

// ---- where the kernels read element (row, k) of a matrix (load_tile / chunk16 of decode_dev.h, the A operand of decode_coopb.hip)
// 4 KiB tiles: K padded to Kp = 16 R, 64 / R rows per tile; lane = (row in tile) * R + 16-deep chunk, float4 j of the lane holds k = 16 chunk + 4 j + e
static size_t tile_pos(int off4, int Kp, int row, int k) {
    const int R = Kp / 16, rpt = 64 / R, t = row / rpt, lane = (row % rpt) * R + k / 16, j = (k % 16) / 4, e = k % 4;
    return (size_t)off4 * 4 + ((size_t)(t * 4 + j) * 64 + lane) * 4 + e;
}
// fragment tiles of 16 rows: per 16-deep chunk c, word c * 64 + lane holds, as element e, M[lane & 15][16 c + 4 e + (lane >> 4)]
static size_t mtile_pos(size_t tile4, int m, int k) {
    const int c = k / 16, e = (k % 16) / 4, lane = ((k % 4) << 4) | m;
    return tile4 * 4 + ((size_t)c * 64 + lane) * 4 + e;
}

struct Checker {
    const Geom& g; const DecodeProgram& d;
    std::vector<char> claimed;      // every position of the map belongs to exactly one matrix
    std::vector<int> stamp;         // which matrix a flat index was last seen in: within one matrix every element appears once
    int n_mats = 0;
    Checker(const Geom& g_, const DecodeProgram& d_) : g(g_), d(d_), claimed(d_.map.size(), 0), stamp((size_t)g_.n_params, -1) {}

    // a 4 KiB-tile matrix at off4: rows x K (padded to Kp); want(row, k) -> flat index, inside `in`
    template <class F> void tiles(int off4, int rows, int K, int Kp, Range in, F want) {
        const int id = n_mats++;
        CHECK(off4 >= 0 && rows % (64 / (Kp / 16)) == 0 && (size_t)off4 * 4 + (size_t)rows * Kp <= d.map.size());
        for (int row = 0; row < rows; ++row) for (int k = 0; k < Kp; ++k) {
            const size_t pos = tile_pos(off4, Kp, row, k);
            CHECK(pos < claimed.size() && !claimed[pos]); claimed[pos] = 1;
            const int v = d.map[pos];
            if (k >= K) { CHECK(v == -1); continue; }      // -1 is exactly the K padding
            CHECK(v >= 0 && in.has(v) && (int64_t)v == want(row, k) && stamp[v] != id); stamp[v] = id;
        }
    }
    // the fragment tile `rel4` of every workgroup's block: valid(w, m) rows x K columns (chunks up to Kp); want(w, m, k) -> flat index; the tile family keeps the
    // same element at tpos(w, m, k).  -> the number of elements it holds
    template <class V, class F, class T> size_t mtiles(int rel4, int K, int Kp, V valid, F want, T tpos) {
        const int id = n_mats++, G = g.C / 8;
        size_t n = 0;
        for (int w = 0; w < G; ++w) for (int m = 0; m < 16; ++m) for (int k = 0; k < Kp; ++k) {
            const size_t tile4 = (size_t)d.cb_base4 + (size_t)w * d.cb_per_w + rel4, pos = mtile_pos(tile4, m, k);
            CHECK(pos >= ((size_t)d.cb_base4 + (size_t)w * d.cb_per_w) * 4 && pos < ((size_t)d.cb_base4 + (size_t)(w + 1) * d.cb_per_w) * 4 && !claimed[pos]); claimed[pos] = 1;
            const int v = d.map[pos];
            if (k >= K || !valid(w, m)) { CHECK(v == -1); continue; }
            CHECK(v >= 0 && (int64_t)v == want(w, m, k) && v == d.map[tpos(w, m, k)] && stamp[v] != id); stamp[v] = id;      // both families read the index tp_*_src gives
            ++n;
        }
        return n;
    }
};

static void check_program(const Geom& g, bool cb, const DecodeProgram& d) {
    ++n_programs;
    const int C = g.C, S = g.S, Q = g.Q, A = g.A, L = g.L, Cp = g.Cp, Sp = g.Sp, Ap = g.Ap;
    const DecodeLds& p = d.lds;
    CHECK(d.rc == QPN_OK && d.err[0] == 0 && d.cb_ok == cb && d.n_map == d.map.size() && d.n_tasks == d.tasks.size() && d.map.size() % 1024 == 0);
    for (int v : d.map) CHECK(v >= -1 && v < g.n_params);

    // ---- LDS regions: in the kernels' order, 4-float aligned, each where the one before ends; state first, then biases, then tasks
    {
        const int off[] = {p.o_xbuf, p.o_xp, p.o_pd, p.o_auxv, p.o_g, p.o_skf, p.o_ska, p.o_y1, p.o_y2, p.o_lg, p.o_samp, p.o_sel, p.o_gl, p.o_bias, p.o_tasks, p.lds_floats};
        const int len[] = {(L + 1) * Cp, L * Cp, 4 * L * C, 2 * L * C, Cp, S, S, Sp, Sp, Q, 4, L, L * Cp, L * (C + S) + S + Q, d.n_slots * QPN_NW * 8};
        CHECK(off[0] == 0);
        for (int i = 0; i < 15; ++i) CHECK(off[i] % 4 == 0 && off[i + 1] == ((off[i] + len[i] + 3) & ~3));
        CHECK(p.state_floats == p.o_bias && p.n_bias == len[13] && d.n_slots % 3 == 0 && d.n_tasks == (size_t)d.n_slots * QPN_NW);
        CHECK(d.single_cu_ok == ((size_t)p.lds_floats * 4 <= 160 * 1024));
    }
    // ---- bias list: every residual, skip and post-net bias once, where FastParams points; the descriptors of k_fold_bias and the launchers' flat offsets
    {
        CHECK((int)d.bias_src.size() == p.n_bias);
        std::vector<char> seen((size_t)g.n_params, 0);
        size_t n = 0;
        auto block = [&](int lds, int64_t flat, int cnt) {
            CHECK(lds >= p.o_bias && lds + cnt <= p.o_bias + p.n_bias);
            for (int i = 0; i < cnt; ++i) { const int v = d.bias_src[(size_t)(lds - p.o_bias + i)]; CHECK((int64_t)v == flat + i && !seen[v]); seen[v] = 1; ++n; }
        };
        for (int l = 0; l < L; ++l) {
            const LayerGeom& y = g.layers[l];
            block(d.fp.b_res[l], y.resb, C); block(d.fp.b_skip[l], y.skipb, S);
            CHECK(d.f_resb[l] == y.resb && d.f_skipb[l] == y.skipb && d.fp.adaptive[l] == y.adaptive);
            const BiasDesc& b = d.bd[l];
            CHECK(b.auxb[0] == y.auxSb && b.auxb[1] == y.auxTb && b.convb[0] == y.bS && b.convb[1] == y.bT && b.convPb[0] == y.bSP && b.convPb[1] == y.bTP && b.adaptive == y.adaptive && b.pad == 0);
        }
        block(d.fp.b_p1, g.post1_b, S); block(d.fp.b_p2, g.post2_b, Q);
        CHECK(n == d.bias_src.size() && d.f_p1b == g.post1_b && d.f_p2b == g.post2_b);
    }
    // ---- the map
    Checker ck(g, d);
    const int cbG = C / 8, SBc = S / cbG, QBc = Q / cbG;
    const size_t cb_floats = cb ? (size_t)d.cb_per_w * cbG * 4 : 0;
    const bool cb_exact = cb && S % cbG == 0 && Q % cbG == 0 && SBc <= 8 && QBc <= 16;      // (forced on a geometry that kernel refuses: positions and indices still hold, the row cover does not)
    if (cb) CHECK(d.cb_base4 == 0 && d.cb_per_w == (3 * L * (Cp / 16) + 2 * (Sp / 16)) * 64 && d.cb_p1 == 3 * L * (Cp / 16) * 64 && d.cb_p2 == d.cb_p1 + (Sp / 16) * 64);
    else { CHECK(d.cb_base4 == 0 && d.cb_per_w == 0 && d.cb_p1 == 0 && d.cb_p2 == 0); for (int l = 0; l < QPN_MAX_LAYERS; ++l) CHECK(!d.cb_zc[l] && !d.cb_zp[l] && !d.cb_rs[l]); }
    const int aux_f4 = d.aux_tiles * 256;
    CHECK(d.logRa == ilog2(Ap / 16) && d.aux_tiles == 2 * C / (64 / (Ap / 16)));
    auto il = [C](int n) { return 2 * (n % C) + n / C; };      // z column half * C + c -> its row in the interleaved order
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        const int w_cur = d.fp.w_cur[l], w_past = d.fp.w_past[l], w_pil = d.w_past_il[l], w_res = d.fp.w_res[l], w_skip = d.fp.w_skip[l];
        CHECK((size_t)w_past * 4 >= cb_floats);      // every 4 KiB tile lies behind the fragment blocks
        auto conv = [&](int n, bool past_tap) { return past_tap && y.adaptive ? Range{n / C ? y.wTP : y.wSP, (int64_t)C * C} : Range{n / C ? y.wT : y.wS, (int64_t)C * C * (y.adaptive ? 1 : 2)}; };
        // (the gate's halves and taps live in tensors of their own: the range is checked per element)
        ck.tiles(w_past, 2 * C, C, Cp, Range{0, g.n_params}, [&](int row, int k) { const int64_t v = tp_gate_src(y, C, A, C + k, row); CHECK(conv(row, true).has(v)); return v; });
        ck.tiles(w_cur, 2 * C, C, Cp, Range{0, g.n_params}, [&](int row, int k) { const int n = (row & 1) * C + (row >> 1); const int64_t v = tp_gate_src(y, C, A, k, n); CHECK(conv(n, false).has(v)); return v; });
        ck.tiles(w_pil, 2 * C, C, Cp, Range{0, g.n_params}, [&](int row, int k) { return tp_gate_src(y, C, A, C + k, (row & 1) * C + (row >> 1)); });
        for (int n = 0; n < 2 * C; ++n) for (int k = 0; k < Cp; ++k) CHECK(d.map[tile_pos(w_pil, Cp, il(n), k)] == d.map[tile_pos(w_past, Cp, n, k)]);      // the row permutation (r, half) -> 2 r + half
        ck.tiles(w_res, C, C, Cp, Range{y.res, (int64_t)C * C}, [&](int row, int k) { return tp_res_src(y, C, k, row); });
        ck.tiles(w_skip, S, C, Cp, Range{y.skip, (int64_t)S * C}, [&](int row, int k) { return tp_skip_src(g, l * C + k, row); });
        ck.tiles(d.aux_woff4 + l * aux_f4, 2 * C, A, Ap, Range{0, g.n_params}, [&](int row, int k) {
            const int64_t v = tp_gate_src(y, C, A, 2 * C + k, row); CHECK((Range{row / C ? y.auxT : y.auxS, (int64_t)C * A}).has(v)); return v; });
        if (cb) {
            CHECK(d.cb_zc[l] == 3 * l * (Cp / 16) * 64 && d.cb_zp[l] == d.cb_zc[l] + (Cp / 16) * 64 && d.cb_rs[l] == d.cb_zp[l] + (Cp / 16) * 64);
            auto gate_n = [C](int w, int m) { return (m >> 3) * C + 8 * w + (m & 7); };
            auto all = [](int, int) { return true; };
            size_t n = ck.mtiles(d.cb_zc[l], C, Cp, all, [&](int w, int m, int k) { return tp_gate_src(y, C, A, k, gate_n(w, m)); }, [&](int w, int m, int k) { return tile_pos(w_cur, Cp, il(gate_n(w, m)), k); });
            CHECK(n == (size_t)2 * C * C);
            n = ck.mtiles(d.cb_zp[l], C, Cp, all, [&](int w, int m, int k) { return tp_gate_src(y, C, A, C + k, gate_n(w, m)); }, [&](int w, int m, int k) { return tile_pos(w_past, Cp, gate_n(w, m), k); });
            CHECK(n == (size_t)2 * C * C);
            n = ck.mtiles(d.cb_rs[l], C, Cp, [&](int, int m) { return m < 8 + SBc; },
                          [&](int w, int m, int k) { return m < 8 ? tp_res_src(y, C, k, 8 * w + m) : tp_skip_src(g, l * C + k, SBc * w + m - 8); },
                          [&](int w, int m, int k) { return m < 8 ? tile_pos(w_res, Cp, 8 * w + m, k) : tile_pos(w_skip, Cp, SBc * w + m - 8, k); });
            if (cb_exact) CHECK(n == (size_t)C * C + (size_t)S * C);
        }
    }
    ck.tiles(d.fp.w_p1, S, S, Sp, Range{g.post1_w, (int64_t)S * S}, [&](int row, int k) { return tp_post1_src(g, k, row); });
    ck.tiles(d.fp.w_p2, Q, S, Sp, Range{g.post2_w, (int64_t)Q * S}, [&](int row, int k) { return tp_post2_src(g, k, row); });
    if (cb) {
        size_t n = ck.mtiles(d.cb_p1, S, Sp, [&](int, int m) { return m < SBc; }, [&](int w, int m, int k) { return tp_post1_src(g, k, SBc * w + m); }, [&](int w, int m, int k) { return tile_pos(d.fp.w_p1, Sp, SBc * w + m, k); });
        if (cb_exact) CHECK(n == (size_t)S * S);
        n = ck.mtiles(d.cb_p2, S, Sp, [&](int, int m) { return m < QBc; }, [&](int w, int m, int k) { return tp_post2_src(g, k, QBc * w + m); }, [&](int w, int m, int k) { return tile_pos(d.fp.w_p2, Sp, QBc * w + m, k); });
        if (cb_exact) CHECK(n == (size_t)Q * S);
    }
    for (size_t i = 0; i < ck.claimed.size(); ++i) CHECK(ck.claimed[i]);      // nothing in the map but these matrices: the blocks are contiguous and disjoint

    // ---- task table: the phases in order; per phase every row of its matrices under exactly one task
    struct Mat { int op, off4, rows, Kp; };
    std::vector<std::vector<Mat>> phases;
    for (int l = 0; l < L; ++l) {
        phases.push_back({{OP_Z, d.fp.w_cur[l], 2 * C, Cp}, {OP_PAST, d.fp.w_past[l], 2 * C, Cp}});
        phases.push_back({{OP_RES, d.fp.w_res[l], C, Cp}, {OP_SKIP, d.fp.w_skip[l], S, Cp}});
    }
    phases.push_back({{OP_POST1, d.fp.w_p1, S, Sp}}); phases.push_back({{OP_POST2, d.fp.w_p2, Q, Sp}});
    int slot = 0;
    auto flags_ok = [&](const Task& k, bool first, bool last_phase) { return ((k.op & TF_BARRIER) != 0) == first && ((k.op & TF_DRAIN) != 0) == (first && last_phase); };
    for (size_t pi = 0; pi < phases.size(); ++pi) {
        const int l = (int)pi / 2;
        size_t ntask = 0;
        for (const Mat& m : phases[pi]) ntask += (size_t)m.rows / (64 / (m.Kp / 16));
        const int ns = (int)((ntask + QPN_NW - 1) / QPN_NW);
        CHECK((size_t)(slot + ns) * QPN_NW <= d.tasks.size());
        std::vector<std::vector<int>> cover;
        for (const Mat& m : phases[pi]) cover.push_back(std::vector<int>((size_t)m.rows, 0));
        for (int s = 0; s < ns; ++s) for (int w = 0; w < QPN_NW; ++w) {
            const Task& k = d.tasks[(size_t)(slot + s) * QPN_NW + w];
            CHECK(flags_ok(k, s == 0, false));
            if ((size_t)s * QPN_NW + w >= ntask) { CHECK((k.op & 0xff) == OP_NOP && !(k.op & TF_HASW)); continue; }
            CHECK(k.op & TF_HASW);
            size_t mi = 0; while (mi < phases[pi].size() && phases[pi][mi].op != (k.op & 0xff)) ++mi;
            CHECK(mi < phases[pi].size());
            const Mat& m = phases[pi][mi];
            const int R = m.Kp / 16, rpt = 64 / R;
            CHECK(((k.op >> 16) & 0xf) == ilog2(R) && (1 << ilog2(R)) == R && k.row0 % rpt == 0 && k.row0 + rpt <= m.rows && k.woff4 == m.off4 + (k.row0 / rpt) * 256);
            CHECK((size_t)k.woff4 * 4 >= cb_floats && ((size_t)k.woff4 * 4 - cb_floats) % 1024 == 0 && (size_t)k.woff4 * 4 + 1024 <= d.map.size());      // inside the map, on a tile boundary
            for (int r = 0; r < rpt; ++r) ++cover[mi][(size_t)k.row0 + r];
            const bool last_layer = l == L - 1;
            switch (k.op & 0xff) {
            case OP_Z: CHECK(k.xoff == p.o_xbuf + l * Cp && k.a == l * 2 * C && k.c == p.o_g); break;
            case OP_PAST: CHECK(k.xoff == p.o_xp + l * Cp && k.a == l * 2 * C && k.b == p.o_xbuf + l * Cp && k.c == l); break;
            case OP_RES: CHECK(k.xoff == p.o_g && k.a == p.o_xbuf + l * Cp && k.b == d.fp.b_res[l] && k.c == p.o_xbuf + (l + 1) * Cp && k.d == (last_layer ? -1 : l + 1)); break;
            case OP_SKIP: CHECK(k.xoff == p.o_g && k.a == (g.layers[l].adaptive ? p.o_ska : p.o_skf) && k.b == d.fp.b_skip[l] && k.d == p.o_y1 && ((k.op & TF_LAST) != 0) == last_layer); break;
            case OP_POST1: CHECK(k.xoff == p.o_y1 && k.b == d.fp.b_p1 && k.c == p.o_y2); break;
            default: CHECK((k.op & 0xff) == OP_POST2 && k.xoff == p.o_y2 && k.b == d.fp.b_p2 && k.c == p.o_lg); break;
            }
        }
        for (const auto& c : cover) for (int n : c) CHECK(n == 1);
        slot += ns;
    }
    for (int w = 0; w < QPN_NW; ++w) {      // the pick / staging phase on its fixed waves: the only one that drains
        const Task& k = d.tasks[(size_t)slot * QPN_NW + w];
        CHECK(flags_ok(k, true, true) && !(k.op & TF_HASW) && (k.op & 0xff) == (w == 0 ? OP_ARGMAX : OP_STAGE));
        if (w) CHECK(k.a == 1 && k.b == QPN_NW - 1);
    }
    for (++slot; slot < d.n_slots; ++slot) for (int w = 0; w < QPN_NW; ++w) { const Task& k = d.tasks[(size_t)slot * QPN_NW + w]; CHECK(k.op == OP_NOP && !k.woff4 && !k.xoff && !k.row0 && !k.a && !k.b && !k.c && !k.d); }
    CHECK(slot == d.n_slots);
}

static void print_golden(const char* nm, const Geom& g, const DecodeProgram& d) {
    golden(nm, "map", d.map.data(), d.map.size());
    golden(nm, "tasks", (const int*)d.tasks.data(), d.tasks.size() * 8);
    golden(nm, "bias_src", d.bias_src.data(), d.bias_src.size());
    const DecodeLds& p = d.lds;
    std::vector<long long> v = {p.o_xbuf, p.o_xp, p.o_pd, p.o_auxv, p.o_g, p.o_skf, p.o_ska, p.o_y1, p.o_y2, p.o_lg, p.o_samp, p.o_sel, p.state_floats,
                                p.o_bias, p.n_bias, p.o_tasks, p.lds_floats, p.o_gl, d.n_slots, d.n_slots};
    golden(nm, "lds", v.data(), v.size());
    golden(nm, "fast", (const int*)&d.fp, sizeof(FastParams) / sizeof(int));
    golden(nm, "w_past_il", d.w_past_il, QPN_MAX_LAYERS);
    v = {d.aux_woff4, d.aux_tiles, d.logRa};
    golden(nm, "aux", v.data(), v.size());
    v = {d.cb_ok, d.cb_base4, d.cb_per_w, d.cb_p1, d.cb_p2};
    for (int l = 0; l < QPN_MAX_LAYERS; ++l) { v.push_back(d.cb_zc[l]); v.push_back(d.cb_zp[l]); v.push_back(d.cb_rs[l]); }
    golden(nm, "cb", v.data(), v.size());
    v = {d.single_cu_ok};
    golden(nm, "single_cu_ok", v.data(), v.size());
    v.clear();
    for (int l = 0; l < g.L; ++l) { const BiasDesc& b = d.bd[l]; for (long long x : {(long long)b.auxb[0], (long long)b.auxb[1], (long long)b.convb[0], (long long)b.convb[1], (long long)b.convPb[0], (long long)b.convPb[1], (long long)b.adaptive, (long long)b.pad}) v.push_back(x); }
    for (int l = 0; l < g.L; ++l) { v.push_back(d.f_resb[l]); v.push_back(d.f_skipb[l]); }
    v.push_back(d.f_p1b); v.push_back(d.f_p2b);
    golden(nm, "biases", v.data(), v.size());
}

// ---- which widths decode, restated HERE from the kernels' tile shape and not from the planner's arithmetic: a matrix with K input columns is cut into 4 KiB tiles of
// 64 lanes x 16 floats; K is padded to 16, 32, 64, ... so a row takes 1, 2, 4, ... lanes and a tile holds 64, 32, 16, 8, 4, 2, 1 rows.  Every matrix of the step must be a
// whole number of tiles: the gate (2 n_resch rows), residual (n_resch) and skip (n_skipch) matrices have K = n_resch; the post-net ones (n_skipch and n_quantize rows) K =
// n_skipch; the feature projection (2 n_resch rows) K = n_aux.  One CU's waves reduce at most 32 lanes of n_resch and 64 of the other two.
static int rows_per_tile(int K) { return K <= 16 ? 64 : K <= 32 ? 32 : K <= 64 ? 16 : K <= 128 ? 8 : K <= 256 ? 4 : K <= 512 ? 2 : K <= 1024 ? 1 : 0; }
static bool rule_accepts(int C, int S, int Q, int A) {
    const int hc = rows_per_tile(C), hs = rows_per_tile(S), ha = rows_per_tile(A);
    if (C > 512 || !hs || !ha) return false;
    return C % hc == 0 && S % hc == 0 && S % hs == 0 && Q % hs == 0 && (2 * C) % ha == 0;
}
static bool names_a_quantity(const char* err) { const std::string e(err); return e.find("n_resch") != std::string::npos && e.find("n_skipch") != std::string::npos && e.find("n_quantize") != std::string::npos; }

struct NG { const char* name; qpn_config c; };
int main() {
    // {n_quantize, n_aux, n_resch, n_skipch, dilationF_depth, dilationF_repeat, dilationA_depth, dilationA_repeat, kernel_size, upsampling_factor}
    static const NG geoms[] = {
        {"tiny", {256, 39, 32, 32, 2, 1, 1, 1, 2, 110}},                 // the 13 geometries of tests/train_plan_sweep.cpp ...
        {"paper", {256, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"default", {256, 39, 512, 256, 4, 3, 4, 1, 2, 110}},            // (batched kernel: 4 of 8 skip rows and 4 of 16 logit rows per workgroup -- padding rows)
        {"deep64", {256, 39, 64, 256, 10, 3, 4, 1, 2, 110}},
        {"paper_aux7", {256, 7, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_aux80", {256, 80, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_up0", {256, 39, 64, 256, 4, 1, 4, 1, 2, 0}},
        {"paper_up8", {256, 39, 64, 256, 4, 1, 4, 1, 2, 8}},
        {"paper_q128", {128, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_q64", {64, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"all_adaptive", {256, 39, 64, 256, 0, 0, 4, 2, 2, 110}},
        {"all_fixed", {256, 39, 64, 256, 4, 2, 0, 0, 2, 110}},
        {"c160", {256, 39, 160, 256, 2, 1, 2, 1, 2, 110}},
        {"c160_s96_a17", {256, 17, 160, 96, 2, 1, 2, 1, 2, 120}},        // ... n_skipch != n_resch, neither a power of two (aux_c160_s96_a17_u120 of tests/golden/cases.py)
        {"c256_q64", {64, 39, 256, 256, 2, 1, 2, 1, 2, 110}},            // ... and the batched kernel with all 8 skip rows but 2 of 16 logit rows per workgroup
    };
    for (const NG& ng : geoms) {
        Geom g;
        CHECK(qpn_build_geom(&ng.c, &g) == QPN_OK);
        for (int cb = 0; cb < 2; ++cb) {
            if (cb && (g.C % 8 || g.C < 128)) continue;      // (the fragment blocks split the channels into workgroups of 8)
            const std::string name = std::string(ng.name) + "/cb" + std::to_string(cb);
            g_ctx = name;
            const DecodeProgram d = decode_program(g, cb != 0);
            check_program(g, cb != 0, d);
            print_golden(name.c_str(), g, d);
        }
    }
    {   // the refusals: their codes and messages, before anything is built
        g_ctx = "refusals";
        Geom g;
        const qpn_config c24 = {256, 39, 24, 32, 2, 1, 1, 1, 2, 110}, c1024 = {256, 39, 1024, 256, 2, 1, 1, 1, 2, 110}, ok = {256, 39, 32, 32, 2, 1, 1, 1, 2, 110};
        CHECK(qpn_build_geom(&c24, &g) == QPN_OK);
        DecodeProgram d = decode_program(g, false);
        CHECK(d.rc == QPN_EINVAL && d.map.empty() && d.tasks.empty());
        printf("REFUSED refused_c24/cb0 %d %s\n", d.rc, d.err);
        CHECK(qpn_build_geom(&c1024, &g) == QPN_OK);
        d = decode_program(g, false);
        CHECK(d.rc == QPN_EINVAL && d.map.empty() && d.tasks.empty());
        printf("REFUSED refused_c1024/cb0 %d %s\n", d.rc, d.err);
        CHECK(qpn_build_geom(&ok, &g) == QPN_OK);
        g.n_params = (int64_t)1 << 31;                   // (no buildable geometry is this large: the planner must refuse before it sizes anything by it)
        d = decode_program(g, false);
        CHECK(d.rc == QPN_EINVAL && d.map.empty() && std::string(d.err) == "model too large for 32-bit gather map");
    }
    const long n_golden = n_programs;
    // ---- widths that are multiples of 16 but not of 32, and the decode-only ones (tests/test_width_classes_gpu.py runs them on the kernels): the invariant checks alone.
    // They get no golden hash -- tests/golden/decode_program.json comes from the code in front of the planner, which nobody ran at these widths -- and are printed as
    // "CHECKED name"; the ones the planner must refuse, by the rule restated in rule_accepts, as "CHECKED name refused"
    static const int wide[][3] = {{72, 72, 64}, {48, 80, 48}, {80, 64, 96}, {112, 144, 80}, {264, 136, 64}, {128, 112, 192}, {64, 48, 32}, {256, 256, 128},      // n_resch, n_skipch, n_quantize: the decode cases
                                  {16, 16, 16}, {80, 48, 96}, {32, 16, 64}, {64, 16, 256}, {64, 272, 144}};                                                           // ... and the training cases that are not among them
    for (const auto& w : wide) {
        const qpn_config c = {w[2], 39, w[0], w[1], 2, 1, 2, 1, 2, 110};
        Geom g;
        CHECK(qpn_build_geom(&c, &g) == QPN_OK);
        for (int cb = 0; cb < 2; ++cb) {
            if (cb && (g.C % 8 || g.C < 128)) continue;
            const std::string name = "w" + std::to_string(w[0]) + "_" + std::to_string(w[1]) + "_" + std::to_string(w[2]) + "/cb" + std::to_string(cb);
            g_ctx = name;
            const DecodeProgram d = decode_program(g, cb != 0);
            if (rule_accepts(w[0], w[1], w[2], 39)) { check_program(g, cb != 0, d); printf("CHECKED %s\n", name.c_str()); }
            else { CHECK(d.rc == QPN_EINVAL && d.map.empty() && d.tasks.empty() && names_a_quantity(d.err)); printf("CHECKED %s refused\n", name.c_str()); }
        }
    }
    const long n_checked = n_programs - n_golden;
    // ---- acceptance: a shallow 2 + 2-layer geometry with n_aux 39; every n_resch that is a multiple of 4 up to 272 (all of 8, 16, ..., 160 among them) with widths of
    // n_skipch and n_quantize on and off every tile height.  The planner's decision is the rule's, and every program it builds passes the checks above
    // (about a thousand programs of a million map entries each: the geometries are independent and are handed out to a few threads)
    struct CSQ { int C, S, Q; };
    std::vector<CSQ> combos;
    for (int C = 4; C <= 272; C += 4) for (int S : {16, 48, 72, 80, 136, 144}) for (int Q : {16, 32, 48, 64, 80, 96, 192}) combos.push_back({C, S, Q});
    std::atomic<size_t> next(0);
    std::atomic<long> accepted(0);
    auto worker = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < combos.size();) {
            const int C = combos[i].C, S = combos[i].S, Q = combos[i].Q;
            const qpn_config c = {Q, 39, C, S, 2, 1, 2, 1, 2, 110};
            Geom g;
            g_ctx = "acceptance C " + std::to_string(C) + " S " + std::to_string(S) + " Q " + std::to_string(Q);
            CHECK(qpn_build_geom(&c, &g) == QPN_OK);
            const DecodeProgram d = decode_program(g, false);
            const bool want = rule_accepts(C, S, Q, 39);
            CHECK((d.rc == QPN_OK) == want);
            if (want) { check_program(g, false, d); ++accepted; }
            else CHECK(d.rc == QPN_EINVAL && d.map.empty() && d.tasks.empty() && names_a_quantity(d.err));
        }
    };
    {
        const unsigned hw = std::thread::hardware_concurrency(), nthr = hw < 2 ? 1 : hw > 8 ? 8 : hw;
        std::vector<std::thread> pool;
        for (unsigned i = 1; i < nthr; ++i) pool.emplace_back(worker);
        worker();
        for (std::thread& th : pool) th.join();
    }
    const long n_swept = (long)combos.size(), n_accepted = accepted.load();
    CHECK(n_accepted > 300 && n_swept - n_accepted > 300);
    {   // where one CU stops holding the step state (n_resch in steps of 16, n_skipch = n_quantize = 64, 2 + 2 layers): the two widths test_width_classes_gpu.py decodes
        int last_ok = 0, first_not = 0;
        for (int C = 16; C <= 512; C += 16) {
            const qpn_config c = {64, 39, C, 64, 2, 1, 2, 1, 2, 110};
            Geom g;
            g_ctx = "single_cu_ok C " + std::to_string(C);
            CHECK(qpn_build_geom(&c, &g) == QPN_OK);
            if (!rule_accepts(C, 64, 64, 39)) continue;
            const DecodeProgram d = decode_program(g, false);
            CHECK(d.rc == QPN_OK);
            if (d.single_cu_ok) { CHECK(!first_not); last_ok = C; }      // (monotonic: no width fits again once one did not)
            else if (!first_not) first_not = C;
        }
        CHECK(last_ok && first_not == last_ok + 16);
        for (int C : {last_ok, first_not}) {
            const qpn_config c = {64, 39, C, 64, 2, 1, 2, 1, 2, 110};
            Geom g;
            g_ctx = "single_cu_ok pair C " + std::to_string(C);
            CHECK(qpn_build_geom(&c, &g) == QPN_OK);
            check_program(g, false, decode_program(g, false));
        }
        printf("SINGLE_CU last %d first_not %d\n", last_ok, first_not);
    }
    printf("DECODE_PROGRAM_SWEEP_OK %ld programs %ld checked %ld swept %ld accepted\n", n_golden, n_checked, n_swept, n_accepted);
    return 0;
}
