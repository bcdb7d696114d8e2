// Stand-alone sweep over the weight-gradient planner (qpnet_amd/csrc/train_wgrad_plan.h): the five contraction records of a step, the kernel instance each gets
// and the row-block split, for the named geometries of tests/train_plan_sweep.cpp and the width classes of tests/test_width_classes_gpu.py, at B = 1 and 2 and six
// knob settings.  Records only -- no memory behind the (fake, distinct) buffer bases.  Checks the invariants the kernels rely on, the boundary cases no GPU test can
// hold, the instances the benchmark names for the paper geometry, and prints one "GOLDEN ..." line per launch of the named geometries, compared with
// tests/golden/wgrad_plan.json (made from the code in front of the planner: MEASUREMENTS.md) by tests/test_wgrad_plan_cpu.py.  Built with the host sanitizers.
#include "../qpnet_amd/csrc/qpn_geom.h"
#include "../qpnet_amd/csrc/train_wgrad_plan.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static char g_err[512] = "";
void qpn_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

static std::string g_ctx;
static long n_steps = 0, n_launches = 0, n_refused = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s (line %d) -- %s\n", #cond, __LINE__, g_ctx.c_str()); exit(1); } } while (0)

// ---- fake buffers: base k << 40 (bytes), so a pointer names its buffer and its offset
enum { FB_DZ = 1, FB_DXA, FB_DXB, FB_DS0, FB_DY0, FB_DLOGITS, FB_X, FB_GATE_TH, FB_GATE_G, FB_S0, FB_Y0, FB_HUP, FB_TAP, FB_XC, FB_SLAB };
template <class T> static T* fake(int k) { return (T*)((uintptr_t)k << 40); }
struct Fnv {      // 64-bit FNV-1a over values widened to 64 bits, little endian
    unsigned long long h = 1469598103934665603ull;
    void add(long long v) { for (int b = 0; b < 8; ++b) { h ^= (unsigned long long)((v >> (8 * b)) & 0xff); h *= 1099511628211ull; } }
    void ptr(const void* p) { const uintptr_t u = (uintptr_t)p; add((long long)(u >> 40)); add((long long)(u & (((uintptr_t)1 << 40) - 1))); }      // buffer, byte offset
};
static unsigned long long hash_rec(const Wg2& w) {      // every field the record carries; the per-layer arrays up to nlayers
    Fnv f;
    f.ptr(w.A); f.ptr(w.A2); f.add((long long)w.A_lstride); f.add(w.lda); f.add(w.M); f.add(w.rowsA);
    f.add(w.bmode); f.ptr(w.B1); f.ptr(w.B2); f.add((long long)w.B_lstride); f.add(w.ldb); f.add(w.N); f.add(w.Nvalid); f.add(w.rowsB);
    f.ptr(w.hup); f.ptr(w.tap); f.add(w.C); f.add(w.Ap); f.ptr(w.xc); f.add(w.nb); f.add(w.nlayers); f.ptr(w.slab); f.add(w.gstage);
    for (int l = 0; l < w.nlayers; ++l) for (int x : {w.row0A[l], w.row0B[l], w.R[l], w.goff[l], w.gbias[l], w.tap_off[l], w.dil[l]}) f.add(x);
    f.add(w.ldc); f.add(w.ncol_groups);
    return f.h;
}
static unsigned long long hash_targs(const TArgs& a, int bmode, int nlayers) {      // hup / tap: where k_gemm_tn reads them (BM_GATHER)
    Fnv f;
    f.add(a.M); f.add(a.N); f.add(a.nb); f.add(a.nsplit); f.ptr(a.a); f.ptr(a.a2); f.add(a.a_ls); f.add(a.lda); f.add(a.rowsA);
    f.ptr(a.b1); f.add(a.b_ls); f.add(a.ldb); f.add(a.rowsB);
    if (bmode == BM_GATHER) { f.ptr(a.hup); f.ptr(a.tap); }
    f.add(a.C); f.add(a.Ap); f.ptr(a.slab); f.add(a.gstage); f.add(a.ldc);
    for (int l = 0; l < nlayers; ++l) for (int x : {a.row0A[l], a.row0B[l], a.R[l], a.goff[l], a.gbias[l], a.tap_off[l], a.dil[l]}) f.add(x);
    return f.h;
}

// ---- one step: the geometry's plan, a synthetic call (increasing s_out, a tap table per layer), the path's flags
struct Step {
    WgradView v; TrainSlabs sl; WgradBufs b; WgradFlags f;
    bool gemm, generic; int nch, nch_side, gstage;
};
// one launch: a 256-row block of a record with its pick (tile path), or the record as k_gemm_tn's arguments (GEMM path)
struct Launch { std::string name; Wg2 w; WgradPick k; TArgs t; int bmode, nlayers, nch; bool early; };

enum { K_DEFAULT, K_GENERIC, K_NO_STACK_Q, K_NO_HOIST, K_NO_PAIR, K_GEMM, K_COUNT };
static const char* const KNOB_NAMES[K_COUNT] = {"default", "generic", "no_stack_queue", "no_hoist", "no_post_pair", "gemm"};
static TrainKnobs default_knobs() { TrainKnobs k = {}; k.aux_hoist = k.persist_fwd = k.persist_bwd = true; k.post_pair = true; return k; }

static bool make_step(const Geom& g, int B, int knob, Step& s) {
    TrainKnobs kn = default_knobs();
    if (knob == K_NO_HOIST) kn.aux_hoist = false;
    const TrainPlan t = train_plan(g, kn, knob == K_GEMM);
    if (t.rc != QPN_OK) return false;
    memset(&s, 0, sizeof(s));
    WgradView& v = s.v;
    const int BL = 300, maxd = 3;
    v.C = g.C; v.S = g.S; v.Q = g.Q; v.L = g.L; v.B = B; v.BL = BL; v.Ap = t.Ap; v.Ktp = t.Ktp; v.hoist = t.hoist;
    int so = 0;
    for (int l = 0; l < g.L; ++l) { v.adaptive[l] = t.layers[l].adaptive; v.dilation[l] = t.layers[l].dilation; so += v.adaptive[l] ? v.dilation[l] * maxd : v.dilation[l]; v.s_out[l] = so; }
    v.N1 = so + BL + 5;
    for (int l = 0; l < g.L; ++l) v.tap_off[l] = l * B * v.N1;
    s.sl = t.slabs; s.gstage = t.gstage; s.gemm = knob == K_GEMM; s.generic = knob == K_GENERIC;
    s.nch = t.nch; s.nch_side = s.gemm ? t.nch : (t.nch <= 48 ? t.nch : 48);      // (the side stream's chunks with the early reduction: qpn_launch_bwd)
    WgradBufs& b = s.b;
    b.DZ = fake<float>(FB_DZ); b.DXA = fake<float>(FB_DXA); b.DXB = fake<float>(FB_DXB); b.DS0 = fake<float>(FB_DS0); b.DY0 = fake<float>(FB_DY0); b.dlogits = fake<float>(FB_DLOGITS);
    b.X = fake<float>(FB_X); b.gate = fake<float>(s.gemm ? FB_GATE_G : FB_GATE_TH); b.S0 = fake<float>(FB_S0); b.Y0 = fake<float>(FB_Y0); b.HUP = fake<float>(FB_HUP);
    b.TAP = fake<int>(FB_TAP); b.XC = fake<int>(FB_XC); b.slab = fake<float>(FB_SLAB); b.gstage = t.gstage;
    // behind the stack queue dXout arrives summed (qpn_launch_bwd: the queue runs where the persistent layer kernels do)
    const bool stack_q = !s.gemm && knob != K_NO_STACK_Q && v.C == 64 && (v.Ktp == 176 || v.hoist) && v.Ap <= 64;
    s.f = s.gemm ? WgradFlags{false, false, false, false} : WgradFlags{stack_q, knob != K_NO_PAIR, true, true};
    return true;
}

// the row-block split of a record: 256 rows each, the record's rows exactly once, A's columns, the slab rows and the bias entries shifted together
static void check_blocks(const Wg2& w) {
    std::vector<Wg2> v;
    for (int i = 0; i < wgrad_n_row_blocks(w); ++i) v.push_back(wgrad_row_block(w, i));
    if (w.M <= 256 || w.bmode == 4) { CHECK(v.size() == 1 && v[0].M == w.M && v[0].A == w.A && v[0].A2 == w.A2 && v[0].ncol_groups == w.ncol_groups && v[0].goff[0] == w.goff[0] && v[0].gbias[0] == w.gbias[0]); return; }
    CHECK((int)v.size() == (w.M + 255) / 256);
    int rows = 0;
    for (const Wg2& x : v) {
        CHECK(x.M == std::min(256, w.M - rows) && x.A == w.A + rows && (w.A2 ? x.A2 == w.A2 + rows : !x.A2) && x.ncol_groups == wgrad_col_groups(x.M, x.N));
        CHECK(x.N == w.N && x.Nvalid == w.Nvalid && x.ldc == w.ldc && x.lda == w.lda && x.nlayers == w.nlayers && x.bmode == w.bmode && x.B1 == w.B1 && x.slab == w.slab);
        for (int l = 0; l < w.nlayers; ++l) CHECK(x.goff[l] == w.goff[l] + rows * w.ldc && x.gbias[l] == (w.gbias[l] >= 0 ? w.gbias[l] + rows : w.gbias[l]) && x.R[l] == w.R[l] && x.row0A[l] == w.row0A[l]);
        rows += x.M;
    }
    CHECK(rows == w.M);
}

// the launches of a step in the order qpn_launch_bwd / qpn_launch_bwd_gemm issue their records; a refused record ends at its first refused block
static std::vector<Launch> step_launches(const Step& s) {
    std::vector<Launch> out;
    auto tile = [&](const char* name, const Wg2& w, int nch, bool early) {
        int i = 0;
        check_blocks(w);
        for (int b = 0; b < wgrad_n_row_blocks(w); ++b) {
            const Wg2 blk = wgrad_row_block(w, b);
            Launch x = {}; x.name = std::string(name) + "." + std::to_string(i++); x.w = blk; x.k = wgrad_pick(blk, nch, s.generic); x.bmode = blk.bmode; x.nlayers = blk.nlayers; x.nch = nch; x.early = early;
            out.push_back(x);
            if (!x.k.family) break;
        }
    };
    auto gemm = [&](const char* name, const Wg2& w, bool early) {
        Launch x = {}; x.name = name; x.w = w; x.t = targs_of(w, s.nch); x.bmode = w.bmode; x.nlayers = w.nlayers; x.nch = s.nch; x.early = early;
        out.push_back(x);
    };
    if (s.gemm) {
        gemm("w1", wgrad_rec_w1(s.v, s.sl, s.b, s.f), false); gemm("wr", wgrad_rec_wr(s.v, s.sl, s.b, s.f), false); gemm("skip", wgrad_rec_skip(s.v, s.sl, s.b, s.f), true);
        gemm("post0", wgrad_rec_post(s.v, s.sl, s.b, s.f, 0), true); gemm("post1", wgrad_rec_post(s.v, s.sl, s.b, s.f, 1), true);
        return out;
    }
    tile("skip", wgrad_rec_skip(s.v, s.sl, s.b, s.f), s.nch_side, true);
    tile("post0", wgrad_rec_post(s.v, s.sl, s.b, s.f, 0), s.nch_side, true);
    if (!wgrad_post_paired(s.v, s.f)) tile("post1", wgrad_rec_post(s.v, s.sl, s.b, s.f, 1), s.nch_side, true);
    tile("wr", wgrad_rec_wr(s.v, s.sl, s.b, s.f), s.nch, false);
    tile("w1", wgrad_rec_w1(s.v, s.sl, s.b, s.f), s.nch, false);
    if (s.sl.g_cw >= 0) tile("causal", wgrad_rec_causal(s.v, s.sl, s.b), s.nch, false);
    return out;
}

static int pad16(int x) { return (x + 15) & ~15; }
struct Span { long lo, hi; };
static void check_step(const Step& s, const std::vector<Launch>& ls, bool may_refuse) {
    ++n_steps;
    std::vector<Span> spans;
    auto take = [&](long lo, long n, bool early) {
        CHECK(lo >= 0 && n > 0 && lo + n <= s.gstage);
        CHECK(early ? (lo >= s.sl.g_early0 && lo + n <= s.sl.g_early1) : (lo + n <= s.sl.g_early0 || lo >= s.sl.g_early1));
        spans.push_back({lo, lo + n});
    };
    for (size_t i = 0; i < ls.size(); ++i) {
        const Launch& x = ls[i];
        const Wg2& w = x.w;
        g_ctx = g_ctx.substr(0, g_ctx.find(" @")) + " @" + x.name;
        int M = w.M, N = w.N;
        if (s.gemm) {      // the conversion, field by field
            const TArgs& a = x.t;
            CHECK(a.M == w.M && a.N == w.Nvalid && a.nb == w.nb && a.nsplit == s.nch && a.a == w.A && a.a2 == w.A2 && a.a_ls == (long)w.A_lstride && a.lda == w.lda && a.rowsA == w.rowsA);
            CHECK(a.b1 == w.B1 && a.b_ls == (long)w.B_lstride && a.ldb == w.ldb && a.rowsB == w.rowsB && a.C == w.C && a.Ap == w.Ap && a.slab == w.slab && a.gstage == w.gstage && a.ldc == w.ldc);
            CHECK(w.bmode == BM_GATHER ? (a.hup == w.hup && a.tap == w.tap) : (!a.hup && !a.tap));
            for (int l = 0; l < TR_MAXL; ++l) {
                const bool in = l < w.nlayers;
                CHECK(a.row0A[l] == (in ? w.row0A[l] : 0) && a.row0B[l] == (in ? w.row0B[l] : 0) && a.R[l] == (in ? w.R[l] : 0) && a.goff[l] == (in ? w.goff[l] : 0) &&
                      a.gbias[l] == (in ? w.gbias[l] : 0) && a.tap_off[l] == (in ? w.tap_off[l] : 0) && a.dil[l] == (in ? w.dil[l] : 0));
            }
            CHECK(w.ncol_groups == 1 && !s.v.hoist && w.Nvalid == (w.bmode == BM_GATHER ? 2 * w.C + w.Ap : w.N));      // never hoisted: every column with a weight is valid
            CHECK(w.A2 ? x.name == "wr" : x.name != "wr");      // two-part dXout
            for (int l = 0; l < w.nlayers; ++l) if (w.bmode == BM_GATHER) CHECK((w.tap_off[l] >= 0) == (s.v.adaptive[l] != 0));      // fixed layers: row - dilation
            N = a.N;
            ++n_launches;
        } else {
            const WgradPick& k = x.k;
            if (!k.family) { CHECK(may_refuse); ++n_refused; continue; }
            ++n_launches;
            const int Ng = w.N / w.ncol_groups;
            CHECK(w.ncol_groups >= 1 && w.N % w.ncol_groups == 0 && k.grid[0] == x.nch && k.grid[1] == w.nlayers && k.grid[2] == w.ncol_groups && k.lds <= 160 * 1024);
            CHECK(64 * k.mpw >= pad16(w.M) && 16 * k.nt >= pad16(Ng));      // the tile budget covers the block
            if (k.family == 3) {      // every precondition of k_wgrad3, restated
                CHECK(k.bmode == w.bmode && w.M == 64 * k.mpw && Ng == 16 * k.nt && k.two_a == (w.A2 != nullptr) && k.minw == ((k.mpw == 4 && k.nt == 4 && !k.two_a) ? QPN_WGRAD_MINW : 1));
                CHECK(w.rowsB < (1 << 24) && (int64_t)w.rowsB * std::max(w.C, w.ldb) < (1ll << 32));
                CHECK(w.Nvalid == w.N || (w.ncol_groups == 1 && w.Nvalid % 4 == 0));
                if (w.bmode == 3) { CHECK(w.ldb == w.C && w.ncol_groups == 1 && w.C % 4 == 0 && w.Ap % 4 == 0 && w.tap); for (int l = 0; l < w.nlayers; ++l) CHECK(w.tap_off[l] >= 0); }
                CHECK(w.bmode == 4 || !s.generic);
                CHECK(k.lds == (size_t)32 * (wgrad_ldt(64 * k.mpw) + wgrad_ldt(16 * k.nt)) * 4);
                bool listed = false;
                for (const Wgrad3Inst& in : WGRAD3_LIST) listed = listed || (in.bmode == k.bmode && in.mpw == k.mpw && in.nt == k.nt);
                CHECK(listed);
            } else {
                CHECK(k.family == 2 && w.bmode != 4 && k.bmode == (w.bmode >= 1 && w.bmode <= 3 ? w.bmode : 0));
                CHECK(k.lds == (size_t)32 * (wgrad_ldt(pad16(w.M)) + wgrad_ldt(pad16(Ng))) * 4);
                bool listed = false;
                for (const Wgrad2Tile& t : WGRAD2_LIST) listed = listed || (t.mpw == k.mpw && t.ntmax == k.nt);
                CHECK(listed);
            }
        }
        // what the launch writes: goff[l] + m ldc + n (m < M, n < N) and the bias slots [gbias[l], gbias[l] + M)
        for (int l = 0; l < w.nlayers; ++l) {
            if (w.ldc == N) take((long)w.goff[l], (long)M * N, x.early);
            else { CHECK(w.ldc > N); for (int m = 0; m < M; ++m) take((long)w.goff[l] + (long)m * w.ldc, N, x.early); }
            if (w.gbias[l] >= 0) take(w.gbias[l], M, x.early);
        }
    }
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    for (size_t i = 1; i < spans.size(); ++i) CHECK(spans[i - 1].hi <= spans[i].lo);      // pairwise disjoint over the whole step
}

static void golden(const char* step, const Launch& x, bool gemm) {
    if (gemm) { printf("GOLDEN %s %s gemm %d %d %d %d %016llx\n", step, x.name.c_str(), x.bmode, x.nlayers, x.t.M, x.t.N, hash_targs(x.t, x.bmode, x.nlayers)); return; }
    const WgradPick& k = x.k;
    if (!k.family) { printf("GOLDEN %s %s refused\n", step, x.name.c_str()); return; }
    printf("GOLDEN %s %s k_wgrad%d %d,%d,%d,%d,%d lds %zu grid %d,%d,%d groups %d nch %d %016llx\n", step, x.name.c_str(), k.family, k.bmode, k.mpw, k.nt, k.family == 3 ? (int)k.two_a : 0,
           k.family == 3 ? k.minw : 0, k.lds, k.grid[0], k.grid[1], k.grid[2], x.w.ncol_groups, x.nch, hash_rec(x.w));
}

static const Launch& find(const std::vector<Launch>& ls, const char* name) {
    for (const Launch& x : ls) if (x.name == name) return x;
    fprintf(stderr, "no launch %s -- %s\n", name, g_ctx.c_str()); exit(1);
}
static bool is3(const Launch& x, int bmode, int mpw, int nt, bool two_a, int minw) {
    return x.k.family == 3 && x.k.bmode == bmode && x.k.mpw == mpw && x.k.nt == nt && x.k.two_a == two_a && x.k.minw == minw;
}

struct NG { const char* name; qpn_config c; };
int main() {
    // {n_quantize, n_aux, n_resch, n_skipch, dilationF_depth, dilationF_repeat, dilationA_depth, dilationA_repeat, kernel_size, upsampling_factor}
    static const NG geoms[] = {      // the named geometries of tests/train_plan_sweep.cpp
        {"tiny", {256, 39, 32, 32, 2, 1, 1, 1, 2, 110}}, {"paper", {256, 39, 64, 256, 4, 1, 4, 1, 2, 110}}, {"default", {256, 39, 512, 256, 4, 3, 4, 1, 2, 110}},
        {"deep64", {256, 39, 64, 256, 10, 3, 4, 1, 2, 110}}, {"paper_aux7", {256, 7, 64, 256, 4, 1, 4, 1, 2, 110}}, {"paper_aux80", {256, 80, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_up0", {256, 39, 64, 256, 4, 1, 4, 1, 2, 0}}, {"paper_up8", {256, 39, 64, 256, 4, 1, 4, 1, 2, 8}}, {"paper_q128", {128, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_q64", {64, 39, 64, 256, 4, 1, 4, 1, 2, 110}}, {"all_adaptive", {256, 39, 64, 256, 0, 0, 4, 2, 2, 110}}, {"all_fixed", {256, 39, 64, 256, 4, 2, 0, 0, 2, 110}},
        {"c160", {256, 39, 160, 256, 2, 1, 2, 1, 2, 110}},
    };
    static const int wide[][3] = {{16, 16, 16}, {48, 80, 48}, {80, 48, 96}, {112, 144, 80}, {32, 16, 64}, {128, 112, 192}, {64, 48, 32}, {64, 16, 256}, {64, 272, 144}};      // TRAIN_CSQ: n_resch, n_skipch, n_quantize
    const int n_named = (int)(sizeof(geoms) / sizeof(geoms[0])), n_wide = (int)(sizeof(wide) / sizeof(wide[0]));
    long n_gemm_steps = 0;
    for (int gi = 0; gi < n_named + n_wide; ++gi) {
        const bool named = gi < n_named;
        const qpn_config c = named ? geoms[gi].c : qpn_config{wide[gi - n_named][2], 39, wide[gi - n_named][0], wide[gi - n_named][1], 2, 1, 2, 1, 2, 110};
        const std::string name = named ? geoms[gi].name : "w" + std::to_string(c.n_resch) + "_" + std::to_string(c.n_skipch) + "_" + std::to_string(c.n_quantize);
        Geom g;
        g_ctx = name;
        CHECK(qpn_build_geom(&c, &g) == QPN_OK);
        for (int B = 1; B <= 2; ++B) for (int knob = 0; knob < K_COUNT; ++knob) {
            const std::string step = name + "/B" + std::to_string(B) + "/" + KNOB_NAMES[knob];
            g_ctx = step;
            Step s;
            if (!make_step(g, B, knob, s)) { CHECK(knob == K_GEMM && (g.C % 32 || g.S % 32 || g.Q % 32)); continue; }      // train_plan refuses the GEMM path: widths off the 32 grid
            n_gemm_steps += knob == K_GEMM;
            const std::vector<Launch> ls = step_launches(s);
            // the tile path trains every width class (multiples of 16); column groups and row blocks bring every record of these geometries
            // inside a kernel's tile budget, the wide stacks included (which train_init sends to the GEMM step) -- nothing is refused
            check_step(s, ls, false);
            if (named) for (const Launch& x : ls) golden(step.c_str(), x, s.gemm);
        }
        if (named) printf("NAMED %s\n", name.c_str()); else printf("CHECKED %s\n", name.c_str());
    }
    {   // ---- the instances bench.py names for the paper geometry (PG_KERNELS)
        Geom g; Step s;
        CHECK(qpn_build_geom(&geoms[1].c, &g) == QPN_OK);
        g_ctx = "pins: paper default"; CHECK(make_step(g, 2, K_DEFAULT, s));
        std::vector<Launch> ls = step_launches(s);
        CHECK(is3(find(ls, "w1.0"), 3, 2, 8, false, 1) && is3(find(ls, "wr.0"), 0, 1, 4, false, 1) && is3(find(ls, "skip.0"), 0, 4, 4, false, 2) && is3(find(ls, "causal.0"), 4, 1, 4, true, 1));
        CHECK(is3(find(ls, "post0.0"), 1, 4, 4, false, 2) && find(ls, "post0.0").w.nlayers == 2 && ls.size() == 5);      // the pair as one two-"layer" launch
        g_ctx = "pins: paper no hoist"; CHECK(make_step(g, 2, K_NO_HOIST, s)); ls = step_launches(s);
        CHECK(is3(find(ls, "w1.0"), 3, 2, 11, false, 1));
        g_ctx = "pins: paper no stack queue"; CHECK(make_step(g, 2, K_NO_STACK_Q, s)); ls = step_launches(s);
        CHECK(is3(find(ls, "wr.0"), 0, 1, 4, true, 1));
        g_ctx = "pins: paper generic"; CHECK(make_step(g, 2, K_GENERIC, s)); ls = step_launches(s);
        for (const Launch& x : ls) CHECK(x.k.family == (x.bmode == 4 ? 3 : 2));

        // ---- boundary cases no GPU test can hold
        g_ctx = "bounds: 24-bit rows"; CHECK(make_step(g, 2, K_DEFAULT, s));
        Wg2 w = wgrad_rec_w1(s.v, s.sl, s.b, s.f);
        w.rowsB = (1 << 24) - 1; CHECK(wgrad_pick(w, 64, false).family == 3);
        w.rowsB = 1 << 24; { const WgradPick k = wgrad_pick(w, 64, false); CHECK(k.family == 2 && k.bmode == 3 && k.mpw == 2 && k.nt == 12); }
        g_ctx = "bounds: 32-bit row x stride";      // a post-net record 512 columns wide: 2^23 rows x 512 = 2^32
        w = wgrad_rec_post(s.v, s.sl, s.b, s.f, 0); w.ldb = w.N = w.Nvalid = w.ldc = 512; w.ncol_groups = 8;
        w.rowsB = (1 << 23) - 1; CHECK(is3(Launch{"", w, wgrad_pick(w, 48, false)}, 1, 4, 4, false, 2));
        w.rowsB = 1 << 23; { const WgradPick k = wgrad_pick(w, 48, false); CHECK(k.family == 2 && k.bmode == 1 && k.mpw == 4 && k.nt == 4); }
        g_ctx = "bounds: a layer without a tap table";
        w = wgrad_rec_w1(s.v, s.sl, s.b, s.f); CHECK(wgrad_pick(w, 64, false).family == 3);
        w.tap_off[1] = -1; CHECK(wgrad_pick(w, 64, false).family == 2);
        g_ctx = "bounds: 272 rows";
        const qpn_config c272 = {144, 39, 64, 272, 2, 1, 2, 1, 2, 110};
        CHECK(qpn_build_geom(&c272, &g) == QPN_OK && make_step(g, 2, K_DEFAULT, s));
        const Wg2 skip272 = wgrad_rec_skip(s.v, s.sl, s.b, s.f);
        const Wg2 blocks[2] = {wgrad_row_block(skip272, 0), wgrad_row_block(skip272, 1)};
        CHECK(wgrad_n_row_blocks(skip272) == 2 && blocks[0].M == 256 && blocks[1].M == 16 && blocks[1].A == blocks[0].A + 256 && blocks[1].goff[1] == blocks[0].goff[1] + 256 * 64 && blocks[1].gbias[0] == blocks[0].gbias[0] + 256 && blocks[1].gbias[1] == -1);
        // the tile budget wgrad_col_groups reads off the k_wgrad2 list
        CHECK(wgrad_col_groups(64, 64) == 1 && wgrad_col_groups(64, 128) == 2 && wgrad_col_groups(128, 176) == 1 && wgrad_col_groups(128, 208) == 2 && wgrad_col_groups(256, 128) == 1 && wgrad_col_groups(256, 272) == 4 && wgrad_col_groups(272, 64) == 1);
    }
    printf("WGRAD_PLAN_SWEEP_OK %ld steps %ld launches %ld refused %ld gemm_steps\n", n_steps, n_launches, n_refused, n_gemm_steps);
    return 0;
}
