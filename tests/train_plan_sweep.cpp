// Stand-alone sweep over the training layout planner (qpnet_amd/csrc/train_plan.h): for a list of geometries, both paths and a few knob settings, every packed block must
// hold each element of its tensor exactly once, every transposed block must be the transpose of its forward block, the gradient map must send the gradient of an element to
// the parameter the forward read it from, and the arena's regions must be disjoint and adjacent where the kernels rely on it.  Prints a hash of every map of the named
// geometries ("GOLDEN ..." lines, compared with tests/golden/train_plan.json by tests/test_train_plan_cpu.py) and the number of plans checked.  The widths that are
// multiples of 16 but not of 32 run the same checks without a hash ("CHECKED ..." lines).  Built with the host sanitizers and run as a child process.
#include "../qpnet_amd/csrc/qpn_geom.h"
#include "../qpnet_amd/csrc/train_plan.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

static char g_err[512] = "";
void qpn_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

static std::string g_ctx;
static long n_plans = 0, n_arenas = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s (line %d) -- %s\n", #cond, __LINE__, g_ctx.c_str()); exit(1); } } while (0)

template <class T> static void golden(const char* name, const char* key, const T* p, size_t n) {      // 64-bit FNV-1a over the values widened to 64 bits, little endian
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { long long v = (long long)p[i]; for (int b = 0; b < 8; ++b) { h ^= (unsigned long long)((v >> (8 * b)) & 0xff); h *= 1099511628211ull; } }
    printf("GOLDEN %s %s %zu %016llx\n", name, key, n, h);
}

struct Range { int64_t lo, n; bool has(int64_t v) const { return v >= lo && v < lo + n; } };
// a logical weight matrix B[k][n] (K x N) with its forward and transposed packed copies, the tensor(s) it is read from and the slab element of its gradient
struct Matrix {
    int K, N;
    std::function<int(int, int)> fwd, tr;               // packed value of B[k][n] in the forward block / of B^T[n][k] in the transposed block
    std::function<bool(int64_t, int, int)> inside;      // the flat index lies in the tensor that (k, n) belongs to
    std::function<int(int, int)> slab;                  // slab element of dB[k][n], or -2 (k_aux_tail's)
};

static void check_plan(const Geom& g, const TrainKnobs& kn, bool use_gemm, const TrainPlan& t) {
    ++n_plans;
    const int C = g.C, S = g.S, Q = g.Q, A = g.A, L = g.L, Ktp = t.Ktp;
    const int64_t NP = g.n_params;
    CHECK(t.rc == QPN_OK && t.use_gemm == use_gemm);
    CHECK(t.hoist == (!use_gemm && C == 64 && g.U >= 16 && A <= 64 && kn.aux_hoist && kn.persist_fwd && kn.persist_bwd));
    CHECK(t.Ap % 4 == 0 && t.Ap >= A && t.Ap < A + 4 && t.Kt == (t.hoist ? 2 * C : 2 * C + t.Ap) && Ktp % 16 == 0 && Ktp >= t.Kt && Ktp < t.Kt + 16 && t.LC == L * C);
    CHECK(t.nch == (kn.wgrad_chunks > 0 ? kn.wgrad_chunks : use_gemm ? 4 : 64));
    const int Kgate = t.hoist ? 2 * C : 2 * C + A;      // gate columns packed with a weight of their own
    const std::vector<int>& map = use_gemm ? t.h_gmap : t.h_wmap;
    CHECK(use_gemm ? t.h_wmap.empty() : t.h_gmap.empty());
    for (int v : map) CHECK(v == -1 || (v >= 0 && v < NP));
    const std::vector<int>& gs = t.h_gsrc;
    CHECK((int64_t)gs.size() == NP);

    // ---- the packed blocks, in the order they were packed: each storage range, and what it must hold
    size_t cursor = 0, n_pad_expected = 0;
    auto frag = [&](int off4, int K, int N) {           // storage of a fragment-ordered K x N block; -> accessor
        CHECK((size_t)off4 * 4 == cursor && K % 16 == 0 && N % 16 == 0); cursor += (size_t)K * N; CHECK(cursor <= map.size());
        std::vector<char> hit((size_t)K * N, 0);        // the fragment order is a bijection of the block
        for (int k = 0; k < K; ++k) for (int n = 0; n < N; ++n) { const size_t p = tp_frag_pos(N, k, n); CHECK(p < hit.size() && !hit[p]); hit[p] = 1; }
        const size_t off = (size_t)off4 * 4;
        return [&map, off, N](int k, int n) { return map[off + tp_frag_pos(N, k, n)]; };
    };
    auto kmajor = [&](long off, int Kp, int Np) {       // storage of a K-major [Kp][Np] block
        CHECK(off >= 0 && (size_t)off == cursor && Np % 128 == 0); cursor += (size_t)Kp * Np; CHECK(cursor <= map.size());
        return [&map, off, Np](int k, int n) { return map[(size_t)off + (size_t)k * Np + n]; };
    };
    std::vector<Matrix> mats;
    std::vector<size_t> block_end;                      // storage end of the two blocks of mats[i]
    std::vector<size_t> block_begin;
    auto qcol = [C](int n) { const int half = n / C, c = n % C; return (c / 64) * 128 + half * 64 + c % 64; };      // GEMM gate block: column of z column n
    for (int l = 0; l < L; ++l) {
        const LayerGeom y = g.layers[l];
        Matrix gate, res;
        block_begin.push_back(cursor);
        gate.K = Kgate; gate.N = 2 * C; res.K = C; res.N = C;
        if (!use_gemm) {
            auto f = frag(t.layers[l].w1_f4, Ktp, 2 * C), ft = frag(t.layers[l].w1t_f4, 2 * C, Ktp);
            gate.fwd = f; gate.tr = [ft](int k, int n) { return ft(n, k); };
            for (int k = Kgate; k < Ktp; ++k) for (int n = 0; n < 2 * C; ++n) CHECK(f(k, n) == -1 && ft(n, k) == -1);
            block_end.push_back(cursor); block_begin.push_back(cursor);
            auto r = frag(t.layers[l].wr_f4, C, C), rt = frag(t.layers[l].wrt_f4, C, C);
            res.fwd = r; res.tr = [rt](int k, int n) { return rt(n, k); };
        } else {
            const TrainGemm& m = t.gm;
            CHECK(m.K1 % 32 == 0 && m.K1 >= 2 * C + A && m.N1g % 128 == 0 && m.N1g >= 2 * C && m.Ktg >= 2 * C + A && m.Cg >= C && m.Sg >= S && m.Qg >= Q && m.LCg >= L * C);
            for (int n = 0; n < 2 * C; ++n) CHECK(qcol(n) < m.N1g && tp_gemm_gate_col(C, qcol(n)) == n);
            auto f = kmajor(m.w1[l], m.K1, m.N1g), ft = kmajor(m.w1t[l], 2 * C, m.Ktg);
            gate.fwd = [f, qcol](int k, int n) { return f(k, qcol(n)); }; gate.tr = [ft](int k, int n) { return ft(n, k); };
            block_end.push_back(cursor); block_begin.push_back(cursor);
            auto r = kmajor(m.wr[l], C, m.Cg), rt = kmajor(m.wrt[l], C, m.Cg);
            res.fwd = r; res.tr = [rt](int k, int n) { return rt(n, k); };
        }
        block_end.push_back(cursor);
        gate.inside = [y, C, A](int64_t v, int k, int n) {
            const int half = n / C;
            const Range conv = {half ? y.wT : y.wS, (int64_t)C * C * (y.adaptive ? 1 : 2)}, convp = {half ? y.wTP : y.wSP, (int64_t)C * C}, aux = {half ? y.auxT : y.auxS, (int64_t)C * A};
            return k < C ? conv.has(v) : k < 2 * C ? (y.adaptive ? convp.has(v) : conv.has(v)) : aux.has(v);
        };
        const int g_w1 = t.slabs.g_w1[l], g_wr = t.slabs.g_wr[l];
        gate.slab = [g_w1, Ktp](int k, int n) { return g_w1 + n * Ktp + k; };
        res.inside = [y, C](int64_t v, int, int) { return Range{y.res, (int64_t)C * C}.has(v); };
        res.slab = [g_wr, C](int k, int n) { return g_wr + n * C + k; };
        mats.push_back(gate); mats.push_back(res);
    }
    {
        Matrix skip, p1, p2;
        skip.K = L * C; skip.N = S; p1.K = S; p1.N = S; p2.K = S; p2.N = Q;
        std::function<int(int, int)> f[6];
        if (!use_gemm) {
            block_begin.push_back(cursor); f[0] = frag(t.ws_f4, L * C, S); f[1] = frag(t.wst_f4, S, L * C); block_end.push_back(cursor);
            block_begin.push_back(cursor); f[2] = frag(t.p1_f4, S, S); f[3] = frag(t.p1t_f4, S, S); block_end.push_back(cursor);
            block_begin.push_back(cursor); f[4] = frag(t.p2_f4, S, Q); f[5] = frag(t.p2t_f4, Q, S); block_end.push_back(cursor);
        } else {
            const TrainGemm& m = t.gm;
            block_begin.push_back(cursor); f[0] = kmajor(m.ws, L * C, m.Sg); f[1] = kmajor(m.wst, S, m.LCg); block_end.push_back(cursor);
            block_begin.push_back(cursor); f[2] = kmajor(m.p1, S, m.Sg); f[3] = kmajor(m.p1t, S, m.Sg); block_end.push_back(cursor);
            block_begin.push_back(cursor); f[4] = kmajor(m.p2, S, m.Qg); f[5] = kmajor(m.p2t, Q, m.Sg); block_end.push_back(cursor);
        }
        skip.fwd = f[0]; skip.tr = [f](int k, int n) { return f[1](n, k); };
        p1.fwd = f[2]; p1.tr = [f](int k, int n) { return f[3](n, k); };
        p2.fwd = f[4]; p2.tr = [f](int k, int n) { return f[5](n, k); };
        skip.inside = [&g, C, S](int64_t v, int k, int) { return Range{g.layers[k / C].skip, (int64_t)S * C}.has(v); };
        const TrainSlabs sl = t.slabs;
        skip.slab = [sl, C](int k, int n) { return sl.g_ws[k / C] + n * C + k % C; };
        p1.inside = [&g, S](int64_t v, int, int) { return Range{g.post1_w, (int64_t)S * S}.has(v); };
        p1.slab = [sl, S](int k, int n) { return sl.g_p1 + n * S + k; };
        p2.inside = [&g, S, Q](int64_t v, int, int) { return Range{g.post2_w, (int64_t)Q * S}.has(v); };
        p2.slab = [sl, S](int k, int n) { return sl.g_p2 + n * S + k; };
        mats.push_back(skip); mats.push_back(p1); mats.push_back(p2);
    }
    CHECK(cursor == map.size() && block_end.size() == mats.size());
    std::vector<int> stamp((size_t)NP, -1);             // which matrix a flat index was seen in: within one block every element appears once
    for (size_t i = 0; i < mats.size(); ++i) {
        const Matrix& m = mats[i];
        for (int k = 0; k < m.K; ++k) for (int n = 0; n < m.N; ++n) {
            const int v = m.fwd(k, n);
            CHECK(v >= 0 && v < NP && m.inside(v, k, n) && stamp[v] != (int)i);
            stamp[v] = (int)i;
            CHECK(m.tr(k, n) == v);                      // the transposed block is the exact transpose
            CHECK(gs[v] == m.slab(k, n));                // the gradient of (k, n) is reduced into the index the forward read
        }
        // everything else in the two blocks' storage is padding, and only padding is -1
        size_t minus = 0;
        for (size_t p = block_begin[i]; p < block_end[i]; ++p) minus += map[p] == -1;
        CHECK(minus == block_end[i] - block_begin[i] - 2 * (size_t)m.K * m.N);
        n_pad_expected += minus;
    }
    CHECK((size_t)std::count(map.begin(), map.end(), -1) == n_pad_expected);
    if (!use_gemm && t.hoist) CHECK(n_pad_expected == 0);

    // ---- the expected state of every flat index: fed by a slab (0), zeroed (-1), the aux tail's (-2)
    std::vector<signed char> want((size_t)NP, 0);
    auto mark = [&](int64_t lo, int64_t n, int st) { CHECK(lo >= 0 && lo + n <= NP); for (int64_t i = lo; i < lo + n; ++i) want[(size_t)i] = (signed char)st; };
    if (t.hoist) { for (int l = 0; l < L; ++l) { mark(g.layers[l].auxS, (int64_t)C * A, -2); mark(g.layers[l].auxT, (int64_t)C * A, -2); } mark(g.up_w, g.U, -2); }
    else if (g.U > 0) mark(g.up_w, g.U, -1);
    if (g.U > 0) mark(g.up_b, 1, -1);
    if (t.slabs.g_cw < 0) { CHECK(t.slabs.g_cb < 0); mark(g.causal_w, (int64_t)C * Q * 2, -1); mark(g.causal_b, C, -1); }
    CHECK((t.slabs.g_cw >= 0) == (C == 64 && Q % 128 == 0 && !use_gemm));
    size_t n_fed = 0, n_zero = 0;
    for (int64_t i = 0; i < NP; ++i) {
        const int s = gs[(size_t)i];
        CHECK(s >= -2 && s < t.gstage);
        CHECK((s >= 0 ? 0 : s) == want[(size_t)i]);
        n_fed += s >= 0; n_zero += s == -1;
    }
    if (!t.hoist) for (int l = 0; l < L; ++l) for (int n = 0; n < 2 * C; ++n) for (int a = 0; a < A; ++a)      // (not hoisted: the aux columns are gate columns like the others -- checked above; hoisted: -2)
        CHECK(gs[(n / C ? g.layers[l].auxT : g.layers[l].auxS) + (int64_t)(n % C) * A + a] == t.slabs.g_w1[l] + n * Ktp + 2 * C + a);

    // ---- packed biases
    CHECK((int)t.h_bstart.size() == t.n_bias + 1 && t.h_bstart[0] == 0 && t.h_bstart[t.n_bias] == (int)t.h_blist.size());
    for (int i = 0; i < t.n_bias; ++i) CHECK(t.h_bstart[i] <= t.h_bstart[i + 1]);
    CHECK(t.n_bias == L * 3 * C + 2 * S + Q);
    std::vector<char> listed((size_t)NP, 0);
    auto bias_is = [&](int packed, std::vector<int64_t> flats, int slab) {      // packed bias `packed` sums exactly these, and they share gradient `slab`
        CHECK(packed >= 0 && packed < t.n_bias && t.h_bstart[packed + 1] - t.h_bstart[packed] == (int)flats.size());
        for (size_t j = 0; j < flats.size(); ++j) {
            const int v = t.h_blist[(size_t)t.h_bstart[packed] + j];
            CHECK(v >= 0 && v < NP && v == flats[j] && !listed[v]); listed[v] = 1;
            CHECK(gs[v] == slab);
        }
    };
    for (int l = 0; l < L; ++l) {
        const LayerGeom& y = g.layers[l];
        CHECK(t.layers[l].adaptive == y.adaptive && t.layers[l].dilation == y.dilation && t.ag.bias1[l] == t.layers[l].bias1 && t.ag.auxS[l] == y.auxS && t.ag.auxT[l] == y.auxT);
        for (int n = 0; n < 2 * C; ++n) {
            const int half = n / C, r = n % C;
            std::vector<int64_t> f = {(half ? y.bT : y.bS) + r, (half ? y.auxTb : y.auxSb) + r};
            if (y.adaptive) f.push_back((half ? y.bTP : y.bSP) + r);
            bias_is(t.layers[l].bias1 + n, f, t.slabs.g_b1[l] + n);
        }
        for (int n = 0; n < C; ++n) bias_is(t.layers[l].biasr + n, {y.resb + n}, t.slabs.g_br[l] + n);
    }
    for (int n = 0; n < S; ++n) { std::vector<int64_t> f; for (int l = 0; l < L; ++l) f.push_back(g.layers[l].skipb + n); bias_is(t.bias_s + n, f, t.slabs.g_bs + n); }      // every skip bias of every layer
    for (int n = 0; n < S; ++n) bias_is(t.bias_p1 + n, {g.post1_b + n}, t.slabs.g_bp1 + n);
    for (int n = 0; n < Q; ++n) bias_is(t.bias_p2 + n, {g.post2_b + n}, t.slabs.g_bp2 + n);
    CHECK((size_t)std::count(listed.begin(), listed.end(), 1) == t.h_blist.size());

    // ---- causal table: its map is a permutation of the causal weight, and (where a slab holds its gradient) consistent with it
    CHECK(t.h_ctmap.size() == (size_t)2 * Q * C);
    for (int tp = 0; tp < 2; ++tp) for (int q = 0; q < Q; ++q) for (int c = 0; c < C; ++c) {
        const int v = t.h_ctmap[((size_t)tp * Q + q) * C + c];
        CHECK(v == g.causal_w + ((int64_t)c * Q + q) * 2 + tp && !listed[v]); listed[v] = 1;
        if (t.slabs.g_cw >= 0) CHECK(gs[v] == t.slabs.g_cw + tp * C * Q + c * Q + q);
    }
    if (t.slabs.g_cw >= 0) for (int c = 0; c < C; ++c) CHECK(gs[g.causal_b + c] == t.slabs.g_cb + c);

    // ---- slabs: disjoint, aligned, inside [0, gstage); the early range holds exactly the skip, skip-bias and post-net blocks
    struct Blk { int off, n; bool early; };
    std::vector<Blk> blks;
    const TrainSlabs& sl = t.slabs;
    for (int l = 0; l < L; ++l) { blks.push_back({sl.g_w1[l], 2 * C * Ktp, false}); blks.push_back({sl.g_b1[l], 2 * C, false}); blks.push_back({sl.g_wr[l], C * C, false});
                                  blks.push_back({sl.g_br[l], C, false}); blks.push_back({sl.g_ws[l], S * C, true}); }
    blks.push_back({sl.g_bs, S, true}); blks.push_back({sl.g_p1, S * S, true}); blks.push_back({sl.g_bp1, S, true}); blks.push_back({sl.g_p2, Q * S, true}); blks.push_back({sl.g_bp2, Q, true});
    if (sl.g_cw >= 0) { blks.push_back({sl.g_cw, 2 * C * Q, false}); blks.push_back({sl.g_cb, C, false}); }
    std::sort(blks.begin(), blks.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
    for (size_t i = 0; i < blks.size(); ++i) {
        const Blk& b = blks[i];
        CHECK(b.off >= 0 && b.off % 64 == 0 && b.off + b.n <= t.gstage && (i + 1 == blks.size() || b.off + b.n <= blks[i + 1].off));
        CHECK(b.early ? (b.off >= sl.g_early0 && b.off + b.n <= sl.g_early1) : (b.off + b.n <= sl.g_early0 || b.off >= sl.g_early1));
    }
    const bool tail = g.post1_b == g.post1_w + (int64_t)S * S && g.post2_w == g.post1_b + S && g.post2_b == g.post2_w + (int64_t)Q * S && g.post2_b + Q == NP;
    CHECK(t.early_first == (tail ? g.post1_w : -1));

    // ---- the CSR inverse of the gradient map and the zero list
    CHECK(t.gdst_start.size() == (size_t)t.gstage + 1 && t.gdst_start[0] == 0 && (size_t)t.gdst_start[t.gstage] == n_fed && t.gdst_list.size() == n_fed + 1);
    std::fill(listed.begin(), listed.end(), 0);
    for (int s = 0; s < t.gstage; ++s) {
        CHECK(t.gdst_start[s] <= t.gdst_start[s + 1]);
        for (int j = t.gdst_start[s]; j < t.gdst_start[s + 1]; ++j) { const int i = t.gdst_list[j]; CHECK(i >= 0 && i < NP && gs[i] == s && !listed[i]); listed[i] = 1; }
    }
    CHECK(t.gzero.size() == n_zero);
    for (int i : t.gzero) { CHECK(i >= 0 && i < NP && gs[i] == -1 && !listed[i]); listed[i] = 1; }      // (with the -2 entries the three sets partition [0, n_params))
}

static void check_arena(const Geom& g, const TrainPlan& t, int B, int N1, int BL, int nfr, bool touch) {
    ++n_arenas;
    const TrainArena a = train_arena(t, g, B, N1, BL, nfr);
    const int C = g.C, S = g.S, L = g.L;
    auto r64 = [](size_t n) { return (n + 63) & ~(size_t)63; };
    struct R { size_t off, n; };
    std::vector<R> rs;
    for (int i = 0; i < TA_COUNT; ++i) {
        const bool want = i == TA_G ? t.use_gemm : (i == TA_PA || i == TA_DPA || i == TA_EB || i == TA_WJ || i == TA_GW) ? t.hoist : true;
        CHECK(a.r[i].on == want);
        if (a.r[i].on) { CHECK(a.r[i].off % 64 == 0 && a.r[i].off + a.r[i].n <= a.total); rs.push_back({a.r[i].off, a.r[i].n}); }
        else { float none = 0.f; CHECK(a.at(&none, i) == nullptr); }
    }
    std::sort(rs.begin(), rs.end(), [](const R& x, const R& y) { return x.off < y.off; });
    for (size_t i = 0; i + 1 < rs.size(); ++i) CHECK(rs[i].off + rs[i].n <= rs[i + 1].off);
    CHECK(a.total % 64 == 0);
    const size_t nDX = (size_t)B * N1 * C, nS = (size_t)B * BL * S;
    CHECK(a.r[TA_X].n == (size_t)(L + 1) * nDX && a.r[TA_SG].n == (size_t)L * nDX && a.r[TA_TH].n == a.r[TA_SG].n && a.r[TA_DZ].n == 2 * (size_t)L * nDX);
    CHECK(a.r[TA_DXA].n == (size_t)(L + 1) * nDX && a.r[TA_DXB].n == a.r[TA_DXA].n && a.r[TA_DXB].off == a.r[TA_DXA].off + r64(a.r[TA_DXA].n));      // one memset clears both
    CHECK(a.r[TA_S0].n == nS + 96 * (size_t)S && a.r[TA_Y0].n == nS + 96 * (size_t)S && a.r[TA_DS0].n == nS && a.r[TA_DY0].n == nS);                  // the tail of one 80-row tile
    CHECK(a.r[TA_HUP].n == (t.hoist ? 64 : (size_t)B * N1 * t.Ap) && a.r[TA_DHUP].n == a.r[TA_HUP].n && a.r[TA_DGS].n == (size_t)B * BL * L * C);
    CHECK(a.r[TA_SLAB].n == (size_t)t.nch * t.gstage && a.r[TA_XC].n == (size_t)B * (N1 + 1) && a.r[TA_SCRATCH].n == (size_t)B * 1024 * 256);
    if (t.use_gemm) CHECK(a.r[TA_G].n == (size_t)L * nDX);
    if (t.hoist) {
        CHECK(a.r[TA_PA].n == (size_t)L * B * (nfr + 1) * 2 * C && a.r[TA_DPA].n == a.r[TA_PA].n && a.r[TA_EB].off == a.r[TA_DPA].off + a.r[TA_DPA].n);   // EB directly behind DPA
        CHECK(a.r[TA_EB].n == (size_t)L * TR_EB_SLOTS * 2 * C && a.r[TA_WJ].n == 2 * (size_t)(N1 + 16) && a.r[TA_GW].n == (size_t)L * B * N1);
    }
    const TrainArena b = train_arena(t, g, B, N1, BL, nfr);      // the sizing pass and the carving pass are the same call
    CHECK(b.total == a.total);
    for (int i = 0; i < TA_COUNT; ++i) CHECK(b.r[i].on == a.r[i].on && b.r[i].off == a.r[i].off && b.r[i].n == a.r[i].n);
    if (touch) {                                                  // a real buffer of `total` floats holds every region (AddressSanitizer watches its ends)
        std::vector<float> buf(a.total);
        for (int i = 0; i < TA_COUNT; ++i) if (a.r[i].on && a.r[i].n) { float* p = a.at(buf.data(), i); CHECK(p == buf.data() + a.r[i].off); p[0] = 1.f; p[a.r[i].n - 1] = 1.f; }
    }
}

static TrainKnobs default_knobs() { TrainKnobs k = {}; k.aux_hoist = k.persist_fwd = k.persist_bwd = true; return k; }

struct NG { const char* name; qpn_config c; };
int main() {
    // {n_quantize, n_aux, n_resch, n_skipch, dilationF_depth, dilationF_repeat, dilationA_depth, dilationA_repeat, kernel_size, upsampling_factor}
    static const NG geoms[] = {
        {"tiny", {256, 39, 32, 32, 2, 1, 1, 1, 2, 110}},                 // TINY, PAPER, DEFAULT, DEEP64 of qpnet_amd/config.py
        {"paper", {256, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"default", {256, 39, 512, 256, 4, 3, 4, 1, 2, 110}},
        {"deep64", {256, 39, 64, 256, 10, 3, 4, 1, 2, 110}},
        {"paper_aux7", {256, 7, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_aux80", {256, 80, 64, 256, 4, 1, 4, 1, 2, 110}},        // n_aux > 64: no hoist
        {"paper_up0", {256, 39, 64, 256, 4, 1, 4, 1, 2, 0}},            // no upsampling kernel
        {"paper_up8", {256, 39, 64, 256, 4, 1, 4, 1, 2, 8}},            // U < 16: no hoist
        {"paper_q128", {128, 39, 64, 256, 4, 1, 4, 1, 2, 110}},         // causal slab on ...
        {"paper_q64", {64, 39, 64, 256, 4, 1, 4, 1, 2, 110}},           // ... and off
        {"all_adaptive", {256, 39, 64, 256, 0, 0, 4, 2, 2, 110}},
        {"all_fixed", {256, 39, 64, 256, 4, 2, 0, 0, 2, 110}},
        {"c160", {256, 39, 160, 256, 2, 1, 2, 1, 2, 110}},              // GEMM path, not a power of two
    };
    for (const NG& ng : geoms) for (int gemm = 0; gemm < 2; ++gemm) for (int knob = 0; knob < 4; ++knob) {
        Geom g;
        g_ctx = std::string(ng.name) + (gemm ? "/gemm" : "/tile") + " knob " + std::to_string(knob);
        CHECK(qpn_build_geom(&ng.c, &g) == QPN_OK);
        TrainKnobs kn = default_knobs();
        if (knob == 1) kn.aux_hoist = false;
        if (knob == 2) kn.persist_fwd = false;
        if (knob == 3) kn.wgrad_chunks = 8;
        const TrainPlan t = train_plan(g, kn, gemm != 0);
        check_plan(g, kn, gemm != 0, t);
        // arenas: B N1 C a multiple of 64 or not (n_resch 32 / 160 with an odd row count), batch_length 1, hoist on and off (the knobs and the path)
        static const int grid[][3] = {{1, 40, 1}, {1, 1237, 500}, {3, 1237, 1}, {3, 1237, 500}, {2, 64, 64}};
        for (const auto& c : grid) check_arena(g, t, c[0], c[1], c[2], t.hoist ? (c[1] + g.U - 1) / g.U + 1 : 0, c[1] == 40 && g.C == 32);
        if (knob == 0) {
            const std::string name = std::string(ng.name) + (gemm ? "/gemm" : "/tile");
            const char* nm = name.c_str();
            golden(nm, "wmap", t.h_wmap.data(), t.h_wmap.size()); golden(nm, "gmap", t.h_gmap.data(), t.h_gmap.size());
            golden(nm, "bstart", t.h_bstart.data(), t.h_bstart.size()); golden(nm, "blist", t.h_blist.data(), t.h_blist.size());
            golden(nm, "gsrc", t.h_gsrc.data(), t.h_gsrc.size()); golden(nm, "gdst_start", t.gdst_start.data(), t.gdst_start.size());
            golden(nm, "gdst_list", t.gdst_list.data(), t.gdst_list.size()); golden(nm, "gzero", t.gzero.data(), t.gzero.size());
            golden(nm, "ctmap", t.h_ctmap.data(), t.h_ctmap.size());
            std::vector<long long> v;
            const TrainSlabs& sl = t.slabs;
            for (int l = 0; l < g.L; ++l) for (long long x : {sl.g_w1[l], sl.g_b1[l], sl.g_wr[l], sl.g_br[l], sl.g_ws[l]}) v.push_back(x);
            for (long long x : {sl.g_bs, sl.g_p1, sl.g_bp1, sl.g_p2, sl.g_bp2, sl.g_early0, sl.g_early1, sl.g_cw, sl.g_cb, t.gstage, t.nch}) v.push_back(x);
            golden(nm, "slabs", v.data(), v.size()); v.clear();
            const TrainGemm& m = t.gm;
            for (long long x : {m.K1, m.N1g, m.Cg, m.Sg, m.Qg, m.LCg, m.Ktg}) v.push_back(x);
            for (int l = 0; l < g.L; ++l) for (long long x : {m.w1[l], m.w1t[l], m.wr[l], m.wrt[l]}) v.push_back(x);
            for (long long x : {m.ws, m.wst, m.p1, m.p1t, m.p2, m.p2t}) v.push_back(x);
            golden(nm, "gemm", v.data(), v.size()); v.clear();
            for (long long x : {(int)t.hoist, t.Ap, t.Kt, t.Ktp, t.LC}) v.push_back(x);
            for (int l = 0; l < g.L; ++l) { const TrainPlanLayer& y = t.layers[l];
                                            for (long long x : {y.adaptive, y.dilation, y.w1_f4, y.wr_f4, y.w1t_f4, y.wrt_f4, y.bias1, y.biasr, t.ag.auxS[l], t.ag.auxT[l], t.ag.bias1[l]}) v.push_back(x); }
            for (long long x : {t.ws_f4, t.p1_f4, t.p2_f4, t.wst_f4, t.p1t_f4, t.p2t_f4, t.bias_s, t.bias_p1, t.bias_p2, t.n_bias}) v.push_back(x);
            v.push_back(t.early_first);
            golden(nm, "params", v.data(), v.size()); v.clear();
            const TrainArena a = train_arena(t, g, 3, 1237, 500, 13);      // the arena of one fixed call: every region's offset (-1: not carved), then the end of the list
            for (int i = 0; i < TA_COUNT; ++i) v.push_back(a.r[i].on ? (long long)a.r[i].off : -1);
            v.push_back((long long)a.total);
            golden(nm, "arena", v.data(), v.size());
        }
    }
    // ---- widths that are multiples of 16 but not of 32 (tests/test_width_classes_gpu.py runs them on the kernels): the invariant checks alone.  They get no golden
    // hash -- tests/golden/train_plan.json comes from the code in front of the planner, which nobody ran at these widths -- and are printed as "CHECKED name"
    long n_checked = 0;
    static const int wide[][3] = {{16, 16, 16}, {48, 80, 48}, {80, 48, 96}, {112, 144, 80}, {32, 16, 64}, {128, 112, 192}, {64, 48, 32}, {64, 16, 256}, {64, 272, 144}};      // n_resch, n_skipch, n_quantize
    for (const auto& w : wide) {
        const qpn_config c = {w[2], 39, w[0], w[1], 2, 1, 2, 1, 2, 110};
        const std::string name = "w" + std::to_string(w[0]) + "_" + std::to_string(w[1]) + "_" + std::to_string(w[2]);
        Geom g;
        g_ctx = name;
        CHECK(qpn_build_geom(&c, &g) == QPN_OK);
        for (int knob = 0; knob < 4; ++knob) {
            g_ctx = name + "/tile knob " + std::to_string(knob);
            TrainKnobs kn = default_knobs();
            if (knob == 1) kn.aux_hoist = false;
            if (knob == 2) kn.persist_fwd = false;
            if (knob == 3) kn.wgrad_chunks = 8;
            const long before = n_plans;
            const TrainPlan t = train_plan(g, kn, false);
            check_plan(g, kn, false, t);
            n_plans = before; ++n_checked;
            CHECK(t.hoist == (w[0] == 64 && knob != 1 && knob != 2));      // the paper-width stacks keep the frame-rate aux path whatever S and Q are
            // arenas: B N1 C and B BL S no multiples of 64 at the narrow widths; the smallest one is carved out of a real buffer
            static const int grid[][3] = {{1, 40, 1}, {1, 181, 17}, {2, 500, 298}, {3, 1237, 500}};
            const long a0 = n_arenas;
            for (const auto& a : grid) check_arena(g, t, a[0], a[1], a[2], t.hoist ? (a[1] + g.U - 1) / g.U + 1 : 0, a[1] == 40);
            n_arenas = a0;
        }
        g_ctx = name + "/gemm";      // none of them is a multiple of 32 in all three: the GEMM path refuses every one
        CHECK(train_plan(g, default_knobs(), true).rc == QPN_EINVAL && std::string(g_err) == "the GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32");
        printf("CHECKED %s/tile\n", name.c_str());
    }
    {   // the refusals: their codes and messages, before anything is built
        g_ctx = "refusals";
        Geom g;
        const qpn_config c72 = {64, 39, 72, 72, 2, 1, 2, 1, 2, 110}, c144 = {64, 39, 144, 144, 2, 1, 2, 1, 2, 110};      // decode takes n_resch 72 (test_width_classes_gpu.py); 144 is a multiple of 16 and trains on the tile path only
        CHECK(qpn_build_geom(&c72, &g) == QPN_OK);
        CHECK(train_plan(g, default_knobs(), false).rc == QPN_EINVAL && std::string(g_err) == "training kernels need n_resch, n_skipch, n_quantize multiples of 16");
        CHECK(qpn_build_geom(&c144, &g) == QPN_OK);
        CHECK(train_plan(g, default_knobs(), true).rc == QPN_EINVAL && std::string(g_err) == "the GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32");
    }
    {
        g_ctx = "refusals (named geometries)";
        Geom g;
        const qpn_config c24 ={256, 39, 24, 32, 2, 1, 1, 1, 2, 110}, c48 = {256, 39, 48, 64, 2, 1, 1, 1, 2, 110}, ok = {256, 39, 32, 32, 2, 1, 1, 1, 2, 110};
        CHECK(qpn_build_geom(&c24, &g) == QPN_OK);
        CHECK(train_plan(g, default_knobs(), false).rc == QPN_EINVAL && std::string(g_err) == "training kernels need n_resch, n_skipch, n_quantize multiples of 16");
        CHECK(qpn_build_geom(&c48, &g) == QPN_OK);
        CHECK(train_plan(g, default_knobs(), false).rc == QPN_OK);
        CHECK(train_plan(g, default_knobs(), true).rc == QPN_EINVAL && std::string(g_err) == "the GEMM training path needs n_resch, n_skipch, n_quantize multiples of 32");
        CHECK(qpn_build_geom(&ok, &g) == QPN_OK);
        g.n_params = (int64_t)1 << 31;                   // (no buildable geometry is this large: the planner must refuse before it sizes anything by it)
        const TrainPlan t = train_plan(g, default_knobs(), false);
        CHECK(t.rc == QPN_EINVAL && t.h_gsrc.empty() && std::string(g_err).find("32 bits") != std::string::npos);
    }
    printf("TRAIN_PLAN_SWEEP_OK %ld plans %ld arenas %ld checked\n", n_plans, n_arenas, n_checked);
    return 0;
}
