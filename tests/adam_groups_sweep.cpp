// adam_groups_sweep.cpp -- CPU check of the Adam parameter-group table (qpnet_amd/csrc/adam_groups.h): includes only that header, built with
// -fsanitize=address,undefined and run as a child process by tests/test_adam_groups_cpu.py.
//   * for hand-made and random tables the normalised table + per-block lookup give EVERY element the group the raw table gives it (brute force);
//   * the normal form has no equal neighbours, keeps n, and the block index has one pair per 256 elements: the segment that holds the block's first element, and
//     that segment's group exactly when the whole block lies inside it;
//   * every rejection rule rejects, naming its argument.
#include "../qpnet_amd/csrc/adam_groups.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static long g_tables = 0, g_elements = 0, g_rejects = 0, g_blocks = 0, g_mixed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static const float LR[8] = {1e-3f, 2e-3f, 0.f, 4e-3f, 5e-3f, 6e-3f, 7e-3f, 8e-3f}, WD[8] = {0.f, 1e-2f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.5f};

static void check_table(int n_groups, const std::vector<int64_t>& end, const std::vector<int32_t>& grp) {
    char err[256] = "";
    CHECK(adam_groups_check(n_groups, LR, WD, (int64_t)end.size(), end.data(), grp.data(), err, sizeof(err)));
    const AdamGroupTable t = adam_groups_build((int64_t)end.size(), end.data(), grp.data());
    const int64_t n = end.back();
    CHECK(t.n == n && t.seg_end.size() == t.seg_group.size() && !t.seg_end.empty() && t.seg_end.back() == n);
    CHECK(t.seg_end.size() <= end.size());
    for (size_t s = 1; s < t.seg_end.size(); ++s) CHECK(t.seg_end[s] > t.seg_end[s - 1] && t.seg_group[s] != t.seg_group[s - 1]);
    const size_t nb = (size_t)((n + QPN_ADAM_BLOCK - 1) / QPN_ADAM_BLOCK);
    CHECK(t.block.size() == 2 * ((nb + QPN_ADAM_WG_BLOCKS - 1) / QPN_ADAM_WG_BLOCKS * QPN_ADAM_WG_BLOCKS));      // padded to whole workgroups ...
    for (size_t b = nb; 2 * b < t.block.size(); ++b) CHECK(t.block[2 * b] == 0 && t.block[2 * b + 1] == QPN_ADAM_FROZEN);      // ... with pairs that touch nothing
    size_t scan = 0;
    for (size_t b = 0; b < nb; ++b) {
        const int32_t s = t.block[2 * b];
        const int64_t lo = (int64_t)b * QPN_ADAM_BLOCK, hi = lo + QPN_ADAM_BLOCK < n ? lo + QPN_ADAM_BLOCK : n;
        CHECK(s >= 0 && (size_t)s < t.seg_end.size());
        CHECK(t.seg_end[(size_t)s] > lo && (s == 0 || t.seg_end[(size_t)s - 1] <= lo));
        // uniform exactly when every element of the block has one group in the RAW table
        bool same = true;
        while (end[scan] <= lo) ++scan;
        const int32_t g0 = grp[scan];
        for (size_t r = scan; r < end.size() && (r == scan || end[r - 1] < hi); ++r) same = same && grp[r] == g0;
        CHECK(same ? t.block[2 * b + 1] == g0 : t.block[2 * b + 1] == QPN_ADAM_MIXED);
        ++g_blocks; g_mixed += !same;
    }
    // brute force: the raw table's answer for every element, by a scan of its own
    size_t raw = 0;
    for (int64_t i = 0; i < n; ++i) {
        while (end[raw] <= i) ++raw;
        CHECK(adam_groups_lookup(t.seg_end.data(), t.seg_group.data(), t.block.data(), i) == grp[raw]);
    }
    // building the normal form again changes nothing, and "the same table" is decided on it
    const AdamGroupTable t2 = adam_groups_build((int64_t)t.seg_end.size(), t.seg_end.data(), t.seg_group.data());
    CHECK(t2.same_segments(t) && t2.block == t.block);
    ++g_tables; g_elements += n;
}

static void reject(const char* word, int n_groups, const float* lr, const float* wd, int64_t n_seg, const int64_t* end, const int32_t* grp) {
    char err[256] = "";
    CHECK(!adam_groups_check(n_groups, lr, wd, n_seg, end, grp, err, sizeof(err)));
    if (!strstr(err, word)) { printf("FAILED: rejection does not name %s: %s\n", word, err); exit(1); }
    ++g_rejects;
}

int main() {
    const int32_t F = QPN_ADAM_FROZEN;
    // ---- hand-made tables
    check_table(1, {1}, {0});                                                      // n_seg = 1, n = 1
    check_table(1, {256}, {0});                                                    // one block exactly
    check_table(1, {257}, {0});
    check_table(3, {5003}, {2});
    check_table(2, {1, 2, 3, 4, 5}, {0, 1, 0, F, 1});                              // one-element segments
    check_table(2, {100, 256, 300, 512, 513}, {0, 1, F, 0, 1});                    // segments that end on a block boundary
    {   // many segments inside one block: every element of block 1 a segment of its own
        std::vector<int64_t> e; std::vector<int32_t> g;
        e.push_back(256); g.push_back(0);
        for (int i = 257; i <= 512; ++i) { e.push_back(i); g.push_back(i % 3 == 0 ? F : i % 3 - 1); }
        e.push_back(2000); g.push_back(1);
        check_table(2, e, g);
    }
    check_table(2, {300, 700, 1000}, {F, 0, F});                                    // first and last frozen, the first spanning block 0
    check_table(2, {10, 20, 30, 1000, 1001}, {F, F, 0, 0, F});                      // neighbours of one group (frozen too) merge
    {   // the edge table of the GPU tests
        std::vector<int64_t> e = {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 768, 1024, 1030};
        for (int i = 1031; i <= 1040; ++i) e.push_back(i);
        e.push_back(4096); e.push_back(5003);
        std::vector<int32_t> g;
        for (size_t s = 0; s < e.size(); ++s) g.push_back(e[s] == 768 || e[s] == 5003 ? F : (int32_t)(s % 3));
        check_table(3, e, g);
    }
    // ---- random tables, n up to a few thousand
    for (int it = 0; it < 400; ++it) {
        const int n_groups = 1 + (int)(rnd() % 8);
        const int64_t n = 1 + (int64_t)(rnd() % 4000);
        const unsigned dens = 1 + rnd() % 600;                                      // mean segment length
        std::vector<int64_t> e; std::vector<int32_t> g;
        int64_t pos = 0;
        while (pos < n) {
            int64_t len = 1 + (int64_t)(rnd() % dens);
            if (rnd() % 5 == 0) len = (pos / 256 + 1) * 256 - pos;                  // up to the next block boundary
            pos = pos + len < n ? pos + len : n;
            e.push_back(pos); g.push_back((int32_t)(rnd() % (unsigned)(n_groups + 1)) - 1);
        }
        bool any = false;
        for (int32_t q : g) any = any || q >= 0;
        if (!any) g[rnd() % g.size()] = 0;
        check_table(n_groups, e, g);
    }
    // ---- every rejection rule
    const int64_t e2[2] = {10, 20}; const int32_t g2[2] = {0, F};
    reject("n_groups", 0, LR, WD, 2, e2, g2);
    reject("n_groups", -1, LR, WD, 2, e2, g2);
    reject("n_groups", 9, LR, WD, 2, e2, g2);
    reject("h_lr", 1, nullptr, WD, 2, e2, g2);
    reject("h_weight_decay", 1, LR, nullptr, 2, e2, g2);
    reject("h_seg_end", 1, LR, WD, 2, nullptr, g2);
    reject("h_seg_group", 1, LR, WD, 2, e2, nullptr);
    const float bad[4] = {NAN, INFINITY, -INFINITY, -1e-3f};
    for (float b : bad) {
        float lr[2] = {1e-3f, b}, wd[2] = {0.f, b};
        reject("h_lr[1]", 2, lr, WD, 2, e2, g2);
        reject("h_weight_decay[1]", 2, LR, wd, 2, e2, g2);
    }
    reject("n_seg", 1, LR, WD, 0, e2, g2);
    reject("n_seg", 1, LR, WD, -3, e2, g2);
    reject("n_seg", 1, LR, WD, (int64_t)QPN_ADAM_MAX_SEGS + 1, e2, g2);
    { const int64_t e[2] = {0, 20}; reject("h_seg_end[0]", 1, LR, WD, 2, e, g2); }
    { const int64_t e[2] = {-4, 20}; reject("h_seg_end[0]", 1, LR, WD, 2, e, g2); }
    { const int64_t e[3] = {10, 10, 20}; const int32_t g[3] = {0, F, 0}; reject("strictly ascending", 1, LR, WD, 3, e, g); }
    { const int64_t e[3] = {10, 9, 20}; const int32_t g[3] = {0, F, 0}; reject("strictly ascending", 1, LR, WD, 3, e, g); }
    { const int32_t g[2] = {0, 1}; reject("h_seg_group[1]", 1, LR, WD, 2, e2, g); }
    { const int32_t g[2] = {-2, 0}; reject("h_seg_group[0]", 1, LR, WD, 2, e2, g); }
    { const int32_t g[2] = {F, F}; reject("no trainable segment", 3, LR, WD, 2, e2, g); }
    // (0 is a value like any other, as in torch)
    { const float z[1] = {0.f}; const int64_t e[1] = {7}; const int32_t g[1] = {0}; char err[64]; CHECK(adam_groups_check(1, z, z, 1, e, g, err, sizeof(err))); }
    CHECK(g_mixed > 100 && g_blocks - g_mixed > 100);
    printf("ADAM_GROUPS_SWEEP_OK %ld tables %ld elements %ld rejections (%ld blocks, %ld of them mixed)\n", g_tables, g_elements, g_rejects, g_blocks, g_mixed);
    return 0;
}
