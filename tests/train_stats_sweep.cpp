// train_stats_sweep.cpp -- CPU check of the per-tensor statistics planner (qpnet_amd/csrc/train_stats_plan.h): includes only that header, built with
// -fsanitize=address,undefined and run as a child process by tests/test_tensor_stats_cpu.py.
//   * for the tables of real geometries (argv[1]: one line "name n_tensors end ..." each, written by the test from the configurations' parameter layout) and for
//     adversarial ones, the items tile every tensor exactly once and in order, none exceeds QPN_STATS_ITEM or crosses a tensor, only a tensor's last item is short,
//     and first_item names exactly the items inside each tensor;
//   * every rejection rule rejects, naming its argument.
#include "../qpnet_amd/csrc/train_stats_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static long g_tables = 0, g_items = 0, g_rejects = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static void check_table(const std::vector<int64_t>& end) {
    char err[256] = "";
    const int nt = (int)end.size();
    CHECK(stats_table_check(end.back(), nt, end.data(), err, sizeof(err)));
    const StatsPlan p = stats_plan_build(nt, end.data());
    CHECK(p.n == end.back() && p.tensor_end == end && p.first_item.size() == end.size() + 1);
    CHECK(p.first_item[0] == 0 && (size_t)p.first_item[(size_t)nt] == p.items.size());
    CHECK(p.same_table(nt, end.data()));
    int64_t at = 0;                                              // the next element no item has covered yet
    size_t i = 0;
    for (int t = 0; t < nt; ++t) {
        const int64_t lo = t > 0 ? end[(size_t)t - 1] : 0, hi = end[(size_t)t];
        CHECK((size_t)p.first_item[(size_t)t] == i && p.first_item[(size_t)t + 1] > p.first_item[(size_t)t]);
        CHECK(p.first_item[(size_t)t + 1] - p.first_item[(size_t)t] == stats_items_of(hi - lo));
        for (; i < (size_t)p.first_item[(size_t)t + 1]; ++i) {
            const StatsItem& it = p.items[i];
            CHECK(it.begin == at && it.end > it.begin);                        // exactly once, in order
            CHECK(it.end - it.begin <= QPN_STATS_ITEM);
            CHECK(it.begin >= lo && it.end <= hi);                              // inside tensor t
            CHECK(it.end == hi || it.end - it.begin == QPN_STATS_ITEM);         // only the last item of a tensor is short
            at = it.end;
        }
        CHECK(at == hi);
    }
    CHECK(i == p.items.size() && at == p.n);
    ++g_tables; g_items += (long)p.items.size();
}

static void reject(const char* word, int64_t n, int nt, const int64_t* end) {
    char err[256] = "";
    CHECK(!stats_table_check(n, nt, end, err, sizeof(err)));
    if (!strstr(err, word)) { printf("FAILED: rejection message '%s' does not name '%s'\n", err, word); exit(1); }
    ++g_rejects;
}

int main(int argc, char** argv) {
    // the real tables
    long real = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        CHECK(f != nullptr);
        char name[64];
        int nt = 0;
        while (fscanf(f, "%63s %d", name, &nt) == 2) {
            CHECK(nt >= 1 && nt <= QPN_STATS_MAX_TENSORS);
            std::vector<int64_t> end((size_t)nt);
            for (int t = 0; t < nt; ++t) { long long e = 0; CHECK(fscanf(f, "%lld", &e) == 1); end[(size_t)t] = e; }
            check_table(end);
            printf("TABLE %s %d tensors %lld elements\n", name, nt, (long long)end.back());
            ++real;
        }
        fclose(f);
    }
    const int64_t I = QPN_STATS_ITEM;
    // adversarial tables
    { std::vector<int64_t> e; for (int64_t t = 1; t <= 1000; ++t) e.push_back(t); check_table(e); }                             // all tensors of size 1
    for (int64_t len : {(int64_t)1, I - 1, I, I + 1, 2 * I - 1, 2 * I, 2 * I + 1, 2 * I + 3, 7 * I + 5}) check_table({len});      // one tensor of length item +- 1 ...
    for (int64_t len : {I - 1, I, I + 1}) check_table({3, 3 + len, 3 + len + 1});                                               // ... and between two small ones, at an odd start
    check_table({1, 2, 112, 115, 371, 371 + 2 * I + 3, 371 + 2 * I + 3 + 64});                                                    // the table of the GPU test
    { std::vector<int64_t> e; int64_t o = 0; for (int t = 0; t < QPN_STATS_MAX_TENSORS; ++t) { o += 1 + (t % 7 == 0 ? I + 1 : 0); e.push_back(o); } check_table(e); }      // 2^20 tensors
    { std::vector<int64_t> e; for (int64_t t = 1; t <= QPN_STATS_MAX_TENSORS; ++t) e.push_back(t); check_table(e); }            // 2^20 tensors of size 1
    // a changed table is not "the same table"
    {
        const int64_t a[3] = {4, 9, 20}, b[3] = {4, 10, 20}, c[2] = {4, 20};
        const StatsPlan p = stats_plan_build(3, a);
        CHECK(p.same_table(3, a) && !p.same_table(3, b) && !p.same_table(2, c));
    }
    // every malformed table is refused
    {
        const int64_t ok[3] = {4, 9, 20};
        reject("h_tensor_end is NULL", 20, 3, nullptr);
        reject("n_tensors", 20, 0, ok);
        reject("n_tensors", 20, -1, ok);
        reject("n_tensors", 20, QPN_STATS_MAX_TENSORS + 1, ok);                  // (refused before the table is read)
        const int64_t zero_first[3] = {0, 9, 20}, neg_first[3] = {-3, 9, 20};
        reject("h_tensor_end[0]", 20, 3, zero_first);
        reject("h_tensor_end[0]", 20, 3, neg_first);
        const int64_t equal[3] = {4, 4, 20}, descending[3] = {4, 3, 20};
        reject("strictly ascending", 20, 3, equal);
        reject("strictly ascending", 20, 3, descending);
        reject("is not n", 21, 3, ok);
        reject("is not n", 19, 3, ok);
        const int64_t huge[1] = {((int64_t)QPN_STATS_MAX_ITEMS + 1) * I};
        reject("work items", huge[0], 1, huge);
    }
    printf("TRAIN_STATS_SWEEP_OK %ld tables %ld real %ld items %ld rejects item %d\n", g_tables, real, g_items, g_rejects, QPN_STATS_ITEM);
    return 0;
}
