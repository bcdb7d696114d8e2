// train_stats_plan.h -- per-tensor training statistics (qpn_tensor_stats): the checks of a caller's tensor table and the work items of the two launches of
// train_stats.hip.  Pure host arithmetic (plain C++: no HIP, no handle, no globals): train_stats.hip uploads what stats_plan_build() returns,
// tests/train_stats_sweep.cpp checks all of it on a CPU.
//
// A table cuts the flat parameter vector [0, n) into tensors: tensor t covers [tensor_end[t-1], tensor_end[t]) (tensor_end[-1] = 0).  Every tensor is cut,
// from its first element on, into work items of at most QPN_STATS_ITEM elements -- the last one of a tensor may be shorter, no item crosses a tensor.  Items are
// numbered in element order, so tensor t owns the items [first_item[t], first_item[t + 1]).  Pass 1 runs one workgroup per item, pass 2 adds a tensor's
// items in item order: the order of every addition is a function of the table alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>

#define QPN_STATS_ITEM 2048                  // elements per work item: 2 quads of each buffer per thread of a 256-thread workgroup, all 8 loads in flight at once (4 quads: 97 VGPRs, half the occupancy)
#define QPN_STATS_MAX_TENSORS (1 << 20)      // tensors of a caller's table (a model has a few hundred)
#define QPN_STATS_MAX_ITEMS (1 << 24)        // items of a plan (2^35 elements in full items: the item index is a 32-bit grid coordinate)

struct StatsItem { int64_t begin, end; };    // elements [begin, end) of the flat vector, inside one tensor

struct StatsPlan {
    int64_t n = 0;                           // elements covered: tensor_end.back()
    std::vector<int64_t> tensor_end;         // the caller's table
    std::vector<StatsItem> items;            // in element order
    std::vector<int32_t> first_item;         // n_tensors + 1 entries: tensor t owns items [first_item[t], first_item[t + 1])
    bool same_table(int n_tensors, const int64_t* end) const {
        if ((size_t)n_tensors != tensor_end.size()) return false;
        for (int t = 0; t < n_tensors; ++t) if (tensor_end[(size_t)t] != end[t]) return false;
        return true;
    }
};

// items of a tensor of len elements
inline int64_t stats_items_of(int64_t len) { return (len + QPN_STATS_ITEM - 1) / QPN_STATS_ITEM; }

// the table rules of qpn_tensor_stats -> true, or false with the offending argument named in err
inline bool stats_table_check(int64_t n, int n_tensors, const int64_t* tensor_end, char* err, size_t err_len) {
    if (!tensor_end) { snprintf(err, err_len, "h_tensor_end is NULL"); return false; }
    if (n_tensors < 1 || n_tensors > QPN_STATS_MAX_TENSORS) { snprintf(err, err_len, "n_tensors must lie in [1, %d] (got %d)", QPN_STATS_MAX_TENSORS, n_tensors); return false; }
    if (tensor_end[0] < 1) { snprintf(err, err_len, "h_tensor_end[0] must be >= 1 (got %lld)", (long long)tensor_end[0]); return false; }
    int64_t items = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (t > 0 && tensor_end[t] <= tensor_end[t - 1]) {
            snprintf(err, err_len, "h_tensor_end must be strictly ascending (h_tensor_end[%d] = %lld after %lld)", t, (long long)tensor_end[t], (long long)tensor_end[t - 1]);
            return false;
        }
        items += stats_items_of(tensor_end[t] - (t > 0 ? tensor_end[t - 1] : 0));
    }
    if (tensor_end[n_tensors - 1] != n) { snprintf(err, err_len, "h_tensor_end[n_tensors - 1] = %lld is not n = %lld", (long long)tensor_end[n_tensors - 1], (long long)n); return false; }
    if (items > QPN_STATS_MAX_ITEMS) { snprintf(err, err_len, "n = %lld makes %lld work items, more than %d", (long long)n, (long long)items, QPN_STATS_MAX_ITEMS); return false; }
    return true;
}

// a CHECKED table -> its plan
inline StatsPlan stats_plan_build(int n_tensors, const int64_t* tensor_end) {
    StatsPlan p;
    p.tensor_end.assign(tensor_end, tensor_end + n_tensors);
    p.n = tensor_end[n_tensors - 1];
    p.first_item.reserve((size_t)n_tensors + 1);
    int64_t begin = 0;
    for (int t = 0; t < n_tensors; ++t) {
        p.first_item.push_back((int32_t)p.items.size());
        for (; begin < tensor_end[t]; begin += QPN_STATS_ITEM) {
            const int64_t end = begin + QPN_STATS_ITEM < tensor_end[t] ? begin + QPN_STATS_ITEM : tensor_end[t];
            p.items.push_back({begin, end});
        }
        begin = tensor_end[t];
    }
    p.first_item.push_back((int32_t)p.items.size());
    return p;
}
