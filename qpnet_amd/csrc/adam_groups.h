// adam_groups.h -- parameter groups of the fused Adam step (qpn_adam_groups): the checks of a caller's group table, its normal form and the per-block
// index the kernels start their lookup from.  Pure host arithmetic (plain C++: no HIP, no handle, no globals): train_host.hip uploads what adam_groups_build()
// returns, the kernels of train_bwd.hip read it as adam_groups_lookup() does; tests/adam_groups_sweep.cpp checks all of it on a CPU.
//
// A table cuts the flat parameter vector [0, n) into segments: segment s covers [seg_end[s-1], seg_end[s]) (seg_end[-1] = 0) and belongs to group seg_group[s]
// (0 .. n_groups-1: updated with that group's lr / weight_decay) or is QPN_ADAM_FROZEN (not touched).  Normal form: adjacent segments of one group are one segment.
// block[2b] = the segment that holds element 256 b, block[2b + 1] = that segment's group when the WHOLE block [256 b, 256 b + 256) lies inside it, QPN_ADAM_MIXED
// otherwise.  A block of the Adam launch reads the pair once (one uniform 8-byte load, issued next to the launch's other first loads): in nearly every block that is
// the whole lookup -- the group is block-uniform, no segment is read; only a block a boundary crosses walks forward from its first segment, thread by thread.  No
// search per element, and 8 bytes of table per 256 elements (7168 bytes of traffic).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#define QPN_ADAM_MAX_GROUPS 8
#define QPN_ADAM_FROZEN (-1)
#define QPN_ADAM_MAX_SEGS (1 << 20)      // segments of a caller's table (a model has a few hundred tensors; 2^20 segments are 12 MB of table)
#define QPN_ADAM_BLOCK 256               // elements per block of the Adam launch (k_adam's block size)
#define QPN_ADAM_MIXED (-2147483647 - 1) // block[2b + 1] of a block that holds a segment boundary
#define QPN_ADAM_WG_BLOCKS 4             // consecutive blocks one workgroup of a grouped launch updates (it reads their pairs at once: the index is padded to a multiple)

struct AdamGroupTable {
    int64_t n = 0;                        // elements covered: seg_end.back()
    std::vector<int64_t> seg_end;         // strictly ascending
    std::vector<int32_t> seg_group;       // no two neighbours equal
    std::vector<int32_t> block;           // (n + 255) / 256 pairs {first segment, its group or QPN_ADAM_MIXED}, then {0, QPN_ADAM_FROZEN} pairs up to a multiple of QPN_ADAM_WG_BLOCKS
    bool same_segments(const AdamGroupTable& o) const { return n == o.n && seg_end == o.seg_end && seg_group == o.seg_group; }
};

// the rules of qpn_adam_groups for n_groups > 0 -> true, or false with the offending argument named in err
inline bool adam_groups_check(int n_groups, const float* lr, const float* weight_decay, int64_t n_seg, const int64_t* seg_end, const int32_t* seg_group,
                              char* err, size_t err_len) {
    if (n_groups < 1 || n_groups > QPN_ADAM_MAX_GROUPS) { snprintf(err, err_len, "n_groups must lie in [0, %d] (got %d)", QPN_ADAM_MAX_GROUPS, n_groups); return false; }
    if (!lr) { snprintf(err, err_len, "h_lr is NULL with n_groups > 0"); return false; }
    if (!weight_decay) { snprintf(err, err_len, "h_weight_decay is NULL with n_groups > 0"); return false; }
    if (!seg_end) { snprintf(err, err_len, "h_seg_end is NULL with n_groups > 0"); return false; }
    if (!seg_group) { snprintf(err, err_len, "h_seg_group is NULL with n_groups > 0"); return false; }
    for (int q = 0; q < n_groups; ++q) {
        if (!(lr[q] >= 0.0f) || isinf(lr[q])) { snprintf(err, err_len, "h_lr[%d] must be a finite number >= 0 (got %g)", q, (double)lr[q]); return false; }
        if (!(weight_decay[q] >= 0.0f) || isinf(weight_decay[q])) { snprintf(err, err_len, "h_weight_decay[%d] must be a finite number >= 0 (got %g)", q, (double)weight_decay[q]); return false; }
    }
    if (n_seg < 1 || n_seg > QPN_ADAM_MAX_SEGS) { snprintf(err, err_len, "n_seg must lie in [1, %d] (got %lld)", QPN_ADAM_MAX_SEGS, (long long)n_seg); return false; }
    if (seg_end[0] < 1) { snprintf(err, err_len, "h_seg_end[0] must be >= 1 (got %lld)", (long long)seg_end[0]); return false; }
    bool trainable = false;
    for (int64_t s = 0; s < n_seg; ++s) {
        if (s > 0 && seg_end[s] <= seg_end[s - 1]) {
            snprintf(err, err_len, "h_seg_end must be strictly ascending (h_seg_end[%lld] = %lld after %lld)", (long long)s, (long long)seg_end[s], (long long)seg_end[s - 1]);
            return false;
        }
        if (seg_group[s] < QPN_ADAM_FROZEN || seg_group[s] >= n_groups) {
            snprintf(err, err_len, "h_seg_group[%lld] = %d is neither QPN_ADAM_FROZEN nor a group in [0, %d)", (long long)s, (int)seg_group[s], n_groups);
            return false;
        }
        trainable = trainable || seg_group[s] >= 0;
    }
    if (!trainable) { snprintf(err, err_len, "h_seg_group holds no trainable segment (every segment is QPN_ADAM_FROZEN)"); return false; }
    return true;
}

// a CHECKED table -> its normal form, block still empty (what "the same table as the handle holds" is decided on: the per-step call of a schedule ends here)
inline AdamGroupTable adam_groups_normalise(int64_t n_seg, const int64_t* seg_end, const int32_t* seg_group) {
    AdamGroupTable t;
    for (int64_t s = 0; s < n_seg; ++s) {
        if (!t.seg_group.empty() && t.seg_group.back() == seg_group[s]) t.seg_end.back() = seg_end[s];      // the neighbour's group: one segment
        else { t.seg_end.push_back(seg_end[s]); t.seg_group.push_back(seg_group[s]); }
    }
    t.n = t.seg_end.back();
    return t;
}
// ... and with the per-block index
inline AdamGroupTable adam_groups_build(int64_t n_seg, const int64_t* seg_end, const int32_t* seg_group) {
    AdamGroupTable t = adam_groups_normalise(n_seg, seg_end, seg_group);
    const int64_t nb = (t.n + QPN_ADAM_BLOCK - 1) / QPN_ADAM_BLOCK;
    const int64_t nb_pad = (nb + QPN_ADAM_WG_BLOCKS - 1) / QPN_ADAM_WG_BLOCKS * QPN_ADAM_WG_BLOCKS;
    t.block.assign((size_t)(2 * nb_pad), 0);
    for (int64_t b = nb; b < nb_pad; ++b) t.block[(size_t)(2 * b + 1)] = QPN_ADAM_FROZEN;
    int32_t s = 0;
    for (int64_t b = 0; b < nb; ++b) {
        while (t.seg_end[(size_t)s] <= b * QPN_ADAM_BLOCK) ++s;      // (b * 256 < n = the last end: s stays inside the table)
        const int64_t last = (b + 1) * QPN_ADAM_BLOCK < t.n ? (b + 1) * QPN_ADAM_BLOCK : t.n;      // one past the block's last element
        t.block[(size_t)(2 * b)] = s;
        t.block[(size_t)(2 * b + 1)] = t.seg_end[(size_t)s] >= last ? t.seg_group[(size_t)s] : QPN_ADAM_MIXED;
    }
    return t;
}

// group of element i < n, found as the kernels find it: the block's pair; where the block is mixed, forward from its first segment (seg_end[last] = n > i ends
// the walk inside the table)
inline int32_t adam_groups_lookup(const int64_t* seg_end, const int32_t* seg_group, const int32_t* block, int64_t i) {
    const int64_t b = i / QPN_ADAM_BLOCK;
    if (block[2 * b + 1] != QPN_ADAM_MIXED) return block[2 * b + 1];
    int32_t s = block[2 * b];
    while (seg_end[s] <= i) ++s;
    return seg_group[s];
}
