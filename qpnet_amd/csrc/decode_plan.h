// decode_plan.h -- the launch plan of a decode call: which of the four decode kernels runs and how the batch is split into launches.  Pure host arithmetic (plain
// C++: no HIP, no handle, no globals): decode.hip executes a plan launch by launch, and tests/decode_plan_sweep.cpp checks the invariants of every plan on a CPU.
#pragma once
#include <cstdio>
#define DECODE_COOPB_NU 16      // most utterances a group of the batched cooperative kernel holds (the utterance columns of its tiles)
struct DecodePlanIn {
    int C, S, Q, Cp, Sp, L;                              // geometry (padded widths as in Geom)
    bool single_cu_ok, pipe_supported, coopb_supported;  // per-geometry predicates computed at qpn_create
    bool coopb_fits;                                     // decode_coopb_fits for this call's rings
    int n_cus, pipe_rows, pipe_nu;                       // device facts
    int coop, coopb, pipe; bool generic;                 // the DecodeKnobs that bear on the plan
    int B; bool retry_one_cu; int retry_G;               // the batch and the attempt: false / 0 at the first try, set by decode_plan_retry
};
enum DecodeKind { DECODE_ONE_CU, DECODE_PIPE, DECODE_COOP, DECODE_COOPB };
// Every call is ONE kind of launch over rows handed out longest first: launch i takes rows [i * rows_per_launch, min(B, (i + 1) * rows_per_launch))
struct DecodePlan {
    DecodeKind kind; int launches, rows_per_launch;
    int G;                      // workgroups per utterance (ONE_CU 1, PIPE 5, COOP) or per group (COOPB)
    int per_group;              // PIPE: utterances a five-role group steps alternately in a full launch
    bool needs_ring;            // pitch-tap histories in ring memory (ONE_CU, PIPE); the cooperative kernels keep them in their exchange blocks
};
struct DecodeLaunch { int first, rows, groups, per_group; };      // launch i of a plan: its rows, and how they are grouped (ONE_CU / COOP: a group is an utterance)
// largest power-of-two group size G <= limit of the per-utterance cooperative kernel: the gate and residual row slices are whole 4 KiB tiles; a skip /
// post-net slice may be a fraction of ONE tile (G = 128 / 256 for the C = 512 geometry -- the workgroup takes the tile that holds its one or two rows)
inline int qpn_coop_group_size(const DecodePlanIn& g, int limit) {
    const int rpt = 64 / (g.Cp / 16), rpts = 64 / (g.Sp / 16);
    auto slice_ok = [](int rows, int per_tile) { return rows % per_tile == 0 || (rows < per_tile && per_tile % rows == 0); };
    int best = 1;
    for (int G = 1; G <= limit; G *= 2) {
        if (g.C % G || g.S % G || g.Q % G) break;
        const int CB = g.C / G, SB = g.S / G, QB = g.Q / G;
        if ((2 * CB) % rpt || CB % rpt || !slice_ok(SB, rpt) || !slice_ok(SB, rpts) || !slice_ok(QB, rpts)) break;
        best = G;
    }
    return best;
}
// The batched cooperative kernel reaches the packed weights and a group's exchange block (16 utterances of ring_floats + step vectors, 8-byte granules) with
// 32-bit byte offsets: where either does not fit, the call takes the per-utterance kernel.  ring_floats: the call's pitch-tap rings, all layers.
inline bool decode_coopb_fits(const DecodePlanIn& g, size_t wpk_bytes, long long ring_floats) {
    const long long stride = (ring_floats + (long long)g.L * g.C + 2 * g.S + g.Q + 15) & ~15LL;
    return wpk_bytes < ((size_t)1 << 32) && stride * DECODE_COOPB_NU * 8 < (1LL << 31);
}
inline DecodePlan decode_plan(const DecodePlanIn& in) {
    DecodePlan p = {}; const int B = in.B, n_cus = in.n_cus;
    // several workgroups per utterance when one CU cannot hold the step state (or QPN_DECODE_COOP=<G> asks): by default up to half the CUs (C = 512, B = 1: 96.7 / 91.6 / 93.1 us per sample with G = 64 / 128 / 256)
    int Gmax = in.coop;
    if (!in.single_cu_ok && Gmax == 0) Gmax = n_cus >= 128 ? n_cus / 2 : n_cus;
    if (in.retry_one_cu && in.single_cu_ok) Gmax = 0;
    // wide geometries: the utterances batched into the contractions, up to 16 per group of C / 8 workgroups and as many groups as fit the chip (all
    // workgroups of a launch must be resident together, one per CU); larger batches take several launches of equal size
    if (Gmax > 0 && !in.retry_one_cu && in.retry_G == 0 && in.coopb_supported && in.coopb_fits && in.coopb > 0 && B >= in.coopb && n_cus >= in.C / 8) {
        const int cap = DECODE_COOPB_NU * (n_cus / (in.C / 8));
        p.kind = DECODE_COOPB; p.G = in.C / 8; p.launches = (B + cap - 1) / cap; p.rows_per_launch = (B + p.launches - 1) / p.launches;
    } else if (Gmax > 0) {
        if (B < n_cus && n_cus / B < Gmax) Gmax = n_cus / B;                  // the whole batch in one launch when it fits the chip (quirk: no cap once B >= n_cus)
        if (in.retry_G > 0 && Gmax > in.retry_G) Gmax = in.retry_G;           // retry with fewer workgroups per utterance
        p.kind = DECODE_COOP; p.G = qpn_coop_group_size(in, Gmax < 1 ? 1 : Gmax);
        const int per = n_cus / p.G > 0 ? n_cus / p.G : 1;                     // all workgroups of a launch must be resident together (one per CU)
        p.rows_per_launch = B < per ? B : per; p.launches = (B + per - 1) / per;
    } else {
        p.kind = DECODE_ONE_CU; p.G = 1; p.launches = 1; p.rows_per_launch = B; p.per_group = 1; p.needs_ring = true;
        if (in.retry_one_cu || in.pipe == 0 || !in.pipe_supported || in.generic || in.pipe_rows < 1) return p;
        // five resident workgroups per utterance (decode_pipe.hip), pipe_rows groups per launch.  Beyond that a group takes a second (third) utterance, stepped alternately with
        // the first (a role is busy ~2 us of an utterance's ~8 us step); beyond pipe_nu * pipe_rows rows, equal-sized launches.  Measured step times with 1 / 2 / 3 per group: 8.4 / 10.0 /
        // 15.3 us (profiles/r03_decode_batches.txt); the smallest (launches x step time) wins -- three per group only pays where it saves a launch (97..144 rows on 48 groups)
        static const double step_us[4] = {0.0, 8.4, 10.0, 15.3};
        const int cap = in.pipe_rows; double best = 1e300;
        p.kind = DECODE_PIPE; p.G = 5;
        for (int nu_max = 2; B > cap && nu_max <= in.pipe_nu; ++nu_max) {
            const int nw = (B + nu_max * cap - 1) / (nu_max * cap), per = (B + nw - 1) / nw, nu = (per + cap - 1) / cap;
            if (nw * step_us[nu] < best) { best = nw * step_us[nu]; p.launches = nw; p.rows_per_launch = per; }
        }
        p.per_group = (p.rows_per_launch + cap - 1) / cap;
    }
    return p;
}
inline DecodeLaunch decode_plan_launch(const DecodePlanIn& in, const DecodePlan& p, int i) {
    DecodeLaunch l; l.first = i * p.rows_per_launch; l.rows = in.B - l.first < p.rows_per_launch ? in.B - l.first : p.rows_per_launch;
    l.groups = p.kind == DECODE_PIPE && l.rows > in.pipe_rows ? in.pipe_rows : l.rows;      // PIPE: as even as possible over the resident groups
    if (p.kind == DECODE_COOPB) {            // as many groups as fit the chip, the utterances spread evenly over them
        const int max_groups = in.n_cus / p.G;
        l.groups = (l.rows + DECODE_COOPB_NU - 1) / DECODE_COOPB_NU;
        if (l.groups < max_groups) l.groups = max_groups < l.rows ? max_groups : l.rows;
        l.per_group = (l.rows + l.groups - 1) / l.groups;
        l.groups = (l.rows + l.per_group - 1) / l.per_group;
    }
    l.per_group = (l.rows + l.groups - 1) / l.groups;
    return l;
}
// What qpn_decode_finish runs after a multi-workgroup launch gave up: the one-CU kernels where one CU holds the step state, otherwise the per-utterance cooperative
// kernel at half the group size (the batched kernel counting as at least 2).  Updates in and p, or returns false where nothing smaller exists (G = 1 already).
inline bool decode_plan_retry(DecodePlanIn& in, DecodePlan& p) {
    if (p.kind == DECODE_ONE_CU || (p.kind == DECODE_COOP && p.G < 2)) return false;
    int G = p.G; if (p.kind == DECODE_COOPB) { DecodePlanIn per = in; per.coopb = 0; G = decode_plan(per).G; if (G < 2) G = 2; }
    if (in.single_cu_ok) in.retry_one_cu = true; else in.retry_G = G / 2;
    p = decode_plan(in);
    return true;
}
// the text of qpn_last_decode_plan (bench.py and the tests parse it)
inline void decode_plan_text(const DecodePlanIn& in, const DecodePlan& p, char* buf, size_t cap) {
    const DecodeLaunch l = decode_plan_launch(in, p, 0);
    if (p.kind == DECODE_COOPB && p.launches > 1) snprintf(buf, cap, "coopb G=%d launches=%d x %d rows=%d", p.G, p.launches, p.rows_per_launch, in.B);
    else if (p.kind == DECODE_COOPB) snprintf(buf, cap, "coopb G=%d groups=%d x %d rows=%d", p.G, l.groups, l.per_group, in.B);
    else if (p.kind == DECODE_COOP) snprintf(buf, cap, "coop G=%d rows=%d", p.G, in.B);
    else if (p.kind == DECODE_PIPE) snprintf(buf, cap, "pipe rows=%d waves=%d x %d (%d per group); one-cu rows=0", in.B, p.launches, p.rows_per_launch, p.per_group);
    else snprintf(buf, cap, "pipe rows=0 waves=0 x 0 (1 per group); one-cu rows=%d", in.B);
}
