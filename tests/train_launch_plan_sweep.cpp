// Stand-alone sweep over the training step's launch planner (qpnet_amd/csrc/train_launch_plan.h): for a list of geometries, every knob setting the GPU tests use, a grid
// of batch sizes, chunk lengths and CU counts, and every run-time fact both ways, the shape, the forward plan and the backward plan must keep the invariants the
// launchers and kernels rely on (grids, LDS, the queue, who does which part of the gradient exactly once, the order of the event edges).  Prints the plan text of a
// fixed subset ("GOLDEN key<TAB>text" lines, compared with tests/golden/train_launch_plan.json -- recorded from the launchers in front of the planner -- by
// tests/test_train_launch_plan_cpu.py) and the number of plans checked.  Built with the host sanitizers and run as a child process.
#include "../qpnet_amd/csrc/qpn_geom.h"
#include "../qpnet_amd/csrc/train_plan.h"
#include "../qpnet_amd/csrc/train_launch_plan.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static char g_err[512] = "";
void qpn_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

static std::string g_ctx;
static long n_plans = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s (line %d) -- %s\n", #cond, __LINE__, g_ctx.c_str()); exit(1); } } while (0)

// the defaults of qpn_train_knobs_parse, and one environment setting applied as it applies it
static TrainKnobs default_knobs() {
    TrainKnobs k = {};
    k.stack_q_fwd = k.stack_q_bwd = k.persist_fwd = k.persist_bwd = k.up_side = k.reduce_early = k.wr_side = k.post_fuse = k.post_pair = k.zero_in_post = k.post_wide = true;
    k.xcd_swizzle = k.aux_hoist = k.prep_fuse = true;
    return k;
}
static void set_knob(TrainKnobs& k, const std::string& name, int v) {
    if (name == "QPN_TRAIN_SERIAL") k.serial = v != 0;
    else if (name == "QPN_STACK_QUEUE") { k.stack_q_fwd = v != 0; k.stack_q_bwd = k.stack_q_bwd && k.stack_q_fwd; }
    else if (name == "QPN_STACK_QUEUE_BWD") k.stack_q_bwd = k.stack_q_fwd && v != 0;
    else if (name == "QPN_STACK_WGS") k.stack_wgs = v;
    else if (name == "QPN_STACK_WGS_BWD") k.stack_wgs_bwd = v;
    else if (name == "QPN_LAYER_PERSIST") k.persist_fwd = v != 0;
    else if (name == "QPN_LAYER_BWD_PERSIST") k.persist_bwd = v != 0;
    else if (name == "QPN_WGRAD_CHUNKS") k.wgrad_chunks = v;
    else if (name == "QPN_WGRAD_CHUNKS_SIDE") k.wgrad_chunks_side = v;
    else if (name == "QPN_UP_SIDE") k.up_side = v != 0;
    else if (name == "QPN_REDUCE_EARLY") k.reduce_early = v != 0;
    else if (name == "QPN_WR_SIDE") k.wr_side = v != 0;
    else if (name == "QPN_POST_FUSE") k.post_fuse = v != 0;
    else if (name == "QPN_POST_WGRAD_PAIR") k.post_pair = v != 0;
    else if (name == "QPN_ZERO_IN_POST") k.zero_in_post = v != 0;
    else if (name == "QPN_POST_WIDE") k.post_wide = v != 0;
    else if (name == "QPN_CE_SEPARATE") k.ce_separate = true;
    else if (name == "QPN_EVENT_FENCE") k.event_fence = v == 1;
    else if (name == "QPN_AUX_HOIST") k.aux_hoist = v != 0;
    else if (name == "QPN_PREP_FUSE") k.prep_fuse = v != 0;
    else { fprintf(stderr, "unknown knob %s\n", name.c_str()); exit(1); }
}
static TrainKnobs knobs_of(const char* setting) {      // "NAME=v,NAME=v"
    TrainKnobs k = default_knobs();
    const std::string s = setting;
    for (size_t i = 0; i < s.size();) {
        size_t e = s.find(',', i); if (e == std::string::npos) e = s.size();
        const std::string kv = s.substr(i, e - i); const size_t q = kv.find('=');
        set_knob(k, kv.substr(0, q), atoi(kv.c_str() + q + 1));
        i = e + 1;
    }
    return k;
}
// the settings of tests/test_train_gpu.py::test_backward_launch_arrangements_agree, then four more
static const char* const KNOBS[] = {"", "QPN_TRAIN_SERIAL=1", "QPN_UP_SIDE=0", "QPN_REDUCE_EARLY=0", "QPN_POST_WGRAD_PAIR=0", "QPN_ZERO_IN_POST=0", "QPN_WR_SIDE=0", "QPN_WGRAD_CHUNKS_SIDE=64",
    "QPN_WGRAD_CHUNKS=48,QPN_WGRAD_CHUNKS_SIDE=32", "QPN_EVENT_FENCE=1", "QPN_STACK_QUEUE_BWD=0", "QPN_STACK_QUEUE=0", "QPN_STACK_WGS_BWD=512", "QPN_STACK_WGS=96,QPN_STACK_WGS_BWD=40",
    "QPN_AUX_HOIST=0", "QPN_AUX_HOIST=0,QPN_STACK_QUEUE=0", "QPN_LAYER_PERSIST=0,QPN_LAYER_BWD_PERSIST=0", "QPN_POST_WIDE=0", "QPN_POST_FUSE=0", "QPN_PREP_FUSE=0", "QPN_CE_SEPARATE=1"};

// the chunk of a sweep call: the shortest x / d / h that hold the rows, with a little room
static const int MAXD = 4;
struct Call { int64_t T, F, Td; };
static Call call_of(const Geom& g, int BL) {
    const int64_t N0 = (int64_t)g.recA * MAXD + g.recF + 1 + BL;
    return Call{N0 + 3, g.U > 0 ? (N0 + g.U - 1) / g.U + 2 : N0 + 2, N0 + 2};
}

static void check_launch(const TlpLaunch& l, unsigned block) {
    CHECK(l.gx >= 1 && l.gy >= 1 && l.gz >= 1 && l.gy <= 65535 && l.gz <= 65535 && l.block == block && l.lds <= TLP_LDS_MAX);
}

static void check_shape(const Geom& g, const TrainLayout& lay, const TrainShape& s, int B, int BL) {
    CHECK(s.rc == QPN_OK && s.B == B && s.BL == BL && s.N1 == s.N0 - 1 && s.N0 == g.recA * MAXD + g.recF + 1 + BL);
    int pos = 0, row = 0;
    for (int l = 0; l < g.L; ++l) {
        CHECK(s.s_in[l] == row && s.s_out[l] > s.s_in[l] && s.s_out[l] < s.N1); row = s.s_out[l];
        CHECK(s.tap_off[l] == l * B * s.N1);
        CHECK(s.qT[l] >= 1 && 16 * s.qT[l] >= s.N1 - s.s_out[l] && 16 * (s.qT[l] - 1) < s.N1 - s.s_out[l]);
        CHECK(s.qP[l] == pos && (l == 0 || s.qP[l] > s.qP[l - 1])); pos += B * s.qT[l];      // monotone; qtotal is the sum of B qT[l]
    }
    CHECK(s.N1 - row == BL);                                       // the last layer's valid rows are the chunk's batch_length
    for (int l = g.L; l <= TR_MAXL; ++l) CHECK(s.qP[l] == pos);
    CHECK(s.qtotal == pos);
    if (lay.hoist) CHECK(s.nfr >= 1 && s.ffirst >= 0 && s.ffirst + s.nfr == s.F && (int64_t)s.ffirst * g.U <= (int64_t)s.F * g.U - s.N1 && (int64_t)(s.ffirst + 1) * g.U > (int64_t)s.F * g.U - s.N1);
    else CHECK(s.nfr == 0 && s.ffirst == 0);
}

static void check_fwd(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s, const TrainFwdFacts& f, const TrainFwdPlan& p) {
    CHECK(p.rc == QPN_OK && p.gemm == lay.use_gemm && p.queues_usable == f.queues_usable);
    check_launch(p.refresh, 256);
    if (p.gemm) { CHECK(!p.fuse_prep && !p.fuse_ce && !p.fuse_post && p.store_logits); return; }
    check_launch(p.prep, 256);
    if (p.fuse_prep) {
        const StepPrepPlan& r = p.roles;
        CHECK(k.prep_fuse && f.flat_aligned16 && p.prep.lds <= TLP_LDS_PREP && p.prep.gy == 1);
        CHECK(r.nx0 >= 1 && r.naux >= 0 && r.nbias >= 1 && r.nwt >= 1 && r.nprep >= 1 && (unsigned)(r.nx0 + r.naux + r.nbias + r.nwt + r.nprep * s.B) == p.prep.gx);
        CHECK(r.rpg >= 16 && r.rpg <= X0_RPG && (int64_t)(r.nx0 / (g.C / X0_CS)) * r.rpg >= (int64_t)s.B * s.N1);      // the table workgroups cover every row
        CHECK((r.naux > 0) == lay.hoist);
    } else CHECK(p.prep.gy == (unsigned)s.B && p.prep_blocks >= 1 && p.prep.gx >= (unsigned)p.prep_blocks);
    CHECK(p.form == (lay.hoist ? 8 : 11) && p.flags0 == (k.xcd_swizzle ? 2 : 0));
    // hoist implies the register-resident kernels; the stack path only where its conditions hold and the queues are usable
    if (lay.hoist) CHECK(p.path != TLP_GENERIC);
    if (p.path != TLP_GENERIC) CHECK(g.C == 64 && k.persist_fwd && s.N1 < (1 << 24));
    if (p.path == TLP_STACK) {
        CHECK(k.stack_q_fwd && f.queues_usable && tlp_stack_fwd_fits(g, lay, s));
        check_launch(p.stack, 256);
        CHECK(p.stack.gy == 1 && p.stack.gx <= (unsigned)(s.qtotal < 1024 ? s.qtotal : 1024));
        const unsigned cap = p.stack.gx / 8 > 1 ? p.stack.gx / 8 : 1;
        CHECK(p.nq >= 1 && p.nq <= (cap < SQ_NQ ? cap : SQ_NQ));
        if (k.stack_wgs > 0 && k.stack_wgs <= s.qtotal && k.stack_wgs <= 1024) CHECK(p.stack.gx == (unsigned)k.stack_wgs);
    } else {
        CHECK(!(k.stack_q_fwd && f.queues_usable && tlp_persist_fwd(g, lay, k, s) && tlp_stack_fwd_fits(g, lay, s)));
        for (int l = 0; l < g.L; ++l) {
            check_launch(p.layer[l], 256);
            CHECK(p.layer[l].gy == (unsigned)s.B && p.layer[l].gx <= (unsigned)s.qT[l] && (p.path == TLP_PERSIST ? p.layer[l].gx <= 1024 && p.layer[l].lds <= TLP_LDS_OPTIN : p.layer[l].gx == (unsigned)s.qT[l]));
        }
    }
    check_launch(p.post_l, 512);
    CHECK(p.post_l.gy == (unsigned)s.B && (int)p.post_l.gx * (p.post == TLP_POST_TILE ? 16 : 80) >= s.BL && ((int)p.post_l.gx - 1) * (p.post == TLP_POST_TILE ? 16 : 80) < s.BL);
    CHECK((p.post != TLP_POST_TILE) == (g.S == 256 && g.Q == 256 && g.C == 64 && k.post_wide));
    CHECK((p.post == TLP_POST_FB) == p.fuse_post);
    if (p.fuse_ce) CHECK(f.targets && !k.ce_separate && !f.soft_targets && !f.loss_opts && g.Q <= g.S && g.Q % 256 == 0);
    CHECK(p.store_logits == !(p.fuse_ce && !f.want_logits));
    // fuse_post implies fuse_ce, the backward's wide form and the zeroing inside it
    if (p.fuse_post) CHECK(p.fuse_ce && f.fuse_bwd && f.dlogits && k.post_fuse && tlp_post_wide_bwd(g, lay, k) && tlp_zero_in_post(g, lay, k));
}

static void check_bwd(const Geom& g, const TrainLayout& lay, const TrainKnobs& k, const TrainShape& s, const TrainFwdPlan& fp, const TrainBwdFacts& f, const TrainBwdPlan& p) {
    CHECK(p.rc == QPN_OK && p.gemm == lay.use_gemm);
    if (p.gemm) { CHECK(p.njobs == 0); return; }
    CHECK(p.post_done == (fp.fuse_post && f.first_bwd && f.same_dlogits));
    if (lay.hoist) CHECK(p.path != TLP_GENERIC);
    if (p.path == TLP_STACK) {
        CHECK(k.stack_q_bwd && f.first_bwd && fp.queues_usable && tlp_persist_bwd(g, lay, k, s) && tlp_stack_bwd_fits(g, lay, s) && p.wr_summed);
        check_launch(p.stack, 256);
        CHECK(p.stack.gy == 1 && p.stack.gx <= (unsigned)(s.qtotal < 1024 ? s.qtotal : 1024));
        const unsigned cap = p.stack.gx / 8 > 1 ? p.stack.gx / 8 : 1;
        CHECK(p.nq >= 1 && p.nq <= (cap < SQ_NQ ? cap : SQ_NQ));
        if (k.stack_wgs_bwd >= 8 && k.stack_wgs_bwd <= s.qtotal && k.stack_wgs_bwd <= 1024) CHECK(p.stack.gx == (unsigned)k.stack_wgs_bwd);
    } else {
        CHECK(!p.wr_summed);
        for (int l = 0; l < g.L; ++l) { check_launch(p.layer[l], 256); CHECK(p.layer[l].gy == (unsigned)s.B && p.layer[l].gx <= (unsigned)s.qT[l] && (p.path == TLP_GENERIC ? p.layer[l].gx == (unsigned)s.qT[l] : p.layer[l].gx <= 1024)); }
    }
    // up_side => early_reduce => overlap => (side stream, not serial, no serial profile); wr_side => overlap
    if (p.up_side) CHECK(p.early_reduce && g.U > 0 && k.up_side);
    if (p.early_reduce) CHECK(p.overlap && k.reduce_early && f.gdst);
    if (p.wr_side) CHECK(p.overlap && k.wr_side);
    if (p.overlap) CHECK(f.side_stream && !k.serial && !f.prof_serial);
    CHECK(p.nch == lay.nch && p.nch_side >= 1 && p.nch_side <= p.nch && (p.early_reduce || p.nch_side == p.nch));
    if (p.early_reduce && k.wgrad_chunks_side > 0 && k.wgrad_chunks_side <= p.nch) CHECK(p.nch_side == k.wgrad_chunks_side);
    CHECK(p.zero_in_post == (p.post == TLP_POST_WIDE && k.zero_in_post));
    CHECK((p.post == TLP_POST_WIDE) == (g.S == 256 && g.Q == 256 && g.C == 64 && (lay.LC == 256 || lay.LC == 512) && k.post_wide));
    check_launch(p.post_l, 512); check_launch(p.zero, 256); check_launch(p.reduce_early, 256); check_launch(p.tail.reduce, 256);
    CHECK(p.post_l.gy == (unsigned)s.B && (int)p.post_l.gx * (p.post == TLP_POST_WIDE ? 80 : 16) >= s.BL);
    CHECK(p.tail.early_done == p.early_reduce && p.tail.up_done == p.up_side);
    if (p.tail.causal_hist) { check_launch(p.tail.causal, 256); CHECK(lay.slabs.g_cw < 0 && p.tail.CB >= 1 && p.tail.causal.lds == (size_t)2 * g.Q * p.tail.CB * 4 && (int64_t)p.tail.rpw * 128 >= (int64_t)s.B * s.N1); }
    if (g.U > 0) { check_launch(p.tail.up, 128); CHECK((int64_t)p.tail.up.gx * g.U >= s.N1 && p.tail.up.gy == (unsigned)s.B); }
    check_launch(p.tail.aux, 128);

    // ---- the jobs: each part of the gradient exactly once across {done in the forward, main, side, the final tail}, in an order the data allows
    CHECK(p.njobs >= 4 && p.njobs <= TLP_MAX_JOBS);
    int count[TJ_CAUSAL_HIST + 1] = {}, at[TJ_CAUSAL_HIST + 1];
    for (int& a : at) a = -1;
    int n_side = 0, post_parts = 0;
    for (int i = 0; i < p.njobs; ++i) {
        const TrainJob& j = p.jobs[i];
        CHECK(j.kind >= TJ_MARK && j.kind <= TJ_CAUSAL_HIST && (j.side == 0 || j.side == 1) && j.mark >= -2 && j.mark < PG_COUNT);
        ++count[j.kind]; at[j.kind] = i; n_side += j.side;
        if (j.side) CHECK(p.overlap);
        if (j.kind == TJ_POST) post_parts = j.n;
        if (j.kind == TJ_SKIP || j.kind == TJ_POST) CHECK(j.arg == p.nch_side && j.side == (p.overlap ? 1 : 0));
        if (j.kind == TJ_W1 || j.kind == TJ_WR || j.kind == TJ_CAUSAL) CHECK(j.arg == p.nch);
        if (j.kind == TJ_W1 || j.kind == TJ_CAUSAL || j.kind == TJ_LAYERS || j.kind == TJ_POST_BWD || j.kind == TJ_ZERO || j.kind == TJ_REDUCE || j.kind == TJ_CAUSAL_HIST || j.kind == TJ_WAIT) CHECK(j.side == 0);
        if (j.kind == TJ_REDUCE_EARLY || j.kind == TJ_EARLY_EVENT || j.kind == TJ_FORK || j.kind == TJ_MID || j.kind == TJ_JOIN) CHECK(j.side == 1);
    }
    if (!p.overlap) CHECK(n_side == 0);
    // the zeroing and the post-net backward: in the forward (post_done), or here -- the zeroing a launch of its own or inside the post-net's
    CHECK(count[TJ_POST_BWD] == (p.post_done ? 0 : 1) && count[TJ_ZERO] == ((p.post_done || p.zero_in_post) ? 0 : 1));
    if (count[TJ_ZERO]) CHECK(at[TJ_ZERO] < at[TJ_POST_BWD]);
    CHECK(count[TJ_SKIP] == 1 && count[TJ_POST] == 1 && post_parts == ((g.Q == g.S && k.post_pair) ? 1 : 2));
    CHECK(count[TJ_LAYERS] == 1 && count[TJ_W1] == 1 && count[TJ_WR] == 1 && count[TJ_REDUCE] == 1);
    CHECK(count[TJ_CAUSAL] + count[TJ_CAUSAL_HIST] == 1 && (count[TJ_CAUSAL] == 1) == (lay.slabs.g_cw >= 0));      // the causal contraction xor the histogram
    CHECK(count[TJ_UP] + count[TJ_AUX_TAIL] == (g.U > 0 ? 1 : 0) && (count[TJ_AUX_TAIL] == 1) == lay.hoist);        // the upsampling gradient xor the aux tail xor neither
    CHECK(count[TJ_INPUT_GRAD] == (f.feature_grad ? 1 : 0));
    CHECK(count[TJ_REDUCE_EARLY] == (p.early_reduce ? 1 : 0));
    CHECK(count[TJ_FORK] == (p.overlap ? 1 : 0) && count[TJ_JOIN] == count[TJ_FORK] && count[TJ_WAIT] == count[TJ_FORK] && count[TJ_MID] == ((p.wr_side || p.up_side) ? 1 : 0));
    CHECK(count[TJ_EARLY_EVENT] == ((p.up_side && f.append_scale && lay.early_first >= 0) ? 1 : 0));
    // the zeroing-and-trailer: the early reduction (n = 1) or the final one, never both
    if (p.early_reduce) CHECK((p.jobs[at[TJ_REDUCE_EARLY]].n == 1) == p.tail.up_done);
    else CHECK(!p.tail.up_done);
    // order
    if (count[TJ_POST_BWD]) CHECK(at[TJ_POST_BWD] < at[TJ_SKIP] && at[TJ_POST_BWD] < at[TJ_LAYERS] && (!p.overlap || at[TJ_POST_BWD] < at[TJ_FORK]));
    CHECK(at[TJ_SKIP] < at[TJ_POST] && at[TJ_LAYERS] < at[TJ_W1] && at[TJ_LAYERS] < at[TJ_WR] && at[TJ_W1] < at[TJ_REDUCE] && at[TJ_WR] < at[TJ_REDUCE] && at[TJ_POST] < at[TJ_REDUCE]);
    if (count[TJ_CAUSAL]) CHECK(at[TJ_LAYERS] < at[TJ_CAUSAL] && at[TJ_CAUSAL] < at[TJ_REDUCE]); else CHECK(at[TJ_REDUCE] < at[TJ_CAUSAL_HIST]);
    if (p.overlap) {
        CHECK(at[TJ_FORK] < at[TJ_SKIP] && at[TJ_FORK] < at[TJ_LAYERS] && at[TJ_JOIN] < at[TJ_WAIT] && at[TJ_WAIT] < at[TJ_REDUCE]);      // the join precedes the final reduction
        for (int i = 0; i < p.njobs; ++i) if (p.jobs[i].side) CHECK(i >= at[TJ_FORK] && i <= at[TJ_JOIN]);
        if (p.early_reduce) CHECK(at[TJ_POST] < at[TJ_REDUCE_EARLY] && at[TJ_REDUCE_EARLY] < at[TJ_JOIN]);
        if (count[TJ_EARLY_EVENT]) CHECK(at[TJ_EARLY_EVENT] == at[TJ_REDUCE_EARLY] + 1);
    }
    // a side-stream job that needs the layer backward sits behind the mid edge, which sits behind the layer backward
    if (count[TJ_MID]) CHECK(at[TJ_LAYERS] < at[TJ_MID]);
    for (int i = 0; i < p.njobs; ++i) {
        const TrainJob& j = p.jobs[i];
        if (j.side && (j.kind == TJ_WR || j.kind == TJ_UP || j.kind == TJ_AUX_TAIL || j.kind == TJ_INPUT_GRAD)) CHECK(count[TJ_MID] == 1 && i > at[TJ_MID]);
        if (!j.side && (j.kind == TJ_UP || j.kind == TJ_AUX_TAIL || j.kind == TJ_INPUT_GRAD)) CHECK(i > at[TJ_REDUCE] && !p.tail.up_done);
    }
    // the aux tail / upsampling gradient sits behind the launch that zeroes its targets
    const int up_at = count[TJ_UP] ? at[TJ_UP] : count[TJ_AUX_TAIL] ? at[TJ_AUX_TAIL] : -1;
    if (up_at >= 0) {
        CHECK((p.jobs[up_at].side == 1) == p.up_side);
        if (p.up_side) CHECK(p.jobs[at[TJ_REDUCE_EARLY]].n == 1 && at[TJ_REDUCE_EARLY] < up_at); else CHECK(at[TJ_REDUCE] < up_at);
    }
    if (count[TJ_INPUT_GRAD]) CHECK((p.jobs[at[TJ_INPUT_GRAD]].side == 1) == p.up_side);
    CHECK((p.jobs[at[TJ_WR]].side == 1) == p.wr_side);
    // post_done: no zeroing and no post-net backward here
    if (p.post_done) CHECK(count[TJ_ZERO] == 0 && count[TJ_POST_BWD] == 0);
}

struct NG { const char* name; qpn_config c; };
int main() {
    // {n_quantize, n_aux, n_resch, n_skipch, dilationF_depth, dilationF_repeat, dilationA_depth, dilationA_repeat, kernel_size, upsampling_factor}: the 13 of tests/train_plan_sweep.cpp
    std::vector<NG> geoms = {
        {"tiny", {256, 39, 32, 32, 2, 1, 1, 1, 2, 110}}, {"paper", {256, 39, 64, 256, 4, 1, 4, 1, 2, 110}}, {"default", {256, 39, 512, 256, 4, 3, 4, 1, 2, 110}},
        {"deep64", {256, 39, 64, 256, 10, 3, 4, 1, 2, 110}}, {"paper_aux7", {256, 7, 64, 256, 4, 1, 4, 1, 2, 110}}, {"paper_aux80", {256, 80, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_up0", {256, 39, 64, 256, 4, 1, 4, 1, 2, 0}}, {"paper_up8", {256, 39, 64, 256, 4, 1, 4, 1, 2, 8}}, {"paper_q128", {128, 39, 64, 256, 4, 1, 4, 1, 2, 110}},
        {"paper_q64", {64, 39, 64, 256, 4, 1, 4, 1, 2, 110}}, {"all_adaptive", {256, 39, 64, 256, 0, 0, 4, 2, 2, 110}}, {"all_fixed", {256, 39, 64, 256, 4, 2, 0, 0, 2, 110}},
        {"c160", {256, 39, 160, 256, 2, 1, 2, 1, 2, 110}},
    };
    const size_t n_named = geoms.size();
    static const int wide[][3] = {{16, 16, 16}, {48, 80, 48}, {80, 48, 96}, {112, 144, 80}, {32, 16, 64}, {128, 112, 192}, {64, 48, 32}, {64, 16, 256}, {64, 272, 144}};      // TRAIN_CSQ of tests/test_width_classes_gpu.py
    static std::vector<std::string> wnames;
    for (const auto& w : wide) wnames.push_back("w" + std::to_string(w[0]) + "_" + std::to_string(w[1]) + "_" + std::to_string(w[2]));
    for (size_t i = 0; i < wnames.size(); ++i) geoms.push_back({wnames[i].c_str(), {wide[i][2], 39, wide[i][0], wide[i][1], 2, 1, 2, 1, 2, 110}});
    static const char* const golden_geoms[] = {"tiny", "paper", "default", "deep64", "paper_up0", "paper_aux80", "c160"};
    static const int Bs[] = {1, 3}, BLs[] = {1, 15, 16, 17, 80, 81, 500}, CUs[] = {256, 64, 32};
    long n_small_g = 0, n_paths[3] = {};
    for (size_t gi = 0; gi < geoms.size(); ++gi) for (const char* kn : KNOBS) {
        const NG& ng = geoms[gi];
        Geom g;
        g_ctx = std::string(ng.name) + " [" + kn + "]";
        CHECK(qpn_build_geom(&ng.c, &g) == QPN_OK);
        const TrainKnobs k = knobs_of(kn);
        // (the layout depends on four knobs only: planned once per geometry and value of those -- the maps of the wide geometries are large)
        struct Cached { size_t gi; bool ah, pf, pb; int wc; TrainLayout lay; };
        static std::vector<Cached> cache;
        const TrainLayout* found = nullptr;
        for (const Cached& c : cache) if (c.gi == gi && c.ah == k.aux_hoist && c.pf == k.persist_fwd && c.pb == k.persist_bwd && c.wc == k.wgrad_chunks) found = &c.lay;
        if (!found) {
            const TrainPlan tp = train_plan(g, k, g.C > 128);
            CHECK(tp.rc == QPN_OK);
            cache.push_back({gi, k.aux_hoist, k.persist_fwd, k.persist_bwd, k.wgrad_chunks, tp});
            found = &cache.back().lay;
        }
        const TrainLayout lay = *found;
        // ---- the golden subset: 256 CUs, every fact as a plain training step has it; the one-call step, then the forward-then-backward pair
        bool is_golden = false;
        for (const char* n : golden_geoms) is_golden = is_golden || std::string(n) == ng.name;
        if (is_golden) {
            static const int bbl[][2] = {{2, 500}, {1, 17}};
            for (const auto& c : bbl) for (int one = 1; one >= 0; --one) {
                const Call cl = call_of(g, c[1]);
                const TrainShape s = train_shape(g, lay, c[0], cl.T, cl.F, cl.Td, c[1], MAXD);
                TrainFwdFacts ff; ff.cus = 256; ff.queues_usable = ff.flat_aligned16 = ff.targets = ff.dlogits = true; ff.fuse_bwd = one != 0;
                TrainBwdFacts bf; bf.cus = 256; bf.side_stream = bf.gdst = bf.first_bwd = bf.same_dlogits = true;
                const TrainFwdPlan fp = train_fwd_plan(g, lay, k, s, ff);
                const TrainBwdPlan bp = train_bwd_plan(g, lay, k, s, fp, bf);
                CHECK(s.rc == QPN_OK && fp.rc == QPN_OK && bp.rc == QPN_OK);
                printf("GOLDEN %s/%s/B%d_BL%d/%s\t%s | %s\n", ng.name, *kn ? kn : "default", c[0], c[1], one ? "step" : "pair", plan_text(g, lay, s, fp).c_str(), plan_text(g, lay, s, bp).c_str());
            }
        }
        // ---- the sweep
        for (int B : Bs) for (int BL : BLs) {
            const Call cl = call_of(g, BL);
            const TrainShape s = train_shape(g, lay, B, cl.T, cl.F, cl.Td, BL, MAXD);
            check_shape(g, lay, s, B, BL);
            for (int cus : CUs) for (int fv = 0; fv <= 8; ++fv) for (int bv = 0; bv <= 8; ++bv) {
                // the base: a plain one-call training step; variant v > 0 flips fact v - 1
                TrainFwdFacts ff; ff.cus = cus;
                ff.queues_usable = fv != 1; ff.flat_aligned16 = fv != 2; ff.targets = fv != 3; ff.want_logits = fv == 4; ff.dlogits = fv != 5; ff.fuse_bwd = fv != 6; ff.soft_targets = fv == 7; ff.loss_opts = fv == 8;
                TrainBwdFacts bf; bf.cus = cus;
                bf.side_stream = bv != 1; bf.prof_serial = bv == 2; bf.gdst = bv != 3; bf.append_scale = bv == 4 ? 1 : bv == 8 ? 2 : 0; bf.feature_grad = bv == 5; bf.first_bwd = bv != 6; bf.same_dlogits = bv != 7;
                g_ctx = std::string(ng.name) + " [" + kn + "] B " + std::to_string(B) + " BL " + std::to_string(BL) + " cus " + std::to_string(cus) + " facts " + std::to_string(fv) + "/" + std::to_string(bv);
                const TrainFwdPlan fp = train_fwd_plan(g, lay, k, s, ff);
                check_fwd(g, lay, k, s, ff, fp);
                const TrainBwdPlan bp = train_bwd_plan(g, lay, k, s, fp, bf);
                check_bwd(g, lay, k, s, fp, bf, bp);
                // the forward and the backward agree: the backward takes the queue only behind a forward that could, and a hoisted step never falls back in one direction alone
                if (bp.path == TLP_STACK) CHECK(fp.queues_usable);
                if (lay.hoist) CHECK(fp.path != TLP_GENERIC && bp.path != TLP_GENERIC);
                if (!lay.use_gemm) { ++n_paths[fp.path]; if (bp.path == TLP_STACK && bp.stack.gx == (unsigned)cus && cus < 64) ++n_small_g; }
                if (fv == 0 || bv == 0) { (void)plan_text(g, lay, s, fp).size(); (void)plan_text(g, lay, s, bp).size(); }      // (the sanitizers watch the formatting too)
                n_plans += 2;
            }
        }
        if (gi >= n_named && std::string(kn).empty()) printf("CHECKED %s\n", ng.name);
    }
    CHECK(n_paths[TLP_GENERIC] > 0 && n_paths[TLP_PERSIST] > 0 && n_paths[TLP_STACK] > 0);
    {   // the three shape refusals: their codes and texts
        g_ctx = "refusals";
        Geom g; const qpn_config paper = {256, 39, 64, 256, 4, 1, 4, 1, 2, 110};
        CHECK(qpn_build_geom(&paper, &g) == QPN_OK);
        const TrainPlan tp = train_plan(g, default_knobs(), false);
        const Call cl = call_of(g, 500);
        CHECK(train_shape(g, tp, 2, cl.T, cl.F, cl.Td, 500, MAXD).rc == QPN_OK);
        CHECK(train_shape(g, tp, 2, cl.T - 4, cl.F, cl.Td, 500, MAXD).rc == QPN_EINVAL && std::string(g_err).find("chunk too short: need receptive field (") == 0);
        CHECK(train_shape(g, tp, 2, cl.T, cl.F, cl.Td - 4, 500, MAXD).rc == QPN_EINVAL && std::string(g_err).find("chunk too short: need receptive field (") == 0);
        CHECK(train_shape(g, tp, 2, cl.T, 1, cl.Td, 500, MAXD).rc == QPN_EINVAL && std::string(g_err).find("chunk too short: need receptive field (") == 0);
        CHECK(train_shape(g, tp, 2, (int64_t)1 << 31, cl.F, cl.Td, 500, MAXD).rc == QPN_EINVAL && std::string(g_err) == "chunk too long: the training kernels index rows with 32 bits");
        CHECK(train_shape(g, tp, 1 << 22, cl.T, cl.F, cl.Td, 500, MAXD).rc == QPN_EINVAL && std::string(g_err) == "chunk too long: the training kernels index rows with 32 bits");      // B N0 >= 2^31
        const int BLbig = (1 << 24) + 8; const Call big = call_of(g, BLbig);
        CHECK(tp.hoist && train_shape(g, tp, 1, big.T, big.F, big.Td, BLbig, MAXD).rc == QPN_EINVAL && std::string(g_err).find("chunk too long for the register-resident layer kernels (") == 0);
        TrainKnobs nh = default_knobs(); nh.aux_hoist = false;
        const TrainPlan tq = train_plan(g, nh, false);      // without the hoist the same chunk passes: the launch plan then leaves the register-resident kernels
        const TrainShape sb = train_shape(g, tq, 1, big.T, big.F, big.Td, BLbig, MAXD);
        CHECK(sb.rc == QPN_OK);
        TrainFwdFacts ff; ff.cus = 256; ff.queues_usable = ff.flat_aligned16 = true;
        CHECK(train_fwd_plan(g, tq, nh, sb, ff).path == TLP_GENERIC);
    }
    // the backward queue's G < 8 fallback (a CU count for the grid) was reached with 32 CUs
    CHECK(n_small_g > 0);
    printf("TRAIN_LAUNCH_PLAN_SWEEP_OK %ld plans\n", n_plans);
    return 0;
}
