// Stand-alone sweep over the decode launch planner (qpnet_amd/csrc/decode_plan.h): every plan of a grid of geometries, CU counts, batch sizes, knob settings
// and attempts must cover its rows exactly once and fit the chip, and every retry chain must end.  Built with the host sanitizers and run as a child
// process by tests/test_decode_plan_cpu.py; prints the number of plans checked.
#include "../qpnet_amd/csrc/decode_plan.h"
#include <cstdlib>

static long n_plans = 0;
#define CHECK(cond) do { if (!(cond)) { char t[160]; decode_plan_text(in, p, t, sizeof(t)); \
    fprintf(stderr, "FAILED %s -- C=%d n_cus=%d B=%d coop=%d coopb=%d pipe=%d pipe_nu=%d retry=%d limit=%d: %s\n", #cond, in.C, in.n_cus, in.B, in.coop, in.coopb, in.pipe, \
            in.pipe_nu, (int)in.retry_one_cu, in.retry_G, t); exit(1); } } while (0)

static void check_plan(const DecodePlanIn& in, const DecodePlan& p) {
    ++n_plans;
    const int B = in.B;
    CHECK(p.launches >= 1 && p.rows_per_launch >= 1);
    CHECK((long)p.launches * p.rows_per_launch >= B && B > (long)(p.launches - 1) * p.rows_per_launch);
    int covered = 0;
    for (int i = 0; i < p.launches; ++i) {
        const DecodeLaunch l = decode_plan_launch(in, p, i);
        CHECK(l.first == covered && l.rows >= 1 && l.groups >= 1 && l.per_group >= 1 && (long)l.groups * l.per_group >= l.rows);
        covered += l.rows;
        if (p.kind == DECODE_PIPE) CHECK(l.per_group <= in.pipe_nu && l.groups == (l.rows < in.pipe_rows ? l.rows : in.pipe_rows) && l.groups * 5 <= in.n_cus);
        if (p.kind == DECODE_COOPB) CHECK(l.per_group <= 16 && l.groups * p.G <= in.n_cus);
    }
    CHECK(covered == B);
    CHECK(p.needs_ring == (p.kind == DECODE_ONE_CU || p.kind == DECODE_PIPE));
    if (p.kind == DECODE_PIPE) {
        CHECK(p.per_group <= in.pipe_nu);
        CHECK((p.rows_per_launch < in.pipe_rows ? p.rows_per_launch : in.pipe_rows) * 5 <= in.n_cus);
    }
    if (p.kind == DECODE_COOP && in.coop <= in.n_cus) {
        const int per = in.n_cus / p.G;
        CHECK(p.G * (B < per ? B : per) <= in.n_cus);
    }
    char t[160]; decode_plan_text(in, p, t, sizeof(t));
    CHECK(t[0] == 'c' || t[0] == 'p');
}

int main() {
    struct G { int C, S, Q, L; bool single_cu_ok, pipe_supported, coopb_supported; };
    static const G geoms[] = {{64, 256, 256, 8, true, true, false},      // PAPER
                              {512, 256, 256, 16, false, false, true},   // DEFAULT
                              {32, 32, 256, 3, true, false, false},      // TINY
                              {256, 256, 256, 16, false, false, true},
                              {4, 32, 256, 3, true, false, false}};      // (C / 8 == 0: the batched kernel's arithmetic must stay unevaluated)
    static const int more_cus[] = {63, 64, 80, 104, 128, 255, 256, 304, 320}, more_B[] = {255, 256, 257, 300, 400};
    int cus[49], Bs[204], nc = 0, nb = 0;
    for (int i = 1; i <= 40; ++i) cus[nc++] = i;
    for (int v : more_cus) cus[nc++] = v;
    for (int i = 1; i <= 199; ++i) Bs[nb++] = i;
    for (int v : more_B) Bs[nb++] = v;
    for (const G& g : geoms) for (int ci = 0; ci < nc; ++ci) for (int bi = 0; bi < nb; ++bi) for (int knob = 0; knob < 6; ++knob) {
        DecodePlanIn in = {};
        in.C = g.C; in.S = g.S; in.Q = g.Q; in.Cp = g.C < 16 ? 16 : g.C; in.Sp = g.S < 16 ? 16 : g.S; in.L = g.L;      // (powers of two: the padded widths are the widths)
        in.single_cu_ok = g.single_cu_ok; in.pipe_supported = g.pipe_supported; in.coopb_supported = g.coopb_supported; in.coopb_fits = true;
        in.n_cus = cus[ci]; in.pipe_rows = (in.n_cus / 40) * 8; in.pipe_nu = knob == 2 ? 2 : 3;
        in.coop = knob == 5 ? 4 : 0; in.coopb = knob == 3 ? 0 : knob == 4 ? 8 : 1; in.pipe = knob == 1 ? 0 : 1; in.generic = false;
        in.B = Bs[bi];
        DecodePlan p = decode_plan(in);
        check_plan(in, p);                                   // attempt 0
        int steps = 0;
        while (decode_plan_retry(in, p)) {                   // attempt 1 and what further give-ups would lead to
            check_plan(in, p);
            if (++steps > 9) { fprintf(stderr, "FAILED: retry chain longer than 9 steps (C=%d n_cus=%d B=%d knob=%d)\n", g.C, cus[ci], Bs[bi], knob); return 1; }
        }
        CHECK(p.kind == DECODE_ONE_CU || (p.kind == DECODE_COOP && p.G == 1));
    }
    printf("DECODE_PLAN_SWEEP_OK %ld plans\n", n_plans);
    return 0;
}
