// train_wgrad_plan.h -- the weight-gradient time contractions as the host sees them: the argument record, the five records of a step, the kernel
// instance each record gets and the row-block split.  Pure host arithmetic (plain C++: no HIP, no handle, no globals).  train_wgrad.hip expands the
// instance lists below into its dispatcher, so an instance cannot be picked without being instantiated, or the reverse; train_bwd.hip (tile path) and
// train_gemm.hip (GEMM path, through targs_of) build their records with the same five functions; tests/wgrad_plan_sweep.cpp checks all of it on a CPU.
#pragma once
#include "train_plan.h"
#include <cstdint>
#include <cstring>

// One launch covers every layer (blockIdx.y) and every time chunk (blockIdx.x): dW = A^T B, the partial result of a chunk written to its slab, with
//   A[row][m]  : plain array, or the sum of two arrays (grad wrt a layer output = own-row + scattered part)
//   B[row][n]  : plain | relu(array) | product of two arrays (gate = sigma*tanh) | [x_cur | x_past | aux | 0]
//                | one-hot of the row's sample class (k_wgrad3 only)
struct Wg2 {
    const float* A; const float* A2; size_t A_lstride; int lda, M;        // per-layer stride (floats)
    int rowsA;                                                              // rows per batch item in A's array
    int bmode; const float* B1; const float* B2; size_t B_lstride; int ldb, N, Nvalid;
    int rowsB;
    const float* hup; const int* tap; int C, Ap;
    const int* xc;                                                          // bmode 4: B[t][q] = (xc[row] == q), one-hot of the sample class
    int nb, nlayers;
    float* slab; int gstage;
    int row0A[TR_MAXL], row0B[TR_MAXL], R[TR_MAXL];                         // window per layer
    int goff[TR_MAXL], gbias[TR_MAXL], tap_off[TR_MAXL], dil[TR_MAXL];
    int ldc, ncol_groups;                                                   // post: N split into column groups (blockIdx.z)
};

// ---------------------------------------------------------------- the kernel instances, once, in order of preference
// k_wgrad3<BMODE, MPW, NT, TWO_A, MINW>: M = 64 MPW rows of dW, 16 NT columns per column group (both TWO_A forms of each)
//   causal table: C = 64, 128- or 64-class groups | dW1: C = 64 (K = 176 / 128: aux at sample / frame rate), C = 32 with n_aux 33..48
//   | res / skip 1x1 at C = 64 (B = the gate product) | post-net (B rectified), 64-column groups
#define WGRAD3_INSTANCES(X) X(4, 1, 8) X(4, 1, 4)  X(3, 2, 11) X(3, 2, 8) X(3, 1, 7)  X(0, 1, 4) X(0, 4, 4)  X(1, 4, 4)
// k_wgrad2<BMODE, MPW, NTMAX>, every BMODE 0..3: up to 64 MPW rows, up to 16 NTMAX columns per column group (<4, 8>: 256 x 128 blocks)
#define WGRAD2_TILES(X) X(1, 4) X(4, 4) X(2, 12) X(4, 8)
#ifndef QPN_WGRAD_MINW
#define QPN_WGRAD_MINW 2
#endif
// the 256 x 64 one-array launches (post-net pair, skip 1x1) are 512 workgroups = two per CU: the allocation may use half a SIMD's registers
// (round 2 asked for a third of it -- three workgroups per CU; with the staging addresses hoisted that cap spills 80-150 B per lane)
constexpr int wgrad3_minw(int mpw, int nt, bool two_a) { return (mpw == 4 && nt == 4 && !two_a) ? QPN_WGRAD_MINW : 1; }
constexpr int wgrad_ldt(int n) { return ((n + 15) / 32) * 32 + 16; }      // tr_ldt (train_common.h): leading dimension of a staged operand
constexpr size_t wgrad_lds(int Mp, int Np) { return (size_t)32 * (wgrad_ldt(Mp) + wgrad_ldt(Np)) * sizeof(float); }      // one 32-row stage of both operands

struct Wgrad3Inst { int bmode, mpw, nt; };
struct Wgrad2Tile { int mpw, ntmax; };
#define X(BM, MPW, NT) {BM, MPW, NT},
static constexpr Wgrad3Inst WGRAD3_LIST[] = {WGRAD3_INSTANCES(X)};
#undef X
#define X(MPW, NTMAX) {MPW, NTMAX},
static constexpr Wgrad2Tile WGRAD2_LIST[] = {WGRAD2_TILES(X)};
#undef X

// smallest number of column groups g (N % g == 0, 4-column granularity kept) such that an M x N/g block fits a kernel's tile budget: the widest
// k_wgrad2 instance among those with the fewest m-tiles per wave that still hold M rows (M <= 64: <1, 4>, <= 128: <2, 12>, otherwise <4, 8>)
inline int wgrad_col_groups(int M, int N) {
    int mpw = 0, mpw_top = 0, nt_max = 0;
    for (const Wgrad2Tile& t : WGRAD2_LIST) {
        if (64 * t.mpw >= M && (!mpw || t.mpw < mpw)) mpw = t.mpw;
        if (t.mpw > mpw_top) mpw_top = t.mpw;
    }
    if (!mpw) mpw = mpw_top;         // (more rows than any instance holds: the tallest ones, which take the blocks of the row split)
    for (const Wgrad2Tile& t : WGRAD2_LIST) if (t.mpw == mpw && t.ntmax > nt_max) nt_max = t.ntmax;
    for (int g = 1; g <= N / 16; ++g)
        if (N % g == 0 && (N / g) % 4 == 0 && (N / g + 15) / 16 <= nt_max) return g;
    return 1;
}

// ---------------------------------------------------------------- which instance a record gets
struct WgradPick {
    int family;                      // 3: k_wgrad3, 2: k_wgrad2, 0: nothing fits
    int bmode, mpw, nt;              // nt: NT of k_wgrad3, NTMAX of k_wgrad2
    bool two_a; int minw;            // k_wgrad3 only
    size_t lds;                      // dynamic LDS bytes
    int grid[3];                     // (time chunks, layers, column groups)
};

// the preconditions of k_wgrad3<bmode, mpw, nt>: tile counts known at compile time, operands the fast staging path can address
inline bool wgrad3_fits(const Wg2& w, int bmode, int mpw, int nt) {
    const int Ng = w.N / w.ncol_groups;
    if (w.bmode != bmode) return false;
    if (w.rowsB >= (1 << 24) || (int64_t)w.rowsB * (w.C > w.ldb ? w.C : w.ldb) >= (1ll << 32)) return false;      // 24 x 24-bit row x stride products of the fast staging path
    if (w.M != 64 * mpw || Ng != 16 * nt || w.N % w.ncol_groups || (w.Nvalid != w.N && (w.ncol_groups != 1 || w.Nvalid % 4))) return false;
    if (bmode == 3 && (w.ldb != w.C || w.ncol_groups != 1 || (w.C % 4) || (w.Ap % 4) || !w.tap)) return false;
    if (bmode == 3) for (int l = 0; l < w.nlayers; ++l) if (w.tap_off[l] < 0) return false;      // the kernel loads taps unconditionally
    return true;
}

// generic: QPN_WGRAD_GENERIC=1, the run-time-tiled kernel wherever it can take the record (the one-hot operand is k_wgrad3's alone)
inline WgradPick wgrad_pick(const Wg2& w, int nch, bool generic) {
    WgradPick k = {};
    k.bmode = w.bmode >= 1 && w.bmode <= 4 ? w.bmode : 0;
    k.grid[0] = nch; k.grid[1] = w.nlayers; k.grid[2] = w.ncol_groups;
    if (w.bmode == 4 || !generic)
        for (const Wgrad3Inst& i : WGRAD3_LIST)
            if (wgrad3_fits(w, i.bmode, i.mpw, i.nt)) {
                k.family = 3; k.mpw = i.mpw; k.nt = i.nt; k.two_a = w.A2 != nullptr; k.minw = wgrad3_minw(i.mpw, i.nt, k.two_a);
                k.lds = wgrad_lds(64 * i.mpw, 16 * i.nt);
                return k;
            }
    if (w.bmode == 4) return k;
    const int Mp = (w.M + 15) & ~15, Np = ((w.N / w.ncol_groups) + 15) & ~15;
    for (const Wgrad2Tile& t : WGRAD2_LIST)
        if (Mp / 16 <= 4 * t.mpw && Np / 16 <= t.ntmax) { k.family = 2; k.mpw = t.mpw; k.nt = t.ntmax; k.lds = wgrad_lds(Mp, Np); return k; }
    return k;
}

// More output rows than a workgroup's tile budget (n_skipch / n_quantize > 256): blocks of 256 rows of dW, each a launch of its own -- the A operand's
// columns, the slab rows and the bias entries shift together.  (No allocation: the launcher runs this every step.)
inline int wgrad_n_row_blocks(const Wg2& w) { return (w.M <= 256 || w.bmode == 4) ? 1 : (w.M + 255) / 256; }
inline Wg2 wgrad_row_block(const Wg2& w, int i) {      // block i of wgrad_n_row_blocks(w)
    if (wgrad_n_row_blocks(w) == 1) return w;
    const int m0 = 256 * i;
    Wg2 sub = w;
    sub.A = w.A + m0; if (w.A2) sub.A2 = w.A2 + m0;
    sub.M = w.M - m0 < 256 ? w.M - m0 : 256;
    for (int l = 0; l < w.nlayers; ++l) { sub.goff[l] = w.goff[l] + m0 * w.ldc; if (w.gbias[l] >= 0) sub.gbias[l] = w.gbias[l] + m0; }
    sub.ncol_groups = wgrad_col_groups(sub.M, sub.N);
    return sub;
}

// ---------------------------------------------------------------- the five records of a step
struct WgradView {                   // the step's geometry
    int C, S, Q, L, B, N1, BL, Ap, Ktp, hoist;
    int s_out[TR_MAXL], tap_off[TR_MAXL], dilation[TR_MAXL], adaptive[TR_MAXL];
};
struct WgradBufs {
    const float* DZ; const float* DXA; const float* DXB; const float* DS0; const float* DY0; const float* dlogits;      // gradients (DXA / DXB: index 0 of the L + 1 arrays)
    const float* X; const float* gate; const float* S0; const float* Y0; const float* HUP;      // gate: the array that holds sigma * tanh (tile path: TrainParams::TH, GEMM path: TrainGemm::G)
    const int* TAP; const int* XC;
    float* slab; int gstage;
};
struct WgradFlags {
    bool wr_summed;                  // the stack queue's tiles have replaced the own-row part of dXout by the sum of both parts (store_dx in k_stack_bwd)
    bool post_pair;                  // QPN_POST_WGRAD_PAIR: both post-net contractions as one two-"layer" launch where their shapes agree
    bool col_groups;                 // N split into column groups (the tile kernels); the GEMM path tiles N itself
    bool fixed_taps;                 // fixed layers read their tap table as well (the tile path: every layer has one); otherwise row - dilation
};
inline Wg2 wgrad_rec_base(const WgradView& v, const WgradBufs& b) {
    Wg2 w; memset(&w, 0, sizeof(w));
    w.slab = b.slab; w.gstage = b.gstage; w.nb = v.B; w.C = v.C; w.Ap = v.Ap; w.hup = b.HUP; w.tap = b.TAP; w.ncol_groups = 1;
    return w;
}
// dW1_l = dZ_l^T [x_cur | x_past | aux],  bias1 grads = colsum(dZ_l)
inline Wg2 wgrad_rec_w1(const WgradView& v, const TrainSlabs& sl, const WgradBufs& b, const WgradFlags& f) {
    const int C = v.C, N1 = v.N1;
    Wg2 w = wgrad_rec_base(v, b);
    w.A = b.DZ; w.A2 = nullptr; w.A_lstride = (size_t)v.B * N1 * 2 * C; w.lda = 2 * C; w.M = 2 * C; w.rowsA = N1;
    w.bmode = 3; w.B1 = b.X; w.B2 = nullptr; w.B_lstride = (size_t)v.B * N1 * C; w.ldb = C; w.N = v.Ktp; w.Nvalid = v.hoist ? 2 * C : 2 * C + v.Ap; w.rowsB = N1;      // (aux hoist: no aux columns -- k_aux_tail)
    w.nlayers = v.L; w.ldc = v.Ktp; w.ncol_groups = f.col_groups ? wgrad_col_groups(w.M, w.N) : 1;
    for (int l = 0; l < v.L; ++l) {
        w.row0A[l] = w.row0B[l] = v.s_out[l]; w.R[l] = N1 - v.s_out[l]; w.goff[l] = sl.g_w1[l]; w.gbias[l] = sl.g_b1[l];
        w.tap_off[l] = (f.fixed_taps || v.adaptive[l]) ? v.tap_off[l] : -1; w.dil[l] = v.dilation[l];
    }
    return w;
}
// dWr_l = dXout_l^T g_l (dXout_l = grad wrt X[l+1]); zero rows for the last layer
inline Wg2 wgrad_rec_wr(const WgradView& v, const TrainSlabs& sl, const WgradBufs& b, const WgradFlags& f) {
    const int C = v.C, N1 = v.N1, L = v.L;
    const size_t nDX = (size_t)v.B * N1 * C;
    Wg2 w = wgrad_rec_base(v, b);
    w.A = b.DXA + nDX; w.A2 = f.wr_summed ? nullptr : b.DXB + nDX; w.A_lstride = nDX; w.lda = C; w.M = C; w.rowsA = N1;
    w.bmode = 0; w.B1 = b.gate; w.B2 = nullptr; w.B_lstride = nDX; w.ldb = C; w.N = C; w.Nvalid = C; w.rowsB = N1; w.ldc = C;
    w.nlayers = L; w.ncol_groups = f.col_groups ? wgrad_col_groups(w.M, w.N) : 1;
    for (int l = 0; l < L; ++l) {
        w.row0A[l] = w.row0B[l] = v.s_out[l];
        w.R[l] = l == L - 1 ? 0 : N1 - v.s_out[l]; w.goff[l] = sl.g_wr[l]; w.gbias[l] = sl.g_br[l]; w.tap_off[l] = -1; w.dil[l] = 0;
    }
    return w;
}
// dWs_l = dS0^T g_l over the last BL rows; the shared skip-bias grad = colsum(dS0) (layer 0's block only)
inline Wg2 wgrad_rec_skip(const WgradView& v, const TrainSlabs& sl, const WgradBufs& b, const WgradFlags& f) {
    const int C = v.C, S = v.S, N1 = v.N1, BL = v.BL;
    Wg2 w = wgrad_rec_base(v, b);
    w.nlayers = v.L;
    w.A = b.DS0; w.A2 = nullptr; w.A_lstride = 0; w.lda = S; w.M = S; w.rowsA = BL;
    w.bmode = 0; w.B1 = b.gate; w.B2 = nullptr; w.B_lstride = (size_t)v.B * N1 * C; w.ldb = C; w.N = C; w.Nvalid = C; w.rowsB = N1; w.ldc = C;
    w.ncol_groups = f.col_groups ? wgrad_col_groups(w.M, w.N) : 1;
    for (int l = 0; l < v.L; ++l) { w.row0A[l] = 0; w.row0B[l] = N1 - BL; w.R[l] = BL; w.goff[l] = sl.g_ws[l]; w.gbias[l] = l == 0 ? sl.g_bs : -1; w.tap_off[l] = -1; }
    return w;
}
// post-net: part 0: dW2[q][s] = dlogits^T relu(Y0), part 1: dW1[o][s] = dY0^T relu(S0); N split into 64-column groups
// (S no multiple of 64: as few groups as fit a kernel's tile budget -- one group of all S columns fits none from S = 144 on, with Q or S rows > 128).
// wgrad_post_paired: both contractions have the same shape -- part 0 is then ONE launch with the second as "layer 1" (strides = the distance between
// the arrays, modulo 2^64), 2 x 256 workgroups = two per CU, so one's staging runs under the other's MFMAs (alone, each launch put one workgroup on
// a CU: 35 % of every stage with the matrix cores idle, in-kernel stamps), and there is no part 1
inline bool wgrad_post_paired(const WgradView& v, const WgradFlags& f) { return v.Q == v.S && f.post_pair; }
inline Wg2 wgrad_rec_post(const WgradView& v, const TrainSlabs& sl, const WgradBufs& b, const WgradFlags& f, int part) {
    const int S = v.S, BL = v.BL;
    Wg2 w = wgrad_rec_base(v, b);
    w.nlayers = 1; w.bmode = 1; w.rowsA = w.rowsB = BL; w.R[0] = BL; w.tap_off[0] = -1;
    w.M = w.lda = part ? S : v.Q; w.A = part ? b.DY0 : b.dlogits; w.B1 = part ? b.S0 : b.Y0; w.ldb = S; w.N = S; w.Nvalid = S; w.ldc = S;
    w.goff[0] = part ? sl.g_p1 : sl.g_p2; w.gbias[0] = part ? sl.g_bp1 : sl.g_bp2;
    w.ncol_groups = !f.col_groups ? 1 : S % 64 == 0 ? S / 64 : wgrad_col_groups(w.M, S);
    if (!part && wgrad_post_paired(v, f)) {
        w.nlayers = 2;
        w.A_lstride = (size_t)(((intptr_t)b.DY0 - (intptr_t)b.dlogits) / (intptr_t)sizeof(float));
        w.B_lstride = (size_t)(((intptr_t)b.S0 - (intptr_t)b.Y0) / (intptr_t)sizeof(float));
        w.R[1] = BL; w.tap_off[1] = -1; w.goff[1] = sl.g_p1; w.gbias[1] = sl.g_bp1;
    }
    return w;
}
// causal conv table: dWc[tap][c][q] = (dX0)^T onehot(class of x[t-1+tap]); bias = colsum(dX0).  64-class groups: 512 workgroups, two per CU (29 -> 25 us)
inline Wg2 wgrad_rec_causal(const WgradView& v, const TrainSlabs& sl, const WgradBufs& b) {
    const int C = v.C, Q = v.Q, N1 = v.N1;
    Wg2 w = wgrad_rec_base(v, b);
    w.nlayers = 2; w.ncol_groups = Q / (Q % 64 == 0 ? 64 : 128); w.bmode = 4; w.xc = b.XC; w.B1 = w.B2 = nullptr; w.B_lstride = 0;
    w.A = b.DXA; w.A2 = b.DXB; w.A_lstride = 0; w.lda = C; w.M = C; w.rowsA = N1;
    w.N = Q; w.Nvalid = Q; w.rowsB = N1 + 1; w.ldb = 0; w.ldc = Q;
    for (int tp = 0; tp < 2; ++tp) { w.row0A[tp] = 0; w.row0B[tp] = tp; w.R[tp] = N1; w.goff[tp] = sl.g_cw + tp * C * Q; w.gbias[tp] = tp == 0 ? sl.g_cb : -1; w.tap_off[tp] = -1; w.dil[tp] = 0; }
    return w;
}

// ---------------------------------------------------------------- the GEMM path's form of a record (k_gemm_tn, train_gemm.hip)
enum { BM_PLAIN = 0, BM_RELU = 1, BM_GATHER = 3 };
struct TArgs {
    int M, N;                        // valid rows / columns of dW
    int nb, nsplit;
    const float* a; const float* a2; long a_ls; int lda; int rowsA;      // A[t][m] (+ a2), per-layer stride, rows per batch item
    const float* b1; long b_ls; int ldb; int rowsB;                      // B[t][n]
    const float* hup; const int* tap; int C, Ap;                         // BM_GATHER: [x_cur | x_past | aux]
    float* slab; long gstage; int ldc;
    int row0A[TR_MAXL], row0B[TR_MAXL], R[TR_MAXL], goff[TR_MAXL], gbias[TR_MAXL], tap_off[TR_MAXL], dil[TR_MAXL];
};
// (a record built without column groups; the kernel tiles M and N itself and pads neither: N = the valid columns.  hup / tap: read in BM_GATHER only)
inline TArgs targs_of(const Wg2& w, int nsplit) {
    TArgs a; memset(&a, 0, sizeof(a));
    a.M = w.M; a.N = w.Nvalid; a.nb = w.nb; a.nsplit = nsplit;
    a.a = w.A; a.a2 = w.A2; a.a_ls = (long)w.A_lstride; a.lda = w.lda; a.rowsA = w.rowsA;
    a.b1 = w.B1; a.b_ls = (long)w.B_lstride; a.ldb = w.ldb; a.rowsB = w.rowsB;
    if (w.bmode == BM_GATHER) { a.hup = w.hup; a.tap = w.tap; }
    a.C = w.C; a.Ap = w.Ap; a.slab = w.slab; a.gstage = w.gstage; a.ldc = w.ldc;
    for (int l = 0; l < w.nlayers; ++l) {
        a.row0A[l] = w.row0A[l]; a.row0B[l] = w.row0B[l]; a.R[l] = w.R[l]; a.goff[l] = w.goff[l]; a.gbias[l] = w.gbias[l]; a.tap_off[l] = w.tap_off[l]; a.dil[l] = w.dil[l];
    }
    return a;
}
