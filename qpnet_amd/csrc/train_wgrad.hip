// train_wgrad.hip -- the weight-gradient time contractions of the tile path: dW[m][n] = sum_t A[t][m] B[t][n], one launch per weight family over
// (time chunk, layer, column group), partial slabs (deterministic), bias grads = colsum(A).
//   k_wgrad2 : tile counts read at run time, the fallback for every geometry
//   k_wgrad3 : tile counts known at compile time, for the geometries listed in train_wgrad_plan.h
// Which instance a record gets, the row-block split and the records themselves are host arithmetic (train_wgrad_plan.h: wgrad_pick,
// wgrad_row_block, wgrad_rec_*); this unit holds the kernels and the one switch from a pick to its instance (qpn_launch_wgrad).
#include "train_common.h"

// ------------------------------------------------------------------------------------------ weight gradients, v2
// A workgroup (4 waves) computes the WHOLE output block dW[M][N] of its layer (blockIdx.y) for its chunk of rows (blockIdx.x): wave w owns m-tiles
// {w, w+4, ...} x all n-tiles, operands staged once per 32 rows with 16-byte loads (no re-reads across output tiles), partial result written to
// its slab.  (The operands a record can name: Wg2, train_wgrad_plan.h.)
struct Wg2L {            // per-workgroup scalars hoisted out of the kernel-argument arrays
    const float* A; const float* A2; const float* B1; const float* B2; const float* hup; const int* tap;
    int lda, ldb, M, Ng, Nvalid, rowsA, rowsB, row0A, row0B, C, Ap, dil, nb, ncol0, rend;
    unsigned uR;
};

// tap rows of the stage starting at rs (pitch-dependent gather source rows), loaded one stage ahead of their use
template <int NB>
__device__ __forceinline__ void wg_taps(const Wg2L& q, int rs, int (&tp)[NB], bool b_act, int b_row0, int b_rstep) {
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int r = b_row0 + k * b_rstep, rr = rs + r;
        int v = 0;
        if (b_act && r < 32 && rr < q.rend) {
            const unsigned b = q.nb > 1 ? (unsigned)rr / q.uR : 0u; const int i = rr - (int)(b * q.uR);
            const int nloc = q.row0B + i;
            v = q.tap ? q.tap[(size_t)b * q.rowsB + nloc] : nloc - q.dil;
        }
        tp[k] = v;
    }
}

template <int BMODE, int NA, int NB>
__device__ __forceinline__ void wg_fetch(const Wg2L& q, int rs, float4 (&ra)[NA], float4 (&ra2)[NA], float4 (&rb)[NB], float4 (&rb2)[NB], const int (&tpv)[NB],
                                         bool a_act, int a_row0, int a_rstep, int a_col, bool b_act, int b_row0, int b_rstep, int b_col) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int r = a_row0 + k * a_rstep, rr = rs + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), v2 = v;
        if (a_act && r < 32 && rr < q.rend && a_col < q.M) {
            const unsigned b = q.nb > 1 ? (unsigned)rr / q.uR : 0u; const int i = rr - (int)(b * q.uR);
            const size_t o = ((size_t)b * q.rowsA + q.row0A + i) * q.lda + a_col;
            v = *(const float4*)(q.A + o);
            if (q.A2) v2 = *(const float4*)(q.A2 + o);
        }
        ra[k] = v; ra2[k] = v2;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int r = b_row0 + k * b_rstep, rr = rs + r;
        const int n = q.ncol0 + b_col;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), v2 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (b_act && r < 32 && rr < q.rend && b_col < q.Ng && n < q.Nvalid) {
            const unsigned b = q.nb > 1 ? (unsigned)rr / q.uR : 0u; const int i = rr - (int)(b * q.uR);
            const int nloc = q.row0B + i;
            const size_t row = (size_t)b * q.rowsB + nloc;
            if (BMODE <= 1) v = *(const float4*)(q.B1 + row * q.ldb + n);
            else if (BMODE == 2) { v = *(const float4*)(q.B1 + row * q.ldb + n); v2 = *(const float4*)(q.B2 + row * q.ldb + n); }
            else {
                if (n < q.C) v = *(const float4*)(q.B1 + row * q.C + n);
                else if (n < 2 * q.C) v = *(const float4*)(q.B1 + ((size_t)b * q.rowsB + tpv[k]) * q.C + (n - q.C));
                else v = *(const float4*)(q.hup + row * q.Ap + (n - 2 * q.C));
            }
        }
        rb[k] = v; rb2[k] = v2;
    }
}

template <int BMODE, int MPW, int NTMAX>
__global__ __launch_bounds__(256) void k_wgrad2(Wg2 w, int nch) {
    extern __shared__ float sm[];
    constexpr int RS = 32;
    constexpr int NA = 2 * MPW;              // staging passes of A: 32 rows / (256 / (Mp/4)) with Mp <= 64*MPW
    constexpr int NB = (NTMAX + 1) / 2 + 1;  // staging passes of B: ceil(32 / floor(256 / (Np/4))), Np <= 16*NTMAX
    const int y = blockIdx.y, ch = blockIdx.x, zg = blockIdx.z;
    const int Mp = (w.M + 15) & ~15, Ng = w.N / w.ncol_groups, Np = (Ng + 15) & ~15;
    const int ldA = tr_ldt(Mp), ldB = tr_ldt(Np);
    float* As = sm; float* Bs = sm + RS * ldA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int MT = Mp / 16, NT = Np / 16;
    const int Rl = w.R[y];
    const int64_t total = (int64_t)Rl * w.nb;
    const int64_t per = ((total + nch - 1) / nch + RS - 1) / RS * RS;
    const int rbeg = (int)(per * ch), rend = (int)(per * ch + per < total ? per * ch + per : total);
    Wg2L q;
    q.A = w.A + (size_t)y * w.A_lstride; q.A2 = w.A2 ? w.A2 + (size_t)y * w.A_lstride : nullptr;
    q.B1 = w.B1 + (size_t)y * w.B_lstride; q.B2 = w.B2 ? w.B2 + (size_t)y * w.B_lstride : nullptr;
    q.hup = w.hup; q.tap = (w.tap && w.tap_off[y] >= 0) ? w.tap + w.tap_off[y] : nullptr;
    q.lda = w.lda; q.ldb = w.ldb; q.M = w.M; q.Ng = Ng; q.Nvalid = w.Nvalid; q.rowsA = w.rowsA; q.rowsB = w.rowsB;
    q.row0A = w.row0A[y]; q.row0B = w.row0B[y]; q.C = w.C; q.Ap = w.Ap; q.dil = w.dil[y]; q.nb = w.nb; q.ncol0 = zg * Ng; q.rend = rend;
    q.uR = (unsigned)(Rl > 0 ? Rl : 1);
    const int gbias = zg == 0 ? w.gbias[y] : -1, goff = w.goff[y];
    const int A4 = Mp / 4, B4 = Np / 4;
    const int a_col = (tid % A4) * 4, a_row0 = tid / A4, a_rstep = 256 / A4;
    const int b_rstep = 256 / B4 > 0 ? 256 / B4 : 1;
    const int b_col = (tid % B4) * 4, b_row0 = tid / B4;
    const bool a_act = tid < a_rstep * A4, b_act = tid < b_rstep * B4;
    f32x4 acc[MPW][NTMAX];
#pragma unroll
    for (int a = 0; a < MPW; ++a)
#pragma unroll
        for (int b = 0; b < NTMAX; ++b) acc[a][b] = (f32x4){0, 0, 0, 0};
    float csum = 0.f;
    float4 ra[NA], ra2[NA], rb[NB], rb2[NB];
    int tpv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) tpv[k] = 0;
    if (BMODE == 3 && rbeg < rend) wg_taps<NB>(q, rbeg, tpv, b_act, b_row0, b_rstep);
    if (rbeg < rend) wg_fetch<BMODE, NA, NB>(q, rbeg, ra, ra2, rb, rb2, tpv, a_act, a_row0, a_rstep, a_col, b_act, b_row0, b_rstep, b_col);
    if (BMODE == 3 && rbeg + RS < rend) wg_taps<NB>(q, rbeg + RS, tpv, b_act, b_row0, b_rstep);
    const int g = lane >> 4, cl = lane & 15;
    for (int rs = rbeg; rs < rend; rs += RS) {
        // registers -> LDS
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int r = a_row0 + k * a_rstep;
            if (a_act && r < RS) {
                float4 v = ra[k];
                v.x += ra2[k].x; v.y += ra2[k].y; v.z += ra2[k].z; v.w += ra2[k].w;
                *(float4*)(As + (size_t)r * ldA + a_col) = v;
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int r = b_row0 + k * b_rstep;
            if (b_act && r < RS) {
                float4 v = rb[k];
                if (BMODE == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                else if (BMODE == 2) { v.x *= rb2[k].x; v.y *= rb2[k].y; v.z *= rb2[k].z; v.w *= rb2[k].w; }
                *(float4*)(Bs + (size_t)r * ldB + b_col) = v;
            }
        }
        __syncthreads();
        // next stage's rows fly while the matrix cores work on this one
        if (rs + RS < rend) wg_fetch<BMODE, NA, NB>(q, rs + RS, ra, ra2, rb, rb2, tpv, a_act, a_row0, a_rstep, a_col, b_act, b_row0, b_rstep, b_col);
        if (BMODE == 3 && rs + 2 * RS < rend) wg_taps<NB>(q, rs + 2 * RS, tpv, b_act, b_row0, b_rstep);   // gather rows of the stage after next
        if (gbias >= 0 && tid < q.M) { float s = 0.f; for (int r = 0; r < RS; ++r) s += As[r * ldA + tid]; csum += s; }
#pragma unroll
        for (int ks = 0; ks < RS / 4; ++ks) {
            float bfr[NTMAX];
#pragma unroll
            for (int nt = 0; nt < NTMAX; ++nt) bfr[nt] = nt < NT ? Bs[(4 * ks + g) * ldB + 16 * nt + cl] : 0.f;
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi) {
                const int mt = wave + 4 * mi;
                if (mt < MT) {
                    const float a = As[(4 * ks + g) * ldA + 16 * mt + cl];
#pragma unroll
                    for (int nt = 0; nt < NTMAX; ++nt)
                        if (nt < NT) acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bfr[nt], acc[mi][nt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    float* out = w.slab + (size_t)ch * w.gstage;
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
        const int mt = wave + 4 * mi;
        if (mt >= MT) continue;
#pragma unroll
        for (int nt = 0; nt < NTMAX; ++nt) {
            if (nt >= NT) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = 16 * mt + 4 * (lane >> 4) + i, n = 16 * nt + (lane & 15);
                if (m < q.M && n < Ng) out[goff + (size_t)m * w.ldc + q.ncol0 + n] = acc[mi][nt][i];
            }
        }
    }
    if (gbias >= 0 && tid < q.M) out[gbias + tid] = csum;
}

// ------------------------------------------------------------------------------------------ weight gradients, v3
// Same contraction and slab layout as k_wgrad2, for the geometries where the tile counts are known at compile time
// (M = 64*MPW rows of dW -> every wave owns exactly MPW m-tiles, N per column group = 16*NT): no per-tile guards in
// the matrix-core loop, no branches around the staging loads (out-of-range rows are clamped and zeroed, the three
// sources of the [x_cur | x_past | aux] operand become one per-thread base/stride), bias column sums taken from the
// staging registers instead of 32 LDS reads per stage.  k_wgrad2 stays as the generic fallback.
// (ch, y, zg) = (time chunk, layer, column group) of this workgroup: blockIdx of the one-contraction launches, decoded from a flat index in k_wgrad_tail
template <int BMODE, int MPW, int NT, bool TWO_A>
__device__ __forceinline__ void wgrad3_body(const Wg2& w, const int nch, const int ch, const int y, const int zg) {
    extern __shared__ float sm[];
    constexpr int RS = 32, Mp = 64 * MPW, Np = 16 * NT;
    constexpr int ldA = ((Mp + 15) / 32) * 32 + 16, ldB = ((Np + 15) / 32) * 32 + 16;       // tr_ldt
    constexpr int A4 = Mp / 4, ARS = 256 / A4, NA = RS / ARS;                               // A: every thread active, NA full passes
    constexpr int B4 = Np / 4, BRS = 256 / B4, NB = (RS + BRS - 1) / BRS;                   // B: threads < BRS*B4 active
    static_assert(256 % A4 == 0 && RS % ARS == 0, "A staging must tile the stage's rows exactly");
    constexpr int BUF = RS * (ldA + ldB);                                                   // floats of one stage buffer
    float* As = sm; float* Bs = sm + RS * ldA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Rl = w.R[y];
    const int64_t total = (int64_t)Rl * w.nb;
    const int64_t per = ((total + nch - 1) / nch + RS - 1) / RS * RS;
    const int rbeg = (int)(per * ch), rend = (int)(per * ch + per < total ? per * ch + per : total);
    const float* A = w.A + (size_t)y * w.A_lstride;
    const float* A2 = TWO_A ? w.A2 + (size_t)y * w.A_lstride : nullptr;      // TWO_A: the A operand is the sum of two arrays (a template flag: the second
                                                                               // staging set costs 32 registers the one-array launches need for a third workgroup per CU)
    const float* B1 = BMODE == 4 ? nullptr : w.B1 + (size_t)y * w.B_lstride;
    const float* B2 = w.B2 ? w.B2 + (size_t)y * w.B_lstride : nullptr;
    const int* tap = BMODE == 3 ? w.tap + w.tap_off[y] : nullptr;      // BMODE 3: a tap table for every layer (the launcher checks)
    const int row0A = w.row0A[y], row0B = w.row0B[y], ncol0 = zg * Np;
    const unsigned uR = (unsigned)(Rl > 0 ? Rl : 1);
    const bool multi = w.nb > 1;
    const int gbias = zg == 0 ? w.gbias[y] : -1, goff = w.goff[y];
    const int a_col = (tid % A4) * 4, a_row0 = tid / A4;
    const int b_col = (tid % B4) * 4, b_row0 = tid / B4;
    const int n = ncol0 + b_col;
    const bool b_act = tid < BRS * B4;
    const bool b_pad = n >= w.Nvalid;                           // zero padding columns of the operand (K padded to 16)
    // B operand source of this thread's four columns
    const float* bbase; int bstride; bool use_tap = false;
    if (BMODE == 3) {
        if (n < w.C) { bbase = B1 + n; bstride = w.C; }
        else if (n < 2 * w.C) { bbase = B1 + (n - w.C); bstride = w.C; use_tap = true; }
        else { bbase = w.hup + (b_pad ? 0 : n - 2 * w.C); bstride = w.Ap; }
    } else if (BMODE == 4) { bbase = nullptr; bstride = 0; }
    else { bbase = B1 + n; bstride = w.ldb; }
    const ptrdiff_t b2off = (BMODE == 2) ? (B2 - B1) : 0;

    f32x4 acc[MPW][NT];
#pragma unroll
    for (int a = 0; a < MPW; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = (f32x4){0, 0, 0, 0};
    float4 cs4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ra[NA], ra2[NA], rb[NB], rb2[NB];
    int tpv[NB];
    int rbi[NB];                     // BMODE 4: sample class of the staged row (the one-hot is made when the stage goes to LDS)
    unsigned okA = 0, okB = 0;       // bit k: staged row k is a real row.  The loaded registers are NOT touched before the stage goes to
                                     // LDS: a select on a just-loaded value puts an s_waitcnt vmcnt in front of the matrix-core loop
                                     // (measured with in-kernel stamps: 6-8 k cycles per stage in the skip 1x1 launch)

    // Staging addresses.  A stage that lies inside one batch item and ends before rend -- all but the last one or two of a chunk -- takes
    // the FAST form: one uniform base per operand and stage plus per-thread offsets fixed for the whole kernel.  The generic form below
    // (row clamp, per-row batch split, 64-bit multiplies: ~650 instructions = 5.7 k cycles per stage in the dW1 launch, as long as its
    // 176 MFMAs) only runs for the others.
    const unsigned a_voff = (unsigned)a_row0 * (unsigned)w.lda + (unsigned)a_col, a_kstep = (unsigned)ARS * (unsigned)w.lda;
    const unsigned b_voff = (unsigned)b_row0 * (unsigned)w.ldb + (unsigned)n, b_kstep = (unsigned)BRS * (unsigned)w.ldb;

    // rows of a stage: r in [0,32); rows at or past rend are clamped to the last valid row and zeroed
    auto rowsplit = [&](int rr, int& b, int& i) { if (multi) { b = (int)((unsigned)rr / uR); i = rr - b * (int)uR; } else { b = 0; i = rr; } };
    auto stage_fast = [&](int rs, int& b0, int& i0) {       // uniform
        rowsplit(rs, b0, i0);
        return rs + RS <= rend && i0 + RS <= (int)uR;
    };
    // (every thread loads its row's tap entry, needed or not: a per-thread condition around the load becomes a branch with an
    //  s_waitcnt behind each load, which also drains the operand loads issued just before -- the next stage's prefetch no longer
    //  ran under the MFMAs)
    auto taps = [&](int rs) {
        int b0, i0;
        if (stage_fast(rs, b0, i0)) {
            const int* tst = tap + ((size_t)b0 * w.rowsB + row0B + i0);
#pragma unroll
            for (int k = 0; k < NB; ++k) { const int r = b_row0 + k * BRS; tpv[k] = tst[r < RS ? r : b_row0]; }
            return;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int r = b_row0 + k * BRS;
            int rr = rs + r; rr = rr < rend ? rr : rend - 1;
            int b, i; rowsplit(rr, b, i);
            const int nloc = row0B + i;
            tpv[k] = tap[(size_t)b * w.rowsB + nloc];
        }
    };
    // Both forms only compute ADDRESSES (and the row masks) under the uniform branch; the loads themselves are issued once, behind it.
    // [Loads in both arms made the merged values phi nodes: the copies at the join need the data, i.e. an s_waitcnt vmcnt(0) in front of
    //  the matrix-core loop -- the whole memory latency exposed in every stage.]
    auto fetch = [&](int rs) {
        const float* pa[NA]; const float* pb[NB]; const int* pi[NB];
        int b0, i0;
        if (stage_fast(rs, b0, i0)) {
            const float* Ast = A + ((size_t)b0 * w.rowsA + row0A + i0) * w.lda;
#pragma unroll
            for (int k = 0; k < NA; ++k) pa[k] = Ast + (k * a_kstep + a_voff);
            okA = ~0u;
            const size_t brow = (size_t)b0 * w.rowsB + row0B + i0;
            const float* bsrc = BMODE == 3 ? bbase + (size_t)b0 * w.rowsB * bstride : B1 + brow * w.ldb;
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = b_row0 + k * BRS;
                if (BMODE == 4) pi[k] = w.xc + brow + (r < RS ? r : b_row0);
                else if (BMODE == 3) {
                    const unsigned row = use_tap ? (unsigned)tpv[k] : (unsigned)(row0B + i0 + (r < RS ? r : b_row0));
                    pb[k] = bsrc + __umul24(row, (unsigned)bstride);
                } else pb[k] = bsrc + ((r < RS ? k * b_kstep : 0u) + b_voff);
            }
            okB = b_pad ? 0u : ~0u;
        } else {
            okA = 0; okB = 0;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int r = a_row0 + k * ARS;
                int rr = rs + r; const bool ok = rr < rend; rr = ok ? rr : rend - 1;
                int b, i; rowsplit(rr, b, i);
                pa[k] = A + (((size_t)b * w.rowsA + row0A + i) * w.lda + a_col);
                okA |= ok ? 1u << k : 0u;
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = b_row0 + k * BRS;
                int rr = rs + r; const bool ok = r < RS && rr < rend && !b_pad; rr = rr < rend ? rr : rend - 1;
                int b, i; rowsplit(rr, b, i);
                const size_t row = (size_t)b * w.rowsB + ((BMODE == 3 && use_tap) ? tpv[k] : row0B + i);
                if (BMODE == 4) pi[k] = w.xc + row; else pb[k] = bbase + row * bstride;
                okB |= ok ? 1u << k : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            ra[k] = *(const float4*)pa[k];
            if (TWO_A) ra2[k] = *(const float4*)(pa[k] + (A2 - A));
        }
        if (b_act) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                if (BMODE == 4) rbi[k] = *pi[k];
                else {
                    rb[k] = *(const float4*)pb[k];
                    if (BMODE == 2) rb2[k] = *(const float4*)(pb[k] + b2off);
                }
            }
        }
    };
    if (rbeg < rend) {
        if (BMODE == 3) taps(rbeg);
        fetch(rbeg);
        if (BMODE == 3 && rbeg + RS < rend) taps(rbeg + RS);
    }
    const int g = lane >> 4, cl = lane & 15;
    // staging registers -> LDS buffer `buf`
    auto to_lds = [&](int buf) {
        float* Ab = As + buf * BUF; float* Bb = Bs + buf * BUF;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            float4 v = ra[k];
            if (TWO_A) { v.x += ra2[k].x; v.y += ra2[k].y; v.z += ra2[k].z; v.w += ra2[k].w; }
            { const bool ok = (okA >> k) & 1u; v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f; }     // (component-wise: a select between float4 objects makes the staging arrays addressable -> scratch)
            cs4.x += v.x; cs4.y += v.y; cs4.z += v.z; cs4.w += v.w;
            *(float4*)(Ab + (size_t)(a_row0 + k * ARS) * ldA + a_col) = v;
        }
        if (b_act) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = b_row0 + k * BRS;
                if (r < RS) {
                    float4 v;
                    if (BMODE == 4) { const int dlt = rbi[k] - n; v = make_float4(dlt == 0 ? 1.f : 0.f, dlt == 1 ? 1.f : 0.f, dlt == 2 ? 1.f : 0.f, dlt == 3 ? 1.f : 0.f); }
                    else v = rb[k];
                    if (BMODE == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    else if (BMODE == 2) { v.x *= rb2[k].x; v.y *= rb2[k].y; v.z *= rb2[k].z; v.w *= rb2[k].w; }
                    { const bool ok = (okB >> k) & 1u; v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f; }
                    *(float4*)(Bb + (size_t)r * ldB + b_col) = v;
                }
            }
        }
    };
    auto ksteps = [&](int buf, int k0, int k1) {
        const float* Ab = As + buf * BUF; const float* Bb = Bs + buf * BUF;
#pragma unroll
        for (int ks = k0; ks < k1; ++ks) {
            float bfr[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bfr[nt] = Bb[(4 * ks + g) * ldB + 16 * nt + cl];
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi) {
                const float a = Ab[(4 * ks + g) * ldA + 16 * (wave + 4 * mi) + cl];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bfr[nt], acc[mi][nt], 0, 0, 0);
            }
        }
    };
    for (int rs = rbeg; rs < rend; rs += RS) {
        to_lds(0);
        __syncthreads();
        // next stage's rows fly while the matrix cores work on this one
        if (rs + RS < rend) {
            fetch(rs + RS);
            if (BMODE == 3 && rs + 2 * RS < rend) taps(rs + 2 * RS);       // gather rows of the stage after next
        }
        ksteps(0, 0, RS / 4);
        __syncthreads();
    }
    float* out = w.slab + (size_t)ch * w.gstage;
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
        const int mt = wave + 4 * mi;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = 16 * mt + 4 * (lane >> 4) + i, nn = 16 * nt + (lane & 15);
                out[goff + (size_t)m * w.ldc + ncol0 + nn] = acc[mi][nt][i];
            }
        }
    }
    if (gbias >= 0) {          // bias grads: column sums of A, reduced over the ARS row groups of the staging layout
        *(float4*)(sm + (size_t)a_row0 * Mp + a_col) = cs4;
        __syncthreads();
        if (tid < Mp) { float s = 0.f; for (int r = 0; r < ARS; ++r) s += sm[r * Mp + tid]; out[gbias + tid] = s; }
    }
}
template <int BMODE, int MPW, int NT, bool TWO_A, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void k_wgrad3(Wg2 w, int nch) {          // MINW: waves per SIMD the register allocation must allow
    wgrad3_body<BMODE, MPW, NT, TWO_A>(w, nch, blockIdx.x, blockIdx.y, blockIdx.z);
}

// ------------------------------------------------------------------------------------------ launcher
template <int BMODE, int MPW, int NTMAX>
static void launch_wgrad2_k(const Wg2& w, int nch, size_t lds, hipStream_t stream) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_wgrad2<BMODE, MPW, NTMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_wgrad2<BMODE, MPW, NTMAX>), dim3(nch, w.nlayers, w.ncol_groups), dim3(256), lds, stream, w, nch);
}
template <int BMODE, int MPW, int NT, bool TWO_A>
static void launch_wgrad3_k(const Wg2& w, int nch, size_t lds, hipStream_t stream) {
    constexpr int MINW = wgrad3_minw(MPW, NT, TWO_A);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_wgrad3<BMODE, MPW, NT, TWO_A, MINW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_wgrad3<BMODE, MPW, NT, TWO_A, MINW>), dim3(nch, w.nlayers, w.ncol_groups), dim3(256), lds, stream, w, nch);
}
// the instance a pick names: the lists of train_wgrad_plan.h, expanded
static bool launch_pick(const Wg2& w, const WgradPick& k, int nch, hipStream_t stream) {
    if (k.family == 3) {
#define X(BM, MPW, NT) \
        if (k.bmode == BM && k.mpw == MPW && k.nt == NT) { \
            if (k.two_a) launch_wgrad3_k<BM, MPW, NT, true>(w, nch, k.lds, stream); else launch_wgrad3_k<BM, MPW, NT, false>(w, nch, k.lds, stream); \
            return true; \
        }
        WGRAD3_INSTANCES(X)
#undef X
    } else if (k.family == 2) {
#define X(MPW, NTMAX) \
        if (k.mpw == MPW && k.nt == NTMAX) { \
            switch (k.bmode) { \
            case 1: launch_wgrad2_k<1, MPW, NTMAX>(w, nch, k.lds, stream); break; \
            case 2: launch_wgrad2_k<2, MPW, NTMAX>(w, nch, k.lds, stream); break; \
            case 3: launch_wgrad2_k<3, MPW, NTMAX>(w, nch, k.lds, stream); break; \
            default: launch_wgrad2_k<0, MPW, NTMAX>(w, nch, k.lds, stream); break; \
            } \
            return true; \
        }
        WGRAD2_TILES(X)
#undef X
    }
    return false;
}

// One contraction record into its `nch` partial slabs: a launch per block of 256 output rows (one, but for n_skipch / n_quantize > 256)
int qpn_launch_wgrad(const Wg2& w, int nch, bool generic, hipStream_t stream) {
    const int nblk = wgrad_n_row_blocks(w);
    for (int i = 0; i < nblk; ++i) {
        const Wg2 blk = wgrad_row_block(w, i);
        if (!launch_pick(blk, wgrad_pick(blk, nch, generic), nch, stream)) {
            qpn_set_error("weight-gradient tiles: unsupported geometry (n_resch <= 128 on this path; wider stacks take the GEMM path)");
            return QPN_EINVAL;
        }
    }
    return QPN_OK;
}
