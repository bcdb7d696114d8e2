// decode_coop_kernel.h -- the body of the per-utterance cooperative decode kernel, included twice by decode_coop.hip: as k_decode_coop (QPN_KERNEL_ROW false) and as
// k_decode_coop_r, the kernel of the calls with per-row sampling records (QPN_KERNEL_ROW true).  Textual inclusion for the reason given in decode_coopb_kernel.h.
__global__ __launch_bounds__(COOP_NT) void QPN_KERNEL(DecodeParams p, FastParams f, CoopParams c, int b0) {
    constexpr int ROW = QPN_KERNEL_ROW;      // (false, true, or 2: the kernel of the calls with a draw track -- sample_pick, decode_dev.h)
    constexpr bool WIDE = QPN_KERNEL_WIDE;   // (true: the kernels of the sampled calls at n_quantize > 256 -- sample_pick, decode_dev.h)
    float* sm = SM; int* smi = SMI;
    const int gidx = blockIdx.x, b = b0 + blockIdx.y;
    const UttView u = make_view(p, p.utts[b]);
    u64* X = c.xch + (size_t)blockIdx.y * c.utt_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, Cp = p.Cp, S = p.S, Q = p.Q, L = p.L;
    const int CB = c.CB, SB = c.SB, QB = c.QB;
    const int c0 = gidx * CB, s0 = gidx * SB, q0 = gidx * QB;
    const int logR = c.logR, R = 1 << logR, rpt = c.rpt, logRs = c.logRs, Rs = 1 << logRs, rpts = c.rpts;
    // LDS layout (floats)
    int o = 0;
    const int o_xa = o; o += Cp; const int o_xb = o; o += Cp; const int o_xp = o; o += L * Cp; const int o_g = o; o += Cp;
    const int o_y1 = o; o += c.Sp; const int o_y2 = o; o += c.Sp; const int o_lg = o; o += (Q + 3) & ~3;
    const int o_acc = o; o += (2 * SB + 3) & ~3; const int o_aux = o; o += L * 2 * CB; const int o_samp = o; o += 4;
    // the biases my rows add, in LDS: read from global memory where they are used, each sat behind its own wait right after a row's
    // reduction (an exposed L2 round trip per tile pass)
    const int o_bres = o; o += L * CB; const int o_bsk = o; o += L * SB; const int o_bp1 = o; o += SB; const int o_bp2 = o; o += QB;
    const int o_rd = o;       // the row's sampling record (stage_row_draw): behind everything else, in the kernel of the calls with per-row records only
    for (int i = tid; i < o_bres; i += COOP_NT) sm[i] = 0.0f;
    for (int i = tid; i < L * CB; i += COOP_NT) sm[o_bres + i] = p.flat[c.f_resb[i / CB] + c0 + i % CB];
    for (int i = tid; i < L * SB; i += COOP_NT) sm[o_bsk + i] = p.flat[c.f_skipb[i / SB] + s0 + i % SB];
    for (int i = tid; i < SB; i += COOP_NT) sm[o_bp1 + i] = p.flat[c.f_p1b + s0 + i];
    for (int i = tid; i < QB; i += COOP_NT) sm[o_bp2 + i] = p.flat[c.f_p2b + q0 + i];
    __syncthreads();
    const int Ttot = u.n0 + u.n_samples;
    if (Ttot < 3) return;
    if (tid == 0) { smi[o_samp] = u.known[0]; smi[o_samp + 1] = u.known[1]; }
    if constexpr (ROW) stage_row_draw(p, u.row, o_rd, tid);
    // the host's stop request (live_put): the publishing lane's state; a launch that starts after the request raises the abort flag before its
    // first step, and every workgroup leaves at the end of it
    int creq = 0;
    if (tid == 0 && gidx == 0 && cancel_requested(p)) { creq = -1; __hip_atomic_store(c.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __syncthreads();
    const int q = lane & (R - 1), grp = lane >> logR, qs = lane & (Rs - 1), grps = lane >> logRs;
    const int n_aux = L * 2 * CB;
    for (int t = 1; t + 1 < Ttot; ++t) {
        const unsigned tag = (unsigned)t + 1u;
        // ---------------- A. this step's layer-0 input (two rows of the causal table, qpnet.py:110-132), aux terms, past rows
        {
            const int s_prev = smi[o_samp], s_cur = smi[o_samp + 1];
            const RingDesc r0 = p.rings[0];
            for (int ch = tid; ch < C; ch += COOP_NT) {
                float v = p.flat[p.causal_w + ((size_t)ch * Q + s_prev) * 2] + p.flat[p.causal_w + ((size_t)ch * Q + s_cur) * 2 + 1];
                v = v + p.flat[p.causal_b + ch];
                sm[o_xa + ch] = v;
                if (ch >= c0 && ch < c0 + CB) gr_store(X + c.o_ring[0] + (size_t)((unsigned)t % (unsigned)r0.len) * C + ch, tag, v);
            }
            const int ut = aux_time(u, t);
            int fr, j;
            if (ut < 0) { fr = 0; j = 0; }
            else if (p.U > 0) { fr = (int)((unsigned)ut / (unsigned)p.U); j = ut - fr * p.U; }
            else { fr = ut; j = 0; }
            const float wj = p.U > 0 ? p.flat[p.up_w + j] : 1.0f;
            const float* pf = u.pproj + (size_t)fr * L * 2 * C;
            if constexpr (ROW == 2) stage_frame_draw(p, u, t, o_rd, tid);      // draw track: this step's frame record, beside its aux terms
            for (int i = tid; i < n_aux; i += COOP_NT) {
                const int l = i / (2 * CB), r = i - l * 2 * CB, half = r / CB, nat = half * C + c0 + (r - half * CB);
                sm[o_aux + i] = __builtin_fmaf(wj, pf[l * 2 * C + nat], p.qb[l * 2 * C + nat]);
            }
            const int widx = t < u.n0 - 1 ? t - (u.n0 - 1) : 0;
            for (int i = tid; i < L * C; i += COOP_NT) {
                const int l = i / C, ch = i - l * C;
                const RingDesc r = p.rings[l];
                int off = tap_offset(r, u, ut, widx);
                if (off < 1 || off >= r.len) { if (ch == 0) atomicOr(p.status, 1); off = off < 1 ? 1 : r.len - 1; }
                const int tp = t - off;                   // a row of an earlier step (slot tp carries tag tp + 1)
                float v = 0.0f;                           // time 0 and before: never written, zeros
                if (tp >= 1) {
                    const u64* src = X + c.o_ring[l] + (size_t)((unsigned)tp % (unsigned)r.len) * C + ch;
                    u64 gv = gr_load(src);
                    unsigned spins = 0;
                    while ((unsigned)(gv >> 32) != (unsigned)tp + 1u && ++spins < 4096u) gv = gr_load(src);     // published a whole step ago: normally no spin
                    if (spins >= 4096u) { __hip_atomic_store(c.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicOr(p.status, 4); }
                    v = __uint_as_float((unsigned)gv);
                }
                sm[o_xp + l * Cp + ch] = v;
            }
            for (int i = tid; i < 2 * SB; i += COOP_NT) sm[o_acc + i] = 0.0f;
        }
        __syncthreads();
        int xin = o_xa, xnext = o_xb;
        const int npair = (2 * CB) / rpt, zt0 = (2 * c0) / rpt;
        // the tiles of a phase's FIRST pass are requested before the wait that precedes the phase (they do not depend on it)
        float4 wcN[4], wqN[4], wrN[4];
        if (wave < npair) { load_tile(wcN, p.wpk, f.w_cur[0] + (zt0 + wave) * 256, lane); load_tile(wqN, p.wpk, c.w_past_il[0] + (zt0 + wave) * 256, lane); }
        for (int l = 0; l < L; ++l) {
            // ---------------- Z: pre-activations of my channels (current + past tap + aux), gate
            for (int i = wave; i < npair; i += COOP_NW) {
                const int ti = zt0 + i;
                float4 x[4], xp[4];
                if (i != wave) {                              // (the first pass's tiles were requested before the wait)
                    load_tile(wcN, p.wpk, f.w_cur[l] + ti * 256, lane);
                    load_tile(wqN, p.wpk, c.w_past_il[l] + ti * 256, lane);
                }
                const float4* xv = (const float4*)(sm + xin + 16 * q);
                const float4* pv = (const float4*)(sm + o_xp + l * Cp + 16 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = xv[k]; xp[k] = pv[k]; }
                const float ac = tree_reduce(chunk16(wcN, x), logR);
                const float ap = tree_reduce(chunk16(wqN, xp), logR);
                const int row = ti * rpt + grp, ch = row >> 1, half = row & 1;
                const float z = (ac + ap) + sm[o_aux + l * 2 * CB + half * CB + (ch - c0)];
                float zo;                                     // the tanh row of the same channel (R lanes up)
                if (R == 32) { const int zi = __float_as_int(z); const auto sw = __builtin_amdgcn_permlane32_swap(zi, zi, false, false); zo = __int_as_float((int)sw[1]); }
                else zo = __shfl_down(z, R);
                if (q == 0 && !half) gr_store(X + c.o_g + (size_t)l * C + ch, tag, qgate(z, zo));
            }
            const bool has_res = l + 1 < L;               // the last block's residual output is unused (qpnet.py:505)
            // (a slice smaller than a 4 KiB tile -- G = 128 / 256 at C = 512: one or two skip / post-net rows per workgroup -- takes the tile that holds its rows
            //  and keeps the lane groups of those rows)
            const int nres = has_res ? CB / rpt : 0, nsk = (SB + rpt - 1) / rpt;
            if (wave < nres + nsk)
                load_tile(wrN, p.wpk, wave < nres ? f.w_res[l] + (c0 / rpt + wave) * 256 : f.w_skip[l] + (s0 / rpt + (wave - nres)) * 256, lane);
            gather_vec(X + c.o_g + (size_t)l * C, C, tag, sm + o_g, tid, c.abort, p.status);
            __syncthreads();
            // ---------------- R: residual 1x1 rows of my channels (-> next layer's input), skip 1x1 rows of my slice
            {
                float4 xg[4];
                const float4* gv = (const float4*)(sm + o_g + 16 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) xg[k] = gv[k];
                for (int i = wave; i < nres + nsk; i += COOP_NW) {
                    if (i != wave) load_tile(wrN, p.wpk, i < nres ? f.w_res[l] + (c0 / rpt + i) * 256 : f.w_skip[l] + (s0 / rpt + (i - nres)) * 256, lane);
                    const float acc = tree_reduce(chunk16(wrN, xg), logR);
                    if (i < nres) {
                        const int row = (c0 / rpt + i) * rpt + grp;
                        if (q == 0) {
                            const float v = (acc + sm[o_bres + l * CB + (row - c0)]) + sm[xin + row];
                            const RingDesc rn = p.rings[l + 1];
                            gr_store(X + c.o_ring[l + 1] + (size_t)((unsigned)t % (unsigned)rn.len) * C + row, tag, v);
                        }
                    } else {
                        const int row = (s0 / rpt + (i - nres)) * rpt + grp;
                        if (q == 0 && row >= s0 && row < s0 + SB) {
                            const int a = o_acc + (f.adaptive[l] ? SB : 0) + (row - s0);
                            sm[a] = sm[a] + (acc + sm[o_bsk + l * SB + (row - s0)]);
                        }
                    }
                }
                if (has_res) {
                    if (wave < npair) { load_tile(wcN, p.wpk, f.w_cur[l + 1] + (zt0 + wave) * 256, lane); load_tile(wqN, p.wpk, c.w_past_il[l + 1] + (zt0 + wave) * 256, lane); }
                    const RingDesc rn = p.rings[l + 1];
                    gather_vec(X + c.o_ring[l + 1] + (size_t)((unsigned)t % (unsigned)rn.len) * C, C, tag, sm + xnext, tid, c.abort, p.status);
                }
            }
            __syncthreads();
            const int tmp = xin; xin = xnext; xnext = tmp;
        }
        // ---------------- tail: relu(skip total) -> post 1x1 #1 -> relu -> post 1x1 #2 (qpnet.py:566-571)
        for (int r = tid; r < SB; r += COOP_NT) {
            const float tot = sm[o_acc + r] + sm[o_acc + SB + r];     // sum(skip_F) + sum(skip_A)  (qpnet.py:505)
            gr_store(X + c.o_y1 + s0 + r, tag, tot > 0.0f ? tot : 0.0f);
        }
        const int np1 = (SB + rpts - 1) / rpts, np2 = (QB + rpts - 1) / rpts;
        if (wave < np1) load_tile(wrN, p.wpk, f.w_p1 + (s0 / rpts + wave) * 256, lane);
        gather_vec(X + c.o_y1, S, tag, sm + o_y1, tid, c.abort, p.status);
        __syncthreads();
        {
            float4 xq[4];
            const float4* yv = (const float4*)(sm + o_y1 + 16 * qs);
#pragma unroll
            for (int k = 0; k < 4; ++k) xq[k] = yv[k];
            for (int i = wave; i < np1; i += COOP_NW) {
                const int ti = s0 / rpts + i;
                if (i != wave) load_tile(wrN, p.wpk, f.w_p1 + ti * 256, lane);
                const float acc = tree_reduce(chunk16(wrN, xq), logRs);
                const int row = ti * rpts + grps;
                if (qs == 0 && row >= s0 && row < s0 + SB) { const float v = acc + sm[o_bp1 + (row - s0)]; gr_store(X + c.o_y2 + row, tag, v > 0.0f ? v : 0.0f); }
            }
        }
        if (wave < np2) load_tile(wrN, p.wpk, f.w_p2 + (q0 / rpts + wave) * 256, lane);
        gather_vec(X + c.o_y2, S, tag, sm + o_y2, tid, c.abort, p.status);
        __syncthreads();
        {
            float4 xq[4];
            const float4* yv = (const float4*)(sm + o_y2 + 16 * qs);
#pragma unroll
            for (int k = 0; k < 4; ++k) xq[k] = yv[k];
            for (int i = wave; i < np2; i += COOP_NW) {
                const int ti = q0 / rpts + i;
                if (i != wave) load_tile(wrN, p.wpk, f.w_p2 + ti * 256, lane);
                const float acc = tree_reduce(chunk16(wrN, xq), logRs);
                const int row = ti * rpts + grps;
                if (qs == 0 && row >= q0 && row < q0 + QB) gr_store(X + c.o_lg + row, tag, acc + sm[o_bp2 + (row - q0)]);
            }
        }
        gather_vec(X + c.o_lg, Q, tag, sm + o_lg, tid, c.abort, p.status);
        __syncthreads();
        // ---------------- pick: every workgroup holds all logits and derives the same next sample
        if (wave == 0) {
            float bv = -INFINITY; int bi = 0x7fffffff;
            for (int i = lane; i < Q; i += 64) { const float v = sm[o_lg + i]; if (v > bv) { bv = v; bi = i; } }
            bi = wave_argmax(bv, bi);
            const int i = t - (u.n0 - 1);
            if (i >= 0 && u.logits && gidx == 0) for (int k = lane; k < Q; k += 64) u.logits[(size_t)i * Q + k] = sm[o_lg + k];
            int next;
            if (i >= 0) {
                if (p.mode != QPN_MODE_ARGMAX) bi = sample_pick<ROW, WIDE>(p, (unsigned)u.row, o_rd, o_lg, Q, (unsigned)i, lane);
                next = bi;
                if (u.teacher) { const int64_t sv = u.teacher[i] % Q; next = (int)(sv < 0 ? sv + Q : sv); }
                if (lane == 0 && gidx == 0) {
                    u.out[i] = bi;
                    if (live_put(p, u, i, bi, creq, c.abort)) __hip_atomic_store(c.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // stop on request: drain like a launch that gave up
                }
            } else next = u.known[t + 1];
            if (lane == 0) {
                smi[o_samp] = smi[o_samp + 1]; smi[o_samp + 1] = next;
                smi[o_samp + 2] = __hip_atomic_load(c.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (smi[o_samp + 2]) break;            // a peer gave up: leave together (the flag was read once, by one lane)
    }
}
