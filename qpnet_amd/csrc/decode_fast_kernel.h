// decode_fast_kernel.h -- the body of the specialised one-CU decode kernel, included twice by decode.hip: as k_decode_fast<...> (QPN_KERNEL_ROW false) and as
// k_decode_fast_r<...>, the kernels of the calls with per-row sampling records (QPN_KERNEL_ROW true).  Textual inclusion for the reason given in decode_coopb_kernel.h.
template <int C, int S, int Q, int NWV, bool RESL>
__global__ __launch_bounds__(NWV * 64) void QPN_KERNEL(DecodeParams p, FastParams f) {
    constexpr int ROW = QPN_KERNEL_ROW;      // (false, true, or 2: the kernel of the calls with a draw track -- sample_pick, decode_dev.h)
    using G = FastGeo<C, S, Q, NWV>;
    static_assert(G::R <= 8 && G::RS <= 32 && G::ZT >= 1 && G::RT >= 1, "geometry not covered by the fast kernel");
    constexpr int NTH = NWV * 64;
    float* sm = SM; int* smi = SMI;
    const UttView u = make_view(p, p.utts[blockIdx.x]);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < p.state_floats; i += NTH) sm[i] = 0.0f;
    for (int i = tid; i < p.n_bias; i += NTH) sm[p.o_bias + i] = p.flat[p.bias_src[i]];
    if constexpr (ROW) stage_row_draw(p, u.row, one_cu_rowd(p), tid);      // (behind the step state: the barriers below come before the first pick)
    __syncthreads();
    const int Ttot = u.n0 + u.n_samples;
    if (Ttot < 3) return;
    if (p.cancel) {      // a row that starts after the host's stop request (qpn_decode_cancel) does not run: one lane reads the word, the workgroup leaves together
        if (tid == 0 && cancel_requested(p)) smi[p.o_samp + 2] = 1;
        __syncthreads();
        if (smi[p.o_samp + 2]) return;
    }
    if (wave == 0) {
        causal_rows(p, u, u.known[0], u.known[1], 1, lane);
        if (lane == 0) { smi[p.o_samp] = u.known[0]; smi[p.o_samp + 1] = u.known[1]; }
    }
    stage_aux(p, u, 1, tid, NTH);
    if constexpr (ROW == 2) stage_frame_draw(p, u, 1, one_cu_rowd(p), tid);      // (the first step's frame record; later ones: beside the pick, a step ahead)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (Ttot > 3) stage_taps(p, u, 2, tid, NTH, p.status);
    __syncthreads();
    if constexpr (RESL) {
        const int per = G::NRES * 256;                                   // float4s per layer
        float4* dst = (float4*)(sm + p.o_wres);
        for (int i = tid; i < (p.L - 1) * per; i += NTH) { const int l = i / per; dst[i] = p.wpk[f.w_res[l] + (i - l * per)]; }
        __syncthreads();
    }
    fast_dispatch<C, S, Q, NWV, RESL, ROW, 0>(p, f, u, wave, lane, tid, Ttot);
}
