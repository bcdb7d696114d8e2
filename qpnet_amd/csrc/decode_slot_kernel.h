// decode_slot_kernel.h -- the body of the task-table interpreter, included twice by decode.hip: as k_decode (QPN_KERNEL_ROW false) and as k_decode_r, the kernel of the
// calls with per-row sampling records (QPN_KERNEL_ROW true).  Textual inclusion for the reason given in decode_coopb_kernel.h.
__global__ __launch_bounds__(QPN_NT) void QPN_KERNEL(DecodeParams p) {
    constexpr int ROW = QPN_KERNEL_ROW;      // (false, true, or 2: the kernel of the calls with a draw track -- sample_pick, decode_dev.h)
    constexpr bool WIDE = QPN_KERNEL_WIDE;   // (true: the kernels of the sampled calls at n_quantize > 256 -- sample_pick, decode_dev.h)
    float* sm = SM;
    int* smi = SMI;
    const UttView u = make_view(p, p.utts[blockIdx.x]);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < p.state_floats; i += QPN_NT) sm[i] = 0.0f;
    for (int i = tid; i < p.n_bias; i += QPN_NT) sm[p.o_bias + i] = p.flat[p.bias_src[i]];
    {
        const int* src = (const int*)p.tasks;
        for (int i = tid; i < p.n_slots * QPN_NW * 8; i += QPN_NT) smi[p.o_tasks + i] = src[i];
    }
    if constexpr (ROW) stage_row_draw(p, u.row, one_cu_rowd(p), tid);      // (behind the step state: the barriers below come before the first pick)
    __syncthreads();
    const int64_t Ttot = (int64_t)u.n0 + u.n_samples;
    if (Ttot < 3) return;                                   // nothing to predict
    if (p.cancel) {      // a row that starts after the host's stop request (qpn_decode_cancel) does not run: one lane reads the word, the workgroup leaves together
        if (tid == 0 && cancel_requested(p)) smi[p.o_samp + 2] = 1;
        __syncthreads();
        if (smi[p.o_samp + 2]) return;
    }
    // state for the first step (t = 1): layer-0 input, aux terms; taps of step 2; pd of step 1 is all-zero
    if (wave == 0) {
        causal_rows(p, u, u.known[0], u.known[1], 1, lane);
        if (lane == 0) { smi[p.o_samp] = u.known[0]; smi[p.o_samp + 1] = u.known[1]; }
    }
    stage_aux(p, u, 1, tid, QPN_NT);
    if constexpr (ROW == 2) stage_frame_draw(p, u, 1, one_cu_rowd(p), tid);      // (the first step's frame record; later ones: OP_STAGE, a step ahead)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (Ttot > 3) stage_taps(p, u, 2, tid, QPN_NT, p.status);
    __syncthreads();

    Ctx c; c.p = &p; c.u = &u; c.lane = lane; c.wave = wave; c.Ttot = Ttot; c.creq = 0; c.stop = 0;
    float4 w0[4], w1[4], w2[4];
    {
        const int* tk = smi + p.o_tasks + wave * 8;
        if (tk[0] & TF_HASW) load_tile(w0, p.wpk, tk[1], lane);
        if (tk[QPN_NW * 8] & TF_HASW) load_tile(w1, p.wpk, tk[QPN_NW * 8 + 1], lane);
        if (tk[2 * QPN_NW * 8] & TF_HASW) load_tile(w2, p.wpk, tk[2 * QPN_NW * 8 + 1], lane);
    }
    for (int64_t t = 1; t + 1 < Ttot; ++t) {
        for (int slot = 0; slot < p.n_slots; slot += 3) {
            run_slot<ROW, WIDE>(c, slot, t, w0);
            run_slot<ROW, WIDE>(c, slot + 1, t, w1);
            run_slot<ROW, WIDE>(c, slot + 2, t, w2);
        }
        if (c.stop) break;      // stopped on request at the previous step's publish point (this step has drained: its pick published nothing)
    }
}
