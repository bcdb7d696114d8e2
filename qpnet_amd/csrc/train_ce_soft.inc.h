// The body of k_ce_distill<NV> and of k_ce_soft_w<NV> (train_fwd.hip), included into both kernels: the text is shared, each kernel is compiled from it directly.
// The including kernel defines  constexpr bool W  (false: the soft-target loss as it always was; true: with the row weights and ignore_index of the loss
// options: w_r multiplies the whole row loss, CE and KL term alike, the row's scale w_r / N is formed once) and  o, a CeOpts (all null with W false, where
// every use of it is discarded).
    __shared__ double part[W ? 3 : 2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float invT = 1.0f / temp, oma = 1.0f - alpha, aT = alpha * temp;
    const float inv = ce_opt_inv<W>(o, rows);
    double csum = 0.0, ksum = 0.0;
    [[maybe_unused]] double msum = 0.0;
    for (int it = 0; it < rpw; ++it) {
        const int64_t row = ((int64_t)blockIdx.x * rpw + it) * 4 + wave;
        if (row >= rows) break;
        const float* lg = logits + (size_t)row * Q;
        const float* tl = teacher + (size_t)row * Q;
        const int64_t b = row / BL, t = row - b * BL;
        int64_t tg = tgt[(size_t)b * tgt_stride + (tgt_stride - BL) + t];
        [[maybe_unused]] float wr = 1.0f;
        if constexpr (W) {          // the row's weight, from the weight and the target alone: a zero-weight row loads no logits
            wr = ce_row_weight(o, row, tg, lane, status);
            if (wr == 0.f) { if (dlogits) ce_zero_row<NV>(dlogits + (size_t)row * Q, Q, lane); continue; }
            msum += (double)wr;
        }
        const float sc = W ? wr * inv : inv;          // the row's scale, formed once
        float ce, kl;
        bool bad = false;
        if constexpr (NV > 0) {
            float4 z[NV], u[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) { z[k] = *(const float4*)(lg + lane * 4 + 256 * k); u[k] = *(const float4*)(tl + lane * 4 + 256 * k); }
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }
            const float ztg = lg[tg];
            float mz = -INFINITY, mt = -INFINITY;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                mz = fmaxf(fmaxf(mz, fmaxf(z[k].x, z[k].y)), fmaxf(z[k].z, z[k].w));
                mt = fmaxf(fmaxf(mt, fmaxf(u[k].x, u[k].y)), fmaxf(u[k].z, u[k].w));
                bad = bad || dk_bad(u[k].x) || dk_bad(u[k].y) || dk_bad(u[k].z) || dk_bad(u[k].w);
            }
            mz = tr_wave_max(mz); mt = tr_wave_max(mt);
            float se = 0.f, sz = 0.f, st = 0.f;
            float4 ez[NV], eu[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                se += (__expf(z[k].x - mz) + __expf(z[k].y - mz)) + (__expf(z[k].z - mz) + __expf(z[k].w - mz));
                ez[k] = make_float4(__expf((z[k].x - mz) * invT), __expf((z[k].y - mz) * invT), __expf((z[k].z - mz) * invT), __expf((z[k].w - mz) * invT));
                eu[k] = make_float4(__expf((u[k].x - mt) * invT), __expf((u[k].y - mt) * invT), __expf((u[k].z - mt) * invT), __expf((u[k].w - mt) * invT));
                sz += (ez[k].x + ez[k].y) + (ez[k].z + ez[k].w);
                st += (eu[k].x + eu[k].y) + (eu[k].z + eu[k].w);
            }
            se = tr_wave_sum(se); sz = tr_wave_sum(sz); st = tr_wave_sum(st);
            const float lse = logf(se) + mz, lsz = logf(sz), lst = logf(st), rz = 1.0f / sz, rt = 1.0f / st;
            float kq = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const float4 pz = make_float4(ez[k].x * rz, ez[k].y * rz, ez[k].z * rz, ez[k].w * rz);
                const float4 pt = make_float4(eu[k].x * rt, eu[k].y * rt, eu[k].z * rt, eu[k].w * rt);
                kq += (pt.x * (((u[k].x - mt) * invT - lst) - ((z[k].x - mz) * invT - lsz)) + pt.y * (((u[k].y - mt) * invT - lst) - ((z[k].y - mz) * invT - lsz))) +
                      (pt.z * (((u[k].z - mt) * invT - lst) - ((z[k].z - mz) * invT - lsz)) + pt.w * (((u[k].w - mt) * invT - lst) - ((z[k].w - mz) * invT - lsz)));
                if (dlogits) {
                    const int q = lane * 4 + 256 * k;
                    float4 g = make_float4(__expf(z[k].x - lse), __expf(z[k].y - lse), __expf(z[k].z - lse), __expf(z[k].w - lse));
                    const int dq = (int)tg - q;
                    if (dq == 0) g.x -= 1.0f; else if (dq == 1) g.y -= 1.0f; else if (dq == 2) g.z -= 1.0f; else if (dq == 3) g.w -= 1.0f;
                    *(float4*)(dlogits + (size_t)row * Q + q) = make_float4((oma * g.x + aT * (pz.x - pt.x)) * sc, (oma * g.y + aT * (pz.y - pt.y)) * sc,
                                                                            (oma * g.z + aT * (pz.z - pt.z)) * sc, (oma * g.w + aT * (pz.w - pt.w)) * sc);
                }
            }
            kl = tr_wave_sum(kq);
            ce = lse - ztg;
        } else {
            if (tg < 0 || tg >= Q) { if (lane == 0) atomicOr(status, 2); tg = tg < 0 ? 0 : Q - 1; }
            const bool vec = (Q & 255) == 0;
            float mz = -INFINITY, mt = -INFINITY;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                mz = fmaxf(fmaxf(mz, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); mt = fmaxf(fmaxf(mt, fmaxf(w.x, w.y)), fmaxf(w.z, w.w));
                bad = bad || dk_bad(w.x) || dk_bad(w.y) || dk_bad(w.z) || dk_bad(w.w);
            } else for (int q = lane; q < Q; q += 64) { const float w = tl[q]; mz = fmaxf(mz, lg[q]); mt = fmaxf(mt, w); bad = bad || dk_bad(w); }
            mz = tr_wave_max(mz); mt = tr_wave_max(mt);
            float se = 0.f, sz = 0.f, st = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                se += (__expf(v.x - mz) + __expf(v.y - mz)) + (__expf(v.z - mz) + __expf(v.w - mz));
                sz += (__expf((v.x - mz) * invT) + __expf((v.y - mz) * invT)) + (__expf((v.z - mz) * invT) + __expf((v.w - mz) * invT));
                st += (__expf((w.x - mt) * invT) + __expf((w.y - mt) * invT)) + (__expf((w.z - mt) * invT) + __expf((w.w - mt) * invT));
            } else for (int q = lane; q < Q; q += 64) { se += expf(lg[q] - mz); sz += expf((lg[q] - mz) * invT); st += expf((tl[q] - mt) * invT); }
            se = tr_wave_sum(se); sz = tr_wave_sum(sz); st = tr_wave_sum(st);
            const float lse = logf(se) + mz, lsz = logf(sz), lst = logf(st), rz = 1.0f / sz, rt = 1.0f / st;
            float kq = 0.f;
            if (vec) for (int q = lane * 4; q < Q; q += 256) {
                const float4 v = *(const float4*)(lg + q), w = *(const float4*)(tl + q);
                const float zv[4] = {v.x, v.y, v.z, v.w}, wv[4] = {w.x, w.y, w.z, w.w};
                float gv[4], kv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = (zv[i] - mz) * invT, c = (wv[i] - mt) * invT;
                    const float pz = __expf(a) * rz, pt = __expf(c) * rt;
                    kv[i] = pt * ((c - lst) - (a - lsz));
                    gv[i] = (oma * (__expf(zv[i] - lse) - (q + i == tg ? 1.0f : 0.0f)) + aT * (pz - pt)) * sc;
                }
                kq += (kv[0] + kv[1]) + (kv[2] + kv[3]);
                if (dlogits) *(float4*)(dlogits + (size_t)row * Q + q) = make_float4(gv[0], gv[1], gv[2], gv[3]);
            } else for (int q = lane; q < Q; q += 64) {
                const float a = (lg[q] - mz) * invT, c = (tl[q] - mt) * invT;
                const float pz = expf(a) * rz, pt = expf(c) * rt;
                kq += pt * ((c - lst) - (a - lsz));
                if (dlogits) dlogits[(size_t)row * Q + q] = (oma * (expf(lg[q] - lse) - (q == tg ? 1.0f : 0.0f)) + aT * (pz - pt)) * sc;
            }
            kl = tr_wave_sum(kq);
            ce = lse - lg[tg];
        }
        if (__any(bad) && lane == 0) atomicOr(status, 32);
        if constexpr (W) { csum += (double)ce * (double)wr; ksum += (double)kl * (double)wr; } else { csum += (double)ce; ksum += (double)kl; }
    }
    if (lane == 0) { part[0][wave] = csum; part[1][wave] = ksum; if constexpr (W) part[2][wave] = msum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double den = ce_opt_den<W>(o, rows);
        const double c = (part[0][0] + part[0][1] + part[0][2] + part[0][3]) / den, k = (part[1][0] + part[1][1] + part[1][2] + part[1][3]) / den;
        atomicAdd(loss + (blockIdx.x & 63), (double)oma * c + (double)alpha * ((double)temp * (double)temp) * k);
        if (comp) { atomicAdd(comp + (blockIdx.x & 63), c); atomicAdd(comp + 64 + (blockIdx.x & 63), k); }
        if constexpr (W) if (o.mass) atomicAdd(o.mass + (blockIdx.x & 63), part[2][0] + part[2][1] + part[2][2] + part[2][3]);
    }
