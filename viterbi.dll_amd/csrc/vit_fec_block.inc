// vit_fec_block.inc -- the body of the FEC kernels, included inside each of them: RS(204,188) over a workgroup's up to 20
// FEC frames of one stream.  The including kernel has in scope `in`, `out` (the stream, and where it goes: in itself for
// in place), `nslots`, `phase`, `nfec` (long long: whole frames from `phase` on), `rec` (u32*: the stream's FEC records)
// and the macro FEC_BLOCK, the workgroup's index among those on this stream: its frames are 20 * FEC_BLOCK ... (none
// behind nfec).  In place a workgroup whose rows are all clean writes nothing.  Out of place every frame is written, and
// workgroup 0 copies the slots in front of the first frame and behind the last.  It is a text and not a __device__
// routine because vit_fec_kernel did not keep its speed as one (profiles/r25_packets_ab.json): the inliner simplifies a
// routine before it inlines it, and the correction path came out 2.4 % slower.
    __shared__ __attribute__((aligned(16))) uint8_t s_img[FEC_IMG];
    __shared__ __attribute__((aligned(16))) u32 s_nib[2 * 16 * 4];
    __shared__ uint8_t s_ato[ATO_SIZE], s_iof[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_rec[FEC_FPB * 16u];
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (WAVE - 1u), wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid / WAVE));
    if (tid < 2u * 16u * 4u) s_nib[tid] = c_fec_nib.w[tid];
    for (u32 k = tid; k < (u32)ATO_SIZE; k += TPB) s_ato[k] = g_gf.ato[k];
    s_iof[tid] = g_gf.iof[tid];
    const uint8_t* ato = s_ato;
    const uint8_t* iof = s_iof;
    const bool inplace = in == out;

    const long long F0 = (long long)FEC_BLOCK * FEC_FPB;
    const u32 nF = F0 < nfec ? (u32)(nfec - F0 < (long long)FEC_FPB ? nfec - F0 : (long long)FEC_FPB) : 0u;
    const u64 off = (u64)SLOT * ((u64)phase + (u64)FEC_SLOTS * (u64)F0);  // the workgroup's first byte
    const u32 n = nF * FEC_FRAME_BYTES;
    const u32 a = (u32)(reinterpret_cast<uintptr_t>(in + off) & 15u);
    if (nF) load_image(in + off, n, s_img, tid, TPB);
    if (!inplace && FEC_BLOCK == 0) {
        const u64 end = (u64)SLOT * (u64)nslots;
        const u64 head = nfec > 0 ? (u64)SLOT * phase : end;  // without a whole frame: everything
        const u64 tail = nfec > 0 ? (u64)SLOT * ((u64)phase + (u64)FEC_SLOTS * (u64)nfec) : end;
        for (u64 k = tid; k < head; k += TPB) out[k] = in[k];
        for (u64 k = tail + tid; k < end; k += TPB) out[k] = in[k];
    }
    __syncthreads();

    const u32 fl = wave * FEC_FPW + lane / ROWS, row = lane % ROWS;
    const bool active = lane < FEC_FPW * ROWS && fl < nF;
    const u32 fb = a + (active ? fl : 0u) * FEC_FRAME_BYTES;  // the frame in the image (idle lanes walk frame 0, to no effect)
    // remainder mod g(x): coefficient j = byte j of (r0, r1, r2, r3)
    u32 r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    const u32 nibbase = (u32)(uintptr_t)(const LDS u32*)s_nib;  // LDS byte address
    {
        const uint8_t* q = s_img + fb + row;
        auto step = [&](u32 d) {
            const u32 f = r3 >> 24;
            const u32x4 lo = *reinterpret_cast<const LDS u32x4*>(nibbase + ((f << 4) & 0xF0u));
            const u32x4 hi = *reinterpret_cast<const LDS u32x4*>(nibbase + 256u + (f & 0xF0u));
            r3 = xor3(__builtin_amdgcn_alignbit(r3, r2, 24), lo.w, hi.w);
            r2 = xor3(__builtin_amdgcn_alignbit(r2, r1, 24), lo.z, hi.z);
            r1 = xor3(__builtin_amdgcn_alignbit(r1, r0, 24), lo.y, hi.y);
            r0 = xor3((r0 << 8) | d, lo.x, hi.x);
        };
#pragma unroll 4
        for (u32 c = 0; c < COLS; c++) step(q[ROWS * c]);
#pragma unroll
        for (u32 j = 0; j < NPAR; j++) step(s_img[fb + fec_byte(row, COLS + j)]);
    }
    const bool err = active && (r0 | r1 | r2 | r3) != 0;
    int nerr = 0;
    bool changed = false;
    if (__any(err)) {
        u32 L = 0;
        bool bad = true;
        u32 lz[TCORR + 1], oz[TCORR];  // locator and evaluator in index form, a zero coefficient as ATO_ZERO
#pragma unroll
        for (u32 k = 0; k <= TCORR; k++) lz[k] = ATO_ZERO;
#pragma unroll
        for (u32 k = 0; k < TCORR; k++) oz[k] = ATO_ZERO;
        if (err) {
            // syndromes S_i = rem(alpha^i) in index form (255: zero)
            u32 slog[NPAR];
            {
                u32 lg[NPAR], s0 = 0;
#pragma unroll
                for (u32 j = 0; j < NPAR; j++) {
                    const u32 c = ((j < 4u ? r0 : j < 8u ? r1 : j < 12u ? r2 : r3) >> (8u * (j & 3u))) & 0xFFu;
                    s0 ^= c;
                    lg[j] = c ? (u32)iof[c] : (u32)ATO_ZERO;
                }
                slog[0] = iof[s0];
#pragma unroll
                for (u32 i = 1; i < NPAR; i++) {
                    u32 v = 0;
#pragma unroll
                    for (u32 j = 0; j < NPAR; j++) v ^= ato[lg[j] + i * j];  // <= 512 + 225
                    slog[i] = iof[v];
                }
            }
            // Berlekamp-Massey; polynomials cut at degree 8: a term above it means L > 8, which fails anyway
            u32 lam[TCORR + 1], llog[TCORR + 1], blog[TCORR + 1];
#pragma unroll
            for (u32 k = 0; k <= TCORR; k++) {
                lam[k] = k ? 0u : 1u;
                llog[k] = blog[k] = k ? (u32)NN : 0u;
            }
#pragma unroll
            for (u32 r = 1; r <= NPAR; r++) {
                u32 dsc = 0;
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++)
                    if (k < r && llog[k] != (u32)NN && slog[r - 1u - k] != (u32)NN) dsc ^= ato[llog[k] + slog[r - 1u - k]];
                const bool grow = dsc != 0 && 2u * L <= r - 1u;
                u32 nb[TCORR + 1];
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++) {
                    const u32 shifted = k ? blog[k - 1u] : (u32)NN;
                    nb[k] = grow ? (llog[k] == (u32)NN ? (u32)NN : mod510(llog[k] + NN - iof[dsc])) : shifted;
                }
                if (dsc) {
                    const u32 dl = iof[dsc];
#pragma unroll
                    for (u32 k = 1; k <= TCORR; k++) {
                        if (blog[k - 1u] != (u32)NN) lam[k] ^= ato[dl + blog[k - 1u]];
                        llog[k] = iof[lam[k]];
                    }
                }
                if (grow) L = r - L;
#pragma unroll
                for (u32 k = 0; k <= TCORR; k++) blog[k] = nb[k];
            }
            u32 deg = 0;
#pragma unroll
            for (u32 k = 1; k <= TCORR; k++)
                if (llog[k] != (u32)NN) deg = k;
            bad = L > TCORR || deg != L;
#pragma unroll
            for (u32 k = 0; k <= TCORR; k++) lz[k] = llog[k] == (u32)NN ? (u32)ATO_ZERO : llog[k];
            // evaluator Omega = S * Lambda mod x^16; only its terms below degree L are used
#pragma unroll
            for (u32 k = 0; k < TCORR; k++) {
                u32 v = 0;
#pragma unroll
                for (u32 j = 0; j <= k; j++)
                    if (llog[j] != (u32)NN && slog[k - j] != (u32)NN) v ^= ato[llog[j] + slog[k - j]];
                oz[k] = v ? (u32)iof[v] : (u32)ATO_ZERO;
            }
            nerr = -1;
        }
        // one row at a time, the whole wavefront on it
        u64 work = __ballot(err && !bad);
        while (work) {
            const int owner = __builtin_ctzll(work);
            work &= work - 1;
            const u32 Lo = (u32)__builtin_amdgcn_readlane((int)L, owner);
            const u32 ofb = (u32)__builtin_amdgcn_readlane((int)fb, owner), orow = (u32)__builtin_amdgcn_readlane((int)row, owner);
            u32 lo_[TCORR + 1];
#pragma unroll
            for (u32 j = 1; j <= TCORR; j++) lo_[j] = (u32)__builtin_amdgcn_readlane((int)lz[j], owner);
            u32 z = 0, cnt = 0;
#pragma unroll
            for (u32 qd = 0; qd < 4u; qd++) {
                const u32 d = lane + WAVE * qd;  // the position whose coefficient has degree d: X = alpha^d
                u32 v = 1;
#pragma unroll
                for (u32 j = 1; j <= TCORR; j++)
                    if (j <= Lo) v ^= ato[lo_[j] + NN - mod255(j * d)];  // lambda_j * X^-j
                const bool hit = d < NCODE && v == 0;
                cnt += (u32)__popcll(__ballot(hit));
                z |= hit ? 1u << qd : 0u;
            }
            if (cnt == Lo) {  // Lo distinct roots, all at real positions
                u32 oo[TCORR];
#pragma unroll
                for (u32 k = 0; k < TCORR; k++) oo[k] = (u32)__builtin_amdgcn_readlane((int)oz[k], owner);
#pragma unroll
                for (u32 qd = 0; qd < 4u; qd++) {
                    if (!((z >> qd) & 1u)) continue;
                    const u32 d = lane + WAVE * qd;
                    u32 num = 0, den = 0;  // Omega(1/X) and Lambda'(1/X); the value is X * num / den
#pragma unroll
                    for (u32 k = 0; k < TCORR; k++)
                        if (k < Lo) num ^= ato[oo[k] + NN - mod255(k * d)];
#pragma unroll
                    for (u32 j = 1; j <= TCORR; j += 2)
                        if (j <= Lo) den ^= ato[lo_[j] + NN - mod255((j - 1u) * d)];
                    if (num && den) s_img[ofb + fec_byte(orow, NCODE - 1u - d)] ^= ato[mod255(d + iof[num] + NN - iof[den])];
                }
                if (lane == (u32)owner) nerr = (int)Lo;
                changed = true;
            }
        }
    }
    if (active) s_rec[fl * 16u + row] = (uint8_t)nerr;
    const bool write = __syncthreads_or(changed) || !inplace;  // (the barrier also orders the patches and s_rec)
    if (tid < nF * 4u) {
        const u32 f = tid >> 2, w = tid & 3u;
        const u32* nr = reinterpret_cast<const u32*>(s_rec + f * 16u);
        u32 v;
        if (w < 3u) {
            v = nr[w];
        } else {
            const uint8_t* h = s_img + a + f * FEC_FRAME_BYTES + FEC_DATA_BYTES;
            u32 ok = 0;
            for (u32 c = 0; c < FEC_PACKETS; c++)
                if (h[SLOT * c] == fec_hdr0(c) && h[SLOT * c + 1u] == FEC_HDR1) ok |= 1u << c;
            v = ok | (((nr[0] | nr[1] | nr[2]) & 0x80808080u) ? 1u << 16 : 0u);
        }
        rec[4u * (u64)(F0 + f) + w] = v;
    }
    if (write && nF) {
        uint8_t* dst = out + off;
        if (((u32)(reinterpret_cast<uintptr_t>(dst)) & 15u) == a) {
            const u32 nwin = (a + n + 15u) >> 4;
            for (u32 w = tid; w < nwin; w += TPB) {
                const int o = (int)(16u * w) - (int)a;
                if (o >= 0 && (u32)o + 16u <= n) {
                    *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(s_img + 16u * w);
                } else {
                    for (u32 j = 0; j < 16u; j++) {
                        const int k = o + (int)j;
                        if (k >= 0 && (u32)k < n) dst[k] = s_img[16u * w + j];
                    }
                }
            }
        } else {  // d_out at another phase in 16 bytes than d_stream
            for (u32 k = tid; k < n; k += TPB) dst[k] = s_img[a + k];
        }
    }
