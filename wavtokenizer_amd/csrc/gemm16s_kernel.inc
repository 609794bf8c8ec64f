// gemm16s_kernel (G16_MIX 0), gemm16s_mixed_kernel (G16_MIX 1) and gemm16h_kernel (G16_HI 1): included three times by gemm16s.hip
// with G16_NAME, G16_PARAMS, G16_MIX and G16_HI set.  With G16_MIX 0 and G16_HI 0 the preprocessed text is exactly the kernel of the
// plans of one length.  G16_MIX 1 is the
// mixed-length form (WT_PLAN_FLAG_MIXED_LENGTH): its second argument is clip 0's {T_in, Tp, T_out} triple of this conv in the
// geometry table (clip stride GEOM_WORDS), which the gather reads per clip; p.T_in / T_out / Tp are then the padded extents.
// G16_HI 1 is the one-product twin (WT_PLAN_FLAG_F16_GEMM): the hi halves of both operands only, hi.hi into the main
// accumulator - no correction accumulators, no lo fragment reads, a third of the MFMAs.  The DMA still moves whole 128-byte
// groups, so the LDS image, the swizzle, the tile walk, the K order and every epilogue are the same text.
template <int BM, int BN, int WAVES_M, int WAVES_N, int NSTAGE, int EPI, int OUT, int DBG = 0, int MF = WT_GEMM16S_MF, int WPS = 2, int KS = 1,
          int PROD = 0>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N * (1 + PROD), WPS) void G16_NAME(const GemmArgs p G16_PARAMS) {
    constexpr int dbg = DBG;
    static_assert(KS == 1 || (KS == 2 && NSTAGE == 6 && MF == 1 && DBG == 0), "two K tiles per barrier: 6 stages (three pairs), 16x16x32 MFMA, no experiment masks");
    static_assert(!PROD || KS == 2, "loader waves: the two-tiles-per-barrier form only");
    constexpr int NW = WAVES_M * WAVES_N, NT = 64 * NW * (1 + PROD);        // NW: MFMA waves
    constexpr int NL = PROD ? NW * PROD : NW;                               // waves that issue the DMA pieces
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int STG = (BM + BN) * 128;                   // bytes per stage
    constexpr int NPA = BM / 8 / NL, NPB = BN / 8 / NL;    // DMA pieces (8 rows x 128 B) per loading wave and K step
    constexpr int NPT = NPA + NPB;
    static_assert(BM % (8 * NL) == 0 && BN % (8 * NL) == 0, "pieces must divide evenly among the loading waves");
    static_assert(WM % 32 == 0 && WN % 32 == 0 && BM % 16 == 0, "32x32 MFMA tiles");
    static_assert((NSTAGE - 2) * NPT < 64, "vmcnt field");
    extern __shared__ __attribute__((aligned(1024))) char smem_s[];

    // the wave index as a SCALAR: with threadIdx.x >> 6 in a vector register every LDS-DMA destination (M0) went through
    // v_add + v_readfirstlane + s_mov per piece, and every per-wave offset cost vector instructions
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_all = (dbg & 65536) ? (tid >> 6) : __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader_wave = PROD && wave_all >= NW;          // (scalar)
    const bool mfma_wave = !loader_wave;
    const bool dma_wave = !PROD || loader_wave;
    const int wave = loader_wave ? wave_all - NW : wave_all;  // index within the role: a loader wave issues the pieces of its twin
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int ntiles = tiles_m * tiles_n;
    const int G = gridDim.x;                 // persistent: this workgroup owns tiles blockIdx.x, + G, + 2G, ...
    if (p.stamp_start && tid == 0)           // timing hook: earliest entry of any workgroup (constant 100 MHz clock)
        __hip_atomic_fetch_min(p.stamp_start, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int z = blockIdx.z;
    const int nclips = p.M / p.T_out;
    constexpr unsigned OOB = 0x80000000u;

    // virtual block -> (row tile, column tile): XCD-contiguous, then grouped GM row tiles at a time (gemm.hip)
    auto tile_coords = [&](int vb, int& bm, int& bn) {
        int tile = xcd_remap_s(vb, ntiles);
        // column blocks of group_n tiles (the last one may be narrower), inside a block groups of group_m row tiles
        const int GN = p.group_n > 0 && p.group_n < tiles_n ? p.group_n : tiles_n;
        const int blk_full = tiles_m * GN, nfull = tiles_n / GN;
        int nblk = tile / blk_full, gn = GN;
        if (nblk >= nfull) { nblk = nfull; gn = tiles_n - nfull * GN; }
        tile -= nblk * blk_full;
        const int per_group = p.group_m * gn;
        const int grp = tile / per_group;
        const int first_m = grp * p.group_m;
        const int gsz = tiles_m - first_m < p.group_m ? tiles_m - first_m : p.group_m;
        const int in_grp = tile - grp * per_group;
        bm = first_m + in_grp % gsz;
        bn = nblk * GN + in_grp / gsz;
    };
    auto first_clip = [&](int bm) { return (bm * BM < p.M ? bm * BM : p.M - 1) / p.T_out; };

    // S32 arrays are addressed in bytes = 4 x the fp32 element offset
    const char* Ag = reinterpret_cast<const char*>(p.A) + (long)z * p.zA * 4;
    const char* Ag2 = reinterpret_cast<const char*>(p.A2);          // second K source (nz = 1: host)
    const char* Wg = reinterpret_cast<const char*>(p.W_hi) + (long)z * p.zW * 4;
    const long w_span = (long)p.N * p.w_rstride * 4;
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(Wg), 0, (int)(w_span < 0x7fffffffL ? w_span : 0x7fffffffL), 0x00020000);

    // bias / gamma cache (see the persistent loop): the vectors of the epilogues that store between their loads
    constexpr bool PCACHE = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_ELU || EPI == EPI_BIAS_RES ||
                            EPI == EPI_BIAS_RES_ELU || EPI == EPI_BIAS_GAMMA_RES || EPI == EPI_HEAD;
    constexpr int PC_BYTES = WN * 4 * (EPI == EPI_BIAS_GAMMA_RES ? 2 : 1);
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.bias ? p.bias : p.C), 0, p.bias ? p.N * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsGamma = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.gamma ? p.gamma : p.C), 0, p.gamma ? p.N * 4 : 0, 0x00020000);
    const char* pcw = smem_s + p.pc_off + wave * PC_BYTES;

    // two [taps][BM] tables of per-(tap, row) byte offsets: the tile being loaded and the one after it
    unsigned* s_rowoff = reinterpret_cast<unsigned*>(smem_s + NSTAGE * STG);
    const int tab_sz = p.taps * BM;
    auto build_table = [&](int vb, int par) {
        if (vb >= ntiles) return;
        int bm, bn;
        tile_coords(vb, bm, bn);
        const int clip0 = first_clip(bm);
        unsigned* tab = s_rowoff + par * tab_sz;
        for (int e = tid; e < tab_sz; e += NT) {
            const int tp = e / BM, r = e - tp * BM;
            const int m = bm * BM + r;
            unsigned off = OOB;
            if (m < p.M) {
                const int b = m / p.T_out;
                const int t = m - b * p.T_out;
                const int tap = p.tap_pair ? (tp >> 1) + (tp & 1) * p.stride : tp;
                int pos = t * p.stride - p.pad_left + tap * p.dil;
#if G16_MIX
                bool ok;
                // this clip's {T_in, Tp, T_out} (reflect padding only: host); its rows past T_out gather nothing, A2 included
                const int* g = mix_geom + (long)b * GEOM_WORDS;
                const int t_in = g[0], tp_c = g[1], t_out = g[2];
                pos = pos < 0 ? -pos : pos;
                pos = pos >= tp_c ? 2 * (tp_c - 1) - pos : pos;
                ok = t < t_out && pos < t_in;
                if (ok) off = (unsigned)(((long)(b - clip0) * p.a_bstride + (long)pos * p.a_rstride) * 4);
                if (p.A2) s_rowoff[2 * tab_sz + par * BM + r] = t < t_out ?
                    (unsigned)(((long)(b - clip0) * p.a2_bstride + (long)t * p.a2_rstride) * 4) : OOB;
#else
                bool ok;
                if (p.pad_mode == PAD_REFLECT) {
                    pos = pos < 0 ? -pos : pos;
                    pos = pos >= p.Tp ? 2 * (p.Tp - 1) - pos : pos;
                    ok = pos < p.T_in;
                } else {
                    ok = (pos >= 0) && (pos < p.T_in);
                }
                if (ok) off = (unsigned)(((long)(b - clip0) * p.a_bstride + (long)pos * p.a_rstride) * 4);
                // second source (taps = 1, stride 1, no padding: pos = t)
                if (p.A2) s_rowoff[2 * tab_sz + par * BM + r] = (unsigned)(((long)(b - clip0) * p.a2_bstride + (long)t * p.a2_rstride) * 4);
#endif
            } else if (p.A2) {
                s_rowoff[2 * tab_sz + par * BM + r] = OOB;
            }
            tab[e] = off;
        }
    };

    // ---- loader: a continuous stream of K tiles that runs NSTAGE-1 steps ahead of the MFMAs and crosses from one
    // output tile into the next without a seam.  DMA piece q = 8 image rows; lane -> (row q*8 + lane/8, physical
    // chunk lane%8); the logical chunk it must fetch is physical ^ ((row >> 1) & 7)
    const int prow = lane >> 3;
    int a_row[NPA];
    unsigned a_chunk[NPA], w_chunk[NPB];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int q = wave + NL * i;
        a_row[i] = q * 8 + prow;
        a_chunk[i] = (unsigned)(((lane & 7) ^ (((q & 1) << 2) | (lane >> 4))) * 16);
    }
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        const int q = BM / 8 + wave + NL * j;
        w_chunk[j] = (unsigned)(((lane & 7) ^ (((q & 1) << 2) | (lane >> 4))) * 16);
    }
    unsigned a_voff[NPA], a2_voff[NPA], w_voff[NPB];
    __amdgpu_buffer_rsrc_t rsA, rsA2;
    int l_vb = blockIdx.x, l_par = 0, tapL = 0, ciL = 0, kL = 0;
    unsigned l_mask = 0;
    auto set_tap = [&](int tap) {
        const unsigned* tab = s_rowoff + l_par * tab_sz;
#pragma unroll
        for (int i = 0; i < NPA; ++i) a_voff[i] = tab[tap * BM + a_row[i]] + a_chunk[i];
    };
    auto loader_set_tile = [&](int vb, int par) {       // the table of `vb` (parity par) must be visible
        l_vb = vb; l_par = par; tapL = 0; ciL = 0; kL = 0;
        if (dbg & 131072) l_mask = OOB;          // timing experiment: every DMA is issued but fetches nothing (zero fill)
        if (vb >= ntiles) { l_mask = OOB; return; }
        int bm, bn;
        tile_coords(vb, bm, bn);
        const int clip0 = first_clip(bm);
        const char* Ablk = Ag + (long)clip0 * p.a_bstride * 4;
        const long a_span = ((long)(nclips - clip0 - 1) * p.a_bstride + (long)p.T_in * p.a_rstride) * 4;
        rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Ablk), 0,
                                                (int)(a_span < 0x7fffffffL ? a_span : 0x7fffffffL), 0x00020000);
        if (p.A2) {
            const long a2_span = ((long)(nclips - clip0 - 1) * p.a2_bstride + (long)p.T_in * p.a2_rstride) * 4;
            rsA2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Ag2 + (long)clip0 * p.a2_bstride * 4), 0,
                                                     (int)(a2_span < 0x7fffffffL ? a2_span : 0x7fffffffL), 0x00020000);
            const unsigned* tab2 = s_rowoff + 2 * tab_sz + par * BM;
#pragma unroll
            for (int i = 0; i < NPA; ++i) a2_voff[i] = tab2[a_row[i]] + a_chunk[i];
        }
#pragma unroll
        for (int j = 0; j < NPB; ++j) {
            const int n = bn * BN + (wave + NL * j) * 8 + prow;
            w_voff[j] = n < p.N ? (unsigned)((long)n * p.w_rstride * 4) + w_chunk[j] : OOB;
        }
        set_tap(0);
    };
    // one DMA piece of the K tile the loader stands at (idx < NPA: activation rows, else weight rows); load_advance() moves on
    auto load_piece = [&](int stage, auto idx_c) {
        constexpr int idx = decltype(idx_c)::value;
        char* sbase = smem_s + stage * STG + wave * 1024;
        if constexpr (idx < NPA) {
            // the K advance rides in the instruction's scalar offset (it is not part of the range check, which the
            // out-of-range marker in the vector offset still fails): no vector add per piece
            if (dbg & 1048576)      // timing experiment: real (non-zero) data, but always the same 8 KB: the cost of the traffic itself
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(sbase + NL * idx * 1024), 16, (int)(a_voff[idx] & 0x1fffu), 0, 0, 0);
            else if (p.A2 && kL >= p.K1)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA2, (lds_ptr_t)(sbase + NL * idx * 1024), 16,
                                                         (int)(a2_voff[idx] | l_mask), (kL - p.K1) * 4, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(sbase + NL * idx * 1024), 16,
                                                         (int)(a_voff[idx] | l_mask), ciL * 4, 0, 0);
        } else {
            constexpr int j = idx - NPA;
            if (dbg & 1048576)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_ptr_t)(sbase + (BM / 8 + NL * j) * 1024), 16, (int)(w_voff[j] & 0x1fffu), 0, 0, 0);
            else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_ptr_t)(sbase + (BM / 8 + NL * j) * 1024), 16,
                                                     (int)(w_voff[j] | l_mask), kL * 4, 0, 0);
        }
    };
    auto load_advance = [&]() {
        kL += SBK; ciL += SBK;
        if (kL >= p.K) {
            if (l_mask == 0) loader_set_tile(l_vb + G, l_par ^ 1);     // on into the next output tile
        } else if (p.taps > 1 && ciL >= p.Cin) {
            ciL = 0; ++tapL; set_tap(tapL);
        }
    };
    auto load_tile = [&](int stage) {
        char* sbase = smem_s + stage * STG + wave * 1024;
        if (p.A2 && kL >= p.K1) {                                    // wave-uniform: this K tile comes from the second source
#pragma unroll
            for (int i = 0; i < NPA; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA2, (lds_ptr_t)(sbase + NL * i * 1024), 16, (int)(a2_voff[i] | l_mask), (kL - p.K1) * 4, 0, 0);
        } else
#pragma unroll
        for (int i = 0; i < NPA; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(sbase + NL * i * 1024), 16, (int)(a_voff[i] | l_mask), ciL * 4, 0, 0);
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_ptr_t)(sbase + (BM / 8 + NL * j) * 1024), 16, (int)(w_voff[j] | l_mask), kL * 4, 0, 0);
        kL += SBK; ciL += SBK;
        if (kL >= p.K) {
            if (l_mask == 0) loader_set_tile(l_vb + G, l_par ^ 1);     // on into the next output tile
        } else if (p.taps > 1 && ciL >= p.Cin) {
            ciL = 0; ++tapL; set_tap(tapL);
        }
    };

    // Two MFMA shapes (template argument MF):
    //   MF = 0  v_mfma_f32_32x32x16_f16: lane (r = lane & 31, h = lane >> 5) holds k = 16 s + 8 h .. + 7 of row r: logical
    //           chunk 2 s + h of the hi half, 4 + 2 s + h of the lo half; a K step is two 16-deep halves
    //   MF = 1  v_mfma_f32_16x16x32_f16 (the default): lane (r = lane & 15, q = lane >> 4) holds k = 8 q .. 8 q + 7 of row r:
    //           chunk q of the hi half, 4 + q of the lo half; a K step is ONE 32-deep MFMA per 16 x 16 tile.  Same LDS
    //           image, same reads per step (16 ds_read_b128 per wave), conflict-free under the same swizzle, same
    //           accumulator count.  The chip holds a higher clock on this shape for the same work: the bare MFMA + LDS
    //           loop of this kernel ran 215 vs 245 us per unit of work at 1.82 vs 1.56 GHz (tools/micro/mfma_shape.hip).
    const int frow = (lane & 31) * 128, fsw = ((lane & 31) >> 1) & 7, fh = lane >> 5;
    int fo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) fo[c] = frow + (((2 * c + fh) ^ fsw) * 16);
    const int r16 = lane & 15, q4 = lane >> 4;
    // 16-row tiles start at multiples of 16 rows, so the swizzle term (row >> 1) & 7 depends on r16 alone
    const int fo16h = r16 * 128 + ((q4 ^ ((r16 >> 1) & 7)) * 16), fo16l = r16 * 128 + (((4 + q4) ^ ((r16 >> 1) & 7)) * 16);
#if G16_HI
    (void)fo16l;
#endif
    const int offA = wm * WM * 128, offB = (BM + wn * WN) * 128;

    // Operand order: the weight fragment is the MFMA's A operand and the activation fragment its B operand, so the
    // accumulator comes out transposed: lane -> output ROW, registers -> 4-column runs.  A 32 x 32 block of the wave tile
    // is four "sub-runs" s = 0..3 of 4 columns per lane:
    //   MF = 0: row = lane & 31,               col = 8 s + 4 (lane >> 5)          (registers 4 s .. 4 s + 3 of the 32x32 tile)
    //   MF = 1: row = 16 (s >> 1) + (lane & 15), col = 16 (s & 1) + 4 (lane >> 4)   (the 16x16 tile (s >> 1, s & 1) of the block)
    // The epilogue then moves 16 bytes (fp32) or 8 + 8 bytes (S32) per lane and store, and bias / gamma are per-register vectors.
    constexpr int TM16 = WM / 16, TN16 = WN / 16, TNH = TN16 / 2;
#if G16_HI
    f32x16 accm[MF ? 1 : TM][MF ? 1 : TN];
    f32x4 am[MF ? TM16 : 1][MF ? TN16 : 1];
    struct Frags { f16x8 ah[TM], bh[TN]; };
#else
    f32x16 accm[MF ? 1 : TM][MF ? 1 : TN], accc[MF ? 1 : TM][MF ? 1 : TN];
    f32x4 am[MF ? TM16 : 1][MF ? TN16 : 1], ac[MF ? TM16 : 1][MF ? TN16 : 1];
    struct Frags { f16x8 ah[TM], al[TM], bh[TN], bl[TN]; };
#endif
    auto read_frags = [&](int stage, int s, Frags& F) {
        const char* sA = smem_s + stage * STG + offA;
        const char* sB = smem_s + stage * STG + offB;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            F.ah[i] = *reinterpret_cast<const f16x8*>(sA + i * 32 * 128 + fo[s]);
#if !G16_HI
            F.al[i] = *reinterpret_cast<const f16x8*>(sA + i * 32 * 128 + fo[2 + s]);
#endif
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            F.bh[j] = *reinterpret_cast<const f16x8*>(sB + j * 32 * 128 + fo[s]);
#if !G16_HI
            F.bl[j] = *reinterpret_cast<const f16x8*>(sB + j * 32 * 128 + fo[2 + s]);
#endif
        }
    };
    auto mfma_block = [&](const Frags& F) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                accm[MF ? 0 : i][MF ? 0 : j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.bh[j], F.ah[i], accm[MF ? 0 : i][MF ? 0 : j], 0, 0, 0);
#if !G16_HI
                accc[MF ? 0 : i][MF ? 0 : j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.bl[j], F.ah[i], accc[MF ? 0 : i][MF ? 0 : j], 0, 0, 0);
                accc[MF ? 0 : i][MF ? 0 : j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(F.bh[j], F.al[i], accc[MF ? 0 : i][MF ? 0 : j], 0, 0, 0);
#endif
            }
    };
    // MF = 1: the activation fragments of a step (all TM16 row tiles) and the weight fragments in two halves of TNH column tiles
#if G16_HI
    struct FragA { f16x8 h[TM16]; };
    struct FragB { f16x8 h[TNH]; };
#else
    struct FragA { f16x8 h[TM16], l[TM16]; };
    struct FragB { f16x8 h[TNH], l[TNH]; };
#endif
    auto read_a16 = [&](int stage, FragA& F) {
        const char* sA = smem_s + stage * STG + offA;
#pragma unroll
        for (int i = 0; i < TM16; ++i) {
            F.h[i] = *reinterpret_cast<const f16x8*>(sA + i * 16 * 128 + fo16h);
#if !G16_HI
            F.l[i] = *reinterpret_cast<const f16x8*>(sA + i * 16 * 128 + fo16l);
#endif
        }
    };
    auto read_b16 = [&](int stage, int half, FragB& F) {
        const char* sB = smem_s + stage * STG + offB + half * TNH * 16 * 128;
#pragma unroll
        for (int j = 0; j < TNH; ++j) {
            F.h[j] = *reinterpret_cast<const f16x8*>(sB + j * 16 * 128 + fo16h);
#if !G16_HI
            F.l[j] = *reinterpret_cast<const f16x8*>(sB + j * 16 * 128 + fo16l);
#endif
        }
    };
    auto mfma16_block = [&](const FragA& A, const FragB& Bf, auto half_c, auto&& between) {
        constexpr int half = decltype(half_c)::value;          // a constant: the accumulators must stay in registers
#pragma unroll
        for (int jj = 0; jj < TNH; ++jj)
#pragma unroll
            for (int i = 0; i < TM16; ++i) {
                between(jj * TM16 + i);
                constexpr int jbase = half * TNH;
                const int j = jbase + jj;
                f32x4& m = am[MF ? i : 0][MF ? j : 0];
#if G16_HI
                m = __builtin_amdgcn_mfma_f32_16x16x32_f16(Bf.h[jj], A.h[i], m, 0, 0, 0);
#else
                f32x4& c = ac[MF ? i : 0][MF ? j : 0];
                m = __builtin_amdgcn_mfma_f32_16x16x32_f16(Bf.h[jj], A.h[i], m, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Bf.l[jj], A.h[i], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Bf.h[jj], A.l[i], c, 0, 0, 0);
#endif
            }
    };

    // NSTAGE-deep ring of LDS stages, ONE barrier per K step, placed in the MIDDLE of the step:
    //   top    : DMA of the K tile NSTAGE-1 steps ahead -> the stage the previous step's tile occupied (all its reads
    //            retired before the previous barrier); read the second-half fragments of this step's tile; MFMAs on
    //            its first half (already in registers)
    //   middle : each wave waits for ITS OWN pieces of the next K tile (counted vmcnt: younger tiles stay in flight)
    //            and for its LDS reads, then the barrier makes that tile visible to everyone
    //   bottom : read the first-half fragments of the next K tile, MFMAs on the second half of this one
    // so no wave sits behind a barrier with nothing to issue: fragments always arrive under the other half's MFMAs.
    // (MF = 0: the halves are the two 16-deep k halves of the step.  MF = 1: the halves are the first and the last TNH
    // weight column tiles; the activation fragments serve both halves, so the next step's are read last in the bottom
    // phase, into the registers the second half's MFMAs have just read.)
    // The stream does not stop at an output-tile boundary: the first K tiles of the workgroup's next output tile are
    // already landing while the last steps of this one run, its first fragments are read before the epilogue, and
    // the epilogue's own loads and stores simply queue behind them.  Past the last tile the DMAs are issued all the
    // same with out-of-range offsets (constant wait counts).
    const int nk = p.K / SBK;
    f32x4 fake = {0.1f * lane, 0.2f, -0.3f, 0.01f * lane};
    const __amdgpu_buffer_rsrc_t rsFake = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 1024, 0x00020000);
    float amax = 0.f;            // largest magnitude this wave converts to the split-f16 form (range_report at the end)
    // operands may carry a per-tensor power-of-two scale (weights at load, the single-stage entry points): the
    // accumulators are brought back by acc_s, exactly (a power of two), before bias and activation
    const float acc_s = p.acc_scale_dev ? *p.acc_scale_dev : p.acc_scale;
#if !G16_HI
    const float lo_s = acc_s * (1.f / 2048.f);
#endif
    if ((dbg & 64) && wave >= NW / 2) __builtin_amdgcn_s_setprio(1);     // experiment: static priority for the younger half
    unsigned long long st_c0 = 0, st_r0 = 0;
    if (dbg & 1024) { st_c0 = __builtin_amdgcn_s_memtime(); st_r0 = __builtin_amdgcn_s_memrealtime(); }
    build_table(blockIdx.x, 0);
    __syncthreads();
    loader_set_tile(blockIdx.x, 0);
    if (dma_wave) {
#pragma unroll
        for (int s = 0; s < (KS == 2 ? 4 : NSTAGE - 1); ++s) load_tile(s);   // needs nk >= NSTAGE - 1 when a next tile exists (host)
    }
    if (KS == 2) wait_vm_lgkm<2 * NPT>(); else wait_vm_lgkm<(NSTAGE - 2) * NPT>();
    __builtin_amdgcn_s_barrier();
    Frags F0, F1;
    FragA Fa;
    FragB F0b, F1b;
    if (MF) { if (mfma_wave) { read_a16(0, Fa); read_b16(0, 0, F0b); } }
    else read_frags(0, 0, F0);
    int rs = 0, ws = KS == 2 ? 4 : NSTAGE - 1;
    int c_par = 0;
    FragA Fa2;           // KS = 2: fragments of the second K tile of a pair
    FragB F0b2, F1b2;
    for (int vb = blockIdx.x; vb < ntiles; vb += G, c_par ^= 1) {
        // the table of this workgroup's next output tile: the loader turns to it NSTAGE-1 steps before this tile's
        // K loop ends, i.e. after at least one of the barriers below (host: nk >= NSTAGE + 1 in persistent launches)
        build_table(vb + G, c_par ^ 1);
        int bm, bn;
        tile_coords(vb, bm, bn);
        // This wave's WN bias (and gamma) values go into a private LDS cache by DMA now, a K loop ahead of their use: a
        // global load in the epilogue would have to wait for vmcnt(0), i.e. for every store issued before it, and the
        // epilogue would run one store round trip at a time (it did: 15 of pwconv1's 110 us).  The K loop's counted
        // waits only ever leave the youngest DMA pieces outstanding, so the cache is complete long before it is read.
        // (loader waves skip the epilogue and would be here while the MFMA waves still read the previous tile's cache: in a
        // persistent launch the two roles meet before it is overwritten)
        if constexpr (PROD != 0 && PCACHE) { if (vb != (int)blockIdx.x) __syncthreads(); }
        if (PCACHE && dma_wave && wave < NW && lane < WN / 4) {
            const int nb4 = (bn * BN + wn * WN + 4 * lane) * 4;
            char* pc = smem_s + p.pc_off + wave * PC_BYTES;
            if (p.bias) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBias, (lds_ptr_t)pc, 16, nb4, 0, 0, 0);
            if (EPI == EPI_BIAS_GAMMA_RES) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsGamma, (lds_ptr_t)(pc + WN * 4), 16, nb4, 0, 0, 0);
        }
        if (MF) {
#pragma unroll
            for (int i = 0; i < TM16; ++i)
#pragma unroll
#if G16_HI
                for (int j = 0; j < TN16; ++j) am[MF ? i : 0][MF ? j : 0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#else
                for (int j = 0; j < TN16; ++j) { am[MF ? i : 0][MF ? j : 0] = (f32x4){0.f, 0.f, 0.f, 0.f}; ac[MF ? i : 0][MF ? j : 0] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#endif
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
#if G16_HI
                    for (int r = 0; r < 16; ++r) accm[MF ? 0 : i][MF ? 0 : j][r] = 0.f;
#else
                    for (int r = 0; r < 16; ++r) { accm[MF ? 0 : i][MF ? 0 : j][r] = 0.f; accc[MF ? 0 : i][MF ? 0 : j][r] = 0.f; }
#endif
        }
        if constexpr (KS == 2) {
            // K tiles kt, kt + 1 (stages rs, rs + 1) are resident and visible; the next pair is in flight since the previous
            // iteration and is waited for at the bottom of this one; the pair after it is requested now.  nk is even (host)
            for (int kt = 0; kt < nk; kt += 2) {
                const int rs1 = rs + 1;                          // rs is even, < 6
                if (dma_wave) {
                    load_tile(ws);
                    load_tile(ws + 1);
                }
                if (mfma_wave) {
                    // every fragment of both tiles is requested before the first MFMA (both tiles have been visible since the
                    // last barrier): the LDS latency is paid once per pair, the MFMAs then run back to back
                    read_b16(rs, 1, F1b);
                    read_a16(rs1, Fa2);
                    read_b16(rs1, 0, F0b2);
                    read_b16(rs1, 1, F1b2);
                    mfma16_block(Fa, F0b, std::integral_constant<int, 0>{}, [](int) {});
                    mfma16_block(Fa, F1b, std::integral_constant<int, 1>{}, [](int) {});
                    mfma16_block(Fa2, F0b2, std::integral_constant<int, 0>{}, [](int) {});
                    mfma16_block(Fa2, F1b2, std::integral_constant<int, 1>{}, [](int) {});
                }
                wait_vm_lgkm<2 * NPT>();     // all but the pair just requested; and this wave's LDS reads (their stages are the next DMA target)
                __builtin_amdgcn_s_barrier();
                rs = rs + 2 == 6 ? 0 : rs + 2;
                ws = ws + 2 == 6 ? 0 : ws + 2;
                if (mfma_wave) {
                    read_a16(rs, Fa);        // first fragments of the next pair (after the last pair: of the next output tile);
                    read_b16(rs, 0, F0b);    // their latency passes under the DMA issue at the top of the loop
                }
            }
        } else
        for (int kt = 0; kt < nk; ++kt) {
            // (tried: the younger half of the waves issuing its DMA pieces after the first-half MFMAs instead of before them,
            // so that one wave's DMA issue runs beside its SIMD partner's MFMAs: 5.79 vs 5.80 ms per step A/B on one box: nothing)
            constexpr bool SPREAD = MF && !(dbg & 2048) && NPT <= TNH * TM16;     // one DMA piece in front of each MFMA group (below)
            if (!(dbg & 1) && !SPREAD) load_tile(ws);
            if (MF) {
                if (!(dbg & 16)) read_b16(rs, 1, F1b);
                if (dbg & 8192) __builtin_amdgcn_s_setprio(1);
                if (!(dbg & 2)) mfma16_block(Fa, F0b, std::integral_constant<int, 0>{}, [&](int grp) {
                    if constexpr (SPREAD) {
                        if (!(dbg & 1)) {
                            // grp is a compile-time constant after unrolling; the pieces go out in front of groups 0 .. NPT-1
#define WT_PIECE(I) if (NPT > I && grp == I) load_piece(ws, std::integral_constant<int, (NPT > I ? I : 0)>{});
                            WT_PIECE(0) WT_PIECE(1) WT_PIECE(2) WT_PIECE(3) WT_PIECE(4) WT_PIECE(5)
                            WT_PIECE(6) WT_PIECE(7) WT_PIECE(8) WT_PIECE(9) WT_PIECE(10) WT_PIECE(11)
#undef WT_PIECE
                        }
                    }
                });
                if (dbg & 8192) __builtin_amdgcn_s_setprio(0);
                if (SPREAD && !(dbg & 1)) load_advance();
            } else {
                if (!(dbg & 16)) read_frags(rs, 1, F1);
                if (!(dbg & 2)) mfma_block(F0);
            }
            // timing experiment: what an epilogue drained inside the K loop would cost - per K step the GELU + split of one
            // 4-column run and its two 8-byte stores (out of range: counted, dropped), scheduled among the MFMAs.  With bit
            // 16777216 the two waves of a SIMD drain in different halves of the step (waves 0-3 after the barrier, 4-7 in front
            // of it), so that one wave's vector work meets the other's MFMAs
            auto fake_drain = [&]() {
                fake = gelu_erfc_s4(fake + (f32x4){1e-3f, 2e-3f, 3e-3f, 4e-3f});
                f16x4 fh, fl;
                split4_f16(fake.x, fake.y, fake.z, fake.w, fh, fl);
                amax = amax4(amax, fake.x, fake.y, fake.z, fake.w);
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, fh), rsFake, (int)0x7ffffff0, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, fl), rsFake, (int)0x7ffffff0, 0, 0);
            };
            if constexpr ((dbg & 2097152) != 0) {
                if (!(dbg & 16777216) || wave >= NW / 2) fake_drain();
            }
            if (dbg & 32768) { if (!(dbg & 32)) wait_vm_lgkm<63>(); }                 // timing experiment: DMA issued, never waited for (races)
            else if (!(dbg & 32)) {
                // (the drain's two stores are younger than this step's DMA pieces only where they were issued behind them)
                if ((dbg & 2097152) && (!(dbg & 16777216) || wave >= NW / 2)) wait_vm_lgkm<(NSTAGE - 2) * NPT + 2>();
                else wait_vm_lgkm<(NSTAGE - 2) * NPT>();
            }
            if (!(dbg & 8)) __builtin_amdgcn_s_barrier();
            rs = rs + 1 == NSTAGE ? 0 : rs + 1;
            ws = ws + 1 == NSTAGE ? 0 : ws + 1;
            if constexpr ((dbg & 2097152) != 0 && (dbg & 16777216) != 0) {
                if (wave < NW / 2) fake_drain();
            }
            if (MF) {
                if (!(dbg & 16)) read_b16(rs, 0, F0b);       // after the very last step: a harmless read of a zero-filled stage
                if (dbg & 8192) __builtin_amdgcn_s_setprio(1);
                if (!(dbg & 2)) mfma16_block(Fa, F1b, std::integral_constant<int, 1>{}, [](int) {});
                if (dbg & 8192) __builtin_amdgcn_s_setprio(0);
                if (!(dbg & 16)) read_a16(rs, Fa);
            } else {
                if (!(dbg & 16)) read_frags(rs, 0, F0);
                if (!(dbg & 2)) mfma_block(F1);
            }
        }
        if (dbg & 4) {      // timing builds without an epilogue: keep the accumulators (and so the MFMAs) alive through
                            // a store the compiler cannot rule out (alpha is never this value)
            if (p.alpha == -12345.f) {
                if (MF) {
#pragma unroll
                    for (int i = 0; i < TM16; ++i)
#pragma unroll
                        for (int j = 0; j < TN16; ++j)
#pragma unroll
#if G16_HI
                            for (int r = 0; r < 4; ++r) p.C[(tid * 4 + r) * 2] = am[MF ? i : 0][MF ? j : 0][r];
#else
                            for (int r = 0; r < 4; ++r) p.C[(tid * 4 + r) * 2] = am[MF ? i : 0][MF ? j : 0][r] + ac[MF ? i : 0][MF ? j : 0][r];
#endif
                } else {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
#pragma unroll
#if G16_HI
                            for (int r = 0; r < 16; ++r) p.C[(tid * 16 + r) * 2] = accm[MF ? 0 : i][MF ? 0 : j][r];
#else
                            for (int r = 0; r < 16; ++r) p.C[(tid * 16 + r) * 2] = accm[MF ? 0 : i][MF ? 0 : j][r] + accc[MF ? 0 : i][MF ? 0 : j][r];
#endif
                }
            }
            continue;
        }

    // ------------------------------------------------------------------------- epilogue
    if (loader_wave) continue;               // (no barrier from here to the end of the tile loop)
    const int m_w = bm * BM + wm * WM, n_w = bn * BN + wn * WN;
    float* __restrict__ Cg = p.C + (long)z * p.zC;
    // sub-run s of a 32 x 32 block: its row and first column inside the block (see the accumulator layouts above)
    auto sub_row = [&](int s) { return MF ? 16 * (s >> 1) + r16 : (lane & 31); };
    auto sub_col = [&](int s) { return MF ? 16 * (s & 1) + 4 * q4 : 8 * s + 4 * (lane >> 5); };
    auto acc4 = [&](int i, int j, int s) {
        f32x4 v;
#if G16_HI
        // one product: the main accumulator is the result (on operands whose lo halves are zero these are the bits of the
        // three-product kernel, whose correction accumulator then holds +0)
        if (MF) {
            v = am[MF ? 2 * i + (s >> 1) : 0][MF ? 2 * j + (s & 1) : 0] * acc_s;
        } else {
            v.x = accm[MF ? 0 : i][MF ? 0 : j][4 * s + 0] * acc_s;
            v.y = accm[MF ? 0 : i][MF ? 0 : j][4 * s + 1] * acc_s;
            v.z = accm[MF ? 0 : i][MF ? 0 : j][4 * s + 2] * acc_s;
            v.w = accm[MF ? 0 : i][MF ? 0 : j][4 * s + 3] * acc_s;
        }
#else
        if (MF) {
            const f32x4 m = am[MF ? 2 * i + (s >> 1) : 0][MF ? 2 * j + (s & 1) : 0], c = ac[MF ? 2 * i + (s >> 1) : 0][MF ? 2 * j + (s & 1) : 0];
            v.x = fmaf(c.x, lo_s, m.x * acc_s);
            v.y = fmaf(c.y, lo_s, m.y * acc_s);
            v.z = fmaf(c.z, lo_s, m.z * acc_s);
            v.w = fmaf(c.w, lo_s, m.w * acc_s);
        } else {
            v.x = fmaf(accc[MF ? 0 : i][MF ? 0 : j][4 * s + 0], lo_s, accm[MF ? 0 : i][MF ? 0 : j][4 * s + 0] * acc_s);
            v.y = fmaf(accc[MF ? 0 : i][MF ? 0 : j][4 * s + 1], lo_s, accm[MF ? 0 : i][MF ? 0 : j][4 * s + 1] * acc_s);
            v.z = fmaf(accc[MF ? 0 : i][MF ? 0 : j][4 * s + 2], lo_s, accm[MF ? 0 : i][MF ? 0 : j][4 * s + 2] * acc_s);
            v.w = fmaf(accc[MF ? 0 : i][MF ? 0 : j][4 * s + 3], lo_s, accm[MF ? 0 : i][MF ? 0 : j][4 * s + 3] * acc_s);
        }
#endif
        return v;
    };

    if constexpr (EPI == EPI_ARGMAX) {
        // VQ (core_vq.py:176-182): per row, the best of this wave's WN columns of -(|x|^2 - 2 x.e + |e|^2), lowest
        // index on ties.  MF = 0: a lane holds one row, its partner lane + 32 the other half of the columns.  MF = 1: a
        // lane holds two rows (16 apart), and the four lanes r16, r16 + 16, + 32, + 48 share a row's columns.
        const int part = bn * WAVES_N + wn;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int rsel = 0; rsel < (MF ? 2 : 1); ++rsel) {
                const int m = m_w + i * 32 + (MF ? 16 * rsel + r16 : (lane & 31));
                const float xx = (m < p.M) ? p.vq_xx[m] : 0.f;
                float best = -INFINITY;
                int bidx = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int ss = 0; ss < (MF ? 2 : 4); ++ss) {
                        const int s = MF ? 2 * rsel + ss : ss;          // ascending columns within the lane either way
                        const int n = n_w + j * 32 + sub_col(s);
                        if (n >= p.N) continue;
                        const f32x4 dot = acc4(i, j, s);
                        const f32x4 ee = *reinterpret_cast<const f32x4*>(p.vq_ee + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float d = -((xx - 2.f * dot[e]) + ee[e]);
                            if (d > best) { best = d; bidx = n + e; }        // ascending n within the lane: strict > keeps the lowest
                        }
                    }
#pragma unroll
                for (int off = (MF ? 16 : 32); off <= 32; off <<= 1) {
                    const float ov = __shfl_xor(best, off, 64);
                    const int oi = __shfl_xor(bidx, off, 64);
                    if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
                }
                if ((MF ? q4 == 0 : lane < 32) && m < p.M) {
                    p.vq_pval[(long)m * p.vq_nparts + part] = best;
                    p.vq_pidx[(long)m * p.vq_nparts + part] = bidx;
                }
            }
    } else if constexpr (EPI == EPI_HEAD) {
        // packed rows come in 32-row groups: 16 log-magnitude rows, then the 16 phase rows of the same spectrum slots
        // (weights.cpp), so every 32 x 32 block holds both halves of 16 slots whatever the tile width: the sub-run s of
        // columns < 16 pairs with the sub-run of the same rows 16 columns on
        auto head_run = [&](int i, int j, int h, f32x4& re, f32x4& im) {
            const int s = MF ? 2 * h : h, sp = MF ? s + 1 : s + 2;
            const int pc = n_w + j * 32 + sub_col(s);         // packed row of the log-magnitude; phase 16 later
            const f32x4 bmag = *reinterpret_cast<const f32x4*>(pcw + (pc - n_w) * 4);
            const f32x4 bph = *reinterpret_cast<const f32x4*>(pcw + (pc + 16 - n_w) * 4);
            const f32x4 lm = acc4(i, j, s) + bmag, ph = acc4(i, j, sp) + bph;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float mag = fminf((dbg & 4194304) ? expf(lm[e]) : exp_head(fminf(lm[e], 88.f)), 100.f);      // heads.py:55-56
                float sn, cs;
                if (dbg & 4194304) sincosf(ph[e], &sn, &cs); else sincos_head(ph[e], sn, cs);     // one range reduction for both
                re[e] = mag * cs;
                im[e] = mag * sn;
            }
        };
        if (OUT == OUT_S32 && WN % 64 == 0 && p.stage_epi && !(dbg & 8388608)) {
            // Staged: two neighbouring blocks hold the 32 slots of one S32 group (128 bytes of a spectrum row, re and im each).
            // The 32 x 32-slot tile goes through the wave's LDS scratch in the S32 row image and leaves as full lines, like
            // the staged epilogue of the hot layers below (direct form: 8-byte pieces, 16 stores per block)
            char* sc = smem_s + p.stage_off + wave * 4096;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jp = 0; jp + 1 < TN; jp += 2) {
                    const int n0 = n_w + jp * 32;
                    if (n0 >= p.N) continue;                       // wave-uniform; N % 64 == 0 (host)
                    f32x4 re[4], im[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) head_run(i, jp + (k >> 1), k & 1, re[k], im[k]);
#pragma unroll
                    for (int pz = 0; pz < 2; ++pz) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int sk = MF ? 2 * (k & 1) : (k & 1);
                            const int rw = sub_row(sk), cw = 16 * (k >> 1) + (sub_col(sk) & 15), sww = (rw >> 1) & 7;
                            const f32x4 v = pz ? im[k] : re[k];
                            amax = amax4(amax, v.x, v.y, v.z, v.w);
                            f16x4 hi, lo;
                            split4_f16(v.x, v.y, v.z, v.w, hi, lo);
                            *reinterpret_cast<f16x4*>(sc + rw * 128 + (((cw >> 3) ^ sww) * 16) + 2 * (cw & 7)) = hi;
                            *reinterpret_cast<f16x4*>(sc + rw * 128 + (((4 + (cw >> 3)) ^ sww) * 16) + 2 * (cw & 7)) = lo;
                        }
                        f32x4 q[4];
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int r = 8 * it + (lane >> 3), ch = lane & 7;
                            q[it] = *reinterpret_cast<const f32x4*>(sc + r * 128 + ((ch ^ ((r >> 1) & 7)) * 16));
                        }
                        const int f0 = (n0 >> 6) * 32 + pz * p.head_kb;           // first slot of the group, as a float index of the row
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int r = 8 * it + (lane >> 3), ch = lane & 7;
                            const int m = m_w + i * 32 + r;
                            if (m < p.M && !(dbg & 128)) store_c16<!(dbg & 4096)>(Cg + (long)m * p.c_rstride + f0 + 4 * ch, q[it]);
                        }
                    }
                }
        } else
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = MF ? 2 * h : h;
                    const int m = m_w + i * 32 + sub_row(s);
                    const int pc = n_w + j * 32 + sub_col(s);
                    if (m >= p.M || pc >= p.N) continue;
                    float* crow = Cg + (long)m * p.c_rstride;
                    f32x4 re, im;
                    head_run(i, j, h, re, im);
                    const int f = (pc >> 5) * 16 + (pc & 15);          // spectrum slot
                    if (dbg & 128) {           // timing experiment: no stores
                        amax = amax4(amax4(amax, re.x, re.y, re.z, re.w), im.x, im.y, im.z, im.w);
                    } else if (OUT == OUT_S32) {
                        store_s32_x4(crow, f, re, amax);
                        store_s32_x4(crow, p.head_kb + f, im, amax);
                    } else {
                        *reinterpret_cast<f32x4*>(crow + f) = re;
                        *reinterpret_cast<f32x4*>(crow + p.head_kb + f) = im;
                    }
                }
        }
    } else {
        // Staged form (the hot layers): a lane holds 4-column runs of ONE row, so direct stores touch 32 rows x 32 B
        // per instruction.  Each 32x32 sub-tile goes through a 4 KB wave-private LDS scratch instead (chunk-swizzled,
        // conflict-free both ways) and is read back with 8 lanes per 128-byte row: every store is then a full line
        // (measured: pwconv1 + GELU 114 -> 109 us; the residual epilogues gained nothing and stay direct).
        constexpr bool DUAL = OUT == OUT_S32_DUAL_ELU || OUT == OUT_F32_AND_S32;
        constexpr bool CAN_STAGE = ((OUT == OUT_F32 || DUAL) && EPI == EPI_BIAS) ||
                                   (OUT == OUT_S32 && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_ELU));
        if (CAN_STAGE && p.stage_epi) {
            char* sc = smem_s + p.stage_off + wave * 4096;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n0 = n_w + j * 32;
                    if (n0 >= p.N) continue;                       // wave-uniform
                    // a dual-output launch sends the block through the scratch twice, once per destination format
#pragma unroll
                    for (int pz = 0; pz < (DUAL ? 2 : 1); ++pz) {
                        const bool as_f32 = OUT == OUT_F32 || (OUT == OUT_F32_AND_S32 && pz == 0);
                        // the block's four bias vectors in one LDS round trip
                        f32x4 bq[4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int n = n0 + sub_col(g);
                            bq[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
                            if (p.bias && n < p.N && !(dbg & 256))
                                bq[g] = PCACHE ? *reinterpret_cast<const f32x4*>(pcw + (n - n_w) * 4) : *reinterpret_cast<const f32x4*>(p.bias + n);
                        }
                        f32x4 vb[4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) vb[g] = acc4(i, j, g) + bq[g];
                        if (EPI == EPI_BIAS_GELU && !(dbg & 512)) {
                            if (dbg & 16384) {
#pragma unroll
                                for (int g = 0; g < 4; ++g) vb[g] = gelu_erf_s4(vb[g]);
                            } else if (dbg & 524288) {
#pragma unroll
                                for (int g = 0; g < 4; ++g) vb[g] = gelu_erfc_s4(vb[g]);
                            } else {
                                gelu_erfc_x16(vb);
                            }
                        }
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int rw = sub_row(g), cw = sub_col(g), sww = (rw >> 1) & 7;
                            f32x4 v = vb[g];
                            if (EPI == EPI_BIAS_ELU || (OUT == OUT_S32_DUAL_ELU && pz == 1)) {
                                v.x = elu_s(v.x); v.y = elu_s(v.y); v.z = elu_s(v.z); v.w = elu_s(v.w);
                            }
                            if (as_f32) {
                                *reinterpret_cast<f32x4*>(sc + rw * 128 + (((cw >> 2) ^ sww) * 16)) = v;
                            } else {
                                amax = amax4(amax, v.x, v.y, v.z, v.w);
                                f16x4 hi, lo;
                                split4_f16(v.x, v.y, v.z, v.w, hi, lo);
                                *reinterpret_cast<f16x4*>(sc + rw * 128 + (((cw >> 3) ^ sww) * 16) + 2 * (cw & 7)) = hi;
                                *reinterpret_cast<f16x4*>(sc + rw * 128 + (((4 + (cw >> 3)) ^ sww) * 16) + 2 * (cw & 7)) = lo;
                            }
                        }
                        // a wave's LDS operations execute in order and the scratch is private to the wave: no barrier
                        float* dbase = pz == 0 ? Cg : p.C2 + (long)z * p.zC;
                        // all four read-backs first (one LDS round trip per 32x32 block, not four), then the stores
                        f32x4 q[4];
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int r = 8 * it + (lane >> 3), ch = lane & 7;
                            q[it] = *reinterpret_cast<const f32x4*>(sc + r * 128 + ((ch ^ ((r >> 1) & 7)) * 16));
                        }
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int r = 8 * it + (lane >> 3), ch = lane & 7;
                            const int m = m_w + i * 32 + r;
                            const int n = n0 + 4 * ch;             // fp32 columns; S32: byte ch * 16 of the group at n0
                            if (m < p.M && (!as_f32 || n < p.N) && !(dbg & 128)) {
                                float* dst = dbase + (long)m * p.c_rstride + n;
                                store_c16<!(dbg & 4096)>(dst, q[it]);
                            }
                        }
                    }
                }
            }
        } else
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int m = m_w + i * 32 + sub_row(g);
                    const int n = n_w + j * 32 + sub_col(g);        // columns n .. n+3 (N % 4 == 0)
                    if (m >= p.M || n >= p.N) continue;
                    float* crow = Cg + (long)m * p.c_rstride;
                    f32x4 v = acc4(i, j, g);
                    if (EPI == EPI_SCALE || EPI == EPI_BIAS_ROW) {
                        v = EPI == EPI_SCALE ? v * p.alpha : v + p.bias[m];
                        // these two take any N: the columns of a partial last run are written as zeros (pad columns
                        // of the row pitch, which the consumers rely on being zero)
                        if (n + 3 >= p.N) { if (n + 1 >= p.N) v.y = 0.f; if (n + 2 >= p.N) v.z = 0.f; v.w = 0.f; }
                    }
                    else if (p.bias) v += PCACHE ? *reinterpret_cast<const f32x4*>(pcw + (n - n_w) * 4) : *reinterpret_cast<const f32x4*>(p.bias + n);
                    if (EPI == EPI_BIAS_RES) {
                        v = v + *reinterpret_cast<const f32x4*>(p.R + (long)m * p.r_rstride + n);
                    } else if (EPI == EPI_BIAS_RES_ELU) {
                        v = v + *reinterpret_cast<const f32x4*>(p.R + (long)m * p.r_rstride + n);
                        v.x = elu_s(v.x); v.y = elu_s(v.y); v.z = elu_s(v.z); v.w = elu_s(v.w);
                    } else if (EPI == EPI_BIAS_ELU) {
                        v.x = elu_s(v.x); v.y = elu_s(v.y); v.z = elu_s(v.z); v.w = elu_s(v.w);
                    } else if (EPI == EPI_BIAS_GELU) {
                        v = (dbg & 16384) ? gelu_erf_s4(v) : gelu_erfc_s4(v);
                    } else if (EPI == EPI_BIAS_GAMMA_RES) {
                        const f32x4 gm = *reinterpret_cast<const f32x4*>(pcw + WN * 4 + (n - n_w) * 4);      // EPI_BIAS_GAMMA_RES: always cached
                        v = *reinterpret_cast<const f32x4*>(p.R + (long)m * p.r_rstride + n) + gm * v;
                    }
                    if (OUT == OUT_S32 || OUT == OUT_S32_DUAL_ELU) store_s32_x4(crow, n, v, amax);
                    else store_c16<(dbg & 262144) != 0>(crow + n, v);
                    if (OUT == OUT_S32_DUAL_ELU) {
                        f32x4 ev;
                        ev.x = elu_s(v.x); ev.y = elu_s(v.y); ev.z = elu_s(v.z); ev.w = elu_s(v.w);
                        store_s32_x4(p.C2 + (long)z * p.zC + (long)m * p.c_rstride, n, ev, amax);
                    } else if (OUT == OUT_F32_AND_S32) {
                        store_s32_x4(p.C2 + (long)z * p.zC + (long)m * p.c_rstride, n, v, amax);
                    }
                }
        }
    }
    }   // persistent tile loop
    if ((dbg & 1024) && p.dbg_stamps && tid == 0) {
        p.dbg_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st_c0;
        p.dbg_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st_r0;
    }
    range_report(p.status, amax);
    if (p.stamp_end) {                       // ... and the latest exit, after every wave's stores have been acknowledged
        wait_vm_lgkm<0>();
        __syncthreads();
        if (tid == 0)
            __hip_atomic_fetch_max(p.stamp_end, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    wait_vm_lgkm<0>();
}
