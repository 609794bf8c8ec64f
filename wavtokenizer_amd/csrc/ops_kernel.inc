// The kernels of ops.hip that a decode plan runs per clip length: transpose, code_rows, GroupNorm (gn_stats, gn_tile, gn_chunk_stats /
// gn_chunk_apply), dwconv_ln, softmax (rmw and reg forms) and istft_ola.  Included twice by ops.hip with OPS_MIX, OPS_K and OPS_L
// set.  With OPS_MIX 0 (OPS_K(x) = x_kernel, OPS_L = L) the preprocessed text is exactly the kernels of the plans of one length.
// OPS_MIX 1 (x_mixed_kernel, OPS_L = Lpad) is the length-aware twin of a WT_PLAN_DECODE_MIXED plan: the tensors have Lpad rows per
// clip, `lens` (device int32 [B]) holds every clip's own length L, clamped to [0, Lpad] before it indexes anything (mix_len).  A
// clip's statistics, softmax sums and overlap-add run over its own L rows in the order of a call of its own; output rows
// [L, Lpad) are zeros.  GroupNorm picks its form per clip: each form's workgroups serve the clips whose own length selects that
// form in a call of their own (lmax / lmin) and leave at once for the others.

// ------------------------------------------------------------------------------------ transpose
// [B][R][C] -> [B][C][R] through a padded 32x32 LDS tile (coalesced on both sides).
__global__ __launch_bounds__(256) void OPS_K(transpose)(const float* __restrict__ in, float* __restrict__ out, int R,
                                                        int C, int s32, unsigned* status
#if OPS_MIX
                                                        , const int* __restrict__ lens     // output rows c >= lens[clip] are zeros
#endif
                                                        ) {
    __shared__ float tile[32][33];
    float amax = 0.f;
    const long boff = (long)blockIdx.z * R * C;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        if (r < R && c < C) tile[i][tx] = in[boff + (long)r * C + c];
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (r < R && c < C) {
#if OPS_MIX
            const float v = c < mix_len(lens, blockIdx.z, C) ? tile[tx][i] : 0.f;      // (a select: what the caller left there is dropped)
            if (s32) store_s32_1(out + boff + (long)c * R, r, v, amax);
            else out[boff + (long)c * R + r] = v;
#else
            if (s32) store_s32_1(out + boff + (long)c * R, r, tile[tx][i], amax);
            else out[boff + (long)c * R + r] = tile[tx][i];
#endif
        }
    }
    range_report(status, amax);
}

// ------------------------------------------------------------------------------------ code_rows
// The first step of a decode-from-codes plan: codes [K][B][L] int64 -> y [B][L][C], row (b, t) = sum over k of
// table[(k * bins + codes[k][b][t]) * C ...], i.e. what codes_to_features_kernel followed by transpose_kernel leaves in bb.in,
// without the (B, C, L) fp32 tensor between them (the codebooks are already row-major [bins][C]).  Same rounding as that pair:
// acc = 0.f, acc += row_k for k = 0 .. K - 1 (plain adds in that order: a -0.0f entry comes out as +0.0f), then the split of
// every other S32 producer.  One wave per frame, four frames per workgroup; a lane owns 16 bytes of every 1 KB of the row (NV =
// ceil(C / 256)).  The frame is wave-uniform, so its codes arrive by scalar loads, once per wave; the row loads of KC codebooks
// are all issued before the first add.  A code outside [0, bins): the table is not read for it, the row becomes NaN and one lane
// sets the model's bad-index word (a plain store at system scope, like codes_to_features_kernel); NaN does not reach amax
// (fmaxf), so the call's status stays clean.
template <int NV>
__global__ __launch_bounds__(256) void OPS_K(code_rows)(const int64_t* __restrict__ codes, const float* __restrict__ table,
                                                        float* __restrict__ y, int K, int bins, int B, int OPS_L, int C, int s32,
                                                        unsigned* status, unsigned* bad
#if OPS_MIX
                                                        , const int* __restrict__ lens     // rows t >= lens[clip] are zeros; their codes are never read
#endif
                                                        ) {
    constexpr int KC = NV <= 2 ? 8 : 4;                    // codebooks whose rows are in flight together
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long frames = (long)B * OPS_L;                   // (below 2^31: the launcher)
    if (m >= frames) return;
    float* row = y + m * C;
    float amax = 0.f;
    f32x4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#if OPS_MIX
    const int b = (int)((unsigned)m / (unsigned)Lpad), t = (int)m - b * Lpad;
    if (t >= mix_len(lens, b, Lpad)) {                     // a pad row of the clip: zeros, whatever the staging holds there
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c >= C) continue;
            if (s32) store_s32_4(row, c, acc[i], amax);
            else *reinterpret_cast<f32x4*>(row + c) = acc[i];
        }
        return;
    }
#endif
    const float qnan = __builtin_nanf("");
    bool any_bad = false;
    for (int k0 = 0; k0 < K; k0 += KC) {
        long code[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) code[j] = k0 + j < K ? codes[(k0 + j) * frames + m] : 0;      // [k][b][t]
        f32x4 v[KC][NV];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            if (k0 + j >= K) continue;
            const bool ok = code[j] >= 0 && code[j] < bins;
            any_bad |= !ok;
            const float* src = table + ((long)(k0 + j) * bins + (ok ? code[j] : 0)) * C;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                v[j][i] = (f32x4){qnan, qnan, qnan, qnan};
                if (ok && c < C) v[j][i] = *reinterpret_cast<const f32x4*>(src + c);
            }
        }
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            if (k0 + j >= K) continue;
#pragma unroll
            for (int i = 0; i < NV; ++i) acc[i] += v[j][i];
        }
    }
    if (any_bad && bad && lane == 0) __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c >= C) continue;
        if (s32) store_s32_4(row, c, acc[i], amax);
        else *reinterpret_cast<f32x4*>(row + c) = acc[i];
    }
    range_report(status, amax);
}

// ---------------------------------------------------------------------------- GroupNorm statistics
// decoder/models.py:15-16 Normalize = GroupNorm(32, C, eps=1e-6, affine): per (clip, group) mean and
// biased variance over L x C/32 values, emitted as the per-(clip, channel) scale/shift
//   y = x * (rstd*gamma[c]) + (beta[c] - mean*rstd*gamma[c])
// (consumed by the row-norm pass for pos_net[5]); APPLY > 0 also writes the normalised (and
// swish-activated) tensor once, which the following conv reads as a plain operand.
template <int APPLY>   // 0: scale/shift only; 1: y = x*scale + shift; 2: y = swish(x*scale + shift)
__global__ __launch_bounds__(256) void OPS_K(gn_stats)(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ scale,
                                                       float* __restrict__ shift, float* __restrict__ y, int OPS_L, int C,
                                                       int cg, float eps, int s32, unsigned* status
#if OPS_MIX
                                                       , const int* __restrict__ lens, int lmax
#endif
                                                       ) {
    __shared__ float red[4];
    float amax = 0.f;
    __shared__ float s_mean, s_rstd;
    const int g = blockIdx.x, b = blockIdx.y;
#if OPS_MIX
    const int L = mix_len(lens, b, Lpad);
    if (L > lmax) return;                   // a clip this long takes the chunked form when it is decoded alone: that launch serves it
#endif
    const float* xb = x + (long)b * OPS_L * C + g * cg;
    const int n = L * cg;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float sum = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = i / cg, j = i - t * cg;
        sum += xb[(long)t * C + j];
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) s_mean = (red[0] + red[1] + red[2] + red[3]) / (float)n;
    __syncthreads();
    const float mean = s_mean;
    float sq = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = i / cg, j = i - t * cg;
        const float d = xb[(long)t * C + j] - mean;
        sq += d * d;
    }
    sq = wave_sum(sq);
    __syncthreads();
    if (lane == 0) red[wv] = sq;
    __syncthreads();
    if (threadIdx.x == 0) s_rstd = 1.f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)n + eps);
    __syncthreads();
    if (threadIdx.x < cg) {
        const int c = g * cg + threadIdx.x;
        const float sc = s_rstd * gamma[c];
        scale[(long)b * C + c] = sc;
        shift[(long)b * C + c] = beta[c] - mean * sc;
    }
    if (APPLY) {
        float* yb = y + (long)b * OPS_L * C + g * cg;
        const float rstd = s_rstd;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int t = i / cg, j = i - t * cg;
            const float sc = rstd * gamma[g * cg + j];
            float v = xb[(long)t * C + j] * sc + (beta[g * cg + j] - mean * sc);
            if (APPLY == 2) v = v / (1.f + expf(-v));
            if (s32) store_s32_1(y + ((long)b * OPS_L + t) * C, g * cg + j, v, amax);
            else yb[(long)t * C + j] = v;
        }
        range_report(status, amax);
    }
}

// GroupNorm apply for short sequences: a block owns GB groups (a 384-byte channel slab for C/32 = 24, GB = 4) of one
// clip, pulls the L x (GB*cg) slab into LDS with full-line loads, takes mean and variance from LDS (two-pass, one
// wave per group), and writes the normalised (swish-activated) slab back once, fp32 or S32: one global read and one
// write per element where gn_stats_kernel makes three strided read passes.
template <int SWISH>
__global__ __launch_bounds__(512) void OPS_K(gn_tile)(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ scale,
                                                      float* __restrict__ shift, float* __restrict__ y, int OPS_L, int C,
                                                      int cg, int GB, float eps, int s32, unsigned* status
#if OPS_MIX
                                                      , const int* __restrict__ lens, int lmax
#endif
                                                      ) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [L][W], W = GB * cg
    float amax = 0.f;
    __shared__ float s_sc[128], s_sh[128], s_red[8];
    const int NT = blockDim.x;                             // 256, or 512 for slabs so large that one workgroup fills the CU
    const int W = GB * cg, W4 = W / 4;
    const int c0 = blockIdx.x * W, b = blockIdx.y;
#if OPS_MIX
    const int L = mix_len(lens, b, Lpad);
    if (L > lmax) return;                   // longer than the slab: the chunked launch serves this clip
#endif
    const float* xb = x + (long)b * OPS_L * C + c0;
    // (row, float4) of element e = threadIdx.x + NT k, advanced without divisions
    const int dt = NT / W4, dq = NT - dt * W4;
    {
        int t = threadIdx.x / W4, q = threadIdx.x - t * W4;
        for (; t < L; t += dt, q += dq) {
            if (q >= W4) { q -= W4; ++t; if (t >= L) break; }
            *reinterpret_cast<f32x4*>(tile + t * W + q * 4) = *reinterpret_cast<const f32x4*>(xb + (long)t * C + q * 4);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = NT >> 6;
    if (nw == 2 * GB) {
        // two waves per group, each over half of the rows; the halves meet in LDS in a fixed order
        const int gl = wv >> 1, part = wv & 1;
        const int r0 = part ? L / 2 : 0, r1 = part ? L : L / 2;
        const int n = L * cg;
        const float* col = tile + gl * cg;
        // a lane reads 4 channels of one row per step: 64 / (cg / 4) rows per wave instruction
        const int cg4 = cg >> 2, rp = 64 / cg4, lr = lane / cg4, lq = lane - lr * cg4;
        float sum = 0.f;
        if (lr < rp)
            for (int t = r0 + lr; t < r1; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                sum += (v.x + v.y) + (v.z + v.w);
            }
        sum = wave_sum(sum);
        if (lane == 0) s_red[wv] = sum;
        __syncthreads();
        const float mean = (s_red[2 * gl] + s_red[2 * gl + 1]) / (float)n;
        __syncthreads();
        float sq = 0.f;
        if (lr < rp)
            for (int t = r0 + lr; t < r1; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
                sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        sq = wave_sum(sq);
        if (lane == 0) s_red[wv] = sq;
        __syncthreads();
        const float rstd = 1.f / sqrtf((s_red[2 * gl] + s_red[2 * gl + 1]) / (float)n + eps);
        if (part == 0 && lane < cg) {
            const int c = c0 + gl * cg + lane;
            const float sc = rstd * gamma[c], sh = beta[c] - mean * sc;
            s_sc[gl * cg + lane] = sc; s_sh[gl * cg + lane] = sh;
            scale[(long)b * C + c] = sc; shift[(long)b * C + c] = sh;
        }
    } else
    for (int gl = wv; gl < GB; gl += nw) {                 // one wave per group
        const int n = L * cg;
        const float* col = tile + gl * cg;
        const int cg4 = cg >> 2, rp = 64 / cg4, lr = lane / cg4, lq = lane - lr * cg4;
        float sum = 0.f;
        if (lr < rp)
            for (int t = lr; t < L; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                sum += (v.x + v.y) + (v.z + v.w);
            }
        const float mean = wave_sum(sum) / (float)n;
        float sq = 0.f;
        if (lr < rp)
            for (int t = lr; t < L; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
                sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)n + eps);
        if (lane < cg) {
            const int c = c0 + gl * cg + lane;
            const float sc = rstd * gamma[c], sh = beta[c] - mean * sc;
            s_sc[gl * cg + lane] = sc; s_sh[gl * cg + lane] = sh;
            scale[(long)b * C + c] = sc; shift[(long)b * C + c] = sh;
        }
    }
    __syncthreads();
    float* yb = y + (long)b * OPS_L * C;
#if OPS_MIX
    for (int e = threadIdx.x; e < (Lpad - L) * W4; e += NT) {      // rows [L, Lpad) of the output are zeros
        const int tz = e / W4, q = e - tz * W4;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (s32) store_s32_4(yb + (long)(L + tz) * C, c0 + q * 4, z, amax);
        else *reinterpret_cast<f32x4*>(yb + (long)(L + tz) * C + c0 + q * 4) = z;
    }
#endif
    {
        int t = threadIdx.x / W4, q = threadIdx.x - t * W4;
        for (; t < L; t += dt, q += dq) {
            if (q >= W4) { q -= W4; ++t; if (t >= L) break; }
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + t * W + q * 4);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(s_sc + q * 4), sh = *reinterpret_cast<const f32x4*>(s_sh + q * 4);
            f32x4 o = v * sc + sh;
            if (SWISH) {     // x * sigmoid(x) on the hardware exp / rcp (relative error ~1e-7)
                o.x *= __builtin_amdgcn_rcpf(1.f + __expf(-o.x)); o.y *= __builtin_amdgcn_rcpf(1.f + __expf(-o.y));
                o.z *= __builtin_amdgcn_rcpf(1.f + __expf(-o.z)); o.w *= __builtin_amdgcn_rcpf(1.f + __expf(-o.w));
            }
            if (s32) store_s32_4(yb + (long)t * C, c0 + q * 4, o, amax);
            else *reinterpret_cast<f32x4*>(yb + (long)t * C + c0 + q * 4) = o;
        }
    }
    range_report(status, amax);
}

// GroupNorm for sequences too long for one LDS slab (30 s clips: L = 1200): the L x 96-channel slab is cut into chunks of
// GN_CH rows.  Pass 1: every (slab, chunk) workgroup pulls its chunk into LDS and leaves, per group, the chunk mean and
// the sum of squared deviations about it.  Pass 2: every workgroup merges the chunk statistics of its groups in chunk
// order (Chan's pairwise update: deterministic, no atomics) and normalises its own chunk straight from global memory.
// Two coalesced reads and one write per element where gn_stats_kernel makes three strided reads.

__global__ __launch_bounds__(256) void OPS_K(gn_chunk_stats)(const float* __restrict__ x, float* __restrict__ part, int OPS_L,
                                                             int C, int cg, int GB, int groups, int nch
#if OPS_MIX
                                                             , const int* __restrict__ lens, int lmin
#endif
                                                             ) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [rows][W]
    const int W = GB * cg, W4 = W / 4;
    const int c0 = blockIdx.x * W, k = blockIdx.y, b = blockIdx.z;
#if OPS_MIX
    const int L = mix_len(lens, b, Lpad);
    if (L <= lmin || k * GN_CH >= L) return;     // a slab-form clip, or a chunk past the clip's own (nch is the padded count)
#endif
    const int t0 = k * GN_CH, rows = L - t0 < GN_CH ? L - t0 : GN_CH;
    const float* xb = x + ((long)b * OPS_L + t0) * C + c0;
    for (int e = threadIdx.x; e < rows * W4; e += 256) {
        const int t = e / W4, q = e - t * W4;
        *reinterpret_cast<f32x4*>(tile + t * W + q * 4) = *reinterpret_cast<const f32x4*>(xb + (long)t * C + q * 4);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int gl = wv; gl < GB; gl += 4) {
        const float* col = tile + gl * cg;
        const int cg4 = cg >> 2, rp = 64 / cg4, lr = lane / cg4, lq = lane - lr * cg4;
        float sum = 0.f;
        if (lr < rp)
            for (int t = lr; t < rows; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                sum += (v.x + v.y) + (v.z + v.w);
            }
        const float mean = wave_sum(sum) / (float)(rows * cg);
        float sq = 0.f;
        if (lr < rp)
            for (int t = lr; t < rows; t += rp) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(col + t * W + lq * 4);
                const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
                sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        sq = wave_sum(sq);
        if (lane == 0) {
            float* o = part + (((long)b * groups + blockIdx.x * GB + gl) * nch + k) * 2;
            o[0] = mean; o[1] = sq;
        }
    }
}

template <int APPLY>   // 0: scale/shift only; 1: y = x*scale + shift; 2: y = swish(x*scale + shift)
__global__ __launch_bounds__(256) void OPS_K(gn_chunk_apply)(const float* __restrict__ x, const float* __restrict__ part,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ scale, float* __restrict__ shift,
                                                             float* __restrict__ y, int OPS_L, int C, int cg, int GB, int groups,
                                                             int nch, float eps, int s32, unsigned* status
#if OPS_MIX
                                                             , const int* __restrict__ lens, int lmin
#endif
                                                             ) {
    __shared__ float s_mean[8], s_rstd[8], s_sc[128], s_sh[128];
    float amax = 0.f;
    const int W = GB * cg, W4 = W / 4;
    const int c0 = blockIdx.x * W, k = blockIdx.y, b = blockIdx.z;
#if OPS_MIX
    const int L = mix_len(lens, b, Lpad);
    if (L <= lmin) return;                  // a slab-form clip: gn_tile (gn_stats) serves it, pad rows included
    const int nch_own = (L + GN_CH - 1) / GN_CH;      // the clip's own chunks are merged, in the order of its solo call
#define OPS_NCH nch_own
#else
#define OPS_NCH nch
#endif
    if (threadIdx.x < GB) {
        const float* pp = part + ((long)b * groups + blockIdx.x * GB + threadIdx.x) * nch * 2;
        float n = 0.f, mean = 0.f, m2 = 0.f;
        for (int q = 0; q < OPS_NCH; ++q) {
            const int rows = L - q * GN_CH < GN_CH ? L - q * GN_CH : GN_CH;
            const float nq = (float)(rows * cg), d = pp[2 * q] - mean, tot = n + nq;
            mean += d * (nq / tot);
            m2 += pp[2 * q + 1] + d * d * (n * nq / tot);
            n = tot;
        }
        s_mean[threadIdx.x] = mean;
        s_rstd[threadIdx.x] = 1.f / sqrtf(m2 / n + eps);
    }
    __syncthreads();
    if (threadIdx.x < W) {
        const int c = c0 + threadIdx.x, gl = threadIdx.x / cg;
        const float sc = s_rstd[gl] * gamma[c], sh = beta[c] - s_mean[gl] * sc;
        s_sc[threadIdx.x] = sc; s_sh[threadIdx.x] = sh;
        if (k == 0) { scale[(long)b * C + c] = sc; shift[(long)b * C + c] = sh; }
    }
    if (APPLY == 0) return;
    __syncthreads();
    const int t0 = k * GN_CH, rows = L - t0 < GN_CH ? L - t0 : GN_CH;
    const float* xb = x + ((long)b * OPS_L + t0) * C + c0;
    float* yb = y + ((long)b * OPS_L + t0) * C;
    for (int e = threadIdx.x; e < rows * W4; e += 256) {
        const int t = e / W4, q = e - t * W4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (long)t * C + q * 4);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(s_sc + q * 4), sh = *reinterpret_cast<const f32x4*>(s_sh + q * 4);
        f32x4 o = v * sc + sh;
        if (APPLY == 2) {
            o.x *= __builtin_amdgcn_rcpf(1.f + __expf(-o.x)); o.y *= __builtin_amdgcn_rcpf(1.f + __expf(-o.y));
            o.z *= __builtin_amdgcn_rcpf(1.f + __expf(-o.z)); o.w *= __builtin_amdgcn_rcpf(1.f + __expf(-o.w));
        }
        if (s32) store_s32_4(yb + (long)t * C, c0 + q * 4, o, amax);
        else *reinterpret_cast<f32x4*>(yb + (long)t * C + c0 + q * 4) = o;
    }
#if OPS_MIX
    {   // rows of this chunk in [L, Lpad) are zeros
        const int rz0 = rows > 0 ? rows : 0, rz1 = Lpad - t0 < GN_CH ? Lpad - t0 : GN_CH;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int e = threadIdx.x + rz0 * W4; e < rz1 * W4; e += 256) {
            const int t = e / W4, q = e - t * W4;
            if (s32) store_s32_4(yb + (long)t * C, c0 + q * 4, z, amax);
            else *reinterpret_cast<f32x4*>(yb + (long)t * C + c0 + q * 4) = z;
        }
    }
#endif
#undef OPS_NCH
    range_report(status, amax);
}

// RN_DWCONV with each wave producing R consecutive frames of one clip: the R + 6 input rows and the 7 tap rows are
// loaded once per 256-channel slice instead of once per output frame (7 row loads + 7 tap loads per frame before).
// Same accumulation order per output as rownorm_kernel, so the results are identical.
template <int NV, int R>
__global__ __launch_bounds__(256) void OPS_K(dwconv_ln)(const float* __restrict__ x, float* __restrict__ y, int B, int OPS_L,
                                                        const float* __restrict__ dw_w, const float* __restrict__ dw_b,
                                                        const float* __restrict__ out_scale,
                                                        const float* __restrict__ out_shift, float eps, int s32, unsigned* status
#if OPS_MIX
                                                        , const int* __restrict__ lens     // taps and rows at or past lens[clip] are absent
#endif
                                                        ) {
    constexpr int C = NV * 256;
    const int lane = threadIdx.x & 63;
    float amax = 0.f;
    const int per_clip = (OPS_L + R - 1) / R;
    const long wq = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wq >= (long)B * per_clip) return;
    const int b = (int)(wq / per_clip);
    const int t0 = (int)(wq - (long)b * per_clip) * R;
#if OPS_MIX
    const int L = mix_len(lens, b, Lpad);
#endif
    const float* xb = x + (long)b * OPS_L * C;
    f32x4 v[R][NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        f32x4 xr[R + 6], w[7];
#pragma unroll
        for (int k = 0; k < R + 6; ++k) {
            const int tt = t0 + k - 3;
            xr[k] = (tt >= 0 && tt < L) ? *reinterpret_cast<const f32x4*>(xb + (long)tt * C + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) w[j] = *reinterpret_cast<const f32x4*>(dw_w + j * C + c);
        const f32x4 bias = *reinterpret_cast<const f32x4*>(dw_b + c);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            f32x4 acc = bias;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int tt = t0 + r + j - 3;
                if (tt >= 0 && tt < L) acc += xr[r + j] * w[j];
            }
            v[r][i] = acc;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#if OPS_MIX
        if (t0 + r >= Lpad) break;
        if (t0 + r >= L) {                  // a pad row of the clip: zeros
            float* zrow = y + ((long)b * Lpad + t0 + r) * C;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (s32) store_s32_4(zrow, c, z, amax);
                else *reinterpret_cast<f32x4*>(zrow + c) = z;
            }
            continue;
        }
#else
        if (t0 + r >= L) break;
#endif
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) sum += (v[r][i].x + v[r][i].y) + (v[r][i].z + v[r][i].w);
        const float mean = wave_sum(sum) * (1.f / C);
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 d = v[r][i] - mean;
            sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
        const float rstd = 1.f / sqrtf(wave_sum(sq) * (1.f / C) + eps);
        float* yrow = y + ((long)b * OPS_L + t0 + r) * C;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            const f32x4 os = *reinterpret_cast<const f32x4*>(out_scale + c);
            const f32x4 oh = *reinterpret_cast<const f32x4*>(out_shift + c);
            const f32x4 o = ((v[r][i] - mean) * rstd) * os + oh;
            if (s32) store_s32_4(yrow, c, o, amax);
            else *reinterpret_cast<f32x4*>(yrow + c) = o;
        }
    }
    range_report(status, amax);
}

// -------------------------------------------------------------------------------------- softmax
// AttnBlock softmax over keys (decoder/models.py:119); one wave per query row; pad columns
// [L, ld) are zero-filled so the P.V contraction can run over the padded length.
__global__ __launch_bounds__(256) void OPS_K(softmax)(float* __restrict__ S, long rows, int OPS_L, int ld, float* __restrict__ P_s32
#if OPS_MIX
                                                      , const int* __restrict__ lens     // Lpad query rows per clip; keys at or past lens[clip] are masked
#endif
                                                      ) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
#if OPS_MIX
    const int L = mix_len(lens, (int)(r / Lpad), Lpad);
#endif
    float* row = S + r * ld;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, row[j]);
    mx = wave_max(mx);
    // a lane owns columns 4 (lane + 64 i) + e, i ascending, like softmax_reg_kernel: the same partial sums in the same order
    float sum = 0.f;
    for (int j0 = 4 * lane; j0 < L; j0 += 256)
        for (int j = j0; j < j0 + 4 && j < L; ++j) {
            const float e = expf(row[j] - mx);
            row[j] = e;
            sum += e;
        }
    sum = wave_sum(sum);
    if (P_s32) {        // probabilities for a split-f16 GEMM: S32 rows in a separate buffer (pad columns zero)
        float unused = 0.f;                                      // probabilities never leave [0, 1]
        for (int j0 = 4 * lane; j0 < ld; j0 += 256)
            for (int j = j0; j < j0 + 4 && j < ld; ++j) store_s32_1(P_s32 + r * ld, j, j < L ? row[j] / sum : 0.f, unused);
    } else {
        for (int j0 = 4 * lane; j0 < ld; j0 += 256)
            for (int j = j0; j < j0 + 4 && j < ld; ++j) row[j] = j < L ? row[j] / sum : 0.f;
    }
}

// The same with the row held in registers (NV4 float4 per lane, row pitch <= 256 * NV4): the scores are read ONCE with
// 16-byte loads and the probabilities written once (S32: 8 + 8 bytes per four values), instead of read / write-back of the
// exponentials / read / 2-byte stores (30 s clips: 737 MB -> 368 MB per launch).  Same arithmetic per element (max, exp(x - max),
// sum in the same lane order, division by the sum).
template <int NV4>
__global__ __launch_bounds__(256) void OPS_K(softmax_reg)(float* __restrict__ S, long rows, int OPS_L, int ld, float* __restrict__ P_s32
#if OPS_MIX
                                                      , const int* __restrict__ lens     // Lpad query rows per clip; keys at or past lens[clip] are masked
#endif
                                                      ) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
#if OPS_MIX
    const int L = mix_len(lens, (int)(r / Lpad), Lpad);
#endif
    const f32x4* row4 = reinterpret_cast<const f32x4*>(S + r * ld);
    f32x4 v[NV4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const int j = 4 * (lane + 64 * i);
        v[i] = j < ld ? row4[lane + 64 * i] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j + e >= L) v[i][e] = -INFINITY;
            mx = fmaxf(mx, v[i][e]);
        }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ex = 4 * (lane + 64 * i) + e < L ? expf(v[i][e] - mx) : 0.f;
            v[i][e] = ex;
            sum += ex;
        }
    sum = wave_sum(sum);
    float unused = 0.f;                                          // probabilities never leave [0, 1]
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const int j = 4 * (lane + 64 * i);
        if (j >= ld) continue;
        f32x4 p;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = j + e < L ? v[i][e] / sum : 0.f;
        if (P_s32) store_s32_4(P_s32 + r * ld, j, p, unused);
        else *reinterpret_cast<f32x4*>(S + r * ld + j) = p;
    }
}

// ------------------------------------------------------------------------------- ISTFT tail
// ISTFT.forward (decoder/spectral_ops.py:33-75) after the four quarter transforms
// Ce, Co, Se, So [frame][0..N/4]: rebuild x_t[n] with the two radix-2 butterflies, multiply by the
// window, overlap-add the n_fft/hop frames that cover an output sample (ascending n, like fold),
// trim and divide by the window-square envelope.  One thread per output sample.
// "same" (:46, 56-73): trim (n_fft - hop) / 2 at both ends, L * hop samples.  "center" (:43-45, torch.istft(center=True)):
// trim n_fft / 2 at both ends, (L - 1) * hop samples; the same overlap-add and the same envelope otherwise.
__global__ __launch_bounds__(256) void OPS_K(istft_ola)(const float* __restrict__ parts, const float* __restrict__ win,
                                                        const float* __restrict__ wsq, float* __restrict__ out,
                                                        long total, long Mrows, int OPS_L, int N, int hop, int Kq, int pad, long Tout
#if OPS_MIX
                                                        , const int* __restrict__ lens, int center
#endif
                                                        ) {
    const int R = N / hop, Q = N / 4, Nh = N / 2;
    const float* Ce = parts;
    const float* Co = parts + Mrows * Kq;
    const float* Se = parts + 2 * Mrows * Kq;
    const float* So = parts + 3 * Mrows * Kq;
    // Workgroup i runs on XCD i % 8 and every spectrum value is read by four output samples up to n_fft apart: with the
    // chunks of 256 samples dealt out round robin each XCD's L2 fetched (nearly) all of `parts` for itself (301 MB of traffic
    // for 93 MB, profiles/r03_pmc_traffic.json).  XCD x takes the x-th contiguous eighth of the chunks instead
    const long nchunk = (long)gridDim.x;                     // a multiple of 8 (host), one chunk per workgroup
    const long chunk = (long)(blockIdx.x & 7) * (nchunk >> 3) + (blockIdx.x >> 3);
    for (long idx = chunk * blockDim.x + threadIdx.x; idx < total; idx += total) {       // (one pass)
        const long b = idx / Tout;
        const long u = idx - b * Tout;
#if OPS_MIX
        // frames at or past the clip's own length are absent; samples past its own waveform are zeros
        const int L = mix_len(lens, (int)b, Lpad);
        if (u >= (center ? (long)hop * (L - 1) : (long)hop * L)) { out[idx] = 0.f; continue; }
#endif
        const long up = u + pad;
        const int jp = (int)(up / hop), r = (int)(up - (long)jp * hop);
        float acc = 0.f, env = 0.f;
        for (int d = 0; d < R; ++d) {
            const int t = jp - d;
            if (t < 0 || t >= L) continue;
            const int n = r + hop * d;
            const int m = n <= Nh ? n : N - n;               // x[N-m] = C[m] + S[m]
            const int mm = m <= Q ? m : Nh - m;              // C[N/2-mm] = Ce - Co, S[N/2-mm] = So - Se
            const long o = (b * OPS_L + t) * Kq + mm;
            const float ce = Ce[o], co = Co[o], se = Se[o], so = So[o];
            const float Cv = m <= Q ? ce + co : ce - co;
            const float Sv = m <= Q ? se + so : so - se;
            const float x = n <= Nh ? Cv - Sv : Cv + Sv;
            acc += x * win[n];
            env += wsq[n];
        }
        out[idx] = acc / env;
    }
}
