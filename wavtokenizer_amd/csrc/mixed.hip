// Mixed-length encode plans (WT_PLAN_FLAG_MIXED_LENGTH): the geometry table that the plan's first step builds from the caller's
// clip lengths, and the padding rule of the outputs that its last compute step applies.  The layout of the table is in common.h
// (GEOM_*); its arithmetic is sconv_geom, the function the host planner uses for plans of one length.
#include "common.h"

namespace wt {

struct MixChain {
    long Tpad;                       // the plan's (padded) length
    int tmin;                        // the shortest clip the plan's route takes
    int n_st;                        // encoder stages
    int k3[GEOM_MAX_STAGES], ksc[GEOM_MAX_STAGES], kd[GEOM_MAX_STAGES], rd[GEOM_MAX_STAGES];
    int kf;                          // final conv
};

// one thread per clip: every conv's {T_in, Tp, T_out} through the encoder, as build_encode derives them for a plan of that length
__global__ __launch_bounds__(64) void mixed_geometry_kernel(const int* __restrict__ lengths, int* __restrict__ geom, int B,
                                                            const MixChain ch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int T = lengths[b];
    const bool valid = T >= ch.tmin && (long)T <= ch.Tpad;
    int* g = geom + (long)b * GEOM_WORDS;
    for (int i = 0; i < GEOM_WORDS; ++i) g[i] = 0;
    long Tc = valid ? T : ch.tmin;
    g[GEOM_VALID] = valid ? 1 : 0;
    g[GEOM_T] = (int)Tc;
    g[GEOM_TREAD] = valid ? (int)Tc : 0;
    for (int s = 0; s < ch.n_st; ++s) {
        int* w = g + GEOM_STAGE0 + s * GEOM_STAGE_WORDS;
        const SConvGeom c3 = sconv_geom(Tc, ch.k3[s], 1, 1), sc = sconv_geom(Tc, ch.ksc[s], 1, 1), d = sconv_geom(Tc, ch.kd[s], ch.rd[s], 1);
        w[GEOM_C3] = (int)Tc; w[GEOM_C3 + 1] = c3.Tp; w[GEOM_C3 + 2] = c3.Tout;
        w[GEOM_SC] = (int)Tc; w[GEOM_SC + 1] = sc.Tp; w[GEOM_SC + 2] = sc.Tout;
        w[GEOM_DOWN] = (int)Tc; w[GEOM_DOWN + 1] = d.Tp; w[GEOM_DOWN + 2] = d.Tout;
        Tc = d.Tout;
    }
    int* f = g + GEOM_STAGE0 + ch.n_st * GEOM_STAGE_WORDS;
    const SConvGeom fg = sconv_geom(Tc, ch.kf, 1, 1);
    f[0] = (int)Tc; f[1] = fg.Tp; f[2] = fg.Tout;
    f[3] = (int)Tc;                  // L
}

int launch_mixed_geometry(const int* lengths, int* geom, int B, long Tpad, int tmin, int n_st, const int* kd, const int* rd,
                          int kf, hipStream_t s) {
    if (!lengths) { set_error("mixed-length encode: no clip lengths"); return -1; }
    if (n_st < 1 || n_st > GEOM_MAX_STAGES) { set_error("mixed-length encode: unsupported number of encoder stages"); return -1; }
    MixChain ch{};
    ch.Tpad = Tpad; ch.tmin = tmin; ch.n_st = n_st; ch.kf = kf;
    for (int i = 0; i < n_st; ++i) { ch.k3[i] = 3; ch.ksc[i] = 1; ch.kd[i] = kd[i]; ch.rd[i] = rd[i]; }
    hipLaunchKernelGGL(mixed_geometry_kernel, dim3((B + 63) / 64), dim3(64), 0, s, lengths, geom, B, ch);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

// grid (D, B): block (d, b) writes channel d of clip b from the clip's first padded frame on (frame 0 for an invalid clip);
// channel 0's block also writes the codes
__global__ __launch_bounds__(256) void mixed_pad_kernel(const int* __restrict__ geom, int l_word, int64_t* __restrict__ codes,
                                                        float* __restrict__ feat, float* __restrict__ emb, int L, int D) {
    const int d = blockIdx.x, b = blockIdx.y;
    const int* g = geom + (long)b * GEOM_WORDS;
    const bool valid = g[GEOM_VALID] != 0;
    const int t0 = valid ? g[l_word] : 0;
    if (t0 >= L) return;
    const float fill = valid ? 0.f : __builtin_nanf("");
    const long row = ((long)b * D + d) * L;
    for (int t = t0 + (int)threadIdx.x; t < L; t += blockDim.x) {
        if (feat) feat[row + t] = fill;
        if (emb) emb[row + t] = fill;
        if (d == 0) codes[(long)b * L + t] = -1;
    }
}

int launch_mixed_pad(const int* geom, int l_word, int64_t* codes, float* feat_ncl, float* emb_ncl, int B, int L, int D,
                     hipStream_t s) {
    hipLaunchKernelGGL(mixed_pad_kernel, dim3(D, B), dim3(256), 0, s, geom, l_word, codes, feat_ncl, emb_ncl, L, D);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(64) void mixed_check_lengths_kernel(const int* __restrict__ lengths, int B, int Lpad, unsigned* status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int l = lengths[b];
    if (l < 1 || l > Lpad) __hip_atomic_fetch_or(status, (unsigned)WT_STATUS_LENGTH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int launch_mixed_check_lengths(const int* lengths, int B, int Lpad, unsigned* status, hipStream_t s) {
    if (!lengths || !status) { set_error("mixed-length decode: no clip lengths"); return -1; }
    hipLaunchKernelGGL(mixed_check_lengths_kernel, dim3((B + 63) / 64), dim3(64), 0, s, lengths, B, Lpad, status);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace wt
