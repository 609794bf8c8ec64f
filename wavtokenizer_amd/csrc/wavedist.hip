// The two time-domain measures of a codec evaluation on the GPU: the scale-invariant signal-to-distortion ratio (Le Roux, Wisdom,
// Erdogan & Hershey 2019) and the plain signal-to-noise ratio, both in dB.  include/wavtokenizer_amd.h states the definition;
// torchmetrics is not available to this project's tests, so the parity with it is unpinned: tests/wavedist_ref.py holds the
// definition in float64 and the kernels are checked against that.
//
// Up to three passes over a pair in blocks of WD_BLOCK samples, each followed by a per-clip reduction of the blocks' partials:
//   pass 0 (zero_mean only)   sum p, sum t                          -> the means
//   pass 1                    sum p' t', sum t'^2                    -> alpha = (sum p' t' + eps) / (sum t'^2 + eps)
//   pass 2                    sum (t' - p')^2, sum (alpha t' - p')^2, sum (alpha t')^2   -> the two ratios
// with p' = p - mean p, t' = t - mean t (the means are 0 without zero_mean).  The residual energies are formed sample by sample and
// never from the moments: in fp32 the expanded form loses the measure above 60 dB.  fp32 throughout, no atomics; the block size and
// the order of every sum depend on T alone: a pair has the same bits alone, in any batch and at any position.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

// sums must not depend on the kernel a device function is inlined into: no contraction by the compiler, fmaf where wanted
// (over fft.h's functions too: the pragma stands before the include)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int WD_BLOCK = 2048;                  // samples per workgroup of a pass: thread t takes samples t, t + 256, ... of the block
constexpr int WD_THREADS = 256;
constexpr int WD_STATE = 4;                     // floats per clip between the passes: mean p, mean t, alpha, sum t'^2
constexpr int WD_ARG_CLIPS = 64;                // descriptors up to this many travel in the launches' argument blocks (ragged.h)
constexpr float WD_EPS = 1.1920928955078125e-07f;            // 2^-23

// One pair of a call (device form of wt_wavedist_clip)
struct WdClip {
    const float* p;                             // the estimate
    const float* t;                             // the target
    float* out;                                 // [2]: SI-SDR, SNR
    long T;
    long part;                                  // the clip's first block among the per-block partials in the workspace
};

// grid (ceil(max T / WD_BLOCK), B): block (x, b) adds samples [WD_BLOCK x, WD_BLOCK (x + 1)) of pair b: the thread its own samples in
// ascending order, the xor butterfly over the wave, the four waves as (0 + 1) + (2 + 3): three partials per block
template <int PASS> __device__ __forceinline__ void wd_sum_block(const WdClip& c, int clip, int centre, const float* state, float* part) {
    __shared__ float ws[WD_THREADS / 64][3];
    const long s0 = (long)blockIdx.x * WD_BLOCK;
    if (s0 >= c.T) return;                                      // (the whole block: no barrier is left waiting)
    const global_ptr<const float> P = (global_ptr<const float>)c.p, Tg = (global_ptr<const float>)c.t;
    const global_ptr<const float> st = (global_ptr<const float>)state + (long)WD_STATE * clip;
    const float mp = PASS > 0 && centre ? st[0] : 0.f, mt = PASS > 0 && centre ? st[1] : 0.f;
    const float alpha = PASS == 2 ? st[2] : 0.f;
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < WD_BLOCK / WD_THREADS; ++i) {
        const long n = s0 + threadIdx.x + WD_THREADS * i;
        if (n < c.T) {
            if (PASS == 0) {
                s[0] += P[n];
                s[1] += Tg[n];
            } else {
                const float p = P[n] - mp, t = Tg[n] - mt;
                if (PASS == 1) {
                    s[0] = fmaf(p, t, s[0]);
                    s[1] = fmaf(t, t, s[1]);
                } else {
                    const float e = t - p, at = alpha * t, r = at - p;
                    s[0] = fmaf(e, e, s[0]);
                    s[1] = fmaf(r, r, s[1]);
                    s[2] = fmaf(at, at, s[2]);
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s[j] = wave_sum(s[j]);
        if (lane == 0) ws[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int j = threadIdx.x;
        ((global_ptr<float>)part)[3 * (c.part + blockIdx.x) + j] = (ws[0][j] + ws[1][j]) + (ws[2][j] + ws[3][j]);
    }
}

// One wave per pair: lane l adds the partials of blocks l, l + 64, ... in ascending order, the xor butterfly adds the lanes
template <int PASS> __device__ __forceinline__ void wd_reduce_block(const WdClip& c, int clip, float* state, const float* part) {
    const int lane = threadIdx.x;
    const long nb = (c.T + WD_BLOCK - 1) / WD_BLOCK;
    const global_ptr<const float> q = (global_ptr<const float>)part + 3 * c.part;
    float s[3] = {0.f, 0.f, 0.f};
    for (long i = lane; i < nb; i += 64) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += q[3 * i + j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = wave_sum(s[j]);
    if (lane != 0) return;
    const global_ptr<float> st = (global_ptr<float>)state + (long)WD_STATE * clip;
    if (PASS == 0) {
        st[0] = s[0] / (float)c.T;
        st[1] = s[1] / (float)c.T;
    } else if (PASS == 1) {
        st[2] = (s[0] + WD_EPS) / (s[1] + WD_EPS);
        st[3] = s[1];
    } else {
        const global_ptr<float> out = (global_ptr<float>)c.out;
        out[0] = 10.f * log10f((s[2] + WD_EPS) / (s[1] + WD_EPS));
        out[1] = 10.f * log10f((st[3] + WD_EPS) / (s[0] + WD_EPS));
    }
}

template <int PASS, class D> __global__ __launch_bounds__(WD_THREADS) void wd_sum_kernel(const D d, int centre, const float* state,
                                                                                         float* part) {
    wd_sum_block<PASS>(d.clip[blockIdx.y], blockIdx.y, centre, state, part);
}
template <int PASS, class D> __global__ __launch_bounds__(64) void wd_reduce_kernel(const D d, float* state, const float* part) {
    wd_reduce_block<PASS>(d.clip[blockIdx.x], blockIdx.x, state, part);
}

static size_t wd_desc_bytes(int B) { return ((size_t)B * sizeof(WdClip) + 15) / 16 * 16; }

}  // namespace wt

using namespace wt;

extern "C" {

size_t wt_wavedist_workspace_bytes(int32_t B, int64_t total_samples) {
    if (B < 1 || total_samples < 0) return 0;
    // descriptors | state [B][4] | partials [3] per block: a clip of T samples has ceil(T / WD_BLOCK) <= T / WD_BLOCK + 1 blocks
    return wd_desc_bytes(B) + (size_t)B * WD_STATE * sizeof(float) + ((size_t)(total_samples / WD_BLOCK) + (size_t)B) * 3 * sizeof(float);
}

int32_t wt_wavedist_block(void) { return WD_BLOCK; }

int wt_wavedist(const wt_wavedist_clip* clips, int32_t B, int32_t zero_mean, void* workspace, void* stream) {
    const std::string fn = "wt_wavedist";
    if (!ragged_call_ok(fn, &fn, clips, workspace, B, 65535)) return WT_ERR_INVALID;          // (there is no handle to be null)
    std::vector<WdClip> dev((size_t)B);
    int64_t max_blocks = 0, total = 0;
    for (int b = 0; b < B; ++b) {
        const wt_wavedist_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.estimate) { set_error(who + "null estimate"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null out"); return WT_ERR_INVALID; }
        if (!c.target) { set_error(who + "null target"); return WT_ERR_INVALID; }
        if (c.length < 1) { set_error(who + "length < 1"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.estimate) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float) ||
            reinterpret_cast<uintptr_t>(c.target) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        const int64_t nb = (c.length + WD_BLOCK - 1) / WD_BLOCK;
        dev[b] = WdClip{c.estimate, c.target, c.out, (long)c.length, (long)total};
        max_blocks = std::max(max_blocks, nb);
        total += nb;
    }
    if (max_blocks > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* state = reinterpret_cast<float*>(static_cast<char*>(workspace) + wd_desc_bytes(B));
    float* part = state + (size_t)B * WD_STATE;
    const dim3 grid((unsigned)max_blocks, (unsigned)B), one((unsigned)B);
    const int centre = zero_mean ? 1 : 0;
    if (int rc = launch_ragged<WD_ARG_CLIPS>("wt_wavedist", dev.data(), B, 128, workspace, s, [&](auto d) {
        using D = decltype(d);
        if (centre) {
            hipLaunchKernelGGL((wd_sum_kernel<0, D>), grid, dim3(WD_THREADS), 0, s, d, centre, state, part);
            hipLaunchKernelGGL((wd_reduce_kernel<0, D>), one, dim3(64), 0, s, d, state, part);
        }
        hipLaunchKernelGGL((wd_sum_kernel<1, D>), grid, dim3(WD_THREADS), 0, s, d, centre, state, part);
        hipLaunchKernelGGL((wd_reduce_kernel<1, D>), one, dim3(64), 0, s, d, state, part);
        hipLaunchKernelGGL((wd_sum_kernel<2, D>), grid, dim3(WD_THREADS), 0, s, d, centre, state, part);
        hipLaunchKernelGGL((wd_reduce_kernel<2, D>), one, dim3(64), 0, s, d, state, part);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // extern "C"
