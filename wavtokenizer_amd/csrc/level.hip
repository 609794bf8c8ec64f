// Per-clip level control on either side of the codec: the measurement (peak and rms of ragged clips), the normalisation of the
// rows of an ingest output (extract_features.py:27-28, EncodecModel._encode_frame, encoder/model.py:153-156) and the scaling of
// decoded segment rows (EncodecModel._decode_frame, encoder/model.py:180-191).  include/wavtokenizer_amd.h states the definitions.
//
// The sum of squares of a clip of n samples is a perfect binary tree over chunks of LEVEL_CHUNK samples, leaves past n being
// zeros (adding them is exact: squares are not negative):
//   a chunk is one workgroup: thread t holds samples 4 t + e + 1024 j (e < 4, j < 4), adds its rounded squares as
//   ((e0 + e1) + (e2 + e3)) per j and ((j0 + j1) + (j2 + j3)), then the xor butterfly over the wave, then the four waves as
//   (0 + 1) + (2 + 3);
//   the chunks' partials are added by ONE workgroup per clip: while more than 256 are left, neighbours are added pairwise
//   (partial 2 i + partial 2 i + 1, ping-pong between two arrays of the workspace), then the butterfly and the waves as above.
// Shape and order depend on n alone, nothing is added by an atomic: a clip has the same bits alone, at any position of any batch
// and whatever the grid.  The peak is a maximum: exact in any order.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

// (sums must not depend on the kernel a device function is inlined into: no contraction by the compiler)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int LEVEL_CHUNK = 4096;               // samples per workgroup of the measurement
constexpr int LEVEL_THREADS = 256;
constexpr int LEVEL_ARG_CLIPS = 64;             // descriptors up to this many travel in the launches' argument blocks (ragged.h)
constexpr int LEVEL_SPAN = 1024;                // samples per workgroup of the two gain kernels: four per thread

typedef float lv_f32x4 __attribute__((ext_vector_type(4)));

// One clip of a call (device form of wt_level_clip)
struct LevelClip {
    const float* x;
    long n;
    float* out;                                 // [2]: peak, rms
    long part;                                  // the clip's first chunk among the per-chunk partials in the workspace
};

// the block's four wave values (lane 0 of each) as (0 + 1) + (2 + 3) and their maximum, in thread 0
__device__ __forceinline__ void level_block_tail(float s, float m, float& sum, float& peak) {
    __shared__ float ws[LEVEL_THREADS / 64][2];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        s = s + __shfl_xor(s, off, 64);
        m = fmaxf(m, __shfl_xor(m, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6][0] = s; ws[threadIdx.x >> 6][1] = m; }
    __syncthreads();
    sum = (ws[0][0] + ws[1][0]) + (ws[2][0] + ws[3][0]);
    peak = fmaxf(fmaxf(ws[0][1], ws[1][1]), fmaxf(ws[2][1], ws[3][1]));
}

// grid (ceil(max n / LEVEL_CHUNK), B): block (c, b) measures chunk c of clip b into peaks[part + c], sums[part + c]
template <class D> __global__ __launch_bounds__(LEVEL_THREADS) void level_chunk_kernel(const D d, float* __restrict__ peaks,
                                                                                    float* __restrict__ sums) {
    const LevelClip c = d.clip[blockIdx.y];
    const long s0 = (long)blockIdx.x * LEVEL_CHUNK;
    if (s0 >= c.n) return;                                      // (the whole block: no barrier is left waiting)
    const global_ptr<const float> x = (global_ptr<const float>)c.x;
    const bool wide = (uintptr_t)c.x % 16 == 0;                 // (a chunk starts 16 KiB behind the last: one answer per clip)
    float q[4];
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = s0 + 1024 * j + 4 * (long)threadIdx.x;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (i + 4 <= c.n && wide) {
            const lv_f32x4 w = *(global_ptr<const lv_f32x4>)(x + i);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (i + e < c.n) v[e] = x[i + e];
        }
        m = fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        q[j] = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    float sum, peak;
    level_block_tail((q[0] + q[1]) + (q[2] + q[3]), m, sum, peak);
    if (threadIdx.x == 0) {
        peaks[c.part + blockIdx.x] = peak;
        sums[c.part + blockIdx.x] = sum;
    }
}

// grid (B): block b folds clip b's chunk partials (sums is rewritten; tmp is its ping-pong twin) and writes out[0] = peak,
// out[1] = sqrt(sum / n), the quotient rounded once
template <class D> __global__ __launch_bounds__(LEVEL_THREADS) void level_finish_kernel(const D d, const float* __restrict__ peaks,
                                                                                     float* sums, float* tmp) {
    const LevelClip c = d.clip[blockIdx.x];
    long count = (c.n + LEVEL_CHUNK - 1) / LEVEL_CHUNK;
    float m = 0.f;
    for (long i = threadIdx.x; i < count; i += LEVEL_THREADS) m = fmaxf(m, peaks[c.part + i]);
    float* a = sums + c.part;
    float* b = tmp + c.part;
    while (count > LEVEL_THREADS) {
        const long half = (count + 1) / 2;
        for (long i = threadIdx.x; i < half; i += LEVEL_THREADS) b[i] = a[2 * i] + (2 * i + 1 < count ? a[2 * i + 1] : 0.f);
        __syncthreads();                                        // (the block's own stores, before any of its threads reads them)
        float* t = a; a = b; b = t;
        count = half;
    }
    float sum, peak;
    level_block_tail((long)threadIdx.x < count ? a[threadIdx.x] : 0.f, m, sum, peak);
    if (threadIdx.x == 0) {
        c.out[0] = peak;
        c.out[1] = __fsqrt_rn((float)((double)sum / (double)c.n));
    }
}

// grid (ceil(max n / LEVEL_SPAN), B): x[i] = x[i] / d * gain over clip b's n samples, d = level + 1e-8 with level = out[mode]
// (0 the peak, 1 the rms); block 0 of the clip leaves d in scales[b]
template <class D> __global__ __launch_bounds__(LEVEL_THREADS) void level_apply_kernel(const D d, int mode, float gain,
                                                                                    float* __restrict__ scales) {
    const LevelClip c = d.clip[blockIdx.y];
    const long i = (long)blockIdx.x * LEVEL_SPAN + 4 * (long)threadIdx.x;
    const float level = ((global_ptr<const float>)c.out)[mode];
    const float div = mode == 0 ? level + 1e-8f : 1e-8f + level;
    if (blockIdx.x == 0 && threadIdx.x == 0) scales[blockIdx.y] = div;
    if (i >= c.n) return;
    const global_ptr<float> x = (global_ptr<float>)const_cast<float*>(c.x);
    if (i + 4 <= c.n && (uintptr_t)(c.x + i) % 16 == 0) {
        lv_f32x4 w = *(global_ptr<lv_f32x4>)(x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = __fdiv_rn(w[e], div);
            if (gain != 1.f) w[e] = w[e] * gain;
        }
        *(global_ptr<lv_f32x4>)(x + i) = w;
        return;
    }
    for (int e = 0; e < 4 && i + e < c.n; ++e) {
        float v = __fdiv_rn(x[i + e], div);
        if (gain != 1.f) v = v * gain;
        x[i + e] = v;
    }
}

// grid (F, ceil(max_len / LEVEL_SPAN)): rows[f][0 .. lens[f]) *= scales[f], one rounded product per sample
__global__ __launch_bounds__(LEVEL_THREADS) void scale_rows_kernel(float* const* __restrict__ rows, const int64_t* __restrict__ lens,
                                                                  const float* __restrict__ scales) {
    const long len = lens[blockIdx.x];
    const long i = (long)blockIdx.y * LEVEL_SPAN + 4 * (long)threadIdx.x;
    if (i >= len) return;
    const global_ptr<float> x = (global_ptr<float>)rows[blockIdx.x];
    const float s = scales[blockIdx.x];
    if (i + 4 <= len && (uintptr_t)(x + i) % 16 == 0) {
        lv_f32x4 w = *(global_ptr<lv_f32x4>)(x + i);
        w = w * s;
        *(global_ptr<lv_f32x4>)(x + i) = w;
        return;
    }
    for (int e = 0; e < 4 && i + e < len; ++e) x[i + e] = x[i + e] * s;
}

static size_t level_descriptor_bytes(int B) { return (size_t)B * sizeof(LevelClip); }

// The descriptors checked and turned into their device form; chunks: the partials the call needs, max_n: its longest clip
static int level_prepare(const std::string& fn, const wt_level_clip* clips, int B, const void* workspace, std::vector<LevelClip>& dev,
                         int64_t& chunks, int64_t& max_n) {
    if (!clips || !workspace || B < 1 || B > 65535) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    dev.resize((size_t)B);
    chunks = 0;
    max_n = 0;
    for (int b = 0; b < B; ++b) {
        const wt_level_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.x) { set_error(who + "null source"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null destination"); return WT_ERR_INVALID; }
        if (c.n < 1) { set_error(who + "n < 1"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.x) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        dev[b] = LevelClip{c.x, (long)c.n, c.out, (long)chunks};
        chunks += (c.n + LEVEL_CHUNK - 1) / LEVEL_CHUNK;
        max_n = std::max<int64_t>(max_n, c.n);
    }
    if ((max_n + LEVEL_CHUNK - 1) / LEVEL_CHUNK > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    return WT_OK;
}

// The measurement's two launches and, with scales, the gain launch behind them, all on one descriptor source
static int level_launch(const char* fn, const std::vector<LevelClip>& dev, int64_t chunks, int64_t max_n, void* workspace, hipStream_t s,
                        int mode, float gain, float* scales) {
    const int B = (int)dev.size();
    float* peaks = reinterpret_cast<float*>(static_cast<char*>(workspace) + level_descriptor_bytes(B));
    float* sums = peaks + chunks;
    float* tmp = sums + chunks;
    const dim3 grid((unsigned)((max_n + LEVEL_CHUNK - 1) / LEVEL_CHUNK), (unsigned)B);
    const dim3 span((unsigned)((max_n + LEVEL_SPAN - 1) / LEVEL_SPAN), (unsigned)B);
    if (int rc = launch_ragged<LEVEL_ARG_CLIPS>(fn, dev.data(), B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL(level_chunk_kernel<decltype(d)>, grid, dim3(LEVEL_THREADS), 0, s, d, peaks, sums);
        hipLaunchKernelGGL(level_finish_kernel<decltype(d)>, dim3((unsigned)B), dim3(LEVEL_THREADS), 0, s, d, peaks, sums, tmp);
        if (scales) hipLaunchKernelGGL(level_apply_kernel<decltype(d)>, span, dim3(LEVEL_THREADS), 0, s, d, mode, gain, scales);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // namespace wt

using namespace wt;

extern "C" {

int32_t wt_level_chunk(void) { return LEVEL_CHUNK; }

size_t wt_level_workspace_bytes(int32_t B, int64_t total_samples) {
    if (B < 1 || total_samples < 1) return 0;
    const size_t chunks = (size_t)(total_samples / LEVEL_CHUNK) + (size_t)B;        // >= sum of ceil(n_b / LEVEL_CHUNK)
    return level_descriptor_bytes(B) + 3 * chunks * sizeof(float) + 8;
}

int wt_level(const wt_level_clip* clips, int32_t B, void* workspace, void* stream) {
    std::vector<LevelClip> dev;
    int64_t chunks = 0, max_n = 0;
    if (int rc = level_prepare("wt_level", clips, B, workspace, dev, chunks, max_n)) return rc;
    return level_launch("wt_level", dev, chunks, max_n, workspace, static_cast<hipStream_t>(stream), 0, 1.f, nullptr);
}

size_t wt_normalize_rows_workspace_bytes(int32_t B, int64_t T_pad) {
    if (B < 1 || T_pad < 1) return 0;
    return wt_level_workspace_bytes(B, (int64_t)B * T_pad) + 2 * (size_t)B * sizeof(float);
}

int wt_normalize_rows(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t mode, float gain, float* scales,
                      void* workspace, void* stream) {
    if (!rows || !n || !scales || !workspace || B < 1 || B > 65535 || T_pad < 1) { set_error("wt_normalize_rows: bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(rows) % sizeof(float) || reinterpret_cast<uintptr_t>(scales) % sizeof(float)) {
        set_error("wt_normalize_rows: rows or scales misaligned"); return WT_ERR_INVALID;
    }
    if (mode != WT_NORM_PEAK && mode != WT_NORM_RMS) { set_error("wt_normalize_rows: mode must be WT_NORM_PEAK or WT_NORM_RMS"); return WT_ERR_INVALID; }
    if (!(gain > 0.f) || !std::isfinite(gain)) { set_error("wt_normalize_rows: gain must be positive and finite"); return WT_ERR_INVALID; }
    if (mode == WT_NORM_RMS && gain != 1.f) { set_error("wt_normalize_rows: WT_NORM_RMS takes gain 1"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error("wt_normalize_rows: workspace misaligned"); return WT_ERR_INVALID; }
    // the rows' statistics lie behind the measurement's own workspace (sized for B rows of T_pad samples)
    float* stats = reinterpret_cast<float*>(static_cast<char*>(workspace) + wt_level_workspace_bytes(B, (int64_t)B * T_pad));
    std::vector<wt_level_clip> clips((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > T_pad) { set_error("wt_normalize_rows: row " + std::to_string(b) + ": n outside [1, T_pad]"); return WT_ERR_INVALID; }
        clips[b] = wt_level_clip{rows + (int64_t)b * T_pad, n[b], stats + 2 * b};
    }
    std::vector<LevelClip> dev;
    int64_t chunks = 0, max_n = 0;
    if (int rc = level_prepare("wt_normalize_rows", clips.data(), B, workspace, dev, chunks, max_n)) return rc;
    return level_launch("wt_normalize_rows", dev, chunks, max_n, workspace, static_cast<hipStream_t>(stream), mode, gain, scales);
}

int wt_scale_rows(float* const* rows, const int64_t* lens, const float* scales, int32_t F, int64_t max_len, void* stream) {
    if (!rows || !lens || !scales || F < 1 || max_len < 1) { set_error("wt_scale_rows: bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(rows) % sizeof(void*) || reinterpret_cast<uintptr_t>(lens) % sizeof(int64_t) ||
        reinterpret_cast<uintptr_t>(scales) % sizeof(float)) {
        set_error("wt_scale_rows: misaligned pointer"); return WT_ERR_INVALID;
    }
    if ((max_len + LEVEL_SPAN - 1) / LEVEL_SPAN > 65535) { set_error("wt_scale_rows: rows too long for one launch"); return WT_ERR_INVALID; }
    const dim3 grid((unsigned)F, (unsigned)((max_len + LEVEL_SPAN - 1) / LEVEL_SPAN));
    hipLaunchKernelGGL(scale_rows_kernel, grid, dim3(LEVEL_THREADS), 0, static_cast<hipStream_t>(stream), rows, lens, scales);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // extern "C"
