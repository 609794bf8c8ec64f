// What loudness.hip shares with r128.hip (the EBU R 128 meter): the device form of a clip, the 100 ms grid in integer arithmetic,
// the gating of one clip as loud_gate_kernel runs it (one text, so that both callers give a clip the same bits), and the host
// entries to the K-weighting's three launches.  The kernels of the filter themselves stay in loudness.hip.
#pragma once
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <string>
#include <vector>

// (sums must not depend on the kernel a device function is inlined into: no contraction by the compiler)
#pragma clang fp contract(off)
#include "fft.h"

namespace wt {

constexpr int LOUD_CHUNK = 128;                 // samples per lane of the two walks (<= 800: at most one 100 ms boundary at 8 kHz)
constexpr int LOUD_THREADS = 256;               // the scan's and the gating's workgroups
constexpr int LOUD_ARG_CLIPS = 64;              // descriptors up to this many travel in the launches' argument blocks (ragged.h);
                                                // with the scan's matrices they fill most of an argument block: see the assertion in loudness.hip
constexpr int LOUD_SLOT_DOUBLES = 20;           // workspace per chunk: end state, start state, wave total, carry (4 each), 2 partials, segment, block

// One clip of a call (device form of wt_loudness_clip)
struct LoudClip {
    const float* x;
    long n;
    long ch_stride;
    float* out;                                 // [3]: L, threshold, gated blocks ([9] for wt_loudness_range)
    float* blocks;                              // nullable: J momentary values
    int part;                                   // the clip's first chunk slot in the workspace (channel c: part + c * chunks)
    int channels;
};

// complete 400 ms blocks of n samples at rate fs: the j with floor((j + 4) fs / 10) <= n
__host__ __device__ __forceinline__ long loud_blocks(long n, int fs) {
    const long m = (10 * (n + 1) - 1) / fs;     // the largest m with floor(m fs / 10) <= n
    return m > 3 ? m - 3 : 0;
}
// first sample of 100 ms segment j
__host__ __device__ __forceinline__ long loud_edge(long j, int fs) { return j * (long)fs / 10; }
// the segment that holds sample s
__host__ __device__ __forceinline__ long loud_segment_of(long s, int fs) { return (10 * (s + 1) - 1) / fs; }

// the workgroup's sum of v and of n: the xor butterfly over the wave, the four waves as (0 + 1) + (2 + 3); every thread gets both
__device__ __forceinline__ void loud_block_sum(double v, int n, double& sum, int& count) {
    __shared__ double wv[LOUD_THREADS / 64];
    __shared__ int wn[LOUD_THREADS / 64];
    __syncthreads();                                            // (the last call's readers are done)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        v = v + __shfl_xor(v, off, 64);
        n = n + __shfl_xor(n, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = v; wn[threadIdx.x >> 6] = n; }
    __syncthreads();
    sum = (wv[0] + wv[1]) + (wv[2] + wv[3]);
    count = (wn[0] + wn[1]) + (wn[2] + wn[3]);
}

__device__ __forceinline__ double loud_lufs(double z) { return -0.691 + 10. * log10(z); }

// What the gating of a clip leaves in every thread of its workgroup
struct LoudGated {
    double sum;                                 // of z over the blocks through both gates
    double gamma;                               // the relative threshold (-inf without a block over -70)
    int count;                                  // blocks through both gates
};

// One workgroup of LOUD_THREADS threads on clip c: the partials become segment sums (seg) and block energies (zblk, and the
// momentary values in c.blocks), then both gates run over fixed trees.  Ends behind a barrier: seg and zblk can be read.
__device__ __forceinline__ LoudGated loud_gate_clip(const LoudClip& c, int fs, const double* __restrict__ part2, double* seg, double* zblk) {
    const long chunks = (c.n + LOUD_CHUNK - 1) / LOUD_CHUNK;
    const long J = loud_blocks(c.n, fs);
    const long segments = J > 0 ? J + 3 : 0;                    // (each is at least 800 samples: there are fewer than chunks)
    for (int ch = 0; ch < c.channels; ++ch) {
        const long base = (long)c.part + (long)ch * chunks;
        for (long j = threadIdx.x; j < segments; j += LOUD_THREADS) {
            const long lo = loud_edge(j, fs) / LOUD_CHUNK, hi = (loud_edge(j + 1, fs) - 1) / LOUD_CHUNK;
            double sum = 0.;
            for (long kk = lo; kk <= hi; ++kk)                  // the chunk began in this segment: its front part, else its back part
                sum = sum + part2[2 * (base + kk) + (loud_segment_of(kk * LOUD_CHUNK, fs) == j ? 0 : 1)];
            seg[base + j] = sum;
        }
    }
    __syncthreads();
    const global_ptr<float> blocks = (global_ptr<float>)c.blocks;
    for (long j = threadIdx.x; j < J; j += LOUD_THREADS) {
        const double len = (double)(loud_edge(j + 4, fs) - loud_edge(j, fs));
        double z = 0.;
        for (int ch = 0; ch < c.channels; ++ch) {
            const double* s = seg + (long)c.part + (long)ch * chunks + j;
            z = z + ((s[0] + s[1]) + (s[2] + s[3])) / len;
        }
        zblk[c.part + j] = z;
        if (c.blocks) blocks[j] = (float)loud_lufs(z);
    }
    __syncthreads();
    double v = 0., sum;
    int n = 0, count;
    for (long j = threadIdx.x; j < J; j += LOUD_THREADS) {
        const double z = zblk[c.part + j];
        if (loud_lufs(z) > -70.) { v = v + z; ++n; }
    }
    loud_block_sum(v, n, sum, count);
    const double inf = __builtin_huge_val();
    LoudGated g;
    g.gamma = count > 0 ? loud_lufs(sum / (double)count) - 10. : -inf;
    v = 0.;
    n = 0;
    for (long j = threadIdx.x; j < J; j += LOUD_THREADS) {
        const double z = zblk[c.part + j];
        const double l = loud_lufs(z);
        if (l > -70. && l > g.gamma) { v = v + z; ++n; }
    }
    loud_block_sum(v, n, g.sum, g.count);
    return g;
}

// out[0..3) of a gated clip (one thread); returns L as stored
__device__ __forceinline__ float loud_store_triple(const LoudGated& g, float* out_) {
    const double inf = __builtin_huge_val();
    const float L = g.count > 0 ? (float)loud_lufs(g.sum / (double)g.count) : (float)-inf;
    const global_ptr<float> out = (global_ptr<float>)out_;
    out[0] = L;
    out[1] = g.count > 0 ? (float)g.gamma : (float)-inf;
    out[2] = (float)g.count;
    return L;
}

// ---- host (loudness.hip) ---------------------------------------------------------------------------------------------------------

bool loud_rate_ok(int fs);

// The descriptors checked and turned into their device form; slots: the chunk slots the call needs, max_n: its longest clip
int loud_prepare(const std::string& fn, const wt_loudness_clip* clips, int B, int fs, const void* workspace, std::vector<LoudClip>& dev,
                 int64_t& slots, int64_t& max_n, int& max_ch);

// Where a call of B clips and `slots` chunk slots keeps the energy partials, the segment sums and the block energies
struct LoudBuffers { double* part2; double* seg; double* zblk; };
LoudBuffers loud_buffers(void* workspace, int B, int64_t slots);

// The K-weighting alone: walk, scan, walk (three launches); the partials are then in loud_buffers(...).part2 and, with more than
// LOUD_ARG_CLIPS clips, the descriptors at the head of workspace
int loud_filter_launch(const char* fn, const std::vector<LoudClip>& dev, int64_t slots, int64_t max_n, int max_ch, int fs, void* workspace,
                       hipStream_t s);

// The measurement's four launches and, with scales, the gain launch behind them, all on one descriptor source.  With true_peaks
// (device, one pair per clip: wt_true_peak's out) a launch in front of the gain raises scales[b] to
// fp32((double)true_peaks[2 b] / ceiling) where that is larger and the clip has a loudness
int loud_launch(const char* fn, const std::vector<LoudClip>& dev, int64_t slots, int64_t max_n, int max_ch, int fs, void* workspace,
                hipStream_t s, float* scales, double target, const float* true_peaks = nullptr, double ceiling = 1.);

}  // namespace wt
