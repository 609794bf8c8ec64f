// The rest of an EBU R 128 meter beside the integrated loudness of loudness.hip: true peak by oversampling (ITU-R BS.1770-4
// Annex 2), short-term loudness (EBU Tech 3341) and loudness range (EBU Tech 3342) of ragged clips, and the true-peak ceiling on
// the gain of wt_normalize_rows_lufs.  include/wavtokenizer_amd.h states the three definitions.
//
// True peak, two launches.  A workgroup stages TP_TILE samples of one channel and the interpolator's halo (24 / F samples on
// either side, zeros outside the clip) in LDS once; thread t takes samples t, t + 256, t + 512, t + 768 of the tile (neighbouring
// lanes read neighbouring words: no bank is asked twice), reads the 48 / F samples under the interpolator once per sample and
// runs the F - 1 phases on them, one fmaf per tap from 0 with k ascending.  The maxima of |y| and of |x| go over the wave by the
// xor butterfly, over the four waves through LDS, into one pair per tile; a second launch, one workgroup per clip, takes the
// maximum of the clip's pairs.  A maximum is exact in any order and a sample's value depends on the clip's samples alone: a clip
// has the same bits alone, at any position of any batch, whatever the grid and whatever its pointer's alignment.
//
// Loudness range, four launches: the K-weighting's three (loudness.hip: walk, scan, walk), then one workgroup per clip that runs
// loud_gate_clip (the text of loud_gate_kernel: segment sums, blocks, both gates of the integrated loudness), adds each 3 s
// window's 30 segment sums in ascending order from the first (fp64, per channel, then the channels in order), runs the two range
// gates over the same fixed trees as the integrated gates and selects the two ranks by a radix select on the windows' bit patterns
// (positive doubles order as their bits do): eight passes of eight bits, most significant first, over a 256-bin histogram in LDS
// filled by integer atomics, whose order does not matter.  No float atomics, nothing sorted, no cap on the number of windows.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

// (sums must not depend on the kernel a device function is inlined into: no contraction by the compiler)
#pragma clang fp contract(off)
#include "loudness_kernels.h"
#include "ragged.h"

namespace wt {

constexpr int TP_TILE = 1024;                   // samples per workgroup: four per thread
constexpr int TP_THREADS = 256;
constexpr int TP_ARG_CLIPS = 64;                // descriptors up to this many travel in the launches' argument blocks (ragged.h)
constexpr int TP_MAX_HALO = 12;                 // 24 / F at the least F that filters (2)
constexpr int RANGE_WINDOW = 30;                // 100 ms segments in a short-term window

// One clip of a true-peak call (device form of wt_true_peak_clip)
struct TpClip {
    const float* x;
    long n;
    long ch_stride;
    float* out;                                 // [2]: true peak, sample peak
    long part;                                  // the clip's first tile among the per-tile pairs in the workspace (channel c: part + c * tiles)
    int channels;
};

// the interpolator: h[j], j < 48 (h[48] = 0 is never read)
struct TpTaps { float h[48]; };

// What wt_loudness_range adds to a LoudClip
struct RangeClip { float* short_term; };

static_assert(sizeof(ArgClips<TpClip, TP_ARG_CLIPS>) + sizeof(TpTaps) + sizeof(void*) <= 4096, "tp_tile_kernel's argument block");
static_assert(sizeof(ArgClips<LoudClip, LOUD_ARG_CLIPS>) + sizeof(ArgClips<RangeClip, LOUD_ARG_CLIPS>) + 8 * sizeof(void*) <= 4096,
              "range_kernel's argument block");

// the workgroup's maxima of a and b (256 threads): the xor butterfly over the wave, then the four waves; every thread gets both
__device__ __forceinline__ void r128_block_max(float& a, float& b) {
    __shared__ float wm[TP_THREADS / 64][2];
    __syncthreads();                                            // (the last call's readers are done)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        a = fmaxf(a, __shfl_xor(a, off, 64));
        b = fmaxf(b, __shfl_xor(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { wm[threadIdx.x >> 6][0] = a; wm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    a = fmaxf(fmaxf(wm[0][0], wm[1][0]), fmaxf(wm[2][0], wm[3][0]));
    b = fmaxf(fmaxf(wm[0][1], wm[1][1]), fmaxf(wm[2][1], wm[3][1]));
}

// grid (ceil(max n / TP_TILE), B, channels): block (t, b, c) leaves the maxima of |y| (all phases, phase 0 = |x| included) and of
// |x| over tile t of channel c of clip b in pairs[2 slot], pairs[2 slot + 1]
template <class D, int F> __global__ __launch_bounds__(TP_THREADS) void tp_tile_kernel(const D d, const TpTaps h, float* __restrict__ pairs) {
    const TpClip c = d.clip[blockIdx.y];
    const int ch = blockIdx.z;
    if (ch >= c.channels) return;                               // (the whole block, here and below: no barrier is left waiting)
    const long s0 = (long)blockIdx.x * TP_TILE;
    if (s0 >= c.n) return;
    const global_ptr<const float> x = (global_ptr<const float>)c.x + (long)ch * c.ch_stride;
    float tp = 0.f, sp = 0.f;
    if constexpr (F == 1) {
#pragma unroll
        for (int e = 0; e < TP_TILE / TP_THREADS; ++e) {
            const long i = s0 + threadIdx.x + TP_THREADS * e;
            if (i < c.n) sp = fmaxf(sp, fabsf(x[i]));
        }
    } else {
        constexpr int HALO = 24 / F, TAPS = 48 / F;
        static_assert(HALO <= TP_MAX_HALO, "halo");
        __shared__ float stage[TP_TILE + 2 * TP_MAX_HALO];
        for (int j = threadIdx.x; j < TP_TILE + 2 * HALO; j += TP_THREADS) {
            const long idx = s0 - HALO + j;
            stage[j] = idx >= 0 && idx < c.n ? x[idx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < TP_TILE / TP_THREADS; ++e) {
            const int li = threadIdx.x + TP_THREADS * e;
            if (s0 + li >= c.n) continue;
            float w[TAPS];                                      // w[k] = x[i + 24 / F - k]: words li + 1 .. li + 2 HALO of the stage
#pragma unroll
            for (int k = 0; k < TAPS; ++k) w[k] = stage[li + 2 * HALO - k];
            sp = fmaxf(sp, fabsf(w[HALO]));
#pragma unroll
            for (int p = 1; p < F; ++p) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) acc = fmaf(h.h[p + F * k], w[k], acc);
                tp = fmaxf(tp, fabsf(acc));
            }
        }
    }
    tp = fmaxf(tp, sp);
    r128_block_max(tp, sp);
    if (threadIdx.x == 0) {
        const long tiles = (c.n + TP_TILE - 1) / TP_TILE;
        const long slot = c.part + (long)ch * tiles + blockIdx.x;
        pairs[2 * slot] = tp;
        pairs[2 * slot + 1] = sp;
    }
}

// grid (B): block b takes the maxima of clip b's pairs into out[0], out[1]
template <class D> __global__ __launch_bounds__(TP_THREADS) void tp_finish_kernel(const D d, const float* __restrict__ pairs) {
    const TpClip c = d.clip[blockIdx.x];
    const long count = (long)c.channels * ((c.n + TP_TILE - 1) / TP_TILE);
    float tp = 0.f, sp = 0.f;
    for (long i = threadIdx.x; i < count; i += TP_THREADS) {
        tp = fmaxf(tp, pairs[2 * (c.part + i)]);
        sp = fmaxf(sp, pairs[2 * (c.part + i) + 1]);
    }
    r128_block_max(tp, sp);
    if (threadIdx.x == 0) {
        const global_ptr<float> out = (global_ptr<float>)c.out;
        out[0] = tp;
        out[1] = sp;
    }
}

// does window energy z pass both range gates
__device__ __forceinline__ bool range_kept(double z, double rel) {
    const double l = loud_lufs(z);
    return l > -70. && l > rel;
}

// The bits of the energy of rank `rank` (0 the least) among the windows of z[0 .. S) that pass both range gates; rank is below
// their number.  All 256 threads call it and get the value
__device__ __forceinline__ unsigned long long range_select(const double* z, long S, double rel, long rank) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long next_prefix;
    __shared__ long next_rank;
    unsigned long long prefix = 0;                              // the bits above the pass's eight, as found so far
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();                                        // (the last pass's readers are done)
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (long j = threadIdx.x; j < S; j += LOUD_THREADS) {
            const double v = z[j];
            if (!range_kept(v, rel)) continue;
            const unsigned long long key = (unsigned long long)__double_as_longlong(v);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long r = rank;
            int b = 0;
            while (b < 255 && r >= (long)hist[b]) { r -= (long)hist[b]; ++b; }
            next_prefix = prefix | ((unsigned long long)b << shift);
            next_rank = r;
        }
        __syncthreads();
        prefix = next_prefix;
        rank = next_rank;
    }
    return prefix;
}

// grid (B), LOUD_THREADS threads: block b gates clip b as loud_gate_kernel does (out[0..3)), then forms its short-term windows,
// the range gates, the two selected windows and the two maxima (out[3..9))
template <class DL, class DR> __global__ __launch_bounds__(LOUD_THREADS) void range_kernel(const DL dl, const DR dr, int fs,
                                                                                          const double* __restrict__ part2, double* seg,
                                                                                          double* zblk, double* zwin) {
    static_assert(LOUD_THREADS == 256 && TP_THREADS == 256, "one histogram bin per thread; r128_block_max");
    const LoudClip c = dl.clip[blockIdx.x];
    const LoudGated g = loud_gate_clip(c, fs, part2, seg, zblk);
    if (threadIdx.x == 0) loud_store_triple(g, c.out);
    const long chunks = (c.n + LOUD_CHUNK - 1) / LOUD_CHUNK;
    const long J = loud_blocks(c.n, fs);
    const long S = J > RANGE_WINDOW - 4 ? J - (RANGE_WINDOW - 4) : 0;       // (window j ends where block j + 26 ends)
    const float ninf = -__builtin_huge_valf();
    float max_m = ninf, max_s = ninf;
    for (long j = threadIdx.x; j < J; j += LOUD_THREADS) max_m = fmaxf(max_m, (float)loud_lufs(zblk[c.part + j]));
    const global_ptr<float> st = (global_ptr<float>)dr.clip[blockIdx.x].short_term;
    double* zw = zwin + c.part;
    for (long j = threadIdx.x; j < S; j += LOUD_THREADS) {
        const double len = (double)(loud_edge(j + RANGE_WINDOW, fs) - loud_edge(j, fs));
        double z = 0.;
        for (int ch = 0; ch < c.channels; ++ch) {
            const double* s = seg + (long)c.part + (long)ch * chunks + j;
            double w = s[0];
            for (int i = 1; i < RANGE_WINDOW; ++i) w = w + s[i];
            z = z + w / len;
        }
        zw[j] = z;
        const float sj = (float)loud_lufs(z);
        if (st) st[j] = sj;
        max_s = fmaxf(max_s, sj);
    }
    __syncthreads();                                            // (the block's own stores, before any of its threads reads them)
    double v = 0., sum;
    int n = 0, count, m;
    for (long j = threadIdx.x; j < S; j += LOUD_THREADS) {
        const double z = zw[j];
        if (loud_lufs(z) > -70.) { v = v + z; ++n; }
    }
    loud_block_sum(v, n, sum, count);
    const double rel = count > 0 ? loud_lufs(sum / (double)count) - 20. : -__builtin_huge_val();
    n = 0;
    for (long j = threadIdx.x; j < S; j += LOUD_THREADS) n += range_kept(zw[j], rel) ? 1 : 0;
    loud_block_sum(0., n, sum, m);
    double l_lo = 0., l_hi = 0.;
    if (m > 0) {                                                // (m is the same in every thread)
        const long lo = ((long)(m - 1) + 5) / 10, hi = (19 * (long)(m - 1) + 10) / 20;
        l_lo = loud_lufs(__longlong_as_double((long long)range_select(zw, S, rel, lo)));
        l_hi = loud_lufs(__longlong_as_double((long long)range_select(zw, S, rel, hi)));
    }
    r128_block_max(max_m, max_s);
    if (threadIdx.x != 0) return;
    const global_ptr<float> out = (global_ptr<float>)c.out;
    const float nan = __builtin_nanf("");
    out[3] = m > 0 ? (float)(l_hi - l_lo) : nan;
    out[4] = m > 0 ? (float)l_lo : nan;
    out[5] = m > 0 ? (float)l_hi : nan;
    out[6] = (float)m;
    out[7] = max_m;
    out[8] = max_s;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

static int tp_factor(int fs) { return fs < 96000 ? 4 : fs < 192000 ? 2 : 1; }

// h[j] = sinc((j - 24) / F) * 0.5 (1 - cos(2 pi j / 48)) in double, rounded to fp32
static TpTaps tp_taps(int F) {
    const double pi = 3.14159265358979323846;
    TpTaps t;
    for (int j = 0; j < 48; ++j) {
        const double u = (double)(j - 24) / (double)F;
        const double sinc = j == 24 ? 1. : std::sin(pi * u) / (pi * u);
        t.h[j] = (float)(sinc * (0.5 * (1. - std::cos(2. * pi * (double)j / 48.))));
    }
    return t;
}

static size_t tp_descriptor_bytes(int B) { return (size_t)B * sizeof(TpClip); }

// The descriptors checked and turned into their device form; tiles: the pairs the call needs, max_n: its longest clip
static int tp_prepare(const std::string& fn, const wt_true_peak_clip* clips, int B, int fs, const void* workspace, std::vector<TpClip>& dev,
                      int64_t& tiles, int64_t& max_n, int& max_ch) {
    if (!clips || !workspace || B < 1 || B > 65535) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (!loud_rate_ok(fs)) { set_error(fn + ": sample_rate outside [8000, 192000]"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    dev.resize((size_t)B);
    tiles = 0;
    max_n = 0;
    max_ch = 1;
    for (int b = 0; b < B; ++b) {
        const wt_true_peak_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.x) { set_error(who + "null source"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null destination"); return WT_ERR_INVALID; }
        if (c.n < 1) { set_error(who + "n < 1"); return WT_ERR_INVALID; }
        if (c.channels != 1 && c.channels != 2) { set_error(who + "channels must be 1 or 2"); return WT_ERR_INVALID; }
        if (c.channels == 2 && c.channel_stride < c.n) { set_error(who + "channel_stride < n"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.x) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        dev[b] = TpClip{c.x, (long)c.n, c.channels == 2 ? (long)c.channel_stride : 0L, c.out, (long)tiles, c.channels};
        tiles += (int64_t)c.channels * ((c.n + TP_TILE - 1) / TP_TILE);
        max_n = std::max<int64_t>(max_n, c.n);
        max_ch = std::max(max_ch, (int)c.channels);
    }
    if ((max_n + TP_TILE - 1) / TP_TILE > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    return WT_OK;
}

// The measurement's two launches on one descriptor source
static int tp_launch(const char* fn, const std::vector<TpClip>& dev, int64_t max_n, int max_ch, int fs, void* workspace, hipStream_t s) {
    const int B = (int)dev.size();
    const int F = tp_factor(fs);
    const TpTaps h = tp_taps(F);
    float* pairs = reinterpret_cast<float*>(static_cast<char*>(workspace) + tp_descriptor_bytes(B));
    const dim3 grid((unsigned)((max_n + TP_TILE - 1) / TP_TILE), (unsigned)B, (unsigned)max_ch);
    if (int rc = launch_ragged<TP_ARG_CLIPS>(fn, dev.data(), B, 128, workspace, s, [&](auto d) {
        if (F == 4) hipLaunchKernelGGL((tp_tile_kernel<decltype(d), 4>), grid, dim3(TP_THREADS), 0, s, d, h, pairs);
        else if (F == 2) hipLaunchKernelGGL((tp_tile_kernel<decltype(d), 2>), grid, dim3(TP_THREADS), 0, s, d, h, pairs);
        else hipLaunchKernelGGL((tp_tile_kernel<decltype(d), 1>), grid, dim3(TP_THREADS), 0, s, d, h, pairs);
        hipLaunchKernelGGL(tp_finish_kernel<decltype(d)>, dim3((unsigned)B), dim3(TP_THREADS), 0, s, d, pairs);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // namespace wt

using namespace wt;

extern "C" {

int32_t wt_true_peak_tile(void) { return TP_TILE; }

size_t wt_true_peak_workspace_bytes(int32_t B, int64_t total_samples) {
    if (B < 1 || total_samples < 1) return 0;
    const size_t tiles = (size_t)(total_samples / TP_TILE) + 2 * (size_t)B;         // >= sum of channels_b * ceil(n_b / TP_TILE)
    return tp_descriptor_bytes(B) + 2 * tiles * sizeof(float) + 8;
}

int wt_true_peak(const wt_true_peak_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream) {
    std::vector<TpClip> dev;
    int64_t tiles = 0, max_n = 0;
    int max_ch = 1;
    if (int rc = tp_prepare("wt_true_peak", clips, B, sample_rate, workspace, dev, tiles, max_n, max_ch)) return rc;
    return tp_launch("wt_true_peak", dev, max_n, max_ch, sample_rate, workspace, static_cast<hipStream_t>(stream));
}

int64_t wt_short_term_blocks(int64_t n, int32_t sample_rate) {
    if (n < 1 || !loud_rate_ok(sample_rate)) return 0;
    const long J = loud_blocks((long)n, sample_rate);
    return J > RANGE_WINDOW - 4 ? J - (RANGE_WINDOW - 4) : 0;
}

size_t wt_loudness_range_workspace_bytes(int32_t B, int64_t total_samples) {
    if (B < 1 || total_samples < 1) return 0;
    const size_t slots = (size_t)(total_samples / LOUD_CHUNK) + 2 * (size_t)B;      // (as wt_loudness_workspace_bytes counts them)
    return wt_loudness_workspace_bytes(B, total_samples) + (size_t)B * sizeof(RangeClip) + slots * sizeof(double);
}

int wt_loudness_range(const wt_loudness_range_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream) {
    const std::string fn = "wt_loudness_range";
    if (!clips || !workspace || B < 1 || B > 65535) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    std::vector<wt_loudness_clip> lc((size_t)B);
    std::vector<RangeClip> rdev((size_t)B);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        const wt_loudness_range_clip& c = clips[b];
        if (reinterpret_cast<uintptr_t>(c.short_term) % sizeof(float)) {
            set_error(fn + ": clip " + std::to_string(b) + ": misaligned pointer"); return WT_ERR_INVALID;
        }
        lc[b] = wt_loudness_clip{c.x, c.n, c.channels, c.channel_stride, c.out, c.momentary};
        rdev[b] = RangeClip{c.short_term};
        if (c.n > 0 && (c.channels == 1 || c.channels == 2)) total += c.n * c.channels;
    }
    std::vector<LoudClip> dev;
    int64_t slots = 0, max_n = 0;
    int max_ch = 1;
    if (int rc = loud_prepare(fn, lc.data(), B, sample_rate, workspace, dev, slots, max_n, max_ch)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = loud_filter_launch("wt_loudness_range", dev, slots, max_n, max_ch, sample_rate, workspace, s)) return rc;
    // the range's own descriptors and its windows lie behind the measurement's workspace (as sized for the clips of this call)
    char* mine = static_cast<char*>(workspace) + wt_loudness_workspace_bytes(B, total);
    double* zwin = reinterpret_cast<double*>(mine + (size_t)B * sizeof(RangeClip));
    const LoudBuffers w = loud_buffers(workspace, B, slots);
    if (int rc = launch_ragged<LOUD_ARG_CLIPS>("wt_loudness_range", rdev.data(), B, 128, mine, s, [&](auto dr) {
        if constexpr (std::is_same_v<decltype(dr), PtrClips<RangeClip>>) {
            // (loud_filter_launch left the LoudClips at the head of the workspace)
            hipLaunchKernelGGL((range_kernel<PtrClips<LoudClip>, decltype(dr)>), dim3((unsigned)B), dim3(LOUD_THREADS), 0, s,
                               PtrClips<LoudClip>{static_cast<const LoudClip*>(workspace)}, dr, sample_rate, w.part2, w.seg, w.zblk, zwin);
        } else {
            ArgClips<LoudClip, LOUD_ARG_CLIPS> dl{};
            memcpy(dl.clip, dev.data(), (size_t)B * sizeof(LoudClip));
            hipLaunchKernelGGL((range_kernel<decltype(dl), decltype(dr)>), dim3((unsigned)B), dim3(LOUD_THREADS), 0, s, dl, dr, sample_rate,
                               w.part2, w.seg, w.zblk, zwin);
        }
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

size_t wt_normalize_rows_lufs_tp_workspace_bytes(int32_t B, int64_t T_pad) {
    if (B < 1 || T_pad < 1) return 0;
    return wt_loudness_workspace_bytes(B, (int64_t)B * T_pad) + 6 * (size_t)B * sizeof(float) + wt_true_peak_workspace_bytes(B, (int64_t)B * T_pad);
}

int wt_normalize_rows_lufs_tp(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t sample_rate, double target_lufs,
                              double max_true_peak_db, float* scales, void* workspace, void* stream) {
    const std::string fn = "wt_normalize_rows_lufs_tp";
    if (!rows || !n || !scales || !workspace || B < 1 || B > 65535 || T_pad < 1) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(rows) % sizeof(float) || reinterpret_cast<uintptr_t>(scales) % sizeof(float)) {
        set_error(fn + ": rows or scales misaligned"); return WT_ERR_INVALID;
    }
    if (!std::isfinite(target_lufs)) { set_error(fn + ": target_lufs must be finite"); return WT_ERR_INVALID; }
    if (!std::isfinite(max_true_peak_db)) { set_error(fn + ": max_true_peak_db must be finite"); return WT_ERR_INVALID; }
    if (!loud_rate_ok(sample_rate)) { set_error(fn + ": sample_rate outside [8000, 192000]"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    // behind the loudness measurement's own workspace (sized for B rows of T_pad samples): its results, four floats per row, the
    // true peaks, two per row, and the true-peak measurement's workspace
    float* stats = reinterpret_cast<float*>(static_cast<char*>(workspace) + wt_loudness_workspace_bytes(B, (int64_t)B * T_pad));
    float* peaks = stats + 4 * (size_t)B;
    void* tp_ws = peaks + 2 * (size_t)B;
    std::vector<wt_loudness_clip> clips((size_t)B);
    std::vector<wt_true_peak_clip> tclips((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > T_pad) { set_error(fn + ": row " + std::to_string(b) + ": n outside [1, T_pad]"); return WT_ERR_INVALID; }
        clips[b] = wt_loudness_clip{rows + (int64_t)b * T_pad, n[b], 1, 0, stats + 4 * b, nullptr};
        tclips[b] = wt_true_peak_clip{rows + (int64_t)b * T_pad, n[b], 1, 0, peaks + 2 * b};
    }
    std::vector<LoudClip> dev;
    std::vector<TpClip> tdev;
    int64_t slots = 0, tiles = 0, max_n = 0;
    int max_ch = 1;
    if (int rc = loud_prepare(fn, clips.data(), B, sample_rate, workspace, dev, slots, max_n, max_ch)) return rc;
    if (int rc = tp_prepare(fn, tclips.data(), B, sample_rate, tp_ws, tdev, tiles, max_n, max_ch)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = tp_launch("wt_normalize_rows_lufs_tp", tdev, max_n, max_ch, sample_rate, tp_ws, s)) return rc;
    return loud_launch("wt_normalize_rows_lufs_tp", dev, slots, max_n, max_ch, sample_rate, workspace, s, scales, target_lufs, peaks,
                       std::pow(10., max_true_peak_db / 20.));
}

}  // extern "C"
