// Integrated loudness (ITU-R BS.1770-4 / EBU R 128) of ragged clips, and the normalisation of ingested rows to a target in LUFS.
// include/wavtokenizer_amd.h states the definition (K-weighting, the 400 ms block grid in integer arithmetic, the two gates).
//
// The K-weighting is a recursive filter: two biquads in transposed direct form II, four values of state s, s' = A s + B x.  It is
// evaluated exactly in chunks of LOUD_CHUNK samples, in fp64, by three launches:
//   1. walk: one lane per chunk walks its samples from ZERO state and leaves its end state z_k (the samples of 64 chunks are
//      staged through LDS 32 columns at a time: the global loads are whole 128-byte rows, the lanes then read their own rows
//      at a pitch of 33 words, one bank each);
//   2. scan: s_{k+1} = M s_k + z_k with M = A^LOUD_CHUNK (built on the host in double by repeated squaring).  One workgroup per
//      clip and channel: a log-step scan over the 64 chunks of a wave with M^(2^i), the waves' totals in sequence with M^64 (wave
//      0, 64 totals per load), then the true start state of chunk 64 g + l as M^l carry_g + the scan's value of its left neighbour;
//   3. walk again from the true start state, adding y^2 into two partial sums, one on each side of the one 100 ms boundary a
//      chunk can hold (LOUD_CHUNK is shorter than 100 ms at 8 kHz);
// and a fourth, one workgroup per clip: the partials of a 100 ms segment are added in ascending order, a block is its four
// segments as (0 + 1) + (2 + 3) over its length, the channels are added, and both gates run over fixed trees (thread t takes
// blocks t, t + 256, ... in ascending order, then the xor butterfly, then the four waves as (0 + 1) + (2 + 3)).  Nothing is added
// by an atomic and every order depends on n and the rate alone: a clip has the same bits alone, at any position of any batch and
// whatever the grid.  Products and sums are the fused multiply-adds written out below and nothing else (contraction is off).
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

// (sums must not depend on the kernel a device function is inlined into: no contraction by the compiler)
#pragma clang fp contract(off)
#include "fft.h"
#include "loudness_kernels.h"
#include "ragged.h"

namespace wt {

// (the chunk, the clip's device form, the 100 ms grid and the gating of one clip: loudness_kernels.h, shared with r128.hip)
constexpr int LOUD_TILE = 32;                   // columns staged per step
constexpr int LOUD_PITCH = LOUD_TILE + 1;       // words between the rows of the staged tile: lane l reads bank (33 l + t) % 64, all distinct
constexpr int LOUD_SPAN = 1024;                 // samples per workgroup of the gain kernel: four per thread

typedef float ld_f32x4 __attribute__((ext_vector_type(4)));

// b0 b1 b2 a1 a2 of the shelf, then of the high pass
struct KwCoef { double c[10]; };
// M^(2^i) for i < 6 and M^64, row-major 4 x 4
struct KwMats { double p[7][16]; };

// The scan's launch carries the descriptors, the matrices and four pointers by value: a field more in LoudClip must not push it past
// the 4 KiB an argument block may hold (then lower LOUD_ARG_CLIPS, or move the matrices into the workspace)
static_assert(sizeof(ArgClips<LoudClip, LOUD_ARG_CLIPS>) + sizeof(KwMats) + 4 * sizeof(void*) <= 4096, "loud_scan_kernel's argument block");

// one sample through both biquads (transposed direct form II): the state moves on, the weighted sample returns
__host__ __device__ __forceinline__ double kw_step(const KwCoef& k, double s[4], double x) {
    const double y1 = fma(k.c[0], x, s[0]);
    s[0] = fma(-k.c[3], y1, fma(k.c[1], x, s[1]));
    s[1] = fma(-k.c[4], y1, k.c[2] * x);
    const double y2 = fma(k.c[5], y1, s[2]);
    s[2] = fma(-k.c[8], y2, fma(k.c[6], y1, s[3]));
    s[3] = fma(-k.c[9], y2, k.c[7] * y1);
    return y2;
}

// r = m v + a, each row as ((m0 v0 + m1 v1) + (m2 v2 + m3 v3)) + a
__host__ __device__ __forceinline__ void kw_matvec_add(const double* m, const double v[4], const double a[4], double r[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = ((m[4 * i] * v[0] + m[4 * i + 1] * v[1]) + (m[4 * i + 2] * v[2] + m[4 * i + 3] * v[3])) + a[i];
}

// grid (ceil(max chunks / 64), B, channels), 64 threads: lane l of block (g, b, c) walks chunk 64 g + l of channel c of clip b.
// ENERGY false: from zero state, the end state goes to zend.  ENERGY true: from start, the sums of y^2 in front of and behind the
// chunk's segment boundary go to part2
template <class D, bool ENERGY> __global__ __launch_bounds__(64) void loud_walk_kernel(const D d, const KwCoef k, int fs, double* __restrict__ zend,
                                                                                      const double* __restrict__ start,
                                                                                      double* __restrict__ part2) {
    const LoudClip c = d.clip[blockIdx.y];
    const int ch = blockIdx.z;
    if (ch >= c.channels) return;                               // (the whole block, here and below: no barrier is left waiting)
    const long chunks = (c.n + LOUD_CHUNK - 1) / LOUD_CHUNK;
    const long k0 = (long)blockIdx.x * 64;
    if (k0 >= chunks) return;
    __shared__ float tile[64 * LOUD_PITCH];
    const int lane = threadIdx.x;
    const global_ptr<const float> x = (global_ptr<const float>)c.x + (long)ch * c.ch_stride;
    const long kk = k0 + lane;
    const long slot = (long)c.part + (long)ch * chunks + kk;
    const bool live = kk < chunks;
    double s[4] = {0., 0., 0., 0.};
    int cut = LOUD_CHUNK, lim = 0;
    if (ENERGY && live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = start[4 * slot + i];
        const long s0 = kk * LOUD_CHUNK;
        const long edge = loud_edge(loud_segment_of(s0, fs) + 1, fs);      // the first boundary behind the chunk's first sample
        cut = (int)(edge - s0 < LOUD_CHUNK ? edge - s0 : LOUD_CHUNK);
        lim = (int)(c.n - s0 < LOUD_CHUNK ? c.n - s0 : LOUD_CHUNK);
    }
    double front = 0., back = 0.;
    for (int t0 = 0; t0 < LOUD_CHUNK; t0 += LOUD_TILE) {
#pragma unroll 8
        for (int i = 0; i < 32; ++i) {
            const int row = 2 * i + (lane >> 5), col = lane & 31;
            const long idx = (k0 + row) * LOUD_CHUNK + t0 + col;
            tile[row * LOUD_PITCH + col] = idx < c.n ? x[idx] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < LOUD_TILE; ++t) {
            const double y = kw_step(k, s, (double)tile[lane * LOUD_PITCH + t]);
            if (ENERGY) {
                const double q = y * y;
                front = front + (t0 + t < cut ? q : 0.);
                back = back + (t0 + t >= cut && t0 + t < lim ? q : 0.);
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (ENERGY) {
        part2[2 * slot] = front;
        part2[2 * slot + 1] = back;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) zend[4 * slot + i] = s[i];
    }
}

// grid (B, channels), LOUD_THREADS threads: the start state of every chunk of channel c of clip b from the zero-state end states
// (zend is rewritten with the scan inside each group of 64; gtot and carry are indexed by group at the channel's slots)
template <class D> __global__ __launch_bounds__(LOUD_THREADS) void loud_scan_kernel(const D d, const KwMats m, double* zend,
                                                                                   double* __restrict__ start, double* gtot, double* carry) {
    const LoudClip c = d.clip[blockIdx.x];
    const int ch = blockIdx.y;
    if (ch >= c.channels) return;
    const long chunks = (c.n + LOUD_CHUNK - 1) / LOUD_CHUNK;
    const long groups = (chunks + 63) / 64;
    const long base = (long)c.part + (long)ch * chunks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long g = wave; g < groups; g += LOUD_THREADS / 64) {
        const long kk = 64 * g + lane;
        double z[4] = {0., 0., 0., 0.};
        if (kk < chunks) {
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = zend[4 * (base + kk) + i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v[4], r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __shfl_up(z[e], 1u << i, 64);
            kw_matvec_add(m.p[i], v, z, r);
            if (lane >= (1 << i)) {
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = r[e];
            }
        }
        if (kk < chunks) {
#pragma unroll
            for (int i = 0; i < 4; ++i) zend[4 * (base + kk) + i] = z[i];
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < 4; ++i) gtot[4 * (base + g) + i] = z[i];
        }
    }
    __syncthreads();                                            // (the block's own stores, before any of its threads reads them)
    if (wave == 0) {
        double run[4] = {0., 0., 0., 0.};
        for (long g0 = 0; g0 < groups; g0 += 64) {
            double t[4] = {0., 0., 0., 0.}, mine[4] = {0., 0., 0., 0.};
            if (g0 + lane < groups) {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = gtot[4 * (base + g0 + lane) + i];
            }
            for (int j = 0; j < 64; ++j) {
                double v[4], r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (lane == j) mine[e] = run[e];
                    v[e] = __shfl(t[e], j, 64);
                }
                kw_matvec_add(m.p[6], run, v, r);
#pragma unroll
                for (int e = 0; e < 4; ++e) run[e] = r[e];
            }
            if (g0 + lane < groups) {
#pragma unroll
                for (int i = 0; i < 4; ++i) carry[4 * (base + g0 + lane) + i] = mine[i];
            }
        }
    }
    __syncthreads();
    const double zero[4] = {0., 0., 0., 0.};
    for (long g = wave; g < groups; g += LOUD_THREADS / 64) {
        const long kk = 64 * g + lane;
        if (kk >= chunks) continue;
        double v[4], left[4] = {0., 0., 0., 0.};
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = carry[4 * (base + g) + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) {                           // M^l carry, l in binary
            double r[4];
            kw_matvec_add(m.p[i], v, zero, r);
            if ((lane >> i) & 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = r[e];
            }
        }
        if (lane > 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) left[i] = zend[4 * (base + kk - 1) + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) start[4 * (base + kk) + i] = v[i] + left[i];
    }
}

// grid (B), LOUD_THREADS threads: block b turns clip b's partials into segment sums, block energies, the two gates and out[0..3);
// with scales, scales[b] = fp32(10^((L - target) / 20)) for a finite L (the value stored in out[0]), else 1
template <class D> __global__ __launch_bounds__(LOUD_THREADS) void loud_gate_kernel(const D d, int fs, const double* __restrict__ part2,
                                                                                   double* seg, double* zblk, float* __restrict__ scales,
                                                                                   double target) {
    const LoudClip c = d.clip[blockIdx.x];
    const LoudGated g = loud_gate_clip(c, fs, part2, seg, zblk);
    if (threadIdx.x != 0) return;
    const float L = loud_store_triple(g, c.out);
    if (scales) scales[blockIdx.x] = g.count > 0 ? (float)exp10(((double)L - target) / 20.) : 1.f;
}

// grid (ceil(B / LOUD_THREADS)): the true-peak ceiling on the divisor of a clip with a loudness (its gated blocks, out[2], are not 0):
// scales[b] = max(scales[b], fp32((double)true_peaks[2 b] / ceiling))
template <class D> __global__ __launch_bounds__(LOUD_THREADS) void loud_ceiling_kernel(const D d, int B, const float* __restrict__ true_peaks,
                                                                                      double ceiling, float* __restrict__ scales) {
    const int b = blockIdx.x * LOUD_THREADS + threadIdx.x;
    if (b >= B) return;
    if (((global_ptr<const float>)d.clip[b].out)[2] == 0.f) return;
    scales[b] = fmaxf(scales[b], (float)((double)true_peaks[2 * b] / ceiling));
}

// grid (ceil(max n / LOUD_SPAN), B): x[i] = x[i] / scales[b] over clip b's n samples; a row whose divisor is 1 is not touched
template <class D> __global__ __launch_bounds__(LOUD_THREADS) void loud_apply_kernel(const D d, const float* __restrict__ scales) {
    const LoudClip c = d.clip[blockIdx.y];
    const long i = (long)blockIdx.x * LOUD_SPAN + 4 * (long)threadIdx.x;
    const float div = scales[blockIdx.y];
    if (i >= c.n || div == 1.f) return;
    const global_ptr<float> x = (global_ptr<float>)const_cast<float*>(c.x);
    if (i + 4 <= c.n && (uintptr_t)(c.x + i) % 16 == 0) {
        ld_f32x4 w = *(global_ptr<ld_f32x4>)(x + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = __fdiv_rn(w[e], div);
        *(global_ptr<ld_f32x4>)(x + i) = w;
        return;
    }
    for (int e = 0; e < 4 && i + e < c.n; ++e) x[i + e] = __fdiv_rn(x[i + e], div);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------

bool loud_rate_ok(int fs) { return fs >= 8000 && fs <= 192000; }

// The K-weighting of rate fs as the bilinear transforms of its two analogue prototypes, in double
static KwCoef kw_coefficients(int fs) {
    const double pi = 3.14159265358979323846;
    KwCoef k;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)fs), Vh = std::pow(10., G / 20.), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1. + K / Q + K * K;
        k.c[0] = (Vh + Vb * K / Q + K * K) / a0;
        k.c[1] = 2. * (K * K - Vh) / a0;
        k.c[2] = (Vh - Vb * K / Q + K * K) / a0;
        k.c[3] = 2. * (K * K - 1.) / a0;
        k.c[4] = (1. - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)fs);
        const double a0 = 1. + K / Q + K * K;
        k.c[5] = 1.;
        k.c[6] = -2.;
        k.c[7] = 1.;
        k.c[8] = 2. * (K * K - 1.) / a0;
        k.c[9] = (1. - K / Q + K * K) / a0;
    }
    return k;
}

static void mat_mul(const double* a, const double* b, double* out) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.;
            for (int e = 0; e < 4; ++e) s += a[4 * i + e] * b[4 * e + j];
            r[4 * i + j] = s;
        }
    memcpy(out, r, sizeof r);
}

// M = A^LOUD_CHUNK and its powers: A's columns are one step of kw_step on the unit states with x = 0; LOUD_CHUNK is a power of two
static KwMats kw_matrices(const KwCoef& k) {
    static_assert((LOUD_CHUNK & (LOUD_CHUNK - 1)) == 0 && LOUD_CHUNK <= 800 && LOUD_CHUNK % LOUD_TILE == 0, "LOUD_CHUNK");
    double a[16];
    for (int j = 0; j < 4; ++j) {
        double s[4] = {0., 0., 0., 0.};
        s[j] = 1.;
        kw_step(k, s, 0.);
        for (int i = 0; i < 4; ++i) a[4 * i + j] = s[i];
    }
    for (int c = 1; c < LOUD_CHUNK; c <<= 1) mat_mul(a, a, a);
    KwMats m;
    memcpy(m.p[0], a, sizeof a);
    for (int i = 1; i < 7; ++i) mat_mul(m.p[i - 1], m.p[i - 1], m.p[i]);
    return m;
}

static size_t loud_descriptor_bytes(int B) { return (size_t)B * sizeof(LoudClip); }

// The descriptors checked and turned into their device form; slots: the chunk slots the call needs, max_n: its longest clip
int loud_prepare(const std::string& fn, const wt_loudness_clip* clips, int B, int fs, const void* workspace, std::vector<LoudClip>& dev,
                 int64_t& slots, int64_t& max_n, int& max_ch) {
    if (!clips || !workspace || B < 1 || B > 65535) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (!loud_rate_ok(fs)) { set_error(fn + ": sample_rate outside [8000, 192000]"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    dev.resize((size_t)B);
    slots = 0;
    max_n = 0;
    max_ch = 1;
    for (int b = 0; b < B; ++b) {
        const wt_loudness_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.x) { set_error(who + "null source"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null destination"); return WT_ERR_INVALID; }
        if (c.n < 1) { set_error(who + "n < 1"); return WT_ERR_INVALID; }
        if (c.channels != 1 && c.channels != 2) { set_error(who + "channels must be 1 or 2"); return WT_ERR_INVALID; }
        if (c.channels == 2 && c.channel_stride < c.n) { set_error(who + "channel_stride < n"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.x) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float) ||
            reinterpret_cast<uintptr_t>(c.blocks) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        if (slots > 0x7fffffffLL) { set_error(fn + ": too many samples for one call"); return WT_ERR_INVALID; }
        dev[b] = LoudClip{c.x, (long)c.n, c.channels == 2 ? (long)c.channel_stride : 0L, c.out, c.blocks, (int)slots, c.channels};
        slots += (int64_t)c.channels * ((c.n + LOUD_CHUNK - 1) / LOUD_CHUNK);
        max_n = std::max<int64_t>(max_n, c.n);
        max_ch = std::max(max_ch, (int)c.channels);
    }
    if (slots > 0x7fffffffLL) { set_error(fn + ": too many samples for one call"); return WT_ERR_INVALID; }
    return WT_OK;
}

// The chunk states' place behind the descriptors' (zend, start, gtot, carry: 4 doubles per slot each), then loud_buffers'
static double* loud_states(void* workspace, int B) { return reinterpret_cast<double*>(static_cast<char*>(workspace) + loud_descriptor_bytes(B)); }

LoudBuffers loud_buffers(void* workspace, int B, int64_t slots) {
    double* part2 = loud_states(workspace, B) + 16 * slots;
    return LoudBuffers{part2, part2 + 2 * slots, part2 + 3 * slots};
}

// The launches of a call on one descriptor source: the K-weighting's three, then (gate) the gating and, with scales, the ceiling
// (with true_peaks) and the gain
static int loud_launches(const char* fn, const std::vector<LoudClip>& dev, int64_t slots, int64_t max_n, int max_ch, int fs, void* workspace,
                         hipStream_t s, bool gate, float* scales, double target, const float* true_peaks, double ceiling) {
    const int B = (int)dev.size();
    const KwCoef k = kw_coefficients(fs);
    const KwMats m = kw_matrices(k);
    double* zend = loud_states(workspace, B);
    double* start = zend + 4 * slots;
    double* gtot = start + 4 * slots;
    double* carry = gtot + 4 * slots;
    const LoudBuffers w = loud_buffers(workspace, B, slots);
    double* part2 = w.part2;
    const int64_t max_chunks = (max_n + LOUD_CHUNK - 1) / LOUD_CHUNK;
    const dim3 walk((unsigned)((max_chunks + 63) / 64), (unsigned)B, (unsigned)max_ch);
    const dim3 span((unsigned)((max_n + LOUD_SPAN - 1) / LOUD_SPAN), (unsigned)B);
    if (int rc = launch_ragged<LOUD_ARG_CLIPS>(fn, dev.data(), B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL((loud_walk_kernel<decltype(d), false>), walk, dim3(64), 0, s, d, k, fs, zend, start, part2);
        hipLaunchKernelGGL(loud_scan_kernel<decltype(d)>, dim3((unsigned)B, (unsigned)max_ch), dim3(LOUD_THREADS), 0, s, d, m, zend, start, gtot,
                           carry);
        hipLaunchKernelGGL((loud_walk_kernel<decltype(d), true>), walk, dim3(64), 0, s, d, k, fs, zend, start, part2);
        if (!gate) return;
        hipLaunchKernelGGL(loud_gate_kernel<decltype(d)>, dim3((unsigned)B), dim3(LOUD_THREADS), 0, s, d, fs, part2, w.seg, w.zblk, scales, target);
        if (scales && true_peaks)
            hipLaunchKernelGGL(loud_ceiling_kernel<decltype(d)>, dim3((unsigned)((B + LOUD_THREADS - 1) / LOUD_THREADS)), dim3(LOUD_THREADS), 0, s, d,
                               B, true_peaks, ceiling, scales);
        if (scales) hipLaunchKernelGGL(loud_apply_kernel<decltype(d)>, span, dim3(LOUD_THREADS), 0, s, d, scales);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

int loud_launch(const char* fn, const std::vector<LoudClip>& dev, int64_t slots, int64_t max_n, int max_ch, int fs, void* workspace,
                hipStream_t s, float* scales, double target, const float* true_peaks, double ceiling) {
    return loud_launches(fn, dev, slots, max_n, max_ch, fs, workspace, s, true, scales, target, true_peaks, ceiling);
}

int loud_filter_launch(const char* fn, const std::vector<LoudClip>& dev, int64_t slots, int64_t max_n, int max_ch, int fs, void* workspace,
                       hipStream_t s) {
    return loud_launches(fn, dev, slots, max_n, max_ch, fs, workspace, s, false, nullptr, 0., nullptr, 1.);
}

}  // namespace wt

using namespace wt;

extern "C" {

int32_t wt_loudness_chunk(void) { return LOUD_CHUNK; }

int64_t wt_loudness_blocks(int64_t n, int32_t sample_rate) {
    if (n < 1 || !loud_rate_ok(sample_rate)) return 0;
    return loud_blocks((long)n, sample_rate);
}

int wt_kweight_coefficients(int32_t sample_rate, double* out) {
    if (!out || !loud_rate_ok(sample_rate)) { set_error("wt_kweight_coefficients: null out or sample_rate outside [8000, 192000]"); return WT_ERR_INVALID; }
    const KwCoef k = kw_coefficients(sample_rate);
    memcpy(out, k.c, sizeof k.c);
    return WT_OK;
}

size_t wt_loudness_workspace_bytes(int32_t B, int64_t total_samples) {
    if (B < 1 || total_samples < 1) return 0;
    const size_t slots = (size_t)(total_samples / LOUD_CHUNK) + 2 * (size_t)B;      // >= sum of channels_b * ceil(n_b / LOUD_CHUNK)
    return loud_descriptor_bytes(B) + LOUD_SLOT_DOUBLES * slots * sizeof(double) + 8;
}

int wt_loudness(const wt_loudness_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream) {
    std::vector<LoudClip> dev;
    int64_t slots = 0, max_n = 0;
    int max_ch = 1;
    if (int rc = loud_prepare("wt_loudness", clips, B, sample_rate, workspace, dev, slots, max_n, max_ch)) return rc;
    return loud_launch("wt_loudness", dev, slots, max_n, max_ch, sample_rate, workspace, static_cast<hipStream_t>(stream), nullptr, 0.);
}

size_t wt_normalize_rows_lufs_workspace_bytes(int32_t B, int64_t T_pad) {
    if (B < 1 || T_pad < 1) return 0;
    return wt_loudness_workspace_bytes(B, (int64_t)B * T_pad) + 4 * (size_t)B * sizeof(float);
}

int wt_normalize_rows_lufs(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t sample_rate, double target_lufs, float* scales,
                           void* workspace, void* stream) {
    const std::string fn = "wt_normalize_rows_lufs";
    if (!rows || !n || !scales || !workspace || B < 1 || B > 65535 || T_pad < 1) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(rows) % sizeof(float) || reinterpret_cast<uintptr_t>(scales) % sizeof(float)) {
        set_error(fn + ": rows or scales misaligned"); return WT_ERR_INVALID;
    }
    if (!std::isfinite(target_lufs)) { set_error(fn + ": target_lufs must be finite"); return WT_ERR_INVALID; }
    if (!loud_rate_ok(sample_rate)) { set_error(fn + ": sample_rate outside [8000, 192000]"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    // the rows' results lie behind the measurement's own workspace (sized for B rows of T_pad samples)
    float* stats = reinterpret_cast<float*>(static_cast<char*>(workspace) + wt_loudness_workspace_bytes(B, (int64_t)B * T_pad));
    std::vector<wt_loudness_clip> clips((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (n[b] < 1 || n[b] > T_pad) { set_error(fn + ": row " + std::to_string(b) + ": n outside [1, T_pad]"); return WT_ERR_INVALID; }
        clips[b] = wt_loudness_clip{rows + (int64_t)b * T_pad, n[b], 1, 0, stats + 4 * b, nullptr};
    }
    std::vector<LoudClip> dev;
    int64_t slots = 0, max_n = 0;
    int max_ch = 1;
    if (int rc = loud_prepare(fn, clips.data(), B, sample_rate, workspace, dev, slots, max_n, max_ch)) return rc;
    return loud_launch("wt_normalize_rows_lufs", dev, slots, max_n, max_ch, sample_rate, workspace, static_cast<hipStream_t>(stream), scales,
                       target_lufs);
}

}  // extern "C"
