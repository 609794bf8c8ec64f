// The short-time objective intelligibility measure and its extended form on the GPU (STOI: Taal, Hendriks, Heusdens & Jensen 2011;
// ESTOI: Jensen & Taal 2016): what the reference's evaluation script computes per file on the CPU with pystoi
// (metrics/infer.py:100-105).  include/wavtokenizer_amd.h states the definition; pystoi is not available to this project's tests, so
// like the mel transform (mel.hip) the parity with it is unpinned: tests/stoi_ref.py holds the definition in float64 and the
// kernels are checked against that.
//
// Six launches per call, all ragged over the call's clips (one clip per blockIdx.y, or per block):
//   stoi_resample_kernel   both signals to 10 kHz: polyphase FIR, one output sample per lane, taps in ascending order (the filter and
//                          the block's stretch of input in LDS where the filter fits: stoi_resample_lds_kernel, the same bits)
//   stoi_energy_kernel     sum of squares of every windowed candidate frame of the clean signal: one wave per frame
//   stoi_select_kernel     per clip: the largest frame, the keep test, the list of kept frames by an exclusive prefix sum
//   stoi_band_kernel       one wave per frame of the silence-removed signals: the frame is gathered through the list of kept
//                          frames (the overlap-added signal is never stored), 512-point real FFT, 15 one-third-octave bands
//   stoi_segment_kernel    one half-wave per 30-frame segment: the 15 x 30 blocks in registers, one partial per segment
//   stoi_mean_kernel       a clip's partials added in a fixed order, one division
// The number of kept frames K never comes back to the host: grids are sized by the candidate-frame count K0 and waves past K leave
// at once.  fp32 throughout, no float atomics, every summation order depends on the clip alone: a clip has the same bits alone, in
// any batch and at any position.  As in mel.hip the two signals of a pair never share a complex transform.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

// (tests/test_stoi_host.py mirrors this layout in ctypes to hand the calls a handle without a GPU: keep the two in step)
struct wt_stoi_handle {
    int device = 0;
    int sample_rate = 0;
    int p = 0, q = 0, L = 0;                    // 10000 / g, sample_rate / g; the filter has 2 L + 1 taps
    float* tab = nullptr;                       // one device block: window | twiddles | phase table | filter
};

// sums and products must not depend on the kernel a device function is inlined into: no contraction by the compiler, fmaf where wanted
// (over fft.h's functions too: the pragma stands before the include)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int STOI_FS = 10000, STOI_FRAME = 256, STOI_HOP = 128, STOI_BANDS = 15, STOI_SEG = 30;
constexpr int STOI_MAX_RATIO = 441;             // the larger of p and q
constexpr int STOI_WAVES = 4;                   // frames per workgroup of the energy and band kernels: one per wave
constexpr float STOI_EPS = 2.220446049250313e-16f;          // 2^-52
constexpr float STOI_CLIP = 6.623413251903491f;              // 1 + 10^(15 / 20)
constexpr float STOI_RANGE = 0.01f;                          // 40 dB
constexpr float STOI_SHORT = 1e-5f;
// layout of wt_stoi_handle::tab, in 4-byte words
constexpr int STOI_TAB_WIN = 0;                              // [256] hanning(258)[1:-1]
constexpr int STOI_TAB_TW = STOI_TAB_WIN + STOI_FRAME;       // [512][2] (cos, -sin)(2 pi n / 512)
constexpr int STOI_TAB_PHASE = STOI_TAB_TW + 2 * 512;        // int [448]: first tap of output sample n, by n mod p
constexpr int STOI_TAB_H = STOI_TAB_PHASE + 448;             // [2 L + 1]

// band i sums bins [EDGE[i], EDGE[i + 1])
__constant__ int STOI_EDGE[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
static const int STOI_EDGE_HOST[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// One clip of a call (device form of wt_stoi_clip)
struct StoiClip {
    const float* clean;
    const float* proc;
    float* res;                                 // the resampled pair, clean then processed, n samples each (null at 10 kHz)
    const float* xr;                            // the 10 kHz signals the later stages read: res, or the inputs themselves
    const float* yr;
    float* out;
    long T, n, K0;                              // input samples, samples at 10 kHz, candidate frames
    long foff;                                  // the clip's first entry in the per-frame arrays
};

// The per-frame arrays of a call; clip c owns [foff, foff + K0) of each, and 30 times that of tob
struct StoiWs {
    float* energy;                              // [K0] sum of squares of the windowed candidate frames
    int* idx;                                   // [K] the kept frames, ascending
    int* counts;                                // [B][2] (K0, K)
    int* keep;                                  // [K0] 0 / 1, or null
    float* tob;                                 // [2][15][K0]: (clean, processed), band, frame j < K - 1
    float* part;                                // [K - 30] one partial per segment
};

struct StoiTab {
    const float* tab;
    int p, q, L;
};

constexpr int STOI_ARG_CLIPS = 32;           // descriptors up to this many travel in the launches' argument blocks (ragged.h)

// 256 complex points as two float planes: point i sits at word swz(i).  Every store of the four passes (strides 4, 16 and 64 between
// a lane's points, lanes 1, 4-with-gaps and 16-with-gaps apart) and every stride-1 load then meets each of the 32 banks once per
// 32-lane half; the split pass's mirrored load alone keeps a two-way conflict (python3 tools/lds_banks.py stoi)
__device__ __forceinline__ int stoi_swz(int i) { return i ^ ((i >> 5) & 3) ^ (((i >> 5) & 3) << 2) ^ (((i >> 6) & 1) << 4); }

// y[n] = sum over the taps k = k0, k0 + p, ... <= 2 L of h[k] x[(n q + L - k) / p], k0 = (n q + L) mod p, the input index within
// [0, T): scipy.signal.resample_poly(x, p, q, window = h / p) written out.  grid (ceil(max n / 256), 2 B): signal blockIdx.y & 1
__device__ __forceinline__ void stoi_resample_block(const StoiClip& c, const StoiTab& tb) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= c.n) return;
    const int sig = blockIdx.y & 1;
    const global_ptr<const float> x = (global_ptr<const float>)(sig ? c.proc : c.clean);
    const global_ptr<const float> h = (global_ptr<const float>)(tb.tab + STOI_TAB_H);
    const global_ptr<const int> phase = (global_ptr<const int>)(tb.tab + STOI_TAB_PHASE);
    const long pos = n * tb.q + tb.L;           // the output sample's place among the zero-stuffed input, shifted by L
    const int k0 = phase[n % tb.p];
    const long i0 = (pos - k0) / tb.p;          // tap k0 + p j meets input sample i0 - j
    const long jlo = i0 > c.T - 1 ? i0 - (c.T - 1) : 0;
    const long kmax = pos < 2L * tb.L ? pos : 2L * tb.L;
    const long jhi = kmax >= k0 ? (kmax - k0) / tb.p : -1;      // k <= 2 L, and k <= pos keeps the input index >= 0
    float acc = 0.f;
    for (long j = jlo; j <= jhi; ++j) acc = fmaf(h[k0 + tb.p * j], x[i0 - j], acc);
    ((global_ptr<float>)c.res)[(long)sig * c.n + n] = acc;
}

// The same sums, tap for tap, with the filter and the block's stretch of the input in LDS (rates whose filter fits: the host
// decides per handle, never per call, and the bits are the same either way).  Output n reads input samples
// [i0(n) - 2 L / p, i0(n)], i0(n) = (n q + L) / p, so the block's 256 outputs read [i0(first) - 2 L / p, i0(last)] within [0, T).
// Dynamic LDS: h [2 L + 1] | x [span]
__device__ __forceinline__ void stoi_resample_lds_block(const StoiClip& c, const StoiTab& tb) {
    extern __shared__ float stoi_sm[];
    const long n0 = (long)blockIdx.x * 256;
    if (n0 >= c.n) return;                                      // (the whole block: no barrier is left waiting)
    const int sig = blockIdx.y & 1;
    const global_ptr<const float> x = (global_ptr<const float>)(sig ? c.proc : c.clean);
    const global_ptr<const float> h = (global_ptr<const float>)(tb.tab + STOI_TAB_H);
    const global_ptr<const int> phase = (global_ptr<const int>)(tb.tab + STOI_TAB_PHASE);
    const int taps = 2 * tb.L + 1;
    float* sh = stoi_sm;
    float* sx = stoi_sm + taps;
    const long nlast = n0 + 255 < c.n ? n0 + 255 : c.n - 1;
    long lo = (n0 * tb.q + tb.L) / tb.p - 2 * tb.L / tb.p, hi = (nlast * tb.q + tb.L) / tb.p;
    if (lo < 0) lo = 0;
    if (hi > c.T - 1) hi = c.T - 1;
    for (int t = threadIdx.x; t < taps; t += 256) sh[t] = h[t];
    for (long t = threadIdx.x; t <= hi - lo; t += 256) sx[t] = x[lo + t];
    __syncthreads();
    const long n = n0 + threadIdx.x;
    if (n >= c.n) return;
    const long pos = n * tb.q + tb.L;
    const int k0 = phase[n % tb.p];
    const long i0 = (pos - k0) / tb.p;
    const long jlo = i0 > c.T - 1 ? i0 - (c.T - 1) : 0;
    const long kmax = pos < 2L * tb.L ? pos : 2L * tb.L;
    const long jhi = kmax >= k0 ? (kmax - k0) / tb.p : -1;
    float acc = 0.f;
    const float* xs = sx + (i0 - lo);
    for (long j = jlo; j <= jhi; ++j) acc = fmaf(sh[k0 + tb.p * j], xs[-j], acc);
    ((global_ptr<float>)c.res)[(long)sig * c.n + n] = acc;
}

// energy[f] = sum over the frame of (w x)^2: lane l adds samples l, l + 64, l + 128, l + 192 in that order, the xor butterfly adds the
// lanes.  grid (ceil(max K0 / 4), B)
__device__ __forceinline__ void stoi_energy_block(const StoiClip& c, const StoiTab& tb, const StoiWs& ws) {
    const int lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * STOI_WAVES + (threadIdx.x >> 6);
    if (f >= c.K0) return;
    const global_ptr<const float> x = (global_ptr<const float>)c.xr + f * STOI_HOP;
    const global_ptr<const float> win = (global_ptr<const float>)(tb.tab + STOI_TAB_WIN);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = win[lane + 64 * r] * x[lane + 64 * r];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) ws.energy[c.foff + f] = s;
}

// One workgroup per clip: a frame is kept when ||w x_f|| + EPS > 0.01 (max ||w x_f|| + EPS).  The kept frames' indices go to idx in
// ascending order: 256 frames at a time, a frame's place is the count of kept frames before it (ballot within the wave, the waves'
// totals through LDS, the chunks' through a running base: integers, so no order matters).
__device__ __forceinline__ void stoi_select_block(const StoiClip& c, const StoiWs& ws, int clip) {
    __shared__ float wmax[4];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const global_ptr<const float> energy = (global_ptr<const float>)(ws.energy + c.foff);
    float m = 0.f;
    for (long f = tid; f < c.K0; f += 256) m = fmaxf(m, energy[f]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float thr = STOI_RANGE * (sqrtf(m) + STOI_EPS);
    int base = 0;
    for (long f0 = 0; f0 < c.K0; f0 += 256) {
        const long f = f0 + tid;
        const bool keep = f < c.K0 && sqrtf(energy[f < c.K0 ? f : 0]) + STOI_EPS > thr;
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                        // (the previous chunk's totals have been read)
        if (lane == 0) wtot[wave] = __popcll(mask);
        __syncthreads();
        int at = base + before;
        for (int w = 0; w < wave; ++w) at += wtot[w];
        if (keep) ws.idx[c.foff + at] = (int)f;
        if (ws.keep && f < c.K0) ws.keep[c.foff + f] = keep ? 1 : 0;
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    }
    if (tid == 0) {
        ws.counts[2 * clip] = (int)c.K0;
        ws.counts[2 * clip + 1] = base;
    }
}

// Frame j of the silence-removed signal x (the 10 kHz signal, frames listed in idx, K of them; 0 <= j < K - 1): the band magnitudes
// of its 512-point real FFT go to tob[band][j] (row stride K0).  Sample t of the frame is w[t] times the overlap-add of the kept
// windowed frames at 128 j + t: kept frames j - 1 (t < 128, j > 0) and j, or j and j + 1 (t >= 128), the earlier frame's term first.
// The 256 samples and 256 zeros are the 256 complex points z[i] = f[2 i] + i f[2 i + 1], transformed by a radix-4 Stockham FFT (four
// passes, four points per lane) and split into the bins of the real transform.  zr, zi [256] and S [256] are the calling wave's own
// LDS; every wave of the block makes the call (the barriers are the block's).
__device__ __forceinline__ void stoi_frame(global_ptr<const float> x, global_ptr<const int> idx, long j, const StoiTab& tb, float* zr,
                                           float* zi, float* S, int lane, bool store, global_ptr<float> tob, long K0) {
    const global_ptr<const float> win = (global_ptr<const float>)(tb.tab + STOI_TAB_WIN);
    const global_ptr<const f32x2> tw = (global_ptr<const f32x2>)(tb.tab + STOI_TAB_TW);
    f32x2 v[4];
    {
        const global_ptr<const float> cur = x + (long)idx[j] * STOI_HOP;
        const global_ptr<const float> nxt = x + (long)idx[j + 1] * STOI_HOP;
        const int t = 2 * lane;                 // samples t, t + 1 (first half) and t + 128, t + 129 (second half)
        const f32x2 w0 = *(global_ptr<const f32x2>)(win + t), w1 = *(global_ptr<const f32x2>)(win + t + STOI_HOP);
        f32x2 a = f32x2{w0.x * cur[t], w0.y * cur[t + 1]};
        if (j > 0) {
            const global_ptr<const float> prv = x + (long)idx[j - 1] * STOI_HOP;
            a = f32x2{w1.x * prv[t + STOI_HOP], w1.y * prv[t + STOI_HOP + 1]} + a;
        }
        const f32x2 b = f32x2{w1.x * cur[t + STOI_HOP], w1.y * cur[t + STOI_HOP + 1]} + f32x2{w0.x * nxt[t], w0.y * nxt[t + 1]};
        v[0] = w0 * a;
        v[1] = w1 * b;
        v[2] = f32x2{0.f, 0.f};
        v[3] = f32x2{0.f, 0.f};
    }
    // pass 1 (sub-transform length 1): no twiddles; output q of lane's butterfly goes to point 4 lane + q
    bfly4(v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int o = stoi_swz(4 * lane + q);
        zr[o] = v[rev2(q)].x;
        zi[o] = v[rev2(q)].y;
    }
    __syncthreads();
    // passes 2-4 (length Ls = 4, 16, 64): k = lane % Ls, twiddle exp(-2 pi i r k / (4 Ls)); output q goes to 4 Ls (lane / Ls) + k + Ls q
#pragma unroll
    for (int ls = 2; ls <= 6; ls += 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = stoi_swz(lane + 64 * r);
            v[r] = f32x2{zr[o], zi[o]};
        }
        const int k = lane & ((1 << ls) - 1);
#pragma unroll
        for (int r = 1; r < 4; ++r) v[r] = cmul(v[r], tw[(r * k) << (7 - ls)]);
        bfly4(v[0], v[1], v[2], v[3]);
        const int j0 = ((lane >> ls) << (ls + 2)) + k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = stoi_swz(j0 + (q << ls));
            zr[o] = v[rev2(q)].x;
            zi[o] = v[rev2(q)].y;
        }
        __syncthreads();
    }
    // split pass: X[k] = (Z[k] + conj Z[256 - k]) / 2 - i / 2 exp(-2 pi i k / 512) (Z[k] - conj Z[256 - k]); the bands need k in [7, 219)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        if (k >= 7 && k < 219) {
            const int o = stoi_swz(k), om = stoi_swz(256 - k);
            S[k] = cpower(real_split_bin(f32x2{zr[o], zi[o]}, f32x2{zr[om], zi[om]}, tw[k]));
        }
    }
    __syncthreads();
    // bands: lane b adds its bins' powers in ascending order
    if (lane < STOI_BANDS) {
        float acc = 0.f;
        for (int k = STOI_EDGE[lane]; k < STOI_EDGE[lane + 1]; ++k) acc += S[k];
        if (store) tob[(long)lane * K0 + j] = sqrtf(acc);
    }
}

// grid (ceil((max K0 - 1) / 4), B), 256 threads: wave w of block (x, b) takes frame 4 x + w of clip b, the clean signal and then the
// processed one
__device__ __forceinline__ void stoi_band_block(const StoiClip& c, const StoiTab& tb, const StoiWs& ws, int clip) {
    __shared__ float lds[STOI_WAVES][3 * 256];
    const long J = (long)ws.counts[2 * clip + 1] - 1;
    const long j0 = (long)blockIdx.x * STOI_WAVES;
    if (j0 >= J) return;                                        // (the whole block: no barrier is left waiting)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long j = j0 + wave;
    const bool valid = j < J;
    const long jr = valid ? j : J - 1;                          // a wave past the last frame keeps the barriers company
    float* zr = lds[wave];
    const global_ptr<const int> idx = (global_ptr<const int>)(ws.idx + c.foff);
    const global_ptr<float> tob = (global_ptr<float>)(ws.tob + 2 * STOI_BANDS * c.foff);
    stoi_frame((global_ptr<const float>)c.xr, idx, jr, tb, zr, zr + 256, zr + 512, lane, valid, tob, c.K0);
    stoi_frame((global_ptr<const float>)c.yr, idx, jr, tb, zr, zr + 256, zr + 512, lane, valid, tob + STOI_BANDS * c.K0, c.K0);
}

// a row of 30 values, one per lane of a 32-lane group (lanes 30 and 31 hold 0 and stay 0): minus its mean, over (its norm + EPS)
__device__ __forceinline__ float stoi_rownorm(float v, bool live) {
    const float mean = half_sum(v) / (float)STOI_SEG;
    v = live ? v - mean : 0.f;
    const float nrm = sqrtf(half_sum(v * v));
    return v / (nrm + STOI_EPS);
}

// Segment s of a clip (frames [s, s + 30) of tob, s < J - 29) on one 32-lane half of a wave: lane f holds the 15 band values of
// frame s + f of both signals; sums over a row's 30 frames are xor butterflies within the half, sums over the 15 bands run in the
// lane in ascending order.  grid (ceil((max K0 - 30) / 8), B), 256 threads.
//   STOI:  per band  alpha = ||X|| / (||Y|| + EPS),  Y' = min(alpha Y, X (1 + 10^(15/20))),  partial = sum over the bands of the
//          correlation of the row-normalised X and Y'
//   ESTOI: rows normalised, then every frame's column of 15 normalised the same way; partial = sum over the frames of the columns'
//          correlations
__device__ __forceinline__ void stoi_segment_block(const StoiClip& c, const StoiWs& ws, int clip, int extended) {
    const long nseg = (long)ws.counts[2 * clip + 1] - 1 - (STOI_SEG - 1);
    const long s = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (s >= nseg) return;                                      // (a whole 32-lane group; the butterflies stay within it)
    const int f = threadIdx.x & 31;
    const bool live = f < STOI_SEG;
    const global_ptr<const float> tx = (global_ptr<const float>)(ws.tob + 2 * STOI_BANDS * c.foff) + s + (live ? f : 0);
    const global_ptr<const float> ty = tx + STOI_BANDS * c.K0;
    float x[STOI_BANDS], y[STOI_BANDS];
#pragma unroll
    for (int b = 0; b < STOI_BANDS; ++b) {
        x[b] = live ? tx[(long)b * c.K0] : 0.f;
        y[b] = live ? ty[(long)b * c.K0] : 0.f;
    }
    float part;
    if (!extended) {
        float acc = 0.f;
#pragma unroll
        for (int b = 0; b < STOI_BANDS; ++b) {
            const float nx = sqrtf(half_sum(x[b] * x[b])), ny = sqrtf(half_sum(y[b] * y[b]));
            const float alpha = nx / (ny + STOI_EPS);
            const float yp = fminf(alpha * y[b], x[b] * STOI_CLIP);
            acc += half_sum(stoi_rownorm(x[b], live) * stoi_rownorm(yp, live));
        }
        part = acc;
    } else {
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int b = 0; b < STOI_BANDS; ++b) {
            x[b] = stoi_rownorm(x[b], live);
            y[b] = stoi_rownorm(y[b], live);
            sx += x[b];
            sy += y[b];
        }
        const float mx = sx / (float)STOI_BANDS, my = sy / (float)STOI_BANDS;
        float qx = 0.f, qy = 0.f;
#pragma unroll
        for (int b = 0; b < STOI_BANDS; ++b) {
            x[b] -= mx;
            y[b] -= my;
            qx += x[b] * x[b];
            qy += y[b] * y[b];
        }
        const float dx = sqrtf(qx) + STOI_EPS, dy = sqrtf(qy) + STOI_EPS;
        float acc = 0.f;
#pragma unroll
        for (int b = 0; b < STOI_BANDS; ++b) acc += (x[b] / dx) * (y[b] / dy);
        part = half_sum(live ? acc : 0.f);
    }
    if (f == 0) ws.part[c.foff + s] = part;
}

// A clip's measure from its per-segment partials: lane l adds partials l, l + 64, ... in ascending order, the xor butterfly adds the
// lanes, one division by (15 or 30) times the segment count (the order mel_mean_kernel uses).  Fewer than 30 frames: 1e-5.
__device__ __forceinline__ void stoi_mean_block(const StoiClip& c, const StoiWs& ws, int clip, int extended) {
    const int lane = threadIdx.x;
    const long nseg = (long)ws.counts[2 * clip + 1] - 1 - (STOI_SEG - 1);
    float s = 0.f;
    for (long i = lane; i < nseg; i += 64) s += ws.part[c.foff + i];
    s = wave_sum(s);
    if (lane == 0) *(global_ptr<float>)c.out = nseg < 1 ? STOI_SHORT : s / ((float)(extended ? STOI_SEG : STOI_BANDS) * (float)nseg);
}

template <class D> __global__ __launch_bounds__(256) void stoi_resample_kernel(const D d, const StoiTab tb) {
    stoi_resample_block(d.clip[blockIdx.y >> 1], tb);
}
template <class D> __global__ __launch_bounds__(256) void stoi_resample_lds_kernel(const D d, const StoiTab tb) {
    stoi_resample_lds_block(d.clip[blockIdx.y >> 1], tb);
}
template <class D> __global__ __launch_bounds__(256) void stoi_energy_kernel(const D d, const StoiTab tb, const StoiWs ws) {
    stoi_energy_block(d.clip[blockIdx.y], tb, ws);
}
template <class D> __global__ __launch_bounds__(256) void stoi_select_kernel(const D d, const StoiWs ws) {
    stoi_select_block(d.clip[blockIdx.x], ws, blockIdx.x);
}
template <class D> __global__ __launch_bounds__(256) void stoi_band_kernel(const D d, const StoiTab tb, const StoiWs ws) {
    stoi_band_block(d.clip[blockIdx.y], tb, ws, blockIdx.y);
}
template <class D> __global__ __launch_bounds__(256) void stoi_segment_kernel(const D d, const StoiWs ws, int extended) {
    stoi_segment_block(d.clip[blockIdx.y], ws, blockIdx.y, extended);
}
template <class D> __global__ __launch_bounds__(64) void stoi_mean_kernel(const D d, const StoiWs ws, int extended) {
    stoi_mean_block(d.clip[blockIdx.x], ws, blockIdx.x, extended);
}

// LDS of stoi_resample_lds_kernel: the filter and the longest stretch of input 256 outputs read
constexpr size_t STOI_RESAMPLE_LDS_MAX = 48 * 1024;
static size_t stoi_resample_lds_bytes(int p, int q, int L) { return sizeof(float) * ((size_t)2 * L + 1 + 255 * (size_t)q / p + 2 * (size_t)L / p + 3); }

template <class D> static void stoi_launch(const D& d, int B, const StoiTab& tb, const StoiWs& ws, bool resample, long max_n, long max_k0,
                                           int extended, hipStream_t s) {
    if (resample) {
        const dim3 grid((unsigned)((max_n + 255) / 256), 2u * B);
        const size_t lds = stoi_resample_lds_bytes(tb.p, tb.q, tb.L);
        if (lds <= STOI_RESAMPLE_LDS_MAX) hipLaunchKernelGGL(stoi_resample_lds_kernel<D>, grid, dim3(256), lds, s, d, tb);
        else hipLaunchKernelGGL(stoi_resample_kernel<D>, grid, dim3(256), 0, s, d, tb);
    }
    hipLaunchKernelGGL(stoi_energy_kernel<D>, dim3((unsigned)((max_k0 + STOI_WAVES - 1) / STOI_WAVES), B), dim3(256), 0, s, d, tb, ws);
    hipLaunchKernelGGL(stoi_select_kernel<D>, dim3(B), dim3(256), 0, s, d, ws);
    if (max_k0 > STOI_SEG) {                    // (K0 <= 30 leaves fewer than 30 frames whatever is kept)
        hipLaunchKernelGGL(stoi_band_kernel<D>, dim3((unsigned)((max_k0 - 1 + STOI_WAVES - 1) / STOI_WAVES), B), dim3(256), 0, s, d, tb, ws);
        hipLaunchKernelGGL(stoi_segment_kernel<D>, dim3((unsigned)((max_k0 - STOI_SEG + 7) / 8), B), dim3(256), 0, s, d, ws, extended);
    }
    hipLaunchKernelGGL(stoi_mean_kernel<D>, dim3(B), dim3(64), 0, s, d, ws, extended);
}

static size_t stoi_desc_bytes(int B) { return ((size_t)B * sizeof(StoiClip) + 15) / 16 * 16; }

static bool stoi_ratio(int sample_rate, int& p, int& q, const char* who) {
    if (sample_rate < 1) { set_error(std::string(who) + ": sample_rate < 1"); return false; }
    const int g = std::gcd(STOI_FS, sample_rate);
    p = STOI_FS / g;
    q = sample_rate / g;
    if (std::max(p, q) > STOI_MAX_RATIO) {
        set_error(std::string(who) + ": 10000 / sample_rate reduces to " + std::to_string(p) + " / " + std::to_string(q) + ", beyond 441");
        return false;
    }
    return true;
}

static int stoi_filter_half(int p, int q) {
    const double fc = 1.0 / (2.0 * std::max(p, q));
    return (int)std::ceil((60.0 - 8.0) / (28.714 * fc / 10.0));
}

// the modified Bessel function I0 by its power series (the arguments here stay below 6)
static double bessel_i0(double x) {
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
    }
    return sum;
}

// The tables in float64, rounded once.  filter [2 L + 1]: kaiser(2 L + 1, 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t), t = -L..L,
// fc = 1 / (2 max(p, q)), divided by its sum and multiplied by p;  window [256]: hanning(258)[1:-1]
static void stoi_tables(int p, int q, std::vector<float>& filter, std::vector<float>& window) {
    const double pi = 3.14159265358979323846;
    const int L = stoi_filter_half(p, q);
    const double fc = 1.0 / (2.0 * std::max(p, q)), beta = 0.1102 * (60.0 - 8.7);
    std::vector<double> h((size_t)2 * L + 1);
    double sum = 0.0;
    for (int i = 0; i <= 2 * L; ++i) {
        const double t = i - L, r = t / L, a = 2.0 * fc * t;
        const double kaiser = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / bessel_i0(beta);
        h[i] = kaiser * 2.0 * p * fc * (t == 0 ? 1.0 : std::sin(pi * a) / (pi * a));
        sum += h[i];
    }
    filter.resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) filter[i] = (float)(h[i] / sum * p);
    window.resize(STOI_FRAME);
    for (int n = 0; n < STOI_FRAME; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (n + 1) / (STOI_FRAME + 1)));
}

static int64_t stoi_resampled(const wt_stoi_handle* h, int64_t T) { return (T * h->p + h->q - 1) / h->q; }
static int64_t stoi_candidates(int64_t n) { return n > STOI_FRAME ? (n - STOI_FRAME + STOI_HOP - 1) / STOI_HOP : 0; }

static bool stoi_handle_ok(const wt_stoi_handle* h) {
    if (!h->tab || h->sample_rate < 1) return false;
    const int g = std::gcd(STOI_FS, h->sample_rate);
    return h->p == STOI_FS / g && h->q == h->sample_rate / g && std::max(h->p, h->q) <= STOI_MAX_RATIO && h->L == stoi_filter_half(h->p, h->q);
}

}  // namespace wt

using namespace wt;

extern "C" {

int wt_stoi_create(int32_t sample_rate, int32_t device, wt_stoi_handle** out) {
    if (!out) { set_error("wt_stoi_create: null out"); return WT_ERR_INVALID; }
    int p = 0, q = 0;
    if (!stoi_ratio(sample_rate, p, q, "wt_stoi_create")) return WT_ERR_INVALID;
    std::vector<float> filter, window;
    stoi_tables(p, q, filter, window);
    const int L = stoi_filter_half(p, q);
    std::vector<float> tab((size_t)STOI_TAB_H + filter.size(), 0.f);
    memcpy(tab.data() + STOI_TAB_WIN, window.data(), window.size() * sizeof(float));
    fill_twiddles(tab.data() + STOI_TAB_TW, 512);
    std::vector<int32_t> phase(448, 0);
    for (int r = 0; r < p; ++r) phase[r] = (int32_t)(((int64_t)r * q + L) % p);
    memcpy(tab.data() + STOI_TAB_PHASE, phase.data(), phase.size() * sizeof(int32_t));
    memcpy(tab.data() + STOI_TAB_H, filter.data(), filter.size() * sizeof(float));
    float* dtab = nullptr;
    if (int rc = upload_table("wt_stoi_create", device, tab, &dtab)) return rc;
    wt_stoi_handle* h = new wt_stoi_handle();
    h->device = device; h->sample_rate = sample_rate; h->p = p; h->q = q; h->L = L; h->tab = dtab;
    *out = h;
    return WT_OK;
}

void wt_stoi_destroy(wt_stoi_handle* h) {
    if (!h) return;
    (void)hipFree(h->tab);
    delete h;
}

int64_t wt_stoi_resampled_length(const wt_stoi_handle* h, int64_t T) {
    if (!h || h->p < 1 || h->q < 1 || T < 0) return -1;
    return stoi_resampled(h, T);
}

int wt_stoi_tables(int32_t sample_rate, int32_t* p, int32_t* q, int32_t* L, float* filter, float* window, int32_t* edges) {
    int pp = 0, qq = 0;
    if (!stoi_ratio(sample_rate, pp, qq, "wt_stoi_tables")) return WT_ERR_INVALID;
    if (p) *p = pp;
    if (q) *q = qq;
    if (L) *L = stoi_filter_half(pp, qq);
    if (filter || window) {
        std::vector<float> f, w;
        stoi_tables(pp, qq, f, w);
        if (filter) memcpy(filter, f.data(), f.size() * sizeof(float));
        if (window) memcpy(window, w.data(), w.size() * sizeof(float));
    }
    if (edges) memcpy(edges, STOI_EDGE_HOST, sizeof(STOI_EDGE_HOST));
    return WT_OK;
}

size_t wt_stoi_workspace_bytes(const wt_stoi_handle* h, int32_t B, int64_t total_resampled, int64_t total_frames) {
    if (!h || B < 1 || total_resampled < 0 || total_frames < 0) return 0;
    // descriptors | resampled pairs | energy, idx, part and 30 band values per candidate frame | (K0, K) per clip
    return stoi_desc_bytes(B) + sizeof(float) * (2 * (size_t)total_resampled + (3 + 2 * STOI_BANDS) * (size_t)total_frames + 2 * (size_t)B);
}

int wt_stoi(const wt_stoi_handle* h, const wt_stoi_clip* clips, int32_t B, int32_t extended, void* workspace, void* stream, const wt_stoi_taps* taps) {
    const std::string fn = "wt_stoi";
    if (!ragged_call_ok(fn, h, clips, workspace, B, 32767)) return WT_ERR_INVALID;
    if (!stoi_handle_ok(h)) { set_error(fn + ": not a handle of wt_stoi_create"); return WT_ERR_INVALID; }
    if (taps && (reinterpret_cast<uintptr_t>(taps->resampled) % 4 || reinterpret_cast<uintptr_t>(taps->keep) % 4 ||
                 reinterpret_cast<uintptr_t>(taps->counts) % 4 || reinterpret_cast<uintptr_t>(taps->tob) % 4)) {
        set_error(fn + ": misaligned tap"); return WT_ERR_INVALID;
    }
    const bool resample = h->p != h->q;
    std::vector<StoiClip> dev((size_t)B);
    int64_t max_n = 0, max_k0 = 0, total_n = 0, total_k0 = 0;
    for (int b = 0; b < B; ++b) {
        const wt_stoi_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.clean) { set_error(who + "null clean"); return WT_ERR_INVALID; }
        if (!c.processed) { set_error(who + "null processed"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null out"); return WT_ERR_INVALID; }
        if (c.length < 1 || c.length > (int64_t)1 << 40) { set_error(who + "length outside 1..2^40"); return WT_ERR_INVALID; }
        const int64_t n = stoi_resampled(h, c.length), K0 = stoi_candidates(n);
        if (K0 < 1) { set_error(who + "length gives " + std::to_string(n) + " samples at 10 kHz: one frame needs more than 256"); return WT_ERR_INVALID; }
        if (K0 > 0x7fffffffLL / 8) { set_error(who + "clip too long for one launch"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.clean) % sizeof(float) || reinterpret_cast<uintptr_t>(c.processed) % sizeof(float) ||
            reinterpret_cast<uintptr_t>(c.out) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        dev[b] = StoiClip{c.clean, c.processed, nullptr, c.clean, c.processed, c.out, (long)c.length, (long)n, (long)K0, (long)total_k0};
        max_n = std::max(max_n, n);
        max_k0 = std::max(max_k0, K0);
        total_n += n;
        total_k0 += K0;
    }
    if (!on_current_device(fn, h->device)) return WT_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the workspace behind the descriptors; a tap takes the place of the workspace's own array
    float* w = reinterpret_cast<float*>(static_cast<char*>(workspace) + stoi_desc_bytes(B));
    float* res = taps && taps->resampled ? taps->resampled : w;
    w += 2 * total_n;
    StoiWs ws{};
    ws.energy = w;
    ws.idx = reinterpret_cast<int*>(w + total_k0);
    ws.part = w + 2 * total_k0;
    ws.tob = taps && taps->tob ? taps->tob : w + 3 * total_k0;
    ws.counts = taps && taps->counts ? taps->counts : reinterpret_cast<int*>(w + (3 + 2 * STOI_BANDS) * total_k0);
    ws.keep = taps ? taps->keep : nullptr;
    if (resample) {
        int64_t at = 0;
        for (int b = 0; b < B; ++b) {
            dev[b].res = res + 2 * at;
            dev[b].xr = dev[b].res;
            dev[b].yr = dev[b].res + dev[b].n;
            at += dev[b].n;
        }
    }
    const StoiTab tb{h->tab, h->p, h->q, h->L};
    if (int rc = launch_ragged<STOI_ARG_CLIPS>("wt_stoi", dev.data(), B, 2 * STOI_ARG_CLIPS, workspace, s,
                                               [&](auto d) { stoi_launch(d, B, tb, ws, resample, max_n, max_k0, extended ? 1 : 0, s); })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // extern "C"
