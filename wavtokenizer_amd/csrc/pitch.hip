// Pitch, periodicity and the voiced / unvoiced F1 on the GPU: the periodicity family of the reference's evaluation
// (metrics/periodicity.py: calculate_periodicity_metrics) with its frame grid, its A-weighted loudness gate and its three formulas,
// and with YIN (de Cheveigne & Kawahara 2002) in the place of CREPE, whose weights this project cannot carry.
// include/wavtokenizer_amd.h states the definition; tests/pitch_ref.py holds it in float64.
//
// Per call, ragged over the clips (two signals per descriptor in a pair call, grid.z):
//   pitch_yin_kernel    one wave per frame.  The frame's 1024 samples lie in the wave's LDS region; lane l owns the five lags
//                       1 + 5 l .. 5 + 5 l (320 lags over the 64 lanes; lag 321, which only the neighbour tests need, is summed
//                       across the lanes).  For a fixed j, x[j] is one address for the whole wave (a broadcast) and x[j + lag] has a
//                       stride of 5 words over the lanes: 5 is odd, so the 32 lanes of a half meet the 32 banks once each.  The
//                       difference function is added term by term in blocks of 19 of its 703 terms (703 = 19 * 37): 23 + 19 LDS
//                       reads feed 95 subtract + FMA pairs, and a lag's sum is 37 block sums added in order.  Then the prefix sum
//                       over the lags (five in the lane, a fixed scan over the lanes), d', the search and the parabola.
//                       One frame per wave and not per workgroup: 321 lags fill 64 lanes at five each with one lag over; over 256
//                       lanes they would leave three quarters of the last pass idle, and a wave needs no barrier but its own.
//   pitch_gate_kernel   one wave per frame: the frame under the periodic Hann window as 512 complex points, three radix-8 Stockham
//                       passes in fp32 (stftd.hip's 512-point layout), the split pass, the power of the 513 bins.  Mode 0 leaves
//                       the frame's largest power; mode 1 computes the transform again (nothing of a frame's 513 values is ever
//                       stored: the workspace stays O(frames)) and, with the clip's maximum known, the mean A-weighted level,
//                       then gates the frame's periodicity and pitch.
//   pitch_clipmax_kernel  one wave per signal: the maximum over its frames (exact in any order).
//   pitch_pair_kernel   one wave per pair: three sums and three counts in an order that depends on the frame count alone.
// fp32 throughout, no float atomics: a clip has the same bits alone, in any batch and at any position.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

// (tests/test_pitch_host.py mirrors this layout in ctypes to hand the calls a handle without a GPU: keep the two in step)
struct wt_pitch {
    int device = 0;
    float* tab = nullptr;                       // window [1024] | twiddles [1024][2] | A-weighting [513], one device block
};

// no product may depend on the kernel a device function is inlined into: no contraction by the compiler, fmaf where wanted
// (over fft.h's functions too: the pragma stands before the include)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int PITCH_RATE = 16000;
constexpr int PITCH_WIN = 1024, PITCH_HOP = 160;
constexpr int PITCH_MAX_LAG = 321;              // lags 1..321; 30..320 are searched, 29 and 321 are neighbours
constexpr int PITCH_TERMS = PITCH_WIN - PITCH_MAX_LAG;          // 703 terms for every lag
constexpr int PITCH_LAG_LO = 30, PITCH_LAG_HI = 320;            // ceil(16000 / 550), floor(16000 / 50)
constexpr int PITCH_BLOCK = 19, PITCH_NBLOCKS = 37;             // 703 = 19 * 37
constexpr int PITCH_LAGS_PER_LANE = 5;
constexpr int PITCH_BINS = PITCH_WIN / 2 + 1;
constexpr int PITCH_WAVES = 4;                  // frames per workgroup: one per wave
constexpr int PITCH_ARG_CLIPS = 64;             // descriptors up to this many travel in the launches' argument blocks (ragged.h)
constexpr int PITCH_FRAME_WORDS = 10;           // workspace floats per frame of a descriptor (see pitch_rows)
constexpr float PITCH_AMIN = 1e-10f, PITCH_TOP_DB = 80.f, PITCH_REF_DB = 20.f;
constexpr int PITCH_TAB_TW = PITCH_WIN, PITCH_TAB_AW = 3 * PITCH_WIN, PITCH_TAB_WORDS = 3 * PITCH_WIN + PITCH_BINS;
static_assert(PITCH_BLOCK * PITCH_NBLOCKS == PITCH_TERMS, "the blocks cover the terms");
static_assert(PITCH_LAGS_PER_LANE * 64 == PITCH_MAX_LAG - 1, "the lanes cover lags 1..320");
static_assert((PITCH_NBLOCKS - 1) * PITCH_BLOCK + 1 + PITCH_LAGS_PER_LANE * 63 + PITCH_BLOCK + PITCH_LAGS_PER_LANE - 2 < PITCH_WIN,
              "the last lane's last window stays inside the frame");

// One clip (track call) or one pair (pair call) of a launch
struct PitchClip {
    const float* x;                             // the clip; pair: the reference signal
    const float* y;                             // pair: the estimate
    float* out;                                 // track: [2][F] f0 | periodicity; pair: [3]
    float* taps;                                // track: [2][F] ungated periodicity | loudness, or null
    long T;
    long part;                                  // the descriptor's first frame among the per-frame rows of the workspace
};

struct PitchPar {
    const float* tab;
    float* rows;                                // the workspace behind the descriptors
    long total_frames;                          // of the call: the clip maxima lie behind 10 total_frames floats
    float threshold, silence, unvoiced;
    int pair;                                   // 1: two signals per descriptor, tracks to the workspace
};

__device__ __forceinline__ long pitch_frames(long T) { return 1 + (T - PITCH_WIN) / PITCH_HOP; }

// The workspace rows of signal s of descriptor d, F floats each: 0 raw f0, 1 raw periodicity, 2 the frame's largest power, 3 the
// gated f0 (NaN: unvoiced), 4 the gated periodicity
__device__ __forceinline__ global_ptr<float> pitch_row(const PitchClip& d, const PitchPar& p, int s, int row, long F) {
    return (global_ptr<float>)p.rows + PITCH_FRAME_WORDS * d.part + (5 * s + row) * F;
}
__device__ __forceinline__ global_ptr<float> pitch_clipmax(const PitchPar& p, int b, int s) {
    return (global_ptr<float>)p.rows + PITCH_FRAME_WORDS * p.total_frames + 2 * b + s;
}

// grid (ceil(max F / PITCH_WAVES), B, signals), 256 threads: wave w of block (x, b, s) takes frame PITCH_WAVES x + w
__device__ __forceinline__ void pitch_yin_block(const PitchClip& d, const PitchPar& p, int s) {
    __shared__ float lds[PITCH_WAVES][PITCH_WIN];
    const long F = pitch_frames(d.T);
    const long first = (long)blockIdx.x * PITCH_WAVES;
    if (first >= F) return;                                     // (the whole block: no barrier is left waiting)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = first + wave;
    const bool valid = f < F;
    const long fr = valid ? f : F - 1;                          // a wave past the clip's end keeps the barriers company
    const global_ptr<const float> x = (global_ptr<const float>)(s ? d.y : d.x) + fr * PITCH_HOP;
    float* xs = lds[wave];
#pragma unroll
    for (int m = 0; m < PITCH_WIN / 64; ++m) xs[lane + 64 * m] = x[lane + 64 * m];     // (fr <= F - 1: the last read is x[T - 1] at most)
    __syncthreads();

    // d(lag) = sum over j < 703 of (x[j] - x[j + lag])^2 for the lane's lags t0 .. t0 + 4: block after block of 19 terms, each block
    // added term by term from 0, the block sums added in order
    const int t0 = 1 + PITCH_LAGS_PER_LANE * lane;
    float dsum[PITCH_LAGS_PER_LANE];
#pragma unroll
    for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) dsum[k] = 0.f;
    for (int c = 0; c < PITCH_NBLOCKS; ++c) {
        const float* a = xs + PITCH_BLOCK * c;                  // one address for the wave: broadcast reads
        const float* w = a + t0;                                // stride 5 words over the lanes: every bank once per half
        float win[PITCH_BLOCK + PITCH_LAGS_PER_LANE - 1], part[PITCH_LAGS_PER_LANE];
#pragma unroll
        for (int i = 0; i < PITCH_BLOCK + PITCH_LAGS_PER_LANE - 1; ++i) win[i] = w[i];
#pragma unroll
        for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) part[k] = 0.f;
#pragma unroll
        for (int i = 0; i < PITCH_BLOCK; ++i) {
            const float xj = a[i];
#pragma unroll
            for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) {
                const float e = xj - win[i + k];
                part[k] = fmaf(e, e, part[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) dsum[k] += part[k];
    }
    // lag 321: lane l adds terms l, l + 64, ... in ascending order, the xor butterfly adds the lanes
    float dlast = 0.f;
    for (int j = lane; j < PITCH_TERMS; j += 64) {
        const float e = xs[j] - xs[j + PITCH_MAX_LAG];
        dlast = fmaf(e, e, dlast);
    }
    dlast = wave_sum(dlast);

    // the running sum over the lags: five in the lane, then a fixed scan over the lanes (lane l adds the sum of lanes l - 1, l - 2,
    // l - 4, ... as they stand: an order that depends on nothing but l)
    float run[PITCH_LAGS_PER_LANE];
    run[0] = dsum[0];
#pragma unroll
    for (int k = 1; k < PITCH_LAGS_PER_LANE; ++k) run[k] = run[k - 1] + dsum[k];
    float inc = run[PITCH_LAGS_PER_LANE - 1];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    float before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0.f;
    const float run_last = __shfl(inc, 63, 64) + dlast;

    // d'(lag) = d(lag) lag / running sum; 1 where that sum is 0 (digital silence, DC)
    float dp[PITCH_LAGS_PER_LANE];
#pragma unroll
    for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) {
        const float sum = before + run[k];
        dp[k] = sum > 0.f ? dsum[k] * (float)(t0 + k) / sum : 1.f;
    }
    const float dp_last = run_last > 0.f ? dlast * (float)PITCH_MAX_LAG / run_last : 1.f;
    __syncthreads();                            // (every wave has read its samples: d' takes their place, at word lag)
#pragma unroll
    for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) xs[t0 + k] = dp[k];
    if (lane == 0) {
        xs[0] = 1.f;
        xs[PITCH_MAX_LAG] = dp_last;
    }
    __syncthreads();
    const float prev = xs[t0 - 1], next = xs[t0 + PITCH_LAGS_PER_LANE];

    // the first lag in range under the threshold that is a local minimum (<= on its left, < on its right); without one, the
    // smallest lag that attains the minimum over the range
    int cand = 0x7fffffff, best = 0x7fffffff;
    float best_v = INFINITY;
#pragma unroll
    for (int k = 0; k < PITCH_LAGS_PER_LANE; ++k) {
        const int lag = t0 + k;
        const float cur = dp[k], le = k ? dp[k - 1] : prev, ri = k + 1 < PITCH_LAGS_PER_LANE ? dp[k + 1] : next;
        if (lag >= PITCH_LAG_LO && lag <= PITCH_LAG_HI) {
            if (cur < p.threshold && cur <= le && cur < ri && lag < cand) cand = lag;
            if (cur < best_v) { best_v = cur; best = lag; }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cand = min(cand, __shfl_xor(cand, off, 64));
        const float ov = __shfl_xor(best_v, off, 64);
        const int ot = __shfl_xor(best, off, 64);
        if (ov < best_v || (ov == best_v && ot < best)) { best_v = ov; best = ot; }
    }
    int lag = cand != 0x7fffffff ? cand : best;
    lag = lag < PITCH_LAG_LO || lag > PITCH_LAG_HI ? PITCH_LAG_LO : lag;        // (a frame of NaN compares false everywhere)
    // the parabola through the three points around the lag
    const float a = xs[lag - 1], b = xs[lag], c = xs[lag + 1];
    const float den = a - 2.f * b + c;
    float off = 0.f;
    if (den > 0.f) off = fminf(fmaxf(0.5f * (a - c) / den, -0.5f), 0.5f);
    const float f0 = (float)PITCH_RATE / ((float)lag + off);
    const float per = fminf(fmaxf(1.f - (b - 0.25f * (a - c) * off), 0.f), 1.f);
    if (valid && lane == 0) {
        pitch_row(d, p, s, 0, F)[f] = f0;
        pitch_row(d, p, s, 1, F)[f] = per;
    }
}

// 512 complex points as two float planes: point i sits at word swz(i) (stftd.hip's layout for 512 points, mel.hip's before it:
// every store of the passes and every stride-1 load meets each of the 32 banks once per half; python3 tools/lds_banks.py stftd)
__device__ __forceinline__ int pitch_swz(int i) { return i ^ ((i >> 3) & 7) ^ (((i >> 6) & 3) << 3); }

// One radix-8 Stockham pass at sub-transform length LS over the 512 points of a wave (stftd.hip's pass at M = 512): the lane holds
// points lane + 64 m in v[m]; its butterfly takes points lane + 64 r, twiddle exp(-2 pi i r k / (8 LS)) with k = lane % LS, and
// output q goes to point (lane / LS) 8 LS + k + LS q
template <int LS> __device__ __forceinline__ void pitch_pass(f32x2 (&v)[8], float* zr, float* zi, global_ptr<const f32x2> tw, int lane) {
    constexpr int M = PITCH_WIN / 2;
    if constexpr (LS > 1) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int o = pitch_swz(lane + 64 * m);
            v[m] = f32x2{zr[o], zi[o]};
        }
    }
    const int k = lane & (LS - 1);
    f32x2 u[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) u[r] = v[r];
    if constexpr (LS > 1) {
#pragma unroll
        for (int r = 1; r < 8; ++r) u[r] = cmul(u[r], tw[r * k * (2 * M / (LS * 8))]);
    }
    bfly8(u);
    const int j0 = (lane / LS) * (LS * 8) + k;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = pitch_swz(j0 + LS * q);
        zr[o] = u[rev3(q)].x;
        zi[o] = u[rev3(q)].y;
    }
    __syncthreads();
}

// grid as pitch_yin_kernel's.  LOUD false: the frame's largest power max(|X[k]|^2, 1e-10) to row 2.  LOUD true: the frame's level, the
// mean over the 513 bins of max(10 log10 max(|X[k]|^2, 1e-10), clip maximum - 80) + A[k] - 20 (the lane's bins k = lane + 64 r in
// ascending order, then the xor butterfly), and with it the gated periodicity and pitch
template <bool LOUD> __device__ __forceinline__ void pitch_gate_block(const PitchClip& d, const PitchPar& p, int b, int s) {
    constexpr int M = PITCH_WIN / 2;
    __shared__ float lds[PITCH_WAVES][2 * M];
    const long F = pitch_frames(d.T);
    const long first = (long)blockIdx.x * PITCH_WAVES;
    if (first >= F) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = first + wave;
    const bool valid = f < F;
    const long fr = valid ? f : F - 1;
    const global_ptr<const float> x = (global_ptr<const float>)(s ? d.y : d.x) + fr * PITCH_HOP;
    const global_ptr<const float> win = (global_ptr<const float>)p.tab;
    const global_ptr<const f32x2> tw = (global_ptr<const f32x2>)(p.tab + PITCH_TAB_TW);
    const global_ptr<const float> aw = (global_ptr<const float>)(p.tab + PITCH_TAB_AW);
    float* zr = lds[wave];
    float* zi = zr + M;
    f32x2 v[8];
    // z[j] = w[2j] x[2j] + i w[2j + 1] x[2j + 1], lane takes j = lane + 64 m (frames are not centred: nothing is reflected)
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int j = lane + 64 * m;
        const f32x2 w = *(global_ptr<const f32x2>)(win + 2 * j);
        v[m] = f32x2{x[2 * j] * w.x, x[2 * j + 1] * w.y};
    }
    pitch_pass<1>(v, zr, zi, tw, lane);
    pitch_pass<8>(v, zr, zi, tw, lane);
    pitch_pass<64>(v, zr, zi, tw, lane);
    float floor_db = 0.f;
    if constexpr (LOUD) floor_db = 10.f * log10f(*pitch_clipmax(p, b, s)) - PITCH_TOP_DB;
    float acc = 0.f;                            // the largest power, or the sum of the levels
#pragma unroll
    for (int r = 0; r <= 8; ++r) {
        const int k = lane + 64 * r;
        if (k <= M) {
            const int o = pitch_swz(k & (M - 1)), om = pitch_swz((M - k) & (M - 1));
            const float pw = fmaxf(cpower(real_split_bin(f32x2{zr[o], zi[o]}, f32x2{zr[om], zi[om]}, tw[k])), PITCH_AMIN);
            if constexpr (LOUD) acc += (fmaxf(10.f * log10f(pw), floor_db) + aw[k]) - PITCH_REF_DB;
            else acc = fmaxf(acc, pw);
        }
    }
    if constexpr (!LOUD) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = fmaxf(acc, __shfl_xor(acc, off, 64));
        if (valid && lane == 0) pitch_row(d, p, s, 2, F)[f] = acc;
    } else {
        const float loud = wave_sum(acc) / (float)PITCH_BINS;
        if (valid && lane == 0) {
            const float raw = pitch_row(d, p, s, 1, F)[f];
            const float per = loud < p.silence ? 0.f : raw;
            const float f0 = per < p.unvoiced ? NAN : pitch_row(d, p, s, 0, F)[f];
            if (p.pair) {
                pitch_row(d, p, s, 3, F)[f] = f0;
                pitch_row(d, p, s, 4, F)[f] = per;
            } else {
                const global_ptr<float> out = (global_ptr<float>)d.out;
                out[f] = f0;
                out[F + f] = per;
                if (d.taps) {
                    const global_ptr<float> taps = (global_ptr<float>)d.taps;
                    taps[f] = raw;
                    taps[F + f] = loud;
                }
            }
        }
    }
}

// grid (B, signals), 64 threads: the largest power over the signal's frames
__device__ __forceinline__ void pitch_clipmax_block(const PitchClip& d, const PitchPar& p, int b, int s) {
    const int lane = threadIdx.x;
    const long F = pitch_frames(d.T);
    const global_ptr<const float> mx = pitch_row(d, p, s, 2, F);
    float m = PITCH_AMIN;
    for (long i = lane; i < F; i += 64) m = fmaxf(m, mx[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) *pitch_clipmax(p, b, s) = m;
}

// grid B, 64 threads: out[0] = sqrt(mean (p^ - p)^2), out[1] = sqrt(mean cents^2) over the frames voiced in both (NaN without one),
// out[2] = F1 of the voiced flags (NaN where precision or recall is 0 / 0, or both are 0).  Lane l adds frames l, l + 64, ... in
// ascending order, the xor butterfly adds the lanes: the order depends on the frame count alone.  The counts are exact in fp32.
__device__ __forceinline__ void pitch_pair_block(const PitchClip& d, const PitchPar& p) {
    const int lane = threadIdx.x;
    const long F = pitch_frames(d.T);
    const global_ptr<const float> f0 = pitch_row(d, p, 0, 3, F), pe = pitch_row(d, p, 0, 4, F);
    const global_ptr<const float> g0 = pitch_row(d, p, 1, 3, F), qe = pitch_row(d, p, 1, 4, F);
    float sp = 0.f, sc = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    for (long i = lane; i < F; i += 64) {
        const float e = qe[i] - pe[i];
        sp = fmaf(e, e, sp);
        const float a = f0[i], b = g0[i];
        const bool va = a == a, vb = b == b;
        if (va && vb) {
            const float cents = 1200.f * (log2f(a) - log2f(b));
            sc = fmaf(cents, cents, sc);
            tp += 1.f;
        } else if (vb) fp += 1.f;
        else if (va) fn += 1.f;
    }
    sp = wave_sum(sp);
    sc = wave_sum(sc);
    tp = wave_sum(tp);
    fp = wave_sum(fp);
    fn = wave_sum(fn);
    if (lane == 0) {
        const global_ptr<float> out = (global_ptr<float>)d.out;
        const float precision = tp / (tp + fp), recall = tp / (tp + fn);
        out[0] = sqrtf(sp / (float)F);
        out[1] = sqrtf(sc / tp);                // 0 / 0: NaN
        out[2] = 2.f * precision * recall / (precision + recall);
    }
}

template <class D> __global__ __launch_bounds__(256) void pitch_yin_kernel(const D d, const PitchPar p) {
    pitch_yin_block(d.clip[blockIdx.y], p, blockIdx.z);
}
template <bool LOUD, class D> __global__ __launch_bounds__(256) void pitch_gate_kernel(const D d, const PitchPar p) {
    pitch_gate_block<LOUD>(d.clip[blockIdx.y], p, blockIdx.y, blockIdx.z);
}
template <class D> __global__ __launch_bounds__(64) void pitch_clipmax_kernel(const D d, const PitchPar p) {
    pitch_clipmax_block(d.clip[blockIdx.x], p, blockIdx.x, blockIdx.y);
}
template <class D> __global__ __launch_bounds__(64) void pitch_pair_kernel(const D d, const PitchPar p) {
    pitch_pair_block(d.clip[blockIdx.x], p);
}

static size_t pitch_desc_bytes(int B) { return ((size_t)B * sizeof(PitchClip) + 15) / 16 * 16; }

static int64_t pitch_frames_host(int64_t T) { return T < PITCH_WIN ? 0 : 1 + (T - PITCH_WIN) / PITCH_HOP; }

// The periodic Hann window of 1024 samples and the A-weighting in dB of the 513 bin frequencies k 16000 / 1024, clipped below at
// -80 (librosa.A_weighting: bin 0 gets -80): float64, rounded once
static void pitch_tables(float* window, float* a_weight) {
    const double pi = 3.14159265358979323846;
    if (window)
        for (int n = 0; n < PITCH_WIN; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * n / PITCH_WIN));
    if (a_weight) {
        const double c0 = 12194.217 * 12194.217, c1 = 20.598997 * 20.598997, c2 = 107.65265 * 107.65265, c3 = 737.86223 * 737.86223;
        a_weight[0] = -80.f;
        for (int k = 1; k < PITCH_BINS; ++k) {
            const double f = (double)k * PITCH_RATE / PITCH_WIN, q = f * f;
            const double w = 2.0 + 20.0 * (std::log10(c0) + 2.0 * std::log10(q) - std::log10(q + c0) - std::log10(q + c1) -
                                           0.5 * std::log10(q + c2) - 0.5 * std::log10(q + c3));
            a_weight[k] = (float)std::max(w, -80.0);
        }
    }
}

// One descriptor of a call as the checks want it: the signals (second null in a track call), the length, out and taps
struct PitchArg { const float* x; const float* y; int64_t length; float* out; float* taps; };

static int pitch_run(const wt_pitch* h, bool pair, const void* clips, int32_t B, float threshold, float silence, float unvoiced,
                     void* workspace, void* stream, const char* name) {
    const std::string fn = name;
    if (!ragged_call_ok(fn, h, clips, workspace, B, 65535)) return WT_ERR_INVALID;
    if (!h->tab) { set_error(fn + ": not a handle of wt_pitch_create"); return WT_ERR_INVALID; }
    if (!(threshold == threshold) || !(silence == silence) || !(unvoiced == unvoiced)) {
        set_error(fn + ": a threshold is NaN"); return WT_ERR_INVALID;
    }
    std::vector<PitchClip> dev((size_t)B);
    int64_t max_frames = 0, total = 0;
    for (int b = 0; b < B; ++b) {
        PitchArg c;
        if (pair) {
            const wt_pitch_pair& q = static_cast<const wt_pitch_pair*>(clips)[b];
            c = PitchArg{q.reference, q.estimate, q.length, q.out, nullptr};
        } else {
            const wt_pitch_clip& q = static_cast<const wt_pitch_clip*>(clips)[b];
            c = PitchArg{q.signal, nullptr, q.length, q.out, q.taps};
        }
        const std::string who = fn + (pair ? ": pair " : ": clip ") + std::to_string(b) + ": ";
        if (!c.x) { set_error(who + (pair ? "null reference" : "null signal")); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null out"); return WT_ERR_INVALID; }
        if (pair && !c.y) { set_error(who + "null estimate"); return WT_ERR_INVALID; }
        if (c.length < PITCH_WIN) { set_error(who + "length < 1024 (one frame needs 1024 samples at 16 kHz)"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.x) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float) ||
            reinterpret_cast<uintptr_t>(c.y) % sizeof(float) || reinterpret_cast<uintptr_t>(c.taps) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        const int64_t F = pitch_frames_host(c.length);
        dev[b] = PitchClip{c.x, c.y, c.out, c.taps, (long)c.length, (long)total};
        max_frames = std::max(max_frames, F);
        total += F;
    }
    if ((max_frames + PITCH_WAVES - 1) / PITCH_WAVES > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    if (!on_current_device(fn, h->device)) return WT_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PitchPar par{};
    par.tab = h->tab;
    par.rows = reinterpret_cast<float*>(static_cast<char*>(workspace) + pitch_desc_bytes(B));
    par.total_frames = (long)total;
    par.threshold = threshold; par.silence = silence; par.unvoiced = unvoiced;
    par.pair = pair ? 1 : 0;
    const unsigned signals = pair ? 2 : 1;
    if (int rc = launch_ragged<PITCH_ARG_CLIPS>(name, dev.data(), B, 128, workspace, s, [&](auto d) {
        using D = decltype(d);
        const dim3 grid((unsigned)((max_frames + PITCH_WAVES - 1) / PITCH_WAVES), (unsigned)B, signals);
        hipLaunchKernelGGL(pitch_yin_kernel<D>, grid, dim3(64 * PITCH_WAVES), 0, s, d, par);
        hipLaunchKernelGGL((pitch_gate_kernel<false, D>), grid, dim3(64 * PITCH_WAVES), 0, s, d, par);
        hipLaunchKernelGGL(pitch_clipmax_kernel<D>, dim3((unsigned)B, signals), dim3(64), 0, s, d, par);
        hipLaunchKernelGGL((pitch_gate_kernel<true, D>), grid, dim3(64 * PITCH_WAVES), 0, s, d, par);
        if (pair) hipLaunchKernelGGL(pitch_pair_kernel<D>, dim3((unsigned)B), dim3(64), 0, s, d, par);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // namespace wt

using namespace wt;

extern "C" {

int wt_pitch_create(int32_t device, wt_pitch** out) {
    if (!out) { set_error("wt_pitch_create: null out"); return WT_ERR_INVALID; }
    std::vector<float> tab(PITCH_TAB_WORDS, 0.f);
    pitch_tables(tab.data(), tab.data() + PITCH_TAB_AW);
    fill_twiddles(tab.data() + PITCH_TAB_TW, PITCH_WIN);
    float* dtab = nullptr;
    if (int rc = upload_table("wt_pitch_create", device, tab, &dtab)) return rc;
    wt_pitch* h = new wt_pitch();
    h->device = device; h->tab = dtab;
    *out = h;
    return WT_OK;
}

void wt_pitch_destroy(wt_pitch* h) {
    if (!h) return;
    (void)hipFree(h->tab);
    delete h;
}

int64_t wt_pitch_frames(int64_t T) { return pitch_frames_host(T); }

int wt_pitch_tables(float* window, float* a_weight) {
    pitch_tables(window, a_weight);
    return WT_OK;
}

size_t wt_pitch_workspace_bytes(int32_t B, int64_t total_frames) {
    if (B < 1 || total_frames < 0) return 0;
    return pitch_desc_bytes(B) + ((size_t)total_frames * PITCH_FRAME_WORDS + (size_t)2 * B) * sizeof(float);
}

int wt_pitch_track(const wt_pitch* h, const wt_pitch_clip* clips, int32_t B, float threshold, float silence_threshold,
                   float unvoiced_threshold, void* workspace, void* stream) {
    return pitch_run(h, false, clips, B, threshold, silence_threshold, unvoiced_threshold, workspace, stream, "wt_pitch_track");
}

int wt_pitch_pairs(const wt_pitch* h, const wt_pitch_pair* pairs, int32_t B, float threshold, float silence_threshold,
                   float unvoiced_threshold, void* workspace, void* stream) {
    return pitch_run(h, true, pairs, B, threshold, silence_threshold, unvoiced_threshold, workspace, stream, "wt_pitch_pairs");
}

}  // extern "C"
