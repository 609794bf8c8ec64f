// The codec's evaluation metric on the GPU: log-mel spectrograms and their L1 distance (the reference's val/mel_loss:
// MelSpecReconstructionLoss, decoder/loss.py:12-39; safe_log, decoder/modules.py:194-205; logged in decoder/experiment.py:257-304).
// The transform restates what torchaudio.transforms.MelSpectrogram(sample_rate, n_fft=1024, hop_length, n_mels, center=True,
// power=1) computes with its defaults (reflect padding by n_fft / 2, periodic Hann window, |rfft|, HTK mel scale, triangular
// filters without area normalisation); torchaudio is not available to this project's tests, so like the resampler (audio.hip) the
// parity with it is unpinned: tests/mel_ref.py holds the definition in float64 and the kernels are checked against that.
//
// One wave computes one frame: the 1024 windowed samples are gathered from the clip (reflect index at both ends, nothing outside
// [0, T) is read) as the 512 complex points z[j] = x[2j] + i x[2j + 1], transformed by a radix-8 Stockham FFT (three passes, eight
// points per lane, fp32, data exchanged through the wave's own LDS region), split into the 513 bins of the real transform, and the
// magnitudes go through the sparse triangular filters.  A frame's result depends on its own 1024 samples alone: no second signal
// or frame shares the complex transform (in fp32 the louder one would leak into the quieter one).
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

// (tests/test_mel_host.py mirrors this layout in ctypes to hand the calls a handle without a GPU: keep the two in step)
struct wt_mel {
    int device = 0;
    int sample_rate = 0, n_fft = 0, hop = 0, n_mels = 0;
    float* tab = nullptr;                       // one device block: window | twiddles | filter weights | filter table
};

// FFT products must not depend on the kernel a device function is inlined into: no contraction by the compiler, fmaf where wanted
// (over fft.h's functions too: the pragma stands before the include)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int MEL_NFFT = 1024, MEL_BINS = MEL_NFFT / 2 + 1, MEL_MAX_MELS = 128;
constexpr int MEL_WAVES = 4;                    // frames per workgroup: one per wave
// layout of wt_mel::tab, in 4-byte words
constexpr int MEL_TAB_WIN = 0;                              // [1024] periodic Hann
constexpr int MEL_TAB_TW = MEL_TAB_WIN + MEL_NFFT;          // [1024][2] (cos, -sin)(2 pi n / 1024)
constexpr int MEL_TAB_FBW = MEL_TAB_TW + 2 * MEL_NFFT;      // [2 * 513 + 6] non-zero filter weights, filter after filter
constexpr int MEL_TAB_FB = MEL_TAB_FBW + 2 * MEL_BINS + 6;  // int [3][128]: first bin, count, offset into the weights
constexpr int MEL_TAB_WORDS = MEL_TAB_FB + 3 * MEL_MAX_MELS;

// One clip of a launch (device form of wt_mel_clip)
struct MelClip {
    const float* a;
    const float* b;                             // distance mode only
    float* out;                                 // spectrogram: [n_mels][F]; distance: one float
    long T, F;
    long part;                                  // distance mode: index of the clip's first per-frame partial in the workspace
};

struct MelTab {
    const float* tab;
    int hop, n_mels;
};

enum : int { MEL_MODE_LINEAR = 0, MEL_MODE_LOG = 1, MEL_MODE_DISTANCE = 2 };

// 512 complex points as two float planes: point i sits at word swz(i).  Every access of the three passes (stride-8 and stride-64
// writes, stride-1 reads) then meets each of the 32 banks once per 32-lane half (tools/lds_banks.py, section mel)
__device__ __forceinline__ int mel_swz(int i) { return i ^ ((i >> 3) & 7) ^ (((i >> 6) & 3) << 3); }

// Frame f of clip x (T samples): mel value (log: its clipped log) of filter `lane` in m0 and of filter lane + 64 in m1 (0 where there
// is no such filter).  zr, zi [512] and S [MEL_BINS] are the calling wave's own LDS; every wave of the block makes the call (the
// barriers are the block's).  The arithmetic is the same whatever the mode, the clip's place in the launch or the wave.
__device__ __forceinline__ void mel_frame(global_ptr<const float> x, long T, long f, const MelTab& tb, float* zr, float* zi, float* S,
                                          int lane, bool take_log, float& m0, float& m1) {
    const global_ptr<const float> win = (global_ptr<const float>)(tb.tab + MEL_TAB_WIN);
    const global_ptr<const f32x2> tw = (global_ptr<const f32x2>)(tb.tab + MEL_TAB_TW);
    const global_ptr<const float> fbw = (global_ptr<const float>)(tb.tab + MEL_TAB_FBW);
    const global_ptr<const int> fb = (global_ptr<const int>)(tb.tab + MEL_TAB_FB);
    const long base = f * tb.hop - MEL_NFFT / 2;
    f32x2 v[8];
    // gather: z[j] = w[2j] x[2j] + i w[2j + 1] x[2j + 1], lane takes j = lane + 64 r.  T > n_fft / 2 makes one reflection enough:
    // base >= -512 gives -n <= 512 <= T - 1, and (F - 1) hop <= T gives n <= T + 511, 2 (T - 1) - n >= T - 513 >= 0
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int j = lane + 64 * r;
        long n0 = base + 2 * j, n1 = n0 + 1;
        n0 = n0 < 0 ? -n0 : (n0 >= T ? 2 * (T - 1) - n0 : n0);
        n1 = n1 < 0 ? -n1 : (n1 >= T ? 2 * (T - 1) - n1 : n1);
        const f32x2 w = *(global_ptr<const f32x2>)(win + 2 * j);
        v[r] = f32x2{x[n0] * w.x, x[n1] * w.y};
    }
    // pass 1 (sub-transform length 1): no twiddles; output q of lane's butterfly goes to point 8 lane + q
    bfly8(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = mel_swz(8 * lane + q);
        zr[o] = v[rev3(q)].x;
        zi[o] = v[rev3(q)].y;
    }
    __syncthreads();
    // pass 2 (length 8): k = lane % 8, twiddle exp(-2 pi i r k / 64); output q goes to 64 (lane / 8) + k + 8 q
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int o = mel_swz(lane + 64 * r);
        v[r] = f32x2{zr[o], zi[o]};
    }
    {
        const int k = lane & 7;
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[16 * r * k]);
        bfly8(v);
        const int j0 = (lane >> 3) * 64 + k;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int o = mel_swz(j0 + 8 * q);
            zr[o] = v[rev3(q)].x;
            zi[o] = v[rev3(q)].y;
        }
    }
    __syncthreads();
    // pass 3 (length 64): k = lane, twiddle exp(-2 pi i r k / 512); output q goes to lane + 64 q: Z in natural order
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int o = mel_swz(lane + 64 * r);
        v[r] = f32x2{zr[o], zi[o]};
    }
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[2 * r * lane]);
    bfly8(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int o = mel_swz(lane + 64 * q);
        zr[o] = v[rev3(q)].x;
        zi[o] = v[rev3(q)].y;
    }
    __syncthreads();
    // split pass: X[k] = (Z[k] + conj Z[512 - k]) / 2 - i / 2 exp(-2 pi i k / 1024) (Z[k] - conj Z[512 - k]), k = 0..512, Z[512] = Z[0]
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        if (k < MEL_BINS) {
            const int o = mel_swz(k & 511), om = mel_swz((512 - k) & 511);
            S[k] = sqrtf(cpower(real_split_bin(f32x2{zr[o], zi[o]}, f32x2{zr[om], zi[om]}, tw[k])));
        }
    }
    __syncthreads();
    // filters: ascending fmaf chain over the filter's own bins
    float m[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int mi = lane + 64 * h;
        float acc = 0.f;
        if (mi < tb.n_mels) {
            const int first = fb[mi], cnt = fb[MEL_MAX_MELS + mi], off = fb[2 * MEL_MAX_MELS + mi];
            for (int i = 0; i < cnt; ++i) acc = fmaf(fbw[off + i], S[first + i], acc);
            if (take_log) acc = logf(fmaxf(acc, 1e-7f));       // safe_log (decoder/modules.py:194-205)
        }
        m[h] = acc;
    }
    m0 = m[0];
    m1 = m[1];
}

// grid (ceil(max F / MEL_WAVES), B), 256 threads: wave w of block (x, b) takes frame MEL_WAVES x + w of clip b.
//   MEL_MODE_LINEAR / _LOG: out[m][f] = M or L
//   MEL_MODE_DISTANCE: part[d.part + f] = sum over the filters of |La - Lb|: lane-local sum of its two filters, then the xor
//   butterfly over the wave: a fixed order
__device__ __forceinline__ void mel_block(const MelClip& d, const MelTab& tb, int mode, float* part) {
    __shared__ float lds[MEL_WAVES][2 * 512 + 520];
    const long f0 = (long)blockIdx.x * MEL_WAVES;
    if (f0 >= d.F) return;                                      // (the whole block: no barrier is left waiting)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = f0 + wave;
    const bool valid = f < d.F;
    const long fr = valid ? f : d.F - 1;                        // a wave past the clip's end keeps the barriers company
    float* zr = lds[wave];
    float* zi = zr + 512;
    float* S = zr + 1024;
    float a0, a1;
    mel_frame((global_ptr<const float>)d.a, d.T, fr, tb, zr, zi, S, lane, mode != MEL_MODE_LINEAR, a0, a1);
    if (mode != MEL_MODE_DISTANCE) {
        if (valid) {
            const global_ptr<float> out = (global_ptr<float>)d.out;
            if (lane < tb.n_mels) out[(long)lane * d.F + f] = a0;
            if (lane + 64 < tb.n_mels) out[(long)(lane + 64) * d.F + f] = a1;
        }
        return;
    }
    float b0, b1;
    mel_frame((global_ptr<const float>)d.b, d.T, fr, tb, zr, zi, S, lane, true, b0, b1);
    const float s = wave_sum((lane < tb.n_mels ? fabsf(a0 - b0) : 0.f) + (lane + 64 < tb.n_mels ? fabsf(a1 - b1) : 0.f));
    if (valid && lane == 0) part[d.part + f] = s;
}

// A clip's distance from its per-frame partials: lane l adds partials l, l + 64, ... in ascending order, the xor butterfly adds the
// lanes, one division by n_mels F.  The order depends on F alone.
__device__ __forceinline__ void mel_mean_block(const MelClip& d, int n_mels, const float* part) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (long i = lane; i < d.F; i += 64) s += part[d.part + i];
    s = wave_sum(s);
    if (lane == 0) *(global_ptr<float>)d.out = s / ((float)n_mels * (float)d.F);
}

// D: the descriptors in the kernel's argument block (up to MEL_ARG_CLIPS clips: no upload and no host wait, so the call can be
// captured into a graph) or in the workspace (ragged.h)
constexpr int MEL_ARG_CLIPS = 64;
template <class D> __global__ __launch_bounds__(256) void mel_frame_kernel(const D d, const MelTab tb, int mode, float* __restrict__ part) {
    mel_block(d.clip[blockIdx.y], tb, mode, part);
}
template <class D> __global__ __launch_bounds__(64) void mel_mean_kernel(const D d, int n_mels, const float* __restrict__ part) {
    mel_mean_block(d.clip[blockIdx.x], n_mels, part);
}

static size_t mel_desc_bytes(int B) { return ((size_t)B * sizeof(MelClip) + 15) / 16 * 16; }

static bool mel_params_ok(int sample_rate, int n_fft, int n_mels, const char* who) {
    if (n_fft != MEL_NFFT) { set_error(std::string(who) + ": n_fft must be 1024"); return false; }
    if (n_mels < 1 || n_mels > MEL_MAX_MELS) { set_error(std::string(who) + ": n_mels outside 1..128"); return false; }
    if (sample_rate < 2) { set_error(std::string(who) + ": sample_rate < 2"); return false; }
    return true;
}

// Window [1024] and the dense filterbank [513][n_mels], computed in float64 and rounded once:
//   all_freqs = linspace(0, sample_rate // 2, 513);  m_pts = linspace(0, 2595 log10(1 + (sample_rate / 2) / 700), n_mels + 2)
//   f_pts = 700 (10^(m_pts / 2595) - 1);  fb[k][m] = max(0, min((all_freqs[k] - f_pts[m]) / (f_pts[m + 1] - f_pts[m]),
//                                                                (f_pts[m + 2] - all_freqs[k]) / (f_pts[m + 2] - f_pts[m + 1])))
static void mel_tables(int sample_rate, int n_mels, std::vector<float>& window, std::vector<float>& fb) {
    const double pi = 3.14159265358979323846;
    window.resize(MEL_NFFT);
    for (int n = 0; n < MEL_NFFT; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * n / MEL_NFFT));
    const double fmax_bins = (double)(sample_rate / 2);
    const double m_max = 2595.0 * std::log10(1.0 + ((double)sample_rate / 2.0) / 700.0);
    std::vector<double> f_pts((size_t)n_mels + 2);
    const double step = m_max / (n_mels + 1);
    for (int i = 0; i < n_mels + 2; ++i) {
        const double mp = i == n_mels + 1 ? m_max : i * step;
        f_pts[i] = 700.0 * (std::pow(10.0, mp / 2595.0) - 1.0);
    }
    fb.assign((size_t)MEL_BINS * n_mels, 0.f);
    const double fstep = fmax_bins / (MEL_BINS - 1);
    for (int k = 0; k < MEL_BINS; ++k) {
        const double fr = k == MEL_BINS - 1 ? fmax_bins : k * fstep;
        for (int m = 0; m < n_mels; ++m) {
            const double up = (fr - f_pts[m]) / (f_pts[m + 1] - f_pts[m]);
            const double down = (f_pts[m + 2] - fr) / (f_pts[m + 2] - f_pts[m + 1]);
            const double v = std::fmax(0.0, std::fmin(up, down));
            fb[(size_t)k * n_mels + m] = (float)v;
        }
    }
}

static int mel_run(const wt_mel* m, const wt_mel_clip* clips, int32_t B, int mode, void* workspace, void* stream, const char* name) {
    const std::string fn = name;
    if (!ragged_call_ok(fn, m, clips, workspace, B, 65535)) return WT_ERR_INVALID;
    if (m->n_fft != MEL_NFFT || m->hop < 1 || m->hop > MEL_NFFT || m->n_mels < 1 || m->n_mels > MEL_MAX_MELS || !m->tab) {
        set_error(fn + ": not a handle of wt_mel_create"); return WT_ERR_INVALID;
    }
    std::vector<MelClip> dev((size_t)B);
    int64_t max_frames = 0, total = 0;
    for (int b = 0; b < B; ++b) {
        const wt_mel_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.a) { set_error(who + "null a"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null out"); return WT_ERR_INVALID; }
        if (mode == MEL_MODE_DISTANCE && !c.b) { set_error(who + "null b"); return WT_ERR_INVALID; }
        if (c.length <= MEL_NFFT / 2) { set_error(who + "length <= n_fft / 2 (reflect padding needs more)"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.a) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float) ||
            (mode == MEL_MODE_DISTANCE && reinterpret_cast<uintptr_t>(c.b) % sizeof(float))) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        const int64_t F = 1 + c.length / m->hop;
        dev[b] = MelClip{c.a, mode == MEL_MODE_DISTANCE ? c.b : nullptr, c.out, (long)c.length, (long)F, (long)total};
        max_frames = std::max(max_frames, F);
        total += F;
    }
    if ((max_frames + MEL_WAVES - 1) / MEL_WAVES > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    if (!on_current_device(fn, m->device)) return WT_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MelTab tb{m->tab, m->hop, m->n_mels};
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + mel_desc_bytes(B));
    const dim3 grid((unsigned)((max_frames + MEL_WAVES - 1) / MEL_WAVES), (unsigned)B);
    if (int rc = launch_ragged<MEL_ARG_CLIPS>(name, dev.data(), B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL(mel_frame_kernel<decltype(d)>, grid, dim3(64 * MEL_WAVES), 0, s, d, tb, mode, part);
        if (mode == MEL_MODE_DISTANCE) hipLaunchKernelGGL(mel_mean_kernel<decltype(d)>, dim3((unsigned)B), dim3(64), 0, s, d, m->n_mels, part);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // namespace wt

using namespace wt;

extern "C" {

int wt_mel_create(int32_t sample_rate, int32_t n_fft, int32_t hop_length, int32_t n_mels, int32_t device, wt_mel** out) {
    if (!out) { set_error("wt_mel_create: null out"); return WT_ERR_INVALID; }
    if (!mel_params_ok(sample_rate, n_fft, n_mels, "wt_mel_create")) return WT_ERR_INVALID;
    if (hop_length < 1 || hop_length > MEL_NFFT) { set_error("wt_mel_create: hop_length outside 1..1024"); return WT_ERR_INVALID; }
    std::vector<float> window, fb;
    mel_tables(sample_rate, n_mels, window, fb);
    std::vector<float> tab((size_t)MEL_TAB_WORDS, 0.f);
    memcpy(tab.data() + MEL_TAB_WIN, window.data(), MEL_NFFT * sizeof(float));
    fill_twiddles(tab.data() + MEL_TAB_TW, MEL_NFFT);
    // sparse form: a triangular filter's non-zero bins are one run; a bin lies in at most two filters, so the runs hold at most
    // 2 * 513 weights
    std::vector<int32_t> fbt((size_t)3 * MEL_MAX_MELS, 0);
    int used = 0;
    for (int m = 0; m < n_mels; ++m) {
        int first = -1, last = -1;
        for (int k = 0; k < MEL_BINS; ++k)
            if (fb[(size_t)k * n_mels + m] != 0.f) { if (first < 0) first = k; last = k; }
        const int cnt = first < 0 ? 0 : last - first + 1;
        if (used + cnt > 2 * MEL_BINS + 6) { set_error("wt_mel_create: filter table overflow"); return WT_ERR_INVALID; }
        fbt[m] = first < 0 ? 0 : first;
        fbt[MEL_MAX_MELS + m] = cnt;
        fbt[2 * MEL_MAX_MELS + m] = used;
        for (int i = 0; i < cnt; ++i) tab[MEL_TAB_FBW + used + i] = fb[(size_t)(first + i) * n_mels + m];
        used += cnt;
    }
    memcpy(tab.data() + MEL_TAB_FB, fbt.data(), fbt.size() * sizeof(int32_t));
    float* dtab = nullptr;
    if (int rc = upload_table("wt_mel_create", device, tab, &dtab)) return rc;
    wt_mel* h = new wt_mel();
    h->device = device; h->sample_rate = sample_rate; h->n_fft = n_fft; h->hop = hop_length; h->n_mels = n_mels; h->tab = dtab;
    *out = h;
    return WT_OK;
}

void wt_mel_destroy(wt_mel* m) {
    if (!m) return;
    (void)hipFree(m->tab);
    delete m;
}

int64_t wt_mel_frames(const wt_mel* m, int64_t T) {
    if (!m || m->hop < 1 || T <= m->n_fft / 2) return -1;
    return 1 + T / m->hop;
}

int wt_mel_tables(int32_t sample_rate, int32_t n_fft, int32_t n_mels, float* window, float* fb) {
    if (!mel_params_ok(sample_rate, n_fft, n_mels, "wt_mel_tables")) return WT_ERR_INVALID;
    std::vector<float> w, f;
    mel_tables(sample_rate, n_mels, w, f);
    if (window) memcpy(window, w.data(), w.size() * sizeof(float));
    if (fb) memcpy(fb, f.data(), f.size() * sizeof(float));
    return WT_OK;
}

size_t wt_mel_workspace_bytes(int32_t B, int64_t total_frames) {
    if (B < 1 || total_frames < 0) return 0;
    return mel_desc_bytes(B) + (size_t)total_frames * sizeof(float);
}

int wt_mel_spectrogram(const wt_mel* m, const wt_mel_clip* clips, int32_t B, int32_t log, void* workspace, void* stream) {
    return mel_run(m, clips, B, log ? MEL_MODE_LOG : MEL_MODE_LINEAR, workspace, stream, "wt_mel_spectrogram");
}

int wt_mel_distance(const wt_mel* m, const wt_mel_clip* clips, int32_t B, void* workspace, void* stream) {
    return mel_run(m, clips, B, MEL_MODE_DISTANCE, workspace, stream, "wt_mel_distance");
}

}  // extern "C"
