// The multi-resolution STFT distance on the GPU (Yamamoto, Song & Kim 2020, Parallel WaveGAN: spectral convergence plus log-magnitude
// L1 per resolution, the mean over the resolutions), the spectral measure codec papers report beside the mel distance.
// include/wavtokenizer_amd.h states the definition; auraloss is not available to this project's tests, so like the mel transform
// (mel.hip) the parity with it is unpinned: tests/stftd_ref.py holds the definition in float64 and the kernels are checked against that.
//
// One launch per resolution, ragged over the call's clips, then one small launch that adds a clip's per-frame partials.  One wave
// computes one frame: the n_fft windowed samples are gathered from the clip (reflect index at both ends, nothing outside [0, T) is
// read) as the n_fft / 2 complex points z[j] = x[2j] + i x[2j + 1], transformed by a Stockham FFT in fp32 through the wave's own LDS
// region (256 points: four radix-4 passes; 512: three radix-8 passes; 1024: a radix-4 and two radix-16 passes, 16 points per lane),
// and split into the n_fft / 2 + 1 bins of the real transform.  The magnitudes stay in registers: lane l holds bins l, l + 64, ...
// The two signals of a pair are transformed one after the other and never share a complex transform (mel.hip gives the reason: in
// fp32 the louder one would leak into the quieter one).  fp32 throughout, no float atomics, every summation order depends on the
// clip's length alone: a pair has the same bits alone, in any batch and at any position.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cmath>
#include <cstring>
#include <vector>

constexpr int STFTD_MAX_RES = 8;

// (tests/test_stftd_host.py mirrors this layout in ctypes to hand the calls a handle without a GPU: keep the two in step)
struct wt_stftd {
    int device = 0;
    int n_res = 0;
    int n_fft[STFTD_MAX_RES] = {}, hop[STFTD_MAX_RES] = {}, win[STFTD_MAX_RES] = {};
    int off[STFTD_MAX_RES] = {};                // resolution r's block in tab, in 4-byte words: window [n_fft] | twiddles [n_fft][2]
    float* tab = nullptr;                       // one device block
};

// FFT products must not depend on the kernel a device function is inlined into: no contraction by the compiler, fmaf where wanted
// (over fft.h's functions too: the pragma stands before the include)
#pragma clang fp contract(off)
#include "fft.h"
#include "ragged.h"

namespace wt {

constexpr int STFTD_WAVES = 4;                  // frames per workgroup: one per wave
constexpr float STFTD_FLOOR = 1e-7f;            // the clamp under the power
constexpr int STFTD_ARG_CLIPS = 64;             // descriptors up to this many travel in the launches' argument blocks (ragged.h)

// One pair of a launch (device form of wt_stftd_clip)
struct StftdClip {
    const float* x;                             // the estimate (magnitude mode: the signal)
    const float* y;                             // the target (distance mode only)
    float* out;                                 // distance: [1 + 2 n_res]; magnitude: [n_fft / 2 + 1][F]
    long T;
    long part;                                  // distance mode: the clip's first frame among the per-frame partials in the workspace
};

struct StftdPar {
    const float* tab;                           // the launch's resolution: window | twiddles
    int r, n_res;
    int hop[STFTD_MAX_RES], n_fft[STFTD_MAX_RES];
};

enum : int { STFTD_MODE_MAGNITUDE = 0, STFTD_MODE_DISTANCE = 1 };

// M complex points as two float planes: point i sits at word swz(i), so that every store of the passes and every stride-1 load meets
// each of the 32 banks once per 32-lane half; the split pass's mirrored load alone keeps a two-way conflict (python3
// tools/lds_banks.py stftd).  256 and 512 points: the layouts of stoi.hip and
// mel.hip.  1024 points: pass 1 stores points 4 lane + q (+ 256 b), bits 5-6 of the point vary with the lane and go to bits 0-1;
// pass 2 stores 64 (lane / 4) + lane % 4 + 4 q, bits 6-8 vary and go to bits 2-4.
template <int M> __device__ __forceinline__ int stftd_swz(int i) {
    if constexpr (M == 256) return i ^ ((i >> 5) & 3) ^ (((i >> 5) & 3) << 2) ^ (((i >> 6) & 1) << 4);
    else if constexpr (M == 512) return i ^ ((i >> 3) & 7) ^ (((i >> 6) & 3) << 3);
    else return i ^ ((i >> 5) & 3) ^ (((i >> 6) & 7) << 2);
}

template <int R> __device__ __forceinline__ void stftd_bfly(f32x2 (&u)[R]) {
    if constexpr (R == 4) bfly4(u[0], u[1], u[2], u[3]);
    else if constexpr (R == 8) bfly8(u);
    else bfly16(u);
}
template <int R> __device__ __forceinline__ int stftd_rev(int q) {
    if constexpr (R == 4) return rev2(q);
    else if constexpr (R == 8) return rev3(q);
    else return rev4(q);
}

// One Stockham pass of radix R at sub-transform length LS over the M points of a wave.  The lane holds points lane + 64 m in v[m]
// (the first pass: from the gather; later ones: loaded here); its butterfly b, j = lane + 64 b of M / R, takes points j + (M / R) r,
// twiddle exp(-2 pi i r k / (LS R)) with k = j % LS, and output q goes to point (j / LS) LS R + k + LS q.
template <int M, int R, int LS> __device__ __forceinline__ void stftd_pass(f32x2 (&v)[M / 64], float* zr, float* zi,
                                                                          global_ptr<const f32x2> tw, int lane) {
    constexpr int P = M / 64, NB = M / R / 64;
    if constexpr (LS > 1) {
#pragma unroll
        for (int m = 0; m < P; ++m) {
            const int o = stftd_swz<M>(lane + 64 * m);
            v[m] = f32x2{zr[o], zi[o]};
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = lane + 64 * b, k = j & (LS - 1);
        f32x2 u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = v[b + NB * r];
        if constexpr (LS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[r * k * (2 * M / (LS * R))]);
        }
        stftd_bfly<R>(u);
        const int j0 = (j / LS) * (LS * R) + k;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int o = stftd_swz<M>(j0 + LS * q);
            zr[o] = u[stftd_rev<R>(q)].x;
            zi[o] = u[stftd_rev<R>(q)].y;
        }
    }
    __syncthreads();
}

// Frame f of clip x (T samples) at one resolution: mag[r] = sqrt(max(|X[k]|^2, 1e-7)) of bin k = lane + 64 r (k <= NFFT / 2; other
// entries are left 0).  zr, zi [NFFT / 2] are the calling wave's own LDS; every wave of the block makes the call (the barriers are
// the block's).  The arithmetic is the same whatever the mode, the clip's place in the launch or the wave.
template <int NFFT> __device__ __forceinline__ void stftd_frame(global_ptr<const float> x, long T, long f, const float* tab, int hop,
                                                                float* zr, float* zi, int lane, float (&mag)[NFFT / 128 + 1]) {
    constexpr int M = NFFT / 2, P = M / 64;
    const global_ptr<const float> win = (global_ptr<const float>)tab;
    const global_ptr<const f32x2> tw = (global_ptr<const f32x2>)(tab + NFFT);
    const long base = f * hop - M;
    f32x2 v[P];
    // gather: z[j] = w[2j] x[2j] + i w[2j + 1] x[2j + 1], lane takes j = lane + 64 m.  T > n_fft / 2 makes one reflection enough:
    // base >= -M gives -n <= M <= T - 1, and (F - 1) hop <= T gives n <= T + M - 1, 2 (T - 1) - n >= T - 1 - M >= 0
#pragma unroll
    for (int m = 0; m < P; ++m) {
        const int j = lane + 64 * m;
        long n0 = base + 2 * j, n1 = n0 + 1;
        n0 = n0 < 0 ? -n0 : (n0 >= T ? 2 * (T - 1) - n0 : n0);
        n1 = n1 < 0 ? -n1 : (n1 >= T ? 2 * (T - 1) - n1 : n1);
        const f32x2 w = *(global_ptr<const f32x2>)(win + 2 * j);
        v[m] = f32x2{x[n0] * w.x, x[n1] * w.y};
    }
    if constexpr (M == 256) {
        stftd_pass<M, 4, 1>(v, zr, zi, tw, lane);
        stftd_pass<M, 4, 4>(v, zr, zi, tw, lane);
        stftd_pass<M, 4, 16>(v, zr, zi, tw, lane);
        stftd_pass<M, 4, 64>(v, zr, zi, tw, lane);
    } else if constexpr (M == 512) {
        stftd_pass<M, 8, 1>(v, zr, zi, tw, lane);
        stftd_pass<M, 8, 8>(v, zr, zi, tw, lane);
        stftd_pass<M, 8, 64>(v, zr, zi, tw, lane);
    } else {
        stftd_pass<M, 4, 1>(v, zr, zi, tw, lane);
        stftd_pass<M, 16, 4>(v, zr, zi, tw, lane);
        stftd_pass<M, 16, 64>(v, zr, zi, tw, lane);
    }
    // split pass: X[k] = (Z[k] + conj Z[M - k]) / 2 - i / 2 exp(-2 pi i k / n_fft) (Z[k] - conj Z[M - k]), k = 0..M, Z[M] = Z[0]
#pragma unroll
    for (int r = 0; r <= P; ++r) {
        const int k = lane + 64 * r;
        mag[r] = 0.f;
        if (k <= M) {
            const int o = stftd_swz<M>(k & (M - 1)), om = stftd_swz<M>((M - k) & (M - 1));
            mag[r] = sqrtf(fmaxf(cpower(real_split_bin(f32x2{zr[o], zi[o]}, f32x2{zr[om], zi[om]}, tw[k])), STFTD_FLOOR));
        }
    }
    __syncthreads();                            // (the next transform's stores wait for these loads)
}

// The clip's first frame of resolution p.r among the per-frame partials: its frames lie resolution after resolution
__device__ __forceinline__ long stftd_part(const StftdClip& d, const StftdPar& p, int r) {
    long at = d.part;
    for (int i = 0; i < r; ++i) at += 1 + d.T / p.hop[i];
    return at;
}

// grid (ceil(max F / STFTD_WAVES), B), 256 threads: wave w of block (x, b) takes frame STFTD_WAVES x + w of clip b.
//   STFTD_MODE_MAGNITUDE: out[k][f] = |X[k]| clamped
//   STFTD_MODE_DISTANCE:  part[3 (first + f) + 0..2] = sums over the bins of (|Y| - |X|)^2, |Y|^2 and |log|Y| - log|X||: the lane's own
//   bins in ascending order, then the xor butterfly over the wave: a fixed order
template <int NFFT> __device__ __forceinline__ void stftd_block(const StftdClip& d, const StftdPar& p, int mode, float* part) {
    constexpr int M = NFFT / 2, P = M / 64;
    __shared__ float lds[STFTD_WAVES][2 * M];
    const int hop = p.hop[p.r];
    const long F = 1 + d.T / hop;
    const long f0 = (long)blockIdx.x * STFTD_WAVES;
    if (f0 >= F) return;                                        // (the whole block: no barrier is left waiting)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = f0 + wave;
    const bool valid = f < F;
    const long fr = valid ? f : F - 1;                          // a wave past the clip's end keeps the barriers company
    float* zr = lds[wave];
    float* zi = zr + M;
    float mx[P + 1];
    stftd_frame<NFFT>((global_ptr<const float>)d.x, d.T, fr, p.tab, hop, zr, zi, lane, mx);
    if (mode == STFTD_MODE_MAGNITUDE) {
        if (valid) {
            const global_ptr<float> out = (global_ptr<float>)d.out;
#pragma unroll
            for (int r = 0; r <= P; ++r) {
                const int k = lane + 64 * r;
                if (k <= M) out[(long)k * F + f] = mx[r];
            }
        }
        return;
    }
    float my[P + 1];
    stftd_frame<NFFT>((global_ptr<const float>)d.y, d.T, fr, p.tab, hop, zr, zi, lane, my);
    float sd = 0.f, sy = 0.f, sl = 0.f;
#pragma unroll
    for (int r = 0; r <= P; ++r) {
        if (lane + 64 * r <= M) {
            const float e = my[r] - mx[r];
            sd = fmaf(e, e, sd);
            sy = fmaf(my[r], my[r], sy);
            sl += fabsf(logf(my[r]) - logf(mx[r]));
        }
    }
    sd = wave_sum(sd);
    sy = wave_sum(sy);
    sl = wave_sum(sl);
    if (valid && lane == 0) {
        const global_ptr<float> o = (global_ptr<float>)part + 3 * (stftd_part(d, p, p.r) + f);
        o[0] = sd;
        o[1] = sy;
        o[2] = sl;
    }
}

// A pair's distance from its per-frame partials, resolution after resolution: lane l adds frames l, l + 64, ... in ascending order,
// the xor butterfly adds the lanes; sc = sqrt(sum (|Y| - |X|)^2) / sqrt(sum |Y|^2), mag = sum |log|Y| - log|X|| / (bins F).  The
// order depends on the clip's length alone.  out[0] = (sum over r, ascending, of (sc_r + mag_r)) / n_res, out[1 + 2r], out[2 + 2r] =
// sc_r, mag_r
__device__ __forceinline__ void stftd_reduce_block(const StftdClip& d, const StftdPar& p, const float* part) {
    const int lane = threadIdx.x;
    const global_ptr<float> out = (global_ptr<float>)d.out;
    long at = d.part;
    float total = 0.f;
    for (int r = 0; r < p.n_res; ++r) {
        const long F = 1 + d.T / p.hop[r];
        const global_ptr<const float> q = (global_ptr<const float>)part + 3 * at;
        float sd = 0.f, sy = 0.f, sl = 0.f;
        for (long i = lane; i < F; i += 64) {
            sd += q[3 * i];
            sy += q[3 * i + 1];
            sl += q[3 * i + 2];
        }
        sd = wave_sum(sd);
        sy = wave_sum(sy);
        sl = wave_sum(sl);
        const float sc = sqrtf(sd) / sqrtf(sy);
        const float mg = sl / ((float)(p.n_fft[r] / 2 + 1) * (float)F);
        if (lane == 0) {
            out[1 + 2 * r] = sc;
            out[2 + 2 * r] = mg;
        }
        total += sc + mg;
        at += F;
    }
    if (lane == 0) out[0] = total / (float)p.n_res;
}

template <int NFFT, class D> __global__ __launch_bounds__(256) void stftd_frame_kernel(const D d, const StftdPar p, int mode,
                                                                                       float* __restrict__ part) {
    stftd_block<NFFT>(d.clip[blockIdx.y], p, mode, part);
}
template <class D> __global__ __launch_bounds__(64) void stftd_reduce_kernel(const D d, const StftdPar p, const float* __restrict__ part) {
    stftd_reduce_block(d.clip[blockIdx.x], p, part);
}

static size_t stftd_desc_bytes(int B) { return ((size_t)B * sizeof(StftdClip) + 15) / 16 * 16; }

static bool stftd_res_ok(int n_fft, int hop, int win) {
    return (n_fft == 512 || n_fft == 1024 || n_fft == 2048) && hop >= 1 && hop <= n_fft && win >= 1 && win <= n_fft;
}

static bool stftd_params_ok(int n_res, const int32_t* n_fft, const int32_t* hop, const int32_t* win, const char* who) {
    if (n_res < 1 || n_res > STFTD_MAX_RES) { set_error(std::string(who) + ": n_res outside 1..8"); return false; }
    if (!n_fft || !hop || !win) { set_error(std::string(who) + ": null parameter array"); return false; }
    for (int r = 0; r < n_res; ++r) {
        const std::string at = std::string(who) + ": resolution " + std::to_string(r) + ": ";
        if (n_fft[r] != 512 && n_fft[r] != 1024 && n_fft[r] != 2048) { set_error(at + "n_fft must be 512, 1024 or 2048"); return false; }
        if (hop[r] < 1 || hop[r] > n_fft[r]) { set_error(at + "hop outside 1..n_fft"); return false; }
        if (win[r] < 1 || win[r] > n_fft[r]) { set_error(at + "win_length outside 1..n_fft"); return false; }
    }
    return true;
}

// The periodic Hann window of win samples, zero-padded to n_fft with (n_fft - win) / 2 zeros on the left: float64, rounded once.
// win = 1 is the window [1.], as torch.hann_window(1) gives (the formula alone would give [0.])
static void stftd_window(int n_fft, int win, float* w) {
    const double pi = 3.14159265358979323846;
    const int left = (n_fft - win) / 2;
    for (int n = 0; n < n_fft; ++n) w[n] = 0.f;
    for (int n = 0; n < win; ++n) w[left + n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * n / win));
    if (win == 1) w[left] = 1.f;
}

template <class D> static void stftd_launch_frames(int n_fft, dim3 grid, hipStream_t s, const D& d, const StftdPar& p, int mode, float* part) {
    if (n_fft == 512) hipLaunchKernelGGL((stftd_frame_kernel<512, D>), grid, dim3(64 * STFTD_WAVES), 0, s, d, p, mode, part);
    else if (n_fft == 1024) hipLaunchKernelGGL((stftd_frame_kernel<1024, D>), grid, dim3(64 * STFTD_WAVES), 0, s, d, p, mode, part);
    else hipLaunchKernelGGL((stftd_frame_kernel<2048, D>), grid, dim3(64 * STFTD_WAVES), 0, s, d, p, mode, part);
}

// dist: the distance over every resolution of the handle; else the magnitudes of resolution res
static int stftd_run(const wt_stftd* h, bool dist, int res, const wt_stftd_clip* clips, int32_t B, void* workspace, void* stream,
                     const char* name) {
    const std::string fn = name;
    if (!ragged_call_ok(fn, h, clips, workspace, B, 65535)) return WT_ERR_INVALID;
    bool sound = h->n_res >= 1 && h->n_res <= STFTD_MAX_RES && h->tab;
    for (int r = 0; sound && r < h->n_res; ++r) sound = stftd_res_ok(h->n_fft[r], h->hop[r], h->win[r]);
    if (!sound) { set_error(fn + ": not a handle of wt_stftd_create"); return WT_ERR_INVALID; }
    if (!dist && (res < 0 || res >= h->n_res)) { set_error(fn + ": no such resolution"); return WT_ERR_INVALID; }
    int need = 0;                               // the reflect padding of the widest transform of the call
    for (int r = 0; r < h->n_res; ++r)
        if (dist || r == res) need = std::max(need, h->n_fft[r] / 2);
    std::vector<StftdClip> dev((size_t)B);
    int64_t max_frames[STFTD_MAX_RES] = {}, total = 0;
    for (int b = 0; b < B; ++b) {
        const wt_stftd_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.estimate) { set_error(who + "null estimate"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null out"); return WT_ERR_INVALID; }
        if (dist && !c.target) { set_error(who + "null target"); return WT_ERR_INVALID; }
        if (c.length <= need) { set_error(who + "length <= n_fft / 2 (reflect padding needs more)"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.estimate) % sizeof(float) || reinterpret_cast<uintptr_t>(c.out) % sizeof(float) ||
            (dist && reinterpret_cast<uintptr_t>(c.target) % sizeof(float))) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        dev[b] = StftdClip{c.estimate, dist ? c.target : nullptr, c.out, (long)c.length, (long)total};
        for (int r = 0; r < h->n_res; ++r) {
            const int64_t F = 1 + c.length / h->hop[r];
            max_frames[r] = std::max(max_frames[r], F);
            if (dist) total += F;
        }
    }
    for (int r = 0; r < h->n_res; ++r)
        if ((max_frames[r] + STFTD_WAVES - 1) / STFTD_WAVES > 0x7fffffffLL) { set_error(fn + ": clip too long for one launch"); return WT_ERR_INVALID; }
    if (!on_current_device(fn, h->device)) return WT_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    StftdPar par{};
    par.n_res = h->n_res;
    for (int r = 0; r < h->n_res; ++r) { par.hop[r] = h->hop[r]; par.n_fft[r] = h->n_fft[r]; }
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + stftd_desc_bytes(B));
    if (int rc = launch_ragged<STFTD_ARG_CLIPS>(name, dev.data(), B, 128, workspace, s, [&](auto d) {
        for (int r = 0; r < h->n_res; ++r) {
            if (!dist && r != res) continue;
            StftdPar p = par;
            p.r = r;
            p.tab = h->tab + h->off[r];
            const dim3 grid((unsigned)((max_frames[r] + STFTD_WAVES - 1) / STFTD_WAVES), (unsigned)B);
            stftd_launch_frames(h->n_fft[r], grid, s, d, p, dist ? STFTD_MODE_DISTANCE : STFTD_MODE_MAGNITUDE, part);
        }
        if (dist) hipLaunchKernelGGL(stftd_reduce_kernel<decltype(d)>, dim3((unsigned)B), dim3(64), 0, s, d, par, part);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // namespace wt

using namespace wt;

extern "C" {

int wt_stftd_create(int32_t n_res, const int32_t* n_fft, const int32_t* hop, const int32_t* win_length, int32_t device, wt_stftd** out) {
    if (!out) { set_error("wt_stftd_create: null out"); return WT_ERR_INVALID; }
    if (!stftd_params_ok(n_res, n_fft, hop, win_length, "wt_stftd_create")) return WT_ERR_INVALID;
    wt_stftd* h = new wt_stftd();
    size_t words = 0;
    for (int r = 0; r < n_res; ++r) {
        h->n_fft[r] = n_fft[r]; h->hop[r] = hop[r]; h->win[r] = win_length[r];
        h->off[r] = (int)words;
        words += (size_t)3 * n_fft[r];
    }
    std::vector<float> tab(words, 0.f);
    for (int r = 0; r < n_res; ++r) {
        stftd_window(n_fft[r], win_length[r], tab.data() + h->off[r]);
        fill_twiddles(tab.data() + h->off[r] + n_fft[r], n_fft[r]);
    }
    float* dtab = nullptr;
    if (int rc = upload_table("wt_stftd_create", device, tab, &dtab)) { delete h; return rc; }
    h->device = device; h->n_res = n_res; h->tab = dtab;
    *out = h;
    return WT_OK;
}

void wt_stftd_destroy(wt_stftd* h) {
    if (!h) return;
    (void)hipFree(h->tab);
    delete h;
}

int64_t wt_stftd_frames(const wt_stftd* h, int32_t r, int64_t T) {
    if (!h || r < 0 || r >= h->n_res || r >= STFTD_MAX_RES || h->hop[r] < 1 || T <= h->n_fft[r] / 2) return -1;
    return 1 + T / h->hop[r];
}

int wt_stftd_tables(int32_t n_fft, int32_t win_length, float* window) {
    if (!stftd_params_ok(1, &n_fft, &n_fft, &win_length, "wt_stftd_tables")) return WT_ERR_INVALID;
    if (window) stftd_window(n_fft, win_length, window);
    return WT_OK;
}

size_t wt_stftd_workspace_bytes(const wt_stftd* h, int32_t B, int64_t total_frames) {
    if (!h || B < 1 || total_frames < 0) return 0;
    return stftd_desc_bytes(B) + (size_t)total_frames * 3 * sizeof(float);
}

int wt_stftd_distance(const wt_stftd* h, const wt_stftd_clip* clips, int32_t B, void* workspace, void* stream) {
    return stftd_run(h, true, 0, clips, B, workspace, stream, "wt_stftd_distance");
}

int wt_stftd_magnitude(const wt_stftd* h, int32_t r, const wt_stftd_clip* clips, int32_t B, void* workspace, void* stream) {
    return stftd_run(h, false, r, clips, B, workspace, stream, "wt_stftd_magnitude");
}

}  // extern "C"
