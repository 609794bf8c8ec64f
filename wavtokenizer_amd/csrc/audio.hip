// Helpers on either side of the hot path: channel mix + resample to the codec rate, float -> PCM16,
// and the linear overlap-add of segment outputs.  All memory-bound, one pass over the samples each.
#include "../../include/wavtokenizer_amd.h"
#include "common.h"
#include "fft.h"
#include "ragged.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

// (tests/test_encode_codes_host.py mirrors this layout in ctypes to hand wt_ingest descriptors without a GPU: keep the two in step)
struct wt_resampler {
    int device = 0;
    int orig = 1, nw = 1, K = 0, width = 0;     // gcd-reduced rates, taps per phase, half width
    float* kern = nullptr;                      // [nw][K]
};

namespace wt {

// convert_audio (encoder/utils.py:79-92): mean over channels, then torchaudio.transforms.Resample(sr, target_sr):
// polyphase windowed sinc, out[n] = sum_k kern[n % new][k] * xpad[(n / new) * orig + k], xpad = x shifted by `width`
// zeros.  A block produces 256 consecutive outputs of one clip from an LDS window of the mixed input.
__global__ __launch_bounds__(256) void resample_mono_kernel(const float* __restrict__ wav, const float* __restrict__ kern,
                                                            float* __restrict__ out, int C, long T, long Tout, int orig,
                                                            int nw, int K, int width) {
    extern __shared__ float win[];
    const long n0 = (long)blockIdx.x * 256;
    const int b = blockIdx.y;
    const long i0 = n0 / nw;
    const long nlast = (n0 + 255 < Tout ? n0 + 255 : Tout - 1);
    const long i1 = nlast / nw;
    const long p0 = i0 * orig - width;                     // input position of win[0]
    const int Lw = (int)((i1 - i0) * orig) + K;
    const float inv = 1.f / (float)C;
    for (int e = threadIdx.x; e < Lw; e += 256) {
        const long p = p0 + e;
        float v = 0.f;
        if (p >= 0 && p < T) {
            for (int c = 0; c < C; ++c) v += wav[((long)b * C + c) * T + p];
            if (C > 1) v *= inv;
        }
        win[e] = v;
    }
    __syncthreads();
    const long n = n0 + threadIdx.x;
    if (n >= Tout) return;
    const long i = n / nw;
    const int ph = (int)(n - i * nw);
    const float* kp = kern + (long)ph * K;
    const float* wp = win + (i - i0) * orig;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(kp[k], wp[k], acc);
    out[(long)b * Tout + n] = acc;
}

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));      // non-negative floats order like their bits
}

// One clip of a ragged ingest launch (device form of wt_ingest_clip): the source array with its element strides, the clip's
// resampler and both lengths.
struct IngestClip {
    const void* src;
    const float* kern;                          // [nw][K]
    long n_in, n_out;
    long cstride, sstride;                      // elements between channels / between samples
    int i16, C;                                 // int16 source (else fp32); 1 or 2 channels
    int orig, nw, K, width;
};

__device__ __forceinline__ float ingest_sample(const IngestClip& d, long p) {
    float v = 0.f;
    if (d.i16) {
        const int16_t* s = static_cast<const int16_t*>(d.src);
        for (int c = 0; c < d.C; ++c) v += (float)s[c * d.cstride + p * d.sstride] * (1.f / 32768.f);
    } else {
        const float* s = static_cast<const float*>(d.src);
        for (int c = 0; c < d.C; ++c) v += s[c * d.cstride + p * d.sstride];
    }
    return d.C > 1 ? v * (1.f / (float)d.C) : v;
}

// resample_mono_kernel over clips of different rates, channel counts, layouts, sample types and lengths in one launch: grid
// (ceil(max n_out / 256), B), row b of out [B][T_pad] receives clip b's n_out samples, the same bits as resample_mono_kernel
// on the clip alone as planar fp32 (int16 / 32768 is exact; same channel sum, same ascending fmaf chain).  Columns from n_out
// on are not written.  The descriptor is uniform over the block.
__global__ __launch_bounds__(256) void ingest_kernel(const IngestClip* __restrict__ clips, float* __restrict__ out, long T_pad) {
    extern __shared__ float win[];
    const IngestClip d = clips[blockIdx.y];
    const long n0 = (long)blockIdx.x * 256;
    if (n0 >= d.n_out) return;
    const long i0 = n0 / d.nw;
    const long nlast = (n0 + 255 < d.n_out ? n0 + 255 : d.n_out - 1);
    const long i1 = nlast / d.nw;
    const long p0 = i0 * d.orig - d.width;                 // input position of win[0]
    const int Lw = (int)((i1 - i0) * d.orig) + d.K;
    for (int e = threadIdx.x; e < Lw; e += 256) {
        const long p = p0 + e;
        win[e] = (p >= 0 && p < d.n_in) ? ingest_sample(d, p) : 0.f;
    }
    __syncthreads();
    const long n = n0 + threadIdx.x;
    if (n >= d.n_out) return;
    const long i = n / d.nw;
    const int ph = (int)(n - i * d.nw);
    const float* kp = d.kern + (long)ph * d.K;
    const float* wp = win + (i - i0) * d.orig;
    float acc = 0.f;
    for (int k = 0; k < d.K; ++k) acc = fmaf(kp[k], wp[k], acc);
    out[(long)blockIdx.y * T_pad + n] = acc;
}

// round-half-even of x * 32768 clipped to int16: the PCM_S 16 conversion (what pcm16_kernel stores)
__device__ __forceinline__ int pcm16_round(float v) {
    const float r = rintf(v * 32768.f);
    return (int)fminf(fmaxf(r, -32768.f), 32767.f);
}

// One clip of a ragged emit launch (device form of wt_emit_clip): the fp32 row at the codec rate, the destination with its
// element strides, the clip's resampler and both lengths.
struct EmitClip {
    const float* src;
    const float* kern;                          // [nw][K]
    void* dst;
    long n_in, n_out;
    long cstride, sstride;                      // elements between channels / between samples
    int i16, C;                                 // int16 destination (else fp32); 1 or 2 channels
    int orig, nw, K, width;
    float limit;
};

// (the descriptors' pointers are device pointers by contract: global_ptr, fft.h)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int EMIT_COPY_SPAN = 2048;            // samples per block of an equal-rate clip: two rounds of four per thread

// The lanes of a wave hold consecutive int16 samples base[n]: two samples that share an aligned 4-byte word leave as one store
// of the lane that holds the lower one.  A sample without its partner (the word's other half lies before the clip, behind it or
// in the next wave) is a 2-byte store.  Every lane of the wave calls this (the shuffle needs them), valid or not.
__device__ __forceinline__ void store_i16_run(global_ptr<int16_t> base, long n, int q, bool valid, bool next_valid) {
    const int lane = threadIdx.x & 63;
    const int qn = __shfl_down(q, 1, 64);
    if (!valid) return;
    global_ptr<int16_t> p = base + n;
    if (((uintptr_t)p & 2) == 0) {
        if (lane < 63 && next_valid) *(global_ptr<uint32_t>)p = (uint32_t)(uint16_t)q | ((uint32_t)(uint16_t)qn << 16);
        else *p = (int16_t)q;
    } else if (lane == 0) {
        *p = (int16_t)q;                        // (any other lane's sample left with its left neighbour's)
    }
}

// An equal-rate clip (K = 1, the table's only tap; n_out = n_in): the window of output n is src[n] alone and the chain one fmaf, so
// nothing goes through LDS, and a block takes EMIT_COPY_SPAN samples instead of 256: per round a thread loads four consecutive
// samples (16 bytes where the row is 16-byte aligned) and stores them in the widest form the destination's alignment allows: fp32
// runs as 16 bytes; int16 runs as 8 bytes, two 4-byte words, or 2 + 4 + 2 bytes on an odd element; interleaved stereo frames as
// 16 bytes (int16: four frames; fp32: two) or one store per frame.  A tail of fewer than four samples and any other strides get
// one store per element.  The same values as emit_block's general path, bit for bit.
// MODE (emit_block): EMIT_PLAIN as described; EMIT_RESCALED: every sample times s instead of the clamp, one rounded product
// (pcm16_kernel's rescale); EMIT_PEAK: nothing is stored, the largest |sample| of the block goes to *peak instead (as absmax_kernel:
// an integer atomicMax on the bits of a non-negative float, the same in any order).
enum : int { EMIT_PLAIN = 0, EMIT_RESCALED = 1, EMIT_PEAK = 2 };

// every lane of the wave calls this
__device__ __forceinline__ void emit_peak_wave(float m, unsigned* peak) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(peak, __float_as_uint(m));
}

template <int MODE> __device__ __forceinline__ void emit_copy_block(const EmitClip& d, float s, unsigned* peak) {
    const long base = (long)blockIdx.x * EMIT_COPY_SPAN;
    if (base >= d.n_out) return;
    const global_ptr<const float> src = (global_ptr<const float>)d.src;
    const float k0 = ((global_ptr<const float>)d.kern)[0];
    const bool frames = d.C == 2 && d.cstride == 1 && d.sstride == 2;      // interleaved stereo
    const bool src16 = (uintptr_t)src % 16 == 0;
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < EMIT_COPY_SPAN / 1024; ++j) {
        const long n = base + j * 1024 + 4 * (long)threadIdx.x;
        if (n >= d.n_out) {
            if (MODE == EMIT_PEAK) break;
            return;
        }
        const int m = d.n_out - n < 4 ? (int)(d.n_out - n) : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (m == 4 && src16) {
            const f32x4 x = *(global_ptr<const f32x4>)(src + n);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < m) v[i] = src[n + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaf(k0, 0.f + v[i], 0.f);      // (resample_mono_kernel's channel sum, then its chain)
        if (MODE == EMIT_PEAK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < m) mx = fmaxf(mx, fabsf(v[i]));
            continue;
        }
        if (MODE == EMIT_RESCALED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] * s;
        }
        if (!d.i16) {
            const global_ptr<float> o = (global_ptr<float>)d.dst;
            if (frames && (uintptr_t)o % 8 == 0) {
                const global_ptr<float> p = o + 2 * n;
                if (m == 4 && (uintptr_t)p % 16 == 0) {
                    ((global_ptr<f32x4>)p)[0] = f32x4{v[0], v[0], v[1], v[1]};
                    ((global_ptr<f32x4>)p)[1] = f32x4{v[2], v[2], v[3], v[3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < m) ((global_ptr<f32x2>)p)[i] = f32x2{v[i], v[i]};
                }
            } else if (d.sstride == 1) {
                for (int c = 0; c < d.C; ++c) {
                    const global_ptr<float> p = o + c * d.cstride + n;
                    if (m == 4 && (uintptr_t)p % 16 == 0) {
                        *(global_ptr<f32x4>)p = f32x4{v[0], v[1], v[2], v[3]};
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (i < m) p[i] = v[i];
                    }
                }
            } else {
                for (int c = 0; c < d.C; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < m) o[c * d.cstride + (n + i) * d.sstride] = v[i];
            }
            continue;
        }
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = (uint32_t)(uint16_t)pcm16_round(MODE == EMIT_RESCALED ? v[i] : fminf(fmaxf(v[i], -d.limit), d.limit));
        const global_ptr<int16_t> o = (global_ptr<int16_t>)d.dst;
        if (frames && (uintptr_t)o % 4 == 0) {
            const global_ptr<uint32_t> p = (global_ptr<uint32_t>)(o + 2 * n);
            if (m == 4 && (uintptr_t)p % 16 == 0) {
                *(global_ptr<u32x4>)p = u32x4{q[0] * 0x10001u, q[1] * 0x10001u, q[2] * 0x10001u, q[3] * 0x10001u};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (i < m) p[i] = q[i] * 0x10001u;
            }
        } else if (d.sstride == 1) {
            for (int c = 0; c < d.C; ++c) {
                const global_ptr<int16_t> p = o + c * d.cstride + n;
                const int a = (int)(((uintptr_t)p >> 1) & 3);              // the run's first element within its 8-byte word
                if (m < 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < m) p[i] = (int16_t)q[i];
                } else if (a == 0) {
                    *(global_ptr<u32x2>)p = u32x2{q[0] | (q[1] << 16), q[2] | (q[3] << 16)};
                } else if (a == 2) {
                    ((global_ptr<uint32_t>)p)[0] = q[0] | (q[1] << 16);
                    ((global_ptr<uint32_t>)p)[1] = q[2] | (q[3] << 16);
                } else {
                    p[0] = (int16_t)q[0];
                    *(global_ptr<uint32_t>)(p + 1) = q[1] | (q[2] << 16);
                    p[3] = (int16_t)q[3];
                }
            }
        } else {
            for (int c = 0; c < d.C; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) if (i < m) o[c * d.cstride + (n + i) * d.sstride] = (int16_t)q[i];
        }
    }
    if (MODE == EMIT_PEAK) emit_peak_wave(mx, peak);
}

// The mirror of ingest_kernel: grid (ceil(max n_out / 256), B), block (x, b) resamples 256 consecutive outputs of row b (fp32 mono
// at the codec rate) to the clip's own rate, the same bits as resample_mono_kernel on the row alone with C = 1 (same window, zeros
// outside [0, n_in), same ascending fmaf chain), and writes them to the clip's destination: fp32 as they are, int16 through
// pcm16_kernel's clamp and rounding; a stereo clip gets the value in both channels.  Nothing past src[n_in - 1] is read and
// nothing outside the clip's n_out * C destination elements is written.  The descriptor is uniform over the block, and so is
// the choice of the store form: one 8- / 4-byte store per interleaved stereo frame, paired int16 stores for runs with sample
// stride 1 (store_i16_run), one store per element for any other strides.  An equal-rate clip takes emit_copy_block's wider blocks
// instead (the host sizes the grid for whichever form each clip takes).
__host__ __device__ inline bool emit_is_copy(int orig, int nw, int K, int width) { return K == 1 && width == 0 && orig == 1 && nw == 1; }

template <int MODE> __device__ __forceinline__ void emit_block(const EmitClip& d, float s, unsigned* peak) {
    extern __shared__ float win[];
    if (emit_is_copy(d.orig, d.nw, d.K, d.width)) { emit_copy_block<MODE>(d, s, peak); return; }
    const long n0 = (long)blockIdx.x * 256;
    if (n0 >= d.n_out) return;
    const long n = n0 + threadIdx.x;
    const bool valid = n < d.n_out;
    const global_ptr<const float> src = (global_ptr<const float>)d.src;
    const global_ptr<const float> kern = (global_ptr<const float>)d.kern;
    const long i0 = n0 / d.nw;
    const long nlast = (n0 + 255 < d.n_out ? n0 + 255 : d.n_out - 1);
    const long i1 = nlast / d.nw;
    const long p0 = i0 * d.orig - d.width;                 // input position of win[0]
    const int Lw = (int)((i1 - i0) * d.orig) + d.K;
    for (int e = threadIdx.x; e < Lw; e += 256) {
        const long p = p0 + e;
        win[e] = (p >= 0 && p < d.n_in) ? 0.f + src[p] : 0.f;        // (resample_mono_kernel's channel sum over one channel)
    }
    __syncthreads();
    float acc = 0.f;
    if (valid) {
        const long i = n / d.nw;
        const int ph = (int)(n - i * d.nw);
        const global_ptr<const float> kp = kern + (long)ph * d.K;
        const float* wp = win + (i - i0) * d.orig;
        for (int k = 0; k < d.K; ++k) acc = fmaf(kp[k], wp[k], acc);
    }
    if (MODE == EMIT_PEAK) { emit_peak_wave(valid ? fabsf(acc) : 0.f, peak); return; }
    if (MODE == EMIT_RESCALED) acc = acc * s;
    const bool frames = d.C == 2 && d.cstride == 1 && d.sstride == 2;      // interleaved stereo
    if (!d.i16) {
        if (!valid) return;
        const global_ptr<float> o = (global_ptr<float>)d.dst;
        if (frames && (uintptr_t)o % 8 == 0) {
            ((global_ptr<f32x2>)o)[n] = f32x2{acc, acc};
        } else {
            for (int c = 0; c < d.C; ++c) o[c * d.cstride + n * d.sstride] = acc;
        }
        return;
    }
    const int q = pcm16_round(MODE == EMIT_RESCALED ? acc : fminf(fmaxf(acc, -d.limit), d.limit));
    const global_ptr<int16_t> o = (global_ptr<int16_t>)d.dst;
    if (frames && (uintptr_t)o % 4 == 0) {
        if (valid) ((global_ptr<uint32_t>)o)[n] = (uint32_t)(uint16_t)q * 0x10001u;
    } else if (d.sstride == 1) {
        for (int c = 0; c < d.C; ++c) store_i16_run(o + c * d.cstride, n, q, valid, n + 1 < d.n_out);
    } else if (valid) {
        for (int c = 0; c < d.C; ++c) o[c * d.cstride + n * d.sstride] = (int16_t)q;
    }
}

// D: the descriptors in the kernel's argument block (up to EMIT_ARG_CLIPS clips) or in the workspace (ragged.h).  The block takes
// its descriptor into registers first, as ingest_kernel does: read in place from the workspace, where nothing says that the block's
// stores leave it alone, its fields are fetched again behind them (36 VGPRs instead of 30, up to 4 % more device time).
constexpr int EMIT_ARG_CLIPS = 64;
template <class D> __global__ __launch_bounds__(256) void emit_kernel(const D d) {
    const EmitClip c = d.clip[blockIdx.y];
    emit_block<EMIT_PLAIN>(c, 1.f, nullptr);
}

// (a kernel, not hipMemsetAsync: a launch like the two behind it, at a launch's host cost)
__global__ __launch_bounds__(256) void emit_zero_peaks_kernel(unsigned* __restrict__ peaks, int B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) peaks[i] = 0u;
}

// wt_emit_rescaled's two launches over one grid: EMIT_PEAK leaves max |sample| of clip b's resampled output in peaks[b] (zeroed
// before the launch), EMIT_RESCALED emits every sample times s = min(limit / peak, 1) (pcm16_kernel's rule: 1 for a silent clip)
template <class D, int MODE> __global__ __launch_bounds__(256) void emit_level_kernel(const D d, unsigned* peaks) {
    const EmitClip c = d.clip[blockIdx.y];
    float s = 1.f;
    if (MODE == EMIT_RESCALED) {
        const float mx = __uint_as_float(peaks[blockIdx.y]);
        s = mx > 0.f ? fminf(c.limit / mx, 1.f) : 1.f;
    }
    emit_block<MODE>(c, s, peaks + blockIdx.y);
}

// The ragged way out: spans [B][2] = {L_b, offset_b}; the first L_b codes of row b of codes [B][L_pad] go to out[offset_b + t].
// A span that does not fit its row or the flat tensor is skipped whole.
__global__ __launch_bounds__(256) void codes_unpack_kernel(const int64_t* __restrict__ codes, long L_pad, const int64_t* __restrict__ spans,
                                                           int64_t* __restrict__ out, long out_numel) {
    const int b = blockIdx.y;
    const long L = spans[2 * b], off = spans[2 * b + 1];
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (L < 0 || L > L_pad || off < 0 || off > out_numel - L || t >= L) return;
    out[off + t] = codes[(long)b * L_pad + t];
}

// save_audio (encoder/utils.py:95-103) + PCM_S 16: clamp to +-limit (or scale by min(limit / max|x|, 1)), then
// round-half-even of x * 32768 clipped to int16
__global__ __launch_bounds__(256) void pcm16_kernel(const float* __restrict__ x, long n, float limit, int rescale,
                                                    const unsigned* __restrict__ amax, int16_t* __restrict__ out) {
    float scale = 1.f;
    if (rescale) {
        const float mx = __uint_as_float(*amax);
        scale = mx > 0.f ? fminf(limit / mx, 1.f) : 1.f;
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = x[i];
        v = rescale ? v * scale : fminf(fmaxf(v, -limit), limit);
        out[i] = (int16_t)pcm16_round(v);
    }
}

// _linear_overlap_add (encoder/utils.py:17-56): out[r][t] = (sum_f w[t - f stride] * frame_f[r][t - f stride]) / (sum_f
// w[t - f stride]) over the frames covering t, added in frame order with separately rounded products and sums like
// the reference's `out += weight * frame` loop (bit-identical)
__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ frames, const float* __restrict__ w,
                                                          int nf, long rows, long flen, long last_len, long stride,
                                                          long total, float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long r = blockIdx.y;
    if (t >= total) return;
    long f0 = t >= flen ? (t - flen) / stride + 1 : 0;      // first frame with f*stride + flen > t
    float acc = 0.f, sw = 0.f;
    for (long f = f0; f < nf && f * stride <= t; ++f) {
        const long o = t - f * stride;
        const long len = f + 1 == nf ? last_len : flen;
        if (o < len) {
            acc = __fadd_rn(acc, __fmul_rn(w[o], frames[((long)f * rows + r) * flen + o]));
            sw = __fadd_rn(sw, w[o]);
        }
    }
    out[r * total + t] = acc / sw;
}

// overlap_add_kernel over recordings of different frame counts, frame lengths, strides and lengths in one launch (wt_overlap_add_ragged):
// grid (ceil(max total / 256), B), block (x, b) writes 256 consecutive outputs of recording b.  Frame f of a recording is the row
// rows[f], valid up to len_f = min(frame_len, total - f * stride): every frame covering t < total holds t, so a row is never read
// past len_f - 1.  The same frames in the same order with the same separately rounded products and sums as overlap_add_kernel, one
// division: bit-identical to it and to the reference's loop.  The descriptor is uniform over the block; reads of a frame and the
// writes are consecutive along t.
__device__ __forceinline__ void overlap_add_block(const wt_overlap_add_clip& d) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= d.total) return;
    const global_ptr<const float> w = (global_ptr<const float>)d.weight;
    const global_ptr<const float* const> rows = (global_ptr<const float* const>)d.rows;
    const long flen = d.frame_len, stride = d.stride, nf = d.n_frames;
    long f = t >= flen ? (t - flen) / stride + 1 : 0;       // first frame with f * stride + flen > t
    float acc = 0.f, sw = 0.f;
    for (; f < nf && f * stride <= t; ++f) {
        const long o = t - f * stride;                       // (o < flen by the choice of the first frame, f * stride + o = t < total)
        const global_ptr<const float> row = (global_ptr<const float>)rows[f];
        const float wo = w[o];
        acc = __fadd_rn(acc, __fmul_rn(wo, row[o]));
        sw = __fadd_rn(sw, wo);
    }
    ((global_ptr<float>)d.out)[t] = acc / sw;
}

constexpr int OLA_ARG_CLIPS = 64;           // (as emit_kernel)
template <class D> __global__ __launch_bounds__(256) void overlap_add_ragged_kernel(const D d) { overlap_add_block(d.clip[blockIdx.y]); }

}  // namespace wt

using namespace wt;

extern "C" {

int wt_resampler_create(int32_t orig_sr, int32_t new_sr, int32_t device, wt_resampler** out) {
    if (!out || orig_sr <= 0 || new_sr <= 0) { set_error("wt_resampler_create: bad argument"); return WT_ERR_INVALID; }
    WT_HIP_CHECK(hipSetDevice(device));
    const int g = std::gcd(orig_sr, new_sr);
    const int orig = orig_sr / g, nw = new_sr / g;
    // torchaudio.functional.resample defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99
    // (wavtokenizer_amd/audio.py resampler_geometry restates width, K and the limit below on the host, for callers that must
    // refuse a rate pair before any GPU work: change the two together)
    const int lpw = 6;
    const double rolloff = 0.99;
    const double base = std::min(orig, nw) * rolloff;
    const bool same = orig == nw;             // Resample.forward returns the waveform unchanged at equal rates
    const int width = same ? 0 : (int)std::ceil(lpw * orig / base);
    const int K = same ? 1 : 2 * width + orig;
    if (256.0 * orig / nw + K > 15000) { set_error("wt_resampler_create: rate ratio too large for the LDS window"); return WT_ERR_INVALID; }
    std::vector<float> k((size_t)nw * K);
    const double pi = 3.14159265358979323846;
    for (int p = 0; p < nw; ++p)
        for (int j = 0; j < K; ++j) {
            double t = (-(double)p / nw + (double)(j - width) / orig) * base;
            t = std::min(std::max(t, -(double)lpw), (double)lpw);
            const double window = std::pow(std::cos(t * pi / lpw / 2), 2);
            t *= pi;
            const double sinc = t == 0.0 ? 1.0 : std::sin(t) / t;
            k[(size_t)p * K + j] = same ? 1.f : (float)(sinc * window * (base / orig));
        }
    wt_resampler* r = new wt_resampler();
    r->device = device; r->orig = orig; r->nw = nw; r->K = K; r->width = width;
    if (hipMalloc(reinterpret_cast<void**>(&r->kern), k.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(r->kern, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("wt_resampler_create: device allocation failed");
        delete r;
        return WT_ERR_HIP;
    }
    *out = r;
    return WT_OK;
}

void wt_resampler_destroy(wt_resampler* r) {
    if (!r) return;
    (void)hipFree(r->kern);
    delete r;
}

int64_t wt_resampler_out_length(const wt_resampler* r, int64_t T) {
    return r ? (int64_t)((r->nw * T + r->orig - 1) / r->orig) : 0;       // ceil(new * length / orig)
}

int wt_convert_audio(const wt_resampler* r, const float* wav, int32_t B, int32_t C, int64_t T, float* out, void* stream) {
    if (!r || !wav || !out || B < 1 || T < 1) { set_error("wt_convert_audio: bad argument"); return WT_ERR_INVALID; }
    if (C != 1 && C != 2) { set_error("wt_convert_audio: audio must be mono or stereo (encoder/utils.py:81)"); return WT_ERR_INVALID; }
    WT_HIP_CHECK(hipSetDevice(r->device));
    const int64_t Tout = wt_resampler_out_length(r, T);
    const size_t smem = (size_t)(256 / r->nw + 2) * r->orig * sizeof(float) + (size_t)r->K * sizeof(float);
    static PerDeviceOnce attr_once;
    if (int rc = attr_once.run([&]() -> int {
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_mono_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        return 0;
    })) return rc;
    dim3 grid((unsigned)((Tout + 255) / 256), B);
    hipLaunchKernelGGL(resample_mono_kernel, grid, dim3(256), smem, static_cast<hipStream_t>(stream), wav, r->kern, out, C,
                       (long)T, (long)Tout, r->orig, r->nw, r->K, r->width);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // extern "C"

namespace wt {

// The host-side staging of the ragged calls' descriptors: two pinned blocks per device, each guarded by the event recorded behind
// the copy that last read it, so the upload never waits for the stream and never reads a block that is being rewritten.
struct DescriptorStage {
    std::mutex mu;
    void* host[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int next = 0;
};
static DescriptorStage g_descriptor_stage[64];

int stage_descriptors(const char* who, const void* descs, size_t bytes, size_t min_bytes, void* workspace, hipStream_t s) {
    int device = 0;
    WT_HIP_CHECK(hipGetDevice(&device));
    if (device < 0 || device >= 64) { set_error(std::string(who) + ": device index"); return WT_ERR_INVALID; }
    DescriptorStage& st = g_descriptor_stage[device];
    std::lock_guard<std::mutex> lock(st.mu);
    const int k = st.next;
    st.next ^= 1;
    if (!st.ev[k]) WT_HIP_CHECK(hipEventCreateWithFlags(&st.ev[k], hipEventDisableTiming));
    else WT_HIP_CHECK(hipEventSynchronize(st.ev[k]));
    if (st.cap[k] < bytes) {
        if (st.host[k]) { (void)hipHostFree(st.host[k]); st.host[k] = nullptr; st.cap[k] = 0; }
        const size_t cap = std::max(bytes, min_bytes);
        WT_HIP_CHECK(hipHostMalloc(&st.host[k], cap, hipHostMallocDefault));
        st.cap[k] = cap;
    }
    memcpy(st.host[k], descs, bytes);
    WT_HIP_CHECK(hipMemcpyAsync(workspace, st.host[k], bytes, hipMemcpyHostToDevice, s));
    WT_HIP_CHECK(hipEventRecord(st.ev[k], s));
    return WT_OK;
}

}  // namespace wt

extern "C" {

static size_t resampler_window_bytes(const wt_resampler* r) {
    return (size_t)(256 / r->nw + 2) * r->orig * sizeof(float) + (size_t)r->K * sizeof(float);
}

size_t wt_ingest_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * sizeof(IngestClip) : 0; }

int wt_ingest(const wt_ingest_clip* clips, int32_t B, int64_t T_pad, float* out, void* workspace, void* stream) {
    if (!clips || !out || !workspace || B < 1 || B > 65535 || T_pad < 1) { set_error("wt_ingest: bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(out) % sizeof(float) || reinterpret_cast<uintptr_t>(workspace) % 8) {
        set_error("wt_ingest: out or workspace misaligned"); return WT_ERR_INVALID;
    }
    std::vector<IngestClip> dev((size_t)B);
    size_t smem = 0;
    int64_t max_out = 0;
    const int device = clips[0].resampler ? clips[0].resampler->device : 0;
    for (int b = 0; b < B; ++b) {
        const wt_ingest_clip& c = clips[b];
        const std::string who = "wt_ingest: clip " + std::to_string(b) + ": ";
        if (!c.src) { set_error(who + "null source"); return WT_ERR_INVALID; }
        if (!c.resampler) { set_error(who + "null resampler"); return WT_ERR_INVALID; }
        if (c.dtype != WT_INGEST_F32 && c.dtype != WT_INGEST_I16) { set_error(who + "sample type must be fp32 or int16"); return WT_ERR_INVALID; }
        if (c.channels != 1 && c.channels != 2) { set_error(who + "audio must be mono or stereo (encoder/utils.py:81)"); return WT_ERR_INVALID; }
        if (c.n_in < 1) { set_error(who + "n_in < 1"); return WT_ERR_INVALID; }
        if (c.ch_stride < 0 || c.sample_stride < 0) { set_error(who + "negative stride"); return WT_ERR_INVALID; }
        if (c.n_out != wt_resampler_out_length(c.resampler, c.n_in)) { set_error(who + "n_out is not wt_resampler_out_length(n_in)"); return WT_ERR_INVALID; }
        if (c.n_out > T_pad) { set_error(who + "n_out > T_pad"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.src) % (c.dtype == WT_INGEST_I16 ? sizeof(int16_t) : sizeof(float))) {
            set_error(who + "misaligned source pointer"); return WT_ERR_INVALID;
        }
        if (c.resampler->device != device) { set_error(who + "resampler of another device"); return WT_ERR_INVALID; }
        const size_t w = resampler_window_bytes(c.resampler);
        if (w > 64 * 1024) { set_error(who + "rate ratio too large for the LDS window"); return WT_ERR_INVALID; }
        smem = std::max(smem, w);
        max_out = std::max(max_out, c.n_out);
        dev[b] = IngestClip{c.src, c.resampler->kern, (long)c.n_in, (long)c.n_out, (long)c.ch_stride, (long)c.sample_stride,
                            c.dtype == WT_INGEST_I16 ? 1 : 0, c.channels, c.resampler->orig, c.resampler->nw, c.resampler->K,
                            c.resampler->width};
    }
    WT_HIP_CHECK(hipSetDevice(device));
    static PerDeviceOnce attr_once;
    if (int rc = attr_once.run([&]() -> int {
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ingest_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        return 0;
    })) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = stage_descriptors("wt_ingest", dev.data(), dev.size() * sizeof(IngestClip), 64 * sizeof(IngestClip), workspace, s)) return rc;
    dim3 grid((unsigned)((max_out + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(ingest_kernel, grid, dim3(256), smem, s, static_cast<const IngestClip*>(workspace), out, (long)T_pad);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

size_t wt_emit_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * sizeof(EmitClip) : 0; }

// The descriptors of wt_emit / wt_emit_rescaled (fn) checked and turned into their device form; rescaled: the limit is every
// clip's, whatever its sample type
static int emit_prepare(const std::string& fn, const wt_emit_clip* clips, int32_t B, const void* workspace, bool rescaled,
                        std::vector<EmitClip>& dev, size_t& smem, int64_t& blocks, int& device) {
    if (!clips || !workspace || B < 1 || B > 65535) { set_error(fn + ": bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return WT_ERR_INVALID; }
    dev.resize((size_t)B);
    smem = 0;
    blocks = 0;
    device = clips[0].resampler ? clips[0].resampler->device : 0;
    for (int b = 0; b < B; ++b) {
        const wt_emit_clip& c = clips[b];
        const std::string who = fn + ": clip " + std::to_string(b) + ": ";
        if (!c.src) { set_error(who + "null source"); return WT_ERR_INVALID; }
        if (!c.dst) { set_error(who + "null destination"); return WT_ERR_INVALID; }
        if (!c.resampler) { set_error(who + "null resampler"); return WT_ERR_INVALID; }
        if (c.dtype != WT_EMIT_F32 && c.dtype != WT_EMIT_I16) { set_error(who + "sample type must be fp32 or int16"); return WT_ERR_INVALID; }
        if (c.channels != 1 && c.channels != 2) { set_error(who + "channels must be 1 or 2"); return WT_ERR_INVALID; }
        if (c.n_in < 1) { set_error(who + "n_in < 1"); return WT_ERR_INVALID; }
        if (c.n_out != wt_resampler_out_length(c.resampler, c.n_in)) { set_error(who + "n_out is not wt_resampler_out_length(n_in)"); return WT_ERR_INVALID; }
        if (c.ch_stride < 0 || c.sample_stride < 0) { set_error(who + "negative stride"); return WT_ERR_INVALID; }
        if (c.channels == 2 && ((c.ch_stride == 0 && c.sample_stride < 2) || (c.sample_stride == 1 && c.ch_stride < c.n_out))) {
            set_error(who + "the two channels overlap"); return WT_ERR_INVALID;
        }
        if (reinterpret_cast<uintptr_t>(c.src) % sizeof(float)) { set_error(who + "misaligned source pointer"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.dst) % (c.dtype == WT_EMIT_I16 ? sizeof(int16_t) : sizeof(float))) {
            set_error(who + "misaligned destination pointer"); return WT_ERR_INVALID;
        }
        if ((rescaled || c.dtype == WT_EMIT_I16) && !(c.limit > 0.f && c.limit <= 1.f)) { set_error(who + "limit outside (0, 1]"); return WT_ERR_INVALID; }
        if (c.resampler->device != device) { set_error(who + "resampler of another device"); return WT_ERR_INVALID; }
        const size_t w = resampler_window_bytes(c.resampler);
        if (w > 64 * 1024) { set_error(who + "rate ratio too large for the LDS window"); return WT_ERR_INVALID; }
        smem = std::max(smem, w);
        const wt_resampler* r = c.resampler;
        const int64_t span = emit_is_copy(r->orig, r->nw, r->K, r->width) ? EMIT_COPY_SPAN : 256;     // outputs per block of this clip
        blocks = std::max(blocks, (c.n_out + span - 1) / span);
        dev[b] = EmitClip{c.src, c.resampler->kern, c.dst, (long)c.n_in, (long)c.n_out, (long)c.ch_stride, (long)c.sample_stride,
                          c.dtype == WT_EMIT_I16 ? 1 : 0, c.channels, c.resampler->orig, c.resampler->nw, c.resampler->K,
                          c.resampler->width, rescaled || c.dtype == WT_EMIT_I16 ? c.limit : 1.f};
    }
    return WT_OK;
}

int wt_emit(const wt_emit_clip* clips, int32_t B, void* workspace, void* stream) {
    std::vector<EmitClip> dev;
    size_t smem = 0;
    int64_t blocks = 0;
    int device = 0;
    if (int rc = emit_prepare("wt_emit", clips, B, workspace, false, dev, smem, blocks, device)) return rc;
    WT_HIP_CHECK(hipSetDevice(device));
    static PerDeviceOnce attr_once;
    if (int rc = attr_once.run([&]() -> int {
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_kernel<PtrClips<EmitClip>>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_kernel<ArgClips<EmitClip, EMIT_ARG_CLIPS>>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        return 0;
    })) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)blocks, (unsigned)B);
    if (int rc = launch_ragged<EMIT_ARG_CLIPS>("wt_emit", dev.data(), B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL(emit_kernel<decltype(d)>, grid, dim3(256), smem, s, d);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

size_t wt_emit_rescaled_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * (sizeof(EmitClip) + sizeof(unsigned)) : 0; }

int wt_emit_rescaled(const wt_emit_clip* clips, int32_t B, void* workspace, void* stream) {
    std::vector<EmitClip> dev;
    size_t smem = 0;
    int64_t blocks = 0;
    int device = 0;
    if (int rc = emit_prepare("wt_emit_rescaled", clips, B, workspace, true, dev, smem, blocks, device)) return rc;
    WT_HIP_CHECK(hipSetDevice(device));
    typedef PtrClips<EmitClip> P;
    typedef ArgClips<EmitClip, EMIT_ARG_CLIPS> A;
    static PerDeviceOnce attr_once;
    if (int rc = attr_once.run([&]() -> int {
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_level_kernel<P, EMIT_PEAK>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_level_kernel<P, EMIT_RESCALED>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_level_kernel<A, EMIT_PEAK>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(emit_level_kernel<A, EMIT_RESCALED>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        return 0;
    })) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the peaks lie behind the descriptors' place in the workspace (which a call of up to 64 clips leaves unused)
    unsigned* peaks = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + (size_t)B * sizeof(EmitClip));
    hipLaunchKernelGGL(emit_zero_peaks_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, peaks, (int)B);
    dim3 grid((unsigned)blocks, (unsigned)B);
    if (int rc = launch_ragged<EMIT_ARG_CLIPS>("wt_emit_rescaled", dev.data(), B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL((emit_level_kernel<decltype(d), EMIT_PEAK>), grid, dim3(256), smem, s, d, peaks);
        hipLaunchKernelGGL((emit_level_kernel<decltype(d), EMIT_RESCALED>), grid, dim3(256), smem, s, d, peaks);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

int wt_codes_unpack(const int64_t* codes, int32_t B, int64_t L_pad, const int64_t* spans, int64_t* out, int64_t out_numel,
                    void* stream) {
    if (!codes || !spans || !out || B < 1 || B > 65535 || L_pad < 1 || out_numel < 0) { set_error("wt_codes_unpack: bad argument"); return WT_ERR_INVALID; }
    if ((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(spans) | reinterpret_cast<uintptr_t>(out)) % 8) {
        set_error("wt_codes_unpack: misaligned pointer"); return WT_ERR_INVALID;
    }
    dim3 grid((unsigned)((L_pad + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(codes_unpack_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), codes, (long)L_pad, spans, out, (long)out_numel);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

int wt_pcm16(const float* x, int64_t n, float limit, int32_t rescale, int16_t* out, void* workspace, void* stream) {
    if (!x || !out || n < 1 || (rescale && !workspace)) { set_error("wt_pcm16: bad argument"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* amax = static_cast<unsigned*>(workspace);
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (rescale) {
        WT_HIP_CHECK(hipMemsetAsync(amax, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(256), 0, s, x, (long)n, amax);
    }
    hipLaunchKernelGGL(pcm16_kernel, dim3(blocks), dim3(256), 0, s, x, (long)n, limit, rescale, amax, out);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

int wt_linear_overlap_add(const float* frames, const float* weight, int32_t n_frames, int64_t rows, int64_t frame_len,
                          int64_t last_len, int64_t stride, float* out, void* stream) {
    if (!frames || !weight || !out || n_frames < 1 || rows < 1 || frame_len < 1 || last_len < 1 || last_len > frame_len ||
        stride < 1 || rows > 65535) {
        set_error("wt_linear_overlap_add: bad argument"); return WT_ERR_INVALID;
    }
    if (stride > frame_len && n_frames > 1) { set_error("wt_linear_overlap_add: stride beyond the frame length leaves uncovered samples"); return WT_ERR_INVALID; }
    const long total = stride * (n_frames - 1) + last_len;
    dim3 grid((unsigned)((total + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(overlap_add_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), frames, weight, n_frames,
                       (long)rows, (long)frame_len, (long)last_len, (long)stride, total, out);
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

size_t wt_overlap_add_ragged_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * sizeof(wt_overlap_add_clip) : 0; }

int wt_overlap_add_ragged(const wt_overlap_add_clip* clips, int32_t B, void* workspace, void* stream) {
    if (!clips || !workspace || B < 1 || B > 65535) { set_error("wt_overlap_add_ragged: bad argument"); return WT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error("wt_overlap_add_ragged: workspace misaligned"); return WT_ERR_INVALID; }
    int64_t max_total = 0;
    for (int b = 0; b < B; ++b) {
        const wt_overlap_add_clip& c = clips[b];
        const std::string who = "wt_overlap_add_ragged: recording " + std::to_string(b) + ": ";
        if (!c.rows) { set_error(who + "null row table"); return WT_ERR_INVALID; }
        if (!c.weight) { set_error(who + "null weight"); return WT_ERR_INVALID; }
        if (!c.out) { set_error(who + "null destination"); return WT_ERR_INVALID; }
        if (c.n_frames < 1) { set_error(who + "n_frames < 1"); return WT_ERR_INVALID; }
        if (c.total < 1) { set_error(who + "total < 1"); return WT_ERR_INVALID; }
        if (c.frame_len < 1) { set_error(who + "frame_len < 1"); return WT_ERR_INVALID; }
        if (c.stride < 1) { set_error(who + "stride < 1"); return WT_ERR_INVALID; }
        if (c.n_frames != (c.total - 1) / c.stride + 1) { set_error(who + "n_frames is not ceil(total / stride)"); return WT_ERR_INVALID; }
        if (c.stride > c.frame_len && c.n_frames > 1) { set_error(who + "stride beyond the frame length leaves uncovered samples"); return WT_ERR_INVALID; }
        // (n_frames - 1 < total / stride: the product cannot overflow)
        if (c.total - c.stride * (c.n_frames - 1) > c.frame_len) { set_error(who + "total beyond the last frame's end"); return WT_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(c.rows) % sizeof(void*) || reinterpret_cast<uintptr_t>(c.weight) % sizeof(float) ||
            reinterpret_cast<uintptr_t>(c.out) % sizeof(float)) {
            set_error(who + "misaligned pointer"); return WT_ERR_INVALID;
        }
        max_total = std::max(max_total, c.total);
    }
    if ((max_total + 255) / 256 > 0x7fffffffLL) { set_error("wt_overlap_add_ragged: recording too long for one launch"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((max_total + 255) / 256), (unsigned)B);
    if (int rc = launch_ragged<OLA_ARG_CLIPS>("wt_overlap_add_ragged", clips, B, 128, workspace, s, [&](auto d) {
        hipLaunchKernelGGL(overlap_add_ragged_kernel<decltype(d)>, grid, dim3(256), 0, s, d);
    })) return rc;
    WT_HIP_CHECK(hipGetLastError());
    return WT_OK;
}

}  // extern "C"
