// Split-f16 GEMM on PRE-SPLIT operands, staged global -> LDS by LDS-DMA (buffer_load ... lds).
//
// Arithmetic: every fp32 operand x is carried as two f16 numbers, x = hi + lo * 2^-11, and a product is formed by three
// f16 MFMAs into a main and a correction fp32 accumulator (hi.hi, then hi.lo + lo.hi scaled by 2^-11): fp32-equivalent
// products.  Both operands arrive already split, in the "S32" layout: every run of 32 consecutive fp32 elements of a row becomes one 128-byte group
//      [32 x f16 hi | 32 x f16 lo]
// so an S32 array has exactly the footprint and the row strides of the fp32 array it stands for, element e of a
// row starts at byte (e & ~31) * 4 + (e & 31) * 2, and one K step (32 deep) of one row is one full 128-byte line.
// Producers write S32 directly (norm kernels, the GELU / head epilogues here, weights once at load), so the K loop
// has no conversion work at all: per step a wave issues a few LDS-DMA loads (8 rows x 128 B each, no VGPRs), 16
// ds_read_b128 and 18 MFMAs.  The conv gather (taps, stride, reflect / zero padding, ragged edges) is the same
// per-(tap, row) byte-offset table as gemm.hip; an out-of-range offset makes the DMA write zeros.
//
// LDS image of a stage: (BM + BN) rows x 128 B; the eight 16-byte chunks of row r are XOR-swizzled with
// (r >> 1) & 7, applied on the SOURCE address of the DMA (its LDS side is lane-linear) and on the ds_read address:
// every ds_read_b128 lane group then covers all 64 banks.
#include "common.h"

#include <cmath>
#include <stdlib.h>
#include <type_traits>

namespace wt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
static constexpr int SBK = 32;          // k elements per step = one 128-byte S32 group per row

__device__ __forceinline__ int xcd_remap_s(int orig, int nwg) {
    int q = nwg >> 3, r = nwg & 7;
    int xcd = orig & 7, idx = orig >> 3;
    int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}
__device__ __forceinline__ float elu_s(float x) { return elu_med3(x); }
// erf to < 1 ulp (max abs error 6.3e-8 against float64 erf over [-6, 6], checked on the host), branch-free: the
// two minimax pieces |a| <= 475/512 (odd polynomial) and beyond (1 - exp(polynomial)) are both evaluated and selected
__device__ __forceinline__ float erf_s(float a) {
    const float t = fabsf(a), s = a * a;
    float r = fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    const float u = fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = fmaf(r, s, u);
    r = fmaf(r, t, -1.06777877e-1f);
    r = fmaf(r, t, -6.34846687e-1f);
    r = fmaf(r, t, -1.28717512e-1f);
    r = fmaf(r, t, -t);
    const float big = copysignf(1.0f - __expf(r), a);
    float q = -5.96761703e-4f;
    q = fmaf(q, s, 4.99119423e-3f);
    q = fmaf(q, s, -2.67681349e-2f);
    q = fmaf(q, s, 1.12819925e-1f);
    q = fmaf(q, s, -3.76125336e-1f);
    q = fmaf(q, s, 1.28379166e-1f);
    const float small = fmaf(q, a, a);
    return t > 0.927734375f ? big : small;
}
__device__ __forceinline__ float gelu_erf_s(float x) { return x * 0.5f * (1.f + erf_s(x * 0.70710678118654752440f)); }
// the same arithmetic on two elements at a time: every polynomial step is one v_pk_fma_f32 / v_pk_mul_f32
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 gelu_erf_s2(f32x2 x) {
    const f32x2 a = x * 0.70710678118654752440f;
    const f32x2 t = __builtin_elementwise_abs(a), s = a * a;
    f32x2 r = fma2((f32x2)(-1.72853470e-5f), t, (f32x2)(3.83197126e-4f));
    const f32x2 u = fma2((f32x2)(-3.88396438e-3f), t, (f32x2)(2.42546219e-2f));
    r = fma2(r, s, u);
    r = fma2(r, t, (f32x2)(-1.06777877e-1f));
    r = fma2(r, t, (f32x2)(-6.34846687e-1f));
    r = fma2(r, t, (f32x2)(-1.28717512e-1f));
    r = fma2(r, t, -t);
    f32x2 q = fma2((f32x2)(-5.96761703e-4f), s, (f32x2)(4.99119423e-3f));
    q = fma2(q, s, (f32x2)(-2.67681349e-2f));
    q = fma2(q, s, (f32x2)(1.12819925e-1f));
    q = fma2(q, s, (f32x2)(-3.76125336e-1f));
    q = fma2(q, s, (f32x2)(1.28379166e-1f));
    const f32x2 small = fma2(q, a, a);
    f32x2 e;
    e.x = t.x > 0.927734375f ? copysignf(1.0f - __expf(r.x), a.x) : small.x;
    e.y = t.y > 0.927734375f ? copysignf(1.0f - __expf(r.y), a.y) : small.y;
    const f32x2 hx = x * 0.5f;
    return fma2(hx, e, hx);
}
__device__ __forceinline__ f32x4 gelu_erf_s4(f32x4 v) {
    const f32x2 lo = gelu_erf_s2((f32x2){v.x, v.y}), hi = gelu_erf_s2((f32x2){v.z, v.w});
    return (f32x4){lo.x, lo.y, hi.x, hi.y};
}

// GELU through erfc on ONE branch: with a = x / sqrt(2), gelu(x) = x * (1 - h) for x >= 0 and x * h for x < 0, where
// h = erfc(|a|) / 2 = 2^p(|a|): p is a degree-9 minimax fit of log2(erfc(t)) - 1 on [0, 4.3] (weighted for the absolute
// error of erfc: 2e-9 in exact arithmetic; |a| is clamped to 4.3, beyond which h < 6e-10).  No second polynomial, no select
// between two formulas, and no cancellation on the negative side (h is formed with relative accuracy, where the
// reference's own fp32 1 + erf(a) carries the rounding of erf near -1): simulated in fp32 against float64 on 2.4 M
// inputs the maximum absolute error is 3.9e-7 (torch's fp32 gelu: 1.2e-6), rms relative 1.0e-7 (2.3e-6).
__device__ __forceinline__ f32x2 gelu_erfc_s2(f32x2 x) {
    const f32x2 a = x * 0.70710678118654752440f;
    f32x2 t = __builtin_elementwise_abs(a);
    t.x = fminf(t.x, 4.3f); t.y = fminf(t.y, 4.3f);
    f32x2 p = fma2((f32x2)(1.146792511e-05f), t, (f32x2)(-1.515573094e-04f));
    p = fma2(p, t, (f32x2)(8.423082181e-04f));
    p = fma2(p, t, (f32x2)(-2.261521295e-03f));
    p = fma2(p, t, (f32x2)(6.768874300e-05f));
    p = fma2(p, t, (f32x2)(2.773740143e-02f));
    p = fma2(p, t, (f32x2)(-1.483134478e-01f));
    p = fma2(p, t, (f32x2)(-9.184416533e-01f));
    p = fma2(p, t, (f32x2)(-1.627907395e+00f));
    p = fma2(p, t, (f32x2)(-1.0f));
    f32x2 h;
    h.x = __builtin_amdgcn_exp2f(p.x);
    h.y = __builtin_amdgcn_exp2f(p.y);
    f32x2 s;
    s.x = a.x >= 0.f ? 1.f - h.x : h.x;
    s.y = a.y >= 0.f ? 1.f - h.y : h.y;
    return x * s;
}
__device__ __forceinline__ f32x4 gelu_erfc_s4(f32x4 v) {
    const f32x2 lo = gelu_erfc_s2((f32x2){v.x, v.y}), hi = gelu_erfc_s2((f32x2){v.z, v.w});
    return (f32x4){lo.x, lo.y, hi.x, hi.y};
}
// The same arithmetic on the four sub-runs of a 32 x 32 block at once, written step by step ACROSS the eight packed pairs:
// a packed fp32 instruction that reads the result of the one in front of it costs a wait state (hipcc pads with s_nop), so
// one Horner chain at a time runs at half rate; eight independent chains need no padding (same results bit for bit)
__device__ __forceinline__ void gelu_erfc_x16(f32x4 (&v)[4]) {
    f32x2 x[8], a[8], t[8], p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = (f32x2){v[i >> 1][2 * (i & 1)], v[i >> 1][2 * (i & 1) + 1]};
        a[i] = x[i] * 0.70710678118654752440f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        t[i] = __builtin_elementwise_abs(a[i]);
        t[i].x = fminf(t[i].x, 4.3f); t[i].y = fminf(t[i].y, 4.3f);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = fma2((f32x2)(1.146792511e-05f), t[i], (f32x2)(-1.515573094e-04f));
    constexpr float c[8] = {8.423082181e-04f, -2.261521295e-03f, 6.768874300e-05f, 2.773740143e-02f, -1.483134478e-01f,
                            -9.184416533e-01f, -1.627907395e+00f, -1.0f};
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = fma2(p[i], t[i], (f32x2)(c[s]));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f32x2 h, sgn;
        h.x = __builtin_amdgcn_exp2f(p[i].x);
        h.y = __builtin_amdgcn_exp2f(p[i].y);
        sgn.x = a[i].x >= 0.f ? 1.f - h.x : h.x;
        sgn.y = a[i].y >= 0.f ? 1.f - h.y : h.y;
        const f32x2 r = x[i] * sgn;
        v[i >> 1][2 * (i & 1)] = r.x;
        v[i >> 1][2 * (i & 1) + 1] = r.y;
    }
}

// sin and cos of one argument for the ISTFT head (heads.py:58-59): three-constant Cody-Waite reduction by pi/2 (exact for the
// |x| < 2^15 it is used for: the first constant has 8 significant bits, every step is one fma) and the classic degree-7 / 8
// minimax polynomials on [-pi/4, pi/4] (about 1 ulp).  libm's sincosf carries a Payne-Hanek path for huge arguments that
// hipcc evaluates branch-free for every lane: 128 64-bit multiply-adds and 450 selects per 16 values in the r02 epilogue.
// Phases beyond 2^15 (never seen; a Linear output) take libm's path.
__device__ __forceinline__ void sincos_head(float x, float& s, float& c) {
    if (__builtin_expect(!(fabsf(x) < 32768.f), 0)) { sincosf(x, &s, &c); return; }
    const float k = rintf(x * 0.63661977236758134308f);
    float r = fmaf(-k, 1.5703125f, x);
    r = fmaf(-k, 4.837512969970703125e-4f, r);
    r = fmaf(-k, 7.54978995489188216e-8f, r);
    const float z = r * r;
    float sp = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    sp = fmaf(sp, z, -1.6666654611e-1f);
    const float sr = fmaf(sp * z, r, r);
    float cp = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    cp = fmaf(cp, z, 4.166664568298827e-2f);
    const float cr = fmaf(cp * z, z, fmaf(z, -0.5f, 1.f));
    const int q = (int)k;
    const float s0 = (q & 1) ? cr : sr, c0 = (q & 1) ? sr : cr;
    s = (q & 2) ? -s0 : s0;
    c = ((q + 1) & 2) ? -c0 : c0;
}
// e^x to about 2 ulp: x = n ln2 + r with a two-constant ln2, 2^n by ldexp (heads.py:55)
__device__ __forceinline__ float exp_head(float x) {
    const float n = rintf(x * 1.44269504088896340736f);
    float r = fmaf(-n, 0.693145751953125f, x);
    r = fmaf(-n, 1.42860682030941723212e-6f, r);
    return ldexpf(__builtin_amdgcn_exp2f(r * 1.44269504088896340736f), (int)n);
}

// fp32 value -> S32 slots of element n (n & 31 = slot) in the group that starts at `grp` (a _Float16*)
__device__ __forceinline__ void store_s32(_Float16* grp, int slot, float v) {
    const _Float16 h = (_Float16)v;
    grp[slot] = h;
    grp[32 + slot] = (_Float16)((v - (float)h) * 2048.f);
}

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
// four consecutive elements n .. n+3 (n % 4 == 0) of a row in S32: 8 bytes of hi halves, 8 bytes of lo halves
__device__ __forceinline__ void store_s32_x4(float* row, int n, const f32x4 v, float& amax) {
    amax = amax4(amax, v.x, v.y, v.z, v.w);
    f16x4 hi, lo;
    split4_f16(v.x, v.y, v.z, v.w, hi, lo);
    _Float16* g = reinterpret_cast<_Float16*>(row) + ((n >> 5) * 64 + (n & 31));
    *reinterpret_cast<f16x4*>(g) = hi;
    *reinterpret_cast<f16x4*>(g + 32) = lo;
}

// 16 bytes of an output tile.  SC1: write-through store that does not keep the line in this XCD's L2 (MI355X_MICROARCH.md,
// "stores of each flavour"): the C tile is never read again by this kernel, and 71 MB of it per launch otherwise push the
// A / W panels, which ARE re-read, out of the 4 MiB L2 (pwconv1: -1.4 us of 93, tools/micro/gemm_lab.hip)
template <bool SC1>
__device__ __forceinline__ void store_c16(float* dst, const f32x4 v) {
    if constexpr (SC1) {
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        const u32x4_t qv = __builtin_bit_cast(u32x4_t, v);
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(dst), "v"(qv) : "memory");
    } else {
        *reinterpret_cast<f32x4*>(dst) = v;
    }
}

template <int N>
__device__ __forceinline__ void wait_vm_lgkm() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// DBG: timing-experiment builds (WT_GEMM16S_DBG, tools/gemm16s_bench.py): a compile-time mask of phases to leave out
// (1 DMA, 2 MFMA, 4 epilogue, 8 barrier, 16 LDS fragment reads, 32 waits, 64 static priority for the younger half, 128
// stores, 256 bias, 512 GELU; 1024: stamp s_memtime / s_memrealtime around the tile loop into GemmArgs::dbg_stamps: the
// clock the chip holds).  The shipped instantiations have DBG = 0.  The mask is a template argument because a run-time
// test in front of every phase (round 1) cuts the K loop and the epilogue into dozens of basic blocks, across which
// hipcc neither overlaps LDS reads with MFMAs nor one 4-column run's GELU with the next one's: 108.7 -> 102.7 us on pwconv1.
#ifndef WT_GEMM16S_MF
#define WT_GEMM16S_MF 1          // MFMA shape of every instantiation (0: 32x32x16, for A/B timing builds; 1: 16x16x32)
#endif
// KS: K tiles per barrier.  1 = the pipeline described at the loop (one barrier in the middle of every K step).  2 = the
// small-problem form (a handful of narrow tiles, one wave per SIMD): two K tiles are made visible by one barrier and their
// fragment reads and MFMAs run back to back - such a launch is a chain of DMA-wait, barrier, LDS-read and MFMA latencies per
// barrier, not of work (tools/step_times.py at B = 1), so half the barriers is most of the time.  Every accumulator still
// sees its K tiles in ascending order: results are bit-identical to KS = 1
// PROD = 1, 2 (with KS = 2): the workgroup carries PROD further sets of WAVES_M x WAVES_N waves that do nothing but the loader's
// work (DMA issue and the wait for it, the pieces shared out among them); the first set does nothing but fragment reads,
// MFMAs and the epilogue.  With one
// wave per SIMD a wave pays for its DMA issue (5 pieces per K tile), its LDS reads and its MFMAs one after the other - at
// B = 1 the sum IS the launch time (ladder in tools/micro/gemm_lab.hip: MFMA 7, LDS reads 4, barriers 3, DMA issue 5, data 8
// of 35 us) - while two waves per SIMD with the roles split run the DMA side under the MFMA side
// G16_HI 1: gemm16h_kernel, the one-product twin (hi halves only: WT_PLAN_FLAG_F16_GEMM).  Its instantiations live in a
// translation unit of their own, gemm16h.hip, which includes this file with WT_GEMM16H_TU set: the kernels, their device
// helpers and the tile choice below are this text, so the twin picks the tile form the default picks for the same problem
#define G16_NAME gemm16s_kernel
#define G16_PARAMS
#define G16_MIX 0
#define G16_HI 0
#include "gemm16s_kernel.inc"
#undef G16_NAME
#undef G16_PARAMS
#undef G16_MIX
#define G16_NAME gemm16s_mixed_kernel
#define G16_PARAMS , const int* __restrict__ mix_geom
#define G16_MIX 1
#include "gemm16s_kernel.inc"
#undef G16_NAME
#undef G16_PARAMS
#undef G16_MIX
#undef G16_HI
#define G16_NAME gemm16h_kernel
#define G16_PARAMS
#define G16_MIX 0
#define G16_HI 1
#include "gemm16s_kernel.inc"
#undef G16_NAME
#undef G16_PARAMS
#undef G16_MIX
#undef G16_HI

#ifndef WT_GEMM16H_TU       // (gemm16h.hip needs the kernels and the tile choice only)
// fp32 -> S32 (flat: rows are multiples of 32 elements, so the layout is a function of the flat index alone)
// `scale` (optional, device): the values are multiplied by scale[0], a power of two chosen by pow2_scale_kernel, first
__global__ __launch_bounds__(256) void split_s32_kernel(const float* __restrict__ x, _Float16* __restrict__ out, long n,
                                                        const float* __restrict__ scale, unsigned* status) {
    const float sc = scale ? scale[0] : 1.f;
    float amax = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = x[i] * sc;
        amax = amax1(amax, v);
        const _Float16 h = (_Float16)v;
        const long g = (i >> 5) * 64 + (i & 31);
        out[g] = h;
        out[g + 32] = (_Float16)((v - (float)h) * 2048.f);
    }
    range_report(status, amax);
}

int launch_split_s32(const float* x, void* out, long n, hipStream_t s, const float* scale_dev) {
    if (n % 32) { set_error("split_s32: element count must be a multiple of 32"); return -1; }
    int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(split_s32_kernel, dim3(blocks), dim3(256), 0, s, x, static_cast<_Float16*>(out), n, scale_dev, g_launch.status);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

// S32 -> fp32 (the lazy fp32 GEMM weights of a model that came from a packed image: weights.cpp ensure_f32_weights)
__global__ __launch_bounds__(256) void unsplit_s32_kernel(const _Float16* __restrict__ in, float* __restrict__ out, long n, float inv_scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long g = (i >> 5) * 64 + (i & 31);
        out[i] = ((float)in[g] + (float)in[g + 32] * (1.f / 2048.f)) * inv_scale;
    }
}
int launch_unsplit_s32(const void* s32, float* out, long n, float inv_scale, hipStream_t s) {
    if (n % 32) { set_error("unsplit_s32: element count must be a multiple of 32"); return -1; }
    int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(unsplit_s32_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const _Float16*>(s32), out, n, inv_scale);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

// Per-tensor power-of-two scale for the single-stage entry points (the plans' producers write S32 directly, with
// the overflow report instead): amax_bits_kernel leaves max |x| (as its bit pattern: positive floats order like
// unsigned integers) in bits[0]; pow2_scale_kernel turns the maxima of two tensors into scale_a, scale_b = powers of two
// that bring each maximum into [1, 2) (1 for an all-zero or non-finite tensor), and out[2] = 1 / (scale_a * scale_b),
// the factor that restores the accumulators.
__global__ __launch_bounds__(256) void amax_bits_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ bits) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(bits, __float_as_uint(m));
}
__global__ void pow2_scale_kernel(const unsigned* __restrict__ bits, float* __restrict__ out) {
    float sc[2];
    for (int i = 0; i < 2; ++i) {
        const unsigned e = (bits[i] >> 23) & 0xffu;             // biased exponent of the maximum
        // 2^(127 - e) brings the maximum into [1, 2); keep the scale itself a normal float, and leave zero / inf / NaN alone
        sc[i] = (e == 0u || e == 255u || e >= 253u) ? 1.f : __uint_as_float((254u - e) << 23);
    }
    out[0] = sc[0];
    out[1] = sc[1];
    out[2] = (1.f / sc[0]) * (1.f / sc[1]);
}
int launch_pow2_scales(const float* a, long na, const float* b, long nb, unsigned* bits2, float* out3, hipStream_t s) {
    WT_HIP_CHECK(hipMemsetAsync(bits2, 0, 2 * sizeof(unsigned), s));
    const int ba = (int)((na + 255) / 256 < 2048 ? (na + 255) / 256 : 2048), bb = (int)((nb + 255) / 256 < 2048 ? (nb + 255) / 256 : 2048);
    hipLaunchKernelGGL(amax_bits_kernel, dim3(ba), dim3(256), 0, s, a, na, bits2);
    hipLaunchKernelGGL(amax_bits_kernel, dim3(bb), dim3(256), 0, s, b, nb, bits2 + 1);
    hipLaunchKernelGGL(pow2_scale_kernel, dim3(1), dim3(1), 0, s, bits2, out3);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

#endif      // WT_GEMM16H_TU

// ---------------------------------------------------------------------------------- host side
// the kernel of a tile form: gemm16s_kernel, with MIX its mixed-length twin, with HI its one-product twin
template <int BM, int BN, int WMs, int WNs, int NSTAGE, int EPI, int OUT, int WPS, int LABDBG, int KS, int PROD, bool MIX, int HI>
static constexpr auto gemm16s_kernel_of() {
    if constexpr (HI) return gemm16h_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>;
    else if constexpr (MIX) return gemm16s_mixed_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>;
    else return gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>;
}

template <int BM, int BN, int WMs, int WNs, int NSTAGE, int EPI, int OUT, int WPS = 2, int LABDBG = 0, int KS = 1, int PROD = 0,
          bool MIX = false, int HI = 0>
static int launch16s_one(const GemmArgs& a, hipStream_t s, const int* mix_geom = nullptr) {
    if (KS == 2 && ((a.K / SBK) % 2 || a.K / SBK < 6)) { set_error("gemm16s: two K tiles per barrier need an even number (>= 6) of K tiles"); return -1; }
    static PerDeviceOnce attr_once;
    constexpr size_t stage_bytes = (size_t)NSTAGE * (BM + BN) * 128;
    size_t smem = stage_bytes + 2ull * a.taps * BM * sizeof(unsigned) + (a.A2 ? 2ull * BM * sizeof(unsigned) : 0);
    constexpr size_t smem_cap = 160 * 1024;
    constexpr size_t smem_want = stage_bytes + 2ull * 32 * BM * sizeof(unsigned) + (size_t)WMs * WNs * 4096 + 8192 + 256;
    constexpr size_t smem_max = smem_want < smem_cap ? smem_want : smem_cap;
    static_assert(stage_bytes + 2 * BM * sizeof(unsigned) <= smem_cap, "LDS budget");
    if (smem > smem_cap) { set_error("gemm16s: too many taps for this tile's LDS budget"); return -1; }
    using kern_t = void (*)(const GemmArgs);
    static_assert(!(MIX && HI), "the one-product twin has no mixed-length form");
    kern_t kern;
    if constexpr (HI) kern = gemm16h_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>;
    else kern = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>;
#ifdef WT_LAB
    // LAB builds only: the timing-experiment builds of the tile the ConvNeXt GEMMs run on (tools/gemm16s_bench.py dbg): the
    // masks of the ablation ladder, each with the clock stamps (+1024), selected by WT_GEMM16S_DBG per launch
    constexpr bool has_dbg = !MIX && !HI && LABDBG == 0 && KS == 1 && BM == 128 && BN == 192 && WMs == 4 && NSTAGE == 3 && ((EPI == EPI_BIAS && OUT == OUT_F32) || (EPI == EPI_BIAS_GELU && OUT == OUT_S32));
    int dbg_req = 0;
    if (const char* e = lab_env("WT_GEMM16S_DBG")) dbg_req = atoi(e);
    kern_t dbg_kerns[8] = {};
    static constexpr int dbg_masks[8] = {1024, 1024 + 4, 1024 + 5, 1024 + 13, 1024 + 45, 1024 + 61, 1024 + 64, 1024 + 21};
    if constexpr (has_dbg) {
        dbg_kerns[0] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024, WT_GEMM16S_MF, WPS>;
        dbg_kerns[1] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 4, WT_GEMM16S_MF, WPS>;
        dbg_kerns[2] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 5, WT_GEMM16S_MF, WPS>;
        dbg_kerns[3] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 13, WT_GEMM16S_MF, WPS>;
        dbg_kerns[4] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 45, WT_GEMM16S_MF, WPS>;
        dbg_kerns[5] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 61, WT_GEMM16S_MF, WPS>;
        dbg_kerns[6] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 64, WT_GEMM16S_MF, WPS>;
        dbg_kerns[7] = gemm16s_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 1024 + 21, WT_GEMM16S_MF, WPS>;
        if (dbg_req) {
            kern = nullptr;
            for (int i = 0; i < 8; ++i) if (dbg_masks[i] == (dbg_req | 1024)) kern = dbg_kerns[i];
            if (!kern) { set_error("gemm16s: no timing-experiment build for this WT_GEMM16S_DBG mask"); return -1; }
        }
    }
#endif
    if (int rc = attr_once.run([&]() -> int {
        WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm16s_kernel_of<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, WPS, LABDBG, KS, PROD, MIX, HI>()),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max));
#ifdef WT_LAB
        for (int i = 0; i < 8; ++i)
            if (dbg_kerns[i]) WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(dbg_kerns[i]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_max));
#endif
        return 0;
    })) return rc;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    const int ntiles = tiles_m * tiles_n;
    // Persistent launch: one workgroup per slot (256 CUs x resident workgroups per CU), each walking tiles
    // b, b + G, ... with its loader streaming across the seams.  The slot count must stay a multiple of 8 so that a
    // workgroup's tiles stay on its XCD, and K must be deep enough for the table hand-over (see the kernel).
    const int per_cu = (WPS >= 2 && WMs * WNs <= 4 && smem * 2 <= smem_cap) ? 2 : 1;
    const int ncu = device_cus();
    int G = (ncu * per_cu / a.nz) & ~7;
    const char* np = lab_env("WT_GEMM16S_NONPERSISTENT");
    if (G < 8 || ntiles <= G || a.K / SBK < NSTAGE + 1 || (np && np[0] == '1')) G = ntiles;
    else {
        // the same number of rounds with the fewest workgroups (720 tiles: 240 x 3 instead of 208 x 3 + 48 x 2): the idle
        // CUs' power goes to the clock of the busy ones
        const bool bal = [] { const char* e = lab_env("WT_GEMM16S_BALANCE"); return !e || e[0] != '0'; }();
        const int rounds = (ntiles + G - 1) / G;
        const int g2 = (((ntiles + rounds - 1) / rounds) + 7) & ~7;
        if (bal && g2 < G) G = g2;
    }
    GemmArgs b = a;
    {   // per-wave bias (+ gamma) cache: WN floats each, filled by DMA at the top of every output tile
        constexpr bool pcache = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_ELU || EPI == EPI_BIAS_RES ||
                                EPI == EPI_BIAS_RES_ELU || EPI == EPI_BIAS_GAMMA_RES || EPI == EPI_HEAD;
        constexpr size_t pc_bytes = (size_t)WMs * WNs * (BN / WNs) * 4 * (EPI == EPI_BIAS_GAMMA_RES ? 2 : 1);
        const size_t off = (smem + 127) / 128 * 128;
        if (pcache && (a.bias || EPI == EPI_BIAS_GAMMA_RES)) {
            if (off + pc_bytes > smem_cap) { set_error("gemm16s: no LDS left for the bias cache"); return -1; }
            if (EPI == EPI_BIAS_GAMMA_RES && !a.gamma) { set_error("gemm16s: this epilogue needs gamma"); return -1; }
            b.pc_off = (int)off;
            smem = off + pc_bytes;
        }
    }
    {   // staged epilogue: 4 KB of scratch per wave after the stages and tables, when it fits and the layout allows
        // (the head pairs two 32-column blocks into one 32-slot S32 group: wave tiles of whole 64-column pairs, N % 64 == 0)
        constexpr bool can_stage = ((OUT == OUT_F32 || OUT == OUT_S32_DUAL_ELU || OUT == OUT_F32_AND_S32) && EPI == EPI_BIAS) ||
                                   (OUT == OUT_S32 && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_ELU)) ||
                                   (OUT == OUT_S32 && EPI == EPI_HEAD && (BN / WNs) % 64 == 0);
        const size_t off = (smem + 127) / 128 * 128;
        const char* ns = lab_env("WT_GEMM16S_NOSTAGE");
        constexpr bool dual = OUT == OUT_S32_DUAL_ELU || OUT == OUT_F32_AND_S32;
        if (can_stage && off + (size_t)WMs * WNs * 4096 <= smem_cap && a.N % (EPI == EPI_HEAD ? 64 : 32) == 0 &&
            !(EPI == EPI_HEAD && (a.head_kb % 32 || a.c_rstride % 32)) && !(ns && ns[0] == '1') &&
            !(dual && ns && ns[0] == '2')) {
            b.stage_epi = 1; b.stage_off = (int)off;
            smem = off + (size_t)WMs * WNs * 4096;
        }
    }
    if (!b.status) b.status = g_launch.status;
    if (g_launch.stamp_start && g_launch.stamp_end) {
        b.stamp_start = g_launch.stamp_start; b.stamp_end = g_launch.stamp_end;
        g_launch.stamp_used = true;
    }
    if (a.form) *a.form = LaunchForm{BM, BN, WMs, WNs, NSTAGE, KS, PROD, b.stage_epi, b.pc_off ? 1 : 0, G, ntiles, a.group_m, a.group_n};
    if constexpr (MIX)
        hipLaunchKernelGGL((gemm16s_mixed_kernel<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, LABDBG, WT_GEMM16S_MF, WPS, KS, PROD>),
                           dim3(G, 1, a.nz), dim3(64 * WMs * WNs * (1 + PROD)), smem, s, b, mix_geom);
    else
        hipLaunchKernelGGL(kern, dim3(G, 1, a.nz), dim3(64 * WMs * WNs * (1 + PROD)), smem, s, b);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

#ifndef WT_GEMM16S_LAB      // tools/micro/gemm_lab.hip includes this file and instantiates the variants it compares itself
static int tile16s_override() {
    const char* e = lab_env("WT_GEMM16S_TILE");      // LAB builds: read per launch, tools/gemm16s_bench.py switches it in-process
    return e ? atoi(e) : -1;
}

// a tile form of launch16s_tiled: the default kernel, or with HI the one-product twin of the same form
template <int HI, int BM, int BN, int WMs, int WNs, int NSTAGE, int EPI, int OUT, int KS = 1, int PROD = 0>
static int launch16s_form(const GemmArgs& a, hipStream_t s) {
    return launch16s_one<BM, BN, WMs, WNs, NSTAGE, EPI, OUT, 2, 0, KS, PROD, false, HI>(a, s);
}

template <int EPI, int OUT, int HI = 0>
static int launch16s_tiled(const GemmArgs& a, hipStream_t s) {
    if constexpr (EPI == EPI_HEAD) {
        // wave tile 32 x 64: one whole 32-slot group per row block, staged full-line stores.  (7680 x 2432: 1140 tiles in 5
        // rounds of 232; 128 x 192 tiles need 4 rounds of 1.5 x the work each: 134 vs 127 us, tools/micro/gemm_lab.hip)
        {   // a few clips: the small-problem form (below); its 32-column wave tile holds whole (log-mag, phase) pairs of 16 slots
            const bool ks2_env = [] { const char* e = lab_env("WT_GEMM16S_KS"); return !e || e[0] != '1'; }();
            const int nkt = a.K / SBK;
            if (ks2_env && nkt % 2 == 0 && nkt >= 6 && ((a.M + 63) / 64) * ((a.N + 31) / 32) * a.nz <= device_cus())
                return launch16s_form<HI, 64, 32, 2, 1, 6, EPI, OUT, 2, 2>(a, s);
        }
        return launch16s_form<HI, 128, 128, 4, 2, 3, EPI, OUT>(a, s);
    } else if constexpr (EPI == EPI_ARGMAX) {
        return launch16s_form<HI, 128, 192, 4, 2, 3, EPI, OUT>(a, s);      // gemm16s_vq_parts() assumes this tile
    } else {
        switch (tile16s_override()) {       // experiment hook (tools/linear_bench.py)
            case 2: return launch16s_form<HI, 128, 192, 4, 2, 3, EPI, OUT>(a, s);
            case 3: return launch16s_form<HI, 128, 128, 4, 2, 3, EPI, OUT>(a, s);
            case 8: return launch16s_form<HI, 128, 32, 4, 1, 3, EPI, OUT>(a, s);
            case 9: return launch16s_form<HI, 128, 64, 4, 1, 3, EPI, OUT>(a, s);
            default: break;
        }
        if (a.N <= 64) {      // narrow outputs (down conv 1)
            // the 256-row tile's two [taps][256] offset tables fit beside its stages and bias cache up to 19 taps; a stage-1 down
            // conv of more (a first encoder ratio of 10 .. 16 off the fused kernel) takes the 128-row tile, which holds 32
            const size_t need = 3ull * (256 + 64) * 128 + 2ull * a.taps * 256 * sizeof(unsigned) + (a.A2 ? 2ull * 256 * sizeof(unsigned) : 0) +
                                2048;      // (launch16s_one's smem and pc_bytes of this form)
            if (need <= 160 * 1024) return launch16s_form<HI, 256, 64, 8, 1, 3, EPI, OUT>(a, s);
            return launch16s_form<HI, 128, 64, 4, 1, 3, EPI, OUT>(a, s);
        }
        // a handful of clips (M of a few hundred rows): with 128-column tiles fewer than 32 CUs would each walk the whole
        // K loop alone, so the problem is cut into 32-column tiles instead (4x the workgroups, a third of the work per
        // K step).  Every tile shape accumulates K in the same order: results do not depend on the choice
        const long t128 = ((a.M + 127) / 128) * ((a.N + 127) / 128) * a.nz;
        // ... and two K tiles per barrier where K allows (KS = 2: these launches are latency chains, see the kernel)
        const bool ks2_env = [] { const char* e = lab_env("WT_GEMM16S_KS"); return !e || e[0] != '1'; }();
        const int nkt = a.K / SBK;
        const bool ks2 = ks2_env && nkt % 2 == 0 && nkt >= 6;
        // (with it a 128 x 32 tile walks K faster than a 128 x 64 tile does: it is used as long as all of its tiles run at once)
        // ... and loader waves beside the MFMA waves (PROD).  Same-process ladder on pwconv2 at B = 1 (tools/micro/gemm_lab.hip):
        // 128x32 one tile per barrier 35.6 us, two per barrier 32.2, + 4 loader waves 28-30; 64x32 + 2 loader waves 25, + 4: 23.7
        const long cols32 = ((a.N + 31) / 32) * a.nz;
        const long t32 = ((a.M + 127) / 128) * cols32, t64 = ((a.M + 63) / 64) * cols32;
        const int ncu = device_cus();
        if (ks2 && t64 <= ncu) return launch16s_form<HI, 64, 32, 2, 1, 6, EPI, OUT, 2, 2>(a, s);
        if (ks2 && t32 <= ncu && a.nz == 1) return launch16s_form<HI, 128, 32, 4, 1, 6, EPI, OUT, 2, 1>(a, s);     // (batched per-clip
                                                    // problems - the attention scores at B = 64 - are better off on 128x64: 21 vs 25 us)
        if (t128 <= 32) return launch16s_form<HI, 128, 32, 4, 1, 3, EPI, OUT>(a, s);
        if (t128 <= 100) {     // up to ~16 clips: 2x the workgroups; with loader waves where six stages fit beside the offset tables
            if (ks2 && a.nz == 1 && a.taps <= 7 && !a.A2) return launch16s_form<HI, 128, 64, 4, 1, 6, EPI, OUT, 2, 1>(a, s);
            return launch16s_form<HI, 128, 64, 4, 1, 3, EPI, OUT>(a, s);
        }
        // one 8-wave workgroup per CU (256 slots): 128x192 unless its last round would be mostly idle
        const long tm = (a.M + 127) / 128;
        auto cost = [&](int bn, double eff) {
            const long t = tm * ((a.N + bn - 1) / bn) * a.nz;
            return std::ceil((double)t / (double)ncu) * bn / eff;
        };
        if (cost(128, 0.82) < cost(192, 1.0)) return launch16s_form<HI, 128, 128, 4, 2, 3, EPI, OUT>(a, s);
        return launch16s_form<HI, 128, 192, 4, 2, 3, EPI, OUT>(a, s);
    }
}

// The (epilogue, output format) pairs of the one-product twin: what build_decode and plan_head run on S32 operands (no argmax, no
// encoder-only pair, no mixed-length form)
#define WT_GEMM16H_PAIRS(X) \
    X(EPI_BIAS, OUT_F32) X(EPI_BIAS_RES, OUT_F32) X(EPI_BIAS, OUT_S32) X(EPI_BIAS_ROW, OUT_S32) X(EPI_SCALE, OUT_F32) \
    X(EPI_BIAS_GELU, OUT_S32) X(EPI_BIAS_GAMMA_RES, OUT_F32) X(EPI_HEAD, OUT_S32)

#ifndef WT_GEMM16H_TU
int gemm16s_vq_parts(int N) { return ((N + 191) / 192) * 2; }      // (column tiles of 192) x (2 wave columns)

// Mixed-length plans (launch_gemm16s's mix_geom): the encoder's convs on three tile forms.  Every form accumulates K in the same order,
// so a clip's rows are the bits its own plan computes whatever form either launch picks
template <int EPI, int OUT>
static int launch16s_mixed(const GemmArgs& a, hipStream_t s, const int* mix_geom) {
    if (a.N <= 64) return launch16s_one<256, 64, 8, 1, 3, EPI, OUT, 2, 0, 1, 0, true>(a, s, mix_geom);
    const long t128 = ((a.M + 127) / 128) * ((a.N + 127) / 128);
    if (t128 <= 100) return launch16s_one<128, 64, 4, 1, 3, EPI, OUT, 2, 0, 1, 0, true>(a, s, mix_geom);
    return launch16s_one<128, 128, 4, 2, 3, EPI, OUT, 2, 0, 1, 0, true>(a, s, mix_geom);
}
// the (epilogue, output format) pairs of the encoder's S32 convs: down convs, resblock k3 convs, shortcut + conv1, final conv
#define WT_GEMM16S_MIXED_PAIRS(X) X(EPI_BIAS, OUT_S32_DUAL_ELU) X(EPI_BIAS, OUT_F32_AND_S32) X(EPI_BIAS_ELU, OUT_S32)

// The (epilogue, output format) pairs the plans use: the one list both the checks and the dispatch read
#define WT_GEMM16S_PAIRS(X) \
    X(EPI_BIAS, OUT_F32) X(EPI_BIAS, OUT_S32) X(EPI_BIAS, OUT_S32_DUAL_ELU) X(EPI_BIAS, OUT_F32_AND_S32) \
    X(EPI_BIAS_RES, OUT_F32) X(EPI_BIAS_ELU, OUT_S32) X(EPI_BIAS_RES_ELU, OUT_S32) X(EPI_BIAS_GELU, OUT_S32) \
    X(EPI_BIAS_GAMMA_RES, OUT_F32) X(EPI_HEAD, OUT_S32) X(EPI_ARGMAX, OUT_F32) X(EPI_SCALE, OUT_F32) X(EPI_BIAS_ROW, OUT_S32)

// Contract: a.A = S32 activations (same strides as the fp32 array),
// a.W_hi = S32 weights [N][K]; out_s32 selects an S32 C (c_rstride in fp32 elements either way).
// prec: GEMM16S_F16X3 (three products, the default) or GEMM16S_F16 (the one-product twin, gemm16h.hip)
int check_gemm16s(const GemmArgs& c, int epi, int out, const int* mix_geom, int prec) {
    bool known = false;
    if (prec == GEMM16S_F16) {
#define WT_PAIR16S(E, O) known = known || (epi == E && out == O);
        WT_GEMM16H_PAIRS(WT_PAIR16S)
#undef WT_PAIR16S
        known = known && !mix_geom;
    } else if (prec == GEMM16S_F16X3) {
#define WT_PAIR16S(E, O) known = known || (epi == E && out == O);
    WT_GEMM16S_PAIRS(WT_PAIR16S)
#undef WT_PAIR16S
    }
    if (!known) { set_error("gemm16s: unsupported epilogue / output-format pair"); return -1; }
    if (mix_geom) {
        bool mixed = false;
#define WT_PAIR16S(E, O) mixed = mixed || (epi == E && out == O);
        WT_GEMM16S_MIXED_PAIRS(WT_PAIR16S)
#undef WT_PAIR16S
        if (!mixed || c.pad_mode != PAD_REFLECT || c.nz != 1) {
            set_error("gemm16s: mixed-length launches exist for the encoder's reflect-padded convs only"); return -1;
        }
    }
    const bool out_s32 = out != OUT_F32;        // some S32 array is written: whole 32-column groups
    if (c.M <= 0 || c.N <= 0 || c.K <= 0 || c.K % SBK || c.Cin % SBK || c.K != c.taps * c.Cin || c.T_out <= 0 ||
        c.M % c.T_out || c.taps > 32 || !c.W_hi || !c.A || (c.w_rstride % 32) || (c.zW % 32) || (c.a_rstride % 32) ||
        (c.a_bstride % 32) || (c.zA % 32) || ((c.N % 4) && !((epi == EPI_SCALE || epi == EPI_BIAS_ROW) && c.c_rstride >= ((c.N + 3) & ~3))) || (c.c_rstride % 4) || (c.zC % 4) || (c.r_rstride % 4) || (out_s32 && ((c.c_rstride % 32) || (c.zC % 32)))) {
        set_error("gemm16s: unsupported problem (S32 operands need every extent and stride in multiples of 32)");
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(c.A) & 127) || (reinterpret_cast<uintptr_t>(c.W_hi) & 127)) {
        set_error("gemm16s: S32 operands must be 128-byte aligned"); return -1;
    }
    {
        const long clips_per_tile = 256 / c.T_out + 2;      // BM <= 256
        if ((clips_per_tile * c.a_bstride + (long)c.T_in * c.a_rstride) * 4 >= 0x40000000L ||
            (long)c.N * c.w_rstride * 4 >= 0x40000000L) {
            set_error("gemm16s: operand window exceeds the 1 GiB buffer-offset range"); return -1;
        }
    }
    if (c.pad_mode == PAD_REFLECT && c.Tp < c.T_in) { set_error("gemm16s: reflect Tp < T_in"); return -1; }
    if (c.A2) {
        const long clips_per_tile = 256 / c.T_out + 2;
        if (c.taps != 1 || c.stride != 1 || c.pad_left != 0 || c.nz != 1 || c.T_in != c.T_out || c.K1 <= 0 || c.K1 >= c.K || (c.K1 % SBK) ||
            (c.a2_rstride % 32) || (c.a2_bstride % 32) || (reinterpret_cast<uintptr_t>(c.A2) & 127) ||
            (clips_per_tile * c.a2_bstride + (long)c.T_in * c.a2_rstride) * 4 >= 0x40000000L) {
            set_error("gemm16s: a second K source needs a plain row-major problem (taps 1, stride 1, no padding) and K1 in multiples of 32");
            return -1;
        }
    }
    if ((out == OUT_S32_DUAL_ELU || out == OUT_F32_AND_S32) && !c.C2) { set_error("gemm16s: this output format needs C2"); return -1; }
    if (epi == EPI_HEAD && (!c.bias || c.N % 32 || c.head_kb <= 0)) { set_error("gemm16s: head epilogue needs a bias, N % 32 == 0 and head_kb"); return -1; }
    if ((!c.C && epi != EPI_ARGMAX) || ((epi == EPI_BIAS_RES || epi == EPI_BIAS_RES_ELU || epi == EPI_BIAS_GAMMA_RES) && !c.R) ||
        (epi == EPI_BIAS_GAMMA_RES && !c.gamma) || (epi == EPI_BIAS_ROW && !c.bias)) {
        set_error("gemm16s: this epilogue needs C and its R / gamma / bias operands"); return -1;
    }
    if (epi == EPI_ARGMAX && (!c.vq_xx || !c.vq_ee || !c.vq_pval || !c.vq_pidx || c.vq_nparts != gemm16s_vq_parts(c.N))) {
        set_error("gemm16s: argmax epilogue needs xx, ee and (value, index) slots for gemm16s_vq_parts(N) parts"); return -1;
    }
    return 0;
}

int launch_gemm16s(const GemmArgs& a_in, int epi, int out, hipStream_t s, const int* mix_geom, int prec) {
    if (int rc = check_gemm16s(a_in, epi, out, mix_geom, prec)) return rc;
    GemmArgs a = a_in;
    // Tile order.  An XCD runs 30 tiles at a time (240 persistent workgroups / 8); a round pulls the A panels of its row tiles
    // and the W panels of its column tiles through that XCD's L2 once.  Wide outputs (ConvNeXt pwconv1: 60 x 12 tiles) walk
    // blocks of 5 row x 6 column tiles = one XCD round each: 132 MB read per launch instead of 156 with groups of 8 row
    // tiles over all 12 columns, at the same launch time (profiles/r03_gmn_traffic.txt; DESIGN section 3 has the 127 MB floor)
    const int tiles_n192 = (a.N + 191) / 192;
    a.group_m = tiles_n192 > 8 ? 8 : 1;
    if (tiles_n192 >= 12 && tiles_n192 % 6 == 0 && a.nz == 1) { a.group_m = 5; a.group_n = 6; }
    if (const char* e = lab_env("WT_GEMM16S_GM")) { a.group_m = atoi(e) > 0 ? atoi(e) : a.group_m; a.group_n = 0; }      // sweeps (tools/gemm16s_bench.py)
    if (const char* e = lab_env("WT_GEMM16S_GN")) a.group_n = atoi(e);
    if (prec == GEMM16S_F16) return launch_gemm16h_tiled(a, epi, out, s);      // (same tile order, same tile choice: gemm16h.hip)
    if (mix_geom) {
#define WT_CASE16S(E, O) if (epi == E && out == O) return launch16s_mixed<E, O>(a, s, mix_geom);
        WT_GEMM16S_MIXED_PAIRS(WT_CASE16S)
#undef WT_CASE16S
    }
#define WT_CASE16S(E, O) if (epi == E && out == O) return launch16s_tiled<E, O>(a, s);
    WT_GEMM16S_PAIRS(WT_CASE16S)
#undef WT_CASE16S
    set_error("gemm16s: unsupported epilogue / output-format pair");
    return -1;
}
#endif      // WT_GEMM16H_TU
#endif      // WT_GEMM16S_LAB

}  // namespace wt
