// The fp32 pieces the frame transforms share (mel.hip: 512 complex points, radix 8; stoi.hip: 256, radix 4): complex values as
// float pairs, the small butterflies, the split pass that turns the transform of z[j] = x[2j] + i x[2j + 1] into the real transform
// of x, the sums over a wave, and the twiddle table.  The Stockham passes stay with their kernels.
//
// A file that uses the arithmetic sets `#pragma clang fp contract(off)` BEFORE this include (mel.hip and stoi.hip do), so that no
// product here depends on the kernel it is inlined into: no contraction by the compiler, fmaf where wanted.  The pragma is not set
// here: it would reach past the include into files that only want global_ptr (audio.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace wt {

// A pointer read from a descriptor in memory is a generic one to the compiler (flat loads and stores); the descriptors of a
// ragged launch hold device pointers by contract, and saying so gives global loads and stores.
template <class T> using global_ptr = __attribute__((address_space(1))) T*;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 cmul(f32x2 a, f32x2 b) {
    return f32x2{fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)};
}
__device__ __forceinline__ void bfly2(f32x2& a, f32x2& b) {
    const f32x2 t = a;
    a = t + b;
    b = t - b;
}
__device__ __forceinline__ f32x2 mul_mi(f32x2 a) { return f32x2{a.y, -a.x}; }     // a * -i
// 4-point DFT in place; output q is left in the rev2(q)-th argument
__device__ __forceinline__ void bfly4(f32x2& a, f32x2& b, f32x2& c, f32x2& d) {
    bfly2(a, c);
    bfly2(b, d);
    d = mul_mi(d);
    bfly2(a, b);
    bfly2(c, d);
}
__device__ __forceinline__ int rev2(int q) { return ((q & 1) << 1) | (q >> 1); }
// 8-point DFT in place; output q is left in v[rev3(q)]
__device__ __forceinline__ void bfly8(f32x2 (&v)[8]) {
    const float h = 0.70710678118654752440f;
    bfly2(v[0], v[4]);
    bfly2(v[1], v[5]);
    bfly2(v[2], v[6]);
    bfly2(v[3], v[7]);
    v[5] = f32x2{(v[5].x + v[5].y) * h, (v[5].y - v[5].x) * h};        // * (1 - i) / sqrt 2
    v[6] = mul_mi(v[6]);
    v[7] = f32x2{(v[7].y - v[7].x) * h, -(v[7].x + v[7].y) * h};       // * (-1 - i) / sqrt 2
    bfly4(v[0], v[1], v[2], v[3]);
    bfly4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ int rev3(int q) { return ((q & 1) << 2) | (q & 2) | (q >> 2); }
// 16-point DFT in place (stftd.hip: 1024 complex points at 16 per lane) as 4 x 4: four 4-point DFTs over v[r0 + 4 r1], the
// products with exp(-2 pi i r0 q1 / 16), four 4-point DFTs over r0; output q is left in v[rev4(q)]
__device__ __forceinline__ int rev4(int q) { return (rev2(q & 3) << 2) | rev2(q >> 2); }
__device__ __forceinline__ void bfly16(f32x2 (&v)[16]) {
    const float h = 0.70710678118654752440f, c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f;
#pragma unroll
    for (int r0 = 0; r0 < 4; ++r0) bfly4(v[r0], v[r0 + 4], v[r0 + 8], v[r0 + 12]);
    // slot 4 rev2(q1) + r0 holds Y[r0][q1]: q1 = 1 in slots 8..11, q1 = 2 in 4..7, q1 = 3 in 12..15
    v[9] = cmul(v[9], f32x2{c1, -s1});                                 // w^1
    v[10] = f32x2{(v[10].x + v[10].y) * h, (v[10].y - v[10].x) * h};   // w^2 = (1 - i) / sqrt 2
    v[11] = cmul(v[11], f32x2{s1, -c1});                               // w^3
    v[5] = f32x2{(v[5].x + v[5].y) * h, (v[5].y - v[5].x) * h};        // w^2
    v[6] = mul_mi(v[6]);                                               // w^4 = -i
    v[7] = f32x2{(v[7].y - v[7].x) * h, -(v[7].x + v[7].y) * h};       // w^6 = (-1 - i) / sqrt 2
    v[13] = cmul(v[13], f32x2{s1, -c1});                               // w^3
    v[14] = f32x2{(v[14].y - v[14].x) * h, -(v[14].x + v[14].y) * h};  // w^6
    v[15] = cmul(v[15], f32x2{-c1, s1});                               // w^9 = -w^1
#pragma unroll
    for (int s = 0; s < 4; ++s) bfly4(v[4 * s], v[4 * s + 1], v[4 * s + 2], v[4 * s + 3]);
}

// Bin k of the real transform X of 2 M points from the M-point transform Z of its even / odd samples:
// X[k] = (Z[k] + conj Z[M - k]) / 2 - i / 2 w (Z[k] - conj Z[M - k]), zk = Z[k], zm = Z[(M - k) mod M], w = exp(-2 pi i k / (2 M))
__device__ __forceinline__ f32x2 real_split_bin(f32x2 zk, f32x2 zm, f32x2 w) {
    const f32x2 e = f32x2{0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
    const f32x2 d = f32x2{zk.x - zm.x, zk.y + zm.y};
    const f32x2 p = cmul(w, d);
    return f32x2{e.x + 0.5f * p.y, e.y - 0.5f * p.x};
}
__device__ __forceinline__ float cpower(f32x2 a) { return fmaf(a.x, a.x, a.y * a.y); }       // |a|^2

// the sum over the wave by the xor butterfly: a fixed order, every lane gets the sum
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}
// the sum over the lane's aligned group of 32
__device__ __forceinline__ float half_sum(float s) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// tw [n][2] = (cos, -sin)(2 pi n / n_points), n < n_points, computed in float64 and rounded once
inline void fill_twiddles(float* tw, int n_points) {
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < n_points; ++n) {
        tw[2 * n] = (float)std::cos(2.0 * pi * n / n_points);
        tw[2 * n + 1] = (float)-std::sin(2.0 * pi * n / n_points);
    }
}

}  // namespace wt
