// Fused SEANetResnetBlock (encoder/modules/seanet.py:21-63) on the f16 matrix pipe with fp32-equivalent products.
//
//   y = shortcut(x) + conv1(elu(conv3(elu(x))))
//
// Same fusion as resblock.hip (x tile with its k=3 halo in LDS, conv1 frame-local, weights resident in LDS, persistent
// workgroups), but every contraction runs as split-f16 (x = hi + lo * 2^-11, three f16 MFMAs per K step, main + correction
// accumulator: gemm16s.hip) instead of v_mfma_f32_32x32x2_f32.  The split is done ONCE per element when the tile is filled
// (ELU too, not once per tap), the LDS images hold rows of [hi | lo] f16 with XOR-swizzled 16-byte chunks so every
// ds_read_b128 fragment read is conflict-free, and the weights are the MFMA's A operand: the accumulator comes out with the
// frame on the lane and 4-channel runs in the registers, so the epilogue stores 16 bytes (fp32) or 8 + 8 bytes (S32) per lane.
// Three forms (template arguments below):
//   C = 32, FOLD: the first encoder conv (k7, 1 -> 32) is the tile fill, itself an MFMA pass over the waveform;
//   C = 32, FOLD, DOWN = r: ... and ELU + the stage's strided conv run on the tile while it is in LDS: encoder stage 1 in one
//       kernel (the shipped plan; wt_resblock_down);
//   C = 64, FPW = 16: the plain block on 8 waves of 16 frames (encoder stage 2, SEANetDecoder).
#include "common.h"

#include <stdlib.h>

namespace wt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rb16_elu(float x) { return elu_med3(x); }

__device__ __forceinline__ void rb16_split8(const float* v, f16x8& hi, f16x8& lo, float& amax) {
    amax = amax4(amax4(amax, v[0], v[1], v[2], v[3]), v[4], v[5], v[6], v[7]);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned a, b; split2_f16(v[2 * i], v[2 * i + 1], a, b); h[i] = a; l[i] = b; }
    hi = __builtin_bit_cast(f16x8, h);
    lo = __builtin_bit_cast(f16x8, l);
}
__device__ __forceinline__ void rb16_split4(const f32x4 v, f16x4& hi, f16x4& lo, float& amax) {
    amax = amax4(amax, v[0], v[1], v[2], v[3]);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 h, l;
#pragma unroll
    for (int i = 0; i < 2; ++i) { unsigned a, b; split2_f16(v[2 * i], v[2 * i + 1], a, b); h[i] = a; l[i] = b; }
    hi = __builtin_bit_cast(f16x4, h);
    lo = __builtin_bit_cast(f16x4, l);
}

// LDS images (bytes).  An activation row of CH channels is CH*4 bytes: per 32 channels a 128-byte group
// [32 x hi | 32 x lo] (CH = 16: one 64-byte group [16 hi | 16 lo]); the 16-byte chunk c of row r is stored at chunk
// c ^ swz(r) with swz chosen per row pitch so that 16 lanes reading the same logical chunk of 16 different rows
// cover all 64 banks:  64-byte rows: (r >> 2) & 3, 128-byte rows: (r >> 1) & 7, 256-byte rows: r & 15.
template <int CH>
struct RbRow {
    static constexpr int bytes = CH * 4;
    static constexpr int chunks = bytes / 16;
    __device__ static __forceinline__ int swz(int r) {
        // 256-byte rows (C = 64): a 4-bit XOR-linear function of r & 7, (r0, r0^r1, r2, r1^r2), found by search with the bank
        // model of tools/lds_banks.py: conflict-free for 16 consecutive rows starting at ANY row (conv3's taps start at
        // offsets 0, 1, 2; round 2's r & 15 was 1.33 LDS cycles per ideal one there) and for the 8-lanes-per-row stores
        return bytes == 64 ? ((r >> 2) & 3) : (bytes == 128 ? ((r >> 1) & 7) : (int)((0x56FC9A30u >> (4 * (r & 7))) & 15u));
    }
    // byte offset of the 8-half chunk holding channels ci .. ci+7 (ci % 8 == 0) of row r; lo = the lo half
    __device__ static __forceinline__ int off(int r, int ci, int lo) {
        constexpr int G = CH < 32 ? CH : 32;                    // channels per [hi | lo] group
        const int c = (ci / G) * (G / 4) + lo * (G / 8) + (ci % G) / 8;
        return r * bytes + ((c ^ swz(r)) * 16);
    }
};

template <int C, int ROWS>
struct Rb16Layout {
    static constexpr int H = C / 2;
    static constexpr int N1 = H < 16 ? 16 : H;       // conv3 output rows: 16 (one 16x16x32 tile) or a multiple of 32
    static constexpr int K1 = 3 * C, K2 = H + C;
    static constexpr int NX = ROWS + 2;
    static constexpr int off_xe = 0;                                 // elu(x), rows -1 .. ROWS
    static constexpr int off_xr = off_xe + NX * C * 4;               // raw x, rows 0 .. ROWS-1 (FOLD: no raw copy exists - the shortcut goes
                                                                     // through the first conv - and the rows only stage elu(y))
    static constexpr int off_he = off_xr + ROWS * C * 4;             // elu(hidden)
    static constexpr int off_w3 = off_he + ROWS * H * 4;             // [K1/16][hi, lo][N1 rows][32 B]
    static constexpr int off_w2 = off_w3 + (K1 / 16) * 2 * N1 * 32;  // [K2/16][hi, lo][C rows][32 B]
    static constexpr int off_b = off_w2 + (K2 / 16) * 2 * C * 32;    // b3[N1], b12[C] fp32
    static constexpr int off_wav = off_b + (N1 + C) * 4;             // folded first conv: ROWS + 8 samples
    static constexpr int total = off_wav + 2 * (ROWS + 8) * 4;       // two windows: the next tile's is written before the barrier that ends this one
};

// weight image: 16-deep k-step ks, part hl, row n: 32 bytes = k 16 ks .. +15 as two 16-byte chunks (k half h),
// stored at chunk h ^ ((n >> 3) & 1): conflict-free for the 16-lane groups of a ds_read_b128
// sw: the image is read as v_mfma_f32_32x32x16_f16 operands (lane = (row of 32, k half)); images read as 16x16x32 operands
// (lane = (row of 16, k quarter)) take no swizzle: there the 16-lane groups of a ds_read_b128 pair rows n and n + 8 with
// OPPOSITE halves already, and the swizzle would put them on the same banks
__device__ __forceinline__ int rb16_woff(int rows, int ks, int hl, int n, int h, bool sw = true) {
    return ((ks * 2 + hl) * rows + n) * 32 + ((h ^ (sw ? ((n >> 3) & 1) : 0)) * 16);
}

// DBG: timing-experiment build (WT_RB16_DBG); the shipped instantiations test nothing at run time.
// DOWN = r > 0 (C = 32 with the folded first conv only): the stage's down conv — ELU, SConv1d(32 -> 64, k = 2r, stride r,
// reflect; seanet.py:123-127) — is computed from the tile's output while it is still in LDS, and only ITS output
// (64 channels at 1/r of the frame rate) goes to HBM: the 590 MB of stage-1 activations are neither written nor read back.
// A tile is the 126-frame window [i*OPT*r - r/2, + 126) that OPT = (126 - 2r)/r + 1 consecutive output frames need
// (30 for r = 4, 62 for r = 2: consecutive windows overlap, 5 % recomputed; the last window of a clip is shifted to end at the
// clip, so lengths that are no multiple of r work too); wave w owns output channels
// [16 w, 16 w + 16) with its 2r x 32 weights resident in registers as v_mfma_f32_16x16x32_f16 operands.
// FPW = frames per wave: 32 (one v_mfma_f32_32x32x16_f16 column block per wave, 4 waves) or 16 (C = 64: 8 waves, everything on
// v_mfma_f32_16x16x32_f16).  The 64-channel tile + weights take 130 KB of LDS, i.e. one workgroup per CU: with 4 waves that is ONE
// wave per SIMD and nothing overlaps its fill, MFMA and store phases; 8 waves of 16 frames give every SIMD a second wave.
#define RB16_NAME resblock16_kernel
#define RB16_PARAMS
#define RB16_MIX 0
#include "resblock16_kernel.inc"
#undef RB16_NAME
#undef RB16_PARAMS
#undef RB16_MIX
#define RB16_NAME resblock16_mixed_kernel
#define RB16_PARAMS , const ResblockMix mx
#define RB16_MIX 1
#include "resblock16_kernel.inc"
#undef RB16_NAME
#undef RB16_PARAMS
#undef RB16_MIX

// MIX: the mixed-length twin (resblock16_mixed_kernel, lengths from mix)
template <int C, int ROWS, int FOLD, int FPW = 32, bool MIX = false>
static int launch_rb16(const ResblockArgs& a, hipStream_t s, const ResblockMix* mix = nullptr) {
    static PerDeviceOnce attr_once;
    constexpr size_t smem = (size_t)Rb16Layout<C, ROWS>::total;
    static_assert(smem <= 160 * 1024, "LDS budget");
    auto kern = resblock16_kernel<C, ROWS, FOLD, false, 0, FPW>;
    int dbg_req = 0;
#ifdef WT_LAB       // the phase-ablation instantiations (tools/rb16_bench.py, WT_RB16_DBG) exist in LAB builds only
    if (const char* e = lab_env("WT_RB16_DBG")) dbg_req = atoi(e);
    if (dbg_req) kern = resblock16_kernel<C, ROWS, FOLD, true, 0, FPW>;
#endif
    if (int rc = attr_once.run([&]() -> int {
        if constexpr (MIX)
            WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_mixed_kernel<C, ROWS, FOLD, false, 0, FPW>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        else
            WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_kernel<C, ROWS, FOLD, false, 0, FPW>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
#ifdef WT_LAB
        if (!MIX) WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_kernel<C, ROWS, FOLD, true, 0, FPW>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
#endif
        return 0;
    })) return rc;
    constexpr int VALID = FOLD ? ROWS - 2 : ROWS;
    const long tiles = (long)a.B * ((a.T + VALID - 1) / VALID);
    const int per_cu = (int)(160 * 1024 / smem) < 4 ? (int)(160 * 1024 / smem) : 4;
    const long slots = (long)device_cus() * per_cu;
    const long grid = tiles < slots ? tiles : slots;
    ResblockArgs b = a;
    b.dbg = dbg_req;
    if (!b.status) b.status = g_launch.status;
    if (RbForm* f = g_launch.rb_form) *f = RbForm{MIX ? 1 : 0, C, FOLD, 0, FPW, (unsigned)grid, (unsigned)(ROWS / FPW * 64), (unsigned)smem, tiles};
    if constexpr (MIX)
        hipLaunchKernelGGL((resblock16_mixed_kernel<C, ROWS, FOLD, false, 0, FPW>), dim3((unsigned)grid), dim3(ROWS / FPW * 64), smem, s, b, *mix);
    else
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(ROWS / FPW * 64), smem, s, b);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

// stage 1 with the down conv fused in: wav [B][T] -> y_down [B][ceil(T / r)][64] fp32 (r = a.R = 2 or 4)
template <int R, bool MIX = false>
static int launch_rb16_down(const ResblockArgs& a, hipStream_t s, const ResblockMix* mix = nullptr) {
    static PerDeviceOnce attr_once;
    constexpr size_t smem = (size_t)Rb16Layout<32, 128>::total;
    constexpr int OPT = (126 - 2 * R) / R + 1;
    auto kern = resblock16_kernel<32, 128, 1, false, R>;
    int dbg_req = 0;
#ifdef WT_LAB
    if (const char* e = lab_env("WT_RB16_DBG")) dbg_req = atoi(e);
    if (dbg_req) kern = resblock16_kernel<32, 128, 1, true, R>;
#endif
    if (int rc = attr_once.run([&]() -> int {
        if constexpr (MIX)
            WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_mixed_kernel<32, 128, 1, false, R>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        else
            WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_kernel<32, 128, 1, false, R>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
#ifdef WT_LAB
        if (!MIX) WT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(resblock16_kernel<32, 128, 1, true, R>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
#endif
        return 0;
    })) return rc;
    const long tiles = (long)a.B * (((a.T + R - 1) / R + OPT - 1) / OPT);
    const int per_cu = (int)(160 * 1024 / smem) < 4 ? (int)(160 * 1024 / smem) : 4;
    const long slots = (long)device_cus() * per_cu;
    const long grid = tiles < slots ? tiles : slots;
    ResblockArgs b = a;
    b.dbg = dbg_req;
    if (!b.status) b.status = g_launch.status;
    if (RbForm* f = g_launch.rb_form) *f = RbForm{MIX ? 1 : 0, 32, 1, R, 32, (unsigned)grid, 256u, (unsigned)smem, tiles};
    if constexpr (MIX)
        hipLaunchKernelGGL((resblock16_mixed_kernel<32, 128, 1, false, R>), dim3((unsigned)grid), dim3(256), smem, s, b, *mix);
    else
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), smem, s, b);
    WT_HIP_CHECK(hipGetLastError());
    return 0;
}

bool resblock16_down_fusable(int C, long T, int r, int k) { return C == 32 && (r == 2 || r == 4) && k == 2 * r && T >= 1024; }

int launch_resblock16_down(const ResblockArgs& a, hipStream_t s, const ResblockMix* mix) {
    if (!a.wav || !a.Wd || !a.bd || !a.y_down || !resblock16_down_fusable(a.C, a.T, a.R, 2 * a.R)) {
        set_error("resblock16_down: needs the waveform, C = 32, stride 2 or 4 with k = 2 * stride, T >= 1024"); return -1;
    }
    if (mix) {       // mixed-length plans: per-clip lengths from the geometry table (every one >= 1024)
        if (!mix->T || !mix->Tread) { set_error("resblock16_down: a mixed-length launch needs both length words"); return -1; }
        return a.R == 4 ? launch_rb16_down<4, true>(a, s, mix) : launch_rb16_down<2, true>(a, s, mix);
    }
    return a.R == 4 ? launch_rb16_down<4>(a, s) : launch_rb16_down<2>(a, s);
}

int launch_resblock16(const ResblockArgs& a, hipStream_t s, const ResblockMix* mix) {
    if (a.wav && a.C != 32) { set_error("resblock16: the folded first conv needs C == 32"); return -1; }
    if (!a.wav && ((reinterpret_cast<uintptr_t>(a.x) & 15) || (a.x_bstride % 4))) {
        set_error("resblock16: x must be 16-byte aligned"); return -1;
    }
    if (mix) {       // mixed-length plans: the encoder's 64-channel stage only
        if (!mix->T || !mix->Tread || a.C != 64 || a.wav) { set_error("resblock16: mixed-length launches exist for the plain C = 64 block only"); return -1; }
        return launch_rb16<64, 128, 0, 16, true>(a, s, mix);
    }
    if (a.C == 32) return a.wav ? launch_rb16<32, 128, 1>(a, s) : launch_rb16<32, 128, 0>(a, s);
    if (a.C == 64) {
        // A/B timing: WT_RB16_FPW=32 is the 4-wave form.  (Tried: 48-row tiles of 3 waves, 75 KB, i.e. two independent
        // workgroups per CU: 252 us against 223 for the 8-wave form and 268 for the 4-wave form, kernel alone, one box.)
#ifdef WT_LAB
        if (const char* e = lab_env("WT_RB16_FPW")) if (atoi(e) == 32) return launch_rb16<64, 128, 0, 32>(a, s);
#endif
        return launch_rb16<64, 128, 0, 16>(a, s);
    }
    set_error("resblock16: fused kernel exists for C = 32 and 64");
    return -1;
}

}  // namespace wt
