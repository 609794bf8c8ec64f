// The one-product twin of the split-f16 GEMM (WT_PLAN_FLAG_F16_GEMM, wt_gemm_probe engine 2): gemm16h_kernel multiplies the hi
// halves of the S32 operands only - f16 products, fp32 accumulation, one MFMA where gemm16s_kernel issues three.  The kernel is
// the third inclusion of gemm16s_kernel.inc (gemm16s.hip), and launch16s_tiled there picks its tile form, so a problem runs
// on the form the default runs it on.  The instantiations are compiled here, beside gemm16s.hip's, to keep the build parallel.
#define WT_GEMM16H_TU
#include "gemm16s.hip"

namespace wt {

// launch_gemm16s's tail for GEMM16S_F16: `a` has passed check_gemm16s and carries the tile order
int launch_gemm16h_tiled(const GemmArgs& a, int epi, int out, hipStream_t s) {
#define WT_CASE16H(E, O) if (epi == E && out == O) return launch16s_tiled<E, O, 1>(a, s);
    WT_GEMM16H_PAIRS(WT_CASE16H)
#undef WT_CASE16H
    set_error("gemm16s: unsupported epilogue / output-format pair");
    return -1;
}

}  // namespace wt
