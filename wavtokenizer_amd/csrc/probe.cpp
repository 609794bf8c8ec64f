// Entry points that launch kernels outside a plan: wt_codes_to_features, the single-stage calls and the probes through
// which the tests reach every GEMM form (wt_gemm_probe), every non-GEMM kernel (wt_op_probe), the fused resblocks
// (wt_resblock_probe), the LSTM recurrence (wt_lstm_probe), the vector quantiser (wt_vq_probe) and the mixed-length geometry
// step (wt_geometry_probe) on their own.
#include "model.h"

using namespace wt;

extern "C" {

int wt_codes_to_features(const wt_model* m, const int64_t* codes, int32_t K, int32_t B, int64_t L, float* features,
                         void* stream) {
    if (!m || !codes || !features) { set_error("wt_codes_to_features: null argument"); return WT_ERR_INVALID; }
    if (K < 1 || K > m->arch.num_quantizers) { set_error("wt_codes_to_features: K exceeds the number of codebooks"); return WT_ERR_INVALID; }
    DeviceGuard dg(m->device);
    if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
    return launch_codes_to_features(codes, m->embed.w, K, m->arch.vq_bins, B, L, 512, features, static_cast<hipStream_t>(stream),
                                    m->bad_codes_dev);
}

int wt_sconv1d(const float* x, const float* w, const float* bias, float* y, int32_t B, int64_t T, int32_t Cin,
               int32_t Cout, int32_t k, int32_t stride, int32_t dilation, int32_t elu_input, void* stream) {
    ConvW cw; cw.w = const_cast<float*>(w); cw.b = const_cast<float*>(bias); cw.cout = Cout; cw.cin = Cin; cw.k = k;
    GemmArgs a = sconv_args(cw, B, T, stride, dilation);
    a.A = x; a.C = y;
    return launch_gemm(a, elu_input ? PRO_ELU : PRO_NONE, EPI_BIAS, static_cast<hipStream_t>(stream));
}

// Both operands of a single-stage S32 call are split here (the plans' producers write S32 directly), each with a
// per-tensor power-of-two scale chosen on the device; `tail` = 256 spare bytes after the two S32 arrays
static int split_pair(const float* w, long nw, const float* x, long nx, char* ws_w, char* ws_x, char* tail, GemmArgs& a,
                      hipStream_t s) {
    unsigned* bits = reinterpret_cast<unsigned*>(tail);
    float* sc = reinterpret_cast<float*>(tail + 16);              // {scale_w, scale_x, 1 / (scale_w * scale_x)}
    if (int rc = launch_pow2_scales(w, nw, x, nx, bits, sc, s)) return rc;
    if (int rc = launch_split_s32(w, ws_w, nw, s, sc)) return rc;
    if (int rc = launch_split_s32(x, ws_x, nx, s, sc + 1)) return rc;
    a.W_hi = ws_w;
    a.A = reinterpret_cast<const float*>(ws_x);
    a.acc_scale_dev = sc + 2;
    return 0;
}

int wt_linear(const float* x, const float* w, const float* bias, float* y, int64_t M, int32_t N, int32_t K,
              int32_t f16x3, void* workspace, void* stream) {
    if (!x || !w || !y) { set_error("wt_linear: null argument"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GemmArgs a = linear_args(w, bias, M, N, K);
    a.A = x; a.C = y;
    if (!f16x3) return launch_gemm(a, PRO_NONE, EPI_BIAS, s);
    if (!workspace) { set_error("wt_linear: the f16x3 modes need a workspace"); return WT_ERR_INVALID; }
    char* hi = static_cast<char*>(workspace);
    if (f16x3 == 1) { set_error("wt_linear: mode 1 (the in-loop split kernel of round 1) was removed; use 2, 3 or 4"); return WT_ERR_INVALID; }
    char* xs = hi + (size_t)N * K * 4;
    if (int rc = split_pair(w, (long)N * K, x, (long)M * K, hi, xs, xs + (size_t)M * K * 4, a, s)) return rc;
    // timing-experiment builds (WT_GEMM16S_DBG: tools/gemm16s_bench.py) leave their clock stamps behind the scales
    a.dbg_stamps = reinterpret_cast<unsigned long long*>(xs + (size_t)M * K * 4 + 256);
    if (f16x3 == 4) return launch_gemm16s(a, EPI_BIAS_GELU, OUT_S32, s);      // ConvNeXt pwconv1: exact-erf GELU epilogue, S32 out
    return launch_gemm16s(a, EPI_BIAS, f16x3 == 3 ? 1 : 0, s);
}

int wt_conv1d_s32(const float* x, const float* w, const float* bias, float* y, int32_t B, int64_t T, int32_t Cin,
                  int32_t Cout, int32_t k, int32_t stride, int32_t zero_same, void* workspace, void* stream) {
    if (!x || !w || !y || !workspace) { set_error("wt_conv1d_s32: null argument"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    ConvW cw; cw.w = const_cast<float*>(w); cw.b = const_cast<float*>(bias); cw.cout = Cout; cw.cin = Cin; cw.k = k;
    GemmArgs a = zero_same ? zconv_args(cw, B, (int)T) : sconv_args(cw, B, T, stride, 1);
    char* ws = static_cast<char*>(workspace);
    char* xs = ws + (size_t)Cout * k * Cin * 4;
    if (int rc = split_pair(w, (long)Cout * k * Cin, x, (long)B * T * Cin, ws, xs, xs + (size_t)B * T * Cin * 4, a, s)) return rc;
    a.C = y;
    return launch_gemm16s(a, EPI_BIAS, 0, s);
}

static size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// wt_gemm_probe: the S32 copies of A, A2 and B in the workspace (same element offsets as the fp32 arrays), then the scale
struct ProbeLayout { long nA = 0, nA2 = 0, nB = 0; size_t oA2 = 0, oB = 0, oScale = 0, total = 0; };
static ProbeLayout probe_layout(const wt_gemm_desc& d) {
    ProbeLayout L;
    const long clips = d.M / d.T_out;
    const long a_cols = d.A2 ? d.K1 : d.Cin;
    L.nA = (d.nz - 1) * d.zA + (clips - 1) * d.a_bstride + (long)(d.T_in - 1) * d.a_rstride + a_cols;
    if (d.A2) L.nA2 = (clips - 1) * d.a2_bstride + (long)(d.T_in - 1) * d.a2_rstride + (d.K - d.K1);
    L.nB = (d.nz - 1) * d.zW + (long)(d.N - 1) * d.w_rstride + d.K;
    L.oA2 = al256((size_t)L.nA * 4);
    L.oB = L.oA2 + al256((size_t)L.nA2 * 4);
    L.oScale = L.oB + al256((size_t)L.nB * 4);
    L.total = L.oScale + 256;
    return L;
}
// mix_geom is the descriptor's last field and optional: `size` may also be the struct's size without it (then NULL)
static bool gemm_desc_size_ok(const wt_gemm_desc* d) {
    return d && (d->size == (int32_t)sizeof(wt_gemm_desc) || d->size == (int32_t)offsetof(wt_gemm_desc, mix_geom));
}
static const int32_t* gemm_desc_mix(const wt_gemm_desc* d) { return d->size == (int32_t)sizeof(wt_gemm_desc) ? d->mix_geom : nullptr; }
// the descriptor as the launchers' arguments; every check that needs no HIP call (the launchers' own included)
static int probe_args(const wt_gemm_desc* d, char* ws, GemmArgs& a) {
    if (!gemm_desc_size_ok(d)) { set_error("wt_gemm_probe: descriptor missing or of another size"); return WT_ERR_INVALID; }
    const int32_t* mix = gemm_desc_mix(d);
    const bool e16 = d && (d->engine == 0 || d->engine == 2);       // gemm16s.hip: three products, or (2) the one-product twin
    if (mix && (!e16 || (reinterpret_cast<uintptr_t>(mix) & 3))) { set_error("wt_gemm_probe: mix_geom is a 4-byte aligned device table for gemm16s"); return WT_ERR_INVALID; }
    if (d->engine < 0 || d->engine > 2) { set_error("wt_gemm_probe: engine is 0 (gemm16s), 1 (gemm) or 2 (gemm16s, one product)"); return WT_ERR_INVALID; }
    if (!d->A || !d->B || !d->C) { set_error("wt_gemm_probe: A, B and C are required"); return WT_ERR_INVALID; }
    if (d->epi == EPI_ARGMAX) { set_error("wt_gemm_probe: the argmax epilogue is reached through wt_vq_probe"); return WT_ERR_INVALID; }
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->T_out <= 0 || d->T_in <= 0 || d->M % d->T_out || d->nz < 1 || d->taps < 1 ||
        d->stride < 1 || d->dil < 1 || d->pad_left < 0 || (d->pad_mode != PAD_ZERO && d->pad_mode != PAD_REFLECT) ||
        d->a_bstride < 0 || d->a_rstride < 0 || d->a2_bstride < 0 || d->a2_rstride < 0 || d->w_rstride < d->K ||
        d->c_rstride < d->N || d->r_rstride < 0 || d->zA < 0 || d->zW < 0 || d->zC < 0 || (d->nz > 1 && d->zC <= 0)) {
        set_error("wt_gemm_probe: bad extents or strides"); return WT_ERR_INVALID;
    }
    if (d->engine == 1 && (d->out != OUT_F32 || d->A2 || d->tap_pair)) {
        set_error("wt_gemm_probe: gemm.hip writes fp32 and has no second K source or tap pairing"); return WT_ERR_INVALID;
    }
    if (e16 && d->pro != PRO_NONE) { set_error("wt_gemm_probe: gemm16s has no operand prologue"); return WT_ERR_INVALID; }
    if (d->tap_pair && (d->taps != 2 * d->stride || d->dil != 1)) { set_error("wt_gemm_probe: tap pairing needs k = 2 * stride, dilation 1"); return WT_ERR_INVALID; }
    if (e16 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 255))) { set_error("wt_gemm_probe: gemm16s needs a 256-byte aligned workspace"); return WT_ERR_INVALID; }
    a = GemmArgs{};
    a.a_bstride = d->a_bstride; a.a_rstride = d->a_rstride; a.T_in = d->T_in; a.T_out = d->T_out; a.Cin = d->Cin; a.taps = d->taps;
    a.stride = d->stride; a.dil = d->dil; a.pad_left = d->pad_left; a.pad_mode = d->pad_mode; a.Tp = d->Tp;
    a.a2_bstride = d->a2_bstride; a.a2_rstride = d->a2_rstride; a.K1 = d->K1;
    a.w_rstride = d->w_rstride; a.bias = d->bias; a.M = d->M; a.N = d->N; a.K = d->K;
    a.C = d->C; a.c_rstride = d->c_rstride; a.C2 = d->C2; a.R = d->R; a.r_rstride = d->r_rstride; a.gamma = d->gamma;
    a.alpha = d->alpha; a.nz = d->nz; a.zA = d->zA; a.zW = d->zW; a.zC = d->zC; a.head_kb = d->head_kb; a.tap_pair = d->tap_pair ? 1 : 0;
    if (d->engine == 1) {
        a.A = d->A; a.W = d->B;
        return check_gemm(a, d->pro, d->epi) ? WT_ERR_INVALID : WT_OK;
    }
    const ProbeLayout L = probe_layout(*d);
    a.A = reinterpret_cast<const float*>(ws);
    a.A2 = d->A2 ? reinterpret_cast<const float*>(ws + L.oA2) : nullptr;
    a.W = d->B; a.W_hi = ws + L.oB;
    a.status = reinterpret_cast<unsigned*>(d->status);
    return check_gemm16s(a, d->epi, d->out, mix, d->engine == 2 ? GEMM16S_F16 : GEMM16S_F16X3) ? WT_ERR_INVALID : WT_OK;
}

size_t wt_gemm_probe_workspace_bytes(const wt_gemm_desc* d) {
    if (!gemm_desc_size_ok(d) || (d->engine != 0 && d->engine != 2) || d->M <= 0 || d->T_out <= 0 || d->nz < 1) return 0;
    return probe_layout(*d).total;
}

int wt_gemm_probe(const wt_gemm_desc* d, wt_launch_form* form, void* workspace, void* stream) {
    char* ws = static_cast<char*>(workspace);
    GemmArgs a;
    if (int rc = probe_args(d, ws, a)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    LaunchForm lf;
    a.form = &lf;
    if (d->engine == 1) {
        if (int rc = launch_gemm(a, d->pro, d->epi, s)) return rc;
    } else {
        const ProbeLayout L = probe_layout(*d);
        float* scale_dev = reinterpret_cast<float*>(ws + L.oScale);
        float scale = 1.f;
        if (!d->b_is_act) {      // a weight: the plans' per-tensor power of two (weights.cpp add_s32), chosen over its logical rows
            std::vector<float> h((size_t)L.nB);
            WT_HIP_CHECK(hipMemcpyAsync(h.data(), d->B, (size_t)L.nB * 4, hipMemcpyDeviceToHost, s));
            WT_HIP_CHECK(hipStreamSynchronize(s));
            float amax = 0.f;
            for (long z = 0; z < d->nz; ++z)
                for (long n = 0; n < d->N; ++n)
                    for (long k = 0; k < d->K; ++k) {
                        const float v = std::fabs(h[(size_t)(z * d->zW + n * d->w_rstride + k)]);
                        if (!(v <= 3.0e38f)) { set_error("wt_gemm_probe: a non-finite weight has no S32 copy"); return WT_ERR_INVALID; }
                        amax = std::max(amax, v);
                    }
            scale = s32_weight_scale(amax);
            if (scale == 0.f) { set_error("wt_gemm_probe: a weight whose maximum lies below 2^-126 has no S32 copy"); return WT_ERR_INVALID; }
            uint32_t bits;
            memcpy(&bits, &scale, 4);
            if (int rc = launch_fill_u32(scale_dev, bits, 16, s)) return rc;
            a.acc_scale = 1.f / scale;
        }
        if (int rc = launch_split_s32(d->B, ws + L.oB, L.nB, s, scale != 1.f ? scale_dev : nullptr)) return rc;
        if (int rc = launch_split_s32(d->A, ws, L.nA, s)) return rc;
        if (d->A2) if (int rc = launch_split_s32(d->A2, ws + L.oA2, L.nA2, s)) return rc;
        if (int rc = launch_gemm16s(a, d->epi, d->out, s, gemm_desc_mix(d), d->engine == 2 ? GEMM16S_F16 : GEMM16S_F16X3)) return rc;
    }
    if (form) *form = wt_launch_form{lf.BM, lf.BN, lf.waves_m, lf.waves_n, lf.stages, lf.ks, lf.prod, lf.staged, lf.bias_cache, lf.G, lf.tiles};
    return WT_OK;
}

// wt_op_probe: every check that needs no HIP call and that the launchers do not make themselves (they trust the plans)
static int op_probe_check(const wt_op_desc* d) {
    auto bad = [](const char* m) { set_error(std::string("wt_op_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || (d->size != (int32_t)sizeof(wt_op_desc) && d->size != (int32_t)offsetof(wt_op_desc, lengths))) return bad("descriptor missing or of another size");
    const int32_t* lengths = d->size == (int32_t)sizeof(wt_op_desc) ? d->lengths : nullptr;
    if (lengths) {
        if (reinterpret_cast<uintptr_t>(lengths) & 3) return bad("lengths misaligned");
        const bool aware = d->op == WT_OP_GN_APPLY || d->op == WT_OP_GN_STATS || (d->op == WT_OP_ROWNORM && d->mode == RN_DWCONV) ||
                           d->op == WT_OP_SOFTMAX || d->op == WT_OP_ISTFT_OLA || d->op == WT_OP_TRANSPOSE || d->op == WT_OP_CODE_ROWS;
        if (!aware) return bad("this op has no length-aware launch");
        if (d->op == WT_OP_SOFTMAX && (d->L <= 0 || d->n % d->L)) return bad("the length-aware softmax needs whole clips of L rows");
    }
    if (d->op < WT_OP_GN_APPLY || (d->op > WT_OP_S32_AMAX && d->op != WT_OP_CODE_ROWS)) return bad("unknown op");     // (11 is unassigned)
    auto al16 = [](const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); };
    const void* ptrs[] = {d->p0, d->p1, d->p2, d->p3, d->p4, d->p5, d->y, d->y2, d->y3};
    for (const void* p : ptrs) if (!al16(p)) return bad("arrays must be 16-byte aligned");
    if (!d->x || (reinterpret_cast<uintptr_t>(d->x) & (d->op == WT_OP_SOFTMAX ? 3 : 15))) return bad("x missing or misaligned");
    if (reinterpret_cast<uintptr_t>(d->status) & 3) return bad("status misaligned");
    const bool shaped = d->op != WT_OP_SOFTMAX && d->op != WT_OP_ROW_SUMSQ && d->op != WT_OP_S32_AMAX;
    if (shaped && (d->B <= 0 || d->L <= 0)) return bad("extents must be positive");
    if (shaped && d->op != WT_OP_CONV_FIRST && d->op != WT_OP_ISTFT_OLA && (d->C <= 0 || (long)d->L * d->C >= (long)INT_MAX)) return bad("extents must be positive (and L * C < 2^31)");
    switch (d->op) {
    case WT_OP_GN_APPLY: case WT_OP_GN_STATS:
        if (!d->p0 || !d->p1 || !d->y2 || !d->y3 || (d->op == WT_OP_GN_APPLY && !d->y)) return bad("null argument");
        if (d->groups <= 0 || d->C % d->groups || d->C / d->groups > 256 || d->B > 65535) return bad("GroupNorm needs C % groups == 0, at most 256 channels per group, B <= 65535");
        break;
    case WT_OP_ROWNORM:
        if (!d->y || !d->p4 || !d->p5) return bad("null argument");
        if (d->mode < RN_DWCONV || d->mode > RN_AFFINE_IN) return bad("rownorm mode is 0, 1 or 2");
        if (d->mode == RN_DWCONV && (!d->p0 || !d->p1)) return bad("null argument");
        if (d->mode == RN_AFFINE_IN && (!d->p2 || !d->p3)) return bad("null argument");
        break;
    case WT_OP_SOFTMAX:
        if (d->n <= 0 || d->n > INT_MAX || d->L <= 0 || d->ld < d->L) return bad("softmax needs rows > 0 and 0 < L <= ld");
        break;
    case WT_OP_ISTFT_OLA:
        if (!d->p0 || !d->p1 || !d->y) return bad("null argument");
        if (d->n_fft <= 0 || d->hop <= 0 || d->n_fft % 4 || d->n_fft % d->hop || (d->n_fft - d->hop) % 2 || d->Kq < d->n_fft / 4 + 1)
            return bad("the ISTFT tail needs n_fft % 4 == 0, n_fft % hop == 0 and Kq > n_fft / 4");
        break;
    case WT_OP_CONV_FIRST:
        if (!d->p0 || !d->p1 || !d->y) return bad("null argument");
        if (d->k <= 0 || d->Cout <= 0 || d->Cout % 4) return bad("conv_first needs k > 0 and Cout % 4 == 0");
        break;
    case WT_OP_CONV_LAST:
        if (!d->p0 || !d->p1 || !d->y) return bad("null argument");
        if (d->k <= 0) return bad("conv_last needs k > 0");
        break;
    case WT_OP_TRANSPOSE:
        if (!d->y) return bad("null argument");
        if (d->B > 65535 || (d->L + 31) / 32 > 65535) return bad("transpose: too many tiles for one launch");
        break;
    case WT_OP_CONVTR:
        if (!d->p0 || !d->p1 || !d->y) return bad("null argument");
        if (d->stride <= 0 || d->k < d->stride || d->Cout <= 0 || d->Cout % 4) return bad("convtr needs k >= stride > 0 and Cout % 4 == 0");
        break;
    case WT_OP_ROW_SUMSQ:
        if (!d->y) return bad("null argument");
        if (d->n <= 0 || d->C <= 0 || d->C % 4) return bad("row_sumsq needs rows > 0 and C % 4 == 0");
        break;
    case WT_OP_S32_AMAX:
        if (!d->y) return bad("null argument");
        if (d->n <= 0 || d->n % 32) return bad("s32_amax needs whole S32 groups of 32 values");
        break;
    case WT_OP_CODE_ROWS:
        if (!d->p0 || !d->y) return bad("null argument");
        if (d->k < 1 || d->n < 1 || d->n > INT_MAX) return bad("code_rows needs k >= 1 codebooks of 1 <= n < 2^31 bins");
        if (d->C % 4 || d->C > 1024) return bad("code_rows needs C % 4 == 0 and C <= 1024");
        if (d->out_s32 && d->C % 32) return bad("code_rows: an S32 output needs C % 32 == 0");
        if ((long)d->B * d->L >= (long)INT_MAX) return bad("code_rows: too many frames for one launch");
        break;
    }
    return WT_OK;
}

int wt_op_probe(const wt_op_desc* d, wt_op_form* form, void* stream) {
    if (int rc = op_probe_check(d)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto F = [](const void* p) { return static_cast<const float*>(p); };
    auto W = [](void* p) { return static_cast<float*>(p); };
    OpForm lf;
    const int* lens = d->size == (int32_t)sizeof(wt_op_desc) ? d->lengths : nullptr;
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    g_launch.form = &lf;
    int rc = 0;
    switch (d->op) {
    case WT_OP_GN_APPLY:
        rc = launch_gn_apply(F(d->x), F(d->p0), F(d->p1), W(d->y2), W(d->y3), W(d->y), d->flag ? 1 : 0, d->B, d->L, d->C, d->groups, d->eps, s,
                             d->out_s32 ? 1 : 0, const_cast<float*>(F(d->p2)), lens);
        break;
    case WT_OP_GN_STATS:
        rc = launch_gn_stats(F(d->x), F(d->p0), F(d->p1), W(d->y2), W(d->y3), d->B, d->L, d->C, d->groups, d->eps, s, const_cast<float*>(F(d->p2)), lens);
        break;
    case WT_OP_ROWNORM:
        rc = launch_rownorm(d->mode, F(d->x), W(d->y), d->B, d->L, d->C, F(d->p0), F(d->p1), F(d->p2), F(d->p3), F(d->p4), F(d->p5), d->eps, s,
                            d->out_s32 ? 1 : 0, lens);
        break;
    case WT_OP_SOFTMAX:
        rc = launch_softmax(const_cast<float*>(F(d->x)), (int)d->n, d->L, d->ld, s, W(d->y), lens);
        break;
    case WT_OP_ISTFT_OLA:
        rc = launch_istft_ola(F(d->x), F(d->p0), F(d->p1), W(d->y), d->B, d->L, d->n_fft, d->hop, d->Kq, d->flag ? 1 : 0, s, lens);
        break;
    case WT_OP_CONV_FIRST:
        rc = launch_conv_first(F(d->x), F(d->p0), F(d->p1), W(d->y), d->B, d->L, d->k, d->Cout, s);
        break;
    case WT_OP_CONV_LAST:
        rc = launch_conv_last(F(d->x), F(d->p0), F(d->p1), W(d->y), d->B, d->L, d->C, d->k, d->flag ? 1 : 0, s);
        break;
    case WT_OP_TRANSPOSE:
        rc = launch_transpose(F(d->x), W(d->y), d->B, d->L, d->C, s, d->out_s32 ? 1 : 0, lens);
        break;
    case WT_OP_CONVTR:
        rc = launch_convtr(F(d->x), F(d->p0), F(d->p1), W(d->y), d->B, d->L, d->C, d->Cout, d->k, d->stride, d->flag ? 1 : 0, s);
        break;
    case WT_OP_ROW_SUMSQ:
        rc = launch_row_sumsq(F(d->x), W(d->y), d->n, d->C, s);
        break;
    case WT_OP_S32_AMAX:
        rc = launch_s32_amax(d->x, d->n, static_cast<unsigned*>(d->y), s);
        break;
    case WT_OP_CODE_ROWS:
        rc = launch_code_rows(static_cast<const int64_t*>(d->x), F(d->p0), d->k, (int)d->n, d->B, d->L, d->C, W(d->y), s, d->out_s32 ? 1 : 0,
                              static_cast<unsigned*>(d->y2), lens);
        break;
    }
    g_launch = saved;
    if (rc) return rc;
    if (form) *form = wt_op_form{lf.kernel, lf.variant, lf.variant2, (int32_t)lf.grid[0], (int32_t)lf.grid[1], (int32_t)lf.grid[2], (int32_t)lf.block, (int32_t)lf.lds};
    return WT_OK;
}

size_t wt_vq_workspace_bytes(int64_t N, int32_t D, int32_t bins) {
    const size_t np = std::max(gemm_vq_parts(bins), gemm16s_vq_parts(bins));
    return al256((size_t)N * D * 4) + al256((size_t)bins * D * 4) + al256((size_t)N * sizeof(float)) +
           2 * al256((size_t)N * np * sizeof(float)) + al256((size_t)bins * sizeof(float)) + 512;
}

// The workspace of wt_vq_nearest / wt_vq_probe (wt_vq_workspace_bytes): S32 copies of x and the codebook, |x|^2, the partial
// (value, index) candidates, |e|^2, then the scales of split_pair
struct VqLayout { char *xs, *es; float* xx; float* pv; int* pi; float* ee; char* tail; int np; };
static VqLayout vq_layout(void* workspace, int64_t N, int32_t D, int32_t bins, bool s32) {
    VqLayout L;
    L.np = s32 ? gemm16s_vq_parts(bins) : gemm_vq_parts(bins);
    char* ws = static_cast<char*>(workspace);
    L.xs = ws; ws += al256((size_t)N * D * 4);
    L.es = ws; ws += al256((size_t)bins * D * 4);
    L.xx = reinterpret_cast<float*>(ws); ws += al256((size_t)N * sizeof(float));
    L.pv = reinterpret_cast<float*>(ws); ws += al256((size_t)N * L.np * sizeof(float));
    L.pi = reinterpret_cast<int*>(ws); ws += al256((size_t)N * L.np * sizeof(float));
    L.ee = reinterpret_cast<float*>(ws); ws += al256((size_t)bins * sizeof(float));
    L.tail = ws;
    return L;
}
// the distance GEMM's arguments as the encoder plan sets them (plan.cpp, "VQ"); ee: the caller's table, or the workspace's
static GemmArgs vq_args(const VqLayout& L, const float* x, const float* embed, const float* ee, int64_t N, int32_t D, int32_t bins,
                        float* pv, int* pi, bool s32) {
    GemmArgs a = linear_args(embed, nullptr, N, bins, D);
    a.A = x; a.vq_xx = L.xx; a.vq_ee = ee ? ee : L.ee; a.vq_pval = pv; a.vq_pidx = pi; a.vq_nparts = L.np;
    if (s32) { a.A = reinterpret_cast<const float*>(L.xs); a.W_hi = L.es; }
    return a;
}
// |x|^2, |e|^2 (rebuilt per call on the device by row_sumsq unless the caller brings the table) and the distance GEMM with
// its per-slab argmax epilogue
static int vq_distances(const VqLayout& L, GemmArgs a, const float* x, const float* embed, bool own_ee, int64_t N, int32_t D,
                        int32_t bins, bool s32, hipStream_t s) {
    if (int rc = launch_row_sumsq(x, L.xx, N, D, s)) return rc;
    if (own_ee) if (int rc = launch_row_sumsq(embed, L.ee, bins, D, s)) return rc;
    if (s32) {
        // what the encoder plan launches: distances on gemm16s.hip, per-slab argmax in its epilogue
        if (int rc = split_pair(embed, (long)bins * D, x, (long)N * D, L.es, L.xs, L.tail, a, s)) return rc;
        return launch_gemm16s(a, EPI_ARGMAX, OUT_F32, s);
    }
    return launch_gemm(a, PRO_NONE, EPI_ARGMAX, s);
}

static int vq_nearest(const float* x, const float* embed, int64_t N, int32_t D, int32_t bins, int64_t* codes_out,
                      void* workspace, void* stream, bool s32) {
    if (!x || !embed || !codes_out || !workspace) { set_error("wt_vq_nearest: null argument"); return WT_ERR_INVALID; }
    if (s32 && (D % 32)) { set_error("wt_vq_nearest: the split-f16 kernel needs D % 32 == 0"); return WT_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const VqLayout L = vq_layout(workspace, N, D, bins, s32);
    const int np = L.np;
    if (int rc = vq_distances(L, vq_args(L, x, embed, nullptr, N, D, bins, L.pv, L.pi, s32), x, embed, true, N, D, bins, s32, s)) return rc;
    for (int64_t r0 = 0; r0 < N; r0 += 8192) {
        const int n = (int)std::min<int64_t>(8192, N - r0);
        if (int rc = launch_vq_finalize(L.pv + r0 * np, L.pi + r0 * np, np, embed, codes_out + r0, nullptr, 1, n, D, bins, s)) return rc;
    }
    return WT_OK;
}
int wt_vq_nearest(const float* x, const float* embed, int64_t N, int32_t D, int32_t bins, int64_t* codes_out,
                  void* workspace, void* stream) {
    return vq_nearest(x, embed, N, D, bins, codes_out, workspace, stream, true);
}
int wt_vq_nearest_f32(const float* x, const float* embed, int64_t N, int32_t D, int32_t bins, int64_t* codes_out,
                      void* workspace, void* stream) {
    return vq_nearest(x, embed, N, D, bins, codes_out, workspace, stream, false);
}

// wt_vq_probe: the launches of the encoder plan's VQ steps (row_sumsq, the argmax GEMM, ONE vq_finalize over B clips of L
// frames) with the partial candidates in the caller's memory.  Every check that needs no HIP call comes first, the launchers'
// own included (check_gemm16s / check_gemm; vq_finalize's D % 256), so a refused problem launches nothing.
int wt_vq_probe(const wt_vq_desc* d, wt_vq_form* form, void* workspace, void* stream) {
    auto bad = [](const char* m) { set_error(std::string("wt_vq_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_vq_desc)) return bad("descriptor missing or of another size");
    if (d->kernel != 0 && d->kernel != 1) return bad("kernel is 0 (gemm16s, split-f16) or 1 (gemm, fp32)");
    if (!d->x || !d->embed || !d->codes || !d->pval || !d->pidx) return bad("x, embed, codes, pval and pidx are required");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return bad("needs a 256-byte aligned workspace");
    if (d->B < 1 || d->B > 65535 || d->L < 1 || d->D < 1 || d->bins < 1 || (long)d->B * d->L >= (long)INT_MAX / 2)
        return bad("needs 1 <= B <= 65535, L >= 1, D >= 1, bins >= 1 and B * L < 2^30");
    const void* p16[] = {d->x, d->embed, d->ee};
    for (const void* p : p16) if (reinterpret_cast<uintptr_t>(p) & 15) return bad("x, embed and ee must be 16-byte aligned");
    const void* p4[] = {d->feat, d->pval, d->pidx, d->status};
    for (const void* p : p4) if (reinterpret_cast<uintptr_t>(p) & 3) return bad("feat, pval, pidx and status must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d->codes) & 7) return bad("codes must be 8-byte aligned");
    if (d->D % 4) return bad("row_sumsq needs D % 4 == 0");
    if (d->D % 256) return bad("vq_finalize: codebook width must be a multiple of 256");
    const bool s32 = d->kernel == 0;
    const int64_t N = (int64_t)d->B * d->L;
    const VqLayout L = vq_layout(workspace, N, d->D, d->bins, s32);
    GemmArgs a = vq_args(L, d->x, d->embed, d->ee, N, d->D, d->bins, d->pval, d->pidx, s32);
    if (s32 ? check_gemm16s(a, EPI_ARGMAX, OUT_F32, nullptr, GEMM16S_F16X3) : check_gemm(a, PRO_NONE, EPI_ARGMAX)) return WT_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    LaunchForm lf;
    a.form = &lf;
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    int rc = vq_distances(L, a, d->x, d->embed, d->ee == nullptr, N, d->D, d->bins, s32, s);
    if (!rc) rc = launch_vq_finalize(d->pval, d->pidx, L.np, d->embed, d->codes, d->feat, d->B, d->L, d->D, d->bins, s);
    g_launch = saved;
    if (rc) return rc;
    if (form) *form = wt_vq_form{lf.BM, lf.BN, lf.waves_m, lf.waves_n, lf.G, lf.tiles, lf.group_m, lf.group_n, L.np, (d->L + 31) / 32, d->B};
    return WT_OK;
}

// wt_vq_residual_probe: one launch of vq_residual_kernel on the caller's arrays (the candidates are the caller's, so any code
// can be forced).  Everything is checked before the first HIP call.
int wt_vq_residual_probe(const wt_vq_residual_desc* d, wt_vq_residual_form* form, void* stream) {
    auto bad = [](const char* m) { set_error(std::string("wt_vq_residual_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_vq_residual_desc)) return bad("descriptor missing or of another size");
    if (!d->pval || !d->pidx || !d->x || !d->embed || !d->codes || !d->r || !d->xx) return bad("pval, pidx, x, embed, codes, r and xx are required");
    if (d->rows < 1 || d->rows >= (int64_t)INT_MAX || d->bins < 1 || d->nparts < 1 || d->D < 1) return bad("needs 1 <= rows < 2^31, D >= 1, bins >= 1 and nparts >= 1");
    if (d->D % 256) return bad("vq_residual: codebook width must be a multiple of 256");
    const void* p16[] = {d->x, d->embed, d->r, d->r_s32};
    for (const void* p : p16) if (reinterpret_cast<uintptr_t>(p) & 15) return bad("x, embed, r and r_s32 must be 16-byte aligned");
    const void* p4[] = {d->pval, d->pidx, d->xx, d->status};
    for (const void* p : p4) if (reinterpret_cast<uintptr_t>(p) & 3) return bad("pval, pidx, xx and status must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d->codes) & 7) return bad("codes must be 8-byte aligned");
    OpForm of;
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    g_launch.form = &of;
    const int rc = launch_vq_residual(d->pval, d->pidx, d->nparts, d->x, d->embed, d->codes, d->r, static_cast<float*>(d->r_s32), d->xx,
                                      (long)d->rows, d->D, d->bins, static_cast<hipStream_t>(stream));
    g_launch = saved;
    if (rc) return rc;
    if (form) *form = wt_vq_residual_form{(int32_t)of.grid[0], (int32_t)of.block, of.variant};
    return WT_OK;
}

int wt_resblock(const float* x, const float* wav, const float* e0_w, const float* e0_b, const float* w3, const float* b3,
                const float* w1, const float* b1, const float* ws, const float* bs, float* y, int32_t B, int64_t T,
                int32_t C, int32_t elu_out, int32_t out_s32, int32_t fp32_chain, void* stream) {
    if ((!x && !wav) || !w3 || !b3 || !w1 || !b1 || !ws || !bs || !y) { set_error("wt_resblock: null argument"); return WT_ERR_INVALID; }
    if (wav && (!e0_w || !e0_b)) { set_error("wt_resblock: the folded first conv needs its weights"); return WT_ERR_INVALID; }
    if (B < 1 || T < 1 || (long)B * T >= (long)INT_MAX) { set_error("wt_resblock: bad shape"); return WT_ERR_INVALID; }
    if (fp32_chain && out_s32) { set_error("wt_resblock: the fp32 kernel writes fp32"); return WT_ERR_INVALID; }
    ResblockArgs a{};
    a.x = wav ? nullptr : x; a.wav = wav; a.e0_w = e0_w; a.e0_b = e0_b;
    a.W3 = w3; a.b3 = b3; a.W1 = w1; a.b1 = b1; a.Ws = ws; a.bs = bs;
    a.y = y; a.B = B; a.T = (int)T; a.C = C; a.elu_out = elu_out ? 1 : 0; a.out_s32 = out_s32 ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return fp32_chain ? launch_resblock(a, s) : launch_resblock16(a, s);
}

// The stage-1 kernel of the shipped encode plan: first conv + SEANetResnetBlock + ELU + the stage's down conv in one launch
// (resblock16.hip, DOWN); wd [64][2r][32], y_down [B][ceil(T / r)][64] fp32.
int wt_resblock_down(const float* wav, const float* e0_w, const float* e0_b, const float* w3, const float* b3, const float* w1,
                     const float* b1, const float* ws, const float* bs, const float* wd, const float* bd, float* y_down,
                     int32_t B, int64_t T, int32_t r, void* stream) {
    if (!wav || !e0_w || !e0_b || !w3 || !b3 || !w1 || !b1 || !ws || !bs || !wd || !bd || !y_down) {
        set_error("wt_resblock_down: null argument"); return WT_ERR_INVALID;
    }
    if (B < 1 || T < 1 || (long)B * T >= (long)INT_MAX) { set_error("wt_resblock_down: bad shape"); return WT_ERR_INVALID; }
    if (!resblock16_down_fusable(32, T, r, 2 * r)) {
        set_error("wt_resblock_down: needs stride 2 or 4 and T >= 1024"); return WT_ERR_INVALID;
    }
    ResblockArgs a{};
    a.wav = wav; a.e0_w = e0_w; a.e0_b = e0_b; a.W3 = w3; a.b3 = b3; a.W1 = w1; a.b1 = b1; a.Ws = ws; a.bs = bs;
    a.Wd = wd; a.bd = bd; a.y_down = y_down; a.R = r; a.B = B; a.T = (int)T; a.C = 32;
    return launch_resblock16_down(a, static_cast<hipStream_t>(stream));
}

// wt_geometry_words: the table layout of common.h (GEOM_*, geom_final, geom_L) for a chain of n_stages encoder stages
int wt_geometry_words(int32_t n_stages, wt_geom_words* out) {
    if (!out || n_stages < 1 || n_stages > GEOM_MAX_STAGES) { set_error("wt_geometry_words: 1 to " + std::to_string((int)GEOM_MAX_STAGES) + " encoder stages"); return WT_ERR_INVALID; }
    *out = wt_geom_words{GEOM_WORDS, GEOM_VALID, GEOM_T, GEOM_TREAD, GEOM_STAGE0, GEOM_STAGE_WORDS, GEOM_C3, GEOM_SC, GEOM_DOWN,
                         geom_final(n_stages), geom_L(n_stages), GEOM_MAX_STAGES};
    return WT_OK;
}

int wt_geometry_probe(const wt_geom_desc* d, void* stream) {
    static_assert(GEOM_MAX_STAGES <= (int)(sizeof(wt_geom_desc::kd) / sizeof(int32_t)), "wt_geom_desc holds every stage the table can");
    auto bad = [](const char* m) { set_error(std::string("wt_geometry_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_geom_desc)) return bad("descriptor missing or of another size");
    if (!d->lengths || !d->geom || (reinterpret_cast<uintptr_t>(d->lengths) & 3) || (reinterpret_cast<uintptr_t>(d->geom) & 3)) return bad("lengths and geom are 4-byte aligned device arrays");
    if (d->B < 1 || d->tmin < 1 || d->Tpad < d->tmin || d->Tpad >= (int64_t)INT_MAX) return bad("needs B >= 1 and 1 <= tmin <= Tpad < 2^31");
    if (d->n_stages < 1 || d->n_stages > GEOM_MAX_STAGES) return bad(("1 to " + std::to_string((int)GEOM_MAX_STAGES) + " encoder stages").c_str());
    for (int i = 0; i < d->n_stages; ++i)
        if (d->rd[i] < 1 || d->kd[i] < d->rd[i]) return bad("a stage's down conv needs kernel size >= stride >= 1");
    if (d->kf < 1) return bad("the final conv needs a kernel size");
    if (int rc = launch_mixed_geometry(d->lengths, d->geom, d->B, d->Tpad, d->tmin, d->n_stages, d->kd, d->rd, d->kf,
                                       static_cast<hipStream_t>(stream))) return rc < -1 ? rc : (int)WT_ERR_INVALID;
    return WT_OK;
}

// wt_resblock_probe: every check that needs no HIP call; the launchers' own refusals come back through their return value,
// which they decide before their first HIP call
int wt_resblock_probe(const wt_resblock_desc* d, wt_resblock_form* form, void* stream) {
    auto bad = [](const char* m) { set_error(std::string("wt_resblock_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_resblock_desc)) return bad("descriptor missing or of another size");
    const bool down = d->r != 0;
    if (!d->w3 || !d->b3 || !d->w1 || !d->b1 || !d->ws || !d->bs || !d->y) return bad("null argument");
    if (!d->x && !d->wav) return bad("needs x or the waveform");
    if (d->wav && (!d->e0_w || !d->e0_b)) return bad("the folded first conv needs its weights");
    if (down && (!d->wav || !d->wd || !d->bd)) return bad("the fused down conv needs the waveform and its weights");
    if (d->B < 1 || d->T < 1 || (long)d->B * d->T >= (long)INT_MAX) return bad("bad shape");
    if (d->fp32_chain && (d->out_s32 || down || d->mix_T || d->mix_Tread)) return bad("the fp32 kernel writes fp32, has no down conv and no mixed-length form");
    if ((d->mix_T != nullptr) != (d->mix_Tread != nullptr)) return bad("a mixed-length launch needs both length words");
    const void* p4[] = {d->wav, d->e0_w, d->e0_b, d->b3, d->b1, d->bs, d->bd, d->status, d->mix_T, d->mix_Tread};
    for (const void* p : p4) if (reinterpret_cast<uintptr_t>(p) & 3) return bad("arrays must be 4-byte aligned");
    const void* p16[] = {d->x, d->w3, d->w1, d->ws, d->wd, d->y};
    for (const void* p : p16) if (reinterpret_cast<uintptr_t>(p) & 15) return bad("x, y and the conv weights must be 16-byte aligned");
    ResblockArgs a{};
    a.x = d->wav ? nullptr : d->x; a.wav = d->wav; a.e0_w = d->e0_w; a.e0_b = d->e0_b;
    a.W3 = d->w3; a.b3 = d->b3; a.W1 = d->w1; a.b1 = d->b1; a.Ws = d->ws; a.bs = d->bs;
    a.B = d->B; a.T = d->T; a.C = d->C;
    if (down) { a.Wd = d->wd; a.bd = d->bd; a.y_down = d->y; a.R = d->r; }
    else { a.y = d->y; a.elu_out = d->elu_out ? 1 : 0; a.out_s32 = d->out_s32 ? 1 : 0; }
    ResblockMix mix;
    mix.T = d->mix_T; mix.Tread = d->mix_Tread;
    const ResblockMix* mp = d->mix_T ? &mix : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RbForm lf;
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    g_launch.rb_form = &lf;
    const int rc = d->fp32_chain ? launch_resblock(a, s) : down ? launch_resblock16_down(a, s, mp) : launch_resblock16(a, s, mp);
    g_launch = saved;
    if (rc) return rc;
    if (form) *form = wt_resblock_form{lf.kernel, lf.C, lf.fold, lf.down, lf.fpw, (int32_t)lf.grid, (int32_t)lf.block, (int32_t)lf.lds, (int32_t)lf.tiles};
    return WT_OK;
}

// wt_lstm_probe: every check that needs no HIP call and that issue_lstm and the launchers leave to the plans
static int lstm_probe_check(const wt_lstm_desc* d) {
    auto bad = [](const char* m) { set_error(std::string("wt_lstm_probe: ") + m); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_lstm_desc)) return bad("descriptor missing or of another size");
    if (d->which != 0 && d->which != 1) return bad("which is 0 (encoder) or 1 (SEANetDecoder)");
    if (d->kernel != LSTM_PERSIST && d->kernel != LSTM_STEP_F16 && d->kernel != LSTM_STEP_F32) return bad("kernel is 0 (persistent), 1 (step, split-f16) or 2 (step, fp32)");
    if (!d->xg || !d->x || !d->y) return bad("null argument");
    const void* p16[] = {d->xg, d->x, d->y};
    for (const void* p : p16) if (reinterpret_cast<uintptr_t>(p) & 15) return bad("xg, x and y must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d->status) & 3) return bad("status misaligned");
    if (d->B < 1 || d->L < 1) return bad("needs B >= 1 and L >= 1");
    if (d->kernel == LSTM_PERSIST && (d->B > 128 || d->L >= 65536)) return bad("the persistent kernel takes B <= 128 and L < 65536");
    if (d->kernel != LSTM_PERSIST && (d->L > 65535 || d->B > 65535 * 64)) return bad("the step kernels take L <= 65535 (and B <= 65535 * 64)");
    // no plan writes S32 from the fp32 chain (plan.cpp: an S32 output needs an S32 plan, whose step kernel is the split-f16 one)
    if (d->kernel == LSTM_STEP_F32 && d->out_s32) return bad("the fp32 step kernel writes fp32 in every plan");
    return WT_OK;
}

size_t wt_lstm_probe_workspace_bytes(const wt_lstm_desc* d) {
    if (lstm_probe_check(d)) return 0;
    if (d->kernel == LSTM_PERSIST) return al256(lstm_persist_hx_bytes() + lstm_persist_ctl_bytes());
    return al256(lstm_step_state_numel(d->B, 512) * sizeof(float));
}

int wt_lstm_probe(const wt_model* m, const wt_lstm_desc* d, wt_lstm_form* form, void* workspace, void* stream) {
    auto bad = [](const char* msg) { set_error(std::string("wt_lstm_probe: ") + msg); return (int)WT_ERR_INVALID; };
    if (int rc = lstm_probe_check(d)) return rc;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return bad("needs a 256-byte aligned workspace");
    if (!m) return bad("null model");
    if (d->which == 1 && !m->has_seadec) return bad("the model holds no SEANetDecoder");
    const LstmW& w = d->which ? m->sd_lstm : m->enc_lstm;
    if (m->H != 512 || !w.b1 || !(d->kernel == LSTM_PERSIST ? w.Wp : d->kernel == LSTM_STEP_F16 ? w.W0h : w.W0)) return bad("the model holds no such packing");
    if (d->kernel == LSTM_PERSIST && !full_chip(m->device)) return bad("the persistent kernel needs a whole 256-CU MI355X");
    DeviceGuard dg(m->device);
    if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    LstmForm lf;
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    g_launch.lstm_form = &lf;
    const int rc = issue_lstm(w, d->xg, d->x, d->y, static_cast<float*>(workspace), d->B, d->L, 512, d->elu_out != 0, d->out_s32 != 0, d->kernel, s);
    g_launch = saved;
    // a persistent launch holds every CU until it ends: it is over before the caller can issue the next one
    if (d->kernel == LSTM_PERSIST && lf.launches) WT_HIP_CHECK(hipStreamSynchronize(s));
    if (rc) return rc;
    if (form) *form = wt_lstm_form{lf.kernel, lf.small, lf.Bx, (int32_t)lf.grid[0], (int32_t)lf.grid[1], (int32_t)lf.block, (int32_t)lf.lds, lf.launches};
    return WT_OK;
}

// wt_split_probe: launch_split_s32, launch_unsplit_s32 and launch_pow2_scales on the caller's arrays, as add_s32,
// ensure_f32_weights and split_pair call them
int wt_split_probe(const wt_split_desc* d, void* stream) {
    auto bad = [](const char* msg) { set_error(std::string("wt_split_probe: ") + msg); return (int)WT_ERR_INVALID; };
    if (!d || d->size != (int32_t)sizeof(wt_split_desc)) return bad("descriptor missing or of another size");
    if (d->op < 0 || d->op > 2) return bad("op is 0 (split), 1 (unsplit) or 2 (power-of-two scales)");
    if (!d->x || !d->out || d->n < 1) return bad("x, out and n >= 1 are required");
    if (d->op != 2 && (d->n % 32)) return bad("the element count must be a multiple of 32");
    if (d->op == 2 && (!d->b || !d->bits || d->nb < 1)) return bad("op 2 needs b, nb >= 1 and bits");
    const void* p4[] = {d->x, d->b, d->out, d->scale, d->bits, d->status};
    for (const void* p : p4) if (reinterpret_cast<uintptr_t>(p) & 3) return bad("arrays must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LaunchCtx saved = g_launch;
    g_launch.status = reinterpret_cast<unsigned*>(d->status);
    int rc;
    if (d->op == 0) rc = launch_split_s32(static_cast<const float*>(d->x), d->out, (long)d->n, s, d->scale);
    else if (d->op == 1) rc = launch_unsplit_s32(d->x, static_cast<float*>(d->out), (long)d->n, d->inv_scale, s);
    else rc = launch_pow2_scales(static_cast<const float*>(d->x), (long)d->n, static_cast<const float*>(d->b), (long)d->nb, d->bits, static_cast<float*>(d->out), s);
    g_launch = saved;
    return rc;
}

}  // extern "C"
