// Launch plans: per (kind, B, len) a flat list of kernel launches over a lifetime-packed workspace.  No compute
// happens on the host at call time.
#include "model.h"

namespace wt {

// The dense chain runs on S32 operands (the shipped path) unless the unfused debug plan or fp32 GEMMs are asked for, or
// the model's weights do not fit the split-f16 range (wt_model::s32_ok)
static bool site_fp32(const wt_plan* P, int site) { return (P->fp32_sites >> site) & 1u; }
static bool plan_fp32(const wt_plan* P) {
    if ((P->flags & WT_PLAN_FLAG_FP32_GEMM) || !P->model->s32_ok) return true;
    if (P->whole_site == SITE_SEADEC && !P->model->sd_s32_ok) return true;
    // plans that are one range site as a whole (wt_plan::whole_site); the decode plan decides site by site (build_decode)
    return P->whole_site >= 0 && site_fp32(P, P->whole_site);
}
static bool plan_unfused(const wt_plan* P) { return P->flags & WT_PLAN_FLAG_UNFUSED; }
static bool plan_s32(const wt_plan* P) { return !plan_unfused(P) && !plan_fp32(P); }

// Everything the S32 chain does not cover (the fp32 plans: WT_PLAN_FLAG_FP32_GEMM, the unfused debug twin, a model whose
// weights do not fit the split-f16 range) runs on the fp32 MFMA chain of gemm.hip
static int gemm_auto(const wt_plan* P, const GemmArgs& a, int pro, int epi, hipStream_t s) {
    // safety net for a model that came from a packed image (its fp32 GEMM weights are rebuilt on demand: wt_plan_create does
    // it for the plans it can tell will need them; any other fp32 GEMM finds them here, in the plan's first, eager call)
    if (P->model->f32_stale.load()) if (int rc = ensure_f32_weights(P->model)) return rc;
    return launch_gemm(a, pro, epi, s);
}

// The weight's S32 copy as the W operand of gemm16s.hip (the argument builders set it; gemm.hip ignores these fields)
static void set_s32(GemmArgs& a, const S32Copy& c) {
    a.W_hi = c.p; a.acc_scale = c.acc_scale; a.tap_pair = c.tap_pair ? 1 : 0;
}

// Both operands pre-split (S32): the activations were written in S32 by their producer, the weight has an S32 copy
// (mix: a mixed-length plan's geometry triple of this conv, launch_gemm16s)
// (prec: Prec16s, plan_prec below)
static int gemm_s32(const GemmArgs& a, int epi, int out, hipStream_t s, const int* mix = nullptr, int prec = GEMM16S_F16X3) {
    if (!a.W_hi) { set_error("internal: no S32 copy of this weight"); return WT_ERR_INVALID; }
    return launch_gemm16s(a, epi, out, s, mix, prec);
}
// WT_PLAN_FLAG_F16_GEMM (the decode kinds only: wt_plan_create_ex): every GEMM that runs on S32 operands multiplies their hi
// halves alone.  Producers, buffers and weights are what they are without the flag; a site on fp32 operands stays on gemm.hip
static int plan_prec(const wt_plan* P) { return (P->flags & WT_PLAN_FLAG_F16_GEMM) ? GEMM16S_F16 : GEMM16S_F16X3; }

// One GEMM step of a layer that runs on either operand form: S32 on gemm16s.hip (`out`: Out16s) or fp32 on gemm.hip
// (`pro`: its operand prologue)
static int dense(const wt_plan* P, bool s32, const GemmArgs& a, int pro, int epi, int out, hipStream_t s, const int* mix = nullptr) {
    if (mix && !s32) { set_error("internal: a mixed-length conv off the S32 route"); return WT_ERR_INVALID; }
    return s32 ? gemm_s32(a, epi, out, s, mix, plan_prec(P)) : gemm_auto(P, a, pro, epi, s);
}

// Activation x activation (attention S and O): the B operand is a plan buffer, S32 in W_hi on gemm16s.hip, fp32 in W on
// gemm.hip
static int dense_act(const wt_plan* P, bool s32, GemmArgs a, const float* b_op, int epi, int out, hipStream_t s) {
    if (s32) { a.W_hi = b_op; return launch_gemm16s(a, epi, out, s, nullptr, plan_prec(P)); }
    a.W = b_op;
    return gemm_auto(P, a, PRO_NONE, epi, s);
}

// The buffers of a GEMM step by id (-1: none), in the order the step lists them, bound to the prototype's pointers when it runs
struct GemmBufs {
    int A, A2, C, C2 = -1;
    bool r_is_c = false;         // the residual operand R is the output (updated in place)
    long x_off = 0;              // A starts this many elements into its buffer (the trimmed view of a transposed conv's output)
    int mix_word = -1;           // mixed-length plans: the conv's triple in the geometry table (launch_gemm16s)
};
// One GEMM step: registers it with the buffers it touches (geometry table, A, A2, C, C2: the order names the step and orders
// the range report), binds them at run time and calls dense().  Declared formats that disagree with what the step reads
// and writes fail the plan's creation (wt_plan::build_rc); BufSpec::holds_s32 stands in for the declaration of the
// SEANetDecoder buffers that wt_plan_buffer_info has always reported as fp32.
static void gemm_step(wt_plan* P, bool s32, const GemmArgs& proto, const GemmBufs& b, int pro, int epi, int out,
                      const std::string& name = "") {
    auto is_s32 = [&](int id) { return (P->bufs[id].fmt & BUF_S32) != 0 || P->bufs[id].holds_s32; };
    const int eff = s32 ? out : OUT_F32;         // gemm.hip writes fp32 whatever `out` says
    const bool c_s32 = eff == OUT_S32 || eff == OUT_S32_DUAL_ELU, dual = eff == OUT_S32_DUAL_ELU || eff == OUT_F32_AND_S32;
    const char* why = nullptr;
    if (dual && b.C2 < 0) why = "a dual output without a second buffer";
    else if (s32 && (!is_s32(b.A) || (b.A2 >= 0 && !is_s32(b.A2)))) why = "an S32 GEMM reads a buffer declared fp32";
    else if ((is_s32(b.C) != c_s32 || (dual && !is_s32(b.C2)))) why = "the output format disagrees with the buffer's declaration";
    if (why && !P->build_rc) {
        set_error("internal: GEMM step into '" + P->bufs[b.C].name + "': " + why);
        P->build_rc = WT_ERR_INVALID;
    }
    const int geom = b.mix_word >= 0 ? P->mix_geom : -1;
    P->step({geom, b.A, b.A2, b.C, b.C2}, [=](const RunCtx& c) {
        GemmArgs a = proto;
        a.A = P->ptr(c, b.A) + b.x_off; a.C = P->ptr(c, b.C);
        if (b.A2 >= 0) a.A2 = P->ptr(c, b.A2);
        if (b.C2 >= 0) a.C2 = P->ptr(c, b.C2);
        if (b.r_is_c) a.R = a.C;
        return dense(P, s32, a, pro, epi, out, c.stream, geom >= 0 ? reinterpret_cast<const int*>(P->ptr(c, geom)) + b.mix_word : nullptr);
    }, 1, name);
}

static GemmBufs in_place(int A, int C) { GemmBufs b{A, -1, C}; b.r_is_c = true; return b; }

static int copy_f32(float* dst, const float* src, size_t numel, hipStream_t s) {
    WT_HIP_CHECK(hipMemcpyAsync(dst, src, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
// A device-to-device copy as a step of its own: plan buffer to plan buffer, or (CALLER) from the call's input / into its output
constexpr int CALLER = -1;
static void copy_step(wt_plan* P, int src, int dst, size_t numel, const std::string& name = "") {
    P->step({src, dst}, [=](const RunCtx& c) {
        return copy_f32(dst == CALLER ? c.out_f : P->ptr(c, dst), src == CALLER ? c.in_f : P->ptr(c, src), numel, c.stream);
    }, 1, name);
}

// SConv1d geometry: sconv_geom (common.h, shared with the mixed-length geometry step)

// x [B][T][cin] (time-major) -> y [B][Tout][cout]; reflect-padded SConv1d as one implicit GEMM
GemmArgs sconv_args(const ConvW& w, int B, long T, int stride, int dil) {
    const SConvGeom g = sconv_geom(T, w.k, stride, dil);
    GemmArgs a;
    a.a_bstride = T * w.cin; a.a_rstride = w.cin;
    a.T_in = (int)T; a.T_out = g.Tout; a.Cin = w.cin; a.taps = w.k; a.stride = stride; a.dil = dil;
    a.pad_left = g.pl; a.pad_mode = PAD_REFLECT; a.Tp = g.Tp;
    a.W = w.w; a.w_rstride = (long)w.k * w.cin; a.bias = w.b;
    a.M = B * g.Tout; a.N = w.cout; a.K = w.k * w.cin;
    a.c_rstride = w.cout;
    set_s32(a, w.s32);
    return a;
}
// zero-padded 'same' Conv1d (decoder/models.py:29-43,177): k odd, padding (k-1)/2
GemmArgs zconv_args(const ConvW& w, int B, int L) {
    GemmArgs a;
    a.a_bstride = (long)L * w.cin; a.a_rstride = w.cin;
    a.T_in = L; a.T_out = L; a.Cin = w.cin; a.taps = w.k; a.pad_left = (w.k - 1) / 2; a.pad_mode = PAD_ZERO;
    a.W = w.w; a.w_rstride = (long)w.k * w.cin; a.bias = w.b;
    a.M = B * L; a.N = w.cout; a.K = w.k * w.cin; a.c_rstride = w.cout;
    set_s32(a, w.s32);
    return a;
}
// plain X[M][K] . W[N][K]^T
GemmArgs linear_args(const float* W, const float* bias, long M, int N, int K) {
    GemmArgs a;
    a.a_bstride = 0; a.a_rstride = K; a.T_in = (int)M; a.T_out = (int)M; a.Cin = K; a.taps = 1;
    a.W = W; a.w_rstride = K; a.bias = bias; a.M = (int)M; a.N = N; a.K = K; a.c_rstride = N;
    return a;
}
GemmArgs linear_args(const GemmW& W, const float* bias, long M, int N, int K) {
    GemmArgs a = linear_args(W.w, bias, M, N, K); set_s32(a, W.s32); return a;
}

// SEANetResnetBlock (seanet.py:62-63): y = shortcut(x) + conv1(elu(conv3(elu(x)))); returns y's buffer
static int plan_resblock(wt_plan* P, const ConvW& c3, const ConvW& c1, const ConvW& sc, int B, long T, int xin,
                         const std::string& name, bool elu_out = false, const wt_model* e0 = nullptr, long x_off = 0,
                         long x_bstride = 0, bool out_s32 = false, int mix_word = -1) {
    const int C = sc.cout;
    if (resblock_fusable(C) && !plan_unfused(P)) {
        // one fused kernel (resblock.hip); with e0 set, xin is unused and the tile is built from the waveform
        const int y = P->buf(name, (size_t)B * T * C, (out_s32 && !plan_fp32(P) ? BUF_S32 : BUF_F32) | (elu_out ? BUF_ELU : 0));
        const int geom = mix_word >= 0 ? P->mix_geom : -1;
        P->step({e0 ? -1 : xin, y, geom}, [=](const RunCtx& c) {
            ResblockArgs a{};
            ResblockMix mix;
            if (geom >= 0) mix.T = mix.Tread = reinterpret_cast<const int*>(P->ptr(c, geom)) + mix_word;
            a.x = e0 ? nullptr : P->ptr(c, xin) + x_off;
            a.x_bstride = x_bstride;
            a.wav = e0 ? c.in_f : nullptr;
            a.e0_w = e0 ? e0->e0_w : nullptr; a.e0_b = e0 ? e0->e0_b : nullptr;
            a.W3 = c3.w; a.b3 = c3.b; a.W1 = c1.w; a.b1 = c1.b; a.Ws = sc.w; a.bs = sc.b;
            a.y = P->ptr(c, y); a.B = B; a.T = (int)T; a.C = C; a.elu_out = elu_out ? 1 : 0;
            if (plan_fp32(P)) return launch_resblock(a, c.stream);
            a.out_s32 = out_s32 ? 1 : 0;
            return launch_resblock16(a, c.stream, geom >= 0 ? &mix : nullptr);
        }, 1, "resblock.fused");
        return y;
    }
    const int h = P->buf(name + ".h", (size_t)B * T * (C / 2));
    const int y = P->buf(name, (size_t)B * T * C, elu_out ? BUF_ELU : BUF_F32);
    GemmArgs a3 = sconv_args(c3, B, T, 1, 1), as = sconv_args(sc, B, T, 1, 1), a1 = sconv_args(c1, B, T, 1, 1);
    if (x_bstride) a3.a_bstride = as.a_bstride = x_bstride;
    a1.r_rstride = C;
    GemmBufs bx{xin, -1, h};
    bx.x_off = x_off;
    gemm_step(P, false, a3, bx, PRO_ELU, EPI_BIAS, OUT_F32);
    bx.C = y;
    gemm_step(P, false, as, bx, PRO_NONE, EPI_BIAS, OUT_F32);
    gemm_step(P, false, a1, in_place(h, y), PRO_ELU, elu_out ? EPI_BIAS_RES_ELU : EPI_BIAS_RES, OUT_F32);
    return y;
}

// The recurrence of an SLSTM, as every plan and wt_lstm_probe issue it: xg [L][B][4H] is the layer-0 input projection with both
// biases (time-major, packed gate order), x [B][L][H] the skip input, y [B][L][H] the output.  LSTM_PERSIST: one launch of
// lstm_persist_kernel, work = lstm_persist_hx_bytes() + lstm_persist_ctl_bytes() (filled with the exchange's marks here);
// LSTM_STEP_F16 / LSTM_STEP_F32: L + 1 launches of lstm_step_kernel, work = lstm_step_state_numel(B, H) floats (zeroed here):
// h0[2][H][Bp], h1[2][H][Bp], c0[B][H], c1[B][H] with the clip pitch Bp of the K-major hidden state
size_t lstm_step_state_numel(int B, int H) {
    const int Bp = (B + 63) / 64 * 64;
    return (size_t)4 * H * Bp + (size_t)2 * B * H;
}
int issue_lstm(const LstmW& w, const float* xg, const float* x, float* y, float* work, int B, int L, int H, bool elu_out,
               bool out_s32, int kernel, hipStream_t stream) {
    if (kernel == LSTM_PERSIST) {
        const size_t hxn = lstm_persist_hx_bytes() / sizeof(float), ctn = lstm_persist_ctl_bytes() / sizeof(float);
        if (int rc = launch_fill_u32(work, 0xFFFFFFFFu, (hxn + ctn) * sizeof(float), stream)) return rc;
        LstmPersistArgs pa;
        const int df_trace = [] { const char* e = lab_env("WT_LSTM_TRACE"); return e ? atoi(e) : 0; }();
        pa.data_flag = 1 | (df_trace ? 4 : 0);
        pa.xg0 = xg; pa.Wp = w.Wp; pa.b1 = w.b1; pa.x = x; pa.y = y;
        pa.hx = work; pa.ctl = reinterpret_cast<unsigned*>(work + hxn);
        pa.B = B; pa.L = L; pa.H = H; pa.Bx = (B + 7) / 8; pa.elu_out = elu_out ? 1 : 0; pa.out_s32 = out_s32 ? 1 : 0;
        return launch_lstm_persist(pa, stream);
    }
    const int Bp = (B + 63) / 64 * 64;
    if (int rc = launch_fill_u32(work, 0u, (lstm_step_state_numel(B, H) * sizeof(float) + 15) / 16 * 16, stream)) return rc;
    LstmArgs la;
    la.f16x3 = kernel == LSTM_STEP_F16 ? 1 : 0;     // recurrent product on split-f16 MFMAs unless fp32 is forced
    la.xg0 = xg; la.W0 = la.f16x3 ? w.W0h : w.W0; la.W1 = la.f16x3 ? w.W1h : w.W1; la.b1 = w.b1;
    la.h0 = work; la.h1 = work + (size_t)2 * H * Bp; la.c0 = work + (size_t)4 * H * Bp; la.c1 = la.c0 + (size_t)B * H;
    la.x = x; la.y = y; la.B = B; la.L = L; la.H = H; la.elu_out = elu_out ? 1 : 0;
    la.out_s32 = out_s32 ? 1 : 0;
    for (int t = 0; t <= L; ++t)
        if (int rc = launch_lstm_step(la, t, stream)) return rc;
    return 0;
}

// SLSTM (lstm.py:31-39) on x [B][L][H]; returns y = lstm(x) + x.  xin_s32 >= 0: an S32 copy of x for the input
// projection (split-f16 GEMM); y_s32: write y in S32 (its only consumer is a split-f16 conv).
static int plan_lstm(wt_plan* P, const LstmW& w, int B, int L, int H, int xin, const std::string& name,
                     bool elu_out = false, int xin_s32 = -1, bool y_s32 = false) {
    const int xg = P->buf(name + ".xg", (size_t)B * L * 4 * H);
    const int st = P->buf(name + ".state", lstm_step_state_numel(B, H));      // h0[2][H][Bp], h1[2][H][Bp], c0[B][H], c1[B][H]
    const int y = P->buf(name, (size_t)B * L * H, (y_s32 ? BUF_S32 : BUF_F32) | (elu_out ? BUF_ELU : 0));
    // input projection written time-major ([L][B][4H]) so each recurrent step reads one contiguous
    // slab: the gather treats a time step as the "clip" (stride H) and the clip as the row (stride L*H)
    GemmArgs ax = linear_args(w.Wih0, w.b0, (long)B * L, 4 * H, H);
    ax.T_in = B; ax.T_out = B; ax.a_bstride = H; ax.a_rstride = (long)L * H;
    const int xsrc = xin_s32 >= 0 ? xin_s32 : xin;
    gemm_step(P, xin_s32 >= 0, ax, {xsrc, -1, xg}, PRO_NONE, EPI_BIAS, OUT_F32);
    // one persistent launch for the whole recurrence (lstm_persist.hip) when the batch fits its per-XCD clip groups and
    // the device is a full MI355X (256 CUs: one resident workgroup per CU, 32 per XCD)
    const bool persist_env = [] { const char* e = lab_env("WT_LSTM_PERSIST"); return !e || e[0] != '0'; }();       // (LAB builds; callers use WT_PLAN_FLAG_STEP_LSTM)
    const bool persist = persist_env && !plan_fp32(P) && !(P->flags & WT_PLAN_FLAG_STEP_LSTM) && w.Wp && H == 512 && B <= 128 && L < 65536 &&
                         full_chip(P->model->device);
    if (persist) P->uses_persist = true;
    const size_t hxn = lstm_persist_hx_bytes() / sizeof(float), ctn = lstm_persist_ctl_bytes() / sizeof(float);
    const int hx = persist ? P->buf(name + ".hx", hxn + ctn) : -1;
    const int kernel = plan_fp32(P) ? LSTM_STEP_F32 : LSTM_STEP_F16;
    P->step({xin, xg, st, hx, y}, [=](const RunCtx& c) {
        const bool now_persist = persist && P->model->persist_ok.load();
        return issue_lstm(w, P->ptr(c, xg), P->ptr(c, xin), P->ptr(c, y), now_persist ? P->ptr(c, hx) : P->ptr(c, st), B, L, H,
                          elu_out, y_s32, now_persist ? LSTM_PERSIST : kernel, c.stream);
    }, L + 2);
    return y;
}

// Unfused SEANetResnetBlock with every operand pre-split: x arrives as S32(x) (shortcut) and S32(elu(x)) (conv3),
// the hidden activation and the output are written as S32(elu(.)); returns the output buffer, or -1 (set_error)
static int plan_resblock_s32(wt_plan* P, const ConvW& c3, const ConvW& sc, const ConvW& cat, int B, long T, int x_raw,
                             int x_elu, const std::string& name, long x_off = 0, long x_bstride = 0, int mix_word = -1) {
    if (!cat.s32.p) { set_error("internal: unfused S32 resblock without an S32 shortcut + conv1 weight"); return -1; }
    const int C = sc.cout;
    const int h = P->buf(name + ".h", (size_t)B * T * (C / 2), BUF_S32 | BUF_ELU);
    GemmArgs a3 = sconv_args(c3, B, T, 1, 1);
    GemmBufs b3{x_elu, -1, h};
    b3.x_off = x_off; b3.mix_word = mix_word >= 0 ? mix_word + GEOM_C3 : -1;
    if (x_bstride) a3.a_bstride = x_bstride;
    gemm_step(P, true, a3, b3, PRO_NONE, EPI_BIAS_ELU, OUT_S32);
    // shortcut + conv1 as one GEMM over K = [x (C) | elu(h) (C/2)] (GemmArgs::A2, weight `cat`: weights.cpp build_cat): the
    // fp32 shortcut tensor is neither written nor read back, and the output goes through the staged full-line epilogue
    const int o = P->buf(name, (size_t)B * T * C, BUF_S32 | BUF_ELU);
    GemmArgs ac = sconv_args(sc, B, T, 1, 1);
    ac.W = cat.w; ac.w_rstride = cat.cin; ac.bias = cat.b; ac.K = cat.cin; ac.Cin = cat.cin;
    set_s32(ac, cat.s32);
    ac.K1 = C; ac.a2_bstride = T * (C / 2); ac.a2_rstride = C / 2;
    if (x_bstride) ac.a_bstride = x_bstride;
    GemmBufs bc{x_raw, h, o};
    bc.x_off = x_off; bc.mix_word = mix_word >= 0 ? mix_word + GEOM_SC : -1;
    gemm_step(P, true, ac, bc, PRO_NONE, EPI_BIAS_ELU, OUT_S32);
    return o;
}

// Greedy residual VQ (core_vq.py:403-413) on the rows x [B * L][512] (fp32; xs: their S32 form when the distance GEMMs run on
// gemm16s.hip): the plan holds num_quantizers rounds and a call launches the first RunCtx::n_q.  Round k: distance GEMM
// against codebook k with the argmax epilogue, then vq_residual (code row k, r -= E_k[code], its S32 form and |r|^2 for the
// next GEMM); the call's last round needs the codes only and ends in vq_finalize.  Round 0 reads x, writes vq.r; the later
// rounds update vq.r in place.  Codes [n_q][B][L]; geom >= 0 (mixed-length): every row is -1 past a clip's frames.
static int plan_rvq_rounds(wt_plan* P, int x, int xs, bool s32, int geom, int l_word) {
    const wt_model* M = P->model;
    const int B = P->B, L = (int)P->L, bins = M->arch.vq_bins, D = M->embed.cols, nq = M->arch.num_quantizers;
    const long rows = (long)B * L;
    const int np = s32 ? gemm16s_vq_parts(bins) : gemm_vq_parts(bins);
    const int xx = P->buf("vq.xx", (size_t)rows);
    const int pv = P->buf("vq.pval", (size_t)rows * np);
    const int pi = P->buf("vq.pidx", (size_t)rows * np);
    const int r = nq > 1 ? P->buf("vq.r", (size_t)rows * D) : -1;
    const int rs = nq > 1 && s32 ? P->buf("vq.r.s32", (size_t)rows * D, BUF_S32) : -1;
    P->n_codes = rows;                   // per round: the guard step takes the call's n_q (plan_end)
    P->step({x, xx}, [=](const RunCtx& c) { return launch_row_sumsq(P->ptr(c, x), P->ptr(c, xx), rows, D, c.stream); });
    for (int k = 0; k < nq; ++k) {
        GemmW W;
        W.w = M->embed.w + (size_t)k * bins * D; W.rows = bins; W.cols = D;
        W.s32 = k ? M->rvq.s32[k - 1] : M->embed.s32;
        const float* ee = k ? M->rvq.ee[k - 1] : M->ee;
        const GemmArgs av = linear_args(W, nullptr, rows, bins, D);
        const int a_f = k ? r : x, a_s = k ? rs : xs;
        const std::string tag = k ? "." + std::to_string(k) : "";
        P->step({a_f, s32 ? a_s : -1, xx, pv, pi}, [=](const RunCtx& c) {
            if (k >= c.n_q) return 0;
            GemmArgs a = av; a.A = P->ptr(c, s32 ? a_s : a_f);
            a.vq_xx = P->ptr(c, xx); a.vq_ee = ee; a.vq_pval = P->ptr(c, pv);
            a.vq_pidx = reinterpret_cast<int*>(P->ptr(c, pi)); a.vq_nparts = np;
            return dense(P, s32, a, PRO_NONE, EPI_ARGMAX, OUT_F32, c.stream);
        }, 1, "vq.argmin" + tag);
        P->step({geom, pv, pi, a_f, r, rs, xx}, [=](const RunCtx& c) {
            if (k >= c.n_q) return 0;
            int64_t* codes = c.codes + (long)k * rows;
            const float* pval = P->ptr(c, pv);
            const int* pidx = reinterpret_cast<const int*>(P->ptr(c, pi));
            int rc;
            if (k == c.n_q - 1) rc = launch_vq_finalize(pval, pidx, np, W.w, codes, nullptr, B, L, D, bins, c.stream);
            else rc = launch_vq_residual(pval, pidx, np, P->ptr(c, a_f), W.w, codes, P->ptr(c, r), rs >= 0 ? P->ptr(c, rs) : nullptr,
                                         P->ptr(c, xx), rows, D, bins, c.stream);
            if (!rc && geom >= 0)
                rc = launch_mixed_pad(reinterpret_cast<const int*>(P->ptr(c, geom)), l_word, codes, nullptr, nullptr, B, L, 1, c.stream);
            return rc;
        }, geom >= 0 ? 2 : 1, (k == nq - 1 ? "vq.finalize" : "vq.residual") + tag);
    }
    return 0;
}

// the checks the two residual VQ plan shapes share, and the tables of codebooks 1 .. num_quantizers - 1 (weights.cpp)
static int rvq_prepare(const wt_plan* P) {
    const wt_model* M = P->model;
    if (M->arch.input_channels != M->embed.cols || M->enc_final.cout != M->embed.cols) {
        set_error("residual VQ plans need input_channels and the encoder width equal to the codebook width"); return WT_ERR_INVALID;
    }
    if ((long)P->B * P->L >= (long)INT_MAX) { set_error("batch too large for one residual VQ plan (32-bit frame index)"); return WT_ERR_INVALID; }
    return ensure_rvq_tables(M);
}

// WT_PLAN_QUANTIZE: features (B, 512, L) fp32 -> codes (n_q, B, L): transpose to rows, split, |x|^2, then the rounds
int build_quantize(wt_plan* P) {
    const wt_model* M = P->model;
    if (int rc = rvq_prepare(P)) return rc;
    const int B = P->B, L = (int)P->L, D = M->embed.cols;
    const long rows = (long)B * L;
    const bool s32 = plan_s32(P) && M->embed.s32.p && M->rvq.s32_ok;
    const int x = P->buf("vq.in", (size_t)rows * D);
    const int xs = s32 ? P->buf("vq.in.s32", (size_t)rows * D, BUF_S32) : -1;
    P->step({x}, [=](const RunCtx& c) { return launch_transpose(c.in_f, P->ptr(c, x), B, D, L, c.stream); });
    if (s32) P->step({x, xs}, [=](const RunCtx& c) { return launch_split_s32(P->ptr(c, x), P->ptr(c, xs), rows * D, c.stream); });
    return plan_rvq_rounds(P, x, xs, s32, -1, 0);
}

int build_encode(wt_plan* P) {
    const wt_model* M = P->model;
    const int B = P->B;
    const long T = P->T;
    const bool rvq = P->flags & WT_PLAN_FLAG_RVQ;
    if (rvq) if (int rc = rvq_prepare(P)) return rc;
    // the first conv is folded into the fused stage-1 resblock unless stage taps are kept
    const bool fold_e0 = !plan_unfused(P) && !M->stages.empty() && M->stages[0].C == 32 &&
                         M->e0_k == 7 && resblock_fusable(32);
    int x = -1;
    if (!fold_e0) {
        x = P->buf("enc.0", (size_t)B * T * M->e0_c);
        const int x0 = x;
        P->step({x0}, [=](const RunCtx& c) {
            return launch_conv_first(c.in_f, M->e0_w, M->e0_b, P->ptr(c, x0), B, T, M->e0_k, M->e0_c, c.stream);
        });
    }
    // ELU is applied once by the producer wherever its only consumer is "ELU -> conv" (resblock
    // output -> down conv, LSTM output -> last conv); the unfused debug plan keeps raw tensors instead
    const bool fuse_elu = !plan_unfused(P);
    // S32 mode (default): from the first fused stage on, every GEMM operand of the encoder is written pre-split by
    // its producer and multiplied by gemm16s.hip; tensors that fp32 kernels read too (fused resblock input, LSTM
    // skip, embeddings) are written in both forms by the producing GEMM
    const bool s32 = plan_s32(P);
    // Route of every stage, decided before any step is added: the fused resblock kernel or the unfused GEMMs, the down conv
    // folded into the fused kernel or not, and whether the stage's GEMMs take S32 operands
    struct Route { bool fused, down, s32; };
    std::vector<Route> route(M->stages.size());
    for (size_t si = 0; si < route.size(); ++si) {
        const ResStage& st = M->stages[si];
        Route& r = route[si];
        r.fused = resblock_fusable(st.C) && !plan_unfused(P);
        // a fused stage only needs the S32 down-conv weights (its own convs run inside resblock16); an unfused one
        // needs S32 copies of all four, and its input in S32 from the stage before
        r.s32 = s32 && st.C % 32 == 0 && st.down.s32.p &&
                (r.fused || (si > 0 && route[si - 1].s32 && st.c3.s32.p && st.c1.s32.p && st.sc.s32.p));
        // stage 1 of the shipped plan: first conv + resblock + ELU + down conv in ONE kernel, the stage's activations never
        // leave LDS (resblock16.hip, DOWN)
        r.down = si == 0 && fold_e0 && r.fused && r.s32 && route.size() > 1 && resblock_fusable(M->stages[1].C) &&
                 st.down.cin == 32 && st.down.cout == 64 && resblock16_down_fusable(st.C, T, st.r, st.down.k);
    }
    // after the last stage the LSTM reads fp32 (skip) and, on S32 operands, an S32 copy (input projection)
    const bool lstm_s32 = !route.empty() && route.back().s32 && M->enc_lstm.Wih0.s32.p;
    const bool tail_s32 = lstm_s32 && M->enc_final.s32.p && M->embed.s32.p;
    // Mixed-length plan (WT_PLAN_FLAG_MIXED_LENGTH): T is the padded length, every clip brings its own.  Only the shipped route
    // takes per-clip lengths (stage 1 fused with its down conv, the 64-channel fused resblock, S32 GEMMs everywhere else)
    const bool mixed = P->flags & WT_PLAN_FLAG_MIXED_LENGTH;
    const int n_st = (int)route.size();
    int geom = -1;
    if (mixed) {
        bool ok = s32 && !(P->flags & (WT_PLAN_FLAG_KEEP_STAGES | WT_PLAN_FLAG_RANGE_REPORT)) && tail_s32 &&
                  n_st >= 2 && n_st <= GEOM_MAX_STAGES && route[0].down;
        for (int si = 1; si < n_st && ok; ++si)
            ok = route[si].s32 && (route[si].fused ? M->stages[si].C == 64 : M->stages[si].cat.s32.p != nullptr);
        for (const ResStage& st : M->stages) ok = ok && st.c3.k == 3 && st.sc.k == 1;     // (the geometry step's k3 / 1x1 convs)
        if (!ok) {
            set_error("mixed-length plans run only the shipped split-f16 encoder route: not with WT_PLAN_FLAG_UNFUSED, "
                      "FP32_GEMM, KEEP_STAGES or RANGE_REPORT, an encoder range site on fp32, weights without S32 copies, or a first "
                      "encoder ratio other than 2 or 4 (no stage-1 kernel with the down conv)");
            return WT_ERR_INVALID;
        }
        P->min_clip = 1024;              // resblock16_down_fusable: the fused stage-1 kernel's shortest clip
        if (T < P->min_clip) { set_error("mixed-length plans need a padded length of at least 1024 samples"); return WT_ERR_INVALID; }
        geom = P->mix_geom = P->buf("mix.geom", (size_t)B * GEOM_WORDS);
        std::vector<int> kd, rd;
        for (const ResStage& st : M->stages) { kd.push_back(st.down.k); rd.push_back(st.r); }
        const int kf = M->enc_final.k;
        const int tmin = (int)P->min_clip;
        P->step({geom}, [=](const RunCtx& c) {
            return launch_mixed_geometry(c.lengths, reinterpret_cast<int*>(P->ptr(c, geom)), B, T, tmin, n_st, kd.data(),
                                         rd.data(), kf, c.stream);
        }, 1, "mix.geom");
    }
    auto mix_ptr = [=](const RunCtx& c, int word) { return reinterpret_cast<const int*>(P->ptr(c, geom)) + word; };
    long Tc = T;
    int idx = 1;
    int x_elu = -1;                      // S32(elu(x)) beside S32(x) for an unfused S32 stage
    int x_s32 = -1;                      // S32 copy of the last down conv output (LSTM input projection)
    for (size_t si = 0; si < route.size(); ++si) {
        const ResStage& st = M->stages[si];
        const Route r = route[si];
        const bool last = si + 1 == route.size();
        GemmArgs ad = sconv_args(st.down, B, Tc, st.r, 1);
        const size_t ynum = (size_t)B * ad.T_out * st.down.cout;
        const std::string out = "enc." + std::to_string(idx + 2);
        if (r.down) {
            const int y = P->buf(out, ynum);
            P->step({-1, y, geom}, [=](const RunCtx& c) {
                ResblockArgs a{};
                ResblockMix mix;
                if (geom >= 0) { mix.T = mix_ptr(c, GEOM_T); mix.Tread = mix_ptr(c, GEOM_TREAD); }
                a.wav = c.in_f; a.e0_w = M->e0_w; a.e0_b = M->e0_b;
                a.W3 = st.c3.w; a.b3 = st.c3.b; a.W1 = st.c1.w; a.b1 = st.c1.b; a.Ws = st.sc.w; a.bs = st.sc.b;
                a.Wd = st.down.w; a.bd = st.down.b; a.y_down = P->ptr(c, y); a.R = st.r;
                a.B = B; a.T = (int)Tc; a.C = st.C;
                return launch_resblock16_down(a, c.stream, geom >= 0 ? &mix : nullptr);
            }, 1, "resblock.fused_down");
            x = y; Tc = ad.T_out; idx += 3;
            continue;
        }
        const std::string name = "enc." + std::to_string(idx);
        const int stage_word = GEOM_STAGE0 + (int)si * GEOM_STAGE_WORDS;     // (mixed-length plans)
        if (r.fused)
            x = plan_resblock(P, st.c3, st.c1, st.sc, B, Tc, x, name, fuse_elu, (si == 0 && fold_e0) ? M : nullptr, 0, 0, r.s32,
                              mixed ? stage_word + GEOM_C3 : -1);
        else if (r.s32)
            x = plan_resblock_s32(P, st.c3, st.sc, st.cat, B, Tc, x, x_elu, name, 0, 0, mixed ? stage_word : -1);
        else
            x = plan_resblock(P, st.c3, st.c1, st.sc, B, Tc, x, name, fuse_elu);
        if (x < 0) return WT_ERR_INVALID;
        // what the next consumer wants: a fused resblock reads fp32, an unfused S32 stage S32 raw + S32 elu
        const bool next_s32 = !last && !route[si + 1].fused && route[si + 1].s32;
        const int y = P->buf(out, ynum, next_s32 ? BUF_S32 : BUF_F32);
        const int y2 = (next_s32 || (last && lstm_s32)) ? P->buf(out + ".s32", ynum, BUF_S32 | (next_s32 ? BUF_ELU : 0)) : -1;
        GemmBufs bd{x, -1, y, y2};
        bd.mix_word = mixed ? stage_word + GEOM_DOWN : -1;
        gemm_step(P, r.s32, ad, bd, fuse_elu ? PRO_NONE : PRO_ELU, EPI_BIAS,
                  next_s32 ? OUT_S32_DUAL_ELU : (y2 >= 0 ? OUT_F32_AND_S32 : OUT_F32));
        if (next_s32) x_elu = y2;
        if (last) x_s32 = y2;
        x = y; Tc = ad.T_out; idx += 3;
    }
    const int L = (int)Tc;
    if (L != P->L) { set_error("internal: frame count mismatch"); return WT_ERR_INVALID; }
    P->n_codes = (long)B * L; P->n_out = P->n_aux = (long)B * 512 * L;
    const int H = M->H;
    x = plan_lstm(P, M->enc_lstm, B, L, H, x, "enc." + std::to_string(idx), fuse_elu, x_s32, tail_s32);
    GemmArgs af = sconv_args(M->enc_final, B, L, 1, 1);
    const int emb = P->buf("enc." + std::to_string(idx + 2), (size_t)B * L * 512);
    const int emb_s32 = tail_s32 ? P->buf("enc." + std::to_string(idx + 2) + ".s32", (size_t)B * L * 512, BUF_S32) : -1;
    GemmBufs bf{x, -1, emb, emb_s32};
    bf.mix_word = mixed ? geom_final(n_st) : -1;
    gemm_step(P, tail_s32, af, bf, fuse_elu ? PRO_NONE : PRO_ELU, EPI_BIAS, OUT_F32_AND_S32);
    // ---- residual VQ with the call's n_q codebooks (WT_PLAN_FLAG_RVQ: codes alone, no features, no emb_out)
    if (rvq) {
        P->n_out = P->n_aux = 0;
        return plan_rvq_rounds(P, emb, emb_s32, tail_s32 && M->rvq.s32_ok, geom, geom_L(n_st));
    }
    // ---- VQ (core_vq.py:175-183, 206-231)
    const int bins = M->arch.vq_bins;
    GemmArgs av = linear_args(M->embed, nullptr, (long)B * L, bins, 512);
    // the argmax epilogue leaves one (value, index) candidate per wave column slab; their number depends on
    // which kernel the distance GEMM runs on
    const int np = tail_s32 ? gemm16s_vq_parts(bins) : gemm_vq_parts(bins);
    const int xx = P->buf("vq.xx", (size_t)B * L);
    const int pv = P->buf("vq.pval", (size_t)B * L * np);
    const int pi = P->buf("vq.pidx", (size_t)B * L * np);
    P->step({emb, xx}, [=](const RunCtx& c) { return launch_row_sumsq(P->ptr(c, emb), P->ptr(c, xx), (long)B * L, 512, c.stream); });
    P->step({emb, emb_s32, xx, pv, pi}, [=](const RunCtx& c) {
        GemmArgs a = av; a.A = P->ptr(c, tail_s32 ? emb_s32 : emb);
        a.vq_xx = P->ptr(c, xx); a.vq_ee = M->ee; a.vq_pval = P->ptr(c, pv);
        a.vq_pidx = reinterpret_cast<int*>(P->ptr(c, pi)); a.vq_nparts = np;
        return dense(P, tail_s32, a, PRO_NONE, EPI_ARGMAX, OUT_F32, c.stream);
    }, 1, "vq.argmin");
    P->step({geom, pv, pi, emb}, [=](const RunCtx& c) {
        if (int rc = launch_vq_finalize(P->ptr(c, pv), reinterpret_cast<int*>(P->ptr(c, pi)), np, M->embed.w, c.codes,
                                        c.out_f, B, L, 512, bins, c.stream)) return rc;
        if (c.aux) if (int rc = launch_transpose(P->ptr(c, emb), c.aux, B, L, 512, c.stream)) return rc;
        // mixed-length plans: codes -1 and features (and emb_out) 0 past each clip's L; -1 / NaN for an invalid length
        if (geom >= 0) return launch_mixed_pad(mix_ptr(c, 0), geom_L(n_st), c.codes, c.out_f, c.aux, B, L, 512, c.stream);
        return 0;
    }, mixed ? 3 : 2);
    return 0;
}

// ISTFTHead (heads.py:53-66) on the backbone output xo [M][dim] (S32 when s32): Linear + exp/clip/cos/sin fused ->
// spectrum rows [re | im]; ISTFT (spectral_ops.py:56-73) as four quarter-size real transforms (one batched GEMM), then
// the butterflies + window + overlap-add + trim + envelope divide in one pass into the caller's audio buffer
static void plan_head(wt_plan* P, int xo, bool s32, bool mixed = false) {
    const wt_model* M = P->model;
    const wt_arch& ar = M->arch;
    const int B = P->B, L = (int)P->L, D = ar.dim;
    const long Mrows = (long)B * L;
    const int Kb = M->Kb, hop = ar.hop_length;
    const int spec = P->buf("head.spec", (size_t)Mrows * 2 * Kb, s32 ? BUF_S32 : BUF_F32);
    GemmArgs ah = linear_args(M->head_W, M->head_b, Mrows, 2 * Kb, D);
    ah.c_rstride = 2 * Kb; ah.head_kb = Kb;
    gemm_step(P, s32, ah, {xo, -1, spec}, PRO_NONE, EPI_HEAD, OUT_S32, "head.out");        // spectrum pre-split for the ISTFT GEMM
    const int Kq = M->Kq;
    const int parts = P->buf("head.parts", (size_t)4 * Mrows * Kq);       // Ce, Co, Se, So: [4][M][Kq]
    GemmArgs ai = linear_args(M->istft_W, nullptr, Mrows, Kq, Kq);
    ai.a_rstride = 2 * Kb; ai.zA = Kq;              // z picks the spectrum quarter
    ai.zW = (long)Kq * Kq; ai.nz = 4;
    ai.c_rstride = Kq; ai.zC = (long)Mrows * Kq;
    gemm_step(P, s32, ai, {spec, -1, parts}, PRO_NONE, EPI_BIAS, OUT_F32, "head.istft");
    P->step({parts}, [=](const RunCtx& c) {
        return launch_istft_ola(P->ptr(c, parts), M->win, M->wsq, c.out_f, B, L, ar.n_fft, hop, Kq, ar.padding_same ? 0 : 1, c.stream,
                                mixed ? c.lengths : nullptr);
    }, 1, "head.ola");
}

int build_decode(wt_plan* P) {
    const wt_model* M = P->model;
    const wt_arch& ar = M->arch;
    const int B = P->B, L = (int)P->L, D = ar.dim, I = ar.intermediate_dim, Cin = ar.input_channels;
    const long Mrows = (long)B * L;
    const int Lp = ((L + 31) / 32) * 32;
    P->n_out = B * wave_samples(M, L); P->n_aux = Mrows * D;
    // S32 mode: every operand of the dense chain is written pre-split by its producer (transpose, norm kernels,
    // GELU / head epilogues) and multiplied by gemm16s.hip; the residual stream and the norm inputs stay fp32
    const bool s32_plan = plan_s32(P) && (Cin % 32 == 0) && (D % 32 == 0) && (I % 32 == 0);
    // ... site by site (model.h Site): a site listed in fp32_sites keeps fp32 operands and runs its GEMMs on gemm.hip
    auto s32_at = [&](int site) { return s32_plan && !site_fp32(P, site); };
    P->cur_site = SITE_BB_EMBED;
    const bool s32_e = s32_at(SITE_BB_EMBED);
    // Mixed-length plan (WT_PLAN_DECODE_MIXED): L is the padded length, every clip brings its own (RunCtx::lengths).  The GEMMs run
    // at (B, L) as they are: they are row-independent, and the steps that reduce over time (GroupNorm, softmax, the dwconv's
    // taps, the overlap-add) read each clip's length and leave zeros in its rows past it, which stand for the zero padding of
    // the convs and add exact zeros to the attention output.  Only the shipped split-f16 route takes lengths
    const bool mixed = P->kind == WT_PLAN_DECODE_MIXED || P->kind == WT_PLAN_DECODE_CODES_MIXED;
    // Decode from codes (WT_PLAN_DECODE_CODES / _MIXED): the first step gathers the codebook rows of the call's codes into bb.in
    // (code_rows) instead of transposing the call's features into it; nothing else in the chain changes
    const bool from_codes = P->kind == WT_PLAN_DECODE_CODES || P->kind == WT_PLAN_DECODE_CODES_MIXED;
    if (from_codes && Cin != M->embed.cols) {
        set_error("decode-from-codes plans need input_channels equal to the codebook width"); return WT_ERR_INVALID;
    }
    if (from_codes && Mrows >= (long)INT_MAX) {      // (code_rows runs one wave per frame under a 32-bit frame index)
        set_error("batch too large for one decode-from-codes plan (32-bit frame index)"); return WT_ERR_INVALID;
    }
    if (mixed) {
        const bool ok = s32_plan && !P->fp32_sites && !(P->flags & (WT_PLAN_FLAG_KEEP_STAGES | WT_PLAN_FLAG_RANGE_REPORT)) &&
                        M->at_Wqk.s32.p && M->at_Wv.s32.p && M->at_Wp.s32.p;
        if (!ok) {
            set_error("mixed-length plans run only the shipped split-f16 decoder route: not with WT_PLAN_FLAG_UNFUSED, "
                      "FP32_GEMM, KEEP_STAGES or RANGE_REPORT, a decoder range site on fp32, or weights without S32 copies");
            return WT_ERR_INVALID;
        }
        const int ctl = P->ctl;
        P->step({ctl}, [=](const RunCtx& c) {
            return launch_mixed_check_lengths(c.lengths, B, L, reinterpret_cast<unsigned*>(P->ptr(c, ctl)), c.stream);
        }, 1, "mix.lengths");
    }
    auto lens = [mixed](const RunCtx& c) { return mixed ? c.lengths : nullptr; };
    const int x0 = P->buf("bb.in", (size_t)Mrows * Cin, s32_e ? BUF_S32 : BUF_F32);
    const int bins = ar.vq_bins;
    if (from_codes)
        P->step({x0}, [=](const RunCtx& c) {
            return launch_code_rows(c.in_codes, M->embed.w, c.n_q, bins, B, L, Cin, P->ptr(c, x0), c.stream, s32_e, M->bad_codes_dev, lens(c));
        }, 1, "code_rows");
    else
        P->step({x0}, [=](const RunCtx& c) { return launch_transpose(c.in_f, P->ptr(c, x0), B, Cin, L, c.stream, s32_e, lens(c)); });
    const int x = P->buf("bb.x", (size_t)Mrows * D);       // residual stream, updated in place
    gemm_step(P, s32_e, zconv_args(M->bb_embed, B, L), {x0, -1, x}, PRO_NONE, EPI_BIAS, OUT_F32);
    const bool keep = P->flags & WT_PLAN_FLAG_KEEP_STAGES;
    auto snapshot = [&](int src, const std::string& name) {   // WT_PLAN_FLAG_KEEP_STAGES: debug taps of the in-place residual streams
        if (keep) copy_step(P, src, P->buf(name, (size_t)Mrows * D), (size_t)Mrows * D);
    };
    snapshot(x, "bb.embed");
    const int sc = P->buf("bb.gn_scale", (size_t)B * D), sh = P->buf("bb.gn_shift", (size_t)B * D);
    const int gp = P->buf("bb.gn_part", gn_part_floats(B, L, 32));       // chunk statistics (long clips)
    const int h1 = P->buf("bb.h1", (size_t)Mrows * D, s32_plan ? BUF_S32 : BUF_F32);
    const int h2 = P->buf("bb.h2", (size_t)Mrows * D);

    // ResnetBlock (models.py:58-78).  GroupNorm+swish is applied ONCE per element by the statistics
    // kernel (a second pass over its own L x 24 slab) instead of in the conv's operand staging,
    // where every element would be re-normalised by each of the 18 (tap, column-tile) re-reads.
    auto resnet = [&](const PosRes& r, const std::string& name, int site) {
        P->cur_site = site;
        const bool s32 = s32_at(site);
        P->bufs[h1].fmt = s32 ? BUF_S32 : BUF_F32;         // (h1 is shared by the sites; the range report reads the format per step)
        P->step({x, sc, sh, h1, gp}, [=](const RunCtx& c) {
            return launch_gn_apply(P->ptr(c, x), r.n1w, r.n1b, P->ptr(c, sc), P->ptr(c, sh), P->ptr(c, h1), 1, B, L, D, 32, 1e-6f, c.stream, s32, P->ptr(c, gp), lens(c));
        }, 1, "res.gn1");
        gemm_step(P, s32, zconv_args(r.c1, B, L), {h1, -1, h2}, PRO_NONE, EPI_BIAS, OUT_F32, "res.conv1");
        P->step({h2, sc, sh, h1, gp}, [=](const RunCtx& c) {
            return launch_gn_apply(P->ptr(c, h2), r.n2w, r.n2b, P->ptr(c, sc), P->ptr(c, sh), P->ptr(c, h1), 1, B, L, D, 32, 1e-6f, c.stream, s32, P->ptr(c, gp), lens(c));
        }, 1, "res.gn2");
        GemmArgs a2 = zconv_args(r.c2, B, L);
        a2.r_rstride = D;
        gemm_step(P, s32, a2, in_place(h1, x), PRO_NONE, EPI_BIAS_RES, OUT_F32, "res.conv2");
        snapshot(x, name);
    };
    resnet(M->res[0], "bb.pos_net.0", SITE_RES0);
    resnet(M->res[1], "bb.pos_net.1", SITE_RES1);
    {   // AttnBlock (models.py:107-127), single head of width D.  On S32 operands every product runs on split-f16 MFMAs:
        // the normalised input, q | k, V^T, the probabilities and the attention output are written pre-split by their
        // producers.  On fp32 operands softmax turns the scores into probabilities in place.
        P->cur_site = SITE_ATTN;
        const bool s32 = s32_at(SITE_ATTN) && M->at_Wqk.s32.p && M->at_Wv.s32.p && M->at_Wp.s32.p;
        const int fmt = s32 ? BUF_S32 : BUF_F32;
        P->bufs[h1].fmt = fmt;
        const int qk = P->buf("bb.attn.qk", (size_t)Mrows * 2 * D, fmt);             // [M][q | k]
        const int vt = P->buf("bb.attn.vt", (size_t)B * D * Lp, fmt);                 // [B][D][Lp]
        const int S = P->buf("bb.attn.s", (size_t)Mrows * Lp);                        // fp32 scores
        const int Ps = s32 ? P->buf("bb.attn.p", (size_t)Mrows * Lp, BUF_S32) : S;    // probabilities
        const int o = P->buf("bb.attn.o", (size_t)Mrows * D, fmt);
        P->step({x, sc, sh, gp, h1}, [=](const RunCtx& c) {
            return launch_gn_apply(P->ptr(c, x), M->at_nw, M->at_nb, P->ptr(c, sc), P->ptr(c, sh), P->ptr(c, h1), 0, B, L, D, 32, 1e-6f, c.stream, s32, P->ptr(c, gp), lens(c));
        }, 1, "attn.gn");
        gemm_step(P, s32, linear_args(M->at_Wqk, M->at_bqk, Mrows, 2 * D, D), {h1, -1, qk}, PRO_NONE, EPI_BIAS, OUT_S32, "attn.qk");
        P->step({h1, vt}, [=](const RunCtx& c) {     // V^T[b] = Wv . hn[b]^T + bv   (D x L, pitch Lp; pad columns stay zero)
            if (int rc = launch_fill_u32(P->ptr(c, vt), 0u, (size_t)B * D * Lp * sizeof(float), c.stream)) return rc;
            GemmArgs a = linear_args(nullptr, M->at_bv, D, L, D);
            a.A = s32 ? static_cast<const float*>(M->at_Wv.s32.p) : M->at_Wv.w; a.acc_scale = M->at_Wv.s32.acc_scale; a.zA = 0;
            a.zW = (long)L * D; a.nz = B;
            a.C = P->ptr(c, vt); a.c_rstride = Lp; a.zC = (long)D * Lp;
            return dense_act(P, s32, a, P->ptr(c, h1), EPI_BIAS_ROW, OUT_S32, c.stream);
        }, 2, "attn.vt");
        P->step({qk, S}, [=](const RunCtx& c) {      // S[b] = q[b] . k[b]^T * D^-0.5
            GemmArgs a = linear_args(nullptr, nullptr, L, L, D);
            a.A = P->ptr(c, qk); a.a_rstride = 2 * D; a.zA = (long)L * 2 * D;
            a.w_rstride = 2 * D; a.zW = (long)L * 2 * D; a.nz = B;
            a.C = P->ptr(c, S); a.c_rstride = Lp; a.zC = (long)L * Lp;
            a.alpha = (float)std::pow((double)D, -0.5);
            return dense_act(P, s32, a, P->ptr(c, qk) + D, EPI_SCALE, OUT_F32, c.stream);
        }, 1, "attn.s");
        P->step({S, Ps}, [=](const RunCtx& c) { return launch_softmax(P->ptr(c, S), (int)Mrows, L, Lp, c.stream, s32 ? P->ptr(c, Ps) : nullptr, lens(c)); });
        P->step({Ps, vt, o}, [=](const RunCtx& c) {  // O[b] = P[b] . V[b]
            GemmArgs a = linear_args(nullptr, nullptr, L, D, Lp);
            a.A = P->ptr(c, Ps); a.zA = (long)L * Lp;
            a.zW = (long)D * Lp; a.nz = B;
            a.C = P->ptr(c, o); a.c_rstride = D; a.zC = (long)L * D;
            return dense_act(P, s32, a, P->ptr(c, vt), EPI_BIAS, OUT_S32, c.stream);
        }, 1, "attn.o");
        GemmArgs ap = linear_args(M->at_Wp, M->at_bp, Mrows, D, D);
        ap.r_rstride = D;
        gemm_step(P, s32, ap, in_place(o, x), PRO_NONE, EPI_BIAS_RES, OUT_F32, "attn.proj");
        snapshot(x, "bb.pos_net.2");
    }
    resnet(M->res[2], "bb.pos_net.3", SITE_RES2);
    resnet(M->res[3], "bb.pos_net.4", SITE_RES3);
    P->cur_site = SITE_CNX0;
    // pos_net[5] GroupNorm + backbone.norm AdaLayerNorm (models.py:213,228), fused into one row pass
    const int xc = P->buf(keep ? "bb.x2" : "bb.norm", (size_t)Mrows * D);
    P->step({x, gp, sc, sh}, [=](const RunCtx& c) {
        return launch_gn_stats(P->ptr(c, x), M->gn5w, M->gn5b, P->ptr(c, sc), P->ptr(c, sh), B, L, D, 32, 1e-6f, c.stream, P->ptr(c, gp), lens(c));
    });
    P->step({x, sc, sh, xc}, [=](const RunCtx& c) {
        return launch_rownorm(RN_AFFINE_IN, P->ptr(c, x), P->ptr(c, xc), B, L, D, nullptr, nullptr, P->ptr(c, sc),
                              P->ptr(c, sh), M->ada_s + (size_t)c.bw_id * D, M->ada_h + (size_t)c.bw_id * D, 1e-6f, c.stream);
    });
    snapshot(xc, "bb.norm");
    // ConvNeXt blocks (modules.py:43-60); xc is the residual stream from here on
    const int nrm = P->buf("bb.cnx.norm", (size_t)Mrows * D, s32_plan ? BUF_S32 : BUF_F32);
    const int mid = P->buf("bb.cnx.mid", (size_t)Mrows * I, s32_plan ? BUF_S32 : BUF_F32);
    for (int i = 0; i < ar.num_layers; ++i) {
        const CnxBlock cb = M->cnx[i];
        P->cur_site = SITE_CNX0 + i;
        const bool s32 = s32_at(SITE_CNX0 + i);
        P->bufs[nrm].fmt = P->bufs[mid].fmt = s32 ? BUF_S32 : BUF_F32;
        P->step({xc, nrm}, [=](const RunCtx& c) {
            return launch_rownorm(RN_DWCONV, P->ptr(c, xc), P->ptr(c, nrm), B, L, D, cb.dw_w, cb.dw_b, nullptr, nullptr,
                                  cb.ada_s + (size_t)c.bw_id * D, cb.ada_h + (size_t)c.bw_id * D, 1e-6f, c.stream, s32, lens(c));
        });
        // GELU output pre-split for pwconv2
        gemm_step(P, s32, linear_args(cb.W1, cb.b1, Mrows, I, D), {nrm, -1, mid}, PRO_NONE, EPI_BIAS_GELU, OUT_S32, "cnx.pwconv1");
        GemmArgs a2 = linear_args(cb.W2, cb.b2, Mrows, D, I);
        a2.r_rstride = D; a2.gamma = cb.gamma;
        gemm_step(P, s32, a2, in_place(mid, xc), PRO_NONE, EPI_BIAS_GAMMA_RES, OUT_F32, "cnx.pwconv2");
        if (i == 0 || i == ar.num_layers / 2 - 1 || i == ar.num_layers - 1) snapshot(xc, "bb.convnext." + std::to_string(i));
    }
    P->cur_site = SITE_HEAD;
    const bool s32 = s32_at(SITE_HEAD);
    const int xo = P->buf("bb.out", (size_t)Mrows * D, s32 ? BUF_S32 : BUF_F32);
    P->step({xc, xo}, [=](const RunCtx& c) {
        if (int rc = launch_rownorm(RN_PLAIN, P->ptr(c, xc), P->ptr(c, xo), B, L, D, nullptr, nullptr, nullptr, nullptr,
                                    M->fln_w, M->fln_b, 1e-6f, c.stream, s32)) return rc;
        if (c.aux && s32)      // the caller wants the backbone output: a second, fp32 pass straight into its buffer
            return launch_rownorm(RN_PLAIN, P->ptr(c, xc), c.aux, B, L, D, nullptr, nullptr, nullptr, nullptr, M->fln_w,
                                  M->fln_b, 1e-6f, c.stream, 0);
        return c.aux ? copy_f32(c.aux, P->ptr(c, xo), (size_t)Mrows * D, c.stream) : 0;
    });
    plan_head(P, xo, s32, mixed);
    return 0;
}

// ISTFTHead alone (decoder/heads.py:42-67 + spectral_ops.py:33-75): x [B][L][dim] fp32 -> audio [B][L*hop]
int build_head(wt_plan* P) {
    const wt_model* M = P->model;
    const int B = P->B, L = (int)P->L, D = M->arch.dim;
    const long Mrows = (long)B * L;
    const bool s32 = plan_s32(P) && (D % 32 == 0) && M->head_W.s32.p && M->istft_W.s32.p;
    const int xo = P->buf("head.in", (size_t)Mrows * D, s32 ? BUF_S32 : BUF_F32);
    if (s32) P->step({xo}, [=](const RunCtx& c) { return launch_split_s32(c.in_f, P->ptr(c, xo), Mrows * D, c.stream); });
    else copy_step(P, CALLER, xo, (size_t)Mrows * D);
    P->n_out = P->B * wave_samples(M, L);
    plan_head(P, xo, s32);
    return 0;
}

// The SEANetDecoder runs on S32 operands (the default) when every GEMM weight it needs has an S32 copy
static bool seadec_s32_ok(const wt_plan* P) {
    const wt_model* M = P->model;
    if (!plan_s32(P) || M->sd_stages.empty() || !M->sd_first.s32.p || !M->sd_lstm.Wih0.s32.p) return false;
    for (const SeaDecStage& st : M->sd_stages) {
        if (!st.tr_wp.s32.p || st.cout % 32) return false;
        if (!resblock_fusable(st.cout) && !(st.c3.s32.p && st.c1.s32.p && st.sc.s32.p)) return false;
    }
    return resblock_fusable(M->sd_stages.back().cout);      // the last conv reads fp32
}

// SEANetDecoder: z -> conv k7 -> LSTM -> per stage: transposed conv -> resblock -> ... -> last conv.  On S32 operands every
// GEMM operand is written pre-split by its producer, as in build_encode: the first conv writes fp32 for the LSTM skip +
// S32 for its input projection, the LSTM S32(elu), each phase GEMM fp32 for a fused resblock (resblock16 reads fp32 and
// writes S32(elu)) or S32 raw + S32 elu for an unfused one.
int build_seanet_decoder(wt_plan* P) {
    const wt_model* M = P->model;
    if (!M->has_seadec) { set_error("checkpoint holds no SEANetDecoder weights"); return WT_ERR_MISSING_TENSOR; }
    const int B = P->B, L = (int)P->L, H = M->H;
    P->n_out = (long)B * L * M->hop;
    const bool s32 = seadec_s32_ok(P);
    const bool fuse_elu = !plan_unfused(P);      // producers store elu(.) for "ELU -> conv" consumers
    const int x0 = P->buf("sdec.in", (size_t)B * L * 512);
    P->step({x0}, [=](const RunCtx& c) { return launch_transpose(c.in_f, P->ptr(c, x0), B, 512, L, c.stream, s32); });
    const int xf = P->buf("sdec.0", (size_t)B * L * H);
    const int xs = s32 ? P->buf("sdec.0.s32", (size_t)B * L * H) : -1;
    // these and an unfused stage's transposed-conv outputs hold S32 under a BUF_F32 declaration (kept: wt_plan_buffer_info)
    P->bufs[x0].holds_s32 = s32;
    if (xs >= 0) P->bufs[xs].holds_s32 = true;
    gemm_step(P, s32, sconv_args(M->sd_first, B, L, 1, 1), {x0, -1, xf, xs}, PRO_NONE, EPI_BIAS, OUT_F32_AND_S32);
    int x = plan_lstm(P, M->sd_lstm, B, L, H, xf, "sdec.1", fuse_elu, xs, s32);
    long Tc = L;
    int di = 2;
    for (size_t si = 0; si < M->sd_stages.size(); ++si) {
        const SeaDecStage st = M->sd_stages[si];
        const long To = Tc * st.r;
        const int xin = x;
        const int Tin = (int)Tc;
        const bool unfused_s32 = s32 && !resblock_fusable(st.cout);
        const bool last = si + 1 == M->sd_stages.size();
        const std::string name = "sdec." + std::to_string(di + 1);
        int y, y2 = -1;
        long y_off = 0, y_bs = 0;
        if (st.tr_wp.w) {
            // SConvTranspose1d (conv.py:232-253) with k = 2*stride: output sample u' = t*stride + r gets
            // x[t].W[r] + x[t-1].W[r+stride], i.e. per phase r one GEMM over rows t = 0..Tin with the two
            // frames as K (zero beyond the clip); the phases are the batch dimension and interleave in the
            // untrimmed output, of which the following resblock reads the trimmed view.
            const int trim_l = (st.k - st.r) - (st.k - st.r) / 2;
            const size_t ynum = (size_t)B * (Tin + 1) * st.r * st.cout;
            y = P->buf(name, ynum);
            if (unfused_s32) { y2 = P->buf(name + ".elu", ynum); P->bufs[y].holds_s32 = P->bufs[y2].holds_s32 = true; }
            y_off = (long)trim_l * st.cout;
            y_bs = (long)(Tin + 1) * st.r * st.cout;
            GemmArgs a;
            a.a_bstride = (long)Tin * st.cin; a.a_rstride = st.cin;
            a.T_in = Tin; a.T_out = Tin + 1; a.Cin = st.cin; a.taps = 2; a.pad_left = 1; a.pad_mode = PAD_ZERO;
            a.W = st.tr_wp.w; a.w_rstride = 2L * st.cin; a.zW = (long)st.cout * 2 * st.cin; a.bias = st.tr_b;
            a.M = B * (Tin + 1); a.N = st.cout; a.K = 2 * st.cin;
            a.c_rstride = (long)st.r * st.cout; a.zC = st.cout; a.nz = st.r;
            set_s32(a, st.tr_wp.s32);
            gemm_step(P, s32, a, {xin, -1, y, y2}, fuse_elu ? PRO_NONE : PRO_ELU, EPI_BIAS, y2 >= 0 ? OUT_S32_DUAL_ELU : OUT_F32, "sdec.convtr");
        } else {
            y = P->buf(name, (size_t)B * To * st.cout);
            P->step({xin, y}, [=](const RunCtx& c) {
                return launch_convtr(P->ptr(c, xin), st.tr_w, st.tr_b, P->ptr(c, y), B, Tin, st.cin, st.cout, st.k, st.r,
                                     fuse_elu ? 0 : 1, c.stream);
            }, 1, "sdec.convtr");
        }
        const std::string rname = "sdec." + std::to_string(di + 2);
        if (unfused_s32)
            x = plan_resblock_s32(P, st.c3, st.sc, st.cat, B, To, y, y2, rname, y_off, y_bs);
        else
            x = plan_resblock(P, st.c3, st.c1, st.sc, B, To, y, rname, fuse_elu, nullptr, y_off, y_bs, s32 && !last);
        if (x < 0) return WT_ERR_INVALID;
        Tc = To; di += 3;
    }
    const int xin = x;
    const long Tf = Tc;
    P->step({xin}, [=](const RunCtx& c) {
        return launch_conv_last(P->ptr(c, xin), M->sd_last_w, M->sd_last_b, c.out_f, B, Tf, 32, 7, fuse_elu ? 0 : 1, c.stream);
    }, 1, "sdec.last");
    return 0;
}


// Every plan starts by zeroing its control block (word 0 = the call's status, common.h) and ends with the guard step
void plan_begin(wt_plan* P) {
    P->ctl = P->buf("ctl", CTL_WORDS);
    const int ctl = P->ctl;
    P->step({ctl}, [=](const RunCtx& c) {
        return launch_fill_u32(P->ptr(c, ctl), 0u, CTL_WORDS * sizeof(unsigned), c.stream);
    }, 1, "ctl.clear");
}

void plan_end(wt_plan* P) {
    const wt_model* M = P->model;
    const int ctl = P->ctl;
    const long nc = P->n_codes, n0 = P->n_out, n1 = P->n_aux;      // what the builder said a call writes
    const bool per_round = plan_rvq(P);      // codes [n_q][B][L], n_q the call's
    P->step({ctl}, [=](const RunCtx& c) {
        return launch_plan_guard(reinterpret_cast<const unsigned*>(P->ptr(c, ctl)), CTL_WORDS, CTL_SITE0, P->status_dev, M->status_dev,
                                 nc ? c.codes : nullptr, per_round ? nc * c.n_q : nc, c.out_f, n0, n1 ? c.aux : nullptr, n1, nullptr, 0, c.stream);
    }, 1, "guard");
}

// SLSTM alone (unit parity tests: lstm_persist_kernel / lstm_step_kernel against the oracle): x [B][L][512] fp32,
// time-major -> y = lstm(x) + x, through exactly the steps the encoder plan uses (S32 copy of x for the input
// projection GEMM, then the recurrence).  WT_PLAN_FLAG_STEP_LSTM selects the launch-per-step kernel.
int build_unit_lstm(wt_plan* P) {
    const wt_model* M = P->model;
    const int B = P->B, L = (int)P->L, H = M->H;
    const bool s32 = plan_s32(P) && M->enc_lstm.Wih0.s32.p;
    const int x = P->buf("lstm.in", (size_t)B * L * H);
    const int xs = s32 ? P->buf("lstm.in.s32", (size_t)B * L * H, BUF_S32) : -1;
    P->n_out = (long)B * L * 512;
    P->step({x, xs}, [=](const RunCtx& c) {
        if (int rc = copy_f32(P->ptr(c, x), c.in_f, (size_t)B * L * H, c.stream)) return rc;
        return s32 ? launch_split_s32(c.in_f, P->ptr(c, xs), (long)B * L * H, c.stream) : 0;
    }, 2, "lstm.in");
    const int y = plan_lstm(P, M->enc_lstm, B, L, H, x, "lstm.out", false, xs, false);
    copy_step(P, y, CALLER, (size_t)B * L * H, "lstm.copy");
    return 0;
}

}  // namespace wt
