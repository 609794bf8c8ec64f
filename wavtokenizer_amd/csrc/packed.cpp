// The model's device arrays, described once (walk_model), and what reads that description: the packed image's model section
// (Archive), the check of a loaded section against the header's architecture (Validator) and the weights by name (Lister);
// then the image itself: header, hash, export and import.  Only model_import's allocate-and-upload loop and model_export's
// read-back make HIP calls: the rest runs without a GPU (tests/host/packed_section_check.cpp drives it on a synthetic model).
#include "model.h"

namespace wt {

// ------------------------------------------------------------------------------------ the one walk
// dims of an array; its extent is their product in the unit of its format: halves for the two f16 lane packings of the LSTM,
// 4-byte words for everything else
struct Dims {
    int n = 0;
    int64_t d[4] = {0, 0, 0, 0};
    Dims(std::initializer_list<int64_t> l) { for (int64_t x : l) d[n++] = x; }
    size_t bytes(int fmt) const {
        size_t p = (fmt == WFMT_LSTM_F16 || fmt == WFMT_LSTM_PERSIST) ? 2 : 4;
        for (int i = 0; i < n; ++i) p *= (size_t)d[i];
        return p;
    }
};

// walk_model visits every member of wt_model that the image stores, in the order of the image's bytes, and tells the visitor
// what the architecture (M->arch alone) says about it.  A visitor has:
//   pod(field)                               a stored value the architecture does not fix
//   dim(field, want, name)                   a stored int that must equal `want`
//   count(vector, limit, want, name)         a stored element count (want < 0: any); returns how many elements to walk
//   arr(name, p, format, dims, optional)     an array of the listing; optional: may be null
//   copy(name, of, s32, dims, pair_ok)       the S32 copy of array `of` (always optional); pair_ok: tap_pair may be set
//   ref(p)                                   a stored pointer that is no array of the listing (the lazy list's)
//   optional(present, expected)              whether to walk a group that a model may lack: the image always holds it
//                                            (as nulls), the other visitors skip an absent one; expected: build_model makes it
template <class V> static void walk_conv(V& v, const std::string& name, ConvW& c, int cout, int cin, int k, bool pair_ok = false) {
    v.arr(name + ".w", c.w, WFMT_F32, {cout, k, cin}); v.arr(name + ".b", c.b, WFMT_F32, {cout});
    v.dim(c.cout, cout, name + ".cout"); v.dim(c.cin, cin, name + ".cin"); v.dim(c.k, k, name + ".k");
    v.copy(name + ".s32", name + ".w", c.s32, {cout, k, cin}, pair_ok);
}
// dims: the listing's shape where it is not the GEMM's rows x cols; the S32 copy has the GEMM's extent
template <class V> static void walk_gemm(V& v, const std::string& name, GemmW& g, int rows, int cols, const Dims& dims, const Dims& cdims) {
    v.arr(name, g.w, WFMT_F32, dims);
    v.dim(g.rows, rows, name + ".rows"); v.dim(g.cols, cols, name + ".cols");
    v.copy(name + ".s32", name, g.s32, cdims, false);
}
template <class V> static void walk_gemm(V& v, const std::string& name, GemmW& g, int rows, int cols) { walk_gemm(v, name, g, rows, cols, {rows, cols}, {rows, cols}); }
template <class V> static void walk_lstm(V& v, const std::string& name, LstmW& l, int H) {
    walk_gemm(v, name + ".Wih0", l.Wih0, 4 * H, H);
    v.arr(name + ".b0", l.b0, WFMT_F32, {4 * H});
    v.arr(name + ".W0", l.W0, WFMT_F32, {4 * H / 16, H / 16, 64, 4});
    v.arr(name + ".W1", l.W1, WFMT_F32, {4 * H / 16, 2 * H / 16, 64, 4});
    v.arr(name + ".b1", l.b1, WFMT_F32, {4 * H});
    v.arr(name + ".W0h", l.W0h, WFMT_LSTM_F16, {4 * H / 16, H / 32, 2, 512}, true);
    v.arr(name + ".W1h", l.W1h, WFMT_LSTM_F16, {4 * H / 16, 2 * H / 32, 2, 512}, true);
    v.arr(name + ".Wp", l.Wp, WFMT_LSTM_PERSIST, {3 * 32 * 4, 16, 2, 512}, true);
}
// the architecture has passed check_arch, or comes from wt_model_create's own checks (n_ratios in 1 .. 8)
template <class V> static void walk_model(wt_model* M, V& v) {
    const wt_arch& a = M->arch;
    const int nf = 32, H = 512, D = a.dim, I = a.intermediate_dim, A = a.adanorm_num_embeddings, N = a.n_fft;
    const int Kq = ((N / 4 + 1 + 31) / 32) * 32, Kb = 2 * Kq;
    auto enc_ratio = [&](size_t i) { return (int)i < a.n_ratios ? a.ratios[a.n_ratios - 1 - i] : 0; };      // seanet.py:100
    auto vec = [&](const std::string& name, float*& p, int64_t n) { v.arr(name, p, WFMT_F32, {n}); };
    int hop = 1;
    for (int i = 0; i < a.n_ratios; ++i) hop *= a.ratios[i];
    v.dim(M->hop, hop, "hop"); v.dim(M->H, H, "H"); v.pod(M->weight_bytes); v.pod(M->s32_ok); v.pod(M->sd_s32_ok); v.pod(M->w_amax);
    size_t n = v.count(M->enc_ratios, 8, a.n_ratios, "the encoder's ratio count");
    for (size_t i = 0; i < n; ++i) v.dim(M->enc_ratios[i], enc_ratio(i), "enc_ratios[" + std::to_string(i) + "]");
    v.arr("enc.e0.w", M->e0_w, WFMT_F32, {7, nf}); vec("enc.e0.b", M->e0_b, nf); v.dim(M->e0_k, 7, "enc.e0.k"); v.dim(M->e0_c, nf, "enc.e0.c");
    n = v.count(M->stages, 8, a.n_ratios, "the encoder's stage count");
    for (size_t i = 0; i < n; ++i) {
        ResStage& st = M->stages[i];
        const std::string p = "enc.stage" + std::to_string(i + 1);
        const int C = nf << i, r = enc_ratio(i);
        walk_conv(v, p + ".c3", st.c3, C / 2, C, 3); walk_conv(v, p + ".c1", st.c1, C, C / 2, 1); walk_conv(v, p + ".sc", st.sc, C, C, 1);
        walk_conv(v, p + ".down", st.down, 2 * C, C, 2 * r, true);       // taps in paired order only where build_splits packs them so
        if (v.optional(st.cat.w || st.cat.s32.p, !resblock_fusable(C))) walk_conv(v, p + ".cat", st.cat, C, C + C / 2, 1);
        v.dim(st.C, C, p + ".C"); v.dim(st.r, r, p + ".r");
    }
    walk_lstm(v, "enc.lstm", M->enc_lstm, H); walk_conv(v, "enc.final", M->enc_final, 512, H, 7);
    // the array holds every codebook, the GEMM and its S32 copy are codebook 0
    walk_gemm(v, "vq.embed", M->embed, a.vq_bins, 512, {a.num_quantizers, a.vq_bins, 512}, {a.vq_bins, 512});
    vec("vq.ee", M->ee, a.vq_bins);
    walk_conv(v, "bb.embed", M->bb_embed, D, a.input_channels, 7);
    for (int i = 0; i < 4; ++i) {
        PosRes& r = M->res[i];
        const std::string p = "bb.res." + std::to_string(i);
        vec(p + ".n1w", r.n1w, D); vec(p + ".n1b", r.n1b, D); vec(p + ".n2w", r.n2w, D); vec(p + ".n2b", r.n2b, D);
        walk_conv(v, p + ".c1", r.c1, D, D, 3); walk_conv(v, p + ".c2", r.c2, D, D, 3);
    }
    vec("bb.attn.nw", M->at_nw, D); vec("bb.attn.nb", M->at_nb, D);
    walk_gemm(v, "bb.attn.Wqk", M->at_Wqk, 2 * D, D); vec("bb.attn.bqk", M->at_bqk, 2 * D);
    walk_gemm(v, "bb.attn.Wv", M->at_Wv, D, D); vec("bb.attn.bv", M->at_bv, D);
    walk_gemm(v, "bb.attn.Wp", M->at_Wp, D, D); vec("bb.attn.bp", M->at_bp, D);
    vec("bb.gn5.w", M->gn5w, D); vec("bb.gn5.b", M->gn5b, D);
    v.arr("bb.ada.s", M->ada_s, WFMT_F32, {A, D}); v.arr("bb.ada.h", M->ada_h, WFMT_F32, {A, D});
    n = v.count(M->cnx, 64, a.num_layers, "the ConvNeXt block count");
    for (size_t i = 0; i < n; ++i) {
        CnxBlock& c = M->cnx[i];
        const std::string p = "bb.cnx." + std::to_string(i);
        v.arr(p + ".dw_w", c.dw_w, WFMT_F32, {7, D}); vec(p + ".dw_b", c.dw_b, D);
        v.arr(p + ".ada_s", c.ada_s, WFMT_F32, {A, D}); v.arr(p + ".ada_h", c.ada_h, WFMT_F32, {A, D});
        walk_gemm(v, p + ".W1", c.W1, I, D); vec(p + ".b1", c.b1, I);
        walk_gemm(v, p + ".W2", c.W2, D, I); vec(p + ".b2", c.b2, D);
        vec(p + ".gamma", c.gamma, D);
    }
    vec("bb.fln.w", M->fln_w, D); vec("bb.fln.b", M->fln_b, D);
    walk_gemm(v, "head.W", M->head_W, 2 * Kb, D); vec("head.b", M->head_b, 2 * Kb);
    v.dim(M->Kb, Kb, "head.Kb"); v.dim(M->Kq, Kq, "head.Kq"); v.dim(M->bins_f, N / 2 + 1, "head.bins"); v.dim(M->R, N / a.hop_length, "head.R");
    walk_gemm(v, "istft.W", M->istft_W, 4 * Kq, Kq, {4, Kq, Kq}, {4, Kq, Kq});
    vec("istft.wsq", M->wsq, N); vec("istft.win", M->win, N);
    v.pod(M->has_seadec);
    if (v.optional(M->has_seadec, M->has_seadec)) {
        walk_conv(v, "sd.first", M->sd_first, nf << a.n_ratios, 512, 7);
        walk_lstm(v, "sd.lstm", M->sd_lstm, H);
        n = v.count(M->sd_stages, 8, a.n_ratios, "the SEANetDecoder's stage count");
        for (size_t i = 0; i < n; ++i) {
            SeaDecStage& st = M->sd_stages[i];
            const std::string p = "sd.stage" + std::to_string(i + 1);
            const int r = a.ratios[i], cin = (nf << a.n_ratios) >> i, h = cin / 2;
            v.arr(p + ".tr_w", st.tr_w, WFMT_F32, {2 * r, cin, h});
            if (v.optional(st.tr_wp.w || st.tr_wp.s32.p, true)) walk_gemm(v, p + ".tr_wp", st.tr_wp, r * h, 2 * cin, {r, h, 2, cin}, {r, h, 2, cin});
            vec(p + ".tr_b", st.tr_b, h);
            v.dim(st.cin, cin, p + ".cin"); v.dim(st.cout, h, p + ".cout"); v.dim(st.k, 2 * r, p + ".k"); v.dim(st.r, r, p + ".r");
            walk_conv(v, p + ".c3", st.c3, h / 2, h, 3); walk_conv(v, p + ".c1", st.c1, h, h / 2, 1); walk_conv(v, p + ".sc", st.sc, h, h, 1);
            if (v.optional(st.cat.w || st.cat.s32.p, !resblock_fusable(h))) walk_conv(v, p + ".cat", st.cat, h, h + h / 2, 1);
        }
        v.arr("sd.last.w", M->sd_last_w, WFMT_F32, {7, nf}); vec("sd.last.b", M->sd_last_b, 1);
    }
    // the fp32 arrays the image leaves out: part of the section, no arrays of the listing (model_import checks the entries)
    n = v.count(M->lazy_f32, 1 << 12, -1, "the list of unstored fp32 arrays");
    for (size_t i = 0; i < n; ++i) { wt_model::LazyF32& z = M->lazy_f32[i]; v.ref(z.w); v.ref(z.s32); v.pod(z.n); v.pod(z.scale); }
}

// ------------------------------------------------------------------------------------ the model section, saved and loaded
// Pods raw in their own widths (bool, int, int64), pointers as (int32 allocation index, int64 byte offset), vectors behind an int32 count.
struct Archive {
    bool saving;
    std::vector<char>* out = nullptr;          // saving
    const char* in = nullptr;                  // loading
    size_t pos = 0, n = 0;
    bool ok = true;
    const std::map<const void*, int>* index = nullptr;      // saving: allocation base -> index
    const std::vector<void*>* allocs = nullptr;             // loading: index -> allocation base
    const std::vector<size_t>* alloc_bytes = nullptr;       // loading: index -> allocation size (pointer offsets are checked)
    void raw(void* p, size_t bytes) {
        if (saving) { const char* c = static_cast<const char*>(p); out->insert(out->end(), c, c + bytes); }
        else { if (!ok || bytes > n - pos) { ok = false; std::memset(p, 0, bytes); return; } std::memcpy(p, in + pos, bytes); pos += bytes; }
    }
    template <class T> void pod(T& v) { raw(&v, sizeof(T)); }
    void dim(int& v, int, const std::string&) { pod(v); }
    // an element count read from the file: bounded before anything is resized by it
    template <class T> size_t count(std::vector<T>& x, int32_t limit, int, const char*) {
        int32_t c = (int32_t)x.size();
        pod(c);
        if (!saving && (c < 0 || c > limit)) { ok = false; c = 0; }
        x.resize(c);
        return c;
    }
    template <class T> void ref(T*& p) {       // a device pointer = (allocation index, byte offset); -1 = null
        int32_t idx = -1;
        int64_t off = 0;
        if (saving && p) {
            auto it = index->upper_bound(static_cast<const void*>(p));
            if (it == index->begin()) { ok = false; }
            else { --it; idx = it->second; off = reinterpret_cast<const char*>(p) - static_cast<const char*>(it->first); }
        }
        pod(idx); pod(off);
        if (!saving) {
            if (idx < 0) p = nullptr;
            else if (!ok || idx >= (int)allocs->size() || off < 0 || (size_t)off >= (*alloc_bytes)[idx]) { ok = false; p = nullptr; }
            else p = reinterpret_cast<T*>(static_cast<char*>((*allocs)[idx]) + off);
        }
    }
    template <class T> void arr(const std::string&, T*& p, int, const Dims&, bool = false) { ref(p); }
    void copy(const std::string&, const std::string&, S32Copy& s, const Dims&, bool) { ref(s.p); pod(s.acc_scale); pod(s.tap_pair); }
    bool optional(bool, bool) { return true; }
};

// The model section of a packed image is data from a file: after it is loaded every dimension is compared with what the
// header's wt_arch fixes (what build_model would have set), and every array's EXTENT - not only its start - must lie inside
// the allocation it points into.  The body hash only detects accidental corruption (it is not cryptographic): a crafted
// file must not be able to make a plan size its launches past an allocation.
struct Validator {
    const wt_model* M;
    std::string bad;                           // the first array or field that is wrong
    void fail(const std::string& name) { if (bad.empty()) bad = name; }
    bool fits(const void* p, size_t bytes) const {
        if (!p) return false;
        const char* c = static_cast<const char*>(p);
        for (size_t i = 0; i < M->allocs.size(); ++i) {
            const char* base = static_cast<const char*>(M->allocs[i]);
            if (c >= base && c < base + M->alloc_bytes[i]) return bytes <= (size_t)(base + M->alloc_bytes[i] - c);
        }
        return false;
    }
    template <class T> void pod(T&) {}
    template <class T> void ref(T*&) {}
    void dim(int& v, int want, const std::string& name) { if (v != want) fail(name); }
    template <class T> size_t count(std::vector<T>& x, int32_t, int want, const char* name) {
        if (want >= 0 && (int64_t)x.size() != want) fail(name);
        return bad.empty() ? x.size() : 0;         // (the walk indexes the architecture by element)
    }
    template <class T> void arr(const std::string& name, T*& p, int fmt, const Dims& d, bool optional = false) {
        if (!(optional && !p) && !fits(p, d.bytes(fmt))) fail(name);
    }
    // an S32 copy is null or has the footprint of the fp32 array it stands for
    void copy(const std::string& name, const std::string&, S32Copy& s, const Dims& d, bool pair_ok) {
        if ((s.p && !fits(s.p, d.bytes(WFMT_S32))) || !(s.acc_scale > 0.f) || !std::isfinite(s.acc_scale) || (s.tap_pair && !pair_ok)) fail(name);
    }
    bool optional(bool present, bool) { return present; }
};

static int bad_image(const std::string& what) { set_error("packed image: " + what + " does not match the architecture in its header"); return WT_ERR_INVALID; }

// The architectures this library runs: the one rule of wt_model_create, wt_model_create_packed and wt_packed_info, made before
// any HIP call.  What passes here has kernels for every step of every plan kind; what does not is refused when the model is
// created, never at plan creation or at a launch.  Returns the refusal (it names the field), empty when the architecture is taken.
std::string arch_refusal(const wt_arch& a) {
    if (a.n_ratios < 1 || a.n_ratios > 8) return "n_ratios out of range";
    // a stage's down conv has 2 * ratio taps and both GEMM engines gather at most 32 (check_gemm16s, launch_gemm: the tap
    // tables' share of LDS): a ratio above 16 loaded and then failed at the conv's launch
    for (int i = 0; i < a.n_ratios; ++i) if (a.ratios[i] < 1 || a.ratios[i] > 16) return "ratios: every ratio must be 1 .. 16 (a down conv has 2 * ratio taps; the GEMM kernels gather at most 32)";
    if ((32 << a.n_ratios) != 512) return "ratios: the encoder width after the last ratio must be 512 (32 * 2^n_ratios: four ratios)";          // mult * nf == H
    if (a.num_quantizers < 1 || a.num_quantizers > 32) return "num_quantizers must be 1 .. 32 (encode_infer uses the first codebook: vq.py:137 forces n_q = 1; codes_to_features sums up to num_quantizers of them)";
    if (a.input_channels != 512) return "input_channels must be 512 (SEANet dimension)";
    // the row kernels (dwconv + LayerNorm, AdaLayerNorm: launch_rownorm) are built for these four widths
    if (a.dim != 256 && a.dim != 512 && a.dim != 768 && a.dim != 1024) return "dim must be 256, 512, 768 or 1024";
    if (a.intermediate_dim < 32 || a.intermediate_dim % 32) return "intermediate_dim must be a positive multiple of 32";
    if (a.num_layers < 1 || a.num_layers > 32) return "num_layers must be 1 .. 32 (one range site per ConvNeXt block)";
    if (a.adanorm_num_embeddings < 1) return "adanorm_num_embeddings must be >= 1: only the AdaLayerNorm backbone is implemented";
    // the shipped encode plan runs the VQ distances on gemm16s.hip, whose argmax epilogue reads |e|^2 four columns at a time
    if (a.vq_bins < 4 || a.vq_bins % 4) return "vq_bins must be a positive multiple of 4 (the VQ distance kernel takes four codebook columns at a time)";
    if (a.n_fft < 4 || a.hop_length < 1) return "n_fft must be >= 4 and hop_length >= 1";
    if (a.n_fft % a.hop_length || a.n_fft % 2 || (a.n_fft - a.hop_length) % 2) return "n_fft must be an even multiple of hop_length (the ISTFT kernel; n_fft and n_fft - hop_length even)";
    if (a.n_fft % 4) return "n_fft % 4 must be 0 (the ISTFT kernel takes the spectrum in quarters)";
    return {};
}

// what the walk takes for granted of the header's architecture
static int check_arch(const wt_arch& a) {
    const std::string why = arch_refusal(a);
    if (why.empty()) return WT_OK;
    set_error("packed image: " + why + " (the architecture in its header)");
    return WT_ERR_INVALID;
}
static int validate_imported(const wt_model* M) {
    if (int rc = check_arch(M->arch)) return rc;
    Validator v{M, {}};
    walk_model(const_cast<wt_model*>(M), v);         // (the visitor modifies nothing)
    return v.bad.empty() ? (int)WT_OK : bad_image(v.bad);
}

// ------------------------------------------------------------------------------------ the weights by name
// Every device array a plan can read (wt_model_weight_info): the walk's arrays that are not null.  numel counts 4-byte words.
struct Lister {
    std::vector<WeightEntry> out;
    std::vector<const float*> paired;          // the tap-paired repackings of the down convs: held by lazy_f32 alone (s32 = null), in stage order
    size_t next_pair = 0;
    WeightEntry* add(const std::string& name, const void* p, int fmt, const Dims& d) {
        if (!p) return nullptr;
        WeightEntry e;
        e.name = name; e.data = p; e.format = fmt; e.ndim = d.n; e.archived = true;
        std::copy(d.d, d.d + 4, e.dims);
        e.numel = (int64_t)(d.bytes(fmt) / 4);
        out.push_back(e);
        return &out.back();
    }
    template <class T> void pod(T&) {}
    template <class T> void ref(T*&) {}
    void dim(int&, int, const std::string&) {}
    template <class T> size_t count(std::vector<T>& x, int32_t, int, const char*) { return x.size(); }
    template <class T> void arr(const std::string& name, T*& p, int fmt, const Dims& d, bool = false) { add(name, p, fmt, d); }
    void copy(const std::string& name, const std::string& of, S32Copy& s, const Dims& d, bool pair_ok) {
        if (WeightEntry* e = add(name, s.p, WFMT_S32, d)) { e->of = of; e->acc_scale = s.acc_scale; e->tap_pair = s.tap_pair; }
        if (pair_ok && s.tap_pair && next_pair < paired.size()) add(of + "pair", paired[next_pair++], WFMT_F32, d);      // "<stage>.down.wpair"
    }
    bool optional(bool present, bool) { return present; }
};

std::vector<WeightEntry> model_weights(const wt_model* M) {
    Lister ls;
    for (const wt_model::LazyF32& z : M->lazy_f32) if (!z.s32) ls.paired.push_back(z.w);
    walk_model(const_cast<wt_model*>(M), ls);        // (the visitor modifies nothing)
    std::vector<WeightEntry>& out = ls.out;
    // the one place where the listing's order is not the image's: the image holds wsq in front of win
    for (size_t i = 0; i + 1 < out.size(); ++i)
        if (out[i].name == "istft.wsq" && out[i + 1].name == "istft.win") { std::swap(out[i], out[i + 1]); break; }
    std::map<const void*, int> index;
    for (size_t i = 0; i < M->allocs.size(); ++i) index[M->allocs[i]] = (int)i;
    for (WeightEntry& e : out) {
        auto at = index.find(e.data);
        if (at != index.end()) e.alloc = at->second;
        for (const wt_model::LazyF32& z : M->lazy_f32)
            if (static_cast<const void*>(z.w) == e.data) { e.lazy = z.s32 ? 1 : 2; e.lazy_scale = z.scale; }
    }
    return out;
}

// ------------------------------------------------------------------------------------ packed image
// a packed on-disk weight format "folded, pre-tiled".  The image is what wt_model_create leaves in HBM, as the
// list of device allocations in creation order, preceded by a header (magic, version, the wt_arch and a hash of it) and the
// model section (walk_model through an Archive).  Loading it is allocate + upload + fix up pointers: nothing is computed again.
static constexpr uint32_t PACK_MAGIC = 0x4b505457u;     // "WTPK"
static constexpr int32_t PACK_VERSION = 7;

static uint64_t arch_hash_of(const wt_arch& a) {        // FNV-1a over the architecture struct and the layout version
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= static_cast<const unsigned char*>(p)[i]; h *= 1099511628211ull; } };
    mix(&a, sizeof(a));
    mix(&PACK_VERSION, sizeof(PACK_VERSION));
    return h;
}

struct PackHeader {
    uint32_t magic;
    int32_t version;
    wt_arch arch;
    uint64_t arch_hash;
    uint64_t n_allocs, struct_bytes, payload_bytes;
    uint64_t body_hash;        // over the allocation table, the model section and the payload (everything behind the header)
};

// 64-bit hash of a byte range, four interleaved multiply-xor lanes over 8-byte words (a serial FNV over ~0.7 GB would
// take longer than the upload itself); the tail bytes and the length go into lane 0
static uint64_t body_hash_of(const char* p, size_t n) {
    uint64_t h[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x27d4eb2f165667c5ull};
    const uint64_t K = 0x100000001b3ull * 0x9e3779b1ull | 1ull;
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        std::memcpy(w, p + i, 32);
        for (int l = 0; l < 4; ++l) { h[l] = (h[l] ^ w[l]) * K; h[l] ^= h[l] >> 29; }
    }
    for (; i < n; ++i) { h[0] = (h[0] ^ (unsigned char)p[i]) * K; h[0] ^= h[0] >> 29; }
    h[0] = (h[0] ^ (uint64_t)n) * K;
    return (h[0] ^ (h[1] * 3) ^ (h[2] * 5) ^ (h[3] * 7)) * K;
}

// allocation table entry of an array the image does not store (wt_model::lazy_f32): its size with this bit set
static constexpr uint64_t PACK_NOT_STORED = 1ull << 63;

static std::vector<bool> lazy_allocs(const wt_model* M) {
    std::vector<bool> lazy(M->allocs.size(), false);
    for (const wt_model::LazyF32& z : M->lazy_f32)
        for (size_t i = 0; i < M->allocs.size(); ++i)
            if (M->allocs[i] == static_cast<const void*>(z.w)) lazy[i] = true;       // lazy arrays are whole allocations
    return lazy;
}

size_t model_export_bytes(const wt_model* M) {
    size_t total = sizeof(PackHeader) + M->allocs.size() * sizeof(uint64_t) + (1u << 17);      // struct section: generous bound
    const std::vector<bool> lazy = lazy_allocs(M);
    for (size_t i = 0; i < M->allocs.size(); ++i) if (!lazy[i]) total += (M->alloc_bytes[i] + 255) / 256 * 256;
    return total + 256;
}

// the model section of M; false: a model pointer lies outside the model's allocations
static bool save_section(const wt_model* M, std::vector<char>* st) {
    std::map<const void*, int> index;
    for (size_t i = 0; i < M->allocs.size(); ++i) index[M->allocs[i]] = (int)i;
    Archive ar;
    ar.saving = true; ar.out = st; ar.index = &index;
    walk_model(const_cast<wt_model*>(M), ar);        // (saving modifies nothing)
    return ar.ok;
}

int model_export(const wt_model* M, void* buf, size_t n) {
    std::vector<char> st;
    if (!save_section(M, &st)) { set_error("wt_model_export: a model pointer lies outside the model's allocations"); return WT_ERR_INVALID; }
    PackHeader h{};
    h.magic = PACK_MAGIC; h.version = PACK_VERSION; h.arch = M->arch; h.arch_hash = arch_hash_of(M->arch);
    h.n_allocs = M->allocs.size(); h.struct_bytes = st.size();
    if (M->f32_stale.load()) if (int rc = ensure_f32_weights(M)) return rc;       // (nothing lazy is exported, but keep the model whole)
    const std::vector<bool> lazy = lazy_allocs(M);
    size_t pos = sizeof(PackHeader) + M->allocs.size() * sizeof(uint64_t) + st.size();
    pos = (pos + 255) / 256 * 256;
    const size_t payload0 = pos;
    for (size_t i = 0; i < M->allocs.size(); ++i) if (!lazy[i]) pos += (M->alloc_bytes[i] + 255) / 256 * 256;
    h.payload_bytes = pos - payload0;
    if (pos > n) { set_error("wt_model_export: buffer too small (wt_model_export_bytes)"); return WT_ERR_INVALID; }
    char* o = static_cast<char*>(buf);
    std::memset(o, 0, payload0);
    for (size_t i = 0; i < M->allocs.size(); ++i) { uint64_t b = M->alloc_bytes[i] | (lazy[i] ? PACK_NOT_STORED : 0); std::memcpy(o + sizeof(h) + i * 8, &b, 8); }
    std::memcpy(o + sizeof(h) + M->allocs.size() * 8, st.data(), st.size());
    pos = payload0;
    WT_HIP_CHECK(hipDeviceSynchronize());
    for (size_t i = 0; i < M->allocs.size(); ++i) {
        if (lazy[i]) continue;
        const size_t b = M->alloc_bytes[i], padded = (b + 255) / 256 * 256;
        WT_HIP_CHECK(hipMemcpy(o + pos, M->allocs[i], b, hipMemcpyDeviceToHost));
        std::memset(o + pos + b, 0, padded - b);
        pos += padded;
    }
    h.body_hash = body_hash_of(o + sizeof(h), pos - sizeof(h));
    std::memcpy(o, &h, sizeof(h));
    return (int)0;
}

int packed_info(const void* buf, size_t n, wt_arch* arch, int32_t* version, uint64_t* arch_hash) {
    if (!buf || n < sizeof(PackHeader)) { set_error("packed image: too short"); return WT_ERR_INVALID; }
    PackHeader h;
    std::memcpy(&h, buf, sizeof(h));
    if (h.magic != PACK_MAGIC) { set_error("packed image: bad magic (not a wavtokenizer_amd packed file)"); return WT_ERR_INVALID; }
    if (version) *version = h.version;
    if (arch) *arch = h.arch;
    if (arch_hash) *arch_hash = h.arch_hash;
    if (h.version != PACK_VERSION) { set_error("packed image: layout version " + std::to_string(h.version) + ", this library reads " + std::to_string(PACK_VERSION)); return WT_ERR_INVALID; }
    if (h.arch_hash != arch_hash_of(h.arch)) { set_error("packed image: architecture hash mismatch (corrupt header)"); return WT_ERR_INVALID; }
    if (int rc = check_arch(h.arch)) return rc;
    // every term is checked against what is left of the file before it is added: nothing here can wrap
    size_t left = n - sizeof(PackHeader);
    if (h.n_allocs > (1u << 16) || h.n_allocs * 8 > left) { set_error("packed image: truncated (allocation table)"); return WT_ERR_INVALID; }
    left -= h.n_allocs * 8;
    if (h.struct_bytes > (1u << 24) || h.struct_bytes > left) { set_error("packed image: truncated (model section)"); return WT_ERR_INVALID; }
    const size_t head = sizeof(PackHeader) + h.n_allocs * 8 + h.struct_bytes, head_pad = (head + 255) / 256 * 256;
    if (head_pad > n || h.payload_bytes > n - head_pad) { set_error("packed image: truncated (payload)"); return WT_ERR_INVALID; }
    return WT_OK;
}

// length of the image that starts at buf (wt_model_export_bytes is an upper bound taken before the model section is written)
size_t packed_bytes(const void* buf, size_t n) {
    if (packed_info(buf, n, nullptr, nullptr, nullptr)) return 0;
    PackHeader h;
    std::memcpy(&h, buf, sizeof(h));
    return (sizeof(PackHeader) + h.n_allocs * 8 + h.struct_bytes + 255) / 256 * 256 + h.payload_bytes;
}

// full check of an image that needs no GPU: header, table and section bounds, and the hash of everything behind the header
int packed_verify(const void* buf, size_t n) {
    if (int rc = packed_info(buf, n, nullptr, nullptr, nullptr)) return rc;
    PackHeader h;
    std::memcpy(&h, buf, sizeof(h));
    const char* in = static_cast<const char*>(buf);
    const size_t head_pad = (sizeof(PackHeader) + h.n_allocs * 8 + h.struct_bytes + 255) / 256 * 256;
    size_t pos = head_pad;
    for (size_t i = 0; i < h.n_allocs; ++i) {
        uint64_t b;
        std::memcpy(&b, in + sizeof(h) + i * 8, 8);
        if (b & PACK_NOT_STORED) {               // allocated on import, filled in later (wt_model::lazy_f32): bounded, no payload
            if ((b & ~PACK_NOT_STORED) == 0 || (b & ~PACK_NOT_STORED) > (1ull << 32)) { set_error("packed image: bad size of an unstored array"); return WT_ERR_INVALID; }
            continue;
        }
        if (b == 0 || b > n - pos || (b + 255) / 256 * 256 > n - pos) { set_error("packed image: allocation table does not fit the payload"); return WT_ERR_INVALID; }
        pos += (b + 255) / 256 * 256;
    }
    if (pos - head_pad != h.payload_bytes) { set_error("packed image: allocation table and payload size disagree"); return WT_ERR_INVALID; }
    if (body_hash_of(in + sizeof(h), pos - sizeof(h)) != h.body_hash) { set_error("packed image: content hash mismatch (corrupt file)"); return WT_ERR_INVALID; }
    return WT_OK;
}

// The GPU-free half of model_import: given M->arch and the allocation table (M->allocs, M->alloc_bytes), parse the model
// section into M, check the lazy list and validate.  Nothing is dereferenced.
static int import_section(wt_model* M, const char* sec, size_t n) {
    if (int rc = check_arch(M->arch)) return rc;
    Archive ar;
    ar.saving = false; ar.in = sec; ar.n = n; ar.allocs = &M->allocs; ar.alloc_bytes = &M->alloc_bytes;
    walk_model(M, ar);
    if (!ar.ok || ar.pos != ar.n) { set_error("packed image: model section does not match this library's layout"); return WT_ERR_INVALID; }
    // every lazy entry must name whole arrays of plausible size (the file is not trusted)
    for (const wt_model::LazyF32& z : M->lazy_f32) {
        size_t iw = M->allocs.size(), is = M->allocs.size();
        for (size_t i = 0; i < M->allocs.size(); ++i) {
            if (M->allocs[i] == static_cast<const void*>(z.w)) iw = i;
            if (z.s32 && M->allocs[i] == z.s32) is = i;
        }
        if (iw == M->allocs.size() || z.n <= 0 || (z.n % 32) || (size_t)z.n * 4 > M->alloc_bytes[iw] ||
            (z.s32 && (is == M->allocs.size() || (size_t)z.n * 4 > M->alloc_bytes[is])) || !(z.scale > 0.f) || !std::isfinite(z.scale)) {
            set_error("packed image: bad entry in the list of unstored fp32 arrays"); return WT_ERR_INVALID;
        }
    }
    return validate_imported(M);
}

int model_import(wt_model* M, const void* buf, size_t n) {
    PackHeader h;
    if (int rc = packed_verify(buf, n)) return rc;
    std::memcpy(&h, buf, sizeof(h));
    M->arch = h.arch;
    const char* in = static_cast<const char*>(buf);
    size_t pos = (sizeof(PackHeader) + h.n_allocs * 8 + h.struct_bytes + 255) / 256 * 256;
    for (size_t i = 0; i < h.n_allocs; ++i) {
        uint64_t b;
        std::memcpy(&b, in + sizeof(h) + i * 8, 8);
        const bool stored = !(b & PACK_NOT_STORED);
        b &= ~PACK_NOT_STORED;
        const size_t padded = (b + 255) / 256 * 256;
        if (stored && pos + padded > n) { set_error("packed image: truncated payload"); return WT_ERR_INVALID; }
        void* d = nullptr;
        WT_HIP_CHECK(hipMalloc(&d, b));
        M->allocs.push_back(d);
        M->alloc_bytes.push_back(b);
        if (stored) {
            WT_HIP_CHECK(hipMemcpy(d, in + pos, b, hipMemcpyHostToDevice));
            pos += padded;
        } else {
            M->f32_stale.store(true);
        }
    }
    return import_section(M, in + sizeof(h) + h.n_allocs * 8, h.struct_bytes);
}

}  // namespace wt
