// CPU check of the packed image's model section (wavtokenizer_amd/csrc/packed.cpp): the walk, the archive, the validator
// and the lister on a synthetic model.  No GPU, no image file, no hash, no HIP call: every "device" array is an allocation
// of exactly its expected size in a made-up address space, and nothing on these paths dereferences one.
//   packed_section_check FILE      FILE: (wt_arch, int32 has_seadec) records, back to back (tests/test_packed_section_host.py writes it)
// Prints one line of counts per architecture; exit status 0 when every check held.
#include "../../wavtokenizer_amd/csrc/packed.cpp"

#include <cstdio>
#include <fstream>
#include <limits>

namespace wt {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
bool resblock_fusable(int C) { return C == 32 || C == 64; }      // resblock.hip's rule
int ensure_f32_weights(const wt_model*) { return WT_OK; }        // (model_export's; never reached here)
}  // namespace wt
using namespace wt;

static int g_failed = 0;
#define CHECK(cond, what)                                                                         \
    do {                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s [%s] (last error: %s)\n", __LINE__, #cond, std::string(what).c_str(), g_err.c_str()); } \
    } while (0)

static const char* const REFUSAL = " does not match the architecture in its header";
static const char* const LAYOUT = "packed image: model section does not match this library's layout";
static const char* const LAZY = "packed image: bad entry in the list of unstored fp32 arrays";
static bool refused_naming(int rc, const std::string& name) { return rc != 0 && g_err == "packed image: " + name + REFUSAL; }

// The fourth visitor: a wt_arch -> a model with every array the architecture calls for, every pod at its expected value
struct Builder {
    wt_model* M;
    uintptr_t next = 0x100000000ull;
    void* alloc(size_t bytes) {
        void* p = reinterpret_cast<void*>(next);
        M->allocs.push_back(p);
        M->alloc_bytes.push_back(bytes);
        next += (bytes + 511) / 256 * 256;         // at least 256 bytes that belong to no allocation behind each
        return p;
    }
    template <class T> void pod(T&) {}
    template <class T> void ref(T*&) {}
    void dim(int& v, int want, const std::string&) { v = want; }
    template <class T> size_t count(std::vector<T>& x, int32_t, int want, const char*) { if (want >= 0) x.resize(want); return x.size(); }
    template <class T> void arr(const std::string&, T*& p, int fmt, const Dims& d, bool = false) { p = static_cast<T*>(alloc(d.bytes(fmt))); }
    void copy(const std::string&, const std::string&, S32Copy& s, const Dims& d, bool pair_ok) {
        s.p = alloc(d.bytes(WFMT_S32));
        s.acc_scale = 1.f;
        s.tap_pair = pair_ok && d.d[1] <= 32;      // build_splits: the down convs with k = 2r <= 32
        if (s.tap_pair) M->lazy_f32.push_back({static_cast<const float*>(alloc(d.bytes(WFMT_F32))), nullptr, (int64_t)(d.bytes(WFMT_F32) / 4), 1.f});
    }
    bool optional(bool, bool expected) { return expected; }
};

// changes the target-th pod that has an expected value by delta
struct PodPoke {
    int target, delta, seen = 0;
    int* hit = nullptr;
    std::string name;
    template <class T> void pod(T&) {}
    template <class T> void ref(T*&) {}
    void dim(int& v, int, const std::string& n) { if (seen++ == target) { v += delta; hit = &v; name = n; } }
    template <class T> size_t count(std::vector<T>& x, int32_t, int, const char*) { return x.size(); }
    template <class T> void arr(const std::string&, T*&, int, const Dims&, bool = false) {}
    void copy(const std::string&, const std::string&, S32Copy&, const Dims&, bool) {}
    bool optional(bool present, bool) { return present; }
};

static void build(wt_model* M, const wt_arch& a, bool seadec) {
    M->arch = a;
    M->has_seadec = seadec;
    Builder b{M};
    walk_model(M, b);
    // one array that the image leaves out and rebuilds from its copy, beside the tap-paired repackings
    M->lazy_f32.push_back({M->enc_final.w, M->enc_final.s32.p, (int64_t)512 * 512 * 7, 1.f});
}

// the inner import on a fresh model over a given allocation table
static int load(const wt_model& like, const std::vector<char>& sec, wt_model* out) {
    out->arch = like.arch; out->allocs = like.allocs; out->alloc_bytes = like.alloc_bytes;
    g_err.clear();
    return import_section(out, sec.data(), sec.size());
}
static int load(const wt_model& like, const std::vector<char>& sec) { wt_model t; return load(like, sec, &t); }
static int validate(const wt_model& M) { g_err.clear(); return validate_imported(&M); }

static bool same_entry(const WeightEntry& x, const WeightEntry& y) {
    return x.name == y.name && x.of == y.of && x.data == y.data && x.numel == y.numel && x.ndim == y.ndim && std::equal(x.dims, x.dims + 4, y.dims) &&
           x.format == y.format && x.acc_scale == y.acc_scale && x.tap_pair == y.tap_pair && x.lazy == y.lazy && x.lazy_scale == y.lazy_scale &&
           x.archived == y.archived && x.alloc == y.alloc;
}

static void check_arch_case(int index, const wt_arch& a, bool seadec) {
    wt_model A;
    build(&A, a, seadec);
    // 1. the synthetic model validates
    CHECK(validate(A) == 0, "the synthetic model");
    // 2. round trip
    std::vector<char> sec, again;
    CHECK(save_section(&A, &sec), "save");
    wt_model B;
    CHECK(load(A, sec, &B) == 0, "load");
    CHECK(save_section(&B, &again) && again == sec, "saving the loaded model gives other bytes");
    const std::vector<WeightEntry> ents = model_weights(&A), ents_b = model_weights(&B);
    CHECK(ents.size() == ents_b.size() && std::equal(ents.begin(), ents.end(), ents_b.begin(), same_entry), "the listings of the two models differ");
    // 3. one byte short, one byte more
    std::vector<char> t(sec.begin(), sec.end() - 1);
    CHECK(load(A, t) != 0 && g_err == LAYOUT, "a section one byte short");
    t = sec; t.push_back(0);
    CHECK(load(A, t) != 0 && g_err == LAYOUT, "a section with a byte appended");
    // 4. every array the lister names, with its allocation one word shorter
    int tried = 0, copies = 0;
    for (const WeightEntry& e : ents) {
        CHECK(e.alloc >= 0 && e.archived && A.alloc_bytes[e.alloc] == (size_t)e.numel * 4, e.name);
        if (e.alloc < 0) continue;
        bool in_lazy = false;
        for (const wt_model::LazyF32& z : A.lazy_f32) in_lazy = in_lazy || z.w == e.data || z.s32 == e.data;
        A.alloc_bytes[e.alloc] -= 4;
        const int rc = load(A, sec);
        // (an allocation of no bytes at all holds no pointer: the archive refuses the record itself)
        CHECK(rc != 0 && (g_err == "packed image: " + e.name + REFUSAL || (in_lazy && g_err == LAZY) || (A.alloc_bytes[e.alloc] == 0 && g_err == LAYOUT)), e.name);
        if (e.lazy != 2) CHECK(refused_naming(validate(A), e.name), e.name);       // (2: held by the lazy list alone, which import_section checks)
        A.alloc_bytes[e.alloc] += 4;
        ++tried;
        copies += e.format == WFMT_S32;
    }
    CHECK(tried == (int)ents.size() && validate(A) == 0, "arrays tried");
    // 5. single mutations
    int pods = 0, mutations = 0;
    for (;; ++pods) {
        bool any = false;
        for (int delta : {-1, 1}) {
            PodPoke pk{pods, delta};
            walk_model(&A, pk);
            if (!pk.hit) break;
            any = true;
            CHECK(refused_naming(validate(A), pk.name), pk.name);
            *pk.hit -= delta;
            ++mutations;
        }
        if (!any) break;
    }
    CHECK(pods > 0 && validate(A) == 0, "pods restored");
    const float inf = std::numeric_limits<float>::infinity();
    for (float bad : {0.f, -1.f, inf, std::numeric_limits<float>::quiet_NaN()}) {
        A.enc_final.s32.acc_scale = bad;
        CHECK(refused_naming(validate(A), "enc.final.s32"), "acc_scale of a conv copy");
        A.enc_final.s32.acc_scale = 1.f;
        A.head_W.s32.acc_scale = bad;
        CHECK(refused_naming(validate(A), "head.W.s32"), "acc_scale of a GEMM copy");
        A.head_W.s32.acc_scale = 1.f;
        mutations += 2;
    }
    A.enc_final.s32.tap_pair = true;
    CHECK(refused_naming(validate(A), "enc.final.s32"), "tap_pair on a conv that is no down conv");
    A.enc_final.s32.tap_pair = false;
    const std::vector<CnxBlock> cnx = A.cnx;
    for (int d : {-1, 1}) {
        A.cnx.resize(a.num_layers + d, A.cnx[0]);
        CHECK(refused_naming(validate(A), "the ConvNeXt block count"), "cnx count");
        std::vector<char> s;
        CHECK(save_section(&A, &s) && load(A, s) != 0, "cnx count through a section");
        A.cnx = cnx;
    }
    A.stages.resize(9);
    { std::vector<char> s; CHECK(save_section(&A, &s) && load(A, s) != 0 && g_err == LAYOUT, "a stage count of 9"); }
    A.stages.resize(a.n_ratios);
    const size_t n_lazy = A.lazy_f32.size();
    A.lazy_f32.resize(4097, A.lazy_f32[0]);
    { std::vector<char> s; CHECK(save_section(&A, &s) && load(A, s) != 0 && g_err == LAYOUT, "a lazy-list count of 4097"); }
    A.lazy_f32.resize(n_lazy, A.lazy_f32[0]);
    mutations += 5;
    // the first pointer record (enc.e0.w) lies behind hop, H, weight_bytes, s32_ok, sd_s32_ok, w_amax and the ratios
    const size_t rec = 4 + 4 + 8 + 1 + 1 + 4 + 4 + 4 * (size_t)a.n_ratios;
    int32_t idx;
    int64_t off;
    std::memcpy(&idx, &sec[rec], 4); std::memcpy(&off, &sec[rec + 4], 8);
    CHECK(idx == 0 && off == 0 && A.allocs[0] == A.e0_w, "the first pointer record is not where this program expects it");
    auto record = [&](int32_t i, int64_t o, const char* what) {
        std::vector<char> s = sec;
        std::memcpy(&s[rec], &i, 4); std::memcpy(&s[rec + 4], &o, 8);
        CHECK(load(A, s) != 0 && g_err == LAYOUT, what);
        ++mutations;
    };
    record((int32_t)A.allocs.size(), 0, "a pointer record with the index equal to the allocation count");
    record(0, -1, "a pointer record with a negative offset");
    record(0, (int64_t)A.alloc_bytes[0], "a pointer record with an offset equal to its allocation's size");
    auto lazy = [&](wt_model::LazyF32 z, const char* what) {
        std::swap(A.lazy_f32[0], z);
        std::vector<char> s;
        CHECK(save_section(&A, &s) && load(A, s) != 0 && g_err == LAZY, what);
        std::swap(A.lazy_f32[0], z);
        ++mutations;
    };
    const wt_model::LazyF32 z0 = A.lazy_f32[0];
    lazy({z0.w + 1, z0.s32, z0.n, z0.scale}, "a lazy entry that names no allocation base");
    lazy({z0.w, z0.s32, z0.n + 1, z0.scale}, "a lazy entry with n % 32 != 0");
    lazy({z0.w, z0.s32, z0.n, 0.f}, "a lazy entry with scale 0");
    lazy({z0.w, z0.s32, z0.n, -1.f}, "a lazy entry with a negative scale");
    again.clear();
    CHECK(validate(A) == 0 && save_section(&A, &again) && again == sec, "the model is as it was");
    std::printf("arch %d: arrays %d (fp32/LSTM %d, S32 copies %d) lister %d, pods %d, mutations %d, section %zu bytes, allocations %zu\n", index, tried,
                tried - copies, copies, (int)ents.size(), pods, mutations, sec.size(), A.allocs.size());
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: packed_section_check FILE\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.empty() || bytes.size() % (sizeof(wt_arch) + 4)) { std::printf("FILE must hold (wt_arch, int32 has_seadec) records\n"); return 2; }
    for (size_t i = 0; i * (sizeof(wt_arch) + 4) < bytes.size(); ++i) {
        wt_arch a;
        int32_t seadec;
        std::memcpy(&a, &bytes[i * (sizeof(wt_arch) + 4)], sizeof(a));
        std::memcpy(&seadec, &bytes[i * (sizeof(wt_arch) + 4) + sizeof(a)], 4);
        check_arch_case((int)i, a, seadec != 0);
    }
    if (g_failed) std::printf("%d checks FAILED\n", g_failed);
    else std::printf("all checks held\n");
    return g_failed ? 1 : 0;
}
