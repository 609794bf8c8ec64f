// The extern "C" entry points declared in include/wavtokenizer_amd.h: models and plans (create, destroy, export, introspection).
// Running a plan is run.cpp; the entry points that launch kernels outside a plan are probe.cpp.
#include "model.h"

namespace wt {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
thread_local LaunchCtx g_launch;
int device_cus() {
    static std::atomic<int> cache[64];
    int d = 0;
    (void)hipGetDevice(&d);
    d &= 63;
    int v = cache[d].load(std::memory_order_relaxed);
    if (v <= 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) v = 256;
        cache[d].store(v, std::memory_order_relaxed);
    }
    return v;
}
bool full_chip(int device) {
    int cus = 0;
    return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus == 256;
}
}  // namespace wt

// ================================================================================== C ABI
using namespace wt;

// a zeroed host-mapped block and its device address (the status words that kernels write and the host reads without a copy)
static int alloc_host_words(size_t bytes, unsigned** host, unsigned** dev, const char* who) {
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, bytes, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        set_error(std::string(who) + ": no host-mapped memory for the status words");
        return WT_ERR_HIP;
    }
    memset(hp, 0, bytes);
    *host = static_cast<unsigned*>(hp);
    *dev = static_cast<unsigned*>(dp);
    return WT_OK;
}
// one block per model: word 0 = wt_codes_to_features' bad-index flag, word 16 = the model-level call status
static int alloc_model_words(wt_model* M, const char* who) {
    if (int rc = alloc_host_words(256, &M->bad_codes_host, &M->bad_codes_dev, who)) return rc;
    M->status_host = M->bad_codes_host + 16;
    M->status_dev = M->bad_codes_dev + 16;
    return WT_OK;
}
static void free_model(wt_model* m) {
    for (void* p : m->allocs) (void)hipFree(p);
    for (void* p : m->load_tmp) (void)hipFree(p);
    for (void* p : m->rvq.allocs) (void)hipFree(p);
    if (m->bad_codes_host) (void)hipHostFree(m->bad_codes_host);
}

// The library holds gfx950 code objects only.  Launch geometry follows the device's CU count (device_cus()); what is tied to
// the full 256-CU / 8-XCD MI355X is the persistent LSTM (plan.cpp: any other CU count runs the launch-per-step kernel) and
// the tuning of the tile orders (speed only).  A device of another architecture is refused here instead of at the first launch.
static int check_device(int device, const char* who) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); set_error(std::string(who) + ": no such device"); return WT_ERR_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string(who) + ": device is " + prop.gcnArchName + "; this library is built for gfx950 (MI355X) only");
        return WT_ERR_INVALID;
    }
    if (prop.multiProcessorCount < 8) { set_error(std::string(who) + ": fewer than 8 compute units"); return WT_ERR_INVALID; }
    return WT_OK;
}

extern "C" {

const char* wt_last_error(void) { return g_err.c_str(); }
#ifdef WT_LAB
const char* wt_version(void) { return "wavtokenizer_amd 0.1 LAB build (gfx950, split-f16 MFMA products, fp32 accumulation; timing experiments and fault hooks compiled in)"; }
#else
const char* wt_version(void) { return "wavtokenizer_amd 0.1 (gfx950, split-f16 MFMA products, fp32 accumulation)"; }
#endif

int wt_model_create(const wt_arch* arch, const wt_tensor* tensors, int32_t n_tensors, int32_t device, wt_model** out) {
    if (!arch || !tensors || !out) { set_error("wt_model_create: null argument"); return WT_ERR_INVALID; }
    // every rule on the architecture is made here, before any HIP call (packed.cpp arch_refusal: the same rule for packed images)
    { const std::string why = arch_refusal(*arch); if (!why.empty()) { set_error(why); return WT_ERR_INVALID; } }
    DeviceGuard dg(device);
    if (!dg.ok) { set_error("wt_model_create: hipSetDevice failed"); return WT_ERR_HIP; }
    if (int rc = check_device(device, "wt_model_create")) return rc;
    std::unique_ptr<wt_model> M(new wt_model());
    M->arch = *arch;
    M->device = device;
    M->hop = 1;
    for (int i = 0; i < arch->n_ratios; ++i) M->hop *= arch->ratios[i];
    for (int i = arch->n_ratios - 1; i >= 0; --i) M->enc_ratios.push_back(arch->ratios[i]);   // seanet.py:100
    TensorMap tm;
    for (int i = 0; i < n_tensors; ++i) tm.m[tensors[i].name] = {tensors[i].data, tensors[i].numel};
    int rc = build_model(M.get(), tm);
    if (!rc) rc = build_splits(M.get());
    if (!rc) rc = alloc_model_words(M.get(), "wt_model_create");
    if (rc) {
        if (rc == WT_ERR_MISSING_TENSOR) set_error("state_dict tensor missing or mis-shaped: " + tm.missing);
        free_model(M.get());
        return rc;
    }
    *out = M.release();
    return WT_OK;
}

size_t wt_model_export_bytes(const wt_model* m) { return m ? model_export_bytes(m) : 0; }
int wt_model_export(const wt_model* m, void* buf, size_t n) {
    if (!m || !buf) { set_error("wt_model_export: null argument"); return WT_ERR_INVALID; }
    DeviceGuard dg(m->device);
    if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
    return model_export(m, buf, n);
}
int wt_packed_info(const void* buf, size_t n, wt_arch* arch, int32_t* version, uint64_t* arch_hash) {
    return packed_info(buf, n, arch, version, arch_hash);
}
size_t wt_packed_bytes(const void* buf, size_t n) { return buf ? packed_bytes(buf, n) : 0; }
int wt_packed_verify(const void* buf, size_t n) {
    try { return packed_verify(buf, n); }
    catch (const std::exception& e) { set_error(std::string("wt_packed_verify: ") + e.what()); return WT_ERR_INVALID; }
}
int wt_model_create_packed(const void* buf, size_t n, int32_t device, wt_model** out) {
    if (!buf || !out) { set_error("wt_model_create_packed: null argument"); return WT_ERR_INVALID; }
    if (int rc = packed_info(buf, n, nullptr, nullptr, nullptr)) return rc;
    DeviceGuard dg(device);
    if (!dg.ok) { set_error("wt_model_create_packed: hipSetDevice failed"); return WT_ERR_HIP; }
    if (int rc = check_device(device, "wt_model_create_packed")) return rc;
    std::unique_ptr<wt_model> M(new wt_model());
    M->device = device;
    int rc;
    try { rc = model_import(M.get(), buf, n); }      // nothing may throw across the C boundary (a bad file must not end the process)
    catch (const std::exception& e) { set_error(std::string("wt_model_create_packed: ") + e.what()); rc = WT_ERR_INVALID; }
    if (!rc) rc = alloc_model_words(M.get(), "wt_model_create_packed");
    if (rc) { free_model(M.get()); return rc; }
    *out = M.release();
    return WT_OK;
}

void wt_model_destroy(wt_model* m) {
    if (!m) return;
    DeviceGuard dg(m->device);
    free_model(m);
    delete m;
}
int wt_model_split_ok(const wt_model* m) { return m && m->s32_ok ? 1 : 0; }
int wt_model_take_bad_codes(const wt_model* m) {
    if (!m || !m->bad_codes_host) return 0;
    const unsigned v = __atomic_exchange_n(m->bad_codes_host, 0u, __ATOMIC_RELAXED);
    return v ? 1 : 0;
}
int wt_model_status(const wt_model* m, int32_t* bits, int32_t clear) {
    if (!m) return WT_ERR_INVALID;
    unsigned b = 0;
    if (m->status_host) b = clear ? __atomic_exchange_n(m->status_host, 0u, __ATOMIC_ACQUIRE) : __atomic_load_n(m->status_host, __ATOMIC_ACQUIRE);
    if (b & WT_STATUS_LSTM) m->persist_ok.store(false);
    if (bits) *bits = (int32_t)b;
    return WT_OK;
}
int wt_model_persistent_lstm(const wt_model* m) {
    return m && m->persist_ok.load() && full_chip(m->device) ? 1 : 0;
}
int wt_device_info(int32_t device, int32_t* compute_units, int32_t* is_gfx950, int32_t* persistent_lstm) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); set_error("wt_device_info: no such device"); return WT_ERR_HIP; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (is_gfx950) *is_gfx950 = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
    if (persistent_lstm) *persistent_lstm = full_chip(device) ? 1 : 0;
    return WT_OK;
}
int wt_model_weight_count(const wt_model* m) { return m ? (int)model_weights(m).size() : 0; }
int wt_model_weight_info(const wt_model* m, int32_t index, wt_weight_info* out) {
    if (!m || !out || out->size != (int32_t)sizeof(wt_weight_info)) { set_error("wt_model_weight_info: null argument or a descriptor of another size"); return WT_ERR_INVALID; }
    const std::vector<WeightEntry> all = model_weights(m);
    if (index < 0 || index >= (int)all.size()) { set_error("wt_model_weight_info: index out of range"); return WT_ERR_INVALID; }
    const WeightEntry& e = all[index];
    if (e.lazy == 1 && m->f32_stale.load()) {       // a packed model holds nothing there yet
        DeviceGuard dg(m->device);
        if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
        if (int rc = ensure_f32_weights(m)) return rc;
    }
    wt_weight_info w{};
    w.size = (int32_t)sizeof(wt_weight_info);
    w.format = e.format;
    std::strncpy(w.name, e.name.c_str(), sizeof(w.name) - 1);
    std::strncpy(w.of, e.of.c_str(), sizeof(w.of) - 1);
    w.data = e.data; w.numel = e.numel; w.ndim = e.ndim; w.tap_pair = e.tap_pair ? 1 : 0;
    for (int i = 0; i < 4; ++i) w.dims[i] = e.dims[i];
    w.acc_scale = e.acc_scale; w.lazy_scale = e.lazy_scale; w.lazy = e.lazy; w.archived = e.archived ? 1 : 0; w.alloc = e.alloc;
    *out = w;
    return WT_OK;
}
int wt_model_codebook_tables(const wt_model* m, int32_t k, const void** s32, const float** ee, float* acc_scale) {
    if (!m || k < 0 || k >= m->arch.num_quantizers) { set_error("wt_model_codebook_tables: no model, or k outside [0, num_quantizers)"); return WT_ERR_INVALID; }
    S32Copy c = m->embed.s32;
    const float* e = m->ee;
    if (k > 0) {
        DeviceGuard dg(m->device);
        if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
        if (int rc = ensure_rvq_tables(m)) return rc;
        c = m->rvq.s32[k - 1]; e = m->rvq.ee[k - 1];
    }
    if (s32) *s32 = c.p;
    if (ee) *ee = e;
    if (acc_scale) *acc_scale = c.acc_scale;
    return WT_OK;
}
int wt_model_hop(const wt_model* m) { return m ? m->hop : 0; }
int64_t wt_model_weight_bytes(const wt_model* m) { return m ? m->weight_bytes : 0; }

int wt_plan_create(const wt_model* m, int32_t kind, int32_t B, int64_t len, int32_t flags, wt_plan** out) {
    return wt_plan_create_ex(m, kind, B, len, flags, 0, out);
}

// The builder of each plan kind and what creation needs to know before it runs; what a call of the kind writes the builder
// records on the plan (plan.cpp).  (The argument checks above still tell encode plans, whose length is in samples, from the rest.)
struct PlanKind {
    int kind;
    int (*build)(wt_plan*);
    int whole_site;      // wt_plan::whole_site
    bool istft;          // ends in the ISTFT head, whose padding='center' needs two frames
    bool samples;        // `len` counts samples, not frames
};
static const PlanKind kPlanKinds[] = {
    {WT_PLAN_ENCODE, build_encode, SITE_ENC, false, true},  {WT_PLAN_DECODE, build_decode, -1, true, false},
    {WT_PLAN_SEANET_DECODER, build_seanet_decoder, SITE_SEADEC, false, false},  {WT_PLAN_HEAD, build_head, SITE_HEAD, true, false},
    {WT_PLAN_UNIT_LSTM, build_unit_lstm, SITE_ENC, false, false},
    {WT_PLAN_DECODE_MIXED, build_decode, -1, true, false},      // build_decode with the clip lengths threaded to its steps
    // build_decode with its first step replaced: bb.in gathered from the call's codes instead of transposed from its features
    {WT_PLAN_DECODE_CODES, build_decode, -1, true, false},  {WT_PLAN_DECODE_CODES_MIXED, build_decode, -1, true, false},
    {WT_PLAN_QUANTIZE, build_quantize, SITE_ENC, false, false},     // the residual VQ rounds alone, on the caller's features
};

int wt_plan_create_ex(const wt_model* m, int32_t kind, int32_t B, int64_t len, int32_t flags, uint64_t fp32_sites, wt_plan** out) {
    if (!m || !out) { set_error("wt_plan_create: null argument"); return WT_ERR_INVALID; }
    if (m->arch.num_layers > SITE_HEAD - SITE_CNX0) { set_error("wt_plan_create: more ConvNeXt blocks than range sites"); return WT_ERR_INVALID; }
    if (B < 1 || len < 1) { set_error("wt_plan_create: B and len must be >= 1"); return WT_ERR_INVALID; }
    if ((flags & WT_PLAN_FLAG_MIXED_LENGTH) && kind != WT_PLAN_ENCODE) {
        set_error("wt_plan_create: WT_PLAN_FLAG_MIXED_LENGTH is an encode-plan flag"); return WT_ERR_INVALID;
    }
    if ((flags & WT_PLAN_FLAG_RVQ) && kind != WT_PLAN_ENCODE) {
        set_error("wt_plan_create: WT_PLAN_FLAG_RVQ is an encode-plan flag (WT_PLAN_QUANTIZE runs the rounds on features)"); return WT_ERR_INVALID;
    }
    if (kind == WT_PLAN_QUANTIZE) {
        const struct { int flag; const char* name; } refused[] = {
            {WT_PLAN_FLAG_UNFUSED, "WT_PLAN_FLAG_UNFUSED"}, {WT_PLAN_FLAG_STEP_LSTM, "WT_PLAN_FLAG_STEP_LSTM"},
            {WT_PLAN_FLAG_MIXED_LENGTH, "WT_PLAN_FLAG_MIXED_LENGTH"}, {WT_PLAN_FLAG_F16_GEMM, "WT_PLAN_FLAG_F16_GEMM"}};
        for (const auto& r : refused)
            if (flags & r.flag) { set_error(std::string("wt_plan_create: ") + r.name + " has no meaning for WT_PLAN_QUANTIZE"); return WT_ERR_INVALID; }
    }
    if (flags & WT_PLAN_FLAG_F16_GEMM) {
        const bool decode_kind = kind == WT_PLAN_DECODE || kind == WT_PLAN_DECODE_MIXED || kind == WT_PLAN_DECODE_CODES ||
                                 kind == WT_PLAN_DECODE_CODES_MIXED;
        if (!decode_kind) { set_error("wt_plan_create: WT_PLAN_FLAG_F16_GEMM is a flag of the decode plan kinds"); return WT_ERR_INVALID; }
        if (flags & (WT_PLAN_FLAG_FP32_GEMM | WT_PLAN_FLAG_UNFUSED)) {
            set_error("wt_plan_create: WT_PLAN_FLAG_F16_GEMM does not combine with WT_PLAN_FLAG_FP32_GEMM or WT_PLAN_FLAG_UNFUSED");
            return WT_ERR_INVALID;
        }
    }
    if ((len + (kind == WT_PLAN_ENCODE ? m->hop - 1 : 0)) / (kind == WT_PLAN_ENCODE ? m->hop : 1) > 12000) {
        set_error("clips longer than 12000 frames are not supported by one plan; split the clip"); return WT_ERR_INVALID;
    }
    DeviceGuard dg(m->device);
    if (!dg.ok) { set_error("wt_plan_create: hipSetDevice failed"); return WT_ERR_HIP; }
    std::unique_ptr<wt_plan> P(new wt_plan());
    P->model = m; P->kind = kind; P->B = B; P->len = len; P->flags = flags; P->fp32_sites = fp32_sites;
    // word 0: status bits; words 2, 3: mask of the range sites that reported
    if (int rc0 = alloc_host_words(64, &P->status_host, &P->status_dev, "wt_plan_create")) return rc0;
    // a model that came from a packed image holds no fp32 copies of its GEMM weights until a plan needs them
    if (m->f32_stale.load() && ((flags & (WT_PLAN_FLAG_FP32_GEMM | WT_PLAN_FLAG_UNFUSED)) || fp32_sites || !m->s32_ok ||
                                (kind == WT_PLAN_SEANET_DECODER && !m->sd_s32_ok)))
        if (int rc0 = ensure_f32_weights(m)) return rc0;
    plan_begin(P.get());
    const PlanKind* pk = std::find_if(std::begin(kPlanKinds), std::end(kPlanKinds), [&](const PlanKind& k) { return k.kind == kind; });
    if (pk == std::end(kPlanKinds)) { set_error("unknown plan kind"); return WT_ERR_INVALID; }
    if (pk->samples) { P->T = len; P->L = (len + m->hop - 1) / m->hop; }
    else { P->L = len; P->T = len * m->hop; }
    if (pk->samples && (long)B * len >= (long)INT_MAX) { set_error("batch too large for one plan (32-bit row index)"); return WT_ERR_INVALID; }
    if (pk->istft && !m->arch.padding_same && len < 2) { set_error("ISTFT padding='center' needs at least two frames"); return WT_ERR_INVALID; }
    P->whole_site = pk->whole_site;
    P->cur_site = std::max(pk->whole_site, 0);
    int rc = pk->build(P.get());
    if (!rc) rc = P->build_rc;
    if (rc) return rc;              // ~wt_plan releases the host-mapped word
    plan_end(P.get());
    P->layout();
    if (!P->range_entries.empty()) {
        if (hipMalloc(reinterpret_cast<void**>(&P->range_dev), (P->range_entries.size() * sizeof(unsigned) + 15) / 16 * 16) != hipSuccess) {
            P->range_dev = nullptr; set_error("wt_plan_create: no memory for the range report"); return WT_ERR_HIP;
        }
        P->range_host.assign(P->range_entries.size(), 0.f);
    }
    *out = P.release();
    return WT_OK;
}
void wt_plan_destroy(wt_plan* p) {
    if (!p) return;
    DeviceGuard dg(p->model->device);
    delete p;
}
size_t wt_plan_workspace_bytes(const wt_plan* p) { return p ? p->ws_bytes : 0; }
int64_t wt_plan_frames(const wt_plan* p) { return p ? p->L : 0; }
int64_t wt_plan_min_clip_length(const wt_plan* p) { return p && (p->flags & WT_PLAN_FLAG_MIXED_LENGTH) ? p->min_clip : 0; }
int wt_sconv_geometry(int64_t T, int32_t k, int32_t stride, int32_t dilation, int32_t out[4]) {
    if (!out || T < 1 || k < 1 || stride < 1 || dilation < 1 || (int64_t)(k - 1) * dilation + 1 < stride || T >= INT_MAX) {
        set_error("wt_sconv_geometry: needs T, k, stride, dilation >= 1 and an effective kernel no shorter than the stride");
        return WT_ERR_INVALID;
    }
    const SConvGeom g = sconv_geom((long)T, k, stride, dilation);
    out[0] = g.pl; out[1] = g.pr_total; out[2] = g.Tout; out[3] = g.Tp;
    return WT_OK;
}
int wt_plan_num_launches(const wt_plan* p) { return p ? p->n_launches : 0; }

int wt_plan_find_buffer(const wt_plan* p, const char* name, size_t* offset, size_t* numel) {
    return wt_plan_buffer_info(p, name, offset, numel, nullptr);
}
int wt_plan_buffer_info(const wt_plan* p, const char* name, size_t* offset, size_t* numel, int32_t* format) {
    if (!p || !name) return WT_ERR_INVALID;
    for (const BufSpec& b : p->bufs)
        if (b.name == name) {
            if (offset) *offset = b.off;
            if (numel) *numel = b.numel;
            if (format) *format = b.fmt;
            return WT_OK;
        }
    set_error(std::string("no stage buffer named ") + name);
    return WT_ERR_INVALID;
}
int wt_plan_buffer_name(const wt_plan* p, int32_t index, const char** name) {
    if (!p || index < 0 || index >= (int)p->bufs.size()) return WT_ERR_INVALID;
    *name = p->bufs[index].name.c_str();
    return WT_OK;
}

int wt_plan_num_steps(const wt_plan* p) { return p ? (int)p->steps.size() : 0; }
int wt_plan_step_name(const wt_plan* p, int32_t index, const char** name) {
    if (!p || index < 0 || index >= (int)p->step_names.size()) return WT_ERR_INVALID;
    *name = p->step_names[index].c_str();
    return WT_OK;
}

}  // extern "C"
