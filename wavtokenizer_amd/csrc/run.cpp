// Running a plan: the call status, the chain of persistent LSTM launches, graph replay, the one loop that issues the steps
// with its timing / range-report observer, the run entry points and the readers of what a run leaves behind.
#include "model.h"

using namespace wt;

// Consumes the failure bits that earlier calls left behind (the plan's lock is held).  Every plan's guard step reports
// into two host-mapped words: the plan's own (attribution: wt_plan_status) and the MODEL's, which is the one that makes
// the next call fail: a caller who never uses a plan twice (one new length per file) still meets the error on its next
// call, and a failure that another plan's call has already consumed and answered is not reported a second time when
// this plan runs again (its own word is then stale and is just cleared).  After a lost-co-residency report every plan
// of the model runs the LSTM one launch per step from now on (wt_model::persist_ok), and a recorded graph that holds a
// persistent launch is dropped.  Returns the model's bits; *own receives this plan's.
static unsigned consume_status(const wt_plan* p, unsigned* own = nullptr) {
    const wt_model* M = p->model;
    const unsigned pb = p->status_host ? __atomic_exchange_n(p->status_host, 0u, __ATOMIC_ACQUIRE) : 0u;
    const unsigned mb = M->status_host ? __atomic_exchange_n(M->status_host, 0u, __ATOMIC_ACQUIRE) : 0u;
    if ((mb | pb) & WT_STATUS_LSTM) M->persist_ok.store(false);
    if (p->graph_exec && p->graph_persist && !M->persist_ok.load()) {
        (void)hipGraphExecDestroy(p->graph_exec);
        p->graph_exec = nullptr; p->graph_persist = false;
        p->last_key = wt_plan::GraphKey{};
    }
    if (own) *own = pb;
    return mb;
}

// Two persistent LSTM launches must never share the GPU: lstm_persist_kernel spins until all of its workgroups are resident
// (one per CU), so two of them enqueued on different streams could each hold part of the CUs and wait for the rest until
// their spin bounds expire (both calls then fail with WT_ERR_LSTM_SYNC).  Calls that carry one are therefore chained per
// device: a call on another stream than the previous one first waits (on the GPU, hipStreamWaitEvent) for the event recorded
// behind that previous call.  The lock is held from the wait to the record, so concurrent host threads are ordered too.
// Kernels of other plans may run beside a persistent launch: they finish on their own and its workgroups then take their CUs.
struct LstmChain {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool any = false;       // a call has been made
    bool multi = false;     // calls have come from more than one stream: from then on every call records the event
    bool have = false;      // ev marks the end of the previous call
};
static LstmChain g_lstm_chain[64];
struct LstmChainScope {
    LstmChain* ch = nullptr;
    hipStream_t stream = nullptr;
    int rc = WT_OK;
    LstmChainScope(const wt_plan* p, hipStream_t s) {
        if (!p->uses_persist || p->model->device < 0 || p->model->device >= 64) return;
        ch = &g_lstm_chain[p->model->device];
        stream = s;
        ch->mu.lock();
        if (!ch->any || ch->last == s) return;
        if (!ch->ev && hipEventCreateWithFlags(&ch->ev, hipEventDisableTiming) != hipSuccess) { ch->ev = nullptr; return; }
        if (!ch->multi) {
            // first call from a second stream.  Single-stream callers never pay for an event record (it is a packet of its own
            // in the stream: 4-7 us), so there is none behind the previous call: order this one behind everything that stream
            // holds right now instead (conservative, once), and record from here on
            ch->multi = true;
            ch->have = hipEventRecord(ch->ev, ch->last) == hipSuccess;
            if (!ch->have) (void)hipGetLastError();      // (the stream may be gone: then so is its work)
        }
        if (ch->have && hipStreamWaitEvent(s, ch->ev, 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); rc = WT_ERR_HIP; }
    }
    ~LstmChainScope() {
        if (!ch) return;
        if (ch->multi) {
            if (!ch->ev && hipEventCreateWithFlags(&ch->ev, hipEventDisableTiming) != hipSuccess) ch->ev = nullptr;
            ch->have = ch->ev && hipEventRecord(ch->ev, stream) == hipSuccess;
        }
        ch->last = stream;
        ch->any = true;
        ch->mu.unlock();
    }
};

// What an eager run does around its steps beside issuing them: times the steps the timing filter names (with events, or with
// device stamps in the "@name" mode), measures the S32 ranges of a WT_PLAN_FLAG_RANGE_REPORT plan, and in LAB builds prints the
// step that left a status bit (WT_DEBUG_STATUS).
struct StepObserver {
    const wt_plan* p;
    const RunCtx& c;
    const bool timing, stamp, dbg_status;
    const std::string filt;
    size_t next_range = 0;
    bool timed = false;
    std::pair<hipEvent_t, hipEvent_t> ev;

    // "@name": no events - the step's gemm16s launch stamps its own entry / exit on the device (LaunchCtx).  An event record
    // is a packet of its own: bracketing a launch puts 4-7 us between it and its neighbours and counts them in (measured:
    // pwconv1 94.6 us between bracketing events, 88.7 us in the rocprofv3 trace of the same run; hipExtLaunchKernel's
    // start / stop events behave the same: 95.1 vs 90.3)
    StepObserver(const wt_plan* plan, const RunCtx& ctx)
        : p(plan), c(ctx), timing(!plan->timing_filter.empty()), stamp(timing && plan->timing_filter[0] == '@'),
          dbg_status(lab_env("WT_DEBUG_STATUS") != nullptr), filt(stamp ? plan->timing_filter.substr(1) : plan->timing_filter) {}
    // an untimed call of a plan without a range report has nothing to observe (LAB builds: unless WT_DEBUG_STATUS is set)
    static bool wanted(const wt_plan* p) { return !p->timing_filter.empty() || p->range_dev || lab_env("WT_DEBUG_STATUS"); }

    int before(size_t i) {
        timed = timing && p->step_names[i].find(filt) != std::string::npos;
        if (!timed) return 0;
        if (stamp) {
            if (p->stamps && p->stamp_next < wt_plan::STAMP_SLOTS) {
                g_launch.stamp_start = p->stamps + p->stamp_next;
                g_launch.stamp_end = p->stamps + wt_plan::STAMP_SLOTS + p->stamp_next;
                g_launch.stamp_used = false;
            }
            return 0;
        }
        if (!p->ev_free.empty()) { ev = p->ev_free.back(); p->ev_free.pop_back(); }
        else { WT_HIP_CHECK(hipEventCreate(&ev.first)); WT_HIP_CHECK(hipEventCreate(&ev.second)); }
        WT_HIP_CHECK(hipEventRecord(ev.first, c.stream));
        return 0;
    }
    int after(size_t i, int step_rc) {
        const bool armed = g_launch.stamp_start != nullptr, used = g_launch.stamp_used;
        g_launch.stamp_start = g_launch.stamp_end = nullptr; g_launch.stamp_used = false;
        if (step_rc) return step_rc;
        // WT_PLAN_FLAG_RANGE_REPORT: behind step i, the largest magnitude in every S32 buffer the step touches
        for (; next_range < p->range_entries.size() && p->range_entries[next_range].step == (int)i; ++next_range) {
            const BufSpec& b = p->bufs[p->range_entries[next_range].buf];
            if (int rc = launch_s32_amax(c.ws + b.off, (long)b.numel, p->range_dev + next_range, c.stream)) return rc;
        }
        if (timed && stamp) {
            if (armed && !used) {
                set_error("wt_plan_set_timing(\"@...\"): step '" + p->step_names[i] + "' does not launch a gemm16s kernel");
                return WT_ERR_INVALID;
            }
            if (armed) ++p->stamp_next;
            return 0;
        }
        if (dbg_status) {        // debugging aid: which step left a non-zero status word (synchronises after every step)
            unsigned st = 0;
            WT_HIP_CHECK(hipStreamSynchronize(c.stream));
            WT_HIP_CHECK(hipMemcpy(&st, c.ws + p->bufs[p->ctl].off, sizeof(st), hipMemcpyDeviceToHost));
            if (st) fprintf(stderr, "[wt status] plan kind %d B %d len %ld: step %zu (%s) -> status 0x%08x\n", p->kind, p->B, (long)p->len, i, p->step_names[i].c_str(), st);
        }
        if (timed) {
            WT_HIP_CHECK(hipEventRecord(ev.second, c.stream));
            p->ev_pending.push_back(ev);
        }
        return 0;
    }
};

// The one walk over a plan's steps, on the caller's stream or on the capture stream.  The step's kernels report into their
// site's word of the control block (model.h Site)
static int issue_steps(const wt_plan* p, const RunCtx& c, StepObserver* obs = nullptr) {
    unsigned* const site0 = reinterpret_cast<unsigned*>(c.ws + p->bufs[p->ctl].off) + CTL_SITE0;
    for (size_t i = 0; i < p->steps.size(); ++i) {
        g_launch.status = site0 + p->step_sites[i];
        if (obs) if (int rc = obs->before(i)) return rc;
        int rc = p->steps[i](c);
        if (obs) rc = obs->after(i, rc);
        if (rc) return rc;
    }
    return WT_OK;
}

// WT_PLAN_FLAG_GRAPH: the first call with a set of buffers runs eagerly (every one-time kernel attribute gets set), the second
// in a row with the same set records the launches on a capture stream, and that call and the later ones replay the recording on
// the caller's stream.  Returns an error, or WT_OK with *eager saying whether the steps are still to be issued (no graph for
// this plan or call, the key only remembered, or a capture that failed: the plan then stays on direct launches for good)
static int run_graph(const wt_plan* p, const RunCtx& c, bool* eager) {
    *eager = true;
    if (!(p->flags & WT_PLAN_FLAG_GRAPH) || !p->timing_filter.empty() || p->graph_failed || p->range_dev) return WT_OK;
    const wt_plan::GraphKey key{c.ws, c.in_codes ? static_cast<const void*>(c.in_codes) : c.in_f, c.out_f, c.codes, c.aux, c.lengths, c.bw_id, c.n_q};
    if (!(p->graph_exec && key == p->graph_key)) {
        if (!(key == p->last_key)) { p->last_key = key; return WT_OK; }
        if (p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; }
        if (!p->cap_stream) WT_HIP_CHECK(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
        RunCtx cc = c;
        cc.stream = p->cap_stream;
        WT_HIP_CHECK(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed));
        const int rc = issue_steps(p, cc);
        hipGraph_t g = nullptr;
        const hipError_t ce = hipStreamEndCapture(p->cap_stream, &g);
        hipError_t ie = hipErrorUnknown;
        if (!rc && ce == hipSuccess && g) ie = hipGraphInstantiate(&p->graph_exec, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (ie != hipSuccess) {
            (void)hipGetLastError();
            p->graph_exec = nullptr; p->graph_failed = true;
            return rc;
        }
        p->graph_key = key;
        // the recording holds a persistent launch only if the model still allowed one when it was made: after a
        // lost-co-residency fallback the steps record the launch-per-step kernel, and such a graph must survive
        // consume_status (it used to be destroyed and re-captured on every other call for the rest of the model's life)
        p->graph_persist = p->uses_persist && p->model->persist_ok.load();
    }
    WT_HIP_CHECK(hipGraphLaunch(p->graph_exec, c.stream));
    ++p->graph_replays;
    *eager = false;
    return WT_OK;
}

// The workspace is the caller's: the library assumes nothing about its contents (every word that can reach a result has been
// written by a step of the same call) and one thing about its address.  Buffers sit at multiples of 256 bytes from its start (wt_plan::buf),
// and what the kernels need of a buffer's address is the largest of: the 16-byte stores of the fills and the 16-byte vector and
// buffer loads of every kernel, the 128-byte S32 groups, and the 256-byte pitch itself, which the GEMMs' LDS-DMA rows and the
// persistent LSTM's 2 KB state rows take for granted.  So the start must be a multiple of 256.
constexpr uintptr_t WS_ALIGN = 256;

static int run_plan(const wt_plan* p, const RunCtx& c) {
    if (reinterpret_cast<uintptr_t>(c.ws) % WS_ALIGN) {      // before any launch, and before an earlier call's status is consumed
        set_error("the workspace must be 256-byte aligned");
        return WT_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard dg(p->model->device);
    if (!dg.ok) { set_error("hipSetDevice failed"); return WT_ERR_HIP; }
    if (const unsigned bits = consume_status(p)) {
        if (bits & WT_STATUS_LSTM) {
            set_error("an earlier persistent LSTM launch of this model lost co-residency (a step barrier timed out); that call's "
                      "outputs were overwritten (codes = -1, NaN); the model's plans now run the LSTM one launch per step: repeat the call");
            return WT_ERR_LSTM_SYNC;
        }
        if (bits & WT_STATUS_LENGTH) {
            set_error("an earlier mixed-length decode call on this model was given a clip length outside [1, padded length]; "
                      "that call's outputs were overwritten (NaN); repeat the call");
            return WT_ERR_INVALID;
        }
        set_error("an earlier call on this model met a value outside the f16 range of the split-f16 (S32) form (|v| >= 65504); "
                  "that call's outputs were overwritten (codes = -1, NaN); re-plan with WT_PLAN_FLAG_FP32_GEMM and repeat the call");
        return WT_ERR_RANGE;
    }
    struct CtxScope {        // the launch functions take the status word from this thread's context while the steps run
        explicit CtxScope(unsigned* s) { g_launch.status = s; }
        ~CtxScope() { g_launch.status = nullptr; }
    } scope(reinterpret_cast<unsigned*>(c.ws + p->bufs[p->ctl].off));
    LstmChainScope chain(p, c.stream);
    if (chain.rc) return chain.rc;
    bool eager;
    if (int rc = run_graph(p, c, &eager)) return rc;
    if (!eager) return WT_OK;
    if (p->range_dev) {
        if (int rc = launch_fill_u32(p->range_dev, 0u, (p->range_entries.size() * sizeof(unsigned) + 15) / 16 * 16, c.stream)) return rc;
        p->range_fresh = false;
    }
    if (!StepObserver::wanted(p)) return issue_steps(p, c);
    StepObserver obs(p, c);
    return issue_steps(p, c, &obs);
}

// device stamps: entry clocks start as all-ones (atomic min), exit clocks as zero (atomic max); one slot per timed launch
static int reset_stamps(const wt_plan* p) {
    const size_t half = (size_t)wt_plan::STAMP_SLOTS * sizeof(unsigned long long);
    WT_HIP_CHECK(hipMemset(p->stamps, 0xFF, half));
    WT_HIP_CHECK(hipMemset(p->stamps + wt_plan::STAMP_SLOTS, 0, half));
    WT_HIP_CHECK(hipDeviceSynchronize());
    p->stamp_next = 0;
    return WT_OK;
}

// a run entry point's first check: the plan is of the kind (and, for encode plans, the length form) the entry point runs
static int check_kind(const wt_plan* p, int kind, int mixed, const char* msg) {
    if (p && p->kind == kind && (mixed < 0 || !(p->flags & WT_PLAN_FLAG_MIXED_LENGTH) == !mixed)) return WT_OK;
    set_error(msg);
    return WT_ERR_INVALID;
}

extern "C" {

int wt_plan_status(const wt_plan* p, int32_t* bits, int32_t clear) {
    if (!p) return WT_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    unsigned b;
    if (clear) {
        DeviceGuard dg(p->model->device);
        unsigned own = 0;
        b = consume_status(p, &own) | own;      // this plan's failures and whatever the model's word still held
    } else {
        b = p->status_host ? __atomic_load_n(p->status_host, __ATOMIC_ACQUIRE) : 0u;
    }
    if (bits) *bits = (int32_t)b;
    return WT_OK;
}

int wt_plan_range_sites(const wt_plan* p, uint64_t* sites, int32_t clear) {
    if (!p || !sites) return WT_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    unsigned lo = 0, hi = 0;
    if (p->status_host) {
        lo = clear ? __atomic_exchange_n(p->status_host + 2, 0u, __ATOMIC_ACQUIRE) : __atomic_load_n(p->status_host + 2, __ATOMIC_ACQUIRE);
        hi = clear ? __atomic_exchange_n(p->status_host + 3, 0u, __ATOMIC_ACQUIRE) : __atomic_load_n(p->status_host + 3, __ATOMIC_ACQUIRE);
    }
    *sites = ((uint64_t)hi << 32) | lo;
    return WT_OK;
}

int wt_plan_range_report(const wt_plan* p, int32_t index, const char** step, const char** buffer, float* amax) {
    if (!p) return WT_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    if (!p->range_dev) { set_error("wt_plan_range_report: the plan was not created with WT_PLAN_FLAG_RANGE_REPORT"); return WT_ERR_INVALID; }
    if (index < 0 || index >= (int)p->range_entries.size()) return WT_ERR_INVALID;       // past the end (no message: callers iterate)
    if (!p->range_fresh) {
        DeviceGuard dg(p->model->device);
        WT_HIP_CHECK(hipDeviceSynchronize());
        static_assert(sizeof(float) == sizeof(unsigned), "bit patterns");
        WT_HIP_CHECK(hipMemcpy(p->range_host.data(), p->range_dev, p->range_entries.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        p->range_fresh = true;
    }
    const wt_plan::RangeEntry& e = p->range_entries[index];
    if (step) *step = p->step_names[e.step].c_str();
    if (buffer) *buffer = p->bufs[e.buf].name.c_str();
    if (amax) *amax = p->range_host[index];
    return WT_OK;
}

int64_t wt_plan_graph_replays(const wt_plan* p) { return p ? p->graph_replays : 0; }

int wt_plan_set_timing(const wt_plan* p, const char* name_substr) {
    if (!p) return WT_ERR_INVALID;
    p->timing_filter = name_substr ? name_substr : "";
    if (!p->timing_filter.empty() && p->timing_filter[0] == '@') {
        DeviceGuard dg(p->model->device);
        if (!p->stamps) WT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p->stamps), 2 * wt_plan::STAMP_SLOTS * sizeof(unsigned long long)));
        WT_HIP_CHECK(hipDeviceSynchronize());
        return reset_stamps(p);
    }
    return WT_OK;
}
int wt_plan_read_timing(const wt_plan* p, double* total_ms, int64_t* launches, int32_t reset) {
    if (!p) return WT_ERR_INVALID;
    for (auto& ev : p->ev_pending) {
        WT_HIP_CHECK(hipEventSynchronize(ev.second));
        float ms = 0.f;
        WT_HIP_CHECK(hipEventElapsedTime(&ms, ev.first, ev.second));
        p->timing_ms += ms;
        p->timing_n += 1;
        p->ev_free.push_back(ev);
    }
    p->ev_pending.clear();
    if (p->stamps && p->stamp_next > 0) {
        DeviceGuard dg(p->model->device);
        WT_HIP_CHECK(hipDeviceSynchronize());
        const int n = p->stamp_next;
        std::vector<unsigned long long> t0(n), t1(n);
        WT_HIP_CHECK(hipMemcpy(t0.data(), p->stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        WT_HIP_CHECK(hipMemcpy(t1.data(), p->stamps + wt_plan::STAMP_SLOTS, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            if (t1[i] > t0[i]) { p->timing_ms += (double)(t1[i] - t0[i]) * 1e-5; p->timing_n += 1; }      // 100 MHz ticks -> ms
        if (int rc = reset_stamps(p)) return rc;
    }
    if (total_ms) *total_ms = p->timing_ms;
    if (launches) *launches = p->timing_n;
    if (reset) { p->timing_ms = 0.0; p->timing_n = 0; }
    return WT_OK;
}

int wt_encode(const wt_plan* p, const float* wav, float* features, int64_t* codes, float* emb_out, void* workspace,
              void* stream) {
    if (int rc = check_kind(p, WT_PLAN_ENCODE, -1, "wt_encode: not an encode plan")) return rc;
    if (int rc = check_kind(p, WT_PLAN_ENCODE, 0, "wt_encode: a mixed-length plan runs through wt_encode_mixed")) return rc;
    if (p->flags & WT_PLAN_FLAG_RVQ) { set_error("wt_encode: a WT_PLAN_FLAG_RVQ plan runs through wt_encode_rvq"); return WT_ERR_INVALID; }
    if (!wav || !codes || !workspace) { set_error("wt_encode: null buffer"); return WT_ERR_INVALID; }
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), wav, features, codes, emb_out, 0};
    return run_plan(p, c);
}

int wt_encode_mixed(const wt_plan* p, const float* wav, const int32_t* lengths, float* features, int64_t* codes, float* emb_out,
                    void* workspace, void* stream) {
    if (int rc = check_kind(p, WT_PLAN_ENCODE, 1, "wt_encode_mixed: not a mixed-length encode plan (WT_PLAN_FLAG_MIXED_LENGTH)")) return rc;
    if (p->flags & WT_PLAN_FLAG_RVQ) { set_error("wt_encode_mixed: a WT_PLAN_FLAG_RVQ plan runs through wt_encode_rvq_mixed"); return WT_ERR_INVALID; }
    if (!wav || !lengths || !codes || !workspace) { set_error("wt_encode_mixed: null buffer"); return WT_ERR_INVALID; }
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), wav, features, codes, emb_out, 0, lengths};
    return run_plan(p, c);
}

int wt_decode(const wt_plan* p, const float* features, int32_t bandwidth_id, float* wav_out, float* backbone_out,
              void* workspace, void* stream) {
    if (p && p->kind == WT_PLAN_DECODE_MIXED) { set_error("wt_decode: a mixed-length plan runs through wt_decode_mixed"); return WT_ERR_INVALID; }
    if (int rc = check_kind(p, WT_PLAN_DECODE, -1, "wt_decode: not a decode plan")) return rc;
    if (!features || !wav_out || !workspace) { set_error("wt_decode: null buffer"); return WT_ERR_INVALID; }
    if (bandwidth_id < 0 || bandwidth_id >= p->model->arch.adanorm_num_embeddings) {
        set_error("wt_decode: bandwidth_id out of range"); return WT_ERR_INVALID;
    }
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), features, wav_out, nullptr, backbone_out, bandwidth_id};
    return run_plan(p, c);
}

int wt_decode_mixed(const wt_plan* p, const float* features, const int32_t* lengths, int32_t bandwidth_id, float* wav_out,
                    void* workspace, void* stream) {
    if (int rc = check_kind(p, WT_PLAN_DECODE_MIXED, -1, "wt_decode_mixed: not a mixed-length decode plan (WT_PLAN_DECODE_MIXED)")) return rc;
    if (!features || !lengths || !wav_out || !workspace) { set_error("wt_decode_mixed: null buffer"); return WT_ERR_INVALID; }
    if (bandwidth_id < 0 || bandwidth_id >= p->model->arch.adanorm_num_embeddings) {
        set_error("wt_decode_mixed: bandwidth_id out of range"); return WT_ERR_INVALID;
    }
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), features, wav_out, nullptr, nullptr, bandwidth_id, lengths};
    return run_plan(p, c);
}

// residual VQ encode: the call's number of rounds, checked before any launch
static int check_n_q(const wt_plan* p, int32_t n_q, const char* who) {
    if (n_q >= 1 && n_q <= p->model->arch.num_quantizers) return WT_OK;
    set_error(std::string(who) + ": n_q must be between 1 and the number of codebooks");
    return WT_ERR_INVALID;
}

int wt_encode_rvq(const wt_plan* p, const float* wav, int32_t n_q, int64_t* codes, void* workspace, void* stream) {
    if (int rc = check_kind(p, WT_PLAN_ENCODE, 0, "wt_encode_rvq: not a plain encode plan with WT_PLAN_FLAG_RVQ")) return rc;
    if (!(p->flags & WT_PLAN_FLAG_RVQ)) { set_error("wt_encode_rvq: not a WT_PLAN_FLAG_RVQ plan (wt_encode runs the others)"); return WT_ERR_INVALID; }
    if (!wav || !codes || !workspace) { set_error("wt_encode_rvq: null buffer"); return WT_ERR_INVALID; }
    if (int rc = check_n_q(p, n_q, "wt_encode_rvq")) return rc;
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), wav, nullptr, codes, nullptr, 0};
    c.n_q = n_q;
    return run_plan(p, c);
}

int wt_encode_rvq_mixed(const wt_plan* p, const float* wav, const int32_t* lengths, int32_t n_q, int64_t* codes, void* workspace,
                        void* stream) {
    if (int rc = check_kind(p, WT_PLAN_ENCODE, 1, "wt_encode_rvq_mixed: not a mixed-length encode plan with WT_PLAN_FLAG_RVQ")) return rc;
    if (!(p->flags & WT_PLAN_FLAG_RVQ)) { set_error("wt_encode_rvq_mixed: not a WT_PLAN_FLAG_RVQ plan (wt_encode_mixed runs the others)"); return WT_ERR_INVALID; }
    if (!wav || !lengths || !codes || !workspace) { set_error("wt_encode_rvq_mixed: null buffer"); return WT_ERR_INVALID; }
    if (int rc = check_n_q(p, n_q, "wt_encode_rvq_mixed")) return rc;
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), wav, nullptr, codes, nullptr, 0, lengths};
    c.n_q = n_q;
    return run_plan(p, c);
}

int wt_quantize(const wt_plan* p, const float* features, int32_t n_q, int64_t* codes, void* workspace, void* stream) {
    if (int rc = check_kind(p, WT_PLAN_QUANTIZE, -1, "wt_quantize: not a WT_PLAN_QUANTIZE plan")) return rc;
    if (!features || !codes || !workspace) { set_error("wt_quantize: null buffer"); return WT_ERR_INVALID; }
    if (int rc = check_n_q(p, n_q, "wt_quantize")) return rc;
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), features, nullptr, codes, nullptr, 0};
    c.n_q = n_q;
    return run_plan(p, c);
}

// decode from codes: the checks the two entry points share
static int check_decode_codes(const wt_plan* p, int32_t K, int32_t bandwidth_id, const std::string& who) {
    if (K < 1 || K > p->model->arch.num_quantizers) {
        set_error(who + ": K must be between 1 and the number of codebooks"); return WT_ERR_INVALID;
    }
    if (bandwidth_id < 0 || bandwidth_id >= p->model->arch.adanorm_num_embeddings) {
        set_error(who + ": bandwidth_id out of range"); return WT_ERR_INVALID;
    }
    return WT_OK;
}

int wt_decode_codes(const wt_plan* p, const int64_t* codes, int32_t K, int32_t bandwidth_id, float* wav_out, float* backbone_out,
                    void* workspace, void* stream) {
    if (p && p->kind == WT_PLAN_DECODE_CODES_MIXED) { set_error("wt_decode_codes: a mixed-length plan runs through wt_decode_codes_mixed"); return WT_ERR_INVALID; }
    if (int rc = check_kind(p, WT_PLAN_DECODE_CODES, -1, "wt_decode_codes: not a decode-from-codes plan (WT_PLAN_DECODE_CODES)")) return rc;
    if (!codes || !wav_out || !workspace) { set_error("wt_decode_codes: null buffer"); return WT_ERR_INVALID; }
    if (int rc = check_decode_codes(p, K, bandwidth_id, "wt_decode_codes")) return rc;
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), nullptr, wav_out, nullptr, backbone_out, bandwidth_id};
    c.in_codes = codes; c.n_q = K;
    return run_plan(p, c);
}

int wt_decode_codes_mixed(const wt_plan* p, const int64_t* codes, int32_t K, const int32_t* lengths, int32_t bandwidth_id,
                          float* wav_out, void* workspace, void* stream) {
    if (int rc = check_kind(p, WT_PLAN_DECODE_CODES_MIXED, -1, "wt_decode_codes_mixed: not a mixed-length decode-from-codes plan (WT_PLAN_DECODE_CODES_MIXED)")) return rc;
    if (!codes || !lengths || !wav_out || !workspace) { set_error("wt_decode_codes_mixed: null buffer"); return WT_ERR_INVALID; }
    if (int rc = check_decode_codes(p, K, bandwidth_id, "wt_decode_codes_mixed")) return rc;
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), nullptr, wav_out, nullptr, nullptr, bandwidth_id, lengths};
    c.in_codes = codes; c.n_q = K;
    return run_plan(p, c);
}

// head, SEANetDecoder and the LSTM unit: one fp32 array in, one out
static int run_in_out(const wt_plan* p, int kind, const float* in, float* out, void* workspace, void* stream, const char* who) {
    if (int rc = check_kind(p, kind, -1, (std::string(who) + ": wrong plan kind").c_str())) return rc;
    if (!in || !out || !workspace) { set_error(std::string(who) + ": null buffer"); return WT_ERR_INVALID; }
    RunCtx c{static_cast<char*>(workspace), static_cast<hipStream_t>(stream), in, out, nullptr, nullptr, 0};
    return run_plan(p, c);
}
int wt_head(const wt_plan* p, const float* x, float* wav_out, void* workspace, void* stream) {
    return run_in_out(p, WT_PLAN_HEAD, x, wav_out, workspace, stream, "wt_head");
}
int wt_seanet_decode(const wt_plan* p, const float* features, float* wav_out, void* workspace, void* stream) {
    return run_in_out(p, WT_PLAN_SEANET_DECODER, features, wav_out, workspace, stream, "wt_seanet_decode");
}
int wt_unit_run(const wt_plan* p, const float* x, float* y, void* workspace, void* stream) {
    return run_in_out(p, WT_PLAN_UNIT_LSTM, x, y, workspace, stream, "wt_unit_run");
}

}  // extern "C"
