// The scaffolding the ragged calls share (wt_ingest, wt_emit, wt_overlap_add_ragged, wt_mel_*, wt_stoi): a launch takes clips of
// different lengths, one device-form descriptor per clip.  Up to N descriptors travel in the kernel's argument block: nothing is
// copied on the stream (a copy and the wait behind it cost more than a short clip's whole work) and the call can be captured into
// a graph.  More are uploaded into the head of the call's workspace.  A kernel is a template over the descriptor source D and reads
// d.clip[i] either way.
#pragma once
#include "../../include/wavtokenizer_amd.h"
#include "common.h"

#include <cstring>
#include <vector>

namespace wt {

template <class C, int N> struct ArgClips { C clip[N]; };      // descriptors in the launch's own argument block
template <class C> struct PtrClips { const C* clip; };         // descriptors in the workspace

// Uploads a launch's device-form descriptors into its workspace on s through the current device's next pinned block (a block that
// has to grow is given at least min_bytes); `who` names the calling function in the error texts (audio.hip)
int stage_descriptors(const char* who, const void* descs, size_t bytes, size_t min_bytes, void* workspace, hipStream_t s);

// Picks the route of B descriptors and hands launch (a generic callable) the source: an ArgClips<C, N> for B <= N (zeros behind the
// B descriptors: blocks read clip[i < B] alone), else a PtrClips<C> over the uploaded copy; the pinned block holds at least
// min_descs descriptors, so that it seldom has to grow
template <int N, class C, class F>
int launch_ragged(const char* who, const C* descs, int B, int min_descs, void* workspace, hipStream_t s, F&& launch) {
    if (B <= N) {
        ArgClips<C, N> args{};
        memcpy(args.clip, descs, (size_t)B * sizeof(C));
        launch(args);
        return WT_OK;
    }
    if (int rc = stage_descriptors(who, descs, (size_t)B * sizeof(C), (size_t)min_descs * sizeof(C), workspace, s)) return rc;
    launch(PtrClips<C>{static_cast<const C*>(workspace)});
    return WT_OK;
}

// What a call on a table handle (wt_mel, wt_stoi_handle) checks first
inline bool ragged_call_ok(const std::string& fn, const void* handle, const void* clips, const void* workspace, int B, int max_B) {
    if (!handle) { set_error(fn + ": null handle"); return false; }
    if (!clips || !workspace) { set_error(fn + ": null clips or workspace"); return false; }
    if (B < 1 || B > max_B) { set_error(fn + ": B outside 1.." + std::to_string(max_B)); return false; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error(fn + ": workspace misaligned"); return false; }
    return true;
}
// and last, when its arguments have passed: the handle's tables lie on the device the launches will go to
inline bool on_current_device(const std::string& fn, int handle_device) {
    int device = -1;
    if (hipGetDevice(&device) == hipSuccess && device == handle_device) return true;
    set_error(fn + ": the handle belongs to another device than the calling thread's current one");
    return false;
}

// A handle's table as one block on `device`; the calling thread's current device is put back before the call returns
inline int upload_table(const std::string& fn, int device, const std::vector<float>& tab, float** out) {
    int prev = 0;
    WT_HIP_CHECK(hipGetDevice(&prev));
    WT_HIP_CHECK(hipSetDevice(device));
    float* d = nullptr;
    const bool ok = hipMalloc(reinterpret_cast<void**>(&d), tab.size() * sizeof(float)) == hipSuccess &&
                    hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        set_error(fn + ": device allocation failed");
        if (d) (void)hipFree(d);
    }
    const hipError_t back = hipSetDevice(prev);
    if (!ok) return WT_ERR_HIP;
    if (back != hipSuccess) {
        set_error(fn + ": could not restore the current device");
        (void)hipFree(d);
        return WT_ERR_HIP;
    }
    *out = d;
    return WT_OK;
}

}  // namespace wt
