// The call sequences that the C-ABI entry points (the api_*.hip files, and only they) share: ordering against the caller's stream, the camera
// table of a batch, frame staging for the host variants, error labels, and the stats getters.
#pragma once
#include "api_internal.h"

// A call's work runs on the context's own stream (render_frames in api_device.hip says why), ordered against the caller's by ev_caller:
// enter_from_caller makes the context's device current, orders its stream after the caller's and returns it; leave_to_caller orders the
// caller's after it.  Plain calls and no destructor: a call that fails on the way records nothing.  `order`: the call site's rule.
inline hipStream_t enter_from_caller(lj_context *ctx, hipStream_t caller, bool order) {
    set_device(ctx);
    if (order) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_caller, 0)); }
    return ctx->stream;
}
inline void leave_to_caller(lj_context *ctx, hipStream_t caller, bool order) {
    if (order) { HIP_CHECK(hipEventRecord(ctx->ev_caller, ctx->stream)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
}
// the camera table of a batch (view_table) onto the device and into the plan; an empty one leaves the plan the scene's own camera
inline void upload_view_table(lj_context *ctx, const std::vector<ljd::DCamera> &table, RenderPlan &plan, hipStream_t s) {
    if (table.empty()) return;
    const size_t table_bytes = table.size() * sizeof(ljd::DCamera);
    ensure(ctx->view_table, table_bytes);
    HIP_CHECK(hipMemcpyAsync(ctx->view_table.p, table.data(), table_bytes, hipMemcpyHostToDevice, s));
    plan.views_dev = (const ljd::DCamera *)ctx->view_table.p;
}
// The frames of a host variant: frame[k] = n_pix * chan[k] four-byte values on the device for every k in [k0, k1) whose host buffer dst[k]
// is given, one after the other in the grow-only workspace `ws`; fetch_frames copies results back into the host buffers and waits.
template <typename H, typename D> void stage_frames(H *const dst[], const size_t chan[], int k0, int k1, size_t n_pix, DevBuf &ws, D *frame[]) {
    size_t need = 0;
    for (int k = k0; k < k1; k++) if (dst[k]) need += n_pix * chan[k];
    ensure(ws, need * 4);
    uint32_t *at = (uint32_t *)ws.p;
    for (int k = k0; k < k1; k++) if (dst[k]) { frame[k] = (D *)at; at += n_pix * chan[k]; }
}
template <typename T> void fetch_frames(T *const dst[], T *const frame[], const size_t chan[], int k0, int k1, size_t n_pix, hipStream_t s) {
    for (int k = k0; k < k1; k++) if (dst[k]) HIP_CHECK(hipMemcpyAsync(dst[k], frame[k], n_pix * chan[k] * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}
// what f() returns; an LjError that leaves it carries the entry point's name in front of its message
template <typename F> auto relabelled(const std::string &me, F &&f) -> decltype(f()) {
    try { return f(); }
    catch (const LjError &e) { throw LjError(e.code, me + ": " + e.what()); }
}
// a lj_get_*_stats entry point: the member of the handle that the last call of its family left
template <typename H, typename S> int get_stats(const H *handle, S H::*member, S *out, const std::string &me) {
    if (!handle || !out) { lj::set_last_error(me + ": null argument"); return LJ_ERR_INVALID_ARG; }
    *out = handle->*member;
    return LJ_OK;
}
