// C-ABI entry points of the denoiser, which take a context and no scene: lj_denoise / _device (denoise) and lj_get_denoise_stats.
#include "api_calls.h"

// lj_denoise / _device: every check first, then pack, one k_atrous launch per iteration, unpack — on the context's stream, ordered against
// the caller's as render_frames orders a render.  The host variant stages its buffers in the context's workspace.
static void denoise(lj_context *ctx, int32_t n, int32_t w, int32_t h, const LjFeatureBuffers *in, const LjDenoiseArgs *args, float *rgb_out, float *variance_out,
                    bool on_device, hipStream_t caller, const std::string &me) {
    if (!ctx || !in || !in->rgb || !rgb_out) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    if (n <= 0 || w <= 0 || h <= 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": n, width and height must be positive");
    const uint64_t limit = 1ull << 31, image = (uint64_t)w * (uint64_t)h;
    if (image > limit || image * (uint64_t)n > limit) throw LjError(LJ_ERR_INVALID_ARG, me + ": more than 2^31 pixels");
    const LjDenoiseArgs a = args ? *args : LjDenoiseArgs{};
    if (a.iterations > ljd::denoise_max_iterations()) throw LjError(LJ_ERR_INVALID_ARG, me + ": at most 8 iterations");
    for (float sg : {a.sigma_color, a.sigma_normal, a.sigma_depth, a.sigma_albedo})
        if (!(sg >= 0.0f) || !(sg <= 3.402823466e38f)) throw LjError(LJ_ERR_INVALID_ARG, me + ": a sigma is negative or not finite");
    if (a.flags & ~(uint32_t)LJ_DENOISE_DEMODULATE) throw LjError(LJ_ERR_INVALID_ARG, me + ": unknown flag");
    if ((a.flags & LJ_DENOISE_DEMODULATE) && !in->albedo) throw LjError(LJ_ERR_INVALID_ARG, me + ": LJ_DENOISE_DEMODULATE needs the albedo buffer");
    if (variance_out && !in->variance) throw LjError(LJ_ERR_INVALID_ARG, me + ": variance_out needs the variance buffer");
    const uint32_t has = ljd::denoise_has(in->variance, in->albedo, in->normal, in->depth, (a.flags & LJ_DENOISE_DEMODULATE) != 0);
    const ljd::DenoiseCall call{has, a.iterations, {a.sigma_color, a.sigma_normal, a.sigma_depth, a.sigma_albedo}};
    const int iterations = ljd::denoise_iterations(call);
    // ---- nothing was written up to here
    // the device variant returns without waiting, so it is ordered against the caller's stream on both sides even when that is the null
    // stream (the context's stream does not synchronise with it by itself)
    hipStream_t s = enter_from_caller(ctx, caller, on_device);
    const uint64_t total = image * (uint64_t)n;
    const float *src[5] = {in->rgb, in->variance, in->albedo, in->normal, in->depth};
    const size_t chan[5] = {3, 3, 3, 3, 1};
    float *out_rgb = rgb_out, *out_var = variance_out;
    if (!on_device) {
        float *staged[5] = {};
        stage_frames(src, chan, 0, 5, total, ctx->dn_in, staged);
        ensure(ctx->dn_out, total * 6 * sizeof(float));
        for (int k = 0; k < 5; k++) if (src[k]) {
            HIP_CHECK(hipMemcpyAsync(staged[k], src[k], total * chan[k] * sizeof(float), hipMemcpyHostToDevice, s));
            src[k] = staged[k];
        }
        out_rgb = (float *)ctx->dn_out.p; out_var = variance_out ? out_rgb + total * 3 : nullptr;
    }
    ensure(ctx->dn_guide, total * ljd::denoise_record_bytes());
    for (DevBuf &b : ctx->dn_dyn) ensure(b, total * ljd::denoise_record_bytes());
    const int lds_iterations = denoise_lds_iterations();
    HIP_CHECK(hipEventRecord(ctx->ev_d0, s));
    ljd::launch_denoise_pack(has, total, src[0], src[1], src[2], src[3], src[4], ctx->dn_guide.p, ctx->dn_dyn[0].p, s);
    for (int i = 0; i < iterations; i++)
        ljd::launch_atrous(call, n, w, h, i, i < lds_iterations, ctx->dn_guide.p, ctx->dn_dyn[i & 1].p, ctx->dn_dyn[(i + 1) & 1].p, s);
    ljd::launch_denoise_unpack(has, total, ctx->dn_guide.p, ctx->dn_dyn[iterations & 1].p, out_rgb, out_var, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ctx->ev_d1, s));
    ctx->denoise_stats = LjDenoiseStats{}; ctx->denoise_stats.launches = (uint64_t)iterations + 2; ctx->denoise_stats.pixels = total;
    ctx->denoise_time_pending = true;
    if (!on_device) {
        HIP_CHECK(hipMemcpyAsync(rgb_out, out_rgb, total * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (variance_out) HIP_CHECK(hipMemcpyAsync(variance_out, out_var, total * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    leave_to_caller(ctx, caller, on_device);
}

extern "C" {

int lj_denoise(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_host, const LjDenoiseArgs *args, float *rgb_out_host, float *variance_out_host) {
    return lj::guard([&]() { denoise(ctx, n, width, height, in_host, args, rgb_out_host, variance_out_host, false, nullptr, "lj_denoise"); });
}

int lj_denoise_device(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_device, const LjDenoiseArgs *args, float *rgb_out_device, float *variance_out_device,
                      void *hip_stream) {
    return lj::guard([&]() { denoise(ctx, n, width, height, in_device, args, rgb_out_device, variance_out_device, true, (hipStream_t)hip_stream, "lj_denoise_device"); });
}

int lj_get_denoise_stats(const lj_context *ctx_in, LjDenoiseStats *out) {
    return lj::guard([&]() {
        if (!ctx_in || !out) throw LjError(LJ_ERR_INVALID_ARG, "lj_get_denoise_stats: null argument");
        lj_context *ctx = const_cast<lj_context *>(ctx_in);
        if (ctx->denoise_time_pending) {   // the last call's launches may still run (the device variant does not wait): their time is read here, once
            set_device(ctx);
            HIP_CHECK(hipEventSynchronize(ctx->ev_d1));
            ctx->denoise_stats.denoise_ms = elapsed_ms(ctx->ev_d0, ctx->ev_d1);
            ctx->denoise_time_pending = false;
        }
        *out = ctx->denoise_stats;
    });
}

} // extern "C"
