// sng_noise.cpp -- the action-noise source's handle (sng_noise_create / set_params / fill / get_counter / set_counter /
// destroy) and the host-only sng_noise_host_fill.  The arithmetic is sng_noise_host.h's on both sides; the kernel is
// sng_noise.h's.  The graphs that begin with a fill are captured in sng_graph.cpp.
#include <algorithm>
#include <vector>

#include "sng_env.h"

using namespace sng;

extern "C" {

int sng_noise_create(SngEnv *env, const SngNoiseSpec *spec, SngNoise **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = noise_spec_check(spec, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngNoise *nz = new SngNoise();
    nz->env = env;
    nz->spec = *spec;
    const size_t floats = 2 * (size_t)spec->act_dim;
    hipError_t e = nz->params.create(floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&nz->d_counter, sizeof(uint64_t));
    if (e == hipSuccess) e = nz->params.upload_now([&](float *h) { std::fill(h, h + floats, 0.f); });
    if (e == hipSuccess) e = hipMemset(nz->d_counter, 0, sizeof(uint64_t));
    if (e != hipSuccess) {
        sng_noise_destroy(nz);
        return create_fail(env, e, "noise");
    }
    *out = nz;
    return SNG_OK;
}

int sng_noise_set_params(SngNoise *nz, const float *mu, const float *scale, void *stream) {
    if (!nz) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null noise handle");
    SngEnv *env = nz->env;
    std::string why;
    if (int rc = noise_params_check(nz->spec.act_dim, mu, scale, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, nz->params.upload(as_stream(stream), [&](float *h) { noise_pack_params(nz->spec, mu, scale, h); }));
    return SNG_OK;
}

int sng_noise_fill(SngNoise *nz, float *out, int32_t days, void *stream) {
    if (!nz) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null noise handle");
    SngEnv *env = nz->env;
    if (days < 1) return fail(env, SNG_ERR_INVALID_ARGUMENT, "noise fill: days = " + std::to_string(days) + " must be >= 1");
    if (!out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null noise output");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_noise_fill(nz->spec, nz->params.d, nz->d_counter, env->p.env_offset, out, days, env->p.T, env->E,
                                   as_stream(stream)));
    return SNG_OK;
}

int sng_noise_get_counter(SngNoise *nz, uint64_t *out, void *stream) {
    if (!nz) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null noise handle");
    SngEnv *env = nz->env;
    if (!out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipMemcpyAsync(out, nz->d_counter, sizeof(uint64_t), hipMemcpyDeviceToHost, as_stream(stream)));
    HIP_TRY(env, hipStreamSynchronize(as_stream(stream)));
    return SNG_OK;
}

int sng_noise_set_counter(SngNoise *nz, uint64_t counter, void *stream) {
    if (!nz) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null noise handle");
    SngEnv *env = nz->env;
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipMemcpyAsync(nz->d_counter, &counter, sizeof(uint64_t), hipMemcpyHostToDevice, as_stream(stream)));
    HIP_TRY(env, hipStreamSynchronize(as_stream(stream)));
    return SNG_OK;
}

void sng_noise_destroy(SngNoise *nz) {
    if (!nz) return;
    DeviceScope scope(nz->env->device);
    nz->params.destroy();
    if (nz->d_counter) (void)hipFree(nz->d_counter);
    delete nz;
}

int sng_noise_host_fill(const SngNoiseSpec *spec, const float *mu, const float *scale, int32_t T, int64_t E,
                        int64_t env_offset, uint64_t counter, int32_t days, float *out) {
    std::string why;
    if (int rc = noise_spec_check(spec, 0, &why)) return fail(nullptr, rc, why);
    if (int rc = noise_params_check(spec->act_dim, mu, scale, &why)) return fail(nullptr, rc, why);
    if (days < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "noise fill: days = " + std::to_string(days) + " must be >= 1");
    if (T < 1 || E < 1)
        return fail(nullptr, SNG_ERR_INVALID_ARGUMENT,
                    "noise fill: T = " + std::to_string(T) + " and E = " + std::to_string(E) + " must be >= 1");
    if (!out) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null noise output");
    std::vector<float> params(2 * (size_t)spec->act_dim);
    noise_pack_params(*spec, mu, scale, params.data());
    noise_host_fill(*spec, params.data(), T, E, env_offset, counter, days, out);
    return SNG_OK;
}

}  // extern "C"
