// sng_policy.cpp -- the MLP actor's handle (sng_policy_create / set_weights / actions / destroy) and the host-only
// sng_policy_host_actions.  The arithmetic is sng_policy_host.h's on the host and sng_policy.h's on the device; the
// graphs with the actor in the loop are captured in sng_graph.cpp.
#include <cstring>

#include "sng_env.h"

using namespace sng;

extern "C" {

int sng_policy_create(SngEnv *env, const SngMlpSpec *spec, SngPolicy **out) {
    if (!env || !spec || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = policy_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPolicy *pol = new SngPolicy();
    pol->env = env;
    pol->spec = *spec;
    if (spec->clip_low) {
        pol->clip_low.assign(spec->clip_low, spec->clip_low + spec->act_dim);
        pol->clip_high.assign(spec->clip_high, spec->clip_high + spec->act_dim);
        pol->spec.clip_low = pol->clip_low.data();
        pol->spec.clip_high = pol->clip_high.data();
    }
    pol->image = policy_image(spec->obs_dim, spec->act_dim, spec->activation, spec->clip_low != nullptr);
    const size_t bytes = pol->image.floats * sizeof(float);
    (void)policy_kernels_init();   // a refusal surfaces at the launch that needs the room
    hipError_t e = hipMalloc((void **)&pol->d_img, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&pol->h_img, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&pol->d_env_actions, (size_t)env->E * (size_t)spec->act_dim * sizeof(float));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pol->uploaded, hipEventDisableTiming);
    // zero weights (and the spec's bounds) until the first upload
    if (e == hipSuccess) {
        const std::vector<float> zero((size_t)kPolicyHidden * (size_t)(spec->obs_dim + kPolicyHidden + spec->act_dim + 2) +
                                      (size_t)spec->act_dim);
        const SngMlpWeights w{zero.data(), zero.data(), zero.data(), zero.data(), zero.data(), zero.data()};
        policy_pack(pol->image, pol->spec, w, pol->h_img);
        e = hipMemcpy(pol->d_img, pol->h_img, bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        sng_policy_destroy(pol);
        return e == hipErrorOutOfMemory ? fail(env, SNG_ERR_OUT_OF_MEMORY, "policy buffers") : hip_fail(env, e, "policy create");
    }
    *out = pol;
    return SNG_OK;
}

int sng_policy_set_weights(SngPolicy *pol, const SngMlpWeights *w, void *stream) {
    if (!pol) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = pol->env;
    std::string why;
    if (int rc = policy_weights_check(pol->spec, w, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipEventSynchronize(pol->uploaded));   // the upload before this one has read the mirror
    policy_pack(pol->image, pol->spec, *w, pol->h_img);
    HIP_TRY(env, hipMemcpyAsync(pol->d_img, pol->h_img, pol->image.floats * sizeof(float), hipMemcpyHostToDevice,
                                as_stream(stream)));
    HIP_TRY(env, hipEventRecord(pol->uploaded, as_stream(stream)));
    return SNG_OK;
}

int sng_policy_actions(SngPolicy *pol, const float *obs, const float *noise, float *actions, float *env_actions,
                       void *stream) {
    if (!pol) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = pol->env;
    if (!obs || !actions) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_policy(pol->d_img, pol->image, obs, noise, actions, env_actions, env->E, as_stream(stream)));
    return SNG_OK;
}

void sng_policy_destroy(SngPolicy *pol) {
    if (!pol) return;
    DeviceScope scope(pol->env->device);
    if (pol->uploaded) {
        (void)hipEventSynchronize(pol->uploaded);
        (void)hipEventDestroy(pol->uploaded);
    }
    if (pol->d_img) (void)hipFree(pol->d_img);
    if (pol->d_env_actions) (void)hipFree(pol->d_env_actions);
    if (pol->h_img) (void)hipHostFree(pol->h_img);
    delete pol;
}

int sng_policy_host_actions(const SngMlpSpec *spec, const SngMlpWeights *w, int64_t rows, const float *obs,
                            const float *noise, float *actions, float *env_actions) {
    std::string why;
    if (int rc = policy_spec_check(spec, 0, 0, &why)) return fail(nullptr, rc, why);
    if (int rc = policy_weights_check(*spec, w, &why)) return fail(nullptr, rc, why);
    if (rows < 0 || (rows > 0 && (!obs || !actions))) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null argument");
    const PolicyImage m = policy_image(spec->obs_dim, spec->act_dim, spec->activation, spec->clip_low != nullptr);
    std::vector<float> img(m.floats);
    policy_pack(m, *spec, *w, img.data());
    mlp_actor_host(m, img.data(), rows, obs, noise, actions, env_actions);
    return SNG_OK;
}

}  // extern "C"
