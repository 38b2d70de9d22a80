// sng_policy.cpp -- the MLP actor's handle (sng_policy_create / sng_policy_create_net / set_weights / actions /
// destroy) and the host-only sng_policy_host_actions and sng_policy_net_host_actions.  The 64-64 actor's arithmetic
// is sng_policy_host.h's on the host and sng_policy.h's on the device, the any-width actor's sng_policy_net_host.h's
// and sng_policy_net.h's; one handle type serves both (SngPolicy::net says which).  The graphs with the actor in the
// loop are captured in sng_graph.cpp.
#include <algorithm>
#include <cstring>

#include "sng_env.h"

using namespace sng;

// The device image, its pinned mirror, the clipped-actions block and the upload event of a new policy, with zero
// weights (and the spec's bounds) in the image until the first upload.  Destroys `pol` where it fails.
static int policy_buffers(SngEnv *env, SngPolicy *pol) {
    const int O = pol->net ? pol->net_spec.obs_dim : pol->spec.obs_dim, A = pol->net ? pol->net_spec.act_dim : pol->spec.act_dim;
    const int H1 = pol->net ? pol->net_spec.hidden1 : kPolicyHidden, H2 = pol->net ? pol->net_spec.hidden2 : kPolicyHidden;
    const size_t bytes = (pol->net ? pol->net_image.floats : pol->image.floats) * sizeof(float);
    (void)policy_kernels_init();   // a refusal surfaces at the launch that needs the room
    hipError_t e = hipMalloc((void **)&pol->d_img, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&pol->h_img, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&pol->d_env_actions, (size_t)env->E * (size_t)A * sizeof(float));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pol->uploaded, hipEventDisableTiming);
    if (e == hipSuccess) {
        const std::vector<float> zero(std::max({(size_t)H1 * (size_t)O, (size_t)H2 * (size_t)H1, (size_t)A * (size_t)H2}));
        const SngMlpWeights w{zero.data(), zero.data(), zero.data(), zero.data(), zero.data(), zero.data()};
        if (pol->net) net_pack(pol->net_image, pol->net_spec, w, pol->h_img);
        else policy_pack(pol->image, pol->spec, w, pol->h_img);
        e = hipMemcpy(pol->d_img, pol->h_img, bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        sng_policy_destroy(pol);
        return e == hipErrorOutOfMemory ? fail(env, SNG_ERR_OUT_OF_MEMORY, "policy buffers") : hip_fail(env, e, "policy create");
    }
    return SNG_OK;
}

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
    if (int rc = policy_buffers(env, pol)) return rc;
    *out = pol;
    return SNG_OK;
}

int sng_policy_create_net(SngEnv *env, const SngMlpNetSpec *spec, SngPolicy **out) {
    if (!env || !spec || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = net_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPolicy *pol = new SngPolicy();
    pol->env = env;
    pol->net = true;
    pol->net_spec = *spec;
    if (spec->low) {
        pol->clip_low.assign(spec->low, spec->low + spec->act_dim);
        pol->clip_high.assign(spec->high, spec->high + spec->act_dim);
        pol->net_spec.low = pol->clip_low.data();
        pol->net_spec.high = pol->clip_high.data();
    }
    pol->net_image = net_image(spec->obs_dim, spec->act_dim, spec->hidden1, spec->hidden2, spec->activation, spec->output,
                               spec->low != nullptr);
    if (int rc = policy_buffers(env, pol)) return rc;
    *out = pol;
    return SNG_OK;
}

int sng_policy_set_weights(SngPolicy *pol, const SngMlpWeights *w, void *stream) {
    if (!pol) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = pol->env;
    std::string why;
    if (int rc = pol->net ? net_weights_check(pol->net_spec, w, &why) : policy_weights_check(pol->spec, w, &why))
        return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipEventSynchronize(pol->uploaded));   // the upload before this one has read the mirror
    if (pol->net) net_pack(pol->net_image, pol->net_spec, *w, pol->h_img);
    else policy_pack(pol->image, pol->spec, *w, pol->h_img);
    const size_t floats = pol->net ? pol->net_image.floats : pol->image.floats;
    HIP_TRY(env, hipMemcpyAsync(pol->d_img, pol->h_img, floats * sizeof(float), hipMemcpyHostToDevice,
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
    if (pol->net)
        HIP_TRY(env, launch_policy_net(pol->d_img, pol->net_image, obs, noise, actions, env_actions, env->E, as_stream(stream)));
    else
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

int sng_policy_net_host_actions(const SngMlpNetSpec *spec, const SngMlpWeights *w, int64_t rows, const float *obs,
                                const float *noise, float *actions, float *env_actions) {
    std::string why;
    if (int rc = net_spec_check(spec, 0, 0, &why)) return fail(nullptr, rc, why);
    if (int rc = net_weights_check(*spec, w, &why)) return fail(nullptr, rc, why);
    if (rows < 0 || (rows > 0 && (!obs || !actions))) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null argument");
    const NetImage m = net_image(spec->obs_dim, spec->act_dim, spec->hidden1, spec->hidden2, spec->activation, spec->output,
                                 spec->low != nullptr);
    std::vector<float> img(m.floats);
    net_pack(m, *spec, *w, img.data());
    mlp_net_host(m, img.data(), rows, obs, noise, actions, env_actions);
    return SNG_OK;
}

}  // extern "C"
