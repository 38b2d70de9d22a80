// sng_policy.cpp -- the MLP actor's handle (sng_policy_create / sng_policy_create_net / set_weights / actions /
// destroy) and the host-only sng_policy_host_actions and sng_policy_net_host_actions.  The 64-64 actor's arithmetic
// is sng_policy_host.h's on the host and sng_policy.h's on the device, the any-width actor's sng_policy_net_host.h's
// and sng_policy_net.h's; one handle type serves both (sng_env.h, SngPolicy, and what depends on its form).  The graphs with the actor in the
// loop are captured in sng_graph.cpp.
#include <algorithm>
#include <cstring>

#include "sng_env.h"

using namespace sng;

// What the two creates share, `pol` holding its form's spec and image: the dims and the owned copy of the bounds
// (*low_at / *high_at: the spec's pointers to them), the device image with zero weights (and the bounds) in it until the
// first upload, and the clipped-actions block.  Destroys `pol` where it fails.
static int policy_finish_create(SngEnv *env, SngPolicy *pol, int O, int A, int H1, int H2, size_t floats,
                                const float **low_at, const float **high_at, SngPolicy **out) {
    pol->env = env;
    pol->O = O, pol->A = A, pol->H1 = H1, pol->H2 = H2;
    pol->floats = floats;
    if (*low_at) {
        pol->clip_low.assign(*low_at, *low_at + A);
        pol->clip_high.assign(*high_at, *high_at + A);
        *low_at = pol->clip_low.data();
        *high_at = pol->clip_high.data();
    }
    (void)policy_kernels_init();   // a refusal surfaces at the launch that needs the room
    hipError_t e = pol->img.create(floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&pol->d_env_actions, (size_t)env->E * (size_t)A * sizeof(float));
    if (e == hipSuccess) {
        const std::vector<float> zero(std::max({(size_t)H1 * (size_t)O, (size_t)H2 * (size_t)H1, (size_t)A * (size_t)H2}));
        const SngMlpWeights w{zero.data(), zero.data(), zero.data(), zero.data(), zero.data(), zero.data()};
        e = pol->img.upload_now([&](float *img) { policy_pack_image(pol, w, img); });
    }
    if (e != hipSuccess) {
        sng_policy_destroy(pol);
        return create_fail(env, e, "policy");
    }
    *out = pol;
    return SNG_OK;
}

extern "C" {

int sng_policy_create(SngEnv *env, const SngMlpSpec *spec, SngPolicy **out) {
    if (!env || !spec || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = policy_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPolicy *pol = new SngPolicy();
    pol->spec = *spec;
    pol->image = policy_image(spec->obs_dim, spec->act_dim, spec->activation, spec->clip_low != nullptr);
    return policy_finish_create(env, pol, spec->obs_dim, spec->act_dim, kPolicyHidden, kPolicyHidden, pol->image.floats,
                                &pol->spec.clip_low, &pol->spec.clip_high, out);
}

int sng_policy_create_net(SngEnv *env, const SngMlpNetSpec *spec, SngPolicy **out) {
    if (!env || !spec || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = net_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPolicy *pol = new SngPolicy();
    pol->net = true;
    pol->net_spec = *spec;
    pol->net_image = net_image(spec->obs_dim, spec->act_dim, spec->hidden1, spec->hidden2, spec->activation, spec->output,
                               spec->low != nullptr);
    return policy_finish_create(env, pol, spec->obs_dim, spec->act_dim, spec->hidden1, spec->hidden2, pol->net_image.floats,
                                &pol->net_spec.low, &pol->net_spec.high, out);
}

int sng_policy_set_weights(SngPolicy *pol, const SngMlpWeights *w, void *stream) {
    if (!pol) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = pol->env;
    std::string why;
    if (int rc = policy_weights_ok(pol, w, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, pol->img.upload(as_stream(stream), [&](float *img) { policy_pack_image(pol, *w, img); }));
    return SNG_OK;
}

int sng_policy_actions(SngPolicy *pol, const float *obs, const float *noise, float *actions, float *env_actions,
                       void *stream) {
    if (!pol) return SNG_ERR_INVALID_ARGUMENT;
    SngEnv *env = pol->env;
    if (!obs || !actions) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_actor(pol, obs, noise, actions, env_actions, env->E, as_stream(stream)));
    return SNG_OK;
}

void sng_policy_destroy(SngPolicy *pol) {
    if (!pol) return;
    DeviceScope scope(pol->env->device);
    pol->img.destroy();
    if (pol->d_env_actions) (void)hipFree(pol->d_env_actions);
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
