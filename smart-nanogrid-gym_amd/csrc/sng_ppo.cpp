// sng_ppo.cpp -- the PPO head's handle (sng_ppo_create / create_net / set_weights / finish / destroy) and the host-only
// sng_ppo_host_finish and sng_ppo_net_host_finish.  The 64-64 head's arithmetic is sng_ppo_host.h's on the host and
// sng_ppo.h's on the device, the any-width head's sng_ppo_net_host.h's and sng_ppo_net.h's; one handle type serves
// both (SngPpo::net says which).
#include <vector>

#include "sng_env.h"

using namespace sng;

// A head of a handle's envs: the device image rollout_gae_kernel reads (sng_ppo_host.h, PpoImage), its pinned host
// mirror, which sng_ppo_set_weights packs and uploads from, and the upload event.
struct SngPpo {
    SngEnv *env = nullptr;
    PpoImage image{};
    float *d_img = nullptr, *h_img = nullptr;
    hipEvent_t uploaded = nullptr;   // the last upload has read h_img
    // sng_ppo_create_net: the value net's spec and the head's image (sng_ppo_net_host.h) in the place of `image`
    bool net = false;
    SngPpoNetSpec net_spec{};
    PpoNetImage net_image{};
};

// The buffers of a head whose image has `floats` floats, and its first upload from the mirror `pack` fills.
template <class Pack>
static int ppo_alloc(SngEnv *env, SngPpo *ppo, size_t floats, Pack pack, SngPpo **out) {
    const size_t bytes = floats * sizeof(float);
    hipError_t e = hipMalloc((void **)&ppo->d_img, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ppo->h_img, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ppo->uploaded, hipEventDisableTiming);
    if (e == hipSuccess) {
        pack(ppo->h_img);
        e = hipMemcpy(ppo->d_img, ppo->h_img, bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        sng_ppo_destroy(ppo);
        return e == hipErrorOutOfMemory ? fail(env, SNG_ERR_OUT_OF_MEMORY, "ppo buffers") : hip_fail(env, e, "ppo create");
    }
    *out = ppo;
    return SNG_OK;
}

extern "C" {

int sng_ppo_create(SngEnv *env, int32_t activation, SngPpo **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = ppo_dims_check(env->p.obs_dim, env->p.act_dim, activation, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPpo *ppo = new SngPpo();
    ppo->env = env;
    ppo->image = ppo_image(env->p.obs_dim, env->p.act_dim, activation);
    (void)ppo_kernels_init();   // a refusal surfaces at the launch that needs the room
    return ppo_alloc(env, ppo, ppo->image.floats, [&](float *img) { ppo_pack_log_std(ppo->image, nullptr, img); }, out);
}

int sng_ppo_create_net(SngEnv *env, const SngPpoNetSpec *spec, SngPpo **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = ppo_net_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    SngPpo *ppo = new SngPpo();
    ppo->env = env;
    ppo->net = true;
    ppo->net_spec = *spec;
    ppo->net_image = ppo_net_image(env->p.obs_dim, env->p.act_dim, *spec);
    (void)ppo_net_kernels_init();   // a refusal surfaces at the launch that needs the room
    return ppo_alloc(env, ppo, ppo->net_image.floats,
                     [&](float *img) { ppo_net_pack_log_std(ppo->net_image, nullptr, img); }, out);
}

int sng_ppo_set_weights(SngPpo *ppo, const SngMlpWeights *value_net, const float *log_std, void *stream) {
    if (!ppo) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null ppo handle");
    SngEnv *env = ppo->env;
    const PpoImage &m = ppo->image;
    const PpoNetImage &nm = ppo->net_image;
    std::string why;
    if (int rc = ppo->net ? ppo_net_weights_check(nm.v.O, nm.head.A, ppo->net_spec, value_net, log_std, &why)
                          : ppo_weights_check(m.v.O, m.A, m.v.activation, value_net, log_std, &why))
        return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, hipEventSynchronize(ppo->uploaded));   // the upload before this one has read the mirror
    if (ppo->net) ppo_net_pack(nm, ppo->net_spec, *value_net, log_std, ppo->h_img);
    else ppo_pack(m, *value_net, log_std, ppo->h_img);
    const size_t floats = ppo->net ? nm.floats : m.floats;
    HIP_TRY(env, hipMemcpyAsync(ppo->d_img, ppo->h_img, floats * sizeof(float), hipMemcpyHostToDevice, as_stream(stream)));
    HIP_TRY(env, hipEventRecord(ppo->uploaded, as_stream(stream)));
    return SNG_OK;
}

int sng_ppo_finish(SngPpo *ppo, const SngPpoRollout *rollout, void *stream) {
    if (!ppo) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null ppo handle");
    SngEnv *env = ppo->env;
    std::string why;
    if (int rc = ppo_rollout_check(rollout, true, &why)) return fail(env, rc, why);
    if (ppo->net) {
        // a day is a row of gae_scan_kernel's grid, and so is a step of the log-probability stage
        const int64_t steps = (rollout->noise && rollout->logp) ? env->p.T : 0;
        if ((int64_t)rollout->days + steps > kPpoMaxLaunchDays)
            return fail(env, SNG_ERR_INVALID_ARGUMENT,
                        "ppo rollout: days" + std::string(steps ? " + T (the log-probability stage's grid rows)" : "") +
                            " must be <= 65535 in one sng_ppo_finish");
        const int64_t blocks = ppo_net_blocks(ppo_net_rows(rollout->days, env->p.T, env->E));
        if (blocks > kPpoNetMaxBlocks)
            return fail(env, SNG_ERR_INVALID_ARGUMENT,
                        "ppo rollout: days * (T + 1) * num_envs / 64 = " + std::to_string(blocks) +
                            " workgroups of value_net_kernel are more than a grid's 2147483647");
        ON_DEVICE_OF(env);
        HIP_TRY(env, launch_ppo_net(ppo->d_img, ppo->net_image, *rollout, env->E, env->p.T, as_stream(stream)));
        return SNG_OK;
    }
    if (rollout->days > kPpoMaxLaunchDays)   // a day is a row of the launch's grid
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "ppo rollout: days must be <= 65535 in one sng_ppo_finish");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_rollout_gae(ppo->d_img, ppo->image, *rollout, env->E, env->p.T, as_stream(stream)));
    return SNG_OK;
}

void sng_ppo_destroy(SngPpo *ppo) {
    if (!ppo) return;
    DeviceScope scope(ppo->env->device);
    if (ppo->uploaded) {
        (void)hipEventSynchronize(ppo->uploaded);
        (void)hipEventDestroy(ppo->uploaded);
    }
    if (ppo->d_img) (void)hipFree(ppo->d_img);
    if (ppo->h_img) (void)hipHostFree(ppo->h_img);
    delete ppo;
}

int sng_ppo_host_finish(int32_t obs_dim, int32_t act_dim, int32_t activation, int32_t T, int64_t E,
                        const SngMlpWeights *value_net, const float *log_std, const SngPpoRollout *r, int values_given) {
    std::string why;
    if (int rc = ppo_dims_check(obs_dim, act_dim, activation, &why)) return fail(nullptr, rc, why);
    if (T < 1 || E < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "ppo rollout: T and E must be >= 1");
    if (int rc = ppo_rollout_check(r, values_given == 0, &why)) return fail(nullptr, rc, why);
    const PpoImage m = ppo_image(obs_dim, act_dim, activation);
    std::vector<float> img(m.floats);
    if (values_given && !value_net) {   // only log_std is packed
        if (int rc = ppo_log_std_check(act_dim, log_std, &why)) return fail(nullptr, rc, why);
        ppo_pack_log_std(m, log_std, img.data());
    } else {
        if (int rc = ppo_weights_check(obs_dim, act_dim, activation, value_net, log_std, &why)) return fail(nullptr, rc, why);
        ppo_pack(m, *value_net, log_std, img.data());
    }
    if (!values_given) ppo_values_host(m, img.data(), r->days, T, E, r->obs, r->values);
    ppo_gae_host(r->days, T, E, r->gamma, r->gae_lambda, r->reward, r->done, r->values, r->advantages, r->returns);
    if (r->noise && r->logp) ppo_logp_host(m, img.data(), r->days, T, E, r->noise, r->logp);
    return SNG_OK;
}

int sng_ppo_net_host_finish(int32_t obs_dim, int32_t act_dim, const SngPpoNetSpec *spec, int32_t T, int64_t E,
                            const SngMlpWeights *value_net, const float *log_std, const SngPpoRollout *r,
                            int values_given) {
    std::string why;
    if (int rc = ppo_net_spec_check(spec, obs_dim, act_dim, &why)) return fail(nullptr, rc, why);
    if (T < 1 || E < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "ppo rollout: T and E must be >= 1");
    if (int rc = ppo_rollout_check(r, values_given == 0, &why)) return fail(nullptr, rc, why);
    const PpoNetImage m = ppo_net_image(obs_dim, act_dim, *spec);
    std::vector<float> img(m.floats);
    if (values_given && !value_net) {   // only log_std is packed
        if (int rc = ppo_log_std_check(act_dim, log_std, &why)) return fail(nullptr, rc, why);
        ppo_net_pack_log_std(m, log_std, img.data());
    } else {
        if (int rc = ppo_net_weights_check(obs_dim, act_dim, *spec, value_net, log_std, &why)) return fail(nullptr, rc, why);
        ppo_net_pack(m, *spec, *value_net, log_std, img.data());
    }
    if (!values_given) ppo_net_values_host(m, img.data(), r->days, T, E, r->obs, r->values);
    ppo_gae_host(r->days, T, E, r->gamma, r->gae_lambda, r->reward, r->done, r->values, r->advantages, r->returns);
    if (r->noise && r->logp) ppo_logp_host(m.head, img.data(), r->days, T, E, r->noise, r->logp);
    return SNG_OK;
}

}  // extern "C"
