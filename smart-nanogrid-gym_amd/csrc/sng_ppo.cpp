// sng_ppo.cpp -- the PPO head's handle (sng_ppo_create / create_net / set_weights / finish / destroy) and the host-only
// sng_ppo_host_finish and sng_ppo_net_host_finish.  The 64-64 head's arithmetic is sng_ppo_host.h's on the host and
// sng_ppo.h's on the device, the any-width head's sng_ppo_net_host.h's and sng_ppo_net.h's; one handle type serves
// both (PpoForm says which).
#include <vector>

#include "sng_env.h"

using namespace sng;

// A head's form: sng_ppo_create's 64-64 value net (image: sng_ppo_host.h) or, with `net`, sng_ppo_create_net's of any
// width (net_spec, net_image: sng_ppo_net_host.h), with the dims and the image's float count whichever it is.  What
// depends on the form is decided in the four functions below and in sng_ppo_finish, and nowhere else.
struct PpoForm {
    bool net = false;
    int O = 0, A = 0, H1 = 0, H2 = 0;
    size_t floats = 0;
    PpoImage image{};
    SngPpoNetSpec net_spec{};
    PpoNetImage net_image{};
};

static PpoForm ppo_form(int O, int A, int activation) {
    PpoForm f;
    f.O = O, f.A = A, f.H1 = f.H2 = kPolicyHidden;
    f.image = ppo_image(O, A, activation);
    f.floats = f.image.floats;
    return f;
}
static PpoForm ppo_net_form(int O, int A, const SngPpoNetSpec &spec) {
    PpoForm f;
    f.net = true;
    f.O = O, f.A = A, f.H1 = spec.hidden1, f.H2 = spec.hidden2;
    f.net_spec = spec;
    f.net_image = ppo_net_image(O, A, spec);
    f.floats = f.net_image.floats;
    return f;
}

static const GaussHead &form_head(const PpoForm &f) { return f.net ? f.net_image.head : f.image.head; }
static int form_weights_check(const PpoForm &f, const SngMlpWeights *w, const float *log_std, std::string *why) {
    return f.net ? ppo_net_weights_check(f.O, f.A, f.net_spec, w, log_std, why)
                 : ppo_weights_check(f.O, f.A, f.image.v.activation, w, log_std, why);
}
static void form_pack(const PpoForm &f, const SngMlpWeights &w, const float *log_std, float *img) {
    if (f.net) ppo_net_pack(f.net_image, f.net_spec, w, log_std, img);
    else ppo_pack(f.image, w, log_std, img);
}
static void form_values_host(const PpoForm &f, const float *img, int32_t days, int32_t T, int64_t E, const float *obs,
                             float *values) {
    if (f.net) ppo_net_values_host(f.net_image, img, days, T, E, obs, values);
    else ppo_values_host(f.image, img, days, T, E, obs, values);
}

// A head of a handle's envs: its form and the device image the finishing kernels read, which sng_ppo_set_weights packs
// and uploads.
struct SngPpo {
    SngEnv *env = nullptr;
    PpoForm form;
    UploadedImage img;
};

// What the two creates share: the image with log_std = 0 and no value net in it until the first upload.
static int ppo_create(SngEnv *env, const PpoForm &form, SngPpo **out) {
    SngPpo *ppo = new SngPpo();
    ppo->env = env;
    ppo->form = form;
    hipError_t e = ppo->img.create(form.floats * sizeof(float));
    if (e == hipSuccess)
        e = ppo->img.upload_now([&](float *img) { ppo_pack_log_std(form_head(form), form.floats, nullptr, img); });
    if (e != hipSuccess) {
        sng_ppo_destroy(ppo);
        return create_fail(env, e, "ppo");
    }
    *out = ppo;
    return SNG_OK;
}

// What the two host finishes share, behind their own checks of the dims.
static int ppo_host_finish(const PpoForm &f, int32_t T, int64_t E, const SngMlpWeights *value_net, const float *log_std,
                           const SngPpoRollout *r, int values_given) {
    std::string why;
    if (T < 1 || E < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "ppo rollout: T and E must be >= 1");
    if (int rc = ppo_rollout_check(r, values_given == 0, &why)) return fail(nullptr, rc, why);
    std::vector<float> img(f.floats);
    if (values_given && !value_net) {   // only log_std is packed
        if (int rc = ppo_log_std_check(f.A, log_std, &why)) return fail(nullptr, rc, why);
        ppo_pack_log_std(form_head(f), f.floats, log_std, img.data());
    } else {
        if (int rc = form_weights_check(f, value_net, log_std, &why)) return fail(nullptr, rc, why);
        form_pack(f, *value_net, log_std, img.data());
    }
    if (!values_given) form_values_host(f, img.data(), r->days, T, E, r->obs, r->values);
    ppo_gae_host(r->days, T, E, r->gamma, r->gae_lambda, r->reward, r->done, r->values, r->advantages, r->returns);
    if (r->noise && r->logp) ppo_logp_host(form_head(f), img.data(), r->days, T, E, r->noise, r->logp);
    return SNG_OK;
}

extern "C" {

int sng_ppo_create(SngEnv *env, int32_t activation, SngPpo **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = ppo_dims_check(env->p.obs_dim, env->p.act_dim, activation, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    (void)ppo_kernels_init();   // a refusal surfaces at the launch that needs the room
    return ppo_create(env, ppo_form(env->p.obs_dim, env->p.act_dim, activation), out);
}

int sng_ppo_create_net(SngEnv *env, const SngPpoNetSpec *spec, SngPpo **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = ppo_net_spec_check(spec, env->p.obs_dim, env->p.act_dim, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    (void)ppo_net_kernels_init();   // a refusal surfaces at the launch that needs the room
    return ppo_create(env, ppo_net_form(env->p.obs_dim, env->p.act_dim, *spec), out);
}

int sng_ppo_set_weights(SngPpo *ppo, const SngMlpWeights *value_net, const float *log_std, void *stream) {
    if (!ppo) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null ppo handle");
    SngEnv *env = ppo->env;
    std::string why;
    if (int rc = form_weights_check(ppo->form, value_net, log_std, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, ppo->img.upload(as_stream(stream), [&](float *img) { form_pack(ppo->form, *value_net, log_std, img); }));
    return SNG_OK;
}

int sng_ppo_finish(SngPpo *ppo, const SngPpoRollout *rollout, void *stream) {
    if (!ppo) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null ppo handle");
    SngEnv *env = ppo->env;
    std::string why;
    if (int rc = ppo_rollout_check(rollout, true, &why)) return fail(env, rc, why);
    if (ppo->form.net) {
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
        HIP_TRY(env, launch_ppo_net(ppo->img.d, ppo->form.net_image, *rollout, env->E, env->p.T, as_stream(stream)));
        return SNG_OK;
    }
    if (rollout->days > kPpoMaxLaunchDays)   // a day is a row of the launch's grid
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "ppo rollout: days must be <= 65535 in one sng_ppo_finish");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_rollout_gae(ppo->img.d, ppo->form.image, *rollout, env->E, env->p.T, as_stream(stream)));
    return SNG_OK;
}

void sng_ppo_destroy(SngPpo *ppo) {
    if (!ppo) return;
    DeviceScope scope(ppo->env->device);
    ppo->img.destroy();
    delete ppo;
}

int sng_ppo_host_finish(int32_t obs_dim, int32_t act_dim, int32_t activation, int32_t T, int64_t E,
                        const SngMlpWeights *value_net, const float *log_std, const SngPpoRollout *r, int values_given) {
    std::string why;
    if (int rc = ppo_dims_check(obs_dim, act_dim, activation, &why)) return fail(nullptr, rc, why);
    return ppo_host_finish(ppo_form(obs_dim, act_dim, activation), T, E, value_net, log_std, r, values_given);
}

int sng_ppo_net_host_finish(int32_t obs_dim, int32_t act_dim, const SngPpoNetSpec *spec, int32_t T, int64_t E,
                            const SngMlpWeights *value_net, const float *log_std, const SngPpoRollout *r,
                            int values_given) {
    std::string why;
    if (int rc = ppo_net_spec_check(spec, obs_dim, act_dim, &why)) return fail(nullptr, rc, why);
    return ppo_host_finish(ppo_net_form(obs_dim, act_dim, *spec), T, E, value_net, log_std, r, values_given);
}

}  // extern "C"
