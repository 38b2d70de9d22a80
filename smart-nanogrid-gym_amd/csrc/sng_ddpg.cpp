// sng_ddpg.cpp -- the off-policy side of DDPG / TD3 behind the C ABI (include/sng.h): the replay ring's handle
// (sng_replay_*), the critic's (sng_critic_*), sng_policy_actions_rows, and the host-only sng_replay_host_indices,
// sng_critic_host_q and sng_critic_host_targets.  The contracts are sng_ddpg_host.h's on the host and sng_ddpg.h's on
// the device.
#include <vector>

#include "sng_env.h"

using namespace sng;

// A ring of a handle's envs: the caller's storage, the host bookkeeping and the sampler's counter.  It owns nothing
// on the device.
struct SngReplay {
    SngEnv *env = nullptr;
    SngReplaySpec spec{};
    ReplayRing ring;
    uint64_t counter = 0;
};

static ReplayStorage storage_of(const SngReplaySpec &s) {
    ReplayStorage r;
    r.obs = s.obs, r.actions = s.actions, r.reward = s.reward, r.done = s.done;
    return r;
}

// What the device and the host target calls share: the row arrays of a target call.
static int targets_args_check(SngEnv *env, int64_t rows, const float *next_obs, const float *reward, const float *done,
                              double gamma, const float *next_actions, const float *y) {
    std::string why;
    if (int rc = critic_gamma_check(gamma, &why)) return fail(env, rc, why);
    if (rows < 1) return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic targets: rows must be >= 1");
    if (!next_obs || !reward || !done || !next_actions || !y)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic targets: null argument");
    return SNG_OK;
}

extern "C" {

int sng_replay_create(SngEnv *env, const SngReplaySpec *spec, SngReplay **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    if (int rc = replay_spec_check(spec, &why)) return fail(env, rc, why);
    SngReplay *r = new SngReplay();
    r->env = env;
    r->spec = *spec;
    r->ring.capacity = spec->capacity_days;
    *out = r;
    return SNG_OK;
}

int sng_replay_push(SngReplay *r, int32_t days, const float *obs, const float *actions, const double *reward,
                    const uint8_t *done, void *stream) {
    if (!r) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null replay handle");
    SngEnv *env = r->env;
    std::string why;
    if (int rc = replay_push_check(r->ring, days, &why)) return fail(env, rc, why);
    if (!obs || !actions || !reward || !done) return fail(env, SNG_ERR_INVALID_ARGUMENT, "replay push: null argument");
    ReplaySource src;
    src.obs = obs, src.actions = actions, src.reward = reward, src.done = done;
    const PushArgs a = replay_push_args(r->ring, days, storage_of(r->spec), src, env->p.T, env->E, env->p.obs_dim,
                                        env->p.act_dim);
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_replay_push(a, as_stream(stream)));
    r->ring = replay_pushed(r->ring, days);
    return SNG_OK;
}

int64_t sng_replay_size(const SngReplay *r) {
    return r ? (int64_t)replay_size(r->ring, r->env->p.T, r->env->E) : 0;
}

int sng_replay_state(const SngReplay *r, int32_t *head, int32_t *filled) {
    if (!r) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null replay handle");
    if (head) *head = r->ring.head;
    if (filled) *filled = r->ring.filled;
    return SNG_OK;
}

int sng_replay_sample(SngReplay *r, int64_t batch, const SngReplayBatch *out, void *stream) {
    if (!r) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null replay handle");
    SngEnv *env = r->env;
    if (batch < 1) return fail(env, SNG_ERR_INVALID_ARGUMENT, "replay sample: batch must be >= 1");
    if (!out || !out->obs || !out->actions || !out->next_obs || !out->reward || !out->done)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "replay sample: null argument");
    const uint64_t n = replay_size(r->ring, env->p.T, env->E);
    if (n == 0) return fail(env, SNG_ERR_INVALID_ARGUMENT, "replay sample: the ring is empty");
    if ((batch + 63) / 64 > 2147483647ll)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "replay sample: batch / 64 workgroups are more than a grid's 2147483647");
    ON_DEVICE_OF(env);
    const uint32_t key = replay_sample_key(r->spec.seed, (uint64_t)env->p.env_offset, r->counter);
    HIP_TRY(env, launch_replay_sample(storage_of(r->spec), *out, key, n, env->p.T, env->E, env->p.obs_dim,
                                      env->p.act_dim, batch, as_stream(stream)));
    ++r->counter;
    return SNG_OK;
}

int sng_replay_get_counter(const SngReplay *r, uint64_t *out) {
    if (!r || !out) return fail(r ? r->env : nullptr, SNG_ERR_INVALID_ARGUMENT, "null argument");
    *out = r->counter;
    return SNG_OK;
}

int sng_replay_set_counter(SngReplay *r, uint64_t counter) {
    if (!r) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null replay handle");
    r->counter = counter;
    return SNG_OK;
}

void sng_replay_destroy(SngReplay *r) { delete r; }

int sng_replay_host_indices(uint64_t seed, int64_t env_offset, uint64_t counter, uint64_t n, int64_t batch,
                            int64_t *out) {
    if (n < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "replay sample: the ring is empty");
    if (batch < 1) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "replay sample: batch must be >= 1");
    if (!out) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "replay sample: null argument");
    replay_host_indices(seed, env_offset, counter, n, batch, out);
    return SNG_OK;
}

int sng_critic_create(SngEnv *env, const SngCriticSpec *spec, SngCritic **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    std::string why;
    const int O = env->p.obs_dim, A = env->p.act_dim;
    if (int rc = critic_spec_check(spec, O, A, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    (void)critic_kernels_init();   // a refusal surfaces at the launch that needs the room
    (void)policy_kernels_init();   // sng_critic_targets launches the target actor
    SngCritic *q = new SngCritic();
    q->env = env;
    q->spec = *spec;
    q->image = critic_image(O, A, *spec);
    hipError_t e = q->img.create(q->image.floats * sizeof(float));
    if (e == hipSuccess)
        e = q->img.upload_now([&](float *img) {
            for (size_t i = 0; i < q->image.floats; ++i) img[i] = 0.f;
        });
    if (e != hipSuccess) {
        sng_critic_destroy(q);
        return create_fail(env, e, "critic");
    }
    *out = q;
    return SNG_OK;
}

int sng_critic_set_weights(SngCritic *q, const SngMlpWeights *w, void *stream) {
    if (!q) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null critic handle");
    SngEnv *env = q->env;
    const int O = env->p.obs_dim, A = env->p.act_dim;
    std::string why;
    if (int rc = critic_weights_check(O, A, q->spec, w, &why)) return fail(env, rc, why);
    ON_DEVICE_OF(env);
    HIP_TRY(env, q->img.upload(as_stream(stream), [&](float *img) { critic_pack(q->image, O, A, q->spec, *w, img); }));
    return SNG_OK;
}

int sng_critic_q(SngCritic *q, int64_t rows, const float *obs, const float *actions, float *out, void *stream) {
    if (!q) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null critic handle");
    SngEnv *env = q->env;
    if (rows < 1) return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic q: rows must be >= 1");
    if (!obs || !actions || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic q: null argument");
    if (critic_blocks(rows) > kCriticMaxBlocks)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic q: rows / 64 workgroups are more than a grid's 2147483647");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_q_net(q->img.d, q->image, env->p.obs_dim, obs, actions, nullptr, nullptr, 0.f, out, rows,
                              as_stream(stream)));
    return SNG_OK;
}

int sng_critic_targets(SngCritic *q, SngPolicy *actor, int64_t rows, const float *next_obs, const float *reward,
                       const float *done, double gamma, float *next_actions, float *y, void *stream) {
    if (!q) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null critic handle");
    SngEnv *env = q->env;
    if (!actor) return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic targets: null target actor");
    if (actor->env != env) return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic targets: the target actor is another env's");
    if (!actor->net)
        return fail(env, SNG_ERR_UNSUPPORTED,
                    "critic targets: the target actor must be made by sng_policy_create_net (policy_net_kernel takes a "
                    "row count; the 64-64 policy_kernel does not)");
    SNG_TRY(targets_args_check(env, rows, next_obs, reward, done, gamma, next_actions, y));
    if (critic_blocks(rows) > kCriticMaxBlocks)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "critic targets: rows / 64 workgroups are more than a grid's 2147483647");
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    HIP_TRY(env, launch_policy_net(actor->img.d, actor->net_image, next_obs, nullptr, next_actions, nullptr, rows, st));
    HIP_TRY(env, launch_q_net(q->img.d, q->image, env->p.obs_dim, next_obs, next_actions, reward, done, (float)gamma, y,
                              rows, st));
    return SNG_OK;
}

void sng_critic_destroy(SngCritic *q) {
    if (!q) return;
    DeviceScope scope(q->env->device);
    q->img.destroy();
    delete q;
}

int sng_critic_host_q(int32_t obs_dim, int32_t act_dim, const SngCriticSpec *spec, const SngMlpWeights *w, int64_t rows,
                      const float *obs, const float *actions, float *out) {
    std::string why;
    if (int rc = critic_spec_check(spec, obs_dim, act_dim, &why)) return fail(nullptr, rc, why);
    if (int rc = critic_weights_check(obs_dim, act_dim, *spec, w, &why)) return fail(nullptr, rc, why);
    if (rows < 0 || (rows > 0 && (!obs || !actions || !out))) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "critic q: null argument");
    const NetImage m = critic_image(obs_dim, act_dim, *spec);
    std::vector<float> img(m.floats);
    critic_pack(m, obs_dim, act_dim, *spec, *w, img.data());
    critic_q_host(m, img.data(), obs_dim, act_dim, rows, obs, actions, out);
    return SNG_OK;
}

int sng_critic_host_targets(int32_t obs_dim, int32_t act_dim, const SngCriticSpec *spec, const SngMlpWeights *w,
                            const SngMlpNetSpec *actor_spec, const SngMlpWeights *actor_w, int64_t rows,
                            const float *next_obs, const float *reward, const float *done, double gamma,
                            float *next_actions, int next_actions_given, float *y) {
    std::string why;
    if (int rc = critic_spec_check(spec, obs_dim, act_dim, &why)) return fail(nullptr, rc, why);
    if (int rc = critic_weights_check(obs_dim, act_dim, *spec, w, &why)) return fail(nullptr, rc, why);
    SNG_TRY(targets_args_check(nullptr, rows, next_obs, reward, done, gamma, next_actions, y));
    if (!next_actions_given) {
        if (int rc = net_spec_check(actor_spec, obs_dim, act_dim, &why)) return fail(nullptr, rc, "target actor: " + why);
        if (int rc = net_weights_check(*actor_spec, actor_w, &why)) return fail(nullptr, rc, "target actor: " + why);
        const NetImage am = net_image(actor_spec->obs_dim, actor_spec->act_dim, actor_spec->hidden1, actor_spec->hidden2,
                                      actor_spec->activation, actor_spec->output, actor_spec->low != nullptr);
        std::vector<float> aimg(am.floats);
        net_pack(am, *actor_spec, *actor_w, aimg.data());
        mlp_net_host(am, aimg.data(), rows, next_obs, nullptr, next_actions, nullptr);
    }
    const NetImage m = critic_image(obs_dim, act_dim, *spec);
    std::vector<float> img(m.floats);
    critic_pack(m, obs_dim, act_dim, *spec, *w, img.data());
    critic_targets_host(m, img.data(), obs_dim, act_dim, rows, next_obs, next_actions, reward, done, gamma, y);
    return SNG_OK;
}

int sng_policy_actions_rows(SngPolicy *pol, int64_t rows, const float *obs, const float *noise, float *actions,
                            float *env_actions, void *stream) {
    if (!pol) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null policy handle");
    SngEnv *env = pol->env;
    if (!pol->net)
        return fail(env, SNG_ERR_UNSUPPORTED,
                    "sng_policy_actions_rows needs a policy made by sng_policy_create_net: policy_kernel runs the env's "
                    "num_envs rows only");
    if (rows < 1) return fail(env, SNG_ERR_INVALID_ARGUMENT, "policy actions: rows must be >= 1");
    if (!obs || !actions) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (critic_blocks(rows) > kCriticMaxBlocks)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "policy actions: rows / 64 workgroups are more than a grid's 2147483647");
    ON_DEVICE_OF(env);
    HIP_TRY(env, launch_policy_net(pol->img.d, pol->net_image, obs, noise, actions, env_actions, rows, as_stream(stream)));
    return SNG_OK;
}

}  // extern "C"
