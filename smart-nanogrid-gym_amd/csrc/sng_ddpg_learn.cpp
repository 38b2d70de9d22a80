// sng_ddpg_learn.cpp -- DDPG's gradient step behind the C ABI (include/sng.h): the learner's handle (sng_learner_*) and
// the host-only sng_learner_host_update.  The contract is sng_ddpg_learn_host.h's on the host and sng_ddpg_learn.h's on
// the device; this file owns the arrays and puts an update's launches in their order.
#include <vector>

#include "sng_env.h"

using namespace sng;

namespace {

// A net's six device arrays inside one allocation, in SngNetArrays' order.
SngNetArrays carve(float *&at, const LearnDims &d) {
    SngNetArrays a;
    float **f[6] = {&a.w1, &a.b1, &a.w2, &a.b2, &a.w3, &a.b3};
    for (int i = 0; i < 6; ++i) *f[i] = at, at += d.size(i);
    return a;
}

// What an update needs per row, and the partials of the weight gradients per segment.
struct LearnWork {
    float *base = nullptr;
    int64_t rows = 0;   // the rows it was made for
    float *x = nullptr, *q = nullptr, *dq = nullptr, *dq_pi = nullptr, *q_pi = nullptr, *a_pi = nullptr, *dmean = nullptr;
    float *c_h1 = nullptr, *c_h2 = nullptr, *c_dh1 = nullptr, *c_dh2 = nullptr;
    float *a_h1 = nullptr, *a_h2 = nullptr, *a_dh1 = nullptr, *a_dh2 = nullptr;
    float *c_part[3] = {nullptr, nullptr, nullptr}, *a_part[3] = {nullptr, nullptr, nullptr};   // layers 1, 2, 3
};

size_t part_floats(const LearnDims &d, int layer) {
    const size_t J[3] = {(size_t)d.H1, (size_t)d.H2, (size_t)d.N}, I[3] = {(size_t)d.K, (size_t)d.H1, (size_t)d.H2};
    return J[layer] * (I[layer] + 1);
}

}  // namespace

struct SngLearner {
    SngEnv *env = nullptr;
    SngPolicy *actor = nullptr, *actor_target = nullptr;
    SngCritic *critic = nullptr, *critic_target = nullptr;
    SngLearnerSpec spec{};
    LearnDims da, dc;
    int64_t step = 0;
    float *store = nullptr;                      // the ten nets' worth of arrays and the two losses
    SngNetArrays arrays[SNG_LEARNER_ARRAYS]{};
    float *losses = nullptr;                     // critic_loss, actor_loss
    LearnWork work;
    int64_t last_rows = 0;
};

static bool actor_like(int which) {
    return which == SNG_LEARNER_ACTOR || which == SNG_LEARNER_ACTOR_TARGET || which == SNG_LEARNER_ACTOR_M ||
           which == SNG_LEARNER_ACTOR_V || which == SNG_LEARNER_ACTOR_GRAD;
}

// The workspace for `rows` rows; grown (freed and allocated anew, which synchronises) when rows exceed it.
static hipError_t ensure_work(SngLearner *L, int64_t rows) {
    LearnWork &w = L->work;
    if (rows <= w.rows) return hipSuccess;
    if (w.base) {
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        (void)hipFree(w.base);
        w = LearnWork{};
        L->last_rows = 0;   // the last update's outputs went with the block
    }
    const LearnDims &da = L->da, &dc = L->dc;
    const size_t R = (size_t)rows, nseg = (size_t)learn_segments(rows);
    const size_t A = (size_t)da.N;
    size_t total = R * (size_t)dc.K + 4 * R + 2 * R * A + 2 * R * (size_t)(dc.H1 + dc.H2) + 2 * R * (size_t)(da.H1 + da.H2);
    for (int l = 0; l < 3; ++l) total += nseg * (part_floats(dc, l) + part_floats(da, l));
    float *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, total * sizeof(float));
    if (e != hipSuccess) return e;
    float *at = base;
    auto take = [&](size_t n) {
        float *p = at;
        at += n;
        return p;
    };
    w.base = base, w.rows = rows;
    w.x = take(R * (size_t)dc.K), w.q = take(R), w.dq = take(R), w.dq_pi = take(R), w.q_pi = take(R);
    w.a_pi = take(R * A), w.dmean = take(R * A);
    w.c_h1 = take(R * (size_t)dc.H1), w.c_dh1 = take(R * (size_t)dc.H1);
    w.c_h2 = take(R * (size_t)dc.H2), w.c_dh2 = take(R * (size_t)dc.H2);
    w.a_h1 = take(R * (size_t)da.H1), w.a_dh1 = take(R * (size_t)da.H1);
    w.a_h2 = take(R * (size_t)da.H2), w.a_dh2 = take(R * (size_t)da.H2);
    for (int l = 0; l < 3; ++l) w.c_part[l] = take(nseg * part_floats(dc, l)), w.a_part[l] = take(nseg * part_floats(da, l));
    return hipSuccess;
}

// out [rows][N] = epilogue(bias + in [rows][K] W^T)
static hipError_t forward(int64_t rows, int K, int N, const float *in, const float *W, const float *bias, float *out,
                          int epi, hipStream_t st, float *c2 = nullptr, int64_t c2_ms = 0) {
    LearnGemm g;
    g.a = in, g.a_ms = K, g.a_ks = 1;
    g.b = W, g.b_ns = K, g.b_ks = 1;
    g.init = bias;
    g.c = out, g.c_ms = N, g.c2 = c2, g.c2_ms = c2_ms;
    g.M = (int32_t)rows, g.N = N, g.K = K, g.S = K;
    return launch_learn_gemm(g, epi, st);
}
// dIn [rows][I] = epilogue(dOut [rows][J] W[:, off .. off + I)), W [J][ldw]
static hipError_t backward(int64_t rows, int J, int I, const float *dOut, const float *W, int ldw, int off,
                           const float *aux, float *dIn, int epi, hipStream_t st) {
    LearnGemm g;
    g.a = dOut, g.a_ms = J, g.a_ks = 1;
    g.b = W + off, g.b_ks = ldw, g.b_ns = 1;
    g.aux = aux, g.aux_ms = I;
    g.c = dIn, g.c_ms = I;
    g.M = (int32_t)rows, g.N = I, g.K = J, g.S = J;
    return launch_learn_gemm(g, epi, st);
}
// part [segment][J][I + 1] = dOut^T [In | 1], a segment's rows at a time
static hipError_t wgrad(int64_t rows, int J, int I, const float *dOut, const float *In, float *part, hipStream_t st) {
    LearnGemm g;
    g.a = dOut, g.a_ms = 1, g.a_ks = J;
    g.b = In, g.b_ks = I, g.b_ns = 1, g.ones = I;
    g.c = part, g.c_ms = I + 1, g.c_zs = (int64_t)J * (I + 1);
    g.M = J, g.N = I + 1, g.K = (int32_t)rows, g.S = kLearnSegment;
    return launch_learn_gemm(g, LEARN_EPI_NONE, st);
}

static LearnStep step_args(const LearnDims &d, const NetImage &m, const SngNetArrays &p, const SngNetArrays &mm,
                           const SngNetArrays &v, const SngNetArrays &g, const SngNetArrays &t, float *const part[3],
                           float *img, float *img_target) {
    LearnStep s;
    const int I[3] = {d.K, d.H1, d.H2}, KP[3] = {m.K1, m.K2, m.K3};
    const size_t w_at[3] = {m.w1, m.w2, m.w3}, b_at[3] = {m.b1, m.b2, m.b3};
    for (int i = 0; i < 6; ++i) {
        const int l = i / 2;
        LearnTensor &x = s.t[i];
        x.p = learn_array(p, i), x.m = learn_array(mm, i), x.v = learn_array(v, i), x.g = learn_array(g, i);
        x.t = learn_array(t, i);
        x.part = part[l];
        x.n = d.size(i);
        x.zs = part_floats(d, l);
        x.cols = I[l];
        x.I = i % 2 == 0 ? I[l] : 0;
        x.KP = KP[l];
        x.img_at = i % 2 == 0 ? w_at[l] : b_at[l];
        s.total += x.n;
    }
    s.img = img, s.img_target = img_target;
    return s;
}

static LearnStep net_step(SngLearner *L, bool is_actor) {
    const LearnWork &w = L->work;
    if (is_actor)
        return step_args(L->da, L->actor->net_image, L->arrays[SNG_LEARNER_ACTOR], L->arrays[SNG_LEARNER_ACTOR_M],
                         L->arrays[SNG_LEARNER_ACTOR_V], L->arrays[SNG_LEARNER_ACTOR_GRAD],
                         L->arrays[SNG_LEARNER_ACTOR_TARGET], w.a_part, L->actor->img.d, L->actor_target->img.d);
    return step_args(L->dc, L->critic->image, L->arrays[SNG_LEARNER_CRITIC], L->arrays[SNG_LEARNER_CRITIC_M],
                     L->arrays[SNG_LEARNER_CRITIC_V], L->arrays[SNG_LEARNER_CRITIC_GRAD],
                     L->arrays[SNG_LEARNER_CRITIC_TARGET], w.c_part, L->critic->img.d, L->critic_target->img.d);
}

static SngMlpNetSpec actor_spec_of(const SngPolicy *p) {
    SngMlpNetSpec s = p->net_spec;
    s.low = p->clip_low.empty() ? nullptr : p->clip_low.data();
    s.high = p->clip_high.empty() ? nullptr : p->clip_high.data();
    return s;
}

extern "C" {

int sng_learner_create(SngEnv *env, SngPolicy *actor, SngPolicy *actor_target, SngCritic *critic,
                       SngCritic *critic_target, const SngLearnerSpec *spec, SngLearner **out) {
    if (!env || !out) return fail(env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (!actor || !actor_target || !critic || !critic_target)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner: null net handle");
    if (actor->env != env || actor_target->env != env || critic->env != env || critic_target->env != env)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner: a net handle is another env's");
    if (actor == actor_target || critic == critic_target)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner: a net and its target must be two handles");
    if (!actor->net || !actor_target->net)
        return fail(env, SNG_ERR_UNSUPPORTED,
                    "learner: the actor and its target must be made by sng_policy_create_net with the squashed output "
                    "(the 64-64 policy_kernel actor has no packed image of that form)");
    std::string why;
    if (int rc = learner_spec_check(spec, &why)) return fail(env, rc, why);
    const SngMlpNetSpec as = actor_spec_of(actor), ts = actor_spec_of(actor_target);
    if (int rc = learner_nets_check(&as, &critic->spec, &why)) return fail(env, rc, why);
    if (as.hidden1 != ts.hidden1 || as.hidden2 != ts.hidden2 || as.activation != ts.activation || as.output != ts.output)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner: the actor and its target differ in widths, activation or output");
    if (critic->spec.hidden1 != critic_target->spec.hidden1 || critic->spec.hidden2 != critic_target->spec.hidden2 ||
        critic->spec.activation != critic_target->spec.activation)
        return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner: the critic and its target differ in widths or activation");
    ON_DEVICE_OF(env);
    SngLearner *L = new SngLearner();
    L->env = env, L->actor = actor, L->actor_target = actor_target, L->critic = critic, L->critic_target = critic_target;
    L->spec = *spec;
    const int O = env->p.obs_dim, A = env->p.act_dim;
    L->da = LearnDims{O, as.hidden1, as.hidden2, A};
    L->dc = LearnDims{O + A, critic->spec.hidden1, critic->spec.hidden2, 1};
    const size_t floats = 5 * (L->da.floats() + L->dc.floats()) + 2;
    hipError_t e = hipMalloc((void **)&L->store, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(L->store, 0, floats * sizeof(float));
    if (e != hipSuccess) {
        sng_learner_destroy(L);
        return create_fail(env, e, "learner");
    }
    float *at = L->store;
    for (int i = 0; i < SNG_LEARNER_ARRAYS; ++i) L->arrays[i] = carve(at, actor_like(i) ? L->da : L->dc);
    L->losses = at;
    *out = L;
    return SNG_OK;
}

int sng_learner_update(SngLearner *L, int64_t rows, const float *obs, const float *actions, const float *y,
                       void *stream) {
    if (!L) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null learner handle");
    SngEnv *env = L->env;
    std::string why;
    if (int rc = learner_rows_check(rows, &why)) return fail(env, rc, why);
    if (!obs || !actions || !y) return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner update: null argument");
    ON_DEVICE_OF(env);
    HIP_TRY(env, ensure_work(L, rows));
    hipStream_t st = as_stream(stream);
    const LearnWork &w = L->work;
    const LearnDims &da = L->da, &dc = L->dc;
    const int O = da.K, A = da.N;
    const SngNetArrays &qa = L->arrays[SNG_LEARNER_CRITIC], &pa = L->arrays[SNG_LEARNER_ACTOR];
    const int64_t t = L->step + 1;
    const float tau = (float)L->spec.tau, one_m_tau = (float)(1.0 - L->spec.tau);
    const int nseg = learn_segments(rows);

    // the critic's forward pass over x = [obs | a]; q, h1 and h2 stay in the workspace for the backward pass
    auto critic_forward = [&](float *q) -> hipError_t {
        hipError_t e = forward(rows, dc.K, dc.H1, w.x, qa.w1, qa.b1, w.c_h1, LEARN_EPI_RELU, st);
        if (e == hipSuccess) e = forward(rows, dc.H1, dc.H2, w.c_h1, qa.w2, qa.b2, w.c_h2, LEARN_EPI_RELU, st);
        if (e == hipSuccess) e = forward(rows, dc.H2, 1, w.c_h2, qa.w3, qa.b3, q, LEARN_EPI_NONE, st);
        return e;
    };
    // dq [rows][1] down to dh2 and dh1
    auto critic_backward = [&](const float *dq) -> hipError_t {
        hipError_t e = backward(rows, 1, dc.H2, dq, qa.w3, dc.H2, 0, w.c_h2, w.c_dh2, LEARN_EPI_MASK, st);
        if (e == hipSuccess) e = backward(rows, dc.H2, dc.H1, w.c_dh2, qa.w2, dc.H1, 0, w.c_h1, w.c_dh1, LEARN_EPI_MASK, st);
        return e;
    };

    // 1. the critic's step
    HIP_TRY(env, launch_learn_concat(obs, actions, w.x, rows, O, A, st));
    HIP_TRY(env, critic_forward(w.q));
    HIP_TRY(env, launch_learn_loss(false, w.q, y, w.dq, L->losses, rows, st));
    HIP_TRY(env, critic_backward(w.dq));
    HIP_TRY(env, wgrad(rows, 1, dc.H2, w.dq, w.c_h2, w.c_part[2], st));
    HIP_TRY(env, wgrad(rows, dc.H2, dc.H1, w.c_dh2, w.c_h1, w.c_part[1], st));
    HIP_TRY(env, wgrad(rows, dc.H1, dc.K, w.c_dh1, w.x, w.c_part[0], st));
    {
        LearnStep s = net_step(L, false);
        s.nseg = nseg, s.tau = tau, s.one_m_tau = one_m_tau;
        s.adam = learn_adam_scalars(L->spec.critic_lr, L->spec.beta1, L->spec.beta2, L->spec.eps, t);
        HIP_TRY(env, launch_learn_step(s, true, st));
    }

    // 2. the actor's step, on the critic as updated; the actor's output stage writes a_pi and x's action columns
    HIP_TRY(env, forward(rows, da.K, da.H1, obs, pa.w1, pa.b1, w.a_h1, LEARN_EPI_RELU, st));
    HIP_TRY(env, forward(rows, da.H1, da.H2, w.a_h1, pa.w2, pa.b2, w.a_h2, LEARN_EPI_RELU, st));
    HIP_TRY(env, forward(rows, da.H2, A, w.a_h2, pa.w3, pa.b3, w.a_pi, LEARN_EPI_TANH, st, w.x + O, dc.K));
    HIP_TRY(env, critic_forward(w.q_pi));
    HIP_TRY(env, launch_learn_loss(true, w.q_pi, nullptr, w.dq_pi, L->losses + 1, rows, st));
    HIP_TRY(env, critic_backward(w.dq_pi));
    HIP_TRY(env, backward(rows, dc.H1, A, w.c_dh1, qa.w1, dc.K, O, w.a_pi, w.dmean, LEARN_EPI_DTANH, st));
    HIP_TRY(env, backward(rows, A, da.H2, w.dmean, pa.w3, da.H2, 0, w.a_h2, w.a_dh2, LEARN_EPI_MASK, st));
    HIP_TRY(env, backward(rows, da.H2, da.H1, w.a_dh2, pa.w2, da.H1, 0, w.a_h1, w.a_dh1, LEARN_EPI_MASK, st));
    HIP_TRY(env, wgrad(rows, A, da.H2, w.dmean, w.a_h2, w.a_part[2], st));
    HIP_TRY(env, wgrad(rows, da.H2, da.H1, w.a_dh2, w.a_h1, w.a_part[1], st));
    HIP_TRY(env, wgrad(rows, da.H1, da.K, w.a_dh1, obs, w.a_part[0], st));
    {
        LearnStep s = net_step(L, true);
        s.nseg = nseg, s.tau = tau, s.one_m_tau = one_m_tau;
        s.adam = learn_adam_scalars(L->spec.actor_lr, L->spec.beta1, L->spec.beta2, L->spec.eps, t);
        HIP_TRY(env, launch_learn_step(s, true, st));
    }
    L->step = t;
    L->last_rows = rows;
    return SNG_OK;
}

int sng_learner_arrays(SngLearner *L, int which, SngNetArrays *out) {
    if (!L) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null learner handle");
    if (!out || which < 0 || which >= SNG_LEARNER_ARRAYS)
        return fail(L->env, SNG_ERR_INVALID_ARGUMENT, "learner arrays: `which` must be one of SNG_LEARNER_*");
    *out = L->arrays[which];
    return SNG_OK;
}

int sng_learner_last(SngLearner *L, SngLearnerLast *out) {
    if (!L) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null learner handle");
    if (!out) return fail(L->env, SNG_ERR_INVALID_ARGUMENT, "null argument");
    if (L->last_rows < 1) return fail(L->env, SNG_ERR_STATE, "learner: no update yet");
    const LearnWork &w = L->work;
    *out = SngLearnerLast{L->last_rows, w.q, w.dq, w.a_pi, w.q_pi, L->losses, L->losses + 1};
    return SNG_OK;
}

int sng_learner_get_step(const SngLearner *L, int64_t *out) {
    if (!L || !out) return fail(L ? L->env : nullptr, SNG_ERR_INVALID_ARGUMENT, "null argument");
    *out = L->step;
    return SNG_OK;
}

// the eight nets' worth of arrays of a state, in SNG_LEARNER_* order
static void state_arrays(const SngLearnerState &s, const SngNetArrays *(&a)[8]) {
    a[SNG_LEARNER_ACTOR] = &s.actor, a[SNG_LEARNER_CRITIC] = &s.critic;
    a[SNG_LEARNER_ACTOR_TARGET] = &s.actor_target, a[SNG_LEARNER_CRITIC_TARGET] = &s.critic_target;
    a[SNG_LEARNER_ACTOR_M] = &s.actor_m, a[SNG_LEARNER_ACTOR_V] = &s.actor_v;
    a[SNG_LEARNER_CRITIC_M] = &s.critic_m, a[SNG_LEARNER_CRITIC_V] = &s.critic_v;
}

int sng_learner_set_state(SngLearner *L, const SngLearnerState *state, void *stream) {
    if (!L) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null learner handle");
    SngEnv *env = L->env;
    if (!learn_state_given(state)) return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner state: null argument");
    if (state->step < 0) return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner state: step must be >= 0");
    const SngNetArrays *src[8];
    state_arrays(*state, src);
    for (int which = 0; which < 8; ++which) {
        const LearnDims &d = actor_like(which) ? L->da : L->dc;
        for (int i = 0; i < 6; ++i)
            for (size_t e = 0; e < d.size(i); ++e)
                if (!std::isfinite(learn_array(*src[which], i)[e]))
                    return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner state: non-finite value");
    }
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    for (int which = 0; which < 8; ++which) {
        const LearnDims &d = actor_like(which) ? L->da : L->dc;
        for (int i = 0; i < 6; ++i)
            HIP_TRY(env, hipMemcpyAsync(learn_array(L->arrays[which], i), learn_array(*src[which], i),
                                        d.size(i) * sizeof(float), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(env, launch_learn_step(net_step(L, false), false, st));
    HIP_TRY(env, launch_learn_step(net_step(L, true), false, st));
    HIP_TRY(env, hipStreamSynchronize(st));
    L->step = state->step;
    return SNG_OK;
}

int sng_learner_get_state(SngLearner *L, const SngLearnerState *state, int64_t *step_out, void *stream) {
    if (!L) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "null learner handle");
    SngEnv *env = L->env;
    if (!learn_state_given(state)) return fail(env, SNG_ERR_INVALID_ARGUMENT, "learner state: null argument");
    const SngNetArrays *dst[8];
    state_arrays(*state, dst);
    ON_DEVICE_OF(env);
    hipStream_t st = as_stream(stream);
    for (int which = 0; which < 8; ++which) {
        const LearnDims &d = actor_like(which) ? L->da : L->dc;
        for (int i = 0; i < 6; ++i)
            HIP_TRY(env, hipMemcpyAsync(learn_array(*dst[which], i), learn_array(L->arrays[which], i),
                                        d.size(i) * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(env, hipStreamSynchronize(st));
    if (step_out) *step_out = L->step;
    return SNG_OK;
}

void sng_learner_destroy(SngLearner *L) {
    if (!L) return;
    DeviceScope scope(L->env->device);
    if (L->work.base) (void)hipFree(L->work.base);
    if (L->store) (void)hipFree(L->store);
    delete L;
}

int sng_learner_host_update(const SngMlpNetSpec *actor_spec, const SngCriticSpec *critic_spec,
                            const SngLearnerSpec *spec, SngLearnerState *state, int64_t rows, const float *obs,
                            const float *actions, const float *y, const float *a_pi, const SngLearnerTrace *trace) {
    std::string why;
    if (int rc = learner_spec_check(spec, &why)) return fail(nullptr, rc, why);
    if (int rc = learner_nets_check(actor_spec, critic_spec, &why)) return fail(nullptr, rc, why);
    if (int rc = learner_rows_check(rows, &why)) return fail(nullptr, rc, why);
    if (!learn_state_given(state)) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "learner state: null argument");
    if (state->step < 0) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "learner state: step must be >= 0");
    if (!obs || !actions || !y || !a_pi) return fail(nullptr, SNG_ERR_INVALID_ARGUMENT, "learner update: null argument");
    learner_update_host(*actor_spec, *critic_spec, *spec, state, rows, obs, actions, y, a_pi, trace);
    return SNG_OK;
}

}  // extern "C"
