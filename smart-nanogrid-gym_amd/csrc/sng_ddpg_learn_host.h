// sng_ddpg_learn_host.h -- DDPG's gradient step in host form (include/sng.h, sng_learner_create): one SB3 TD3.train
// iteration with one critic, policy_delay = 1 and no target noise, as a list of float32 expressions with a fixed
// operation order.  It is the contract: the kernels of sng_ddpg_learn.h give these values (==; the sign of a zero
// apart, as everywhere the MFMA appends zero terms to a chain), and Adam's step and the polyak blend are this header's
// own functions, compiled for the device as sng_ddpg_host.h's sampling law and TD target are.  No HIP: it compiles with
// plain g++ (tests/native/ddpg_learn_host_check.cpp); build with -ffp-contract=off.
//
// Arrays are plain row-major float32, weights in torch's nn.Linear layout [out][in].  A net is three layers
// (K -> H1 -> H2 -> N) with relu between them.
//   forward        out[b][j] = the fmaf chain over k ascending of in[b][k] * W[j][k], started from bias[j]; hidden
//                  layers keep relu(out) = out > 0 ? out : 0.
//   data gradient  dIn[b][i] = the fmaf chain over j ascending of dOut[b][j] * W[j][off + i], started from 0, then
//                  (hidden layers) kept where the layer's activation In[b][i] > 0 and 0 elsewhere.
//   weight grads   dW[j][i] = the fmaf chain over rows b ascending of dOut[b][j] * In[b][i], started from 0;
//                  db[j] the same with In = 1 (fmaf(d, 1, s) = s + d).  The rows are cut into segments of
//                  kLearnSegment; each segment is its own chain from 0 and the segments' partials are added in
//                  ascending order, g = p0, g = g + p1, ...; rows <= kLearnSegment is one chain.
//   critic step    q = Q(s, a);  dq[b] = (2 (q[b] - y[b])) / (float)B;  critic_loss = (sum_b (q[b] - y[b])^2) / (float)B,
//                  s = s + d * d in row order from 0, product and sum rounded on their own, by the weight gradients'
//                  segment law (a chain per kLearnSegment rows, the partials added in ascending order).
//   actor step     on the critic as updated: x = [s | a_pi], q_pi = Q(x); dq_pi[b] = -(1 / (float)B);
//                  actor_loss = -((sum_b q_pi[b]) / (float)B), the sum by the same law; the critic's data path down to the action columns of
//                  its input, dmean[b][j] = dx[b][O + j] * (1 - a_pi[b][j] * a_pi[b][j]), then the actor's layers.
//                  a_pi = tanh(mean) is the device's tanhf and an input here.
//   Adam, polyak   learn_adam and learn_polyak below, element by element.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sng.h"
#include "sng_ddpg_host.h"

namespace sng {

constexpr int kLearnSegment = SNG_LEARNER_SEGMENT;
constexpr int64_t kLearnMaxRows = SNG_LEARNER_MAX_ROWS;

// Adam's scalars of one step, all float32.  t is the step's number (1 for the first); the two bias corrections are
// computed in double: step_size = (float)(lr / (1 - beta1^t)), bc2_sqrt = (float)sqrt(1 - beta2^t).
struct LearnAdam {
    float beta1 = 0.f, one_m_beta1 = 0.f, beta2 = 0.f, one_m_beta2 = 0.f, step_size = 0.f, bc2_sqrt = 0.f, eps = 0.f;
};
inline LearnAdam learn_adam_scalars(double lr, double beta1, double beta2, double eps, int64_t t) {
    LearnAdam a;
    a.beta1 = (float)beta1;
    a.one_m_beta1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.one_m_beta2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)t));
    a.eps = (float)eps;
    return a;
}

// Division and square root, IEEE's correctly rounded ones on both sides: the device compiles `/` and llvm's sqrt
// without fast-math, which hipcc expands to the correctly rounded sequences (HIP's __fsqrt_rn is the native
// approximation and is not used).
SNG_NOISE_HD float learn_div(float a, float b) { return a / b; }
SNG_NOISE_HD float learn_sqrt(float a) { return __builtin_sqrtf(a); }

// torch.optim.Adam (no weight decay, no amsgrad) on one element, every operation rounded to float32 on its own; the
// square root and the two divisions are IEEE's correctly rounded ones on both sides:
//     m = beta1 m + (1 - beta1) g;   v = beta2 v + ((1 - beta2) g) g
//     p = p - step_size (m / (sqrt(v) / bc2_sqrt + eps))
SNG_NOISE_HD float learn_adam(float p, float g, float *m, float *v, const LearnAdam &a) {
    const float m1 = noise_add(noise_mul(a.beta1, *m), noise_mul(a.one_m_beta1, g));
    const float v1 = noise_add(noise_mul(a.beta2, *v), noise_mul(noise_mul(a.one_m_beta2, g), g));
    *m = m1;
    *v = v1;
    const float denom = noise_add(learn_div(learn_sqrt(v1), a.bc2_sqrt), a.eps);
    return noise_sub(p, noise_mul(a.step_size, learn_div(m1, denom)));
}

// SB3's polyak_update on one element: target = (1 - tau) target + tau p, tau = (float)tau and one_m_tau =
// (float)(1 - tau) from the double; products and sum rounded on their own.
SNG_NOISE_HD float learn_polyak(float target, float p, float tau, float one_m_tau) {
    return noise_add(noise_mul(one_m_tau, target), noise_mul(tau, p));
}

// dq of the critic's loss, dq_pi of the actor's, and what the actor's output stage passes down
SNG_NOISE_HD float learn_dq(float q, float y, float rows_f) {
    return learn_div(noise_mul(2.0f, noise_sub(q, y)), rows_f);
}
SNG_NOISE_HD float learn_dq_pi(float rows_f) {
    return -learn_div(1.0f, rows_f);
}
SNG_NOISE_HD float learn_dtanh(float dx, float a) { return noise_mul(dx, noise_sub(1.0f, noise_mul(a, a))); }
SNG_NOISE_HD float learn_mean_of(float sum, float rows_f) {
    return learn_div(sum, rows_f);
}

// --------------------------------------------------------------------------------- what the kernels are given
// One product C = epilogue(init + A B) of learn_gemm_kernel (sng_ddpg_learn.h) over plain arrays:
//     A(m, k) = a[m a_ms + k a_ks],  B(k, n) = b[k b_ks + n b_ns]  (column `ones` of B is 1.0: a bias gradient's In),
//     C(m, n) = c[z c_zs + m c_ms + n]  for the segment z of S k's (S >= K: one segment),
// every C(m, n) one fmaf chain over the segment's k ascending, started from init[n] (null: 0).
enum LearnEpilogue : int32_t {
    LEARN_EPI_NONE = 0,    // the chain
    LEARN_EPI_RELU = 1,    // chain > 0 ? chain : 0
    LEARN_EPI_MASK = 2,    // aux(m, n) > 0 ? chain : 0
    LEARN_EPI_TANH = 3,    // tanhf(chain), written to c and to c2(m, n) = c2[m c2_ms + n]
    LEARN_EPI_DTANH = 4    // learn_dtanh(chain, aux(m, n))
};
struct LearnGemm {
    const float *a = nullptr, *b = nullptr, *init = nullptr, *aux = nullptr;
    float *c = nullptr, *c2 = nullptr;
    int64_t a_ms = 0, a_ks = 0, b_ks = 0, b_ns = 0, aux_ms = 0, c_ms = 0, c_zs = 0, c2_ms = 0;
    int32_t M = 0, N = 0, K = 0, S = 0, ones = -1;
};
SNG_NOISE_HD int learn_segments(int64_t rows) { return (int)((rows + kLearnSegment - 1) / kLearnSegment); }

// Where W[j][k] of a layer padded to KP inputs sits in the layer's block of a NetImage: net_weight_at
// (sng_policy_net_host.h), for both sides.
SNG_NOISE_HD size_t learn_image_at(int KP, int j, int k) {
    const size_t t = (size_t)(j / 32), g = (size_t)(k / 8);
    const size_t lane = (size_t)((k & 1) * 32 + (j & 31)), i = (size_t)((k & 7) >> 1);
    return ((t * (size_t)(KP / 8) + g) * 64 + lane) * 4 + i;
}

// learn_step_kernel's arguments: a net's six arrays as tensors of n elements.  Element e of a weight [J][I] is
// (j, i) = (e / I, e % I), of a bias (I = 0) j = e; its gradient is the ordered sum of the nseg partials
// part[z zs + j (cols + 1) + (I ? i : cols)] (cols: the layer's inputs), and its place in a packed image
// img_at + (I ? learn_image_at(KP, j, i) : j).
struct LearnTensor {
    float *p = nullptr, *m = nullptr, *v = nullptr, *g = nullptr, *t = nullptr;
    const float *part = nullptr;
    uint64_t n = 0, zs = 0, img_at = 0;
    int32_t I = 0, cols = 0, KP = 0;
};
struct LearnStep {
    LearnTensor t[6];
    uint64_t total = 0;
    int32_t nseg = 1;
    LearnAdam adam;
    float tau = 0.f, one_m_tau = 0.f;
    float *img = nullptr, *img_target = nullptr;   // the net's and its target's packed images
};

// ------------------------------------------------------------------------------------------------------- validation
inline int learner_spec_check(const SngLearnerSpec *s, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!s) return no("null learner spec");
    const double v[6] = {s->actor_lr, s->critic_lr, s->tau, s->beta1, s->beta2, s->eps};
    for (double x : v)
        if (!std::isfinite(x)) return no("learner: the hyper-parameters must be finite");
    if (!(s->actor_lr > 0.0) || !(s->critic_lr > 0.0)) return no("learner: actor_lr and critic_lr must be > 0");
    if (!(s->tau >= 0.0 && s->tau <= 1.0)) return no("learner: tau " + std::to_string(s->tau) + " must be in [0, 1]");
    if (!(s->beta1 >= 0.0 && s->beta1 < 1.0) || !(s->beta2 >= 0.0 && s->beta2 < 1.0))
        return no("learner: beta1 and beta2 must be in [0, 1)");
    if (!(s->eps >= 0.0)) return no("learner: eps must be >= 0");
    return SNG_OK;
}

// The nets a learner takes: a squashed relu actor of sng_policy_create_net's form and a relu critic.
inline int learner_nets_check(const SngMlpNetSpec *actor, const SngCriticSpec *critic, std::string *why) {
    auto no = [&](int code, const std::string &msg) {
        if (why) *why = msg;
        return code;
    };
    if (!actor || !critic) return no(SNG_ERR_INVALID_ARGUMENT, "learner: null net spec");
    std::string inner;
    if (int rc = net_spec_check(actor, 0, 0, &inner)) return no(rc, "learner actor: " + inner);
    if (int rc = critic_spec_check(critic, actor->obs_dim, actor->act_dim, &inner)) return no(rc, "learner " + inner);
    if (actor->output != SNG_MLP_OUT_SQUASH)
        return no(SNG_ERR_UNSUPPORTED, "learner: the actor must have the squashed output (SNG_MLP_OUT_SQUASH), as DDPG's has");
    if (actor->activation != POLICY_RELU || critic->activation != POLICY_RELU)
        return no(SNG_ERR_UNSUPPORTED, "learner: hidden layers must be relu; tanh hidden layers have no backward pass here");
    return SNG_OK;
}

inline int learner_rows_check(int64_t rows, std::string *why) {
    if (rows < 1 || rows > kLearnMaxRows) {
        if (why) *why = "learner update: rows " + std::to_string(rows) + " must be 1 .. " + std::to_string(kLearnMaxRows);
        return SNG_ERR_INVALID_ARGUMENT;
    }
    return SNG_OK;
}

inline bool learn_arrays_given(const SngNetArrays &a) { return a.w1 && a.b1 && a.w2 && a.b2 && a.w3 && a.b3; }
inline bool learn_state_given(const SngLearnerState *s) {
    return s && learn_arrays_given(s->actor) && learn_arrays_given(s->critic) && learn_arrays_given(s->actor_target) &&
           learn_arrays_given(s->critic_target) && learn_arrays_given(s->actor_m) && learn_arrays_given(s->actor_v) &&
           learn_arrays_given(s->critic_m) && learn_arrays_given(s->critic_v);
}

// ------------------------------------------------------------------------------------------------------ arithmetic
// A net's dims and the sizes of its six arrays, in SngNetArrays' order.
struct LearnDims {
    int K = 0, H1 = 0, H2 = 0, N = 0;
    size_t size(int i) const {
        const size_t s[6] = {(size_t)H1 * (size_t)K, (size_t)H1, (size_t)H2 * (size_t)H1, (size_t)H2,
                             (size_t)N * (size_t)H2, (size_t)N};
        return s[i];
    }
    size_t floats() const {
        size_t n = 0;
        for (int i = 0; i < 6; ++i) n += size(i);
        return n;
    }
};
inline float *learn_array(const SngNetArrays &a, int i) {
    float *const p[6] = {a.w1, a.b1, a.w2, a.b2, a.w3, a.b3};
    return p[i];
}

inline void learn_forward_host(int64_t rows, int K, int N, const float *in, const float *W, const float *bias, bool relu,
                               float *out) {
    for (int64_t b = 0; b < rows; ++b)
        for (int j = 0; j < N; ++j) {
            float h = bias[j];
            for (int k = 0; k < K; ++k) h = std::fmaf(in[(size_t)b * K + k], W[(size_t)j * K + k], h);
            out[(size_t)b * N + j] = relu ? (h > 0.f ? h : 0.f) : h;
        }
}

// dIn [rows][I] from dOut [rows][J] and columns off .. off + I of W [J][ldw]; act [rows][I]: the mask, or null
inline void learn_backward_host(int64_t rows, int J, int I, const float *dOut, const float *W, int ldw, int off,
                                const float *act, float *dIn) {
    for (int64_t b = 0; b < rows; ++b)
        for (int i = 0; i < I; ++i) {
            float s = 0.f;
            for (int j = 0; j < J; ++j) s = std::fmaf(dOut[(size_t)b * J + j], W[(size_t)j * ldw + off + i], s);
            dIn[(size_t)b * I + i] = (!act || act[(size_t)b * I + i] > 0.f) ? s : 0.f;
        }
}

inline void learn_wgrad_host(int64_t rows, int J, int I, const float *dOut, const float *In, float *dW, float *db) {
    for (int j = 0; j < J; ++j)
        for (int i = 0; i <= I; ++i) {
            float g = 0.f;
            for (int64_t b0 = 0; b0 < rows; b0 += kLearnSegment) {
                const int64_t b1 = b0 + kLearnSegment < rows ? b0 + kLearnSegment : rows;
                float p = 0.f;
                for (int64_t b = b0; b < b1; ++b)
                    p = std::fmaf(dOut[(size_t)b * J + j], i < I ? In[(size_t)b * I + i] : 1.0f, p);
                g = b0 == 0 ? p : noise_add(g, p);
            }
            if (i < I) dW[(size_t)j * I + i] = g;
            else db[j] = g;
        }
}

// A loss's sum over the rows, by the weight gradients' segment law: term(b) added in row order from 0 within a segment
// of kLearnSegment rows, the segments' partials added in ascending order.
template <class Term>
inline float learn_loss_sum_host(int64_t rows, Term term) {
    float g = 0.f;
    for (int64_t b0 = 0; b0 < rows; b0 += kLearnSegment) {
        const int64_t b1 = b0 + kLearnSegment < rows ? b0 + kLearnSegment : rows;
        float p = 0.f;
        for (int64_t b = b0; b < b1; ++b) p = noise_add(p, term(b));
        g = b0 == 0 ? p : noise_add(g, p);
    }
    return g;
}
// the critic's term of row b: (q - y)^2, difference and product rounded on their own
SNG_NOISE_HD float learn_sq_error(float q, float y) {
    const float d = noise_sub(q, y);
    return noise_mul(d, d);
}

// A net's activations and gradients of one pass.
struct LearnPass {
    std::vector<float> h1, h2, out, dh2, dh1;
    void size(int64_t rows, const LearnDims &d) {
        h1.assign((size_t)rows * d.H1, 0.f), h2.assign((size_t)rows * d.H2, 0.f), out.assign((size_t)rows * d.N, 0.f);
        dh2.assign((size_t)rows * d.H2, 0.f), dh1.assign((size_t)rows * d.H1, 0.f);
    }
};
inline void learn_net_forward(const LearnDims &d, const SngNetArrays &w, int64_t rows, const float *x, LearnPass *p) {
    learn_forward_host(rows, d.K, d.H1, x, w.w1, w.b1, true, p->h1.data());
    learn_forward_host(rows, d.H1, d.H2, p->h1.data(), w.w2, w.b2, true, p->h2.data());
    learn_forward_host(rows, d.H2, d.N, p->h2.data(), w.w3, w.b3, false, p->out.data());
}
// dh2 and dh1 from dOut [rows][N]
inline void learn_net_backward(const LearnDims &d, const SngNetArrays &w, int64_t rows, const float *dOut, LearnPass *p) {
    learn_backward_host(rows, d.N, d.H2, dOut, w.w3, d.H2, 0, p->h2.data(), p->dh2.data());
    learn_backward_host(rows, d.H2, d.H1, p->dh2.data(), w.w2, d.H1, 0, p->h1.data(), p->dh1.data());
}
inline void learn_net_wgrads(const LearnDims &d, int64_t rows, const float *x, const float *dOut, const LearnPass &p,
                             const SngNetArrays &g) {
    learn_wgrad_host(rows, d.N, d.H2, dOut, p.h2.data(), g.w3, g.b3);
    learn_wgrad_host(rows, d.H2, d.H1, p.dh2.data(), p.h1.data(), g.w2, g.b2);
    learn_wgrad_host(rows, d.H1, d.K, p.dh1.data(), x, g.w1, g.b1);
}
// Adam on a net's six arrays, then the polyak blend of its target
inline void learn_net_step(const LearnDims &d, const SngNetArrays &w, const SngNetArrays &g, const SngNetArrays &m,
                           const SngNetArrays &v, const SngNetArrays &target, const LearnAdam &a, float tau,
                           float one_m_tau) {
    for (int i = 0; i < 6; ++i) {
        float *p = learn_array(w, i), *gi = learn_array(g, i), *mi = learn_array(m, i), *vi = learn_array(v, i),
              *ti = learn_array(target, i);
        for (size_t e = 0; e < d.size(i); ++e) {
            p[e] = learn_adam(p[e], gi[e], &mi[e], &vi[e], a);
            ti[e] = learn_polyak(ti[e], p[e], tau, one_m_tau);
        }
    }
}

inline void learn_concat_host(int64_t rows, int O, int A, const float *obs, const float *act, float *x) {
    const size_t K = (size_t)O + (size_t)A;
    for (int64_t b = 0; b < rows; ++b) {
        for (int k = 0; k < O; ++k) x[(size_t)b * K + k] = obs[(size_t)b * O + k];
        for (int k = 0; k < A; ++k) x[(size_t)b * K + O + k] = act[(size_t)b * A + k];
    }
}

// One update of `st` (masters, moments, targets, step) on a batch: obs [rows][O], actions [rows][A], y [rows],
// a_pi [rows][A] (the device's tanh of the updated-critic step's actor forward, or any stand-in for it).  The specs and
// the arrays have been checked.  trace: where given, q, dq, q_pi [rows], the twelve gradients and the two losses.
inline void learner_update_host(const SngMlpNetSpec &actor, const SngCriticSpec &critic, const SngLearnerSpec &spec,
                                SngLearnerState *st, int64_t rows, const float *obs, const float *actions,
                                const float *y, const float *a_pi, const SngLearnerTrace *trace) {
    const int O = actor.obs_dim, A = actor.act_dim;
    const LearnDims dc{O + A, critic.hidden1, critic.hidden2, 1}, da{O, actor.hidden1, actor.hidden2, A};
    const int64_t t = st->step + 1;
    const float rows_f = (float)rows, tau = (float)spec.tau, one_m_tau = (float)(1.0 - spec.tau);
    std::vector<float> gc_store(dc.floats()), ga_store(da.floats());
    auto carve = [](std::vector<float> &store, const LearnDims &d) {
        SngNetArrays a;
        float *p = store.data();
        float **f[6] = {&a.w1, &a.b1, &a.w2, &a.b2, &a.w3, &a.b3};
        for (int i = 0; i < 6; ++i) *f[i] = p, p += d.size(i);
        return a;
    };
    const SngNetArrays gc = carve(gc_store, dc), ga = carve(ga_store, da);
    std::vector<float> x((size_t)rows * dc.K), dq((size_t)rows);
    LearnPass pc, pa;
    pc.size(rows, dc), pa.size(rows, da);

    // the critic's step
    learn_concat_host(rows, O, A, obs, actions, x.data());
    learn_net_forward(dc, st->critic, rows, x.data(), &pc);
    float sum = learn_loss_sum_host(rows, [&](int64_t b) { return learn_sq_error(pc.out[b], y[b]); });
    for (int64_t b = 0; b < rows; ++b) dq[b] = learn_dq(pc.out[b], y[b], rows_f);
    if (trace && trace->critic_loss) *trace->critic_loss = learn_mean_of(sum, rows_f);
    if (trace && trace->q) for (int64_t b = 0; b < rows; ++b) trace->q[b] = pc.out[b];
    if (trace && trace->dq) for (int64_t b = 0; b < rows; ++b) trace->dq[b] = dq[b];
    learn_net_backward(dc, st->critic, rows, dq.data(), &pc);
    learn_net_wgrads(dc, rows, x.data(), dq.data(), pc, gc);
    learn_net_step(dc, st->critic, gc, st->critic_m, st->critic_v, st->critic_target,
                   learn_adam_scalars(spec.critic_lr, spec.beta1, spec.beta2, spec.eps, t), tau, one_m_tau);

    // the actor's step, on the critic as updated
    learn_net_forward(da, st->actor, rows, obs, &pa);
    learn_concat_host(rows, O, A, obs, a_pi, x.data());
    learn_net_forward(dc, st->critic, rows, x.data(), &pc);
    sum = learn_loss_sum_host(rows, [&](int64_t b) { return pc.out[b]; });
    for (int64_t b = 0; b < rows; ++b) dq[b] = learn_dq_pi(rows_f);
    if (trace && trace->actor_loss) *trace->actor_loss = -learn_mean_of(sum, rows_f);
    if (trace && trace->q_pi) for (int64_t b = 0; b < rows; ++b) trace->q_pi[b] = pc.out[b];
    learn_net_backward(dc, st->critic, rows, dq.data(), &pc);
    std::vector<float> dmean((size_t)rows * A);
    learn_backward_host(rows, dc.H1, A, pc.dh1.data(), st->critic.w1, dc.K, O, nullptr, dmean.data());
    for (size_t e = 0; e < dmean.size(); ++e) dmean[e] = learn_dtanh(dmean[e], a_pi[e]);
    learn_net_backward(da, st->actor, rows, dmean.data(), &pa);
    learn_net_wgrads(da, rows, obs, dmean.data(), pa, ga);
    learn_net_step(da, st->actor, ga, st->actor_m, st->actor_v, st->actor_target,
                   learn_adam_scalars(spec.actor_lr, spec.beta1, spec.beta2, spec.eps, t), tau, one_m_tau);
    st->step = t;

    if (trace)
        for (int i = 0; i < 6; ++i) {
            if (float *o = learn_array(trace->critic_grad, i))
                for (size_t e = 0; e < dc.size(i); ++e) o[e] = learn_array(gc, i)[e];
            if (float *o = learn_array(trace->actor_grad, i))
                for (size_t e = 0; e < da.size(i); ++e) o[e] = learn_array(ga, i)[e];
        }
}

}  // namespace sng
