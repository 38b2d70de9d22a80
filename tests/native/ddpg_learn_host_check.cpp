// The host model of DDPG's gradient step (csrc/sng_ddpg_learn_host.h, learner_update_host) against naive loops written
// from the formulas of include/sng.h, bitwise: nets (8, 8), (33, 65) and (400, 300), batches of 1, 63, 64, 65, S, S + 1
// and 2 S + 37 rows (S = SNG_LEARNER_SEGMENT), critic input widths O + A of 13 and 160; the two narrower nets take two
// updates in a row (the second with non-zero moments and t = 2).  Four more cases take one state through batches in
// descending order (2 S + 37, 200, 1, 64, 33, S + 1, 7), and through SNG_LEARNER_MAX_ROWS - 1 and SNG_LEARNER_MAX_ROWS
// rows (64 segments, the last of S - 1 and of S rows) with 64 rows behind them.  The cases run on a few threads; build
// with -ffp-contract=off -pthread.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "sng_ddpg_learn_host.h"

using namespace sng;
typedef std::vector<float> V;

namespace {

struct Rng {
    uint64_t s;
    float uniform(float lo, float hi) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return lo + (hi - lo) * (float)((s >> 40) & 0xffffff) / 16777216.0f;
    }
};

struct Net {   // K -> H1 -> H2 -> N
    int K, H1, H2, N;
    V w1, b1, w2, b2, w3, b3;
    void init(int k, int h1, int h2, int n, Rng &r, float out_scale) {
        K = k, H1 = h1, H2 = h2, N = n;
        auto fill = [&](V &w, V &b, int out, int in, float scale) {
            const float a = scale / std::sqrt((float)in);
            w.resize((size_t)out * in), b.resize(out);
            for (float &x : w) x = r.uniform(-a, a);
            for (float &x : b) x = r.uniform(-a, a);
        };
        fill(w1, b1, h1, k, 1.f), fill(w2, b2, h2, h1, 1.f), fill(w3, b3, n, h2, out_scale);
    }
    void zero_like(const Net &o) {
        *this = o;
        for (V *v : {&w1, &b1, &w2, &b2, &w3, &b3}) std::fill(v->begin(), v->end(), 0.f);
    }
    SngNetArrays arrays() { return SngNetArrays{w1.data(), b1.data(), w2.data(), b2.data(), w3.data(), b3.data()}; }
    V *all(int i) {
        V *p[6] = {&w1, &b1, &w2, &b2, &w3, &b3};
        return p[i];
    }
};

struct Pass {
    V h1, h2, out;
};

// ---- the naive side: every formula as a loop of its own
Pass naive_forward(const Net &n, int B, const V &x) {
    Pass p;
    p.h1.resize((size_t)B * n.H1), p.h2.resize((size_t)B * n.H2), p.out.resize((size_t)B * n.N);
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < n.H1; ++j) {
            float h = n.b1[j];
            for (int k = 0; k < n.K; ++k) h = std::fmaf(x[(size_t)b * n.K + k], n.w1[(size_t)j * n.K + k], h);
            p.h1[(size_t)b * n.H1 + j] = h > 0.f ? h : 0.f;
        }
        for (int j = 0; j < n.H2; ++j) {
            float h = n.b2[j];
            for (int k = 0; k < n.H1; ++k) h = std::fmaf(p.h1[(size_t)b * n.H1 + k], n.w2[(size_t)j * n.H1 + k], h);
            p.h2[(size_t)b * n.H2 + j] = h > 0.f ? h : 0.f;
        }
        for (int j = 0; j < n.N; ++j) {
            float h = n.b3[j];
            for (int k = 0; k < n.H2; ++k) h = std::fmaf(p.h2[(size_t)b * n.H2 + k], n.w3[(size_t)j * n.H2 + k], h);
            p.out[(size_t)b * n.N + j] = h;
        }
    }
    return p;
}

// dh2, dh1 and (with dx) the gradient of the input's columns off .. off + dx_cols
void naive_backward(const Net &n, int B, const Pass &p, const V &dout, V &dh2, V &dh1, V *dx, int off, int dx_cols) {
    dh2.assign((size_t)B * n.H2, 0.f), dh1.assign((size_t)B * n.H1, 0.f);
    if (dx) dx->assign((size_t)B * dx_cols, 0.f);
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < n.H2; ++j) {
            float s = 0.f;
            if (n.N == 1) s = dout[b] * n.w3[j];   // dq_b w3[j]
            else for (int a = 0; a < n.N; ++a) s = std::fmaf(dout[(size_t)b * n.N + a], n.w3[(size_t)a * n.H2 + j], s);
            dh2[(size_t)b * n.H2 + j] = p.h2[(size_t)b * n.H2 + j] > 0.f ? s : 0.f;
        }
        for (int i = 0; i < n.H1; ++i) {
            float s = 0.f;
            for (int j = 0; j < n.H2; ++j) s = std::fmaf(dh2[(size_t)b * n.H2 + j], n.w2[(size_t)j * n.H1 + i], s);
            dh1[(size_t)b * n.H1 + i] = p.h1[(size_t)b * n.H1 + i] > 0.f ? s : 0.f;
        }
        if (dx)
            for (int c = 0; c < dx_cols; ++c) {
                float s = 0.f;
                for (int i = 0; i < n.H1; ++i) s = std::fmaf(dh1[(size_t)b * n.H1 + i], n.w1[(size_t)i * n.K + off + c], s);
                (*dx)[(size_t)b * dx_cols + c] = s;
            }
    }
}

void naive_wgrad(int B, int J, int I, const V &dOut, const V &In, V &dW, V &db) {
    const int S = SNG_LEARNER_SEGMENT;
    dW.assign((size_t)J * I, 0.f), db.assign(J, 0.f);
    for (int j = 0; j < J; ++j) {
        for (int i = 0; i < I; ++i) {
            float g = 0.f;
            for (int s0 = 0; s0 < B; s0 += S) {
                float part = 0.f;
                for (int b = s0; b < B && b < s0 + S; ++b) part = std::fmaf(dOut[(size_t)b * J + j], In[(size_t)b * I + i], part);
                g = s0 == 0 ? part : g + part;
            }
            dW[(size_t)j * I + i] = g;
        }
        float g = 0.f;
        for (int s0 = 0; s0 < B; s0 += S) {
            float part = 0.f;
            for (int b = s0; b < B && b < s0 + S; ++b) part = part + dOut[(size_t)b * J + j];
            g = s0 == 0 ? part : g + part;
        }
        db[j] = g;
    }
}

// a loss's sum: a chain per segment of S rows, the partials added in ascending order
float naive_segment_sum(const V &terms) {
    const int S = SNG_LEARNER_SEGMENT, B = (int)terms.size();
    float g = 0.f;
    for (int s0 = 0; s0 < B; s0 += S) {
        float part = 0.f;
        for (int b = s0; b < B && b < s0 + S; ++b) part = part + terms[b];
        g = s0 == 0 ? part : g + part;
    }
    return g;
}

void naive_adam_polyak(Net &w, Net &g, Net &m, Net &v, Net &target, double lr, const SngLearnerSpec &s, int64_t t) {
    const float b1 = (float)s.beta1, c1 = (float)(1.0 - s.beta1), b2 = (float)s.beta2, c2 = (float)(1.0 - s.beta2);
    const float step = (float)(lr / (1.0 - std::pow(s.beta1, (double)t)));
    const float bc2 = (float)std::sqrt(1.0 - std::pow(s.beta2, (double)t)), eps = (float)s.eps;
    const float tau = (float)s.tau, omt = (float)(1.0 - s.tau);
    for (int i = 0; i < 6; ++i)
        for (size_t e = 0; e < w.all(i)->size(); ++e) {
            const float grad = (*g.all(i))[e];
            float &mm = (*m.all(i))[e], &vv = (*v.all(i))[e], &p = (*w.all(i))[e], &tg = (*target.all(i))[e];
            const float m_a = b1 * mm, m_b = c1 * grad;
            mm = m_a + m_b;
            const float v_a = b2 * vv, v_b = c2 * grad, v_c = v_b * grad;
            vv = v_a + v_c;
            const float root = std::sqrt(vv), scaled = root / bc2, denom = scaled + eps, ratio = mm / denom;
            const float delta = step * ratio;
            p = p - delta;
            const float t_a = omt * tg, t_b = tau * p;
            tg = t_a + t_b;
        }
}

struct State {
    Net actor, critic, actor_t, critic_t, am, av, cm, cv;
    int64_t step = 0;
};
struct Trace {
    V q, dq, q_pi;
    Net gc, ga;
    float critic_loss = 0.f, actor_loss = 0.f;
};

void naive_update(State &st, const SngLearnerSpec &spec, int B, int O, int A, const V &obs, const V &act, const V &y,
                  const V &a_pi, Trace &tr) {
    const int K = O + A;
    const int64_t t = st.step + 1;
    V x((size_t)B * K);
    auto concat = [&](const V &a) {
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < K; ++k) x[(size_t)b * K + k] = k < O ? obs[(size_t)b * O + k] : a[(size_t)b * A + k - O];
    };
    V dh2, dh1, dq(B);
    // critic
    concat(act);
    Pass pc = naive_forward(st.critic, B, x);
    V terms(B);
    for (int b = 0; b < B; ++b) {
        const float d = pc.out[b] - y[b], dd = d * d;
        terms[b] = dd;
        const float two = 2.0f * d;
        dq[b] = two / (float)B;
    }
    tr.critic_loss = naive_segment_sum(terms) / (float)B;
    tr.q = pc.out, tr.dq = dq;
    naive_backward(st.critic, B, pc, dq, dh2, dh1, nullptr, 0, 0);
    tr.gc.zero_like(st.critic);
    naive_wgrad(B, 1, st.critic.H2, dq, pc.h2, tr.gc.w3, tr.gc.b3);
    naive_wgrad(B, st.critic.H2, st.critic.H1, dh2, pc.h1, tr.gc.w2, tr.gc.b2);
    naive_wgrad(B, st.critic.H1, K, dh1, x, tr.gc.w1, tr.gc.b1);
    naive_adam_polyak(st.critic, tr.gc, st.cm, st.cv, st.critic_t, spec.critic_lr, spec, t);
    // actor
    Pass pa = naive_forward(st.actor, B, obs);
    concat(a_pi);
    pc = naive_forward(st.critic, B, x);
    for (int b = 0; b < B; ++b) dq[b] = -(1.0f / (float)B);
    tr.actor_loss = -(naive_segment_sum(pc.out) / (float)B);
    tr.q_pi = pc.out;
    V dx;
    naive_backward(st.critic, B, pc, dq, dh2, dh1, &dx, O, A);
    for (size_t e = 0; e < dx.size(); ++e) {
        const float sq = a_pi[e] * a_pi[e], one_m = 1.0f - sq;
        dx[e] = dx[e] * one_m;
    }
    naive_backward(st.actor, B, pa, dx, dh2, dh1, nullptr, 0, 0);
    tr.ga.zero_like(st.actor);
    naive_wgrad(B, A, st.actor.H2, dx, pa.h2, tr.ga.w3, tr.ga.b3);
    naive_wgrad(B, st.actor.H2, st.actor.H1, dh2, pa.h1, tr.ga.w2, tr.ga.b2);
    naive_wgrad(B, st.actor.H1, O, dh1, obs, tr.ga.w1, tr.ga.b1);
    naive_adam_polyak(st.actor, tr.ga, st.am, st.av, st.actor_t, spec.actor_lr, spec, t);
    st.step = t;
}

std::atomic<long> g_compared{0};
std::atomic<int> g_failed{0};

bool same(const V &a, const V &b, const char *what, int h1, int h2, int B, int K) {
    g_compared += (long)a.size();
    if (a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0)) return true;
    size_t at = 0;
    while (at < a.size() && at < b.size() && std::memcmp(&a[at], &b[at], 4) == 0) ++at;
    std::printf("MISMATCH %s net (%d, %d) B %d K %d at %zu: host %.9g naive %.9g\n", what, h1, h2, B, K, at,
                at < a.size() ? a[at] : 0.f, at < b.size() ? b[at] : 0.f);
    ++g_failed;
    return false;
}

// One state through one update per entry of `batches`, in that order.
void run_case(int h1, int h2, const std::vector<int> &batches, int K) {
    const int A = K == 13 ? 2 : 51, O = K - A;
    Rng r{(uint64_t)(h1 * 1000003 + h2 * 1009 + batches[0] * 31 + K)};
    State host, naive;
    host.actor.init(O, h1, h2, A, r, 2.f), host.actor_t.init(O, h1, h2, A, r, 2.f);
    host.critic.init(K, h1, h2, 1, r, 10.f), host.critic_t.init(K, h1, h2, 1, r, 10.f);
    host.am.zero_like(host.actor), host.av.zero_like(host.actor), host.cm.zero_like(host.critic), host.cv.zero_like(host.critic);
    naive = host;
    const SngLearnerSpec spec{1e-3, 2e-3, 0.005, 0.9, 0.999, 1e-8};
    V lo(A, -1.f), hi(A, 1.f);
    const SngMlpNetSpec aspec{O, A, h1, h2, POLICY_RELU, SNG_MLP_OUT_SQUASH, lo.data(), hi.data()};
    const SngCriticSpec cspec{h1, h2, POLICY_RELU};
    for (int update = 0; update < (int)batches.size(); ++update) {
        const int B = batches[update];
        V obs((size_t)B * O), act((size_t)B * A), y(B), a_pi((size_t)B * A);
        for (float &v : obs) v = r.uniform(0.f, 1.f);
        for (float &v : act) v = r.uniform(-1.f, 1.f);
        for (float &v : y) v = r.uniform(-30.f, 5.f);
        for (float &v : a_pi) v = std::tanh(r.uniform(-2.f, 2.f));
        Trace th, tn;
        th.q.resize(B), th.dq.resize(B), th.q_pi.resize(B);
        th.gc.zero_like(host.critic), th.ga.zero_like(host.actor);
        SngLearnerState st{host.actor.arrays(), host.critic.arrays(), host.actor_t.arrays(), host.critic_t.arrays(),
                           host.am.arrays(),    host.av.arrays(),     host.cm.arrays(),      host.cv.arrays(), host.step};
        const SngLearnerTrace trace{th.q.data(), th.dq.data(), th.q_pi.data(), th.gc.arrays(), th.ga.arrays(),
                                    &th.critic_loss, &th.actor_loss};
        learner_update_host(aspec, cspec, spec, &st, B, obs.data(), act.data(), y.data(), a_pi.data(), &trace);
        host.step = st.step;
        naive_update(naive, spec, B, O, A, obs, act, y, a_pi, tn);
        bool ok = host.step == naive.step && host.step == update + 1;
        ok &= same(th.q, tn.q, "q", h1, h2, B, K) & same(th.dq, tn.dq, "dq", h1, h2, B, K) &
              same(th.q_pi, tn.q_pi, "q_pi", h1, h2, B, K);
        ok &= same(V{th.critic_loss, th.actor_loss}, V{tn.critic_loss, tn.actor_loss}, "losses", h1, h2, B, K);
        Net *pairs[10][2] = {{&th.gc, &tn.gc},           {&th.ga, &tn.ga},           {&host.actor, &naive.actor},
                             {&host.critic, &naive.critic}, {&host.actor_t, &naive.actor_t}, {&host.critic_t, &naive.critic_t},
                             {&host.am, &naive.am},      {&host.av, &naive.av},      {&host.cm, &naive.cm},
                             {&host.cv, &naive.cv}};
        const char *names[10] = {"critic grad", "actor grad", "actor", "critic", "actor target", "critic target",
                                 "actor m",     "actor v",    "critic m", "critic v"};
        for (int p = 0; p < 10; ++p)
            for (int i = 0; i < 6; ++i) ok &= same(*pairs[p][0]->all(i), *pairs[p][1]->all(i), names[p], h1, h2, B, K);
        // not a comparison of zeros
        size_t nz = 0;
        for (float v : tn.gc.w2) nz += v != 0.f;
        for (float v : tn.ga.w2) nz += v != 0.f;
        if (B >= 63 && 4 * nz < tn.gc.w2.size() + tn.ga.w2.size()) {
            std::printf("DEGENERATE net (%d, %d) B %d K %d: %zu non-zero hidden gradients\n", h1, h2, B, K, nz);
            ++g_failed;
        }
        if (!ok) return;
    }
}

}  // namespace

int main() {
    // the packed image's index law, written for both sides, is sng_policy_net_host.h's
    for (int KP : {8, 16, 112, 400, 512})
        for (int j = 0; j < 70; ++j)
            for (int k = 0; k < KP; ++k)
                if (learn_image_at(KP, j, k) != net_weight_at(KP, j, k)) {
                    std::printf("learn_image_at(%d, %d, %d) differs from net_weight_at\n", KP, j, k);
                    return 1;
                }
    const int S = SNG_LEARNER_SEGMENT;
    struct Case {
        int h1, h2;
        std::vector<int> batches;
        int K;
    };
    std::vector<Case> cases;
    const int nets[3][2] = {{400, 300}, {33, 65}, {8, 8}};
    for (auto &n : nets)
        for (int B : {2 * S + 37, S + 1, S, 65, 64, 63, 1})
            for (int K : {160, 13})   // the widest net's chains once: they are the time
                cases.push_back({n[0], n[1], n[0] == 400 ? std::vector<int>{B} : std::vector<int>{B, B}, K});
    // one state through batches in descending and mixed order (the segments of an update are its own, whatever the
    // update before it had), and the most segments there are: 64 whole ones, and 63 with one of S - 1 rows
    cases.push_back({33, 65, {2 * S + 37, 200, 1, 64, 33, S + 1, 7}, 13});
    cases.push_back({8, 8, {2 * S + 37, 200, 1}, 13});
    cases.push_back({8, 8, {SNG_LEARNER_MAX_ROWS - 1}, 13});
    cases.push_back({8, 8, {SNG_LEARNER_MAX_ROWS, 64}, 13});
    std::atomic<size_t> next{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < nt; ++i)
        pool.emplace_back([&] {
            for (size_t c; (c = next++) < cases.size();) run_case(cases[c].h1, cases[c].h2, cases[c].batches, cases[c].K);
        });
    for (auto &t : pool) t.join();
    if (g_failed) return 1;
    std::printf("ddpg learn host ok %zu cases %ld values\n", cases.size(), g_compared.load());
    return 0;
}
