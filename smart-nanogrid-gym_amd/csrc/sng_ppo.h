// sng_ppo.h -- rollout_gae_kernel: what a PPO update reads beside the trajectory a policy graph left -- the critic's
// values, the advantages and returns, and the log-probabilities -- in one launch.  Included by sng_kernels.hip only,
// behind sng_policy.h (policy_chains, policy_activation and the hidden rows' stride are its).  gae_advantage / gae_step
// and logp_term, the recurrence's step and the log-probability's term, are defined here for gae_scan_kernel
// (sng_ppo_net.h) too.
//
// The arithmetic is the contract of sng_ppo_host.h.  One workgroup of kPolicyWaves wavefronts owns 64 envs of one
// day and walks the day backwards, t = T .. 0: the value net over the step's observation tile as policy_kernel runs
// the actor's hidden layers (lane l of every wavefront on row l, a wavefront on 16 of a layer's 64 chains, weights
// as scalar operands), then the output layer's single chain on wavefront 0, whose lanes keep V[t + 1] and the running
// gae of their env in registers from step to step and store the step's value, advantage and return as 256-byte rows.
// Wavefront 1 meanwhile sums the step's log-probability terms from the noise tile.  Every f32 operation of the
// recurrence and of the log-probability is rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn).
//
// A step's inputs are requested a step ahead: the tile of obs[t - 1] goes into registers (RowsStage) before step t's
// layers run and into the second LDS tile after them, step t's noise tile likewise around hidden layer 1, and
// wavefront 0 asks for reward / done of step t - 1 as soon as it has used step t's.  Tiles above a stage's registers
// (an obs_dim above 128, an act_dim above 32) or not 16 B aligned are copied at the commit point instead, and where
// two observation tiles do not fit a compute unit's LDS (ppo_lds_bytes) the one tile is refilled behind hidden
// layer 1's barrier.
#pragma once

#include "sng_ppo_host.h"

namespace sng {

constexpr int kPpoObsStage = 8;     // float4 per thread of the observation prefetch: tiles of up to 8,192 floats
constexpr int kPpoNoiseStage = 2;   // ... of the noise prefetch: up to 2,048 floats
constexpr int kPpoMaxLds = 160 * 1024;

// The LDS of one workgroup, in floats: one or two observation tiles [64][O], the hidden rows [64][kPolicyHStride]
// and, with the log-probability stage, the noise tile [64][A].
inline size_t ppo_lds_bytes(int O, int A, bool two_tiles, bool noise) {
    return (size_t)((two_tiles ? 2 : 1) * policy_lds_obs(O) + policy_lds_hidden() + (noise ? policy_lds_act(A) : 0)) *
           sizeof(float);
}

// A tile requested ahead of its use: issue() puts an aligned tile of up to K float4 per thread into registers, commit()
// writes it to LDS; any other tile (unaligned, or larger) is copied at commit().  TileStage's split (sng_dev_util.h)
// without its staged one-float form and with a small copy behind it, which keeps the registers of the fallback down.
template <int K, int BLOCK>
struct RowsStage {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v[K];
    const float *src;
    int count;
    bool vec, staged;
    __device__ __forceinline__ void issue(const float *__restrict__ s, int cnt, bool vec_io, int tid) {
        src = s;
        count = cnt;
        vec = vec_io && (cnt & 3) == 0;
        staged = vec && (cnt >> 2) <= K * BLOCK;
        if (!staged) return;
        const v4f *s4 = reinterpret_cast<const v4f *>(s);
        const int n4 = cnt >> 2;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = k * BLOCK + tid;
            v[k] = s4[i < n4 ? i : n4 - 1];
        }
    }
    __device__ __forceinline__ void commit(float *__restrict__ dst, int tid) {
        if (!staged) {
            copy_in<2, BLOCK>(dst, src, count, vec, tid);
            return;
        }
        v4f *d4 = reinterpret_cast<v4f *>(dst);
        const int n4 = count >> 2;
#pragma unroll
        for (int k = 0; k < K; ++k) {   // out-of-range threads rewrite the last element (same value)
            const int i = k * BLOCK + tid;
            d4[i < n4 ? i : n4 - 1] = v[k];
        }
    }
};

// One step of the recurrence (sng_ppo_host.h, ppo_gae_step): `gae` in, the step's advantage out (the new gae).
__device__ __forceinline__ float gae_advantage(float g, float gl, float r, float nn, float v, float v_next, float gae) {
    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(g, v_next), nn)), v);
    return __fadd_rn(delta, __fmul_rn(__fmul_rn(gl, nn), gae));
}
// ... and the step's return with it: ret = advantage + v.
__device__ __forceinline__ float gae_step(float g, float gl, float r, float nn, float v, float v_next, float gae,
                                          float &ret) {
    const float a = gae_advantage(g, gl, r, nn, v, v_next, gae);
    ret = __fadd_rn(a, v);
    return a;
}

// One term of a row's log-probability (sng_ppo_host.h, ppo_logp_row)
__device__ __forceinline__ float logp_term(float noise, float inv_std, float log_std) {
    const float z = __fmul_rn(noise, inv_std);
    return __fsub_rn(__fsub_rn(__fmul_rn(__fmul_rn(-0.5f, z), z), log_std), kHalfLog2Pi);
}

// obs [days][T + 1][E][O], reward / done [days][T][E], noise [T][E][A] or null (no log-probability stage), values
// [days][T + 1][E], advantages / returns / logp [days][T][E].  g, gl: gamma and gamma * lambda (ppo_gamma_f32,
// ppo_gamma_lambda_f32).  Grid (ceil(E / 64), days).
template <bool TANH>
__global__ __launch_bounds__(kPolicyBlock) void rollout_gae_kernel(const float *__restrict__ img, PpoImage m,
                                                                   const float *__restrict__ obs,
                                                                   const double *__restrict__ reward,
                                                                   const uint8_t *__restrict__ done,
                                                                   const float *__restrict__ noise,
                                                                   float *__restrict__ values,
                                                                   float *__restrict__ advantages,
                                                                   float *__restrict__ returns, float *__restrict__ logp,
                                                                   int64_t E, int T, float g, float gl, int two_tiles,
                                                                   int vec_obs, int vec_noise) {
    extern __shared__ float4 ppo_lds4[];
    constexpr int H = kPolicyHidden, NJ = H / kPolicyWaves;
    const int O = m.v.O, A = m.head.A;
    float *s_obs = reinterpret_cast<float *>(ppo_lds4);
    float *s_h = s_obs + (two_tiles ? 2 : 1) * policy_lds_obs(O);
    float *s_nz = s_h + policy_lds_hidden();
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t e0 = (int64_t)blockIdx.x * kWave;
    const int rows = E - e0 < kWave ? (int)(E - e0) : kWave;
    const size_t d = blockIdx.y;
    const bool live = lane < rows;
    const size_t tile = (size_t)E * (size_t)O;   // floats from one step's observation block to the next
    const float *obs_d = obs + d * (size_t)(T + 1) * tile + (size_t)e0 * (size_t)O;
    const size_t out_d = d * (size_t)T * (size_t)E + (size_t)e0 + (size_t)lane;        // of step 0, this lane's env
    const size_t val_d = d * (size_t)(T + 1) * (size_t)E + (size_t)e0 + (size_t)lane;

    // the rows past the last env (the last workgroup's) hold zeros in every tile: every lane computes, on defined inputs
    for (int i = rows * O + tid; i < kWave * O; i += kPolicyBlock) {
        s_obs[i] = 0.f;
        if (two_tiles) s_obs[policy_lds_obs(O) + i] = 0.f;
    }
    if (noise)
        for (int i = rows * A + tid; i < kWave * A; i += kPolicyBlock) s_nz[i] = 0.f;
    copy_in<2, kPolicyBlock>(s_obs, obs_d + (size_t)T * tile, rows * O, vec_obs != 0, tid);
    // wavefront 0, lane = env: the step's reward and done, V[t + 1] and the running gae
    double rw = 0.0;
    uint8_t dn = 0;
    if (wave == 0 && live) {
        rw = reward[out_d + (size_t)(T - 1) * (size_t)E];
        dn = done[out_d + (size_t)(T - 1) * (size_t)E];
    }
    float v_next = 0.f, gae = 0.f;
    __syncthreads();

    RowsStage<kPpoObsStage, kPolicyBlock> next_obs;
    RowsStage<kPpoNoiseStage, kPolicyBlock> step_noise;
    float *hrow = s_h + lane * kPolicyHStride;
    const int j0 = wave * NJ;
    int cur = 0;
#pragma unroll 1
    for (int t = T; t >= 0; --t) {
        const float *s_x = s_obs + cur * policy_lds_obs(O);
        float *s_nx = s_obs + (two_tiles ? (cur ^ 1) * policy_lds_obs(O) : 0);
        const bool lp_step = noise != nullptr && t < T;
        // The image is read anew every step, through the scalar cache: behind an offset it cannot see through the
        // compiler keeps none of it across the steps (it kept the biases and a run of weights, and spilled them to VGPR
        // lanes).  The offset, not the pointer: a pointer out of an asm statement is no kernel argument any more, and
        // its loads were per-lane flat loads, not scalar loads.
        int step_off = 0;
        asm volatile("" : "+s"(step_off));
        const float *wimg = img + step_off;
        const float *w1 = wimg + m.v.w1t, *w2 = wimg + m.v.w2t, *w3 = wimg + m.v.w3t;
        if (two_tiles && t > 0) next_obs.issue(obs_d + (size_t)(t - 1) * tile, rows * O, vec_obs != 0, tid);
        if (lp_step) step_noise.issue(noise + ((size_t)t * (size_t)E + (size_t)e0) * (size_t)A, rows * A, vec_noise != 0, tid);
        float acc[NJ];
        // hidden layer 1: K = O
        policy_chains<NJ>(acc, s_x + lane * O, O, w1, H, wimg + m.v.b1, j0);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) hrow[j0 + jj] = policy_activation<TANH>(acc[jj]);
        __syncthreads();
        // the one tile is free once every wavefront has read it; the noise tile since the step before's last barrier
        if (!two_tiles && t > 0) copy_in<2, kPolicyBlock>(s_nx, obs_d + (size_t)(t - 1) * tile, rows * O, vec_obs != 0, tid);
        if (lp_step) step_noise.commit(s_nz, tid);
        // hidden layer 2: K = 64, from the row all wavefronts wrote; its outputs replace the row once all have read it
        policy_chains<NJ>(acc, hrow, H, w2, H, wimg + m.v.b2, j0);
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) hrow[j0 + jj] = policy_activation<TANH>(acc[jj]);
        __syncthreads();
        if (wave == 0) {
            // the output layer's one chain, then the step of the recurrence
            float v1[1];
            policy_chains<1>(v1, hrow, H, w3, m.v.AP, wimg + m.v.b3, 0);
            const float v = v1[0];
            if (live) SNG_ST(values[val_d + (size_t)t * (size_t)E], v);
            if (t < T) {
                const float r = (float)rw, nn = __fsub_rn(1.0f, (float)dn);
                gae = gae_advantage(g, gl, r, nn, v, v_next, gae);
                if (live) {
                    const size_t at = out_d + (size_t)t * (size_t)E;
                    SNG_ST(advantages[at], gae);
                    SNG_ST(returns[at], __fadd_rn(gae, v));
                    if (t > 0) {   // the step before's, behind a step of layers
                        rw = reward[at - (size_t)E];
                        dn = done[at - (size_t)E];
                    }
                }
            }
            v_next = v;
        } else if (wave == 1 && lp_step && logp != nullptr) {
            const float *nz = s_nz + lane * A, *ls = wimg + m.head.log_std, *is = wimg + m.head.inv_std;
            float lp = 0.0f;
            for (int j = 0; j < A; ++j) lp = __fadd_rn(lp, logp_term(nz[j], is[j], ls[j]));
            if (live) SNG_ST(logp[out_d + (size_t)t * (size_t)E], lp);
        }
        if (two_tiles && t > 0) next_obs.commit(s_nx, tid);
        __syncthreads();   // the next step's writes of the hidden rows and the tiles stay behind this step's reads
        if (two_tiles) cur ^= 1;
    }
}

}  // namespace sng
