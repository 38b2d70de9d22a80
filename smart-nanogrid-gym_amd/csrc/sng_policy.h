// sng_policy.h -- the MLP actor on the device: mlp_actor_tile, a workgroup's 64 observation rows in LDS to its
// 64 action rows in LDS, and policy_kernel, which stages the rows of a block of envs around it.  Included by
// sng_kernels.hip only, behind sng_dev_util.h.
//
// The arithmetic is the contract of sng_policy_host.h: every output is the k-ordered f32 fmaf chain started from
// the bias.  A lane works on one env's row and keeps 16 of a layer's chains in VGPRs (four wavefronts share a row
// block and split the outputs); k is the outer loop, so every chain takes its terms in order, and one k's weights
// are a wave-uniform run of the image ([in][out]) that the scalar unit loads: each FMA takes its weight as an SGPR
// operand, one rounding per term, as std::fmaf does on the host.  The f32 MFMAs keep the same chain at the same rate (one rounding per product, no wider
// accumulation); they would free the VALU, which matters only next to an env step in the same kernel.
#pragma once

#include "sng_policy_host.h"

namespace sng {

constexpr int kPolicyHStride = kPolicyHidden + 1;   // a lane's hidden row in LDS: odd, so the lanes' rows differ in bank

// The LDS of one workgroup of policy_kernel, in floats: the observation tile [64][O], the hidden rows
// [64][kPolicyHStride], and the two action tiles [64][A] (a, which holds the noise on entry, and the clipped actions).
__host__ __device__ inline int policy_lds_obs(int O) { return round4(kWave * O); }
__host__ __device__ inline int policy_lds_hidden() { return round4(kWave * kPolicyHStride); }
__host__ __device__ inline int policy_lds_act(int A) { return round4(kWave * A); }
inline size_t policy_lds_bytes(int O, int A) {
    return (size_t)(policy_lds_obs(O) + policy_lds_hidden() + 2 * policy_lds_act(A)) * sizeof(float);
}

// The wavefronts of a policy workgroup: they share the workgroup's 64 rows and split every layer's outputs, so a
// SIMD holds several wavefronts whose scalar weight loads overlap (one wavefront per 64 rows left every load's
// latency exposed: 35.9 us a launch at 65,536 x N = 8, profiles/policy_day_ab.txt).
constexpr int kPolicyWaves = 4;
constexpr int kPolicyBlock = kPolicyWaves * kWave;

template <bool TANH>
__device__ __forceinline__ float policy_activation(float h) {
    if constexpr (TANH) return tanhf(h);
    else return h > 0.f ? h : 0.f;
}

// Outputs [j0, j0 + NJ) of one layer: the chains of the lane's row over the K inputs in[0], in[is], .. (is: the
// floats between two inputs of a row), weights w [K][ldw] and biases b of the image, into acc.
template <int NJ, int IS = 1>
__device__ __forceinline__ void policy_chains(float (&acc)[NJ], const float *__restrict__ in, int K,
                                              const float *__restrict__ w, int ldw, const float *__restrict__ b, int j0) {
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) acc[jj] = b[j0 + jj];
    for (int k = 0; k < K; ++k) {
        const float xk = in[k * IS];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) acc[jj] = __builtin_fmaf(xk, w[(size_t)k * ldw + j0 + jj], acc[jj]);
    }
}

// The output stage of a lane's row: outputs [c0, c0 + NJ) of the output layer (acc) to s_a [64][A] (a = mean, + the
// noise s_a holds on entry when `noise`) and s_env [64][A] (a clipped to the image's bounds lo, hi where it has them);
// the padded outputs past A are dropped.
template <int NJ>
__device__ __forceinline__ void policy_output_store(const PolicyImage &m, const float (&acc)[NJ], int c0,
                                                    float *__restrict__ s_a, float *__restrict__ s_env, bool noise,
                                                    int lane, const float *lo, const float *hi) {
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = c0 + jj;
        if (j < m.A) {
            const int at = lane * m.A + j;
            const float a = noise ? acc[jj] + s_a[at] : acc[jj];
            s_a[at] = a;
            float c = a;
            if (m.clip) {
                c = a < lo[j] ? lo[j] : a;
                c = hi[j] < c ? hi[j] : c;
            }
            s_env[at] = c;
        }
    }
}

// policy_kernel's form of the tile.  One workgroup of kPolicyWaves wavefronts: s_obs [64][O] -> s_a [64][A] (a = mean, + the noise s_a holds on entry
// when `noise`) and s_env [64][A] (what the env is stepped with: a clipped to the image's bounds where it has them).
// s_h: the rows' hidden values, [64][kPolicyHStride].  Lane l of every wavefront works on row l; wavefront `wave`
// (wave-uniform) computes outputs [16 wave, 16 wave + 16) of the hidden layers and every kPolicyWaves-th chunk of
// the output layer, each chain in one lane, k-ordered.  Every lane computes, whether an env is behind its row or
// not: the tiles have 64 rows, and the caller zeroes the rows without an env.  The caller has a barrier between its tile copies and this, and one after it.
template <bool TANH>
__device__ __forceinline__ void mlp_actor_block(const float *__restrict__ img, const PolicyImage &m,
                                                const float *__restrict__ s_obs, float *__restrict__ s_h,
                                                float *__restrict__ s_a, float *__restrict__ s_env, bool noise,
                                                int wave, int lane) {
    constexpr int H = kPolicyHidden, NJ = H / kPolicyWaves;
    static_assert(NJ == kPolicyOutChunk, "one chunk of outputs per wavefront and pass");
    float acc[NJ];
    float *hrow = s_h + lane * kPolicyHStride;
    const int j0 = wave * NJ;
    // hidden layer 1: K = O
    policy_chains<NJ>(acc, s_obs + lane * m.O, m.O, img + m.w1t, H, img + m.b1, j0);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) hrow[j0 + jj] = policy_activation<TANH>(acc[jj]);
    __syncthreads();
    // hidden layer 2: K = 64, from the row all wavefronts wrote; its outputs replace the row once all have read it
    policy_chains<NJ>(acc, hrow, H, img + m.w2t, H, img + m.b2, j0);
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) hrow[j0 + jj] = policy_activation<TANH>(acc[jj]);
    __syncthreads();
    // the output layer, a chunk of kPolicyOutChunk outputs at a time (the image pads A to it with zero weights)
    const float *lo = img + m.low, *hi = img + m.high;
    for (int c0 = wave * NJ; c0 < m.AP; c0 += kPolicyWaves * NJ) {
        policy_chains<NJ>(acc, hrow, H, img + m.w3t, m.AP, img + m.b3, c0);
        policy_output_store<NJ>(m, acc, c0, s_a, s_env, noise, lane, lo, hi);
    }
}

// The actor over E rows: 64 rows per workgroup, staged through LDS as the step kernels stage theirs.  obs [E][O],
// noise [E][A] or null, actions [E][A] (a), env_actions [E][A] or null.
template <bool TANH>
__global__ __launch_bounds__(kPolicyBlock) void policy_kernel(const float *__restrict__ img, PolicyImage m,
                                                              const float *__restrict__ obs,
                                                              const float *__restrict__ noise,
                                                              float *__restrict__ actions,
                                                              float *__restrict__ env_actions, int64_t E, int vec_io) {
    extern __shared__ float4 policy_lds4[];
    float *s_obs = reinterpret_cast<float *>(policy_lds4);
    float *s_h = s_obs + policy_lds_obs(m.O);
    float *s_a = s_h + policy_lds_hidden();
    float *s_env = s_a + policy_lds_act(m.A);
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t e0 = (int64_t)blockIdx.x * kWave;
    const int rows = E - e0 < kWave ? (int)(E - e0) : kWave;
    const bool vec = vec_io != 0;
    copy_in<2, kPolicyBlock>(s_obs, obs + (size_t)e0 * m.O, rows * m.O, vec, tid);
    if (noise) copy_in<1, kPolicyBlock>(s_a, noise + (size_t)e0 * m.A, rows * m.A, vec, tid);
    // the rows past the last env (the last workgroup's) hold zeros: every lane computes, on defined inputs
    for (int i = rows * m.O + tid; i < kWave * m.O; i += kPolicyBlock) s_obs[i] = 0.f;
    for (int i = rows * m.A + tid; i < kWave * m.A; i += kPolicyBlock) s_a[i] = 0.f;
    __syncthreads();
    mlp_actor_block<TANH>(img, m, s_obs, s_h, s_a, s_env, noise != nullptr, wave, lane);
    __syncthreads();
    copy_out<kPolicyBlock>(actions + (size_t)e0 * m.A, s_a, rows * m.A, vec, tid);
    if (env_actions) copy_out<kPolicyBlock>(env_actions + (size_t)e0 * m.A, s_env, rows * m.A, vec, tid);
}

// ---------------------------------------------------------------------------------------------------------------
// The wavefront-wide tile and the fused day: day_lean_kernel (sng_step_day.h) with the actor between the steps.
// ---------------------------------------------------------------------------------------------------------------
// One wavefront on its own, no barrier: s_obs [64][O] -> s_a [64][A] (a = mean, + the noise s_a holds on entry when
// `noise`) and s_env [64][A] (a clipped to the image's bounds where it has them).  A lane owns row `lane` and keeps a
// hidden layer's 64 chains in 64 VGPRs; the hidden values pass through s_hT [64][64], transposed (value j of lane l
// at j * 64 + l: the lanes of a wavefront read and write consecutive words).  A lane reads back only what it wrote,
// so nothing is fenced inside; the caller fences between its tile copies and this.  The activation is a wave-uniform
// branch on the image's (the fused day is compiled once per plan, not once per activation).
__device__ __forceinline__ void policy_hidden_store(float *__restrict__ hcol, const float (&acc)[kPolicyHidden], bool tanh_) {
    constexpr int H = kPolicyHidden;
    if (tanh_) {   // tanhf stays out of the unrolled chains: one rolled loop per layer
#pragma unroll
        for (int j = 0; j < H; ++j) hcol[j * kWave] = acc[j];
#pragma unroll 2
        for (int j = 0; j < H; ++j) hcol[j * kWave] = tanhf(hcol[j * kWave]);
    } else {
#pragma unroll
        for (int j = 0; j < H; ++j) hcol[j * kWave] = acc[j] > 0.f ? acc[j] : 0.f;
    }
}
__device__ __forceinline__ void mlp_actor_tile(const float *__restrict__ img, const PolicyImage &m,
                                               const float *__restrict__ s_obs, float *__restrict__ s_hT,
                                               float *__restrict__ s_a, float *__restrict__ s_env, bool noise,
                                               int lane) {
    constexpr int H = kPolicyHidden, NJ = kPolicyOutChunk;
    const bool tanh_ = m.activation == POLICY_TANH;
    float *hcol = s_hT + lane;
    {
        float acc[H];
        policy_chains<H>(acc, s_obs + lane * m.O, m.O, img + m.w1t, H, img + m.b1, 0);
        policy_hidden_store(hcol, acc, tanh_);
        policy_chains<H, kWave>(acc, hcol, H, img + m.w2t, H, img + m.b2, 0);
        policy_hidden_store(hcol, acc, tanh_);
    }
    const float *lo = img + m.low, *hi = img + m.high;
    for (int c0 = 0; c0 < m.AP; c0 += NJ) {
        float o[NJ];
        policy_chains<NJ, kWave>(o, hcol, H, img + m.w3t, m.AP, img + m.b3, c0);
        policy_output_store<NJ>(m, o, c0, s_a, s_env, noise, lane, lo, hi);
    }
}

// The fused day's LDS: LeanLds<NC>'s tiles (the actions tile holds the clipped actions the step reads), then the
// tile of a (the noise on entry) and the hidden values.
template <int NC>
struct PolicyDayLds {
    static constexpr int HID = kWave * kPolicyHidden;
    static constexpr size_t BYTES = LeanLds<NC>::WAVE_BYTES + (size_t)(LeanLds<NC>::ACT + HID) * 4;
};

// day_lean_kernel with the actor between the steps: per step mlp_actor_tile(s_obs -> s_act) and then the unchanged
// LeanGroup::run<true>, one independent wavefront per workgroup as there.  The weights are re-read every step
// through the scalar cache (the image is shared by every wavefront of the device).
//   obs0         the day's t = 0 observation block [E][O] (the reset or the caller wrote it), copied into s_obs
//                before the first step
//   stream       takes the place of the actions stream and keeps its one-step prefetch ahead of the stores: the
//                noise blocks, stream_step floats apart, added to the mean in the tile when has_noise.  Without
//                noise LeanGroup's prefetch still issues its tile load (LeanGroup is not edited): the caller passes
//                a valid [E][A] block and stream_step = 0, and the tile is never committed
//   actions_out  a, act_step floats from one step's block to the next (0: every step overwrites one block), next to
//                obs_step / out_step
template <int NC, bool PK, bool REQ>
__global__ __launch_bounds__(kLeanBlock) __attribute__((amdgpu_waves_per_eu(kDayLeanWaves))) void
day_lean_policy_kernel(const float *__restrict__ img, PolicyImage m, const float *__restrict__ stream,
                       int64_t stream_step, int has_noise, const float *obs0, float *obs,
                       float *__restrict__ actions_out, double *__restrict__ reward, uint8_t *__restrict__ done,
                       int64_t E, int t0, int nt, int vec_io, int vec_act, int64_t obs_step, int64_t out_step,
                       int64_t act_step, Params p, DeviceState s, InfoPtrs info) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const LeanTiles<NC> tl(lds, 0);
    float *s_a = lds + LeanLds<NC>::WAVE_BYTES / 4;
    float *s_hT = s_a + LeanLds<NC>::ACT;
    LeanGroup<NC, PK, REQ> g;
    g.template issue<true, false>((int64_t)blockIdx.x * kLeanBlock, stream, E, t0, vec_io, p, s, info, lane);
    g.issue_step_inputs(stream, E, t0, vec_io, p, s, lane);
    copy_in<4, kWave>(tl.s_obs, obs0 + g.ew * p.obs_dim, (g.nw > 0 ? g.nw : 1) * p.obs_dim, vec_io != 0, lane);
    // the rows of idle lanes hold zeros: every lane computes the actor, on defined inputs
    for (int i = (g.nw > 0 ? g.nw : 1) * p.obs_dim + lane; i < kWave * p.obs_dim; i += kWave) tl.s_obs[i] = 0.f;
    for (int i = lane; i < kWave * p.act_dim; i += kWave) s_a[i] = 0.f;
    const int t1 = t0 + nt;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        g.take_step_inputs(p);
        if (has_noise) g.act_tile.commit(s_a, lane);
        wave_lds_fence();
        const StepConst k = g.kn;
        mlp_actor_tile(img, m, tl.s_obs, s_hT, s_a, tl.s_act, has_noise != 0, lane);
        wave_lds_fence();
        if (t + 1 < t1)   // ahead of this step's stores
            g.issue_step_inputs(stream + (size_t)(t + 1 - t0) * (size_t)stream_step, E, t + 1, vec_io, p, s, lane);
        if (g.nw > 0) copy_out<kWave>(actions_out + g.e0 * p.act_dim, s_a, g.nw * p.act_dim, vec_act != 0, lane);
        g.template run<true>(tl.s_act, tl.s_obs, tl.s_pos, tl.s_neg, obs, reward, done, E, t, vec_io, k, p, s, info, lane);
        wave_lds_fence();   // the next step's tile writes stay behind this step's reads of the tiles
        obs += obs_step;
        reward += out_step;
        done += out_step;
        actions_out += act_step;
    }
    g.store_state(E, p, s, info);
    bump_day_counter<PK>(p, s, t0);
}

}  // namespace sng
