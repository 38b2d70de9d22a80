// sng_policy_net.h -- the MLP actor of any width on the f32-input MFMA: policy_net_kernel, the device side of
// sng_policy_create_net, and net_trunk, everything of it up to the output stage, which value_net_kernel
// (sng_ppo_net.h) runs a value net through as well.  Included by sng_kernels.hip only, behind sng_policy.h.
//
// The arithmetic is the contract of sng_policy_net_host.h: every output is the k-ordered f32 fmaf chain started from
// the bias.  v_mfma_f32_32x32x2_f32 computes D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) for 32 rows x 32 outputs, one
// rounding per product and no wider accumulation, so a tile's accumulators started from the bias and taken through
// the layer's k's two at a time, in order, ARE the 1,024 chains.  What the kernel adds to a chain is only trailing
// zero terms (K rounded up to a weight group, zero inputs times zero weights), which can turn a -0 into +0 and
// nothing else; the padded outputs it computes (zero weights, zero bias: act(0) = 0) enter the next layer as such
// trailing terms and are never stored.
//
// A workgroup of four wavefronts takes 64 rows, two 32-row tiles.  Wavefront w works on row tile w & 1 and on the
// output tiles of slot w >> 1, one 16-register accumulator at a time (the MFMA's dependent latency equals its issue
// interval).  Its operands:
//   A  the layer's input from LDS, lane l reading in[row l & 31][k + (l >> 5)]: rows with an odd stride, so the 32
//      rows of a half-wavefront differ in bank;
//   B  the weights from the image (sng_policy_net_host.h, NetImage): one 16-byte load per lane and group of 8 k's,
//      1 KB in a row per wavefront, prefetched kNetPrefetch groups ahead; the two wavefronts of a slot read the same
//      groups.
// D comes back as out[row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][col l & 31]; it is activated and written to the next
// layer's LDS rows (an accumulator cannot be the next layer's operand as it stands: its k order inside an MFMA would
// be permuted).  hidden1's rows stay in LDS whole; hidden2 is produced in chunks of 64 outputs, and the output
// layer's chains advance over each chunk as it is finished, in k order, so hidden2 needs one chunk of LDS (the chunk
// takes the place of the observation rows, which are dead by then).  The output tile's accumulators go straight to
// global memory with the output stage applied.
#pragma once

#include "sng_policy_net_host.h"

namespace sng {

constexpr int kNetWaves = 4;
constexpr int kNetBlock = kNetWaves * kWave;
constexpr int kNetPrefetch = 6;   // weight groups in flight per wavefront: 6 x 256 cycles of MFMA cover an L2 hit

typedef float net_f32x16 __attribute__((ext_vector_type(16)));
typedef float net_f32x4 __attribute__((ext_vector_type(4)));

// One tile's chains over `ng` weight groups (8 k's each).  a: the lane's first A operand (its row of the input, at
// k = lane >> 5); w: the lane's 16 bytes of the tile's first group, the groups 64 float4 apart.
__device__ __forceinline__ void net_tile_chain(net_f32x16 &acc, const float *__restrict__ a,
                                               const net_f32x4 *__restrict__ w, int ng) {
    net_f32x4 b[kNetPrefetch];
#pragma unroll
    for (int i = 0; i < kNetPrefetch; ++i) b[i] = w[(size_t)(i < ng ? i : ng - 1) * 64];
    // a group's four A operands
    auto a_load = [&](float (&v)[4], int g) {
        const float *ag = a + g * kNetKGroup;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ag[2 * i];
    };
    auto group = [&](const net_f32x4 bg, const float (&v)[4]) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[0], bg.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[1], bg.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[2], bg.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[3], bg.w, acc, 0, 0, 0);
    };
    // Whole rounds of the ring, without a branch inside.  The order of a group is pinned (sched_barrier): the next
    // group's LDS reads, this group's MFMAs, then the load that refills the group's ring slot -- behind the MFMAs
    // that read the slot, so it lands in the same registers and nothing waits for it before its turn comes (left to
    // itself the scheduler moved a round's six loads to the round's end and waited for all of them there).  The loads
    // and reads past the last group re-read it and are dropped.
    float a_now[4], a_next[4];
    a_load(a_now, 0);
    int g = 0;
    for (; g + kNetPrefetch <= ng; g += kNetPrefetch) {
#pragma unroll
        for (int i = 0; i < kNetPrefetch; ++i) {
            const int next = g + i + 1, ahead = g + i + kNetPrefetch;
            a_load(a_next, next < ng ? next : ng - 1);
            __builtin_amdgcn_sched_barrier(0);
            group(b[i], a_now);
            __builtin_amdgcn_sched_barrier(0);
            b[i] = w[(size_t)(ahead < ng ? ahead : ng - 1) * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 4; ++k) a_now[k] = a_next[k];
        }
    }
    // the groups of the last, partial round are in the ring
#pragma unroll
    for (int i = 0; i < kNetPrefetch - 1; ++i)
        if (g + i < ng) {   // wave-uniform
            if (i > 0) a_load(a_now, g + i);
            group(b[i], a_now);
        }
}

__device__ __forceinline__ net_f32x16 net_bias(float b) {
    net_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b;
    return acc;
}

// the row of a 32-row tile that register `reg` of lane `lane` holds
__device__ __forceinline__ int net_acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// A tile's accumulators, activated, into LDS rows of `stride` floats: out points at the tile's [row 0][col 0].
template <bool TANH>
__device__ __forceinline__ void net_store_hidden(float *__restrict__ out, int stride, const net_f32x16 &acc, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[net_acc_row(r, lane) * stride + (lane & 31)] = policy_activation<TANH>(acc[r]);
}

// What net_trunk hands a kernel's output stage: the output tile's accumulators (real where has_out), and where the
// wavefront stands: the workgroup's first row e0 and its `rows` rows with an env, the first row row0 of the
// wavefront's row tile (rt * kNetTile) and its output tile otile.
struct NetTrunk {
    net_f32x16 out;
    int64_t e0;
    int rows, row0, otile;
    bool has_out;
};

// The trunk of policy_net_kernel and value_net_kernel (sng_ppo_net.h): a workgroup's 64 rows of obs [E][O] staged,
// both hidden layers, and the output tile's chains advanced over every chunk of hidden2.  ONE_TILE: the output layer
// has one tile (the value net's), known at compile time.  That flag, the image's description by value, the row tile
// as its first row and the lane left to the kernels are what make both kernels compile to the code they had with the
// trunk written out in each, but for the sense of a branch behind the layers; other spellings of this interface cost
// either kernel about half a percent (profiles/mlp_refactor_ab.txt).  TWO_SRC (q_net_kernel, sng_ddpg.h): a row is
// obs[row][0 .. O1) followed by src2[row][0 .. m.O - O1), the staging loop's sibling below; the kernels without it
// compile to the code they had before it existed (profiles/ddpg_codeobj_diff.txt).
template <bool TANH, bool ONE_TILE = false, bool TWO_SRC = false>
__device__ __forceinline__ NetTrunk net_trunk(const float *__restrict__ img, const NetImage m,
                                              const float *__restrict__ obs, int64_t E,
                                              const float *__restrict__ src2 = nullptr, int O1 = 0) {
    extern __shared__ float4 policy_net_lds4[];
    float *s_h1 = reinterpret_cast<float *>(policy_net_lds4);
    const int h1s = net_lds_h1_stride(m.N1), xs = net_lds_obs_stride(m.K1), cs = net_lds_chunk_stride();
    float *s_x = s_h1 + kNetRows * h1s;   // net_lds_h1: the observation rows, then hidden2's chunk
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = wave & 1, slot = wave >> 1;
    const int64_t e0 = (int64_t)blockIdx.x * kNetRows;
    const int rows = E - e0 < kNetRows ? (int)(E - e0) : kNetRows;
    // the observation rows; zeros past O (the chains' trailing terms) and in the rows without an env
    if constexpr (TWO_SRC) {
        const int O2 = m.O - O1;
        for (int i = tid; i < kNetRows * m.K1; i += kNetBlock) {
            const int r = i / m.K1, c = i - r * m.K1;
            float v = 0.f;
            if (r < rows && c < O1) v = obs[(size_t)(e0 + r) * (size_t)O1 + (size_t)c];
            else if (r < rows && c < m.O) v = src2[(size_t)(e0 + r) * (size_t)O2 + (size_t)(c - O1)];
            s_x[r * xs + c] = v;
        }
    } else {
        for (int i = tid; i < kNetRows * m.K1; i += kNetBlock) {
            const int r = i / m.K1, c = i - r * m.K1;
            s_x[r * xs + c] = (r < rows && c < m.O) ? obs[(size_t)(e0 + r) * (size_t)m.O + (size_t)c] : 0.f;
        }
    }
    __syncthreads();
    const int arow = rt * kNetTile + (lane & 31), ak = lane >> 5;
    const net_f32x4 *img4 = reinterpret_cast<const net_f32x4 *>(img);
    // hidden layer 1: K = O, every tile of N1 outputs into s_h1
    {
        const int ng = m.K1 / kNetKGroup;
        for (int t = slot; t < m.N1 / kNetTile; t += 2) {
            net_f32x16 acc = net_bias(img[m.b1 + (size_t)(t * kNetTile + (lane & 31))]);
            net_tile_chain(acc, s_x + arow * xs + ak, img4 + m.w1 / 4 + (size_t)t * (size_t)ng * 64 + lane, ng);
            net_store_hidden<TANH>(s_h1 + rt * kNetTile * h1s + t * kNetTile, h1s, acc, lane);
        }
    }
    __syncthreads();
    // hidden layer 2 in chunks of kNetChunk outputs (a tile per slot), and the output layer's chains over each chunk
    // the output tile this wavefront keeps, where the layer has that many: one per slot, so act_dim <= kNetMaxAct
    // (net_spec_check refuses more, and launch_policy_net an image with more); the value net's one tile (N3 = 32, of
    // which column 0 is V) is slot 0's
    const int otile = ONE_TILE ? 0 : slot;
    const bool has_out = ONE_TILE ? slot == 0 : otile < m.N3 / kNetTile;
    net_f32x16 out = net_bias(has_out ? img[m.b3 + (size_t)(otile * kNetTile + (lane & 31))] : 0.f);
    const int ng2 = m.K2 / kNetKGroup, ng3 = m.K3 / kNetKGroup;
    for (int c = 0; c < m.N2 / kNetChunk; ++c) {
        const int t = 2 * c + slot;
        net_f32x16 acc = net_bias(img[m.b2 + (size_t)(t * kNetTile + (lane & 31))]);
        net_tile_chain(acc, s_h1 + arow * h1s + ak, img4 + m.w2 / 4 + (size_t)t * (size_t)ng2 * 64 + lane, ng2);
        if (c > 0) __syncthreads();   // the output layer has read the chunk before this one
        net_store_hidden<TANH>(s_x + rt * kNetTile * cs + slot * kNetTile, cs, acc, lane);
        __syncthreads();
        if (has_out) {
            const int g0 = c * (kNetChunk / kNetKGroup);
            const int n = ng3 - g0 < kNetChunk / kNetKGroup ? ng3 - g0 : kNetChunk / kNetKGroup;
            if (n > 0)
                net_tile_chain(out, s_x + arow * cs + ak,
                               img4 + m.w3 / 4 + ((size_t)otile * (size_t)ng3 + (size_t)g0) * 64 + lane, n);
        }
    }
    return {out, e0, rows, rt * kNetTile, otile, has_out};
}

// The actor over E rows.  obs [E][O], noise [E][A] or null, actions [E][A] (a), env_actions [E][A] or null.
template <bool TANH>
__global__ __launch_bounds__(kNetBlock) void policy_net_kernel(const float *__restrict__ img, NetImage m,
                                                               const float *__restrict__ obs,
                                                               const float *__restrict__ noise,
                                                               float *__restrict__ actions,
                                                               float *__restrict__ env_actions, int64_t E) {
    const NetTrunk k = net_trunk<TANH>(img, m, obs, E);
    const int lane = threadIdx.x & (kWave - 1);
    // the output stage, from the accumulators: a and the env action of the rows with an env
    if (k.has_out) {
        const int j = k.otile * kNetTile + (lane & 31);
        if (j < m.A) {
            const float lo = img[m.low + j], hi = img[m.high + j], span = img[m.span + j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = k.row0 + net_acc_row(r, lane);
                if (row < k.rows) {
                    const size_t at = (size_t)(k.e0 + row) * (size_t)m.A + (size_t)j;
                    float a, env;
                    if (m.output == SNG_MLP_OUT_SQUASH) {
                        a = tanhf(k.out[r]);
                        if (noise) {
                            a = a + noise[at];
                            a = a < -1.f ? -1.f : a;
                            a = 1.f < a ? 1.f : a;
                        }
                        // SB3's unscale_action as numpy rounds it: the product and the sum on their own
                        env = __fadd_rn(lo, __fmul_rn(__fmul_rn(0.5f, __fadd_rn(a, 1.0f)), span));
                    } else {
                        a = noise ? k.out[r] + noise[at] : k.out[r];
                        env = a;
                        if (m.clip) {
                            env = a < lo ? lo : a;
                            env = hi < env ? hi : env;
                        }
                    }
                    actions[at] = a;
                    if (env_actions) env_actions[at] = env;
                }
            }
        }
    }
}

}  // namespace sng
