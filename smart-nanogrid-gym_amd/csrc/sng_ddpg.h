// sng_ddpg.h -- the device side of sng_replay_* and sng_critic_* (include/sng.h): replay_push_kernel,
// replay_sample_kernel and q_net_kernel.  Included by sng_kernels.hip only, behind sng_policy_net.h (net_trunk and
// net_acc_row are its).  The contracts are sng_ddpg_host.h's: the sampling law and the TD target are that header's
// own functions, compiled here for the device.
//
// replay_push_kernel copies a push's segments (sng_ddpg_host.h, replay_push_args: one per run of consecutive slots
// and array), grid y over the segments, x over a segment's 16-byte groups.  A segment whose source and destination
// reach a 16-byte boundary at the same element is copied 16 bytes a lane between its unaligned ends (a day's blocks
// are whole multiples of 16 bytes at every population that is a multiple of 4 envs); any other an element a lane.
//
// replay_sample_kernel takes 64 batch rows a workgroup of four wavefronts: the first 64 threads compute their row's
// index once, gather its reward and done and leave the index and the observation row in LDS; then the workgroup's
// 64 O (and 64 A) output floats, which are contiguous, are written one dword a lane, each lane reading the float of
// its row, so a row's reads are contiguous runs of O (A) dwords and the writes are dense.  O = 2N + 9 and A = N + 1
// are odd, so nothing here assumes a row is 16-byte aligned.
//
// q_net_kernel is policy_net_kernel's trunk with a row staged from two arrays, obs[row] | actions[row], and
// value_net_kernel's output stage (column 0 of the one output tile); with TARGET the TD target follows, reading the
// row's reward and done.
#pragma once

#include "sng_ddpg_host.h"

namespace sng {

constexpr int kPushBlock = 256;
constexpr int kPushPer = 4;   // 16-byte groups a thread, at the grid's size

typedef float push_f32x4 __attribute__((ext_vector_type(4)));
typedef double push_f64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t push_u32x4 __attribute__((ext_vector_type(4)));

// n elements from src to dst, converted: S float / double / uint8_t, D float / uint8_t.
template <class S, class D>
__device__ __forceinline__ void push_copy(const S *__restrict__ src, D *__restrict__ dst, int64_t n, int64_t tid,
                                          int64_t stride) {
    constexpr int V = 16 / (int)sizeof(D);   // elements of a 16-byte store
    // the elements before dst's first 16-byte boundary
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / (unsigned)sizeof(D));
    head = head < n ? head : n;
    const bool vec = ((uintptr_t)(src + head) & 15u) == 0;   // src's vector loads are aligned from there too
    const int64_t groups = vec ? (n - head) / V : 0;
    const S *sv = src + head;
    D *dv = dst + head;
    for (int64_t j = tid; j < groups; j += stride) {
        if constexpr (sizeof(S) == 8) {   // two 16-byte loads, one 16-byte store
            const push_f64x2 a = reinterpret_cast<const push_f64x2 *>(sv)[2 * j];
            const push_f64x2 b = reinterpret_cast<const push_f64x2 *>(sv)[2 * j + 1];
            const push_f32x4 v = {(float)a.x, (float)a.y, (float)b.x, (float)b.y};
            reinterpret_cast<push_f32x4 *>(dv)[j] = v;
        } else if constexpr (sizeof(D) == 4) {
            reinterpret_cast<push_f32x4 *>(dv)[j] = reinterpret_cast<const push_f32x4 *>(sv)[j];
        } else {
            reinterpret_cast<push_u32x4 *>(dv)[j] = reinterpret_cast<const push_u32x4 *>(sv)[j];
        }
    }
    // the ends (everything, where the two sides' alignments differ), an element a thread
    const int64_t tail = head + groups * V;
    for (int64_t i = tid; i < head; i += stride) dst[i] = (D)src[i];
    for (int64_t i = tail + tid; i < n; i += stride) dst[i] = (D)src[i];
}

__global__ __launch_bounds__(kPushBlock) void replay_push_kernel(PushArgs a) {
    const PushSegment s = a.seg[blockIdx.y];
    const int64_t tid = (int64_t)blockIdx.x * kPushBlock + threadIdx.x, stride = (int64_t)gridDim.x * kPushBlock;
    if (s.kind == PUSH_F32)
        push_copy(static_cast<const float *>(s.src), static_cast<float *>(s.dst), s.n, tid, stride);
    else if (s.kind == PUSH_F64_F32)
        push_copy(static_cast<const double *>(s.src), static_cast<float *>(s.dst), s.n, tid, stride);
    else
        push_copy(static_cast<const uint8_t *>(s.src), static_cast<uint8_t *>(s.dst), s.n, tid, stride);
}

constexpr int kSampleRows = 64;
constexpr int kSampleBlock = 256;

// `batch` rows drawn from the ring's n transitions (TE = T * E per slot) with the sample's key (replay_sample_key).
// Grid ceil(batch / 64).
__global__ __launch_bounds__(kSampleBlock) void replay_sample_kernel(ReplayStorage ring, SngReplayBatch out,
                                                                     uint32_t key, uint64_t n, uint64_t TE, uint64_t E,
                                                                     int O, int A, int64_t batch) {
    __shared__ uint64_t s_at[kSampleRows], s_row[kSampleRows];   // the transition; its row of the ring's obs
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kSampleRows;
    const int rows = batch - b0 < kSampleRows ? (int)(batch - b0) : kSampleRows;
    if (tid < rows) {
        const int64_t b = b0 + tid;
        const uint64_t i = replay_sample_index(replay_sample_bits(key, (uint64_t)b), n);
        s_at[tid] = i;
        s_row[tid] = replay_obs_row(i, TE, E);
        out.reward[b] = ring.reward[i];
        out.done[b] = (float)ring.done[i];
        if (out.index) out.index[b] = (int64_t)i;
    }
    __syncthreads();
    const size_t sO = (size_t)O, sA = (size_t)A, next = (size_t)E * sO;   // a step's observation block
    const float *__restrict__ r_obs = ring.obs;
    const float *__restrict__ r_act = ring.actions;
    float *__restrict__ o_obs = out.obs + (size_t)b0 * sO;
    float *__restrict__ o_next = out.next_obs + (size_t)b0 * sO;
    float *__restrict__ o_act = out.actions + (size_t)b0 * sA;
    for (int j = tid; j < rows * O; j += kSampleBlock) {
        const int r = j / O, c = j - r * O;
        const size_t at = (size_t)s_row[r] * sO + (size_t)c;
        o_obs[j] = r_obs[at];
        o_next[j] = r_obs[at + next];
    }
    for (int j = tid; j < rows * A; j += kSampleBlock) {
        const int r = j / A, c = j - r * A;
        o_act[j] = r_act[(size_t)s_at[r] * sA + (size_t)c];
    }
}

// obs [rows][O], actions [rows][m.O - O] -> out [rows]: Q, or with TARGET the TD target of reward / done [rows] and
// g = (float)gamma.  Grid ceil(rows / 64); rows and every row offset are 64-bit.
template <bool TANH, bool TARGET>
__global__ __launch_bounds__(kNetBlock) void q_net_kernel(const float *__restrict__ img, NetImage m,
                                                          const float *__restrict__ obs,
                                                          const float *__restrict__ actions, int O,
                                                          const float *__restrict__ reward,
                                                          const float *__restrict__ done, float g,
                                                          float *__restrict__ out, int64_t rows_all) {
    const NetTrunk k = net_trunk<TANH, true, true>(img, m, obs, rows_all, actions, O);
    const int lane = threadIdx.x & (kWave - 1);
    // Q: column 0 of the output tile, of the rows below rows_all
    if (k.has_out && (lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = k.row0 + net_acc_row(r, lane);
            if (row < k.rows) {
                const size_t at = (size_t)(k.e0 + row);
                if constexpr (TARGET) out[at] = critic_td_target(reward[at], done[at], g, k.out[r]);
                else out[at] = k.out[r];
            }
        }
    }
}

}  // namespace sng
