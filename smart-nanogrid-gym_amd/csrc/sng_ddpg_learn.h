// sng_ddpg_learn.h -- the device side of sng_learner_* (include/sng.h): learn_concat_kernel, learn_gemm_kernel,
// learn_loss_kernel and learn_step_kernel.  Included by sng_kernels.hip only, behind sng_policy_net.h (net_f32x16,
// net_bias and net_acc_row are its).  The contract is sng_ddpg_learn_host.h's: Adam's step, the polyak blend and the
// loss gradients are that header's own functions, compiled here for the device.
//
// learn_gemm_kernel is every matrix product of an update, over plain row-major arrays described by strides
// (LearnGemm): a wavefront owns one 32 x 32 tile of C and takes its 1,024 chains through the reduction index two k's
// an MFMA, ascending, in one 16-register accumulator started from the bias (or 0) -- v_mfma_f32_32x32x2_f32 computes
// D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), so the accumulators ARE the host model's fmaf chains (sng_policy_net.h).
// Lane l's operands are A(m0 + (l & 31), k + (l >> 5)) and B(k + (l >> 5), n0 + (l & 31)), read from global memory as
// they lie; what lies outside M, N or the segment's k's is read as 0, a chain's trailing zero terms.  The three shapes:
//     forward     A = the layer's input [rows][K], B(k, n) = W[n][k], init = bias, relu / none / tanh epilogue
//     dOut W      A = dOut [rows][J], B(k, n) = W[k][off + n], the relu mask (or 1 - a^2) as epilogue
//     dOut^T In   A(m, k) = dOut[k][m], B(k, n) = In[k][n] with a column of ones behind it (the bias gradient), the
//                 rows cut into segments of SNG_LEARNER_SEGMENT along grid z, each segment's chains written to its own
//                 block of partials; learn_step_kernel adds the blocks in ascending order.
// A workgroup is four wavefronts, four row tiles of one column tile.  Nothing is staged through LDS: the operands of
// an update at the default 256 rows fit the caches, and the kernels are bound by launch and latency there.
//
// learn_step_kernel is elementwise over a net's six arrays: the ordered sum of the gradient's partials, Adam on the
// master, the polyak blend of the target's master, and both new values written to their places in the two packed
// NetImages that policy_net_kernel and q_net_kernel read (the padding of an image stays as net_pack left it).
#pragma once

#include "sng_ddpg_learn_host.h"

namespace sng {

constexpr int kLearnBlock = 256;
constexpr int kLearnUnroll = 8;   // MFMAs between two batches of loads

// x [rows][O + A] = [obs row | action row]
__global__ __launch_bounds__(kLearnBlock) void learn_concat_kernel(const float *__restrict__ obs,
                                                                   const float *__restrict__ act,
                                                                   float *__restrict__ x, int64_t rows, int O, int A) {
    const int K = O + A;
    const int64_t n = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * kLearnBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLearnBlock) {
        const int64_t r = i / K;
        const int c = (int)(i - r * K);
        x[i] = c < O ? obs[r * O + c] : act[r * A + (c - O)];
    }
}

template <int EPI>
__global__ __launch_bounds__(kLearnBlock) void learn_gemm_kernel(LearnGemm g) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = ((int)blockIdx.y * (kLearnBlock / kWave) + wave) * kNetTile, n0 = (int)blockIdx.x * kNetTile;
    if (m0 >= g.M) return;   // wave-uniform
    const int z = (int)blockIdx.z;
    const int k0 = z * g.S, k1 = g.K - k0 < g.S ? g.K : k0 + g.S;
    const int am = m0 + (lane & 31), bn = n0 + (lane & 31), kh = lane >> 5;
    const bool a_in = am < g.M, b_in = bn < g.N, b_one = bn == g.ones;
    const float *__restrict__ pa = g.a + (a_in ? (int64_t)am * g.a_ms : 0);
    const float *__restrict__ pb = g.b + (b_in && !b_one ? (int64_t)bn * g.b_ns : 0);
    net_f32x16 acc = net_bias(g.init && b_in ? g.init[bn] : 0.f);
    int k = k0;
    // whole batches of kLearnUnroll MFMAs: the loads first, so that they are in flight together
    for (; k + 2 * kLearnUnroll <= k1; k += 2 * kLearnUnroll) {
        float av[kLearnUnroll], bv[kLearnUnroll];
#pragma unroll
        for (int i = 0; i < kLearnUnroll; ++i) {
            const int64_t kk = k + 2 * i + kh;
            av[i] = a_in ? pa[kk * g.a_ks] : 0.f;
            bv[i] = b_in ? (b_one ? 1.0f : pb[kk * g.b_ks]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kLearnUnroll; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
    }
    // the rest, a pair of k's at a time; a k past the segment's end is a zero term
    for (; k < k1; k += 2) {
        const int64_t kk = k + kh;
        const bool in = kk < k1;
        const float av = a_in && in ? pa[kk * g.a_ks] : 0.f;
        const float bv = b_in && in ? (b_one ? 1.0f : pb[kk * g.b_ks]) : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (!b_in) return;
    float *__restrict__ c = g.c + (int64_t)z * g.c_zs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + net_acc_row(r, lane);
        if (row < g.M) {
            float v = acc[r];
            if constexpr (EPI == LEARN_EPI_RELU) v = v > 0.f ? v : 0.f;
            if constexpr (EPI == LEARN_EPI_MASK) v = g.aux[(int64_t)row * g.aux_ms + bn] > 0.f ? v : 0.f;
            if constexpr (EPI == LEARN_EPI_TANH) {
                v = tanhf(v);
                g.c2[(int64_t)row * g.c2_ms + bn] = v;
            }
            if constexpr (EPI == LEARN_EPI_DTANH) v = learn_dtanh(v, g.aux[(int64_t)row * g.aux_ms + bn]);
            c[(int64_t)row * g.c_ms + bn] = v;
        }
    }
}

// The loss's gradient over the rows, and in the grid's last workgroup the loss itself by the segment law
// (learn_loss_sum_host): thread s < the segments (at most 64) adds segment s's terms in row order, all segments side by
// side, 64 rows of each at a time staged through LDS by the whole workgroup (rows of 65 floats: the segments' reads
// differ in bank); then one thread adds the partials in ascending order.  ACTOR: dq = -(1 / rows), loss = -(sum q /
// rows); else the critic's dq = (2 (q - y)) / rows and loss = (sum (q - y)^2) / rows.  Grid ceil(rows / 256) + 1.
constexpr int kLossTile = 64;        // rows of a segment per round
constexpr int kLossSegments = 64;    // SNG_LEARNER_MAX_ROWS / SNG_LEARNER_SEGMENT
static_assert(kLossSegments * (int64_t)kLearnSegment >= kLearnMaxRows && kLearnSegment % kLossTile == 0, "loss tiles");
template <bool ACTOR>
__global__ __launch_bounds__(kLearnBlock) void learn_loss_kernel(const float *__restrict__ q,
                                                                 const float *__restrict__ y, float *__restrict__ dq,
                                                                 float *__restrict__ loss, int64_t rows) {
    __shared__ float s_term[kLossSegments * (kLossTile + 1)];
    __shared__ float s_part[kLossSegments];
    const float rows_f = (float)rows;
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int64_t b = (int64_t)blockIdx.x * kLearnBlock + tid;
        if (b < rows) dq[b] = ACTOR ? learn_dq_pi(rows_f) : learn_dq(q[b], y[b], rows_f);
        return;
    }
    const int nseg = learn_segments(rows);   // <= kLossSegments: launch_learn_loss refuses more rows
    const int seg_len = rows < kLearnSegment ? (int)rows : kLearnSegment;
    float sum = 0.f;
    for (int r0 = 0; r0 < seg_len; r0 += kLossTile) {
        __syncthreads();   // the round before has been added
        for (int i = tid; i < nseg * kLossTile; i += kLearnBlock) {
            const int seg = i / kLossTile, r = i - seg * kLossTile;
            const int64_t b = (int64_t)seg * kLearnSegment + r0 + r;
            float term = 0.f;
            if (b < rows) term = ACTOR ? q[b] : learn_sq_error(q[b], y[b]);
            s_term[seg * (kLossTile + 1) + r] = term;
        }
        __syncthreads();
        if (tid < nseg) {
            const int64_t left = rows - ((int64_t)tid * kLearnSegment + r0);   // rows of this segment from r0 on
            const int n = left < kLossTile ? (left > 0 ? (int)left : 0) : kLossTile;
            for (int i = 0; i < n; ++i) sum = noise_add(sum, s_term[tid * (kLossTile + 1) + i]);
        }
    }
    if (tid < nseg) s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        float g = s_part[0];
        for (int z = 1; z < nseg; ++z) g = noise_add(g, s_part[z]);
        *loss = ACTOR ? -learn_mean_of(g, rows_f) : learn_mean_of(g, rows_f);
    }
}

// ADAM: the gradient, Adam, polyak and both images; else the images only, from the masters as they are
// (sng_learner_set_state).
template <bool ADAM>
__global__ __launch_bounds__(kLearnBlock) void learn_step_kernel(LearnStep s) {
    for (uint64_t e = (uint64_t)blockIdx.x * kLearnBlock + threadIdx.x; e < s.total;
         e += (uint64_t)gridDim.x * kLearnBlock) {
        uint64_t at = e;
        int i = 0;
#pragma unroll
        for (int n = 0; n < 5; ++n)
            if (i == n && at >= s.t[n].n) at -= s.t[n].n, i = n + 1;
        const LearnTensor &t = s.t[i];
        const int j = t.I ? (int)(at / (uint64_t)t.I) : (int)at, col = t.I ? (int)(at - (uint64_t)j * t.I) : 0;
        float p = t.p[at], tg = t.t[at];
        if constexpr (ADAM) {
            const float *part = t.part + (uint64_t)j * (uint64_t)(t.cols + 1) + (uint64_t)(t.I ? col : t.cols);
            float grad = part[0];
            for (int zz = 1; zz < s.nseg; ++zz) grad = noise_add(grad, part[(uint64_t)zz * t.zs]);
            float m = t.m[at], v = t.v[at];
            p = learn_adam(p, grad, &m, &v, s.adam);
            tg = learn_polyak(tg, p, s.tau, s.one_m_tau);
            t.g[at] = grad, t.m[at] = m, t.v[at] = v, t.p[at] = p, t.t[at] = tg;
        }
        const uint64_t img = t.img_at + (t.I ? (uint64_t)learn_image_at(t.KP, j, col) : (uint64_t)j);
        s.img[img] = p;
        s.img_target[img] = tg;
    }
}

}  // namespace sng
