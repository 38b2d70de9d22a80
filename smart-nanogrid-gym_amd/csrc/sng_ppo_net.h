// sng_ppo_net.h -- what finishes a PPO rollout whose value net has any two hidden widths: value_net_kernel and
// gae_scan_kernel, the device side of sng_ppo_create_net.  Included by sng_kernels.hip only, behind sng_policy_net.h
// (net_tile_chain, net_bias, net_store_hidden and the LDS plan are its).
//
// The arithmetic is the contract of sng_ppo_net_host.h.  A trajectory obs [days][T + 1][E][O] is days (T + 1) E
// contiguous observation rows, so the value net runs over it as one flat batch, 64 rows a workgroup, exactly as
// policy_net_kernel runs an actor: hidden1 whole in LDS, hidden2 in chunks of 64 outputs, the output layer's chains
// advancing over each chunk in k order.  The output tile has one real column (V), which the lanes holding column 0
// store.  A row block may straddle steps and days; nothing in the kernel knows of either.
//
// gae_scan_kernel then reads the values back.  Its grid's y dimension holds the days and, with the log-probability
// stage, T more rows: a workgroup of one wavefront with y < days walks 64 consecutive envs of day y backwards,
// one thread an env, V[t + 1] and gae in registers, the loads of kScanAhead steps issued ahead of their recurrence
// steps (none of them depends on it); a workgroup with y = days + t sums the log-probabilities of step t's 64 rows
// from a noise tile staged through LDS (coalesced global reads, rows of an odd stride in LDS) and stores them to
// every day's logp.  Every f32 operation of both is rounded on its own.
#pragma once

#include "sng_ppo_net_host.h"

namespace sng {

// obs [rows][O] -> values [rows].  Grid ceil(rows / 64); rows and every row offset are 64-bit.
template <bool TANH>
__global__ __launch_bounds__(kNetBlock) void value_net_kernel(const float *__restrict__ img, NetImage m,
                                                              const float *__restrict__ obs,
                                                              float *__restrict__ values, int64_t rows_all) {
    extern __shared__ float4 value_net_lds4[];
    float *s_h1 = reinterpret_cast<float *>(value_net_lds4);
    const int h1s = net_lds_h1_stride(m.N1), xs = net_lds_obs_stride(m.K1), cs = net_lds_chunk_stride();
    float *s_x = s_h1 + kNetRows * h1s;   // net_lds_h1: the observation rows, then hidden2's chunk
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = wave & 1, slot = wave >> 1;
    const int64_t e0 = (int64_t)blockIdx.x * kNetRows;
    const int rows = rows_all - e0 < kNetRows ? (int)(rows_all - e0) : kNetRows;
    // the observation rows; zeros past O (the chains' trailing terms) and in the rows past the last one
    for (int i = tid; i < kNetRows * m.K1; i += kNetBlock) {
        const int r = i / m.K1, c = i - r * m.K1;
        s_x[r * xs + c] = (r < rows && c < m.O) ? obs[(size_t)(e0 + r) * (size_t)m.O + (size_t)c] : 0.f;
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
    // hidden layer 2 in chunks of kNetChunk outputs (a tile per slot); the output layer has one tile (N3 = 32, of
    // which column 0 is V), kept by the wavefronts of slot 0, whose chains advance over each chunk
    const bool has_out = slot == 0;
    net_f32x16 out = net_bias(has_out ? img[m.b3 + (size_t)(lane & 31)] : 0.f);
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
            if (n > 0) net_tile_chain(out, s_x + arow * cs + ak, img4 + m.w3 / 4 + (size_t)g0 * 64 + lane, n);
        }
    }
    // V: column 0 of the output tile, of the rows below rows_all
    if (has_out && (lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rt * kNetTile + net_acc_row(r, lane);
            if (row < rows) values[(size_t)(e0 + row)] = out[r];
        }
    }
}

constexpr int kScanBlock = kWave;   // envs of a workgroup: one wavefront
constexpr int kScanAhead = 8;       // steps whose reward, done and V are requested before their recurrence steps run

// gae_scan_kernel's LDS with the log-probability stage: the noise tile [64][A | 1] (an odd stride: a wavefront's 64
// rows differ in bank at every j)
constexpr int gae_scan_noise_stride(int A) { return A | 1; }
inline size_t gae_scan_lds_bytes(int A) { return (size_t)kScanBlock * (size_t)gae_scan_noise_stride(A) * sizeof(float); }

// One step of the recurrence (sng_ppo_host.h, ppo_gae_step): `gae` in, the step's advantage out; ret = advantage + v.
__device__ __forceinline__ float gae_step(float g, float gl, float r, float nn, float v, float v_next, float gae,
                                          float &ret) {
    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(g, v_next), nn)), v);
    const float a = __fadd_rn(delta, __fmul_rn(__fmul_rn(gl, nn), gae));
    ret = __fadd_rn(a, v);
    return a;
}

// One term of a row's log-probability (sng_ppo_host.h, ppo_logp_row)
__device__ __forceinline__ float logp_term(float noise, float inv_std, float log_std) {
    const float z = __fmul_rn(noise, inv_std);
    return __fsub_rn(__fsub_rn(__fmul_rn(__fmul_rn(-0.5f, z), z), log_std), kHalfLog2Pi);
}

// reward / done [days][T][E], values [days][T + 1][E] (read), advantages / returns [days][T][E]; with LOGP noise
// [T][E][A] and logp [days][T][E], log_std / inv_std at img + log_std_at / inv_std_at.  g, gl: gamma and
// gamma * lambda (ppo_gamma_f32, ppo_gamma_lambda_f32).  Grid (ceil(E / 64), days + (LOGP ? T : 0)).
template <bool LOGP>
__global__ __launch_bounds__(kScanBlock) void gae_scan_kernel(const float *__restrict__ img, size_t log_std_at,
                                                              size_t inv_std_at, int A,
                                                              const double *__restrict__ reward,
                                                              const uint8_t *__restrict__ done,
                                                              const float *__restrict__ noise,
                                                              const float *__restrict__ values,
                                                              float *__restrict__ advantages,
                                                              float *__restrict__ returns, float *__restrict__ logp,
                                                              int64_t E, int T, int days, float g, float gl) {
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kScanBlock, e = e0 + tid;
    const int y = blockIdx.y;
    if (!LOGP || y < days) {
        if (e >= E) return;
        const size_t sE = (size_t)E;
        const size_t out_d = (size_t)y * (size_t)T * sE + (size_t)e;         // of step 0, this thread's env
        const size_t val_d = (size_t)y * (size_t)(T + 1) * sE + (size_t)e;
        float v_next = values[val_d + (size_t)T * sE], gae = 0.0f;
#pragma unroll 1
        for (int t1 = T; t1 > 0; t1 -= kScanAhead) {
            float r[kScanAhead], nn[kScanAhead], v[kScanAhead];
#pragma unroll
            for (int k = 0; k < kScanAhead; ++k) {   // the steps below 0 re-read step 0 and are dropped
                const int t = t1 - 1 - k < 0 ? 0 : t1 - 1 - k;
                const size_t at = out_d + (size_t)t * sE;
                r[k] = (float)reward[at];
                nn[k] = __fsub_rn(1.0f, (float)done[at]);
                v[k] = values[val_d + (size_t)t * sE];
            }
#pragma unroll
            for (int k = 0; k < kScanAhead; ++k) {
                const int t = t1 - 1 - k;
                if (t >= 0) {
                    float ret;
                    gae = gae_step(g, gl, r[k], nn[k], v[k], v_next, gae, ret);
                    const size_t at = out_d + (size_t)t * sE;
                    SNG_ST(advantages[at], gae);
                    SNG_ST(returns[at], ret);
                    v_next = v[k];
                }
            }
        }
        return;
    }
    if constexpr (LOGP) {
        extern __shared__ float4 gae_scan_lds4[];
        float *s_nz = reinterpret_cast<float *>(gae_scan_lds4);
        const int t = y - days, stride = gae_scan_noise_stride(A);
        const int rows = E - e0 < kScanBlock ? (int)(E - e0) : kScanBlock;
        // step t's noise rows of these envs are rows * A floats in a row: thread i takes floats i, i + 64, ..
        const float *src = noise + ((size_t)t * (size_t)E + (size_t)e0) * (size_t)A;
        const int count = rows * A, qr = kScanBlock / A, qc = kScanBlock - qr * A;
        int r = tid / A, c = tid - r * A;
#pragma unroll 4
        for (int i = tid; i < count; i += kScanBlock) {
            s_nz[r * stride + c] = src[i];
            r += qr;
            c += qc;
            if (c >= A) {
                c -= A;
                ++r;
            }
        }
        __syncthreads();
        if (tid < rows) {
            const float *nz = s_nz + tid * stride, *ls = img + log_std_at, *is = img + inv_std_at;
            float lp = 0.0f;
            for (int j = 0; j < A; ++j) lp = __fadd_rn(lp, logp_term(nz[j], is[j], ls[j]));
            const size_t at = (size_t)t * (size_t)E + (size_t)e, day = (size_t)T * (size_t)E;
            for (int d = 0; d < days; ++d) SNG_ST(logp[(size_t)d * day + at], lp);
        }
    }
}

}  // namespace sng
