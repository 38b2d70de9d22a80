// sng_ppo_net.h -- what finishes a PPO rollout whose value net has any two hidden widths: value_net_kernel and
// gae_scan_kernel, the device side of sng_ppo_create_net.  Included by sng_kernels.hip only, behind sng_policy_net.h
// (net_trunk and net_acc_row are its) and sng_ppo.h (gae_step and logp_term are its).
//
// The arithmetic is the contract of sng_ppo_net_host.h.  A trajectory obs [days][T + 1][E][O] is days (T + 1) E
// contiguous observation rows, so the value net runs over it as one flat batch, 64 rows a workgroup, through the trunk
// that policy_net_kernel runs an actor through (net_trunk; the layout is explained at the head of sng_policy_net.h).
// The output tile has one real column (V), which the lanes holding column 0 store.  A row block may straddle steps
// and days; nothing in the kernel knows of either.
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
    const NetTrunk k = net_trunk<TANH, true>(img, m, obs, rows_all);
    const int lane = threadIdx.x & (kWave - 1);
    // V: column 0 of the output tile, of the rows below rows_all
    if (k.has_out && (lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = k.row0 + net_acc_row(r, lane);
            if (row < k.rows) values[(size_t)(k.e0 + row)] = k.out[r];
        }
    }
}

constexpr int kScanBlock = kWave;   // envs of a workgroup: one wavefront
constexpr int kScanAhead = 8;       // steps whose reward, done and V are requested before their recurrence steps run

// gae_scan_kernel's LDS with the log-probability stage: the noise tile [64][A | 1] (an odd stride: a wavefront's 64
// rows differ in bank at every j)
constexpr int gae_scan_noise_stride(int A) { return A | 1; }
inline size_t gae_scan_lds_bytes(int A) { return (size_t)kScanBlock * (size_t)gae_scan_noise_stride(A) * sizeof(float); }

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
