// sng_noise.h -- action_noise_kernel<KIND>, the device side of a noise source (include/sng.h, sng_noise_create), and the
// one-thread kernel that advances its counter.  Included by sng_kernels.hip only.  The arithmetic is sng_noise_host.h's,
// the same text the host model compiles.
//
// A block [T][E][A] is T rows of E A consecutive floats.  A thread owns four consecutive elements of the row -- it
// derives their (env, action) once, with one division a thread, builds their stream keys once per block, and walks t: per
// step a hash (three 32-bit multiplies), a count of leading zeros, one 16-byte LDS read of the segment's coefficients
// at a lane-dependent address, three fmaf, and the kind's own one or two operations; the OU state of its four
// elements stays in registers, and the Gaussian kind runs the same loop without that dependency.  A step's four
// values leave as one 16-byte nontemporal store where the rows are 16-byte aligned (the block's base is, and E A is a
// multiple of four), else as four 4-byte stores under the row's bound.  The coefficient table (1,984 B) is copied to
// LDS once per workgroup.  Half of all lanes read octave 0's four slots and a quarter octave 1's, and lanes that read
// the same address are served together, so the lookup's conflicts are the tail octaves' only.  Grid x covers the row, y
// the blocks of a fill (a workgroup loops where a fill has more blocks than a grid has rows); offsets are 64-bit.
#pragma once

#include "sng_noise_host.h"

namespace sng {

constexpr int kNoiseBlock = 256;   // threads of a workgroup
constexpr int kNoisePer = 4;       // consecutive elements of a row per thread
constexpr int kNoiseMaxGridDays = 65535;

// params: mu [A], sd [A] (noise_pack_params); counter: the source's, read by every thread and advanced behind this
// kernel (noise_bump_kernel), never by it; out [days][T][E][A].  vec: every row of out is 16-byte aligned.
template <int KIND>
__global__ __launch_bounds__(kNoiseBlock) void action_noise_kernel(const float *__restrict__ params,
                                                                   const uint64_t *__restrict__ counter, uint64_t seed,
                                                                   int64_t env_offset, float theta, float dt,
                                                                   float *__restrict__ out, int days, int T, int64_t E,
                                                                   int A, int vec) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    __shared__ v4f s_tab[kNoiseOctaves * kNoiseSubs];
    const int tid = threadIdx.x;
    if (tid < kNoiseOctaves * kNoiseSubs) {
        const v4f c = {kNoiseIcdf[4 * tid], kNoiseIcdf[4 * tid + 1], kNoiseIcdf[4 * tid + 2], kNoiseIcdf[4 * tid + 3]};
        s_tab[tid] = c;
    }
    __syncthreads();
    const int64_t row = E * (int64_t)A;
    const int64_t i0 = ((int64_t)blockIdx.x * kNoiseBlock + tid) * kNoisePer;
    if (i0 >= row) return;
    uint64_t ge[kNoisePer];
    uint32_t j[kNoisePer];
    float mu[kNoisePer], sd[kNoisePer];
    // one division a thread: the first element's (env, action), the others by stepping the action.  An element past
    // the row's end gets the env after the last one (or a later action of the last) and is never stored.
    int64_t e = i0 / A;
    uint32_t ja = (uint32_t)(i0 - e * A);
#pragma unroll
    for (int k = 0; k < kNoisePer; ++k) {
        j[k] = ja;
        ge[k] = (uint64_t)(env_offset + e);
        mu[k] = params[ja];
        sd[k] = params[A + ja];
        if (++ja == (uint32_t)A) {
            ja = 0;
            ++e;
        }
    }
    const uint64_t c0 = *counter;
    for (int d = blockIdx.y; d < days; d += gridDim.y) {
        const uint32_t dk = noise_day_key(seed, c0 + (uint64_t)d);
        uint32_t key[kNoisePer];
        float x[kNoisePer];
#pragma unroll
        for (int k = 0; k < kNoisePer; ++k) {
            key[k] = noise_key_of(dk, ge[k], j[k]);
            x[k] = 0.f;
        }
        float *o = out + (size_t)d * (size_t)T * (size_t)row + (size_t)i0;
#pragma unroll 2
        for (int t = 0; t < T; ++t, o += row) {
#pragma unroll
            for (int k = 0; k < kNoisePer; ++k) {
                const uint32_t h = noise_hash(key[k], (uint32_t)t);
                float f;
                const v4f c = s_tab[noise_segment(h, &f)];
                const float z = noise_variate(h, f, c.x, c.y, c.z, c.w);
                x[k] = KIND == SNG_NOISE_OU ? noise_ou_step(x[k], mu[k], sd[k], theta, dt, z) : noise_gaussian(mu[k], sd[k], z);
            }
            if (vec) {
                const v4f v = {x[0], x[1], x[2], x[3]};
                SNG_ST(*reinterpret_cast<v4f *>(o), v);
            } else {
#pragma unroll
                for (int k = 0; k < kNoisePer; ++k)
                    if (i0 + k < row) SNG_ST(o[k], x[k]);
            }
        }
    }
}

// Behind a fill on the same stream: nothing reads the counter while it runs.
__global__ void noise_bump_kernel(uint64_t *counter, uint64_t amount) { *counter += amount; }

}  // namespace sng
