// sng_dev_util.h -- device primitives every kernel file builds on: the wavefront size, the streaming-store macro
// and the diagnostic hooks, raw buffer loads / stores (bld, bst and their 2 B and 16 B forms), the byte offsets
// of the packed-record quads and SoC pairs, the LDS tile stagers (copy_in, TileStage, copy_out) and the
// wavefront-local LDS fence.  Needs <hip/hip_runtime.h>, <stdint.h> and sng_layout.h (DeviceState, the record
// fields).  Included by sng_kernels.hip only, first.
#pragma once

namespace sng {

constexpr int kWave = 64;

// Streaming (nontemporal) stores for the step's bulk outputs (SoC, observations): they leave
// less dirty L2 for the end-of-kernel release (measured 8.92 -> 8.17 us per step at 65,536 x 10).
#define SNG_ST(dst, v) __builtin_nontemporal_store((v), &(dst))
#include "sng_diag_hooks.h"   // empty hooks in libsng.so (tools/diag builds fill them)

__host__ __device__ constexpr int round4(int x) { return (x + 3) & ~3; }

// Raw buffer access: V# = an array (or a per-step timeline plane) in SGPRs, a wave-uniform
// byte offset (soffset, e.g. the charger row) and a per-lane 32-bit byte offset (the env).  The
// adds happen in the buffer unit instead of as 64-bit VALU adds per access.  Every array or plane
// addressed this way is < 4 GiB (checked at sng_create).  dword3 0x00020000: gfx9 raw buffer.
using Rsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ Rsrc rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, -1, 0x00020000);
}
constexpr int kNT = 2;   // buffer cache-policy bit: nontemporal (streaming) access
typedef unsigned v2u __attribute__((ext_vector_type(2)));
template <class T, int POL = 0>
__device__ __forceinline__ T bld(const T *base, uint32_t voff, uint32_t soff = 0) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4 or 8 byte elements");
    if constexpr (sizeof(T) == 8)
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rsrc(base), voff, soff, POL));
    else
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(rsrc(base), voff, soff, POL));
}
template <int POL = 0, class T>
__device__ __forceinline__ void bst(T *base, uint32_t voff, T v, uint32_t soff = 0) {
    static_assert(sizeof(T) == 1 || sizeof(T) == 4 || sizeof(T) == 8, "1, 4 or 8 byte elements");
    if constexpr (sizeof(T) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), rsrc(base), voff, soff, POL);
    else if constexpr (sizeof(T) == 4)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc(base), voff, soff, POL);
    else
        __builtin_amdgcn_raw_buffer_store_b8(__builtin_bit_cast(unsigned char, v), rsrc(base), voff, soff, POL);
}
// 2 B buffer accesses (the packed records of a device-RNG day, sng_layout.h), zero-extended.
__device__ __forceinline__ uint32_t bld16(const uint16_t *base, uint32_t voff, uint32_t soff = 0) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rsrc(base), voff, soff, 0);
}
template <int POL = 0>
__device__ __forceinline__ void bst16(uint16_t *base, uint32_t voff, uint32_t v, uint32_t soff = 0) {
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, rsrc(base), voff, soff, POL);
}
// A device-RNG day's packed records (u16 [T+1][N][E] in the aux buffer) and a record's capacity field; a
// host-RNG or injected day's word carries it in bits 8-15 (sng_layout.h).
__device__ __forceinline__ const uint16_t *packed_records(const DeviceState &s) {
    return reinterpret_cast<const uint16_t *>(s.aux);
}
template <bool PK>
__device__ __forceinline__ uint32_t cap_field(uint32_t w) {
    return PK ? (w >> P_CAP_SHIFT) & P_CAP_MASK : (w >> W_CAP_SHIFT) & 0xffu;
}
// Byte offset of charger c of env el in a packed-record plane (charger quads, sng_layout.h rec_index): the
// per-lane part (v) and the wave-uniform quad row (s).
struct RecOff {
    uint32_t v, s;
};
__device__ __forceinline__ RecOff rec_off(int c, int n, int64_t E, uint32_t el) {
    const int c0 = c & ~3;
    const uint32_t w = (uint32_t)(n - c0 < 4 ? n - c0 : 4);
    return {(el * w + (uint32_t)(c & 3)) * 2u, (uint32_t)c0 * (uint32_t)E * 2u};
}
// The four records of one 8 B quad slot.
__device__ __forceinline__ void unpack_quad(uint64_t x, uint32_t *w) {
    w[0] = (uint32_t)x & 0xffffu;
    w[1] = (uint32_t)(x >> 16) & 0xffffu;
    w[2] = (uint32_t)(x >> 32) & 0xffffu;
    w[3] = (uint32_t)(x >> 48);
}
// Two f64 in one 16 B buffer access (a charger pair of the SoC state, sng_layout.h).
typedef unsigned v4u __attribute__((ext_vector_type(4)));
template <int POL = 0>
__device__ __forceinline__ void bld2(const double *base, uint32_t voff, uint32_t soff, double &a, double &b) {
    const v4u x = __builtin_amdgcn_raw_buffer_load_b128(rsrc(base), voff, soff, POL);
    a = __builtin_bit_cast(double, (uint64_t)x.x | ((uint64_t)x.y << 32));
    b = __builtin_bit_cast(double, (uint64_t)x.z | ((uint64_t)x.w << 32));
}
// The wave-uniform offset goes into the V# base, not the soffset field: a MUBUF store of more than 8 B reads
// its data VGPRs a cycle late, and the compiler (ROCm 7.2 LLVM) inserts the wait state a VALU write of those
// VGPRs needs only when soffset is not a register.  gfx950 needs it either way: with an SGPR soffset, a
// v_cvt writing the pair's high dword right after the store corrupted ~0.1 % of the stored SoC slots at
// 65,536 envs (two waves per SIMD; tests/test_gpu_bench_kernel.py, tools/dbg/pairs_dbg.py).
template <int POL = 0>
__device__ __forceinline__ void bst2(double *base, uint32_t voff, double a, double b, uint32_t soff = 0) {
    const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
    const v4u x = {(unsigned)ua, (unsigned)(ua >> 32), (unsigned)ub, (unsigned)(ub >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(x, rsrc(reinterpret_cast<char *>(base) + soff), voff, 0, POL);
}
// Byte offset of charger c of the env whose 8 B slot offset is el8 (8 * env) in the SoC state (charger
// pairs, sng_layout.h soc_index), split into the per-lane part (v) and the wave-uniform part (s).
struct SocOff {
    uint32_t v, s;
};
__device__ __forceinline__ SocOff soc_off(int c, int n, int64_t E, uint32_t el8) {
    const int c0 = c & ~1;
    const bool two = c0 + 2 <= n;
    return {two ? 2u * el8 : el8, (uint32_t)c0 * (uint32_t)E * 8u + (two ? (uint32_t)(c & 1) * 8u : 0u)};
}

// Copy `count` floats global -> LDS with 16 B per lane when the run is aligned.  Each thread
// issues up to K loads before the first LDS write (clamped, unconditional loads: no per-element
// branch + wait), so the whole copy is one HBM round trip when count <= K * 4 * BLOCK floats.
template <int K, int BLOCK>
__device__ __forceinline__ void copy_in(float *__restrict__ dst, const float *__restrict__ src, int count,
                                        bool vec, int tid) {
    if (vec && (count & 3) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        const int n4 = count >> 2;
        for (int base = 0; base < n4; base += K * BLOCK) {
            float4 v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = base + k * BLOCK + tid;
                v[k] = s4[i < n4 ? i : n4 - 1];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {   // out-of-range threads rewrite the last element (same value)
                const int i = base + k * BLOCK + tid;
                d4[i < n4 ? i : n4 - 1] = v[k];
            }
        }
    } else {
        for (int base = 0; base < count; base += 4 * K * BLOCK) {
            float v[4 * K];
#pragma unroll
            for (int k = 0; k < 4 * K; ++k) {
                const int i = base + k * BLOCK + tid;
                v[k] = src[i < count ? i : count - 1];
            }
#pragma unroll
            for (int k = 0; k < 4 * K; ++k) {
                const int i = base + k * BLOCK + tid;
                dst[i < count ? i : count - 1] = v[k];
            }
        }
    }
}

// The same copy split in two so other loads can be issued in between: issue() puts the
// block's tile in registers (one load per lane and k), commit() writes it to LDS.  When the
// tile does not fit one round (count > 4 * K * BLOCK floats) issue() does nothing and commit()
// falls back to copy_in.  Native vector types only (HIP's float4 wrapper keeps the array
// from being promoted to registers).
// VEC_ONLY: only the aligned form (16 B loads) is staged in registers; an unaligned tile goes through copy_in at
// commit() whatever its size.  For a caller that issues in one loop iteration and commits in the next (the day
// kernel): the compiler's wait insertion does not know that the two forms exclude each other, sees the
// one-float loads of one iteration pending where the next overwrites the same registers with its 16 B loads,
// and makes every wavefront wait there for all it has in flight.  (At the day kernel's geometry the one-float
// form held only a last wavefront of at most 11 envs.)
template <int K, int BLOCK, bool VEC_ONLY = false>
struct TileStage {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v[K];
    const float *src;
    int count;
    bool vec, one_round;
    __device__ __forceinline__ void issue(const float *__restrict__ s, int cnt, bool vec_io, int tid) {
        src = s;
        count = cnt;
        vec = vec_io && (cnt & 3) == 0;
        one_round = vec ? (cnt >> 2) <= K * BLOCK : !VEC_ONLY && cnt <= K * BLOCK;
        if (!one_round) return;
        if (VEC_ONLY || vec) {
            const v4f *s4 = reinterpret_cast<const v4f *>(s);
            const int n4 = cnt >> 2;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = k * BLOCK + tid;
                v[k] = s4[i < n4 ? i : n4 - 1];
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = k * BLOCK + tid;
                v[k].x = s[i < cnt ? i : cnt - 1];
            }
        }
    }
    __device__ __forceinline__ void commit(float *__restrict__ dst, int tid) {
        if (!one_round) {
            copy_in<K, BLOCK>(dst, src, count, vec, tid);
            return;
        }
        if (VEC_ONLY || vec) {
            v4f *d4 = reinterpret_cast<v4f *>(dst);
            const int n4 = count >> 2;
#pragma unroll
            for (int k = 0; k < K; ++k) {   // out-of-range threads rewrite the last element (same value)
                const int i = k * BLOCK + tid;
                d4[i < n4 ? i : n4 - 1] = v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = k * BLOCK + tid;
                dst[i < count ? i : count - 1] = v[k].x;
            }
        }
    }
};

template <int BLOCK>
__device__ __forceinline__ void copy_out(float *__restrict__ dst, const float *__restrict__ src, int count,
                                         bool vec, int tid) {
    if (vec && (count & 3) == 0) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f *s4 = reinterpret_cast<const v4f *>(src);
        v4f *d4 = reinterpret_cast<v4f *>(dst);
        for (int i = tid; i < (count >> 2); i += BLOCK) SNG_ST(d4[i], s4[i]);
    } else {
        for (int i = tid; i < count; i += BLOCK) dst[i] = src[i];
    }
}

// LDS ordering inside one wavefront: a wave's LDS operations complete in issue order, so a
// compiler-level fence is all that is needed between the writes of some lanes and the reads of
// others (no s_barrier).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Global memory ordering inside one wavefront: some lanes' stores before other lanes' loads of the same
// addresses.  A wavefront's vector memory operations go through one L1 in issue order; the workgroup-scope
// fences (a workgroup is one wavefront wherever this is used) also wait for the stores, which the rare paths
// that use it can afford.
__device__ __forceinline__ void wave_mem_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Wait until every vector memory operation the wavefront has issued is complete: s_waitcnt vmcnt(0) (the
// gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima).  vmcnt counts
// loads and stores in issue order, and the compiler places the wait a loaded register needs at its first use,
// with the count of the shortest path from the load to there.  In a loop that issues a load ahead of stores and
// uses it an iteration later, that shortest path is the loop's entry, where no store is in between: on the back
// edge the same count makes the use wait for the stores as well.  A caller that drains its loads explicitly
// before its stores, on every path into the use, leaves the compiler nothing to wait for there.
__device__ __forceinline__ void wave_vmem_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }

}  // namespace sng
