// sng_noise_host.h -- the action noise's contract (include/sng.h, sng_noise_create): the hash, the stream key, the
// standard normal variate and the two kinds' arithmetic, written once as host-and-device functions, so that
// action_noise_kernel (sng_noise.h) and the host model (noise_host_fill, sng_noise_host_fill) compile from the same
// text and agree bit for bit; and the checks of the sng_noise_* calls.  No HIP: it compiles with plain g++
// (tests/native/noise_host_check.cpp), where the qualifiers below are empty.  Must be compiled with -ffp-contract=off,
// as the library and its tests are.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "sng.h"

#if defined(__HIPCC__)
#define SNG_NOISE_HD __host__ __device__ __forceinline__
#else
#define SNG_NOISE_HD inline
#endif

namespace sng {

constexpr uint32_t kDomainNoise = 0x6e7a0000u;   // | action index j (< 256); apart from kDomainPV / Price / Ratio / Replay
constexpr int kNoiseMaxAct = 255;
constexpr int kNoiseOctaves = 31, kNoiseSubs = 4;

// "triple32", as sng_dev_env.h's mix32 and the oracle's: restated here so that the host model has it.
SNG_NOISE_HD uint32_t noise_mix32(uint32_t x) {
    x ^= x >> 17;
    x *= 0xed5ad4bbu;
    x ^= x >> 11;
    x *= 0xac4c1b51u;
    x ^= x >> 15;
    x *= 0x31848babu;
    x ^= x >> 14;
    return x;
}

// What (seed, counter) give every stream of a block: stream_key's first mix, with the counter's high word mixed in too.
SNG_NOISE_HD uint32_t noise_day_key(uint64_t seed, uint64_t c) {
    const uint32_t k0 = noise_mix32((uint32_t)seed ^ noise_mix32((uint32_t)(seed >> 32) + (uint32_t)c * 0x9e3779b9u));
    return noise_mix32(k0 ^ ((uint32_t)(c >> 32) * 0x85ebca6bu + 0x165667b1u));
}
// The stream key of (seed, global env ge, action j, counter c): all 64 bits of ge and of c enter it.
SNG_NOISE_HD uint32_t noise_key_of(uint32_t day_key, uint64_t ge, uint32_t j) {
    const uint32_t k1 = noise_mix32(day_key ^ (uint32_t)ge);
    return noise_mix32(k1 ^ ((uint32_t)(ge >> 32) * 0x85ebca6bu + (kDomainNoise | j) * 0xc2b2ae35u + 0x27d4eb2fu));
}
SNG_NOISE_HD uint32_t noise_key(uint64_t seed, uint64_t ge, uint32_t j, uint64_t c) {
    return noise_key_of(noise_day_key(seed, c), ge, j);
}
// Step t's hash of a stream.
SNG_NOISE_HD uint32_t noise_hash(uint32_t key, uint32_t t) { return noise_mix32(key + t * 0x9e3779b9u); }

// Where a hash's variate is in the table, and its fraction: u = max(h & 0x7fffffff, 1), octave k = 30 - msb(u), the bits
// below u's leading one left-aligned in a word w: its top 2 bits are the sub-segment, the next 24 the fraction x (exact
// in float32; the up to 4 bits below them are dropped: at most 16 neighbouring u of octave 0 share a variate, 1.2e-8
// apart in z).  Returns the segment's index k * 4 + s.
SNG_NOISE_HD int noise_segment(uint32_t h, float *x) {
    uint32_t u = h & 0x7fffffffu;
    u = u ? u : 1u;
    const int lz = __builtin_clz(u);   // 1 .. 31
    const uint32_t w = (u << lz) << 1;
    *x = (float)((w >> 6) & 0xffffffu) * 0x1.0p-24f;
    return (lz - 1) * kNoiseSubs + (int)(w >> 30);
}
// The variate from the segment's cubic c0 .. c3 (r ~ -ndtri(p), p = (u + 0.5) 2^-32 in (0, 0.5)): three fmaf, a floor
// that keeps r positive next to p = 0.5 (the true r there is 2.9e-10, below the cubic's error), and the sign bit.
SNG_NOISE_HD float noise_variate(uint32_t h, float x, float c0, float c1, float c2, float c3) {
    float r = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(c3, x, c2), x, c1), x, c0);
    r = r > 0x1.0p-32f ? r : 0x1.0p-32f;
    return (h >> 31) ? -r : r;
}

// f32 operations rounded one by one, whatever the compiler's contraction setting on the device.
SNG_NOISE_HD float noise_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
SNG_NOISE_HD float noise_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
SNG_NOISE_HD float noise_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
// SNG_NOISE_GAUSSIAN: n = mu + scale * z
SNG_NOISE_HD float noise_gaussian(float mu, float scale, float z) { return noise_add(mu, noise_mul(scale, z)); }
// SNG_NOISE_OU: one step of the process from x; sd = (float)(scale * sqrt(dt))
SNG_NOISE_HD float noise_ou_step(float x, float mu, float sd, float theta, float dt, float z) {
    return noise_add(noise_add(x, noise_mul(noise_mul(theta, noise_sub(mu, x)), dt)), noise_mul(sd, z));
}

// [octave][sub-segment][c0 c1 c2 c3]: tools/fit_noise_table.py
constexpr float kNoiseIcdf[kNoiseOctaves * kNoiseSubs * 4] = {
    0x1.595672p-1f, -0x1.92a7f4p-3f, 0x1.9f8bc4p-7f, -0x1.d3fb6ap-10f,   // octave 0
    0x1.f4819p-2f, -0x1.697ef4p-3f, 0x1.e8ff9ep-8f, -0x1.1ce7fap-10f,
    0x1.46494ap-2f, -0x1.5187acp-3f, 0x1.1724ecp-8f, -0x1.98282ep-11f,
    0x1.422c0ap-3f, -0x1.44d5aap-3f, 0x1.00739p-9f, -0x1.583b0ap-11f,
    0x1.267d2ap+0f, -0x1.36c456p-3f, 0x1.a72cbcp-7f, -0x1.9182f4p-10f,   // octave 1
    0x1.028ea8p+0f, -0x1.0b1a7ap-3f, 0x1.149a9ap-7f, -0x1.c4960cp-11f,
    0x1.c63804p-1f, -0x1.db7e3ap-4f, 0x1.82b9dap-8f, -0x1.1a5cdcp-11f,
    0x1.8d871ep-1f, -0x1.b1ad9cp-4f, 0x1.1a5b0cp-8f, -0x1.7b8702p-12f,
    0x1.88bcp+0f, -0x1.0412aep-3f, 0x1.8b64d4p-7f, -0x1.6f40bcp-10f,   // octave 2
    0x1.6af4b2p+0f, -0x1.b62f72p-4f, 0x1.055ea8p-7f, -0x1.9ae4a8p-11f,
    0x1.516922p+0f, -0x1.7e50e6p-4f, 0x1.73a412p-8f, -0x1.fb8ac8p-12f,
    0x1.3ad802p+0f, -0x1.55b93cp-4f, 0x1.15decap-8f, -0x1.504dd2p-12f,
    0x1.dcdbe2p+0f, -0x1.c66f2ap-4f, 0x1.6e6d84p-7f, -0x1.543f68p-10f,   // octave 3
    0x1.c2fcc8p+0f, -0x1.7a78ep-4f, 0x1.e48fbep-8f, -0x1.7b989ap-11f,
    0x1.ad0a5cp+0f, -0x1.46a726p-4f, 0x1.58fdep-8f, -0x1.d39adep-12f,
    0x1.99dbbp+0f, -0x1.20ee0cp-4f, 0x1.029c3p-8f, -0x1.34fbb8p-12f,
    0x1.13b21ep+1f, -0x1.97b8ecp-4f, 0x1.55059ap-7f, -0x1.3dc7cep-10f,   // octave 4
    0x1.0821a8p+1f, -0x1.5113eep-4f, 0x1.c22dbcp-8f, -0x1.61c28p-11f,
    0x1.fcc80cp+0f, -0x1.20f5dep-4f, 0x1.401f78p-8f, -0x1.b2f354p-12f,
    0x1.ebdda2p+0f, -0x1.fbefe4p-5f, 0x1.df8fdp-9f, -0x1.1eea32p-12f,
    0x1.357286p+1f, -0x1.7475c4p-4f, 0x1.3f6046p-7f, -0x1.2acb86p-10f,   // octave 5
    0x1.2ae8e4p+1f, -0x1.325a7ap-4f, 0x1.a4c442p-8f, -0x1.4c027ap-11f,
    0x1.2213b6p+1f, -0x1.056926p-4f, 0x1.2ab802p-8f, -0x1.978e1ep-12f,
    0x1.1a710cp+1f, -0x1.c98e3ap-5f, 0x1.bee2bap-9f, -0x1.0c764ap-12f,
    0x1.547d0cp+1f, -0x1.58b148p-4f, 0x1.2ced44p-7f, -0x1.1a8f8ap-10f,   // octave 6
    0x1.4ac122p+1f, -0x1.1a7388p-4f, 0x1.8bbbdcp-8f, -0x1.397946p-11f,
    0x1.429fcep+1f, -0x1.e06b9cp-5f, 0x1.188264p-8f, -0x1.804636p-12f,
    0x1.3b9e6p+1f, -0x1.a32b32p-5f, 0x1.a3137ap-9f, -0x1.f9a388p-13f,
    0x1.715c7p+1f, -0x1.4221a6p-4f, 0x1.1d1308p-7f, -0x1.0c8628p-10f,   // octave 7
    0x1.6846eap+1f, -0x1.073524p-4f, 0x1.76493cp-8f, -0x1.297f6ap-11f,
    0x1.60b5dp+1f, -0x1.be8ed6p-5f, 0x1.08f11p-8f, -0x1.6c432p-12f,
    0x1.5a34acp+1f, -0x1.84bc5cp-5f, 0x1.8b571cp-9f, -0x1.decef8p-13f,
    0x1.8c7344p+1f, -0x1.2f5a5cp-4f, 0x1.0f5174p-7f, -0x1.004306p-10f,   // octave 8
    0x1.83e7cp+1f, -0x1.ee9bb2p-5f, 0x1.63bb8ap-8f, -0x1.1b94f8p-11f,
    0x1.7ccd78p+1f, -0x1.a2bf5ap-5f, 0x1.f704b2p-9f, -0x1.5adfc2p-12f,
    0x1.76b566p+1f, -0x1.6be1bp-5f, 0x1.76e768p-9f, -0x1.c78be4p-13f,
    0x1.a60a64p+1f, -0x1.1f6baap-4f, 0x1.0343a6p-7f, -0x1.eae5b6p-11f,   // octave 9
    0x1.9df3ap+1f, -0x1.d3c68cp-5f, 0x1.5386p-8f, -0x1.0f57cep-11f,
    0x1.973d56p+1f, -0x1.8b6714p-5f, 0x1.df9b52p-9f, -0x1.4b9d9cp-12f,
    0x1.917d44p+1f, -0x1.571c54p-5f, 0x1.652208p-9f, -0x1.b32c82p-13f,
    0x1.be5962p+1f, -0x1.11b0cep-4f, 0x1.f1364cp-8f, -0x1.d7aa2ep-11f,   // octave 10
    0x1.b6a7p+1f, -0x1.bcc2ap-5f, 0x1.453af8p-8f, -0x1.047c0cp-11f,
    0x1.b0464ep+1f, -0x1.7775b6p-5f, 0x1.cb02a2p-9f, -0x1.3e1b14p-12f,
    0x1.aad148p+1f, -0x1.456e22p-5f, 0x1.5587c2p-9f, -0x1.a12afap-13f,
    0x1.d58bc4p+1f, -0x1.05b47cp-4f, 0x1.de358ap-8f, -0x1.c66e5cp-11f,   // octave 11
    0x1.ce30dap+1f, -0x1.a8bf3ep-5f, 0x1.388516p-8f, -0x1.f58cf4p-12f,
    0x1.c81a74p+1f, -0x1.662d2ep-5f, 0x1.b8bb98p-9f, -0x1.320c3p-12f,
    0x1.c2e65ep+1f, -0x1.362728p-5f, 0x1.47b5a6p-9f, -0x1.911f5p-13f,
    0x1.ebc456p+1f, -0x1.f64152p-5f, 0x1.cd24c8p-8f, -0x1.b6e226p-11f,   // octave 12
    0x1.e4b678p+1f, -0x1.9724bep-5f, 0x1.2d216cp-8f, -0x1.e410bp-12f,
    0x1.dee158p+1f, -0x1.570462p-5f, 0x1.a862c6p-9f, -0x1.27351ep-12f,
    0x1.d9e626p+1f, -0x1.28c958p-5f, 0x1.3b5e72p-9f, -0x1.82b7d8p-13f,
    0x1.008fb2p+2f, -0x1.e3695ep-5f, 0x1.bdb78p-8f, -0x1.a8c55ap-11f,   // octave 13
    0x1.fa5614p+1f, -0x1.8781f6p-5f, 0x1.22daf2p-8f, -0x1.d43896p-12f,
    0x1.f4bad8p+1f, -0x1.4995b4p-5f, 0x1.99a9a6p-9f, -0x1.1d6636p-12f,
    0x1.eff202p+1f, -0x1.1cf7ccp-5f, 0x1.30453ap-9f, -0x1.75b3acp-13f,
    0x1.0ada2ep+2f, -0x1.d27dc8p-5f, 0x1.afb022p-8f, -0x1.9be3dcp-11f,   // octave 14
    0x1.07944p+2f, -0x1.798094p-5f, 0x1.198728p-8f, -0x1.c5c844p-12f,
    0x1.04e08cp+2f, -0x1.3d940cp-5f, 0x1.8c5176p-9f, -0x1.14790ep-12f,
    0x1.02929cp+2f, -0x1.126c6p-5f, 0x1.26397ap-9f, -0x1.69de9cp-13f,
    0x1.14cb66p+2f, -0x1.c330d2p-5f, 0x1.a2dc82p-8f, -0x1.9012cap-11f,   // octave 15
    0x1.11a13ep+2f, -0x1.6cdd6ap-5f, 0x1.110392p-8f, -0x1.b88e3cp-12f,
    0x1.0f04e2p+2f, -0x1.32c3b6p-5f, 0x1.802778p-9f, -0x1.0c4e4cp-12f,
    0x1.0ccb3p+2f, -0x1.08f0fcp-5f, 0x1.1d140ap-9f, -0x1.5f0e2ep-13f,
    0x1.1e6ba8p+2f, -0x1.b54484p-5f, 0x1.971316p-8f, -0x1.852e38p-11f,   // octave 16
    0x1.1b5abcp+2f, -0x1.61633cp-5f, 0x1.0933c6p-8f, -0x1.ac6146p-12f,
    0x1.18d392p+2f, -0x1.28f59ep-5f, 0x1.75020cp-9f, -0x1.04cbecp-12f,
    0x1.16ac34p+2f, -0x1.005b2ap-5f, 0x1.14b4e8p-9f, -0x1.551f4p-13f,
    0x1.27c206p+2f, -0x1.a8868ap-5f, 0x1.8c30b8p-8f, -0x1.7b172cp-11f,   // octave 17
    0x1.24c82ep+2f, -0x1.56e716p-5f, 0x1.01ffeep-8f, -0x1.a11e32p-12f,
    0x1.22545cp+2f, -0x1.2003f8p-5f, 0x1.6abe6ep-9f, -0x1.fbb7cp-13f,
    0x1.203db6p+2f, -0x1.f111e2p-6f, 0x1.0d017cp-9f, -0x1.4bf43cp-13f,
    0x1.30d498p+2f, -0x1.9ccd0cp-5f, 0x1.82168p-8f, -0x1.71b19cp-11f,   // octave 18
    0x1.2deff6p+2f, -0x1.4d458ap-5f, 0x1.f6a6bep-9f, -0x1.96a5b2p-12f,
    0x1.2b8de6p+2f, -0x1.17cfc4p-5f, 0x1.613ed2p-9f, -0x1.eed596p-13f,
    0x1.298692p+2f, -0x1.e2bd32p-6f, 0x1.05e31ep-9f, -0x1.43735ap-13f,
    0x1.39a898p+2f, -0x1.91f3e6p-5f, 0x1.78a77p-8f, -0x1.68e1d6p-11f,   // octave 19
    0x1.36d796p+2f, -0x1.44607p-5f, 0x1.ea365ap-9f, -0x1.8cd9c8p-12f,
    0x1.3485e8p+2f, -0x1.103ee8p-5f, 0x1.58685ep-9f, -0x1.e2cd06p-13f,
    0x1.328cb2p+2f, -0x1.d589eep-6f, 0x1.fe8b56p-10f, -0x1.3b84dap-13f,
    0x1.42428cp+2f, -0x1.87d9d8p-5f, 0x1.6fc51ap-8f, -0x1.60888ap-11f,   // octave 20
    0x1.3f83c6p+2f, -0x1.3c1cb8p-5f, 0x1.de8888p-9f, -0x1.839a04p-12f,
    0x1.3d415p+2f, -0x1.093a56p-5f, 0x1.5020d2p-9f, -0x1.d7781ap-13f,
    0x1.3b5532p+2f, -0x1.c94facp-6f, 0x1.f22bcp-10f, -0x1.34108ap-13f,
    0x1.4aa636p+2f, -0x1.7e5cd4p-5f, 0x1.674a2p-8f, -0x1.587bd2p-11f,   // octave 21
    0x1.47f88cp+2f, -0x1.345fbap-5f, 0x1.d370d8p-9f, -0x1.7abd18p-12f,
    0x1.45c452p+2f, -0x1.02ac04p-5f, 0x1.484acep-9f, -0x1.cca872p-13f,
    0x1.43e46ap+2f, -0x1.bde89cp-6f, 0x1.e67dccp-10f, -0x1.2cf9e8p-13f,
    0x1.52d694p+2f, -0x1.75540ep-5f, 0x1.5f0052p-8f, -0x1.507a64p-11f,   // octave 22
    0x1.50392ap+2f, -0x1.2d0b3ap-5f, 0x1.c8b1fp-9f, -0x1.72053ap-12f,
    0x1.4e1262p+2f, -0x1.f8f7e6p-6f, 0x1.40bf84p-9f, -0x1.c21b2ap-13f,
    0x1.4c3dfep+2f, -0x1.b32ceep-6f, 0x1.db4c64p-10f, -0x1.261924p-13f,
    0x1.5ad592p+2f, -0x1.6c8596p-5f, 0x1.568e32p-8f, -0x1.48137ep-11f,   // octave 23
    0x1.5847ecp+2f, -0x1.25f68p-5f, 0x1.bde9fap-9f, -0x1.690a38p-12f,
    0x1.562e18p+2f, -0x1.ed1688p-6f, 0x1.3943p-9f, -0x1.b7621cp-13f,
    0x1.5464bcp+2f, -0x1.a8eb54p-6f, 0x1.d0480cp-10f, -0x1.1f2e2cp-13f,
    0x1.62a386p+2f, -0x1.63934ep-5f, 0x1.4d54cap-8f, -0x1.3e7aa4p-11f,   // octave 24
    0x1.6025c4p+2f, -0x1.1ee1cep-5f, 0x1.b26e1p-9f, -0x1.5f10e2p-12f,
    0x1.5e18d2p+2f, -0x1.e15692p-6f, 0x1.316e72p-9f, -0x1.abb982p-13f,
    0x1.5c5a52p+2f, -0x1.9edba4p-6f, 0x1.c4eadp-10f, -0x1.17c876p-13f,
    0x1.6a3e0ap+2f, -0x1.59d838p-5f, 0x1.4232e6p-8f, -0x1.323ac4p-11f,   // octave 25
    0x1.67d156p+2f, -0x1.175f64p-5f, 0x1.a50824p-9f, -0x1.52c2eap-12f,
    0x1.65d1eep+2f, -0x1.d51a4cp-6f, 0x1.288848p-9f, -0x1.9dbb92p-13f,
    0x1.641eaap+2f, -0x1.94865p-6f, 0x1.b844a4p-10f, -0x1.0f1ac4p-13f,
    0x1.719ddcp+2f, -0x1.4e2d42p-5f, 0x1.33248ap-8f, -0x1.20c3a4p-11f,   // octave 26
    0x1.6f4546p+2f, -0x1.0eab2p-5f, 0x1.9388fep-9f, -0x1.41bc92p-12f,
    0x1.6d555ap+2f, -0x1.c7492ep-6f, 0x1.1d3ffap-9f, -0x1.8ae2a8p-13f,
    0x1.6baea2p+2f, -0x1.891818p-6f, 0x1.a8a116p-10f, -0x1.03b07ep-13f,
    0x1.78b322p+2f, -0x1.3e9356p-5f, 0x1.1cd39cp-8f, -0x1.06036cp-11f,   // octave 27
    0x1.767502p+2f, -0x1.036bb6p-5f, 0x1.7a35c2p-9f, -0x1.280b18p-12f,
    0x1.7498d2p+2f, -0x1.b5f0e4p-6f, 0x1.0d4b5ep-9f, -0x1.6ee7cp-13f,
    0x1.7301acp+2f, -0x1.7b17f8p-6f, 0x1.92fdbcp-10f, -0x1.e60c1ep-14f,
    0x1.7f5fe2p+2f, -0x1.27ebb4p-5f, 0x1.f5507ep-9f, -0x1.b9f5c4p-12f,   // octave 28
    0x1.7d47cep+2f, -0x1.e6db2ep-6f, 0x1.53849ap-9f, -0x1.004e82p-12f,
    0x1.7b8762p+2f, -0x1.9dcd6ep-6f, 0x1.ea3292p-10f, -0x1.439474p-13f,
    0x1.7a05bp+2f, -0x1.680196p-6f, 0x1.7281dep-10f, -0x1.b29446p-14f,
    0x1.857258p+2f, -0x1.066802p-5f, 0x1.91dc4cp-9f, -0x1.46f67ap-12f,   // octave 29
    0x1.8392aap+2f, -0x1.b76aa2p-6f, 0x1.19bf46p-9f, -0x1.8d0684p-13f,
    0x1.81fb5cp+2f, -0x1.7a25d6p-6f, 0x1.a0e89ep-10f, -0x1.030a3p-13f,
    0x1.80994p+2f, -0x1.4c0688p-6f, 0x1.40f1dap-10f, -0x1.64b2p-14f,
    0x1.8aa6c8p+2f, -0x1.afe804p-6f, 0x1.152afcp-9f, -0x1.86b3f8p-13f,   // octave 30
    0x1.891678p+2f, -0x1.73a2e6p-6f, 0x1.9a15d8p-10f, -0x1.fdc6a8p-14f,
    0x1.87ba78p+2f, -0x1.46455cp-6f, 0x1.3ba8fp-10f, -0x1.5ef21ep-14f,
    0x1.86868ep+2f, -0x1.22e09p-6f, 0x1.f4ff8ep-11f, -0x1.f7cabap-15f,
};

// Host side of a variate: the table read where the kernel reads its LDS copy.
inline float noise_z_host(uint32_t h) {
    float x;
    const float *c = kNoiseIcdf + 4 * noise_segment(h, &x);
    return noise_variate(h, x, c[0], c[1], c[2], c[3]);
}

// The per-action parameters as the kernel reads them: mu [A], then sd [A] -- scale for the Gaussian kind, and
// (float)(scale * sqrt(dt)), formed in double, for the OU kind.  mu null: zeros.
inline void noise_pack_params(const SngNoiseSpec &spec, const float *mu, const float *scale, float *params) {
    const int A = spec.act_dim;
    for (int j = 0; j < A; ++j) {
        params[j] = mu ? mu[j] : 0.f;
        const float s = scale ? scale[j] : 0.f;
        params[A + j] = spec.kind == SNG_NOISE_OU ? (float)((double)s * std::sqrt(spec.dt)) : s;
    }
}

// SNG_OK, or SNG_ERR_INVALID_ARGUMENT with `why` naming the value: a spec (env_act_dim 0: any act_dim in range).
inline int noise_spec_check(const SngNoiseSpec *spec, int env_act_dim, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!spec) return no("null noise spec");
    if (spec->kind != SNG_NOISE_GAUSSIAN && spec->kind != SNG_NOISE_OU)
        return no("noise kind " + std::to_string(spec->kind) + " is neither SNG_NOISE_GAUSSIAN (0) nor SNG_NOISE_OU (1)");
    if (spec->act_dim < 1 || spec->act_dim > kNoiseMaxAct)
        return no("noise act_dim " + std::to_string(spec->act_dim) + " is outside 1 .. 255");
    if (env_act_dim && spec->act_dim != env_act_dim)
        return no("noise act_dim " + std::to_string(spec->act_dim) + " is not the env's " + std::to_string(env_act_dim));
    if (!std::isfinite(spec->theta)) return no("noise theta " + std::to_string(spec->theta) + " is not finite");
    if (!std::isfinite(spec->dt)) return no("noise dt " + std::to_string(spec->dt) + " is not finite");
    if (spec->kind == SNG_NOISE_OU && spec->dt < 0.0) return no("noise dt " + std::to_string(spec->dt) + " is negative");
    return SNG_OK;
}
// ... and the per-action parameters: scale is required, finite and not negative; mu finite or null.
inline int noise_params_check(int A, const float *mu, const float *scale, std::string *why) {
    auto no = [&](const std::string &msg) {
        if (why) *why = msg;
        return (int)SNG_ERR_INVALID_ARGUMENT;
    };
    if (!scale) return no("null noise scale");
    for (int j = 0; j < A; ++j) {
        if (mu && !std::isfinite(mu[j])) return no("noise mu[" + std::to_string(j) + "] = " + std::to_string(mu[j]) + " is not finite");
        if (!std::isfinite(scale[j]))
            return no("noise scale[" + std::to_string(j) + "] = " + std::to_string(scale[j]) + " is not finite");
        if (scale[j] < 0.f) return no("noise scale[" + std::to_string(j) + "] = " + std::to_string(scale[j]) + " is negative");
    }
    return SNG_OK;
}

// The host model: `days` blocks [T][E][A] of counters counter, counter + 1, .. for global envs env_offset + e, from the
// packed parameters.  The loops are the kernel's, one element after another.
inline void noise_host_fill(const SngNoiseSpec &spec, const float *params, int32_t T, int64_t E, int64_t env_offset,
                            uint64_t counter, int32_t days, float *out) {
    const int A = spec.act_dim;
    const float theta = (float)spec.theta, dt = (float)spec.dt;
    const size_t row = (size_t)E * (size_t)A;
    for (int32_t d = 0; d < days; ++d) {
        const uint32_t dk = noise_day_key(spec.seed, counter + (uint64_t)d);
        float *block = out + (size_t)d * (size_t)T * row;
        for (int64_t e = 0; e < E; ++e)
            for (int j = 0; j < A; ++j) {
                const uint32_t key = noise_key_of(dk, (uint64_t)(env_offset + e), (uint32_t)j);
                const float mu = params[j], sd = params[A + j];
                float x = 0.f;
                for (int32_t t = 0; t < T; ++t) {
                    const float z = noise_z_host(noise_hash(key, (uint32_t)t));
                    x = spec.kind == SNG_NOISE_OU ? noise_ou_step(x, mu, sd, theta, dt, z) : noise_gaussian(mu, sd, z);
                    block[(size_t)t * row + (size_t)e * (size_t)A + (size_t)j] = x;
                }
            }
    }
}

}  // namespace sng
