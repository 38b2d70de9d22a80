// sng_generate.h -- resets on the device: the counter-hash draws, the t = 0 observation kernel
// (observe0_kernel), the profile keys (profile_kernel) and the device-RNG day generator with its fused t = 0
// observation blocks (generate_kernel, observe_day0).
// Needs sng_mt.h (a reference-RNG env's Python stream, py_ratio_lane; mt_twist_lane is defined in
// sng_ref_day.h), sng_dev_util.h (buffer stores, copy_out, soc_off) and sng_dev_env.h (write_obs_header,
// stream_key, profile factors, departure_obs).  Included by sng_kernels.hip only.
#pragma once

namespace sng {

// ---------------------------------------------------------------------------------
// Counter-based draws shared by the device generator and the t = 0 observation kernels: draw i
// of a stream is mix32(key + i * golden), three 32-bit multiplies (the earlier 64-bit SplitMix
// streams cost ~4x the VALU; the generator is bound by its dense timeline stores otherwise).
// ---------------------------------------------------------------------------------
struct HashStream {
    uint32_t key, ctr;
    __device__ __forceinline__ uint32_t next() { return mix32(key + (ctr++) * 0x9e3779b9u); }
};

__device__ __forceinline__ double u32_unit(uint32_t x) { return (double)x * 0x1.0p-32; }   // [0, 1)

__device__ __forceinline__ int below(uint32_t x, int n) {   // floor(x * n / 2^32)
    return (int)(((uint64_t)x * (uint64_t)n) >> 32);
}

constexpr uint32_t kDomainRatio = 0x7a710000u;    // a generated day's PV ratio
constexpr uint32_t kDomainReplay = 0x7a720000u;   // the PV ratio of a replayed day

// random.randint(0, 180) / 100 (smart_nanogrid_environment.py:349) of device day `day`
__device__ __forceinline__ double pv_ratio_draw(uint64_t seed, uint64_t ge, uint64_t day) {
    HashStream r2{stream_key(seed, ge, kDomainRatio, day), 0u};
    return (double)below(r2.next(), 181) / 100;
}

// The ratio a replayed device day redraws (reset(generate_new_initial_values=False) redraws
// random_pv_shift_ratio, smart_nanogrid_environment.py:347-349): replay number `replay` of the handle.
__device__ __forceinline__ double replay_ratio_draw(uint64_t seed, uint64_t ge, uint64_t replay) {
    HashStream r2{stream_key(seed, ge, kDomainReplay, replay), 0u};
    return (double)below(r2.next(), 181) / 100;
}

// ---------------------------------------------------------------------------------
// One env's Python `random` stream (RefStreams, tempered words, two blocks) on its lane: the day-end
// random.randint(0, 180) the last step owes (end_draw; smart_nanogrid_environment.py:181) and the
// reset's random.randint(0, 180) / 100 (draw; :349) -- _randbelow(181) as getrandbits(8) rejection.
// A block boundary without a ready successor is twisted on the lane (mt_twist_lane).  Returns the
// ratio (or `keep` when nothing is drawn) and stores the stream's new position.
// ---------------------------------------------------------------------------------
__device__ __noinline__ void mt_twist_lane(const uint32_t *A, uint32_t *B);
__device__ __forceinline__ double py_ratio_lane(const RefStreams &ps, int64_t e, bool end_draw, bool draw,
                                                double keep) {
    uint32_t *blk = ps.mt + (size_t)e * 2 * kMtN;
    const int32_t pos = ps.pos[e];
    int cur = (pos >> 16) & 1, mti = pos & kMtPosMask;
    bool ready = (pos & kMtNextReady) != 0;
    auto next = [&]() -> uint32_t {
        if (mti >= kMtN) {
            if (!ready) mt_twist_lane(blk + cur * kMtN, blk + (cur ^ 1) * kMtN);
            cur ^= 1;
            mti -= kMtN;
            ready = false;
        }
        return blk[cur * kMtN + mti++];   // tempered in HBM
    };
    auto randint180 = [&]() -> int {
        uint32_t r;
        do {
            r = next() >> 24;
        } while (r >= 181u);
        return (int)r;
    };
    if (end_draw) (void)randint180();
    const double ratio = draw ? (double)randint180() / 100 : keep;
    ps.pos[e] = (cur << 16) | (ready ? kMtNextReady : 0) | mti;
    return ratio;
}

// ---------------------------------------------------------------------------------
// Observation at t = 0 after a reset (SmartNanogridEnv.reset -> __get_observations,
// smart_nanogrid_environment.py:349-351): SOC[c, 0] as generated, departure times at 0.
// mode (Obs0Mode, sng_layout.h) says where the PV ratio comes from and who advances the day
// counter; replay = the handle's replay number (OBS0_REPLAY of a device day), else -1.
// ---------------------------------------------------------------------------------
template <int BLOCK, bool PK>
__global__ __launch_bounds__(BLOCK) void observe0_kernel(Params p, DeviceState s, float *__restrict__ obs,
                                                         double *__restrict__ ep_return, int64_t E, int vec_io,
                                                         int mode, int64_t replay, RefStreams ps, int py) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = p.n, O = p.obs_dim;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * BLOCK;
    const int nblk = (int)((E - e0) < BLOCK ? (E - e0) : BLOCK);
    const int64_t e = e0 + tid;
    float *o_row = lds + tid * O;
    if (tid < nblk) {
        const uint64_t ge = (uint64_t)(e + p.env_offset);
        double ratio;
        if (py) {   // reference-RNG days: the Python stream's draws (py bit 0: the ratio, bit 1: the day-end draw)
            ratio = py_ratio_lane(ps, e, (py & 2) != 0, (py & 1) != 0, 0.0);
            if (py & 1)
                s.ratio[e] = ratio;
            else
                ratio = s.ratio[e];
        } else if (mode == OBS0_DEVICE) {   // the day's draw, as the fused generator's t = 0 blocks make it
            ratio = pv_ratio_draw(p.seed, ge, *s.episode);
            s.ratio[e] = ratio;
        } else if (mode == OBS0_REPLAY && replay >= 0) {
            ratio = replay_ratio_draw(p.seed, ge, (uint64_t)replay);
            s.ratio[e] = ratio;
        } else {
            ratio = s.ratio[e];
        }
        // a generated day's python index -1 slot holds zeros; a replayed day's Requested_SOC is 0
        if (mode != OBS0_HOST) s.pen0[e] = 0.0;   // OBS0_GENERATED included
        double fpv[4] = {1.0, 1.0, 1.0, 1.0}, fpr[4] = {1.0, 1.0, 1.0, 1.0};
        if (p.noise) profile_factors(p, s, (uint32_t)e * 8u, 0, fpv, fpr);
        write_obs_header(o_row, p, s.tables->irr_norm, s.tables->price_norm, ratio, fpv, fpr);
        const int k = p.pv ? 8 : 4;
        const uint32_t *__restrict__ word = s.word;
        const double *__restrict__ auxv = s.aux;
        double *__restrict__ socv = s.soc;
        // batches of 16 chargers: all loads of a batch issued before its stores (t = 0 slice); a packed
        // day's two planes are both loaded up front (the plane-0 record is used only where plane 1 is
        // occupied), so a batch is one memory round trip (config-5 reset 293 -> 257 us, A/B)
        constexpr int B = 16;
        for (int c0 = 0; c0 < n; c0 += B) {
            uint32_t w[B];
            double aux[B];
            if (PK) {   // packed device-day records (sng_layout.h): t = 0 is plane 1; plane 0 carries
                        // the SoC of the t = 0 arrivals
                const uint16_t *rec = packed_records(s);
                uint32_t r0[B], r1[B];
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const int c = c0 + j < n ? c0 + j : n - 1;
                    const size_t ri = rec_index(c, e, n, E);   // charger quads (sng_layout.h)
                    r1[j] = rec[(size_t)n * E + ri];
                    r0[j] = rec[ri];
                }
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    w[j] = (r1[j] & W_OCC) ? r1[j] : 0u;   // an empty charger's record carries a SoC, not a departure
                    aux[j] = (r1[j] & W_OCC) ? (double)rec_soc(r0[j]) : 0.0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const int c = c0 + j < n ? c0 + j : n - 1;
                    w[j] = word[(size_t)c * E + e];
                    aux[j] = auxv[(size_t)c * E + e];
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int c = c0 + j;
                if (c < n) {
                    // the SoC state in charger pairs (sng_layout.h): one 16 B store per pair (c0 is even)
                    if (c + 1 < n && !(j & 1))
                        bst2<kNT>(socv, (uint32_t)soc_index(c, e, n, E) * 8u, aux[j], aux[j + 1 < B ? j + 1 : j]);
                    else if (c + 1 == n && !(j & 1))
                        bst<kNT>(socv, (uint32_t)soc_index(c, e, n, E) * 8u, aux[j]);
                    o_row[k + c] = (float)aux[j];
                    o_row[k + n + c] = departure_obs<PK>(w[j]);
                }
            }
        }
        if (p.bess) o_row[O - 1] = (float)s.bess[e];
        if (ep_return) ep_return[e] = 0.0;
    }
    // a host day: profile_kernel read the counter for this day's factors, so the next day draws the
    // next value (a device day's counter is advanced by its first step; a replay keeps its day's)
    if ((mode == OBS0_HOST || mode == OBS0_GENERATED) && blockIdx.x == 0 && tid == 0) *s.episode += 1;
    __syncthreads();
    copy_out<BLOCK>(obs + e0 * O, lds, nblk * O, vec_io != 0, tid);
}

// ---------------------------------------------------------------------------------
// Stochastic PV / price profiles of the day (build-defined, SngConfig.pv_noise / price_noise): the env's
// day keys prof_key[e] = {PV key, price key}, from which the step and observation kernels expand the factor
// of entry k (profile_factor_key).  Runs in every reset before observe0_kernel, which advances the day
// counter it reads.  Thread = env.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void profile_kernel(Params p, DeviceState s, int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint64_t day = *s.episode;
    const uint64_t env_seed = p.seed + (uint64_t)p.env_offset + (uint64_t)e;
    s.prof_key[2 * e] = stream_key(env_seed, 0, kDomainPV, day);
    s.prof_key[2 * e + 1] = stream_key(env_seed, 0, kDomainPrice, day);
}

// ---------------------------------------------------------------------------------
// Device RNG day generator: the reference's per-charger vehicle process
// (charging_station.py:200-279: arrival with p = 0.4 when the charger is free, arrival SoC
// U(0.1, 0.9), capacity U{15..119}, requested SoC, departure U{t+4/dt .. min(t+10/dt, T+1/dt)-1})
// with counter-based 32-bit hash streams (HashStream), one per (global env, charger, day).
// Thread = (env, charger); writes the dense packed-record (/ req) timeline.
// ---------------------------------------------------------------------------------
// An arrival happens iff round(rand() - 0.1) == 1, i.e. rand() > 0.6 (p = 0.4) at each free step.

constexpr int kGenBlock = 256;       // 4 waves of consecutive envs, same charger
// vehicles per charger and day: each stays >= 4/dt steps and leaves one empty step, so at most
// T / (4/dt + 1) + 1 <= 7 (checked on the host); slots for 8
constexpr int kDayVehicles = 8;
constexpr float kInvLog2Q = -1.3569154488567239f;   // 1 / log2(0.6)

// LDS slots per thread: the list's kDayVehicles entries and one more, which phase 2's look-ahead may
// read (never use) once the walk has reached the sentinel in slot 7
constexpr int kDaySlots = kDayVehicles + 1;
__host__ __device__ constexpr size_t generate_lds_bytes(bool with_req) {
    return (size_t)kDaySlots * kGenBlock * (sizeof(uint32_t) + sizeof(float) + (with_req ? sizeof(double) : 0));
}

// One vehicle's draws (charging_station.py:257-279), in stream order: the geometric wait from
// tfree to the arrival, arrival SoC, capacity + departure, requested SoC.  Phase 1 below and the
// t = 0 observation blocks share it, so both see the same first vehicle.
// Two 32-bit draws per vehicle (three with requested SoC), from a two-multiply hash (GenStream):
// the generator is bound by the VALU it issues (18.4 us for ~1,000 VALU per (env, charger) thread
// at 65,536 x 10), and the draws were a third of it.  x1's top 24 bits give the geometric wait, x2's
// top 24 bits the SoC (a float32 value in [0.1f, 0.9f], computed in float), and the 16 low bits of
// the two drive capacity (floor(r * 105 / 2^16)) and, through the low half of r * 105 (a bijection
// of r, as 105 is odd), the departure.
struct VehicleDraw {
    int ta, dep;
    uint32_t cap;
    double soc;          // code_soc(code)
    uint32_t req_draw;
    uint32_t code;       // the arrival SoC's 13-bit code (sng_layout.h)
};
__device__ __forceinline__ uint32_t mix32_gen(uint32_t x) {   // "lowbias32" (two multiplies, bijective)
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
struct GenStream {
    uint32_t key, ctr;
    __device__ __forceinline__ uint32_t next() { return mix32_gen(key + (ctr++) * 0x9e3779b9u); }
};
// Stream key of (seed, global env, charger, day) for the generator: one hash per (env, charger) over the
// index ge * 128 + c (unique for ge < 2^25 and c < 128, the ABI's maximum station), the day's seed hash k0
// offset by ge >> 25 beyond that.  k0 is wave-uniform (scalar).
__device__ __forceinline__ uint32_t gen_key(uint64_t seed, uint64_t ge, uint32_t c, uint64_t day) {
    const uint32_t k0 = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + (uint32_t)day * 0x9e3779b9u));
    return mix32((k0 + (uint32_t)(ge >> 25) * 0x85ebca6bu) ^ (((uint32_t)ge << 7) | c));
}
__device__ __forceinline__ VehicleDraw draw_vehicle(const Params &p, GenStream &rng, int tfree, int i4, int i10,
                                                    int i1) {
    VehicleDraw d;
    const uint32_t x1 = rng.next(), x2 = rng.next();
    const float u = ((float)(x1 >> 8) + 1.0f) * 0x1.0p-24f;   // (0, 1]
    d.ta = tfree + (int)(__log2f(u) * kInvLog2Q);               // floor: the product is >= 0
    // uniform(0.1, 0.9) on 8,192 float32 values (the packed record holds the code, sng_layout.h code_soc)
    d.code = x2 >> (32 - kSocCodeBits);
    d.soc = (double)code_soc(d.code);
    const uint32_t r = ((x1 & 0xffu) << 8) | (x2 & 0xffu);
    const uint32_t rc = r * 105u;
    d.cap = p.diff_caps ? 15u + (rc >> 16) : 40u;   // randint(15, 120)
    const uint32_t yd = (p.diff_caps ? rc : r) & 0xffffu;
    const int hi_c = d.ta + i10, hi_d = p.T + i1;
    const int high = hi_c < hi_d ? hi_c : hi_d;
    const int low = d.ta + i4;
    d.dep = (low >= high) ? low : low + (int)(__umul24(yd, (uint32_t)(high - low)) >> 16);   // 16 x 8 bits
    d.req_draw = p.req_enabled ? rng.next() : 0u;
    return d;
}

// The t = 0 observation of a device-RNG day, computed from the streams rather than read back from
// the timeline, so it runs as extra blocks of the generator's grid with no dependency on the
// timeline blocks (SmartNanogridEnv.reset -> __get_observations, smart_nanogrid_environment.py:
// 349-351): each charger's first vehicle, if it arrives at t = 0, gives SOC[c, 0] and the
// departure entry; the PV ratio, the day's profile factors, the header and the BESS entry; the
// running SoC is seeded and the day return zeroed.  64 envs per block, lane = env, and the block's
// four wavefronts split the row: wavefront 0 the header (PV ratio, profile factors, BESS entry),
// wavefronts 1-3 the chargers round-robin; profile entries go to all four.  Grid rows y = N .. N + 3
// cover a timeline block's 256 envs.  A thread's work is then a few vehicles, like a timeline
// thread's, instead of the whole station (one thread per env ran ~10x longer and finished last),
// no wavefront runs the header under a mask, and the 64-row tile (7.4 KB at N = 10) no longer caps
// the grid at 5 workgroups per CU.
constexpr int kObsParts = kGenBlock / kWave;       // wavefronts per observation block (threads per env)
constexpr int kObsEnvs = kGenBlock / kObsParts;    // envs per observation block
constexpr int kObsBlocks = kGenBlock / kObsEnvs;   // observation blocks per 256 envs
static_assert(kObsEnvs == kGenObsEnvs, "generator_fused (sng_graph_form.h) sizes the observation tile");
// obs == nullptr (the overlapped reset of a captured graph, sng_graph.cpp): the day's values are written -- ratio,
// pen0, the profile keys, the SoC seed, the zeroed return -- and the row is not: step 0 overwrites it before a
// caller could read it, and neither the observation buffer nor the BESS state is touched, which the day being
// stepped beside this generator owns.
__device__ __forceinline__ void observe_day0(const Params &p, const DeviceState &s, uint64_t seed, int64_t E, int i4,
                                             int i10, int i1, uint64_t day, float *__restrict__ obs,
                                             double *__restrict__ ep_return, int vec_io, float *lds, int q) {
    const int n = p.n, O = p.obs_dim;
    const int tid = threadIdx.x, part = __builtin_amdgcn_readfirstlane(tid / kWave), le = tid % kWave;
    const int64_t e0 = (int64_t)blockIdx.x * kGenBlock + (int64_t)q * kObsEnvs;
    if (e0 >= E) return;   // the whole block (before any barrier)
    const int nblk = (int)((E - e0) < kObsEnvs ? (E - e0) : kObsEnvs);
    const int64_t e = e0 + le;
    float *o_row = lds + le * O;
    if (le < nblk) {
        const uint64_t ge = (uint64_t)(e + p.env_offset);
        const uint64_t env_seed = p.seed + (uint64_t)p.env_offset + (uint64_t)e;
        if (p.noise && part == 0) {   // the day's profile keys (profile_kernel's)
            s.prof_key[2 * e] = stream_key(env_seed, 0, kDomainPV, day);
            s.prof_key[2 * e + 1] = stream_key(env_seed, 0, kDomainPrice, day);
        }
        if (part == 0) {
            const double ratio = pv_ratio_draw(seed, ge, day);
            s.ratio[e] = ratio;
            s.pen0[e] = 0.0;
            double fpv[4] = {1.0, 1.0, 1.0, 1.0}, fpr[4] = {1.0, 1.0, 1.0, 1.0};
            if (p.noise) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (p.pv_noise != 0.0) fpv[k] = profile_factor(env_seed, kDomainPV, day, k, p.pv_noise);
                    if (p.price_noise != 0.0) fpr[k] = profile_factor(env_seed, kDomainPrice, day, k, p.price_noise);
                }
            }
            if (obs) {
                write_obs_header(o_row, p, s.tables->irr_norm, s.tables->price_norm, ratio, fpv, fpr);
                if (p.bess) o_row[O - 1] = (float)s.bess[e];
            }
            if (ep_return) ep_return[e] = 0.0;
        }
        const int k = p.pv ? 8 : 4;
        const uint32_t el8 = (uint32_t)e * 8u;
        // wavefronts 1..3: charger pairs part - 1, part + 2, ... (the SoC state's 16 B slots, sng_layout.h)
        for (int c0 = 2 * (part - 1); part > 0 && c0 < n; c0 += 2 * (kObsParts - 1)) {
            double soc0[2] = {0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = c0 + i;
                if (c >= n) break;
                GenStream rng{gen_key(seed, ge, (uint32_t)c, day), 0u};
                const VehicleDraw d = draw_vehicle(p, rng, 0, i4, i10, i1);
                const bool occ0 = d.ta == 0;   // t = 0 < T always, and dep >= 4/dt > 0
                soc0[i] = occ0 ? d.soc : 0.0;
                if (obs) {
                    o_row[k + c] = (float)soc0[i];
                    o_row[k + n + c] = departure_obs(pack_word(occ0, occ0, false, 0u, occ0 ? (uint32_t)d.dep : 0u));
                }
            }
            const SocOff so = soc_off(c0, n, E, el8);
            if (c0 + 1 < n)
                bst2<kNT>(s.soc, so.v, soc0[0], soc0[1], so.s);
            else
                bst<kNT>(s.soc, so.v, soc0[0], so.s);
        }
    }
    if (!obs) return;   // the whole grid alike
    __syncthreads();
    copy_out<kGenBlock>(obs + e0 * O, lds, nblk * O, vec_io != 0, tid);
}

// Two phases per (env, charger):
//  1. the day's vehicles: the waiting time to the next arrival is the number of failed
//     Bernoulli(0.4) trials before the first success (geometric, one draw via -log2(u)/-log2(0.6)),
//     then arrival SoC, capacity and departure -- a few draws per vehicle instead of one per free
//     step, without the per-step divergent arrival branch;
//  2. the dense timeline, step by step, from the vehicle list kept in LDS.
// Grid (E / 256, rows + 4): blocks y < gen_rows(N) the timeline of charger quad y / 4, the last 4 rows the
// t = 0 observation (observe_day0).  The day counter is read here and advanced by the day's first step
// (step_kernel, t = 0), so no block of this grid waits on another.  day_delta: the day drawn is the counter's
// plus this -- 0 but in an overlapped reset graph, whose generators all run before anything advances the counter
// (sng_graph_form.h day_shape).
// The timeline records leave as streaming (nontemporal) stores: reset 24.5-24.7 -> 22.5-22.7 us per day
// at 65,536 x 10 (A/B, one box), the steps' code and state staying in L2.  Diagnostic builds
// (round 2's -DSNG_GX_* builds, in commits before 8be1f55) split the reset's time: without the t = 0 observation blocks 24.3-24.9 us
// (they run beside the timeline blocks), without phase 1's draws 20.7, without the record stores 16-16.8.
// Write-through record stores (sc1 | nt, sc0 | sc1 | nt) left the day and the reset unchanged (A/B,
// profiles/r03_ab_generator_store_policy.txt).
constexpr int kGenRecPol = kNT;
// Timeline rows of the generator's grid (see generate_kernel): four rows of 64 envs per full charger quad; a
// last partial quad of w = N mod 4 chargers has 256 / w envs per row (w = 1, 2: one or two rows), or 64 envs
// with one lane in four idle (w = 3: four rows).
__host__ __device__ constexpr int gen_part_lanes(int w) { return w == 3 ? 4 : w; }   // lanes per env
__host__ __device__ constexpr int gen_rows(int n) { return 4 * (n / 4) + (n % 4 == 0 ? 0 : 4 * gen_part_lanes(n % 4) / 4); }
constexpr int kVehArrShift = 24;                   // vehicle list entry: arrival step (bits 24-31)
constexpr uint32_t kVehRecMask = 0x3fff8u;         // capacity (3-9) and departure (10-17)
// Vehicle list entries (LDS) are kept in the packed record's own layout: capacity in bits 3-9, departure
// step in 10-17 and arrival step in 24-31, so an occupied step's record is (entry & 0x3fff8 | flags) -
// t << 10 (the departure field becomes the steps left: it is > t while the vehicle is present, so nothing
// borrows, and below 64, so bits 16-17 clear); the arrival SoC is kept as the carry bits an empty record
// holds (rec_carry), computed once per vehicle in phase 1.  TT: the day's step count as
// a compile-time constant (the walk unrolled: 24 for the 1 h day), 0 for a runtime p.T; REQ: the
// requested-SoC stream.
template <int TT, bool REQ>
__global__ __launch_bounds__(kGenBlock) void generate_kernel(Params p, DeviceState s, uint64_t seed, int64_t E,
                                                             int i4, int i10, int i1, float *__restrict__ obs,
                                                             double *__restrict__ ep_return, int vec_io,
                                                             int day_delta) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint32_t *s_veh = reinterpret_cast<uint32_t *>(lds);                      // [V][BLOCK] arr | cap<<8 | dep<<16
    uint32_t *s_car = s_veh + kDaySlots * kGenBlock;                           // [V][BLOCK] arrival SoC carry bits
    double *s_req = reinterpret_cast<double *>(s_car + kDaySlots * kGenBlock);     // [V][BLOCK] (REQ only)
    const int tid = threadIdx.x;
    // grid rows: the timeline first, row u of charger quad u / 4 and 64 envs [256 x + 64 (u mod 4), +64), thread =
    // (env tid / 4, charger tid mod 4 of the quad), so a wavefront's record stores are 16 envs x the quad's
    // records, contiguous in the quad layout (sng_layout.h rec_index); then the t = 0 observation blocks
    // (gridDim.y - gen_rows(N) of them).  Dispatched last, they fill the CUs behind the timeline's VALU-bound
    // waves instead of delaying them: reset 16.0-16.3 -> 15.5-15.6 us (A/B three times on one box, same days,
    // profiles/r06_ab_generator_obs_order.txt; round 3's kernel had measured the opposite order 0.6 % better)
    const int u = (int)blockIdx.y;
    const uint64_t day = *s.episode + (uint64_t)day_delta;
    if (u >= gen_rows(p.n)) {
        observe_day0(p, s, seed, E, i4, i10, i1, day, obs, ep_return, vec_io, lds, u - gen_rows(p.n));
        return;
    }
    const int full = 4 * (p.n / 4);                              // timeline rows of the full quads
    const int q4 = u < full ? (u >> 2) * 4 : p.n & ~3;          // the quad's first charger
    const int qw = p.n - q4 < 4 ? p.n - q4 : 4;                 // its width (the last quad may be partial)
    const int lpe = u < full ? 4 : gen_part_lanes(qw);          // lanes per env: 256 / lpe envs per row
    const int sub = u < full ? (u & 3) : u - full;              // the row's env block within the 256
    const int c = q4 + tid % lpe;
    const int64_t e = (int64_t)blockIdx.x * kGenBlock + (int64_t)sub * (kGenBlock / lpe) + tid / lpe;
    if (e >= E || c >= p.n) return;
    const uint64_t ge = (uint64_t)(e + p.env_offset);   // global env id
    GenStream rng{gen_key(seed, ge, (uint32_t)c, day), 0u};
    const int T = TT > 0 ? TT : p.T;
    const int n = p.n;

    // phase 1 (charging_station.py:200-279)
    int tfree = 0, nv = 0;
    for (int v = 0; v < kDayVehicles - 1; ++v) {   // the last slot holds the sentinel
        if (tfree >= T) break;
        const VehicleDraw d = draw_vehicle(p, rng, tfree, i4, i10, i1);
        if (d.ta >= T) break;
        s_veh[v * kGenBlock + tid] = ((uint32_t)d.ta << kVehArrShift) | (d.cap << P_CAP_SHIFT) | ((uint32_t)d.dep << P_DEP_SHIFT);
        s_car[v * kGenBlock + tid] = rec_carry(false, d.code);
        if (REQ) {
            const double lo = d.soc <= 0.9 ? d.soc + 0.1 : 1.0;
            s_req[v * kGenBlock + tid] = lo + (1.0 - lo) * u32_unit(d.req_draw);
        }
        nv = v + 1;
        tfree = d.dep + 1;   // the departure step stays empty (charging_station.py:239-251)
    }

    // slot nv: a sentinel that never arrives or departs (arrival = departure = 255), so phase 2 walks
    // the list without a per-step bound check or branch (nv <= 7 < kDayVehicles, checked on the host)
    s_veh[nv * kGenBlock + tid] = (0xffu << kVehArrShift) | (0xffu << P_DEP_SHIFT);
    s_car[nv * kGenBlock + tid] = 0u;
    if (REQ) s_req[nv * kGenBlock + tid] = 1.0;

    // phase 2: the timeline.  An empty step's record carries the SoC of a vehicle arriving at the
    // next step (sng_layout.h), and plane 0 that of a vehicle arriving at t = 0.  cur = list[v] is the
    // vehicle of step t (until it has departed), nxt = list[v + 1] the one after it, read from LDS a
    // step before it can be needed; the record is assembled branch-free.
    uint32_t cur = s_veh[tid], nxt = s_veh[kGenBlock + tid];
    uint32_t car_cur = s_car[tid], car_nxt = s_car[kGenBlock + tid];
    double req_cur = REQ ? s_req[tid] : 1.0, req_nxt = REQ ? s_req[kGenBlock + tid] : 1.0;
    int nx = kGenBlock + tid;   // the slot of list[v + 1]
    bool prev_occ = false;
    bool pen = false;   // step t is in the penalty-check list observe(t-1) built
    // step t occupied / its vehicle arriving at t, carried from step to step: step t + 1 is occupied iff
    // its vehicle arrives then (arr1) or step t's vehicle stays past t + 1
    bool occ = (cur >> kVehArrShift) == 0u, stat = occ;
    // penalty-check list built by observe(t-1) (charging_station.py:42-63) as one unsigned range
    // test on the steps the vehicle at t-1 had left: on_departure {1}, sparse {1..3}, dense any;
    // no_penalty never (lo = 256 > any remainder)
    const uint32_t pen_lo = (p.penalty_mode == SNG_PENALTY_NONE) ? 256u : 1u;
    const uint32_t pen_span = (p.penalty_mode == SNG_PENALTY_SPARSE) ? 2u
                              : (p.penalty_mode == SNG_PENALTY_DENSE) ? 254u : 0u;
    // the record slot (quad layout: the quad row in soffset, env and charger in the lane offset) and the
    // requested-SoC slot ([N][E] planes: charger row and env in the lane offset)
    const uint32_t el2 = ((uint32_t)e * (uint32_t)qw + (uint32_t)(c - q4)) * 2u;
    const uint32_t r2 = (uint32_t)q4 * (uint32_t)E * 2u;
    const uint32_t el8 = ((uint32_t)c * (uint32_t)E + (uint32_t)e) * 8u;
    uint16_t *rec = reinterpret_cast<uint16_t *>(s.aux);
    const size_t nE = (size_t)n * (size_t)E;
    // raw buffer stores: the plane in the V#, the quad row in soffset, the slot in the lane offset
    bst16<kGenRecPol>(rec, el2, ((cur >> kVehArrShift) == 0u) ? car_cur : 0u, r2);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        // the vehicle of step t + 1: past the current departure, the next one (the list ends in a
        // sentinel that never arrives or departs)
        const bool adv = (uint32_t)(t + 1) > ((cur >> P_DEP_SHIFT) & 0xffu);
        const uint32_t v1 = adv ? nxt : cur;
        const uint32_t car1 = adv ? car_nxt : car_cur;
        const double req1 = adv ? req_nxt : req_cur;
        nx += adv ? kGenBlock : 0;   // list[v + 1] for step t + 1 (slot 8 at most, kDaySlots)
        const uint32_t nxt1 = s_veh[nx];
        const uint32_t car_nxt1 = s_car[nx];
        const double req_nxt1 = REQ ? s_req[nx] : 1.0;

        const uint32_t flags = W_OCC | (stat ? W_STATIC : 0u) | (pen ? W_PEN : 0u);
        // capacity and departure in place, the departure becoming the steps left (dep > t while the vehicle
        // is present, and dep - t <= 10 / dt < 64 fits the record's 6 bits: nothing borrows or spills)
        const uint32_t w_occ = ((cur & kVehRecMask) | flags) - ((uint32_t)t << P_DEP_SHIFT);
        const bool arr1 = (v1 >> kVehArrShift) == (uint32_t)(t + 1);   // step t + 1's vehicle arrives then
        const uint32_t carry = arr1 ? car1 : 0u;
        const uint32_t w_emp = (pen ? W_PEN : 0u) | carry;
        bst16<kGenRecPol>(rec + (size_t)(t + 1) * nE, el2, occ ? w_occ : w_emp, r2);
        // requested SoC timeline (sng_layout.h): Requested_SOC[c, t-1] at t >= 1 -- the step reads
        // it where W_PEN is set -- and Requested_SOC[c, T-1] in the t = 0 slot (written below)
        if (REQ && t > 0) bst(s.req + (size_t)t * nE, el8, prev_occ ? req_cur : 0.0);
        prev_occ = occ;
        // step t + 1's penalty check: occupied at t with dep - t steps left in [pen_lo, pen_lo + pen_span]
        // (w_occ's departure field holds dep - t; an empty charger is never in the list)
        pen = occ && (w_occ >> P_DEP_SHIFT) - pen_lo <= pen_span;
        occ = (occ && (uint32_t)(t + 1) < ((cur >> P_DEP_SHIFT) & 0xffu)) || arr1;
        stat = arr1;
        cur = v1;
        car_cur = car1;
        req_cur = req1;
        nxt = nxt1;
        car_nxt = car_nxt1;
        req_nxt = req_nxt1;
    }
    if (REQ) bst(s.req, el8, prev_occ ? req_cur : 0.0);
}

}  // namespace sng
