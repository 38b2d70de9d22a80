// sng_ref_day.h -- reference-RNG days on the device: MT19937 per env (mt_seed_kernel, mt_prepare_kernel,
// mt_twist_lane, which sng_generate.h declares for py_ratio_lane) and the reference-day generator
// (MtRingT, ref_day2_kernel).
// Needs sng_mt.h (kMtN, tempering, the position word), sng_layout.h (pack_word) and sng_dev_util.h (kWave, bst,
// wave_lds_fence, the stamp hooks).  Included by sng_kernels.hip only, behind probe_copy_kernel, so the
// kernels keep the order they have had in the code object.
#pragma once

namespace sng {

// ---------------------------------------------------------------------------------
// Reference-RNG days on the GPU (SngRngMode SNG_RNG_REFERENCE): numpy's MT19937 stream of each env
// (np.random.seed(seed + global env), RandomState's state and draw semantics, sng_mt.h restates them
// for the host) drives ChargingStation.generate_initial_vehicle_presence_per_charger
// (charging_station.py:200-279) draw for draw, and the day is encoded into the word / f64 aux (/ req)
// timeline exactly as the host encoder does it (sng_host_day.h encode_day).  Three kernels:
//   mt_seed_kernel     init_genrand per env (once per seeding)
//   mt_prepare_kernel  per env, one wavefront: the state one twist ahead into the other block (the
//                      twist's three dependent ranges, 64 words at a time, in LDS)
//   ref_day2_kernel    per env, one lane: the day's draws (phase 1) and its timeline (phase 2)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) { return mt_temper_word(y); }
__device__ __forceinline__ uint32_t mt_untemper(uint32_t y) { return mt_untemper_word(y); }

__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b) {   // twist term of words kk, kk + 1
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// B = twist(A), both 624 words (MT19937's in-place twist, its ranges computed out of place):
// B[k] = A[k+M] ^ mix(A[k], A[k+1]) for k < N-M; B[k] = B[k+M-N] ^ mix(A[k], A[k+1]) up to N-2;
// B[N-1] = B[M-1] ^ mix(A[N-1], B[0]).
__device__ __forceinline__ void mt_twist_wave(const uint32_t *A, uint32_t *B, int lane) {
    constexpr int NM = kMtN - kMtM;   // 227
    for (int k = lane; k < NM; k += kWave) B[k] = A[k + kMtM] ^ mt_mix(A[k], A[k + 1]);
    wave_lds_fence();
    for (int k = NM + lane; k < 2 * NM; k += kWave) B[k] = B[k - NM] ^ mt_mix(A[k], A[k + 1]);
    wave_lds_fence();
    for (int k = 2 * NM + lane; k < kMtN - 1; k += kWave) B[k] = B[k - NM] ^ mt_mix(A[k], A[k + 1]);
    wave_lds_fence();
    if (lane == 0) B[kMtN - 1] = B[kMtM - 1] ^ mt_mix(A[kMtN - 1], B[0]);
    wave_lds_fence();
}

// the same by one thread, in place of the stream's exhausted other block (a day that draws past two
// blocks: not reachable by the generator's draw counts, kept for completeness)
// (both blocks tempered, as the streams keep them)
__device__ __noinline__ void mt_twist_lane(const uint32_t *A, uint32_t *B) {
    constexpr int NM = kMtN - kMtM;
    auto a = [&](int k) { return mt_untemper(A[k]); };
    auto b = [&](int k) { return mt_untemper(B[k]); };
    for (int k = 0; k < NM; ++k) B[k] = mt_temper(a(k + kMtM) ^ mt_mix(a(k), a(k + 1)));
    for (int k = NM; k < kMtN - 1; ++k) B[k] = mt_temper(b(k - NM) ^ mt_mix(a(k), a(k + 1)));
    B[kMtN - 1] = mt_temper(b(kMtM - 1) ^ mt_mix(a(kMtN - 1), b(0)));
}

// np.random.seed(s): init_genrand(s & 0xffffffff); mti = N, so the first draw twists
__global__ __launch_bounds__(256) void mt_seed_kernel(RefStreams rs, uint64_t seed0, int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    uint32_t *b = rs.mt + (size_t)e * 2 * kMtN;
    uint32_t x = (uint32_t)(seed0 + (uint64_t)e);
    b[0] = mt_temper(x);
    for (int i = 1; i < kMtN; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
        b[i] = mt_temper(x);
    }
    rs.pos[e] = kMtN;   // block 0, mti = N
}

// Before a day: an exhausted current block (mti = N) is replaced by its successor, and the block after the
// current one is put into the other slot, so the day has >= 624 draws without a twist of its own.  The
// position word is cur << 16 | kMtNextReady | mti; kMtNextReady says the other slot already holds the
// current block's successor (a day of ~300 draws leaves it untouched), so most days need no twist here.
__global__ __launch_bounds__(256) void mt_prepare_kernel(RefStreams rs, int64_t E) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4][2][kMtN];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= E) return;   // wave-uniform
    const int32_t pos = rs.pos[e];
    int cur = (pos >> 16) & 1, mti = pos & kMtPosMask;
    const bool next_ready = (pos & kMtNextReady) != 0;
    if (next_ready && mti < kMtN) return;   // nothing to prepare
    uint32_t *blk = rs.mt + (size_t)e * 2 * kMtN;
    uint32_t *A = lds[wave][0], *B = lds[wave][1];
    if (mti >= kMtN && next_ready) {   // the successor is in place: it becomes the current block
        cur ^= 1;
        mti -= kMtN;
    }
    // 16 B per lane: a block is 156 groups of 4 words
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    auto load_block = [&](int slot, uint32_t *dst) {
        for (int g = lane; g < kMtN / 4; g += kWave) {
            u32x4 x = *reinterpret_cast<const u32x4 *>(blk + slot * kMtN + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = mt_untemper(x[i]);
            *reinterpret_cast<u32x4 *>(dst + 4 * g) = x;
        }
    };
    auto store_block = [&](int slot, const uint32_t *src) {
        for (int g = lane; g < kMtN / 4; g += kWave) {
            u32x4 x = *reinterpret_cast<const u32x4 *>(src + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = mt_temper(x[i]);
            *reinterpret_cast<u32x4 *>(blk + slot * kMtN + 4 * g) = x;
        }
    };
    load_block(cur, A);
    wave_lds_fence();
    if (mti >= kMtN) {
        mt_twist_wave(A, B, lane);
        uint32_t *x = A;
        A = B;
        B = x;
        cur ^= 1;
        mti -= kMtN;
        store_block(cur, A);
    }
    mt_twist_wave(A, B, lane);
    store_block(cur ^ 1, B);
    if (lane == 0) rs.pos[e] = (cur << 16) | kMtNextReady | mti;
}

// One env's numpy stream inside ref_day2_kernel: RandomState.random_sample / uniform / randint
// (legacy, masked rejection) over the tempered words of the prepared blocks (sng_mt.h, host twin).
//
// The words reach the lane through a ring of 64 words in LDS, topped up for the whole wavefront at
// once: the draws of a day are data-dependent (a free step draws two words, an arrival ~10), so the
// 64 lanes of a wavefront desynchronise, and a global load per draw made every draw of every lane
// wait out a memory round trip (0.53 ms per day at any population size).  A lane's draw is an LDS
// read; when any lane's ring holds <= kTopUp words, every lane holding <= kRefill words commits the
// next kRefill words into its ring.  Those words were loaded into registers one refill earlier (pf:
// 8 aligned 16 B loads), so a refill waits for loads issued a refill ago, not for a fresh round trip:
// the wavefront that draws issues no global stores (the timeline is the writer wavefront's, see
// ref_day2_kernel), so nothing else is counted in vmcnt ahead of those loads.  A draw that finds the
// ring empty (a rejection streak) refills its lane the same way.
// Stream word q counts from the start of the day's current block: block k = q / 624 sits in slot
// (cur0 + k) & 1, and a 4-word group never straddles two blocks (624 = 4 * 156).  Blocks 0 and 1 are
// prepared (mt_prepare_kernel); a day that draws into block 2 or beyond twists it on its lane into the
// slot of block k - 2, which the ring has consumed by then (it runs at most 96 words ahead: 64 in the
// ring, 32 in registers).
// LDS layout ring[slot][lane]: lanes reading any slots hit distinct banks.
constexpr int kRing = 64;     // words per lane in LDS
constexpr int kRefill = 32;   // words per refill (8 aligned 16 B groups)
constexpr int kTopUp = 24;    // after a top_up every lane holds more than this: the peeks reach head + 23
static_assert(kTopUp + kRefill <= kRing, "ring sizes");
// RandomState.random_sample from two tempered words (numpy's rk_double: 53 bits, a >> 5 and b >> 6)
__device__ __forceinline__ double rand53(uint32_t wa, uint32_t wb) {
    const int32_t a = (int32_t)(wa >> 5), b = (int32_t)(wb >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
}
template <int ENVS>
struct MtRingT {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    uint32_t *blk;
    uint32_t *ring;   // this lane's ring: ring[slot * ENVS], slot < kRing
    int cur0;
    int head, tail;   // stream words (from the current block's start) drawn / committed into the ring
    int q0;           // the day's first word (mti at the start)
    int avail;        // stream blocks materialised: 0 .. avail - 1
    u32x4 pf[kRefill / 4];   // words [tail, tail + kRefill), loaded ahead of their refill
    __device__ __forceinline__ void materialise(int last) {   // blocks up to that of word `last`
        const int kmax = last / kMtN;
        while (avail <= kmax) {   // rare: a day of more than ~1,000 draws
            mt_twist_lane(blk + ((cur0 + avail - 1) & 1) * kMtN, blk + ((cur0 + avail) & 1) * kMtN);
            ++avail;
        }
    }
    // pf <- words [tail, tail + kRefill): they span at most two blocks (word tail + 4g is in block k0 up to
    // offset 624)
    __device__ __forceinline__ void prefetch() {
        materialise(tail + kRefill - 1);
        const int k0 = tail / kMtN, off0 = tail - k0 * kMtN;
        const uint32_t *b0 = blk + ((cur0 + k0) & 1) * kMtN, *b1 = blk + ((cur0 + k0 + 1) & 1) * kMtN;
#pragma unroll
        for (int g = 0; g < kRefill / 4; ++g) {
            const int off = off0 + 4 * g;
            pf[g] = *reinterpret_cast<const u32x4 *>(off < kMtN ? b0 + off : b1 + (off - kMtN));
        }
    }
    // the day's start: the ring is empty (tail = the first word's aligned group), its first words in flight
    __device__ __forceinline__ void start(int mti) {
        head = q0 = mti;
        tail = mti & ~3;
        avail = 2;
        prefetch();
    }
    // this lane: the prefetched words into the ring (which then holds <= kRing), the next ones in flight
    __device__ __forceinline__ void refill_lane() {
#pragma unroll
        for (int g = 0; g < kRefill / 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) ring[((tail + 4 * g + i) & (kRing - 1)) * ENVS] = pf[g][i];   // tempered
        tail += kRefill;
        prefetch();
    }
    // wave-uniform test: lanes holding <= kRefill words refill, so every lane then holds > kTopUp
    __device__ __forceinline__ void top_up() {
        if (__builtin_amdgcn_ballot_w64(tail - head <= kTopUp))
            if (tail - head <= kRefill) refill_lane();
    }
    __device__ __forceinline__ uint32_t next() {
        if (head >= tail) refill_lane();   // the ring ran dry inside one step (a rejection streak)
        const uint32_t y = ring[(head & (kRing - 1)) * ENVS];
        ++head;
        return y;
    }
    // word head + k, without advancing: valid for k <= kTopUp after a top_up
    __device__ __forceinline__ uint32_t peek(int k) const { return ring[((head + k) & (kRing - 1)) * ENVS]; }
    __device__ __forceinline__ double random() {
        const uint32_t a = next();
        return rand53(a, next());
    }
    __device__ __forceinline__ double uniform(double lo, double hi) { return lo + (hi - lo) * random(); }
    __device__ __forceinline__ int randint(int low, int high) {   // exclusive high; one value: no draw
        if (high - 1 - low == 0) return low;
        uint32_t mask = (uint32_t)(high - 1 - low);
        mask |= mask >> 1;
        mask |= mask >> 2;
        mask |= mask >> 4;
        mask |= mask >> 8;
        mask |= mask >> 16;
        const uint32_t rng = (uint32_t)(high - 1 - low);
        uint32_t v;
        while ((v = (next() & mask)) > rng) {
        }
        return low + (int)v;
    }
    // the stream position after the day, as MtLane kept it: the block of the last word drawn and the
    // words drawn from it (624 = exhausted, twisted lazily at the next draw); kMtNextReady when the
    // other slot holds that block's successor
    __device__ __forceinline__ int32_t position() const {
        if (head == q0) return (cur0 << 16) | kMtNextReady | q0;
        const int k = (head - 1) / kMtN;
        return (((cur0 + k) & 1) << 16) | (k + 1 < avail ? kMtNextReady : 0) | (head - k * kMtN);
    }
};
// kRefGroups groups of ENVS envs per workgroup (lanes >= ENVS mirror them), each with a drawing wavefront
// (wavefront g) and a timeline wavefront (wavefront kRefGroups + g).  One group per workgroup: the
// dispatcher then puts two drawing wavefronts (and a timeline one) on ~96 of the 1,024 SIMDs, and their
// workgroups set the kernel's span (84 us against a median of 68 us).  Four groups (a workgroup of 8
// wavefronts fills one CU, wavefronts w and w + 4 on one SIMD) placed every drawing wavefront beside a
// timeline one, but the workgroup's barriers then couple four drawing wavefronts, and the span stayed at
// 85 us (A/B, profiles/r05_ab_refday_two_wavefronts.txt).
constexpr int kRefGroups = 1;
constexpr int kRefBlock = 2 * kRefGroups * kWave;

// The same day in two phases per charger, as generate_kernel draws a device day: (1) the charger's
// vehicles, visiting only the steps that draw (a free step draws the arrival test, an arrival the
// vehicle's values; an occupied step and a departure step draw nothing, charging_station.py:200-279),
// into a per-lane list in LDS; (2) the word / f64 aux (/ req) timeline from the list, branch-free, step
// by step.  Round 2's steps-major kernel executed the arrival path under a mask in nearly every (charger,
// step) iteration of a wavefront; here a wavefront iterates once per draw step of its busiest lane
// (about 5 of a charger's 24 steps draw).  The stream is consumed draw for draw.
// Round 5: the phases run on two wavefronts of one workgroup.  The drawing wavefront (0) writes charger
// c's list into LDS buffer c & 1 and meets the timeline wavefront (1) at one barrier per charger; the
// timeline wavefront then writes charger c's timeline from that buffer while the drawing wavefront draws
// charger c + 1 into the other one.  Round 4's single wavefront issued ~50 timeline stores per charger,
// and on gfx9 stores count in vmcnt ahead of any later load, so the next charger's first ring refill
// waited for all of them to complete (~0.8 us per charger) and the stores did not overlap the draws.
constexpr int kRefVeh = 8;   // vehicles per charger-day (T / (4/dt + 1) + 1 <= 7 for every dt dividing 24 h) + sentinel
// Phase 1 reads each draw step's words from the ring in two batches of LDS reads instead of one round
// trip per word: after a top_up every lane still drawing holds more than kTopUp words, so the 10 words
// an arrival may need first (arrival test, SoC, the discarded uniform, four capacity candidates) and the
// 6 it may need next (requested SoC, four departure candidates) are peeked without a bound check.  A
// masked rejection (numpy's legacy bounded randint) takes the first of four candidates that passes; all
// four rejected (p < 0.2 % for a capacity, < 0.4 % for a departure) continues word by word.
// A step without a vehicle draws only its arrival test, so phase 1 tests the next kScan steps together
// (integer compares, arrives()) and takes the first arrival with its vehicle in the same iteration: a
// wavefront iterates ~5 times per charger-day instead of once per drawing step of its busiest lane (~15).
// Round 5 (A/B, reference reset obs-ready at 65,536 envs): kScan 2 0.133 ms, 3 0.124, 4 0.119-0.121,
// 5 0.117-0.118, 6 0.117-0.119 (with a larger top-up).
constexpr int kScan = 5;
// the furthest peek of an iteration: the arrival tests up to 2 kScan - 1, then from an arrival at scan
// position kScan - 1 (skip 2 (kScan - 1)) the capacity path's 10 words and the departure's 6
static_assert(2 * (kScan - 1) + 10 + 5 <= kTopUp, "phase 1's peeks stay inside a topped-up ring");
// round(random.rand() - 0.1) == 1 (charging_station.py:214-215) on the 53-bit draw K = (a >> 5) << 26 |
// (b >> 6), random.rand() = K / 2^53 (rk_double): fl(K / 2^53 - 0.1) > 0.5 is monotone in K and holds
// from K = 0x13333333333334 on (checked against the double expression at every K within 3,000 of it and
// at 10^5 random K; tests/test_ref_arrival_threshold.py)
constexpr uint64_t kArrive53 = 0x13333333333334ull;
__device__ __forceinline__ bool arrives(uint32_t wa, uint32_t wb) {
    return ((((uint64_t)(wa >> 5)) << 26) | (uint64_t)(wb >> 6)) >= kArrive53;
}
// Vehicle-list buffers of ref_day2_kernel: charger c's list is in buffer c mod D.  The drawing wavefront's
// lanes do not wait for each other at the end of a charger: a lane that has drawn charger c's vehicles goes
// on to charger c + 1 while the wavefront's slowest lane still draws charger c (D = 3: one charger ahead;
// the timeline wavefront reads the buffer of charger c - 1 meanwhile).  A wavefront then iterates about as
// often as its busiest lane over the whole station (~41 times a day, simulated) instead of the sum over the
// chargers of each one's busiest lane (~51).  With the requested-SoC lists (REQ) two buffers fit the LDS
// of four workgroups per CU, and the lanes keep in step charger by charger.
__host__ __device__ constexpr int ref_day2_lists(bool req) { return req ? 2 : 3; }
// LDS of ref_day2_kernel: the rings, then the list buffers ([V][ENVS] each: entry, arrival SoC, and the
// requested SoC with REQ)
__host__ __device__ constexpr size_t ref_day2_list_bytes(bool req, int envs) {
    return (size_t)kRefVeh * envs * (4 + 8 + (req ? 8 : 0));
}
__host__ __device__ constexpr size_t ref_day2_group_bytes(bool req, int envs) {
    return (size_t)kRing * envs * 4 + (size_t)ref_day2_lists(req) * ref_day2_list_bytes(req, envs);
}
__host__ __device__ constexpr size_t ref_day2_lds_bytes(bool req, int envs) {
    return (size_t)kRefGroups * ref_day2_group_bytes(req, envs);
}
static_assert(ref_day2_lds_bytes(true, 64) <= 160 * 1024 && ref_day2_lds_bytes(false, 64) <= 160 * 1024,
              "a ref_day2_kernel workgroup fits one CU's LDS");
template <int TT, bool REQ, int ENVS>
__global__ __launch_bounds__(kRefBlock) __attribute__((amdgpu_waves_per_eu(2))) void ref_day2_kernel(Params p, DeviceState s, RefStreams rs, int64_t E,
                                                             int i4, int i10, int i1) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rd_lds[];
    // At most two wavefronts per SIMD: a VGPR count above 512 / 3 (v175 reserved here; the kernel needs ~160).
    // With room for three, the dispatcher stacked two drawing wavefronts and a timeline one on ~96 of the
    // 1,024 SIMDs and left others with one, and those SIMDs' workgroups set the span: 86.9 -> 77.5 us,
    // reference reset 0.128 -> 0.119 ms obs-ready (A/B, profiles/r05_ab_refday_two_wavefronts.txt).  This assumes
    // gfx950's 512 VGPRs per SIMD lane with an allocation granule of 8 (176 > 512 / 3); tests/test_kernel_resources.py
    // reads the built code object's VGPR count and fails when the cap no longer holds
    // (profiles/r06_kernel_resources.txt: without this line the compiler allocates 158 VGPRs, three per SIMD).
    asm volatile("v_mov_b32 v175, 0" ::: "v175");
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int wv = w / kRefGroups, g = w % kRefGroups;   // wv 0 draws, 1 writes group g's timeline
    const int wl = (int)threadIdx.x % kWave;
    const int lane = wl % ENVS;   // the env slot; lanes >= ENVS of either wavefront mirror it
    const int rec = (int)blockIdx.x * kRefGroups + g;   // the group's index (diagnostic stamps)
    const int64_t e0 = (int64_t)rec * ENVS;
    const bool live = e0 + lane < E && wl < ENVS;
    const int64_t e = e0 + lane < E ? e0 + lane : E - 1;   // past E: env E - 1's stream, nothing stored
    // the group's LDS: its ring [kRing][ENVS], then its list buffers
    uint32_t *glds = rd_lds + (size_t)g * ref_day2_group_bytes(REQ, ENVS) / 4;
    uint32_t *rings = glds;
    // list buffer b (charger c's is c mod D): entries ta | cap << W_CAP_SHIFT | dep << W_DEP_SHIFT, then arrival
    // SoC, then requested SoC (REQ)
    constexpr int D = ref_day2_lists(REQ);
    auto list_veh = [&](int b) {
        return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(glds) + (size_t)kRing * ENVS * 4 +
                                            (size_t)b * ref_day2_list_bytes(REQ, ENVS));
    };
    auto list_soc = [&](int b) { return reinterpret_cast<double *>(list_veh(b) + kRefVeh * ENVS); };
    auto list_req = [&](int b) { return list_soc(b) + kRefVeh * ENVS; };
    const int T = TT > 0 ? TT : p.T, n = p.n;
    const uint32_t pen_lo = (p.penalty_mode == SNG_PENALTY_NONE) ? 256u : 1u;   // as generate_kernel
    const uint32_t pen_span = (p.penalty_mode == SNG_PENALTY_SPARSE) ? 2u
                              : (p.penalty_mode == SNG_PENALTY_DENSE) ? 254u : 0u;
    const uint32_t el8 = (uint32_t)e * 8u;
    const size_t nE = (size_t)n * (size_t)E;
    // diagnostic builds: stamps 0 / 1 the drawing wavefront's start and end, 2 its ticks in phase 1 (6, 7 its
    // XCC id and HW_ID); 3 the timeline wavefront's ticks in phase 2, 4 its end, 5 its HW_ID | XCC id << 32
    SNG_WSTAMP_DECL;
    SNG_WSTAMP(0);
    if (wv == 0) {
        [[maybe_unused]] const unsigned long long t1_ = SNG_WNOW();
        MtRingT<ENVS> rng;
        const int32_t pos = rs.pos[e];
        rng.blk = rs.mt + (size_t)e * 2 * kMtN;
        rng.ring = rings + lane;
        rng.cur0 = (pos >> 16) & 1;
        rng.start(pos & kMtPosMask);
        // phase 1: every lane draws its chargers' vehicles, one iteration per step that draws, charger after
        // charger; the wavefront meets the timeline wavefronts once all its lanes are past charger k (barrier
        // k + 1: the workgroup's, so the groups' drawing wavefronts meet there too), and a lane draws charger c
        // only while c <= k + D - 2 (its buffer is free)
        int c = 0, cb = 0, t = 0, nv = 0;   // the lane's charger, its buffer (c mod D), step, vehicles so far
        int kb = 0;                          // barriers passed (wave-uniform): k above
        uint32_t *s_veh = list_veh(0);
        double *s_soc = list_soc(0), *s_req = list_req(0);
        while (kb < n) {
            if (c < n && c <= kb + D - 2) {
                rng.top_up();   // ballots over the lanes drawing: each then holds > kTopUp words
                // the next kScan steps' arrival draws at once: the first that arrives, the free steps before
                // it consumed together
                uint32_t a[2 * kScan];
#pragma unroll
                for (int k = 0; k < 2 * kScan; ++k) a[k] = rng.peek(k);
                int j = kScan;
#pragma unroll
                for (int kk = kScan - 1; kk >= 0; --kk) j = arrives(a[2 * kk], a[2 * kk + 1]) ? kk : j;
                const int skip = min(j, T - t);
                rng.head += 2 * skip;
                t += skip;
                if (t < T && j < kScan) {   // an arrival at step t
                    uint32_t w[10];   // from the arrival draw: w[0], w[1] are it (not reread)
#pragma unroll
                    for (int k = 2; k < 10; ++k) w[k] = rng.peek(k);
                    const double soc = 0.1 + (0.9 - 0.1) * rand53(w[2], w[3]);      // uniform(0.1, 0.9), :257-259
                    const double lo = soc <= 0.9 ? soc + 0.1 : 1.0;
                    // w[4], w[5]: the discarded uniform (:219)
                    uint32_t cap = 40u;
                    bool seq = false;   // the draws continue word by word (a rejection streak)
                    if (p.diff_caps) {   // randint(15, 120) (:267-269): mask 127, accept <= 104
                        int k = 4;
                        uint32_t cv = 0u;
#pragma unroll
                        for (int kk = 3; kk >= 0; --kk) {   // the first candidate that passes, without an index
                            const uint32_t x = w[6 + kk] & 127u;
                            k = (x <= 104u) ? kk : k;
                            cv = (x <= 104u) ? x : cv;
                        }
                        if (k < 4) {
                            cap = 15u + cv;
                            rng.head += 7 + k;
                        } else {
                            rng.head += 10;
                            cap = (uint32_t)rng.randint(15, 120);
                            seq = true;
                        }
                    } else {
                        rng.head += 6;
                    }
                    double rq = 1.0;
                    const int high = min(t + i10, T + i1), low = t + i4;             // :271-279
                    int dep = low;
                    if (!seq) {
                        uint32_t v[6];
#pragma unroll
                        for (int k = 0; k < 6; ++k) v[k] = rng.peek(k);
                        constexpr int U = REQ ? 2 : 0;
                        if (REQ) rq = lo + (1.0 - lo) * rand53(v[0], v[1]);       // uniform(lo, 1), :261-265
                        int used = U;
                        if (low < high && high - 1 - low > 0) {   // randint(low, high); one value draws nothing
                            const uint32_t span = (uint32_t)(high - 1 - low);
                            uint32_t mask = span;
                            mask |= mask >> 1;
                            mask |= mask >> 2;
                            mask |= mask >> 4;
                            mask |= mask >> 8;
                            mask |= mask >> 16;
                            int k = 4;
                            uint32_t dv = 0u;
#pragma unroll
                            for (int kk = 3; kk >= 0; --kk) {
                                const uint32_t x = v[U + kk] & mask;
                                k = (x <= span) ? kk : k;
                                dv = (x <= span) ? x : dv;
                            }
                            if (k < 4) {
                                dep = low + (int)dv;
                                used += k + 1;
                            } else {
                                rng.head += U + 4;
                                used = 0;
                                uint32_t x;
                                while ((x = (rng.next() & mask)) > span) {
                                }
                                dep = low + (int)x;
                            }
                        }
                        rng.head += used;
                    } else {
                        rq = REQ ? rng.uniform(lo, 1.0) : 1.0;
                        dep = (low >= high) ? low : rng.randint(low, high);
                    }
                    const int vi = nv < kRefVeh - 1 ? nv : kRefVeh - 2;   // at most 7 (see kRefVeh)
                    s_veh[vi * ENVS + lane] = (uint32_t)t | (cap << W_CAP_SHIFT) | ((uint32_t)dep << W_DEP_SHIFT);
                    s_soc[vi * ENVS + lane] = soc;
                    if (REQ) s_req[vi * ENVS + lane] = rq;
                    nv = vi + 1;
                    t = dep + 1;   // occupied until dep - 1; the departure step is empty and draws nothing
                }
                if (t >= T) {   // the charger's list is complete: the sentinel, then the next charger
                    s_veh[nv * ENVS + lane] = 0xffu | (0xffu << W_DEP_SHIFT);   // never arrives
                    s_veh[(nv + 1 < kRefVeh ? nv + 1 : nv) * ENVS + lane] = 0xffu | (0xffu << W_DEP_SHIFT);
                    ++c;
                    cb = cb + 1 == D ? 0 : cb + 1;
                    t = 0;
                    nv = 0;
                    s_veh = list_veh(cb);
                    s_soc = list_soc(cb);
                    s_req = list_req(cb);
                }
            }
            // every lane past charger k: its list is complete, and the timeline wavefront may take it
            while (kb < n && __builtin_amdgcn_ballot_w64(c <= kb) == 0) {
                __syncthreads();   // barrier k + 1 (the timeline wavefront's of charger k)
                ++kb;
            }
        }
        SNG_WACC(2, t1_);
        if (live) rs.pos[e] = rng.position();
    } else {
        for (int c = 0; c < n; ++c) {
            __syncthreads();   // charger c's list is complete, in buffer c mod D
            [[maybe_unused]] const unsigned long long t2_ = SNG_WNOW();
            const uint32_t *s_veh = list_veh(c % D);
            const double *s_soc = list_soc(c % D), *s_req = list_req(c % D);
            // phase 2: the timeline (encode_day, sng_host_day.h): cur = the vehicle of step t until step t has
            // passed its departure step, nxt the one after it (read a step ahead); a stay of zero steps
            // (dep == arrival, possible when 4/dt < 1) still marks its arrival step STATIC, as the host
            // encoder's arrival list does
            int v = 0;
            uint32_t cur = s_veh[lane], nxt = s_veh[ENVS + lane];
            double soc_cur = s_soc[lane], soc_nxt = s_soc[ENVS + lane];
            double req_cur = REQ ? s_req[lane] : 1.0, req_nxt = REQ ? s_req[ENVS + lane] : 1.0;
            bool prev_occ = false;
            uint32_t prev_rem = 0u;
            double prev_req = 0.0;
#pragma unroll
            for (int tt = 0; tt < T; ++tt) {
                const uint32_t ta = cur & 0xffu, dep = cur >> W_DEP_SHIFT;
                const bool adv = (uint32_t)(tt + 1) > dep;   // step t + 1 belongs to the next vehicle
                const int vr = v + 2 < kRefVeh ? v + 2 : kRefVeh - 1;
                const uint32_t nn = s_veh[vr * ENVS + lane];   // list[v + 2], for when nxt becomes current
                const double soc_nn = s_soc[vr * ENVS + lane];
                const double req_nn = REQ ? s_req[vr * ENVS + lane] : 1.0;
                const bool occ = (uint32_t)tt >= ta && (uint32_t)tt < dep;
                const bool arrived = (uint32_t)tt == ta;
                const bool running = !arrived && prev_occ;
                const uint32_t rem = occ ? dep - (uint32_t)tt : 0u;
                const bool pen = prev_rem - pen_lo <= pen_span;   // prev_rem = 0: empty at t-1
                const size_t plane = (size_t)tt * nE;
                // every lane stores: a lane that is not live mirrors a live one (the same env's stream, so
                // the same values to the same addresses)
                {
                    // plain global stores (a uniform plane pointer + the env): one buffer descriptor per plane
                    // would not fit the SGPRs of the unrolled walk
                    const size_t row = plane + (size_t)c * (size_t)E;
                    s.word[row + (size_t)e] = pack_word(occ, !running, pen, occ ? (cur >> W_CAP_SHIFT) & 0xffu : 0u, rem);
                    s.aux[row + (size_t)e] = (occ && !running) ? soc_cur : 0.0;
                    if (REQ && tt > 0) s.req[row + (size_t)e] = prev_req;   // Requested_SOC[c, t-1]
                }
                prev_occ = occ;
                prev_rem = rem;
                prev_req = occ ? req_cur : 0.0;
                v += adv ? 1 : 0;
                cur = adv ? nxt : cur;
                soc_cur = adv ? soc_nxt : soc_cur;
                req_cur = adv ? req_nxt : req_cur;
                nxt = adv ? nn : nxt;
                soc_nxt = adv ? soc_nn : soc_nxt;
                req_nxt = adv ? req_nn : req_nxt;
            }
            if (REQ) bst(s.req, el8, prev_req, (uint32_t)c * (uint32_t)E * 8u);   // slot 0: Requested_SOC[c, T-1]
            SNG_WACC(3, t2_);
        }
    }
    const int t0 = w * kWave;   // the wavefront's first thread writes its stamps
    if (wv == 0) {
        SNG_WSTAMP(1);
        SNG_WSTAMP_PUT(0, stamp_[0], rec, t0);
        SNG_WSTAMP_PUT(1, stamp_[1], rec, t0);
        SNG_WSTAMP_PUT(2, stamp_[2], rec, t0);
        SNG_WSTAMP_PUT(6, (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20), rec, t0);
        SNG_WSTAMP_PUT(7, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4), rec, t0);
    } else {
        SNG_WSTAMP(4);
        SNG_WSTAMP_PUT(3, stamp_[3], rec, t0);
        SNG_WSTAMP_PUT(4, stamp_[4], rec, t0);
        SNG_WSTAMP_PUT(5, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                              ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32), rec, t0);
    }
}

}  // namespace sng
