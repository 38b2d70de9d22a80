// sng_dev_env.h -- one env's step arithmetic, shared by the three step kernels and the t = 0 observation kernels:
// the observation header, the profile-factor hash streams, one charger's step (charger_step), the
// BESS step, the env tail (grid, cost, reward, flags, diagnostics) and this step's table constants.
// Needs sng.h / sng_layout.h (Params, DeviceState, InfoPtrs, Tables, the word / record fields) and
// sng_dev_util.h (bld / bst, kNT, v2u).  Included by sng_kernels.hip only.
#pragma once

namespace sng {

// Observation header (smart_nanogrid_environment.py:190-231, central_management_system.py:53-60):
// [solar(t), price(t), solar(t+1..t+3), price(t+1..t+3)] with PV, [price(t), price(t+1..t+3)] without.
// irr / pn point at irr_norm[t] / price_norm[t] (the step kernel's LDS copy, or the tables);
// fpv / fpr are the env's profile factors for t..t+3 (1.0 without stochastic profiles).
__device__ __forceinline__ void write_obs_header(float *o, const Params &p, const double *irr, const double *pn,
                                                 double ratio, const double *fpv, const double *fpr) {
    int k = 0;
    if (p.pv) o[k++] = (float)((irr[0] * ratio) * fpv[0]);
    o[k++] = (float)(pn[0] * fpr[0]);
    if (p.pv) {
#pragma unroll
        for (int j = 1; j <= 3; ++j) o[k++] = (float)((irr[j] * ratio) * fpv[j]);
    }
#pragma unroll
    for (int j = 1; j <= 3; ++j) o[k++] = (float)(pn[j] * fpr[j]);
}

// The same header for the default station (PV, no stochastic profiles: every factor is 1.0 and x * 1.0 is x), for
// day_station_kernel: the four price entries do not depend on the env, so the caller has them as float32 already
// (pnf[j] = (float)price_norm[t + j], the value the product by 1.0 rounds to).
__device__ __forceinline__ void write_obs_header_station(float *o, const double *irr, const float *pnf, double ratio) {
    o[0] = (float)(irr[0] * ratio);
    o[1] = pnf[0];
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
        o[1 + j] = (float)(irr[j] * ratio);
        o[4 + j] = pnf[j];
    }
}

// ---------------------------------------------------------------------------------
// Counter-based 32-bit hash streams (device generator, stochastic profiles).  The oracle
// restates mix32 / stream_key / profile_factor bit for bit (oracle/sng_oracle.c).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint32_t x) {   // "triple32" integer hash (bijective)
    x ^= x >> 17;
    x *= 0xed5ad4bbu;
    x ^= x >> 11;
    x *= 0xac4c1b51u;
    x ^= x >> 15;
    x *= 0x31848babu;
    x ^= x >> 14;
    return x;
}

// Stream key of (seed, global env, charger | domain, day).
__device__ __forceinline__ uint32_t stream_key(uint64_t seed, uint64_t ge, uint32_t lane, uint64_t day) {
    const uint32_t k0 = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + (uint32_t)day * 0x9e3779b9u));
    const uint32_t k1 = mix32(k0 ^ (uint32_t)ge);
    return mix32(k1 ^ ((uint32_t)(ge >> 32) * 0x85ebca6bu + lane * 0xc2b2ae35u + 0x27d4eb2fu));
}

constexpr uint32_t kDomainPV = 0x50560000u;
constexpr uint32_t kDomainPrice = 0x50520000u;

// Build-defined stochastic profile factor 1 + sigma * z, z = h * 2^-31 - 1 in [-1, 1), of table
// entry k for the env with seed env_seed on day `day` (SngConfig.pv_noise / price_noise).
// The same from the day's key of the env and domain, stream_key(env_seed, 0, domain, day): what a reset keeps
// per env (DeviceState::prof_key) and the step kernels expand (round 4; round 3 stored every factor, 1.6 KB
// per env and day at config 5, and loaded 64 B per env-step).  sigma = 0 gives 1.0 exactly.
__device__ __forceinline__ double profile_factor_key(uint32_t key, int k, double sigma) {
    if (sigma == 0.0) return 1.0;
    const uint32_t h = mix32(key + (uint32_t)k * 0x9e3779b9u);
    const double z = (double)h * 0x1.0p-31 - 1.0;
    return 1.0 + sigma * z;
}
__device__ __forceinline__ double profile_factor(uint64_t env_seed, uint32_t domain, uint64_t day, int k,
                                                 double sigma) {
    return profile_factor_key(stream_key(env_seed, 0, domain, day), k, sigma);
}
// The day's profile keys of an env (PV, price) from DeviceState::prof_key ([E][2] u32, one 8 B load).
__device__ __forceinline__ v2u profile_keys(const DeviceState &s, uint32_t el8) {
    return __builtin_bit_cast(v2u, bld(reinterpret_cast<const uint64_t *>(s.prof_key), el8));
}
// The factors of t..t+3 from the day's keys (the day kernel loads the keys once a day).
__device__ __forceinline__ void expand_profile_factors(const Params &p, v2u kk, int t, double *fpv, double *fpr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        fpv[j] = profile_factor_key(kk.x, t + j, p.pv_noise);
        fpr[j] = profile_factor_key(kk.y, t + j, p.price_noise);
    }
}
__device__ __forceinline__ void profile_factors(const Params &p, const DeviceState &s, uint32_t el8, int t,
                                                double *fpv, double *fpr) {
    expand_profile_factors(p, profile_keys(s, el8), t, fpv, fpr);
}

// Per-step constants staged in LDS by the step kernel: irr_norm[t..t+3], price_norm[t..t+3],
// pv_power[t], price[t].
enum { CST_IRR = 0, CST_PN = 4, CST_PV = 8, CST_PRICE = 9, CST_COUNT = 10 };
__host__ __device__ inline double step_constant(const Tables *tb, int t, int i) {
    return i < CST_PN ? tb->irr_norm[t + i]
                      : i < CST_PV ? tb->price_norm[t + i - CST_PN] : i == CST_PV ? tb->pv_power[t] : tb->price[t];
}

// The same through the constant address space, for a kernel that stores between its steps (day_wide_kernel): no
// kernel writes the tables, but the compiler cannot know that once the kernel has stored anything, and then
// turns a uniform load of them into a vector load: 20 VGPRs per step's constants, counted in vmcnt between the
// step's other loads and stores.  Constant-address-space loads are scalar loads (the scalar cache, lgkmcnt).
__device__ __forceinline__ double step_constant_scalar(const Tables *tb, int t, int i) {
    typedef const __attribute__((address_space(4))) double *ConstF64;
    const double *q = i < CST_PN ? &tb->irr_norm[t + i]
                                 : i < CST_PV ? &tb->price_norm[t + i - CST_PN] : i == CST_PV ? &tb->pv_power[t] : &tb->price[t];
    return *(ConstF64)(uintptr_t)q;
}

// Remaining time to departure / 24 (smart_nanogrid_environment.py:207-208) as float32.
// The reference rounds d / 24 in float64 and then to float32; for integers d < 256 that equals the
// correctly rounded float32 quotient (d/24 is never a float32 rounding midpoint), which
// q = d*r; q + fma(-q, 24, d)*r reproduces for every d < 256 (checked exhaustively).
template <bool PK = false>   // PK: a packed record's steps-left field (bits 10-15; the record is zero-extended)
__device__ __forceinline__ float departure_obs(uint32_t w) {
    const float d = PK ? (float)(w >> P_DEP_SHIFT) : (float)((w >> W_DEP_SHIFT) & 0xffu);
    constexpr float r24 = 1.0f / 24.0f;
    const float q = d * r24;
    return __builtin_fmaf(__builtin_fmaf(-q, 24.0f, d), r24, q);
}

// x / c for a float32-valued x and an integer c in [1, 255] with r = fl(1/c):
// q = x*r, remainder fma(-q, c, x) (exact), q' = fma(rem, r, q).  x/c is never a float64
// rounding midpoint and lies >= ulp/(2c) from one, while q' differs from x/c by < 2^-50 ulp,
// so q' is the correctly rounded quotient -- bitwise equal to x / c.  Checked exhaustively for
// every float32 mantissa and every c (tools/check_division.c; scaling by 2^k is exact).
// That argument is about finite x, and the callers pass a magnitude: x >= +0.0 or NaN (charger_step takes the
// sign off a discharging product and subtracts the quotient; IEEE division is symmetric in the sign).
// x = +inf (the float32 charging product of an action of about 1.6e37 / dt and above overflows) has q = inf and
// the remainder inf - inf = NaN, where x / c is inf.  So the remainder goes through min(remainder, q): for a
// finite x the remainder (at most 2^-44 x) is below q >= x / 255, or both are +0, and it passes unchanged; for
// x = inf v_min_f64 returns its other operand for the NaN, q = inf, and fma(inf, r, inf) is inf.  q is live
// until the last fma anyway: no constant, no further register.  A NaN x stays NaN.
__device__ __forceinline__ double div_by_cap(double x, double c, double r) {
    const double q = x * r;
    return __builtin_fma(__builtin_fmin(__builtin_fma(-q, c, x), q), r, q);
}

// 1/c for an integer capacity c in [1, 255]: v_rcp_f64 and one Newton step.  div_by_cap needs only a
// relative error far below 2^-31 here (its quotient then errs by < 2^-62 relative before the last
// rounding, which x/c's distance from a rounding midpoint, >= 2^-62, absorbs): v_rcp_f64's error
// squared by the Newton step is ~2^-46.  c = 0 (empty charger) gives NaN, which charger_step selects away.
__device__ __forceinline__ double recip_cap(double c) {
    const double r0 = __builtin_amdgcn_rcp(c);
    return __builtin_fma(r0, __builtin_fma(-c, r0, 1.0), r0);
}

// ---------------------------------------------------------------------------------
// One charger, one step: penalty term of the vehicle present at t-1 and the EV update.
// penalise_charging_vehicles_outside_bounds (penaliser.py:39-57, 71-87): SoC and requested
// SoC at python index t-1.  Charger.charge_or_discharge_vehicle (charger.py:37-56, 58-94,
// 108-144) and reset_info_values (:146-156).
// ---------------------------------------------------------------------------------
struct ChargerResult {
    double pw;      // charger power value (kW), f64 array element of charging_station.py:282
    double q;       // insufficient-charge penalty term (0 if not checked / not insufficient)
    double soc;     // SOC[c, t] after the step
    uint32_t nx;    // 1: non-zero action on an empty charger (100 penalty points, diagnostics only)
    uint32_t fl;
};

// Written with selects rather than branches so the chargers of an env interleave (ILP hides the
// f64 latency at one wavefront per SIMD); the general variant keeps a (divergent) branch for the
// inverted-flag discharge division when dt is not a power of two.  Occupied chargers have cap in [1, 255]
// (validated when a scenario is encoded).
// FAST (NumPy-2 promotion and dt a power of two, e.g. the 1 h default) is straight-line code, so the
// compiler interleaves the chargers of an env.
// NONNEG: the caller knows a >= +0.0 (not NaN, not -0.0; +inf and anything above the Box included, no action is
// clipped): the wide kernel's fast loop, which a wavefront takes only when none of its actions is negative, -0.0
// or NaN.  An action whose float32 product overflows charges to SoC 1.0 and bills +inf (div_by_cap keeps the
// infinite quotient).  Then a vehicle either charges (a > 0) or idles, so the discharge
// branch -- the inverted-flag power (charger.py:122-132) and max(0, calc) -- is never selected and is not
// computed; every value this returns equals the general form's for such actions.
// PK: w is a device-RNG day's packed record (its capacity in bits 3-9), else a word.
template <bool FAST, bool NONNEG = false, bool PK = false>
__device__ __forceinline__ ChargerResult charger_step(const Params &p, uint32_t w, double aux, double run, double req,
                                                      float a, int t, double rcap) {
    ChargerResult o;
    SNG_DIAG_CHARGER(o, aux, run, a);
    const double margin = 0.05 * req;
    const double d = (req - run) * 10;
    const bool insufficient = (t > 0) && (w & W_PEN) && (run < req - margin);
    o.q = insufficient ? d * d : 0.0;

    const bool occ = (w & W_OCC) != 0;
    // previous SoC of an occupied charger, or the recorded SOC[c, t] of an empty one
    const double prev = (occ && !(w & W_STATIC)) ? run : aux;
    const uint32_t capi = cap_field<PK>(w);
    const double cap = (double)capi;
    const bool idle = (a == 0.0f);
    const bool chg = (a > 0.0f);
    // calc: the SoC a charging action computes, prev + change; calc_dis: what a discharging action (a < 0, or NaN)
    // computes, prev + change as well, from the magnitude of its change
    static_assert(FAST || !NONNEG, "the NONNEG form is the wide kernel's: NumPy-2 promotion");
    double pc, calc, calc_dis;
    float pf = 0.0f;   // the float32 power (NumPy 2)
    if (!FAST && p.legacy) {   // NumPy < 2: float32 scalar * int -> float64 (float64 numerator: plain division)
        pc = ((double)a * p.ev_power) * p.ev_eff;
        calc = calc_dis = prev + (pc * p.dt) / cap;
    } else {          // NumPy 2 (NEP 50): float32 product
        pf = __fmul_rn(__fmul_rn(a, p.ev_power_f), p.ev_eff_f);
        const float pdt = __fmul_rn(pf, p.dt_f);
        pc = (double)pf;
        // exact reciprocal-fma division with rcap ~ 1/c (the LDS table, or recip_cap): the IEEE quotient, +-inf
        // for an infinite product
        const double mag = div_by_cap(NONNEG ? (double)pdt : __builtin_fabs((double)pdt), cap, rcap);
        calc = prev + mag;
        calc_dis = prev - mag;
    }
    if constexpr (NONNEG) {   // a > 0 charges, a == 0 idles (chg == !idle)
        const bool moved = occ && chg && p.bounded;
        o.soc = moved ? ((1.0 < calc) ? 1.0 : calc) : prev;
        o.pw = (double)(moved ? pf : 0.0f);   // pc or 0.0, selected before the conversion: one select, not two
        o.nx = (!occ && chg) ? 1u : 0u;
        o.fl = (occ && chg && !p.bounded) ? (uint32_t)SNG_FLAG_CHARGING_MODE : 0u;
        return o;
    }
    // inverted flag, charger.py:122-132: ceil(0.5 * (1 + sign(calc))) * 22 is 0 only for calc < 0; a NaN calc (a
    // NaN action) makes it NaN, which `if` takes for true, so a NaN action bills the finite clamp power
    double pw_dis = pc;
    if (FAST) {
        pw_dis = !(calc_dis < 0.0) ? -((prev * cap) * p.rdt) : pc;
    } else if (occ && !idle && !chg && !(calc_dis < 0.0)) {
        const double x = prev * cap;
        pw_dis = -(p.dt_pow2 ? x * p.rdt : x / p.dt);
    }
    const double soc_chg = (1.0 < calc) ? 1.0 : calc;           // min(calc, 1.0)
    const double soc_dis = (calc_dis > 0.0) ? calc_dis : 0.0;   // max(0.0, calc)
    const bool moved = occ && !idle && p.bounded;
    o.soc = moved ? (chg ? soc_chg : soc_dis) : prev;
    o.pw = moved ? (chg ? pc : pw_dis) : 0.0;                   // full power billed when charging
    o.nx = (!occ && !idle) ? 1u : 0u;
    o.fl = (occ && !idle && !p.bounded) ? (uint32_t)SNG_FLAG_CHARGING_MODE : 0u;
    return o;
}

// ---------------------------------------------------------------------------------
// One charger's visit by a step kernel: charger_step on the charger's record as the kernel loaded it, and what
// every kernel then writes for that charger.  What a packed (device-RNG) day's record means is said here and
// nowhere else (sng_layout.h has the format):
//   - an arriving vehicle's SoC is the running SoC the step before stored (the record it carried), so the step
//     sees no STATIC bit and no aux plane (aux is not read);
//   - an empty charger's SoC state is the record's own SoC field, and its departure entry is that of a record
//     without steps left.
// The caller stores `soc` where and how its layout has it, writes the two observation entries, and keeps the
// sums of r.pw, r.q, r.nx and r.fl in its own order.  1 / capacity is recip_cap's, or with TABLE the entry of
// the caller's table by capacity (the general kernel stages one in LDS for N <= 16); both are exact (div_by_cap).
// ---------------------------------------------------------------------------------
template <bool PK>
struct ChargerVisit {
    ChargerResult r;
    double soc;       // the charger's SoC state after the step
    uint32_t w_dep;   // the record whose steps-left field the observation shows
    // the charger's observation entries: SOC[c, t] and the time to departure / 24
    __device__ __forceinline__ float obs_soc() const { return (float)r.soc; }
    __device__ __forceinline__ float obs_dep() const { return departure_obs<PK>(w_dep); }
};
template <bool FAST, bool NONNEG, bool PK, bool TABLE = false>
__device__ __forceinline__ ChargerVisit<PK> visit_charger(const Params &p, uint32_t w, const double &aux, double run,
                                                          double req, float a, int t, const double *rcp_table = nullptr) {
    const uint32_t capi = cap_field<PK>(w);
    const bool occ = (w & W_OCC) != 0;
    ChargerVisit<PK> v{charger_step<FAST, NONNEG, PK>(p, PK ? (w & ~W_STATIC) : w, PK ? 0.0 : aux, run, req, a, t,
                                                      TABLE ? rcp_table[capi] : recip_cap((double)capi)),
                       0.0, (PK && !occ) ? 0u : w};
    v.soc = (PK && !occ) ? (double)rec_soc(w) : v.r.soc;
    return v;
}

// ---------------------------------------------------------------------------------
// The BESS step of an env (central_management_system.py:93-94, battery_energy_storage_system.py:30-106,
// penaliser.py:104-111): the new SoC (stored), its penalty and powers, and what it adds to the grid
// balance.  It needs only the BESS SoC and action, not the chargers, so the wide step kernel runs it
// before the charger loop (while the chargers' loads are in flight); env_tail runs it in place otherwise.
// STORE = false (the day kernel): the new SoC stays with the caller (BessStep::bess), who stores it after the
// day's last step; the day's initial SoC (bess0, t = 0) is stored either way.
// ---------------------------------------------------------------------------------
struct BessStep {
    double bess, pen_b, bpow, bcalc, pw, dp;
    bool moved, chg;
    uint32_t fl;
};
template <bool STORE = true>
__device__ __forceinline__ BessStep bess_step(const Params &p, const DeviceState &s, uint32_t el8, int t, double bess,
                                              float bess_action) {
    BessStep b{bess, 0.0, 0.0, 0.0, 0.0, 0.0, false, false, 0u};
    if (!p.bess) return b;
    if (t == 0) bst(s.bess0, el8, bess);                       // :93-94
    // charge (ba > 0, battery_energy_storage_system.py:46-74) and discharge (ba < 0, :76-106) share one
    // select-based path with one division: the two branches differ only in their constants, the
    // over-discharge clamp and the SoC bound
    const double ba = (double)bess_action;
    b.chg = ba > 0.0;
    b.pw = (ba * (b.chg ? p.bess_pmax_ch : p.bess_pmax_dis)) * (b.chg ? p.bess_eff_ch : p.bess_eff_dis);
    const double calc = bess + (b.pw * p.dt) / p.bess_cap;
    const double empty = bess * p.bess_cap;   // the over-discharge clamp's energy
    // :82-94: the flag 1 - ceil(0.5 * (1 + sign(calc))) is 0 only for calc >= 0; NaN for a NaN action, and true
    b.dp = !(calc >= 0.0) ? -(p.dt_pow2 ? empty * p.rdt : empty / p.dt) : b.pw;
    if (ba == 0.0) {
        b.bpow = 0.0;
        b.bcalc = 0.0;
    } else if (!p.bounded) {
        b.fl |= SNG_FLAG_CHARGING_MODE;
    } else {
        b.moved = true;
        b.bcalc = b.pw;
        b.bess = b.chg ? ((1.0 < calc) ? 1.0 : calc) : ((calc > 0.0) ? calc : 0.0);
        b.bpow = b.chg ? b.pw : b.dp;
    }
    if (b.bess < p.bess_dod) {                                 // penaliser.py:104-111
        const double d = (p.bess_dod - b.bess) * 10;
        b.pen_b = d * d;
    } else if (!(b.bess <= 1.0)) {
        b.fl |= SNG_FLAG_BESS_SOC_ABOVE_1;
    }
    if constexpr (STORE) bst<kNT>(s.bess, el8, b.bess);
    return b;
}

// ---------------------------------------------------------------------------------
// Env tail: BESS (unless PRE: bess_step ran before the chargers), grid energy, cost, reward
// (central_management_system.py:99-185, penaliser.py:177-187, accountant.py:26-40) and the observation's
// BESS entry.  Leader lane only.  KEEP (the day kernel, with PRE): the day return so far goes to *ret_keep instead
// of memory.
// ---------------------------------------------------------------------------------
static_assert((SNG_FLAG_NEGATIVE_DEMAND | SNG_FLAG_CHARGING_MODE | SNG_FLAG_BESS_SOC_ABOVE_1 | SNG_FLAG_V2X_BREAKPOINT) == 0xfu,
              "env_tail ORs the flag summary bit by bit: bits 0-3");
template <bool DIAG, bool PRE = false, bool KEEP = false>
__device__ __forceinline__ void env_tail(const Params &p, const DeviceState &s, const InfoPtrs &info, int64_t e0, uint32_t lo, uint32_t el1, uint32_t el8,
                                         int t, double ratio, double bess, float bess_action, double p_ch,
                                         double p_dis, double pen_v, double nonexist, uint32_t fl, float *o_row,
                                         const double *cst, const double *fpv, const double *fpr, double ret_prev,
                                         double bess0, double *__restrict__ reward, uint8_t *__restrict__ done,
                                         const BessStep *pre = nullptr, double *ret_keep = nullptr) {
    // no global loads in here: a load would wait (vmcnt) for every SoC store the env just issued
    const double solar = p.pv ? (cst[CST_PV] * ratio) * fpv[0] : 0.0;   // central_management_system.py:99-103
    const double demand = p_ch + p_dis;                            // :105
    if (demand < 0.0) fl |= p.v2x ? SNG_FLAG_V2X_BREAKPOINT : SNG_FLAG_NEGATIVE_DEMAND;
    double rem = demand - solar;                                   // :167

    if (p.bess && t == 0) bess0 = bess;
    const BessStep b = PRE ? *pre : bess_step(p, s, el8, t, bess, bess_action);
    fl |= b.fl;
    if (b.moved) rem = b.chg ? -((-rem) - b.pw) : rem + b.dp;     // battery_energy_storage_system.py:46-106
    const double pen_b = b.pen_b, bpow = b.bpow, bcalc = b.bcalc;
    bess = b.bess;

    const double grid = rem;
    const double energy = grid * p.dt;
    const double price = cst[CST_PRICE] * fpr[0];
    const double cost = (energy < 0.0) ? (energy * p.sell_coef) * price : energy * price;
    const double tot_pen = p.bat_pen_w * pen_b + pen_v;
    const double total = p.grid_w * fabs(cost) + tot_pen;
    bst<kNT>(reward, el8, -total);
    bst<kNT>(done, el1, (uint8_t)((t + 1 == p.T) ? 1 : 0));

    // (the observation header was written before the chargers: step_kernel)
    if (p.bess && !PRE) o_row[p.obs_dim - 1] = (float)bess;

    if (fl) atomicOr(s.flags + e0 + lo, fl);   // sticky per-env error bits; no-return atomics, nothing waits
    // the flag summary (SngInfo.flag_summary): the wavefront's active lanes' bits ORed by one ballot per flag
    // bit (four: sng.h), then one atomic per wavefront into the wavefront's own word.  A V2X station flags
    // most envs on most steps: one atomic per flagged env into one shared word cost 18.9 us per
    // step at N = 10, one per wavefront into that word 17.6 us -- the device-scope atomics on one address run
    // one after another at the memory side, and the last wavefronts waited ~10 us for theirs
    // (profiles/r05_stamps_v2x.txt) -- and one per wavefront into its own word 7.1 us.  A wavefront without a
    // flag pays one ballot.
    if (info.flag_any && __builtin_amdgcn_ballot_w64(fl != 0u)) {
        uint32_t any = 0u;
#pragma unroll
        for (uint32_t b = 1u; b <= SNG_FLAG_V2X_BREAKPOINT; b <<= 1)
            any |= __builtin_amdgcn_ballot_w64((fl & b) != 0u) ? b : 0u;
        if (__lane_id() == (unsigned)__builtin_ctzll(__builtin_amdgcn_read_exec()))
            atomicOr(info.flag_any + ((uint32_t)(e0 >> 5) & (SNG_FLAG_SUMMARY_WORDS - 1)), any);
    }
    if (info.flags) bst(info.flags, el1 * 4u, fl);
    if constexpr (KEEP) *ret_keep = ret_prev + -total;
    else if (info.episode_return) bst<kNT>(info.episode_return, el8, ret_prev + -total);
    if (DIAG) {
        if (info.grid_power) bst(info.grid_power, el8, (double)(grid));
        if (info.p_charge) bst(info.p_charge, el8, (double)(p_ch));
        if (info.p_discharge) bst(info.p_discharge, el8, (double)(p_dis));
        if (info.bess_soc) bst(info.bess_soc, el8, (double)(p.bess ? bess : 0.0));
        if (info.pen_vehicle) bst(info.pen_vehicle, el8, (double)(pen_v));
        if (info.pen_battery) bst(info.pen_battery, el8, (double)(pen_b));
        if (info.grid_cost) bst(info.grid_cost, el8, (double)(cost));
        if (info.total_cost) bst(info.total_cost, el8, (double)(total));
        if (info.solar) bst(info.solar, el8, (double)(solar));
        if (info.bess_power) bst(info.bess_power, el8, (double)(bpow));
        if (info.bess_calc_power) bst(info.bess_calc_power, el8, (double)(bcalc));
        if (info.nonexistent) bst(info.nonexistent, el8, (double)(nonexist));
        if (info.bess_initial) bst(info.bess_initial, el8, (double)(p.bess ? bess0 : 0.0));
    }
}

// This step's table constants by value: a kernel argument of the lean and the wide step kernel (launch_step
// fills it), so their loads need no round trip through the tables pointer.
struct StepConst {
    double v[CST_COUNT];   // step_constant(tables, t, i) for i < CST_COUNT
};

// The NEP 50 float32 charging power of action a (charger.py:92-94), as charger_step computes it.
__device__ __forceinline__ double charging_power(const Params &p, float a) {
    return (double)__fmul_rn(__fmul_rn(a, p.ev_power_f), p.ev_eff_f);
}

// Requested_SOC[c, t-1] of a day without the stream: 1.0 (requested SoC disabled, charging_station.py:230-232),
// or the cleared 0.0 of a replayed day (sng_layout.h, Params::req_zero).
__device__ __forceinline__ double req_default(const Params &p) { return p.req_zero ? 0.0 : 1.0; }

// A device-RNG day's first step (PK, t = 0) advances the day counter its reset read (generate_kernel), as the
// last thing the lean and the wide step kernel do; a no-return atomic, so nothing waits for it.  A replayed day
// (bump_day = 0) drew no counter value of its own.
template <bool PK>
__device__ __forceinline__ void bump_day_counter(const Params &p, const DeviceState &s, int t) {
    if (PK && t == 0 && p.bump_day && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_fetch_add(s.episode, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace sng
