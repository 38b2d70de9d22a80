// sng_host_tables.h -- what a configuration becomes before any device is touched: the checked SngConfig, the
// reference's PV and price tables, the kernels' Params and Tables, and the checkpoint's configuration
// fingerprint.  Host only, no HIP: it compiles with plain g++.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sng.h"
#include "sng_layout.h"
#include "sng_step_plan.h"

namespace sng {

// numpy pairwise_sum (contiguous float64), used by ndarray.mean() in
// PVSystemManager.calculate_solar_irradiance_mean (pv_system_manager.py:34-44)
static inline double pairwise_sum(const double *a, long n) {
    if (n < 8) {
        double res = 0.0;
        for (long i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    long n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

struct HostTables {
    std::vector<double> irr, pv_power, price;
    double irr_max = 0, price_max = 0;
};

// PVSystemManager (pv_system_manager.py:10-91) and Accountant price tables (accountant.py:17-101)
static inline bool build_tables(const SngConfig &c, int T, HostTables &tb, std::string &err) {
    const double dt = c.time_interval_hours;
    const int steps_min = (int)(60 * dt);
    const int padded = 2 * T;
    if ((int64_t)padded * steps_min > c.irradiance_minutes) {
        err = "irradiance data too short for two days at this time interval";
        return false;
    }
    tb.irr.assign(padded, 0.0);
    tb.pv_power.assign(padded, 0.0);
    for (int k = 0; k < padded; ++k)
        tb.irr[k] = pairwise_sum(c.irradiance_per_minute + (int64_t)k * steps_min, steps_min) / (double)steps_min;
    double mx = 0.0;
    for (double v : tb.irr)
        if (v >= 0 && v > mx) mx = v;
    tb.irr_max = mx;
    const double scaling_pv = ((2.279 * 1.134) * 20) * 0.21 / 1000;   // PVSystem(...), pv_system_manager.py:17, :72-73
    for (int k = 0; k < padded; ++k) tb.pv_power[k] = ((tb.irr[k] * scaling_pv) * 1.5) / dt;

    const double high = (0.028 + 0.148933333) + 0.014;   // set_grid_tariffs, accountant.py:17-24
    const double low = (0.013333333 + 0.087613333) + 0.014;
    static const double m1[24] = {0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.1, 0.1, 0.1, 0.1, 0.1,
                                  0.1,  0.1,  0.1,  0.1,  0.1,  0.1,  0.1,  0.1, 0.05, 0.05, 0.05, 0.05};
    static const double m2[24] = {0.05, 0.05, 0.05, 0.05, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1,  0.1,  0.1,
                                  0.08, 0.06, 0.05, 0.05, 0.05, 0.06, 0.06, 0.06, 0.06, 0.05, 0.05, 0.05};
    static const double m3[24] = {0.071, 0.060, 0.056, 0.056, 0.056, 0.060, 0.060, 0.060, 0.066, 0.066, 0.076, 0.080,
                                  0.080, 0.1,   0.1,   0.076, 0.076, 0.1,   0.082, 0.080, 0.085, 0.079, 0.086, 0.070};
    static const double m4[24] = {0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.08, 0.08, 0.1,  0.1,  0.1,
                                  0.1, 0.1, 0.1,  0.1,  0.1,  0.06, 0.06, 0.06, 0.1,  0.1,  0.1,  0.1};
    double day[24];
    switch (c.price_model) {
        case 0:
            for (int h = 0; h < 24; ++h) day[h] = (h < 7 || h >= 20) ? low : high;   // accountant.py:69-73
            break;
        case 1: std::memcpy(day, m1, sizeof day); break;
        case 2: std::memcpy(day, m2, sizeof day); break;
        case 3: std::memcpy(day, m3, sizeof day); break;
        case 4: std::memcpy(day, m4, sizeof day); break;
        default:
            err = "price_model must be 0..4 (model 5 raises TypeError in accountant.py:90-98)";
            return false;
    }
    if (!c.extended_day) {
        tb.price.assign(kPriceLen, 0.0);
        for (int k = 0; k < kPriceLen; ++k) tb.price[k] = day[k % 24];   // concatenate([day, day]), accountant.py:100
    } else {
        // build-defined extended day: the per-step tariff loop of accountant.py:61-68 for model 0,
        // the hourly value of hour floor(i*dt) for models 1-4; concatenated twice
        tb.price.assign(2 * T, 0.0);
        for (int i = 0; i < T; ++i) {
            const double v = (c.price_model == 0) ? ((i < 7 / dt || i > 19 / dt) ? low : high)
                                                  : day[(int)std::floor(i * dt) % 24];
            tb.price[i] = v;
            tb.price[i + T] = v;
        }
    }
    mx = 0.0;
    for (double v : tb.price)
        if (v >= 0 && v > mx) mx = v;
    tb.price_max = mx;
    return true;
}

static inline int validate(const SngConfig *c, int *T_out, std::string &err) {
    if (!c) { err = "null config"; return SNG_ERR_INVALID_ARGUMENT; }
    if (c->abi_version != SNG_ABI_VERSION) { err = "SngConfig.abi_version mismatch"; return SNG_ERR_INVALID_ARGUMENT; }
    if (c->number_of_chargers < 1 || c->number_of_chargers > kMaxChargers) {
        err = "number_of_chargers must be in [1, 128]";
        return SNG_ERR_UNSUPPORTED;
    }
    const double dt = c->time_interval_hours;
    if (!(dt > 0)) { err = "Wrong time interval was provided"; return SNG_ERR_INVALID_ARGUMENT; }
    const double steps = 24.0 / dt;
    const int T = (int)steps;
    if ((double)T != steps) {
        err = "24h / time_interval must be an integer (the reference never ends the day otherwise)";
        return SNG_ERR_UNSUPPORTED;
    }
    if (T > 24 && !c->extended_day) {
        err = "time intervals below 1h are not runnable in the reference (25-slot arrays, charger.py:16-19); "
              "set extended_day for the build-defined extension";
        return SNG_ERR_UNSUPPORTED;
    }
    if (T > kMaxT) { err = "at most 128 steps per day"; return SNG_ERR_UNSUPPORTED; }
    if (!(c->pv_noise >= 0.0 && c->pv_noise <= 1.0) || !(c->price_noise >= 0.0 && c->price_noise <= 1.0)) {
        err = "pv_noise / price_noise must be in [0, 1]";
        return SNG_ERR_INVALID_ARGUMENT;
    }
    if (T < 4) { err = "time interval too long (fewer than 4 steps per day)"; return SNG_ERR_UNSUPPORTED; }
    if (c->penalty_mode < 0 || c->penalty_mode > 3) {
        err = "Error: Wrong vehicle uncharged - penalty mode provided!";
        return SNG_ERR_INVALID_ARGUMENT;
    }
    if (c->price_model < 0 || c->price_model > 4) { err = "price_model must be 0..4"; return SNG_ERR_UNSUPPORTED; }
    if (!c->irradiance_per_minute || c->irradiance_minutes <= 0) {
        err = "irradiance_per_minute is required";
        return SNG_ERR_INVALID_ARGUMENT;
    }
    *T_out = T;
    return SNG_OK;
}

// What the day generators take beside Params: 4 h, 10 h and 1 h in steps, and the per-charger array length
// of scenarios (25, charger.py:16-19; T + 1 with extended_day).
struct DaySpans {
    int i4, i10, i1, slots;
};
static inline int day_slots(const SngConfig &c, int T) { return c.extended_day ? T + 1 : kSlots; }

// The Params of a validated configuration with T steps a day; the four loaded-day fields stay zero (no day is
// loaded).  False: step_lanes_per_env is not available for this charger count.
static inline bool fill_params(const SngConfig &c, int T, uint64_t seed, Params &p, DaySpans &spans) {
    p.n = c.number_of_chargers;
    p.T = T;
    p.pv = c.pv_system_available ? 1 : 0;
    p.bess = c.battery_system_available ? 1 : 0;
    p.v2x = c.vehicle_to_everything ? 1 : 0;
    p.bounded = c.charging_mode_bounded ? 1 : 0;
    p.legacy = c.numpy_legacy_promotion ? 1 : 0;
    p.penalty_mode = c.penalty_mode;
    p.diff_caps = c.different_vehicle_capacities ? 1 : 0;
    p.req_enabled = c.requested_state_of_charge ? 1 : 0;
    p.obs_dim = (1 + p.pv) * 4 + 2 * p.n + p.bess;   // smart_nanogrid_environment.py:90-96
    p.act_dim = p.n + p.bess;                          // :101-118
    p.dt = c.time_interval_hours;
    p.dt_f = (float)c.time_interval_hours;
    {
        int ex = 0;
        p.dt_pow2 = (std::frexp(p.dt, &ex) == 0.5) ? 1 : 0;   // dt = 2^k: x / dt == x * 2^-k
        p.rdt = 1.0 / p.dt;
    }
    p.ev_power = c.ev_max_power_kw;
    p.ev_eff = c.ev_efficiency;
    p.ev_power_f = (float)c.ev_max_power_kw;
    p.ev_eff_f = (float)c.ev_efficiency;
    p.bess_cap = c.bess_capacity_kwh;
    p.bess_pmax_ch = c.bess_max_charging_kw;
    p.bess_pmax_dis = c.bess_max_discharging_kw;
    p.bess_eff_ch = c.bess_charging_efficiency;
    p.bess_eff_dis = c.bess_discharging_efficiency;
    p.bess_dod = c.bess_depth_of_discharge;
    p.grid_w = c.grid_cost_weight;
    p.bat_pen_w = c.battery_penalty_weight;
    p.sell_coef = c.selling_price_coefficient;
    if (c.step_lanes_per_env) {
        if (!station_lanes_supported(p.n, c.step_lanes_per_env)) return false;
        p.lanes = c.step_lanes_per_env;
    } else {
        // tuned on MI355X at E=65,536 (bench.py --lanes): 1 lane per env at N=10 (7.6 / 8.9 / 11.4 us
        // for 1 / 2 / 4 lanes) and at N=50, config 5 (38.9 / 42.1 / 51.9 us)
        p.lanes = 1;
    }
    spans.i4 = (int)(4 / p.dt);
    spans.i10 = (int)(10 / p.dt);
    spans.i1 = (int)(1 / p.dt);
    spans.slots = day_slots(c, T);
    p.noise = (c.pv_noise > 0.0 || c.price_noise > 0.0) ? 1 : 0;
    p.pv_noise = c.pv_noise;
    p.price_noise = c.price_noise;
    p.seed = seed;
    return true;
}

// The device tables (their host copy) of a configuration's HostTables
static inline void fill_tables(const HostTables &tb, Tables &ht) {
    std::memset(&ht, 0, sizeof ht);
    const int n_irr = (int)tb.irr.size();
    ht.n_irr = n_irr;
    for (int k = 0; k < n_irr; ++k) {
        ht.irr_norm[k] = tb.irr[k] / tb.irr_max;   // pv_system_manager.py:81-85
        ht.pv_power[k] = tb.pv_power[k];
    }
    for (int k = 0; k < (int)tb.price.size(); ++k) {
        ht.price[k] = tb.price[k];
        ht.price_norm[k] = tb.price[k] / tb.price_max;   // accountant.py:42-46
    }
    ht.recip[0] = 0.0;
    for (int c = 1; c < 256; ++c) ht.recip[c] = 1.0 / (double)c;
}

// FNV-1a over a byte range (the checkpoint's configuration fingerprint)
static inline uint64_t fnv1a(const void *data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

// The checkpoint's configuration fingerprint: every SngConfig field that changes the simulation, hashed
// field by field (the struct's padding and -0.0 vs 0.0 must not make an identical configuration differ
// across processes or bindings).  The irradiance enters through the tables, hashed next to it.
static inline uint64_t config_fingerprint(const SngConfig &c) {
    uint64_t h = 1469598103934665603ull;
    auto i32 = [&h](int32_t v) { h = fnv1a(&v, sizeof v, h); };
    auto f64 = [&h](double v) {
        if (v == 0.0) v = 0.0;   // -0.0 -> 0.0
        h = fnv1a(&v, sizeof v, h);
    };
    i32(c.abi_version);
    i32(c.number_of_chargers);
    f64(c.time_interval_hours);
    i32(c.price_model);
    i32(c.pv_system_available);
    i32(c.battery_system_available);
    i32(c.vehicle_to_everything);
    i32(c.different_vehicle_capacities);
    i32(c.requested_state_of_charge);
    i32(c.charging_mode_bounded);
    i32(c.penalty_mode);
    i32(c.numpy_legacy_promotion);
    for (double v : {c.grid_cost_weight, c.battery_penalty_weight, c.selling_price_coefficient, c.bess_capacity_kwh,
                     c.bess_initial_soc, c.bess_max_charging_kw, c.bess_max_discharging_kw, c.bess_charging_efficiency,
                     c.bess_discharging_efficiency, c.bess_depth_of_discharge, c.ev_max_power_kw, c.ev_efficiency})
        f64(v);
    i32(c.extended_day);
    f64(c.pv_noise);
    f64(c.price_noise);
    return h;
}

}  // namespace sng
