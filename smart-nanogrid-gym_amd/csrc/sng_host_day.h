// sng_host_day.h -- the reference's day in host form: one env's day in the reference's own layout (DayView),
// the reference generator drawn from a host MT19937, the encoder into the per-charger-step word / aux / req
// planes the step kernels read (sng_layout.h) and its inverse.  Host only, no HIP: it compiles with plain g++
// (tests/native/host_day_check.cpp runs the encoder against the decoder on the CPU).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "sng.h"
#include "sng_layout.h"
#include "sng_mt.h"

namespace sng {

static inline bool in_list(const int32_t *l, int n, int v) {
    for (int i = 0; i < n; ++i)
        if (l[i] == v) return true;
    return false;
}

static inline int list_len(const int32_t *l, int V) {
    int n = 0;
    while (n < V && l[n] >= 0) ++n;
    return n;
}

// One day of one environment in the reference's layout.
struct DayView {
    double *soc, *occ, *cap, *req;   // [N][S]
    int32_t *arr, *dep;              // [N][V], -1 padded
    int V;
    int S;                           // slots per charger: 25 (charger.py:16-19), T+1 with extended_day
};

// ChargingStation.generate_initial_vehicle_presence_per_charger and the draws it makes
// (charging_station.py:200-279), clear_initialisation_variables first (:138-150).
static inline bool generate_day(const SngConfig &c, int T, MT19937 &rng, DayView d) {
    const int N = c.number_of_chargers;
    const double dt = c.time_interval_hours;
    const int S = d.S;
    std::fill(d.soc, d.soc + N * S, 0.0);
    std::fill(d.occ, d.occ + N * S, 0.0);
    std::fill(d.cap, d.cap + N * S, 0.0);
    std::fill(d.req, d.req + N * S, 0.0);
    std::fill(d.arr, d.arr + N * d.V, -1);
    std::fill(d.dep, d.dep + N * d.V, -1);
    for (int ch = 0; ch < N; ++ch) {
        double *soc = d.soc + ch * S, *occ = d.occ + ch * S, *cap = d.cap + ch * S, *req = d.req + ch * S;
        int32_t *arr = d.arr + ch * d.V, *dep_l = d.dep + ch * d.V;
        int na = 0;
        bool present = false, cap_gen = false, req_gen = false;
        int dep = 0;
        double cur_cap = 0, cur_req = 0;
        for (int t = 0; t < T; ++t) {
            if (!present) {
                const double r = rng.random();
                if ((r - 0.1) > 0.5 && t < T) {   // round(random.rand() - 0.1) == 1, :214-215
                    present = true;
                    soc[t] = rng.uniform(0.1, 0.9);                              // :257-259
                    {                                                            // discarded draw, :219
                        const double lo = soc[t] <= 0.9 ? soc[t] + 0.1 : 1.0;
                        (void)rng.uniform(lo, 1.0);
                    }
                    if (c.different_vehicle_capacities && !cap_gen) {
                        cur_cap = (double)rng.randint(15, 120);                  // :267-269
                        cap_gen = true;
                    } else if (!c.different_vehicle_capacities && !cap_gen) {
                        cur_cap = 40;
                        cap_gen = true;
                    }
                    if (c.requested_state_of_charge && !req_gen) {
                        const double lo = soc[t] <= 0.9 ? soc[t] + 0.1 : 1.0;   // :261-265
                        cur_req = rng.uniform(lo, 1.0);
                        req_gen = true;
                    } else if (!c.requested_state_of_charge && !req_gen) {
                        cur_req = 1.0;
                        req_gen = true;
                    }
                    if (na >= d.V) return false;
                    arr[na] = t;
                    // generate_random_vehicle_departure_time, :271-279
                    const int max_charging = t + (int)(10 / dt);
                    const int max_departing = T + (int)(1 / dt);
                    const int high = std::min(max_charging, max_departing);
                    const int low = t + (int)(4 / dt);
                    dep = (low >= high) ? low : (int)rng.randint(low, high);
                    dep_l[na] = dep;
                    ++na;
                }
            }
            if (present && t < dep) {
                occ[t] = 1;
                cap[t] = cur_cap;
                req[t] = cur_req;
            } else {
                present = false;
                occ[t] = 0;
                cap[t] = 0;
                cap_gen = false;
                cur_cap = 0.0;
                req[t] = 0;
                cur_req = 0;
                req_gen = false;
            }
        }
    }
    return true;
}

// Membership test of find_vehicles_for_penalty_check (charging_station.py:42-63, 79-90)
// for the list built by observe(t).
static inline bool penalty_window(int mode, const int32_t *deps, int nd, int t) {
    switch (mode) {
        case SNG_PENALTY_ON_DEPARTURE: return in_list(deps, nd, t + 1);
        case SNG_PENALTY_SPARSE:
            return in_list(deps, nd, t + 1) || in_list(deps, nd, t + 2) || in_list(deps, nd, t + 3);
        case SNG_PENALTY_DENSE: return true;
        default: return false;
    }
}

// Encode one env's day into the dense per-charger-step timeline (sng_layout.h).
// req_out may be null; need_req reports whether any penalised requested SoC differs from 1.0.
static inline bool encode_day(const Params &p, int64_t E, int64_t e, const DayView &d, uint32_t *word, double *aux,
                              double *req_out, double *pen0, bool *need_req, std::string &err) {
    const int N = p.n, T = p.T;
    double pen_t0 = 0.0;
    for (int c = 0; c < N; ++c) {
        const int S = d.S;
        const double *soc = d.soc + c * S, *occ = d.occ + c * S, *cap = d.cap + c * S, *req = d.req + c * S;
        const int32_t *arr = d.arr + c * d.V, *dep = d.dep + c * d.V;
        const int na = list_len(arr, d.V), nd = list_len(dep, d.V);
        for (int t = 0; t < T; ++t) {
            const double o = occ[t];
            if (o != 0.0 && o != 1.0) {
                err = "occupancy values must be 0 or 1";
                return false;
            }
            const bool occupied = (o == 1.0);
            const bool arrived = in_list(arr, na, t);
            const int prev = arrived ? t : (t >= 1 ? t - 1 : S - 1);   // python index t-1
            // SOC[prev] is the running value only when step t-1 wrote it (charger occupied at t-1)
            const bool running = !arrived && t >= 1 && occ[t - 1] == 1.0;
            uint32_t capv = 0, rem = 0;
            double a = 0.0;
            if (occupied) {
                const double cv = cap[prev];
                if (!(cv >= 1.0 && cv <= 255.0 && cv == std::floor(cv))) {
                    err = "vehicle capacities of occupied chargers must be integers in [1, 255]";
                    return false;
                }
                capv = (uint32_t)cv;
                if (t == 0 && !arrived) {
                    err = "charger occupied at t=0 without an arrival at t=0";
                    return false;
                }
                int found = -1;
                for (int v = 0; v < nd; ++v)
                    if (t <= dep[v]) {
                        found = dep[v] - t;
                        break;
                    }
                if (found < 0 || found > 255) {
                    err = "occupied charger without a departure time >= t (or > 255 steps ahead)";
                    return false;
                }
                rem = (uint32_t)found;
                a = running ? 0.0 : soc[prev];
            } else {
                a = soc[t];
            }
            bool pen = false;
            if (t >= 1 && occ[t - 1] != 0.0) pen = penalty_window(p.penalty_mode, dep, nd, t - 1);
            const size_t idx = ((size_t)t * N + c) * (size_t)E + (size_t)e;
            word[idx] = pack_word(occupied, !running, pen, capv, rem);
            aux[idx] = a;
            if (pen && req[t - 1] != 1.0) *need_req = true;
            // Requested_SOC[c, t-1]; slot 0 keeps Requested_SOC[c, T-1] (sng_layout.h)
            if (req_out) req_out[idx] = req[t >= 1 ? t - 1 : T - 1];
        }
        // penalty at t = 0 reads python index -1 (slot 24) of SOC / Requested_SOC (penaliser.py:59-69)
        if (occ[0] != 0.0 && penalty_window(p.penalty_mode, dep, nd, 0)) {
            const double rq = req[S - 1], cur = soc[S - 1];
            if (cur < rq - 0.05 * rq) {
                const double x = (rq - cur) * 10;
                pen_t0 += x * x;
            }
        }
    }
    *pen0 = pen_t0;
    return true;
}

// A device-RNG day's packed records as words and aux values: rec holds T + 1 planes of `plane` records
// (charger-major, unquadded), w and aux the T planes of the steps.  Step t's record is plane t + 1 (as a word:
// capacity and steps left in the word's fields); an arrival's SoC is carried by the record before it (plane
// t), and an empty charger shows 0.
static inline void records_to_words(const uint16_t *rec, size_t plane, int T, uint32_t *w, double *aux) {
    for (size_t i = 0; i < (size_t)T * plane; ++i) {
        const uint32_t r = rec[plane + i];
        const bool occ = (r & W_OCC) != 0;
        w[i] = occ ? pack_word(true, (r & W_STATIC) != 0, (r & W_PEN) != 0, rec_cap(r), rec_dep(r)) : (r & W_PEN);
        aux[i] = (occ && (r & W_STATIC)) ? (double)rec_soc(rec[i]) : 0.0;
    }
}

// Inverse of encode_day / generate_kernel for env column k of [T][N][pitch] planes: the word stream gives
// occupancy, capacity and (at each arrival, W_STATIC on an occupied step) the departure; aux gives the
// arrival SoC and the SOC[c, t] of empty chargers; the req stream (rq, null when the day has none) holds
// Requested_SOC[c, t-1] at t >= 1 and Requested_SOC[c, T-1] at t = 0.  n_vehicles: [N], the arrivals of each
// charger (those past d.V are counted, not listed).
static inline void decode_day(const Params &p, size_t pitch, size_t k, const uint32_t *w, const double *aux,
                              const double *rq, const DayView &d, int32_t *n_vehicles) {
    const int N = p.n, T = p.T, S = d.S, V = d.V;
    std::fill(d.soc, d.soc + (size_t)N * S, 0.0);
    std::fill(d.occ, d.occ + (size_t)N * S, 0.0);
    std::fill(d.cap, d.cap + (size_t)N * S, 0.0);
    std::fill(d.req, d.req + (size_t)N * S, 0.0);
    std::fill(d.arr, d.arr + (size_t)N * V, -1);
    std::fill(d.dep, d.dep + (size_t)N * V, -1);
    for (int c = 0; c < N; ++c) {
        int nv = 0;
        for (int t = 0; t < T; ++t) {
            const size_t i = ((size_t)t * N + c) * pitch + k;
            const uint32_t word = w[i];
            const bool occ = (word & W_OCC) != 0;
            const size_t o = (size_t)c * S + t;
            if (occ) {
                d.occ[o] = 1.0;
                d.cap[o] = (double)((word >> W_CAP_SHIFT) & 0xffu);
                if (word & W_STATIC) {   // arrival: SOC[c, t] as generated, departure t + remaining
                    d.soc[o] = aux[i];
                    if (nv < V) {
                        d.arr[(size_t)c * V + nv] = t;
                        d.dep[(size_t)c * V + nv] = t + (int)((word >> W_DEP_SHIFT) & 0xffu);
                    }
                    ++nv;
                }
            } else {
                d.soc[o] = aux[i];
            }
            if (rq)
                d.req[o] = rq[((t + 1 < T ? (size_t)(t + 1) * N : 0) + c) * pitch + k];
            else   // a replayed day keeps the cleared zeros (charging_station.py:138-150)
                d.req[o] = (occ && !p.req_zero) ? 1.0 : 0.0;
        }
        n_vehicles[c] = nv;
    }
}

// `episodes` days of num_envs envs as the reference draws them, env i from np.random.seed(seed + i) and
// random.seed(seed + i): `out` holds the arrays of day 0, env 0 (day ep of env i follows at index
// ep * num_envs + i), pv_ratio one value per day.  False: a charger had more than out.V vehicles in a day.
static inline bool generate_scenarios(const SngConfig &cfg, int T, int64_t num_envs, uint64_t seed, int32_t episodes,
                                      const DayView &out, double *pv_ratio) {
    const int N = cfg.number_of_chargers, S = out.S, V = out.V;
    bool overflow = false;
    for (int64_t i = 0; i < num_envs; ++i) {
        MT19937 np_rng, py_rng;
        np_rng.seed_numpy((uint32_t)(seed + (uint64_t)i));
        py_rng.seed_python(seed + (uint64_t)i);
        for (int ep = 0; ep < episodes; ++ep) {
            if (ep > 0) (void)py_rng.py_randint(0, 180);   // day-end draw, smart_nanogrid_environment.py:181
            const size_t k = (size_t)ep * num_envs + i;
            DayView d{out.soc + k * N * S, out.occ + k * N * S, out.cap + k * N * S, out.req + k * N * S,
                      out.arr + k * N * V, out.dep + k * N * V, V, S};
            if (!generate_day(cfg, T, np_rng, d)) overflow = true;
            pv_ratio[k] = (double)py_rng.py_randint(0, 180) / 100;
        }
    }
    return !overflow;
}

}  // namespace sng
