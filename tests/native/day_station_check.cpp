// CPU check of day_station_fixed / day_station_selected (csrc/sng_step_plan.h): which handles step their captured
// days with day_station_kernel (tests/test_day_station_kernel_cpu.py).  The Params are the library's own: a
// configuration goes through fill_params (sng_host_tables.h) and the loaded day's key through with_day
// (sng_state_format.h), as sng_create and a capture do.
//   day_station_check                 the headline station, then the headline with one fact flipped, one per line:
//                                     "<name> <fixed> <selected> <selected under generic_day>"
//   day_station_check N hours pv bess bounded v2x legacy req noise device replay
//                                     one station (a row of the station matrix): prints "<fixed>"
#include <cstdio>
#include <cstdlib>

#include "sng_host_tables.h"
#include "sng_state_format.h"
#include "sng_step_plan.h"

using namespace sng;

struct Station {
    int n = 10;
    double hours = 1.0;
    int pv = 1, bess = 1, bounded = 1, v2x = 0, legacy = 0, req = 0, noise = 0;
    int device = 1, replay = 0, diag = 0, lanes = 0;
};

static bool params_of(const Station &st, Params &p) {
    SngConfig c{};
    c.number_of_chargers = st.n;
    c.time_interval_hours = st.hours;
    c.pv_system_available = st.pv;
    c.battery_system_available = st.bess;
    c.charging_mode_bounded = st.bounded;
    c.vehicle_to_everything = st.v2x;
    c.numpy_legacy_promotion = st.legacy;
    c.requested_state_of_charge = st.req;
    c.pv_noise = st.noise ? 0.2 : 0.0;
    c.extended_day = st.hours < 1.0;
    c.step_lanes_per_env = st.lanes;
    c.ev_max_power_kw = 22;
    c.ev_efficiency = 0.95;
    DaySpans spans{};
    p = Params{};
    if (!fill_params(c, (int)(24.0 / st.hours), 1, p, spans)) return false;
    DayKey k = st.device ? DayKey::device_day(p) : DayKey::host_day(st.req != 0);
    if (st.replay) k = k.replayed();
    p = with_day(p, k);
    return true;
}

static int fixed_of(const Station &st) {
    Params p;
    if (!params_of(st, p)) return -1;
    return day_station_fixed(step_plan(p, st.diag != 0), p) ? 1 : 0;
}

static int line(const char *name, const Station &st, int want) {
    Params p;
    if (!params_of(st, p)) return 1;
    const StepPlan pl = step_plan(p, st.diag != 0);
    const int fixed = day_station_fixed(pl, p) ? 1 : 0;
    printf("%s %d %d %d\n", name, fixed, (int)day_station_selected(pl, p, false), (int)day_station_selected(pl, p, true));
    // the selection never reaches past the predicate, and generic_day always keeps the generic kernel
    if (day_station_selected(pl, p, true)) return 1;
    if (day_station_selected(pl, p, false) != (fixed != 0 && day_station_faster())) return 1;
    return fixed == want ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 12) {
        Station st;
        st.n = atoi(argv[1]);
        st.hours = atof(argv[2]);
        int *f[] = {&st.pv, &st.bess, &st.bounded, &st.v2x, &st.legacy, &st.req, &st.noise, &st.device, &st.replay};
        for (int i = 0; i < 9; ++i) *f[i] = atoi(argv[3 + i]);
        const int r = fixed_of(st);
        if (r < 0) return 2;
        printf("%d\n", r);
        return 0;
    }
    if (argc != 1) return 2;
    int bad = 0;
    Station h;
    bad += line("headline", h, 1);
    auto flip = [&](const char *name, auto set) {
        Station st;
        set(st);
        bad += line(name, st, 0);
    };
    flip("unbounded", [](Station &s) { s.bounded = 0; });
    flip("v2x", [](Station &s) { s.v2x = 1; });
    flip("no_pv", [](Station &s) { s.pv = 0; });
    flip("no_bess", [](Station &s) { s.bess = 0; });
    flip("legacy", [](Station &s) { s.legacy = 1; });
    flip("requested_soc", [](Station &s) { s.req = 1; });
    flip("noise", [](Station &s) { s.noise = 1; });
    flip("replayed", [](Station &s) { s.replay = 1; });
    flip("replayed_requested_soc", [](Station &s) { s.req = s.replay = 1; });
    flip("host_day", [](Station &s) { s.device = 0; });
    flip("day_2h", [](Station &s) { s.hours = 2.0; });       // dt a power of two, T = 12
    flip("day_15min", [](Station &s) { s.hours = 0.25; });   // dt a power of two, T = 96
    flip("day_20min", [](Station &s) { s.hours = 1.0 / 3.0; });
    flip("diagnostics", [](Station &s) { s.diag = 1; });
    flip("two_lanes", [](Station &s) { s.lanes = 2; });
    for (int n : {1, 2, 4, 8, 9, 11, 16, 50}) {
        char name[16];
        snprintf(name, sizeof name, "n%d", n);
        Station st;
        st.n = n;
        bad += line(name, st, 0);
    }
    // a Params whose dimensions are not the station's (no configuration gives one): the predicate reads them
    {
        Params p;
        params_of(h, p);
        const StepPlan pl = step_plan(p, false);
        Params q = p;
        q.act_dim = 10;
        bad += day_station_fixed(pl, q) ? 1 : 0;
        q = p;
        q.obs_dim = 25;
        bad += day_station_fixed(pl, q) ? 1 : 0;
        bad += day_station_fixed(pl, p) ? 0 : 1;
    }
    return bad ? 1 : 0;
}
