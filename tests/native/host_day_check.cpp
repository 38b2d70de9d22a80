// Host-only check of sng_host_day.h and sng_state_format.h (tests/test_host_day_cpu.py builds it with g++,
// under AddressSanitizer and UBSan when they link):
//   1. encode_day against decode_day: reference days drawn by generate_day from MT19937::seed_numpy(s), s = 0..199,
//      at N in {1, 3, 10} x (dt = 1 h | dt = 0.25 h with extended_day) x requested SoC on / off x different
//      capacities on / off, encoded into env column 1 of [T][N][3] planes and decoded again, must come back
//      element for element (every array, arrival / departure lists and vehicle counts included).
//   2. the checkpoint's stream conversion: saved_to_stream(stream_to_saved(x)) == x for both blocks and
//      mti in {0, 1, 623, 624}; a stream seeded by seed_python(12345) saves as MT19937::save does; a saved
//      position of 626 is refused.
// (sng_layout.h has no host-side packer of the device days' 2 B records, so their decoder, records_to_words, is
// not exercised here; the GPU tests of sng_get_scenario cover it.)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sng_host_day.h"
#include "sng_host_tables.h"
#include "sng_state_format.h"

using namespace sng;

static int g_failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            if (++g_failures > 20) return; \
        }                                 \
    } while (0)

struct Day {
    std::vector<double> soc, occ, cap, req;
    std::vector<int32_t> arr, dep;
    Day(int N, int S, int V) : soc(N * S, -1.0), occ(N * S, -1.0), cap(N * S, -1.0), req(N * S, -1.0), arr(N * V, -7), dep(N * V, -7) {}
    DayView view(int V, int S) { return DayView{soc.data(), occ.data(), cap.data(), req.data(), arr.data(), dep.data(), V, S}; }
};

static void check_days(int N, double dt, bool extended, bool req_on, bool diff_caps, long *days) {
    static const double irradiance[1] = {0.0};
    SngConfig cfg{};
    cfg.abi_version = SNG_ABI_VERSION;
    cfg.number_of_chargers = N;
    cfg.time_interval_hours = dt;
    cfg.extended_day = extended ? 1 : 0;
    cfg.requested_state_of_charge = req_on ? 1 : 0;
    cfg.different_vehicle_capacities = diff_caps ? 1 : 0;
    cfg.charging_mode_bounded = 1;
    cfg.penalty_mode = SNG_PENALTY_SPARSE;
    cfg.irradiance_per_minute = irradiance;
    cfg.irradiance_minutes = 1;
    int T = 0;
    std::string err;
    CHECK(validate(&cfg, &T, err) == SNG_OK, "validate N=%d dt=%g: %s", N, dt, err.c_str());
    Params p{};
    DaySpans spans{};
    CHECK(fill_params(cfg, T, 0, p, spans), "fill_params N=%d", N);
    p = with_day(p, DayKey::host_day(true));
    const int S = spans.slots, V = 8;
    const int64_t E = 3, e = 1;
    const size_t tl = (size_t)T * N * E;
    for (uint32_t s = 0; s < 200; ++s, ++*days) {
        MT19937 rng;
        rng.seed_numpy(s);
        Day in(N, S, V), out(N, S, V);
        CHECK(generate_day(cfg, T, rng, in.view(V, S)), "generate_day overflowed %d vehicles (seed %u)", V, s);
        // poisoned planes: a write to, or a read from, another env's column shows
        std::vector<uint32_t> word(tl, 0xffffffffu);
        std::vector<double> aux(tl, NAN), rq(tl, NAN);
        double pen0 = NAN;
        bool need_req = false;
        CHECK(encode_day(p, E, e, in.view(V, S), word.data(), aux.data(), rq.data(), &pen0, &need_req, err),
              "encode_day seed %u: %s", s, err.c_str());
        for (size_t i = 0; i < tl; ++i)
            if ((int64_t)(i % E) != e)
                CHECK(word[i] == 0xffffffffu && std::isnan(aux[i]) && std::isnan(rq[i]), "encode_day wrote column %zu", i % E);
        CHECK(pen0 == 0.0, "a generated day's t = 0 penalty is %g", pen0);
        std::vector<int32_t> nv(N, -7);
        decode_day(p, (size_t)E, (size_t)e, word.data(), aux.data(), rq.data(), out.view(V, S), nv.data());
        const char *names[] = {"soc", "occupancy", "capacity", "requested_soc"};
        const std::vector<double> *a[] = {&in.soc, &in.occ, &in.cap, &in.req}, *b[] = {&out.soc, &out.occ, &out.cap, &out.req};
        for (int f = 0; f < 4; ++f)
            for (size_t i = 0; i < a[f]->size(); ++i)
                CHECK((*a[f])[i] == (*b[f])[i], "%s[c=%zu, slot=%zu] %.17g -> %.17g (N=%d dt=%g req=%d caps=%d seed=%u)", names[f],
                      i / S, i % S, (*a[f])[i], (*b[f])[i], N, dt, (int)req_on, (int)diff_caps, s);
        for (size_t i = 0; i < in.arr.size(); ++i) {
            CHECK(in.arr[i] == out.arr[i], "arrivals[c=%zu, v=%zu] %d -> %d (N=%d dt=%g seed=%u)", i / V, i % V, in.arr[i],
                  out.arr[i], N, dt, s);
            CHECK(in.dep[i] == out.dep[i], "departures[c=%zu, v=%zu] %d -> %d (N=%d dt=%g seed=%u)", i / V, i % V, in.dep[i],
                  out.dep[i], N, dt, s);
        }
        for (int c = 0; c < N; ++c)
            CHECK(nv[c] == list_len(in.arr.data() + c * V, V), "n_vehicles[%d] = %d (N=%d dt=%g seed=%u)", c, nv[c], N, dt, s);
    }
}

static void check_streams() {
    MT19937 fill;
    fill.seed_numpy(2024);
    uint32_t blocks[2 * kMtN], saved[MT19937::kStateWords], words[kMtN];
    for (uint32_t &w : blocks) w = fill.next();
    for (int cur = 0; cur < 2; ++cur)
        for (int mti : {0, 1, 623, 624}) {
            int32_t pos = -1;
            stream_to_saved(blocks, (cur << 16) | mti, saved);
            CHECK(saved[kMtN] == (uint32_t)mti, "saved mti %u, want %d", saved[kMtN], mti);
            CHECK(saved_to_stream(saved, words, &pos), "saved_to_stream refused cur=%d mti=%d", cur, mti);
            CHECK(pos == mti, "position %d, want block 0, mti %d", pos, mti);
            CHECK(std::memcmp(words, blocks + cur * kMtN, sizeof words) == 0, "block %d does not come back (mti %d)", cur, mti);
        }
    // a stream as the library seeds Python's: seed, save, into the device layout (block 0; block 1 is not read)
    MT19937 m;
    m.seed_python(12345);
    uint32_t want[MT19937::kStateWords];
    m.save(want);
    int32_t pos = -1;
    CHECK(saved_to_stream(want, blocks, &pos) && pos == kMtN, "a freshly seeded stream is at position %d", pos);
    stream_to_saved(blocks, pos, saved);
    CHECK(std::memcmp(saved, want, sizeof want) == 0, "seed_python(12345) does not save as MT19937::save does");
    want[kMtN] = 626;
    CHECK(!saved_to_stream(want, words, &pos), "a saved position of 626 was accepted");
}

int main() {
    long days = 0;
    for (int N : {1, 3, 10})
        for (int ext = 0; ext < 2; ++ext)
            for (int req = 0; req < 2; ++req)
                for (int caps = 0; caps < 2; ++caps) check_days(N, ext ? 0.25 : 1.0, ext != 0, req != 0, caps != 0, &days);
    check_streams();
    if (g_failures) return 1;
    std::printf("host day ok: %ld days round-trip, streams convert both ways\n", days);
    return 0;
}
