// sng_state_format.h -- the bytes of a checkpoint that no device is needed for: the loaded-day key, the blob's
// header, and the conversion between the reference RNG streams as the device keeps them (RefStreams,
// sng_layout.h) and as a blob stores them (MT19937::save, sng_mt.h).  Host only, no HIP: it compiles with
// plain g++ (tests/native/host_day_check.cpp checks the stream conversion on the CPU).
#pragma once
#include <cstddef>

#include "sng_layout.h"
#include "sng_mt.h"

namespace sng {

// The Params fields that say how the loaded day is encoded and stepped; a steps-only graph
// captures them and may replay only over a day with the same key.  Nothing else writes those four fields:
// a day kind below makes the key, load_day / with_day put it into a Params.  (Four int32 and no constructor:
// the checkpoint header stores the key as it is.)
struct DayKey {
    int32_t packed, req_stream, req_zero, bump_day;
    bool operator==(const DayKey &o) const {
        return packed == o.packed && req_stream == o.req_stream && req_zero == o.req_zero && bump_day == o.bump_day;
    }
    static DayKey of(const Params &p) { return DayKey{p.packed, p.req_stream, p.req_zero, p.bump_day}; }
    // a device-RNG day: the generator writes packed records (sng_layout.h); the day owns a day-counter value,
    // which its first step advances
    static DayKey device_day(const Params &p) { return DayKey{1, p.req_enabled, 0, 1}; }
    // a reference-RNG or injected day: word + f64 aux planes, with or without the requested-SoC stream
    static DayKey host_day(bool req_stream) { return DayKey{0, req_stream ? 1 : 0, 0, 0}; }
    // the loaded day replayed: Requested_SOC reads 0 and the steps do not count the day again
    DayKey replayed() const { return DayKey{packed, req_stream, 1, 0}; }
    // sng_set_seed: the day counter restarts, so an unstepped device day no longer owns day 0
    DayKey disowned() const { return DayKey{packed, req_stream, req_zero, 0}; }
    bool unstepped_device_day(int t) const { return packed && bump_day && t == 0; }
};
static inline Params with_day(Params p, const DayKey &k) {
    p.packed = k.packed;
    p.req_stream = k.req_stream;
    p.req_zero = k.req_zero;
    p.bump_day = k.bump_day;
    return p;
}

// ---------------------------------------------------------------------------------
// Checkpoint / resume: header, then the sections in this order (host byte order):
//   soc f64[N/2][E][2] (charger pairs) | bess, bess0, ratio, pen0 f64[E] | flags u32[E] | [word u32[T][N][E], host days]
//   | aux 8B[T][N][E] (a packed day: its u16 records in charger quads, sng_layout.h) | [req f64[T][N][E]]
//   | [profile keys u32[E][2]] | [episode return f64[E]]
//   | [reference streams u32[E][2][625]]
// ---------------------------------------------------------------------------------
struct StateHeader {
    char magic[8];
    int32_t abi, header_bytes;
    int64_t num_envs;
    int32_t n, T, slots, obs_dim;
    uint64_t config_hash, seed;
    int64_t env_offset;
    int32_t t, day_finished;
    DayKey day;   // packed, req_stream, req_zero, bump_day
    int32_t gen_mode, gen_loaded;
    uint64_t replays, day_counter;
    int32_t has_word, has_req, has_prof, has_return, has_streams, reserved;
    uint64_t total_bytes;
};
static_assert(sizeof(StateHeader) == 144 && offsetof(StateHeader, day) == 72 && sizeof(DayKey) == 16,
              "the checkpoint header's bytes are format 5's");
// the last byte is the checkpoint format version: '3' since the configuration fingerprint is hashed
// field by field (round 3), '5' since the SoC state is stored in charger pairs, a day's stochastic profiles
// as per-env keys and a device day's records in 2 B (round 4); a blob of another version is refused as such
static const char kStateMagic[8] = {'S', 'N', 'G', 'S', 'T', 'A', 'T', '5'};

// The stream section: per env numpy's RandomState, then Python's random, each as MT19937::save lays it out
// (the current block's 624 raw state words, then mti).
// One stream as the device keeps it -- blocks: its [2][624] tempered words, pos: cur << 16 | flags | mti --
// into the 625 saved words.
static inline void stream_to_saved(const uint32_t *blocks, int32_t pos, uint32_t *out) {
    const int cur = (pos >> 16) & 1, mti = pos & kMtPosMask;
    const uint32_t *src = blocks + (size_t)cur * kMtN;
    for (int k = 0; k < kMtN; ++k) out[k] = mt_untemper_word(src[k]);   // the raw state
    out[kMtN] = (uint32_t)mti;
}
// ... and back: the 624 words of block 0 (RefStreams keep tempered words) and the position (block 0, mti).
// False: no MT19937 saves such a position (a corrupt blob).
static inline bool saved_to_stream(const uint32_t *in, uint32_t *words, int32_t *pos) {
    if (in[kMtN] > (uint32_t)kMtN + 1) return false;
    for (int q = 0; q < kMtN; ++q) words[q] = mt_temper_word(in[q]);
    // mti = N + 1 (never seeded) cannot come from a seeded generator
    *pos = (int32_t)(in[kMtN] < (uint32_t)kMtN ? in[kMtN] : (uint32_t)kMtN);
    return true;
}

}  // namespace sng
