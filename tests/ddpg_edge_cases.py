"""Shared by tests/test_ddpg_cpu.py and tests/test_gpu_ddpg_edges.py: the cases of the ring's edge tests and what can
be said about them without a GPU -- which of push_copy's three paths (csrc/sng_ddpg.h) every copy of a push takes, and
the sampler seeds and keys the device tests use.

push_copy copies a segment (one array of one run of consecutive slots) 16 bytes a lane where the source and the
destination reach a 16-byte boundary at the same element, and an element a lane elsewhere:
    head   = the elements before dst's first 16-byte boundary (at most n)
    vec    = src + head is 16-byte aligned
    groups = vec ? (n - head) / V : 0,   V = 16 / sizeof(dst element)
"whole" is groups > 0 with head == 0, "peeled" groups > 0 with head > 0 (the head and the tail of less than V elements
go an element a lane), "element" groups == 0.  copy_path is that arithmetic on byte offsets from a 16-byte boundary;
torch's allocations start on a 256-byte one, so a tensor's base is offset 0 and a slice x[d:d + 1] or slot s lies d or
s day blocks behind it."""
import numpy as np

from smart_nanogrid_gym import ddpg

ARRAYS = {"obs": ("f32", 4, 4), "actions": ("f32", 4, 4), "reward": ("f64_f32", 8, 4), "done": ("u8", 1, 1)}
PATHS = ("whole", "peeled", "element")

# (N, interval, E): the populations of the push tests.  T E is a multiple of 4 at both day lengths, so the reward's
# float32 day block is a whole number of 16-byte groups at every E, and so is the action block at N = 1 (A = 2); what E
# moves is the observation block (25 E 11 floats at N = 1: 12, 4 and 4 bytes past a boundary at E = 1, 3 and 67, none
# at 256) and the flags' (24 E bytes: 8 past at odd E; 36 bytes at "2h", E = 3: 4 past).
PUSH_CASES = [(1, "1h", 1), (1, "1h", 3), (1, "1h", 67), (1, "1h", 256), (4, "2h", 3)]

# The pushes of one population, (ring, days, first day of the two-day source): into "wrap" (capacity 3) two days at
# once, then the two days one by one from slices (slot 2, then slot 0 behind the wrap-around); into "slots" (capacity
# 3) day d from its slice into slot d, where source and destination lie the same distance behind a boundary.
PUSH_SEQUENCE = [("wrap", 2, 0), ("wrap", 1, 0), ("wrap", 1, 1), ("slots", 1, 0), ("slots", 1, 1)]

# Storage and sources that do not start on a 16-byte boundary, in elements: a ring on storage of the caller's own
# (include/sng.h: SngReplaySpec's pointers), which is the only way the reward's float32 destination leaves a boundary.
# (N, interval, E, storage displacement, [source displacement of each one-day push])
DISPLACED = (1, "1h", 3, dict(obs=1, actions=3, reward=2, done=5),
             [dict(obs=0, actions=0, reward=0, done=0), dict(obs=1, actions=3, reward=1, done=5)])

# The sampler-key test's env offset, ring seed and counter: above 2^32 each, so the key's high halves take part.
KEY_OFFSET, KEY_SEED, KEY_COUNTER = 2 ** 33 + 5, 2 ** 63 + 5, 2 ** 32 + 9


def station_dims(N, interval="1h"):
    """(T, obs_dim, act_dim) of a station of N chargers with PV and a battery (the tests' BASE)."""
    return {"1h": 24, "2h": 12}[interval], 2 * N + 9, N + 1


def day_elements(T, E, O, A):
    return dict(obs=(T + 1) * E * O, actions=T * E * A, reward=T * E, done=T * E)


def copy_path(src_offset, dst_offset, n, src_size, dst_size):
    """push_copy's path for n elements at these byte offsets from a 16-byte boundary."""
    V = 16 // dst_size
    head = min(((16 - dst_offset % 16) % 16) // dst_size, n)
    vec = (src_offset + head * src_size) % 16 == 0
    groups = (n - head) // V if vec else 0
    if groups == 0:
        return "element"
    return "peeled" if head else "whole"


def push_paths(T, E, O, A, capacity, head, days, src_day0=0, src_disp=None, dst_disp=None):
    """{(array, run): path} of one push of `days` days, read from day src_day0 of its source, into a ring whose next
    slot is `head` (replay_runs and replay_push_args of csrc/sng_ddpg_host.h); displacements in elements."""
    first = min(days, capacity - head)
    runs = [(0, head, first)] + ([(first, 0, days - first)] if days > first else [])
    out = {}
    for array, n_day in day_elements(T, E, O, A).items():
        _, ssize, dsize = ARRAYS[array]
        s0 = (src_disp or {}).get(array, 0)
        d0 = (dst_disp or {}).get(array, 0)
        for r, (day0, slot0, nd) in enumerate(runs):
            out[array, r] = copy_path((s0 + (src_day0 + day0) * n_day) * ssize, (d0 + slot0 * n_day) * dsize,
                                      nd * n_day, ssize, dsize)
    return out


def sequence_paths(N, interval, E, capacity=3):
    """[(ring, push number, array, run, path)] of PUSH_SEQUENCE at one population."""
    T, O, A = station_dims(N, interval)
    heads, out = {}, []
    for number, (ring, days, day0) in enumerate(PUSH_SEQUENCE):
        head = heads.get(ring, 0)
        for (array, run), path in push_paths(T, E, O, A, capacity, head, days, day0).items():
            out.append((ring, number, array, run, path))
        heads[ring] = (head + days) % capacity
    return out


def displaced_paths():
    """[(push number, array, path)] of DISPLACED's one-day pushes into slots 0, 1, .."""
    N, interval, E, dst_disp, sources = DISPLACED
    T, O, A = station_dims(N, interval)
    out = []
    for number, src_disp in enumerate(sources):
        for (array, _), path in push_paths(T, E, O, A, 3, number, 1, 0, src_disp, dst_disp).items():
            out.append((number, array, path))
    return out


def paths_reached():
    """{kind: the set of paths} over PUSH_CASES x PUSH_SEQUENCE and DISPLACED."""
    reached = {kind: set() for kind, _, _ in ARRAYS.values()}
    for N, interval, E in PUSH_CASES:
        for _, _, array, _, path in sequence_paths(N, interval, E):
            reached[ARRAYS[array][0]].add(path)
    for _, array, path in displaced_paths():
        reached[ARRAYS[array][0]].add(path)
    return reached


def seed_where(samples, T, E, env_offset=0, limit=10000):
    """The first sampler seed with which every sample (counter, batch, n, slots) holds a last-step row and a row of
    each of the first `slots` slots (as test_gpu_ddpg's seed_with_last_steps, with n per sample)."""
    for seed in range(limit):
        for counter, batch, n, slots in samples:
            idx = ddpg.replay_host_indices(seed, env_offset, counter, n, batch)
            if not ((idx // E) % T == T - 1).any() or set(np.unique(idx // (T * E))) != set(range(slots)):
                break
        else:
            return seed
    raise AssertionError("no seed found")


def partly_filled_samples(T, E):
    """The four samples of the partly filled ring: 64 and 200 rows at filled = 1 (counters 0, 1), then at filled = 2."""
    return [(0, 64, T * E, 1), (1, 200, T * E, 1), (2, 64, 2 * T * E, 2), (3, 200, 2 * T * E, 2)]


def special_rewards(n):
    """n float64 rewards that try a conversion to float32, the list below repeated over the array (so that they lie in
    a copy's vector body and in its peeled ends alike), and their names."""
    f32, f64 = np.float32, np.float64
    up = lambda x: f64(np.nextafter(f32(x), f32(np.inf)))   # noqa: E731
    even, odd = f32(1.0), np.nextafter(f32(1.0), f32(2.0))   # last mantissa bit 0 and 1
    small_even, small_odd = f32(-40.25), np.nextafter(f32(-40.25), f32(-41.0))
    values = {
        "exact": [1.5, -40.25, float(f32(0.1)), float(np.finfo(f32).max), float(np.finfo(f32).tiny), 0.0],
        "halfway, even below": [(f64(even) + up(even)) / 2, (f64(small_even) + f64(np.nextafter(small_even, f32(-41.0)))) / 2],
        "halfway, odd below": [(f64(odd) + up(odd)) / 2, (f64(small_odd) + f64(np.nextafter(small_odd, f32(-41.0)))) / 2],
        "subnormal": [1e-40, -1e-40, float(f32(1e-45)), 0.75 * float(f32(1e-45))],
        "negative zero": [-0.0],
        "beyond the range": [1e39, -1e39, float(np.finfo(f32).max) * (1 + 2.0 ** -24)],
        "one float64 step off a float32": [np.nextafter(f64(f32(x)), s * np.inf) for x in (0.1, -17.3, 3e38, 1e-38)
                                           for s in (1, -1)],
    }
    flat = np.array([v for vs in values.values() for v in vs], np.float64)
    return np.resize(flat, n), values
