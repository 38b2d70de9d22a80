"""The device-RNG day cases shared by the CPU checks of the oracle's day model (test_device_day_model_cpu.py) and
the GPU test that pins generate_kernel to it (test_gpu_device_day_exact.py).

One row per generator shape: the charger-quad widths of the timeline grid (sng_generate.h gen_rows: full quads,
a last partial quad of width 1, 2 or 3), the fused and the unfused t = 0 observation, every generate_kernel
instantiation (<24 | 96 | 0, requested SoC on | off>), fixed capacities, the four penalty modes, and the stream
keys' corners (a seed above 2^32, global env ids across 2^25 and above 2^32).  E is small and ragged on purpose
(no multiple of a wavefront, a block row or a quad row), and sized so that stepping the oracle's envs in Python
takes a few seconds per row.
"""
import collections

import numpy as np

import oracle as O

DAYS = 3                      # consecutive days per row
AMBIGUOUS_SHARE_MAX = 1e-3    # of a row's vehicles; the expected share is 2e-5 (342 of the 2^24 draws)

Case = collections.namedtuple("Case", "name N interval req diff_caps penalty E env_offset seed extra")


def _case(name, N, interval, E, penalty, seed, req=False, diff_caps=True, env_offset=0, **extra):
    return Case(name, N, interval, req, diff_caps, penalty, E, env_offset, seed, extra)


CASES = [
    # a partial quad only: one, two, three lanes per env (width 3: one lane in four idle)
    _case("width1", 1, "1h", 77, "sparse", 11),
    _case("width2_offset_above_2^32", 2, "1h", 77, "dense", 12, env_offset=2 ** 32 + 12345),
    _case("width3_no_penalty", 3, "1h", 77, "no_penalty", 13),
    # full quads only, and full quads with a partial quad of width 3, 2, 1
    _case("quad4_on_departure", 4, "1h", 300, "on_departure", 14),
    _case("quads7", 7, "1h", 300, "sparse", 15),
    _case("quads10_seed_above_2^32", 10, "1h", 333, "no_penalty", 0x1234_5678_9abc),
    _case("quads33", 33, "1h", 130, "on_departure", 17),
    # the widest fused reset (global envs straddle 2^25) and the unfused one (observe0_kernel, OBS0_DEVICE)
    _case("fused50_across_2^25", 50, "1h", 100, "sparse", 18, env_offset=2 ** 25 - 37),
    _case("unfused128", 128, "1h", 70, "dense", 19),
    # generate_kernel<24, true>
    _case("req24_dense", 10, "1h", 200, "dense", 20, req=True),
    # generate_kernel<96, false> with profile noise (config 5)
    _case("noise96", 50, "15min", 64, "sparse", 21, extended_day=True, pv_noise=0.2, price_noise=0.1),
    # generate_kernel<0, true>
    _case("req96", 10, "15min", 100, "sparse", 22, req=True, extended_day=True),
    # generate_kernel<0, false>: T = 48, 72, 12
    _case("t48", 7, "30min", 150, "on_departure", 23, extended_day=True),
    _case("t72", 6, "20min", 100, "dense", 24, extended_day=True),
    _case("t12", 4, "2h", 300, "sparse", 25),
    # fixed capacities: the departure comes from r itself
    _case("fixed_capacity", 10, "1h", 200, "sparse", 26, diff_caps=False),
]
IDS = [c.name for c in CASES]


def env_kwargs(case):
    kw = dict(number_of_chargers=case.N, time_interval=case.interval, charging_mode="bounded",
              vehicle_uncharged_penalty_mode=case.penalty, pv_system_available_in_model=True,
              battery_system_available_in_model=True, enable_requested_state_of_charge=case.req,
              enable_different_vehicle_battery_capacities=case.diff_caps)
    kw.update(case.extra)
    return kw


def model_days(case, day, follow=None, cfg=None):
    """The model's day `day` of every env of the row; follow: per env, the GPU's exported arrivals ([N][V])."""
    cfg = cfg or O.OracleConfig(**env_kwargs(case))
    return [O.device_day(cfg, case.seed, case.env_offset + e, day, None if follow is None else follow[e])
            for e in range(case.E)]


def padded(lists, V=8):
    """Ragged per-charger lists as an [N][V] int32 array padded with -1."""
    out = np.full((len(lists), V), -1, np.int32)
    for c, row in enumerate(lists):
        out[c, :len(row)] = row
    return out
