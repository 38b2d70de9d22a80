"""ctypes binding of libsng.so (the C ABI in include/sng.h).

The shared library is the only compute path: there is no Python/NumPy fallback, and
loading fails loudly if the library is missing.  torch is imported first (when present)
so that libsng.so binds to the HIP runtime torch already loaded (both carry the SONAME
libamdhip64.so.7) and torch streams / device pointers are valid in both.
"""
import ctypes
import os

try:  # share torch's HIP runtime; torch is the device-memory/stream plumbing
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNG_LIBRARY", os.path.join(os.path.dirname(PKG_DIR), "lib", "libsng.so"))
DATA_DIR = os.path.join(PKG_DIR, "data")
IRRADIANCE_FILE = os.path.join(DATA_DIR, "solar_irradiance_1min.f64")

ABI_VERSION = 10
SNG_OK = 0
RNG_REFERENCE = 0
RNG_DEVICE = 1
GRAPH_RESET = 1        # sng.h SNG_GRAPH_RESET
GRAPH_STEP_NODES = 2   # sng.h SNG_GRAPH_STEP_NODES
GRAPH_TRAJECTORY = 4   # sng.h SNG_GRAPH_TRAJECTORY
GRAPH_SERIAL_RESET = 8   # sng.h SNG_GRAPH_SERIAL_RESET
GRAPH_OVERLAPPED_RESET = 16   # sng.h SNG_GRAPH_OVERLAPPED_RESET
GRAPH_POLICY_FUSED = 32   # sng.h SNG_GRAPH_POLICY_FUSED
GRAPH_GENERIC_DAY = 64   # sng.h SNG_GRAPH_GENERIC_DAY
FLAG_NEGATIVE_DEMAND = 0x1
FLAG_CHARGING_MODE = 0x2
FLAG_BESS_SOC_ABOVE_1 = 0x4
FLAG_V2X_BREAKPOINT = 0x8
FLAG_SUMMARY_WORDS = 1024   # SngInfo.flag_summary words (sng.h SNG_FLAG_SUMMARY_WORDS)
COMM_ID_BYTES = 128

c_double_p = ctypes.POINTER(ctypes.c_double)
c_float_p = ctypes.POINTER(ctypes.c_float)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_uint32_p = ctypes.POINTER(ctypes.c_uint32)


class SngConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("number_of_chargers", ctypes.c_int32),
        ("time_interval_hours", ctypes.c_double),
        ("price_model", ctypes.c_int32),
        ("pv_system_available", ctypes.c_int32),
        ("battery_system_available", ctypes.c_int32),
        ("vehicle_to_everything", ctypes.c_int32),
        ("different_vehicle_capacities", ctypes.c_int32),
        ("requested_state_of_charge", ctypes.c_int32),
        ("charging_mode_bounded", ctypes.c_int32),
        ("penalty_mode", ctypes.c_int32),
        ("numpy_legacy_promotion", ctypes.c_int32),
        ("grid_cost_weight", ctypes.c_double),
        ("battery_penalty_weight", ctypes.c_double),
        ("selling_price_coefficient", ctypes.c_double),
        ("bess_capacity_kwh", ctypes.c_double),
        ("bess_initial_soc", ctypes.c_double),
        ("bess_max_charging_kw", ctypes.c_double),
        ("bess_max_discharging_kw", ctypes.c_double),
        ("bess_charging_efficiency", ctypes.c_double),
        ("bess_discharging_efficiency", ctypes.c_double),
        ("bess_depth_of_discharge", ctypes.c_double),
        ("ev_max_power_kw", ctypes.c_double),
        ("ev_efficiency", ctypes.c_double),
        ("irradiance_per_minute", c_double_p),
        ("irradiance_minutes", ctypes.c_int64),
        ("step_lanes_per_env", ctypes.c_int32),
        ("extended_day", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("pv_noise", ctypes.c_double),
        ("price_noise", ctypes.c_double),
    ]


class SngDims(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("timesteps", ctypes.c_int32),
                ("number_of_chargers", ctypes.c_int32), ("num_envs", ctypes.c_int64),
                ("step_lanes_per_env", ctypes.c_int32), ("slots", ctypes.c_int32)]


INFO_FIELDS = ["grid_power", "total_charging_power", "total_discharging_power", "battery_state_of_charge",
               "total_vehicle_penalty", "total_battery_penalty", "grid_energy_cost", "total_cost",
               "utilized_solar_energy", "battery_power_value", "battery_calculated_power",
               "nonexistent_vehicle_penalty", "initial_battery_soc"]


class SngInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in INFO_FIELDS] + [("flags", ctypes.c_void_p),
                                                               ("episode_return", ctypes.c_void_p),
                                                               ("charger_power", ctypes.c_void_p),
                                                               ("vehicle_soc", ctypes.c_void_p),
                                                               ("flag_summary", ctypes.c_void_p)]


class SngScenario(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_int32), ("max_vehicles", ctypes.c_int32),
                ("soc", c_double_p), ("occupancy", c_double_p), ("capacity", c_double_p),
                ("requested_soc", c_double_p), ("arrivals", c_int32_p), ("departures", c_int32_p),
                ("pv_ratio", c_double_p)]


class SngMlpSpec(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("hidden", ctypes.c_int32),
                ("activation", ctypes.c_int32), ("clip_low", c_float_p), ("clip_high", c_float_p)]


class SngMlpWeights(ctypes.Structure):
    _fields_ = [(f, c_float_p) for f in ("w1", "b1", "w2", "b2", "w3", "b3")]


MLP_OUT_MEAN = 0     # sng.h SNG_MLP_OUT_MEAN
MLP_OUT_SQUASH = 1   # sng.h SNG_MLP_OUT_SQUASH


class SngMlpNetSpec(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32),
                ("hidden2", ctypes.c_int32), ("activation", ctypes.c_int32), ("output", ctypes.c_int32),
                ("low", c_float_p), ("high", c_float_p)]


class SngPpoNetSpec(ctypes.Structure):
    _fields_ = [("hidden1", ctypes.c_int32), ("hidden2", ctypes.c_int32), ("activation", ctypes.c_int32)]


class SngPpoRollout(ctypes.Structure):
    _fields_ = [("days", ctypes.c_int32), ("gamma", ctypes.c_double), ("gae_lambda", ctypes.c_double),
                ("obs", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("noise", ctypes.c_void_p), ("values", ctypes.c_void_p), ("advantages", ctypes.c_void_p),
                ("returns", ctypes.c_void_p), ("logp", ctypes.c_void_p)]


NOISE_GAUSSIAN = 0   # sng.h SNG_NOISE_GAUSSIAN
NOISE_OU = 1         # sng.h SNG_NOISE_OU


class SngNoiseSpec(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("seed", ctypes.c_uint64),
                ("theta", ctypes.c_double), ("dt", ctypes.c_double)]


class SngReplaySpec(ctypes.Structure):
    _fields_ = [("capacity_days", ctypes.c_int32), ("seed", ctypes.c_uint64), ("obs", ctypes.c_void_p),
                ("actions", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p)]


class SngReplayBatch(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("obs", "actions", "next_obs", "reward", "done", "index")]


class SngCriticSpec(ctypes.Structure):
    _fields_ = [("hidden1", ctypes.c_int32), ("hidden2", ctypes.c_int32), ("activation", ctypes.c_int32)]


LEARNER_SEGMENT = 1024     # sng.h SNG_LEARNER_SEGMENT
LEARNER_MAX_ROWS = 65536   # sng.h SNG_LEARNER_MAX_ROWS
# sng.h SNG_LEARNER_*: sng_learner_arrays' `which`
LEARNER_ARRAYS = ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v",
                  "actor_grad", "critic_grad")


class SngLearnerSpec(ctypes.Structure):
    _fields_ = [(f, ctypes.c_double) for f in ("actor_lr", "critic_lr", "tau", "beta1", "beta2", "eps")]


class SngNetArrays(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("w1", "b1", "w2", "b2", "w3", "b3")]


class SngLearnerState(ctypes.Structure):
    _fields_ = [(f, SngNetArrays) for f in LEARNER_ARRAYS[:8]] + [("step", ctypes.c_int64)]


class SngLearnerLast(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int64)] + [(f, ctypes.c_void_p) for f in ("q", "dq", "a_pi", "q_pi", "critic_loss",
                                                                           "actor_loss")]


class SngLearnerTrace(ctypes.Structure):
    _fields_ = [("q", ctypes.c_void_p), ("dq", ctypes.c_void_p), ("q_pi", ctypes.c_void_p),
                ("critic_grad", SngNetArrays), ("actor_grad", SngNetArrays), ("critic_loss", ctypes.c_void_p),
                ("actor_loss", ctypes.c_void_p)]


_H, _S = ctypes.c_void_p, ctypes.c_void_p   # handle, hipStream_t
EXPORTS = {
    "sng_abi_version": (ctypes.c_int32, []),
    "sng_build_id": (ctypes.c_char_p, []),
    "sng_config_defaults": (None, [ctypes.POINTER(SngConfig)]),
    "sng_create": (ctypes.c_int, [ctypes.POINTER(SngConfig), ctypes.c_int, ctypes.c_int64, ctypes.c_uint64,
                                  ctypes.POINTER(ctypes.c_void_p)]),
    "sng_destroy": (None, [_H]),
    "sng_last_error": (ctypes.c_char_p, [_H]),
    "sng_get_dims": (ctypes.c_int, [_H, ctypes.POINTER(SngDims)]),
    "sng_get_timestep": (ctypes.c_int, [_H]),
    "sng_set_env_offset": (ctypes.c_int, [_H, ctypes.c_int64]),
    "sng_set_seed": (ctypes.c_int, [_H, ctypes.c_uint64, _S]),
    "sng_reset": (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_void_p, _S]),
    "sng_reset_replay": (ctypes.c_int, [_H, ctypes.c_void_p, _S]),
    "sng_reset_from_scenario": (ctypes.c_int, [_H, ctypes.POINTER(SngScenario), ctypes.c_void_p, _S]),
    "sng_step": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.POINTER(SngInfo), _S]),
    "sng_step_host": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.POINTER(SngInfo), _S]),
    "sng_step_kernel_name": (ctypes.c_int, [_H, ctypes.POINTER(SngInfo), ctypes.c_char_p, ctypes.c_int32]),
    "sng_read_errors": (ctypes.c_int, [_H, c_uint32_p, ctypes.c_int, _S]),
    "sng_get_battery_soc": (ctypes.c_int, [_H, c_double_p, _S]),
    "sng_set_battery_soc": (ctypes.c_int, [_H, c_double_p, _S]),
    "sng_get_pv_ratio": (ctypes.c_int, [_H, c_double_p, _S]),
    "sng_get_vehicle_soc": (ctypes.c_int, [_H, c_double_p, _S]),
    "sng_set_vehicle_soc": (ctypes.c_int, [_H, c_double_p, _S]),
    "sng_state_size": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "sng_get_state": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, _S]),
    "sng_set_state": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, _S]),
    "sng_get_scenario": (ctypes.c_int, [_H, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, c_double_p, c_double_p,
                                        c_double_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, _S]),
    "sng_get_tables": (ctypes.c_int, [_H, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                      c_int32_p]),
    "sng_graph_create": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.POINTER(SngInfo), ctypes.c_int, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "sng_graph_launch": (ctypes.c_int, [ctypes.c_void_p, _S]),
    "sng_graph_step_nodes": (ctypes.c_int, [ctypes.c_void_p]),
    "sng_graph_reset_overlapped": (ctypes.c_int, [ctypes.c_void_p]),
    "sng_graph_day_kernel_name": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32]),
    "sng_graph_describe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "sng_graph_destroy": (None, [ctypes.c_void_p]),
    "sng_time_step_kernels": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.POINTER(SngInfo), ctypes.c_int32, c_float_p,
                                             c_float_p, _S]),
    "sng_policy_create": (ctypes.c_int, [_H, ctypes.POINTER(SngMlpSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_policy_set_weights": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngMlpWeights), _S]),
    "sng_policy_actions": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, _S]),
    "sng_policy_destroy": (None, [ctypes.c_void_p]),
    "sng_graph_create_policy": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SngInfo), ctypes.c_int,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "sng_policy_host_actions": (ctypes.c_int, [ctypes.POINTER(SngMlpSpec), ctypes.POINTER(SngMlpWeights),
                                               ctypes.c_int64, c_float_p, c_float_p, c_float_p, c_float_p]),
    "sng_policy_create_net": (ctypes.c_int, [_H, ctypes.POINTER(SngMlpNetSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_policy_net_host_actions": (ctypes.c_int, [ctypes.POINTER(SngMlpNetSpec), ctypes.POINTER(SngMlpWeights),
                                                   ctypes.c_int64, c_float_p, c_float_p, c_float_p, c_float_p]),
    "sng_ppo_create": (ctypes.c_int, [_H, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    "sng_ppo_set_weights": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngMlpWeights), c_float_p, _S]),
    "sng_ppo_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngPpoRollout), _S]),
    "sng_ppo_host_finish": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_int64, ctypes.POINTER(SngMlpWeights), c_float_p,
                                           ctypes.POINTER(SngPpoRollout), ctypes.c_int]),
    "sng_ppo_destroy": (None, [ctypes.c_void_p]),
    "sng_ppo_create_net": (ctypes.c_int, [_H, ctypes.POINTER(SngPpoNetSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_ppo_net_host_finish": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SngPpoNetSpec),
                                               ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(SngMlpWeights),
                                               c_float_p, ctypes.POINTER(SngPpoRollout), ctypes.c_int]),
    "sng_noise_create": (ctypes.c_int, [_H, ctypes.POINTER(SngNoiseSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_noise_set_params": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, _S]),
    "sng_noise_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, _S]),
    "sng_noise_get_counter": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), _S]),
    "sng_noise_set_counter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, _S]),
    "sng_noise_destroy": (None, [ctypes.c_void_p]),
    "sng_noise_host_fill": (ctypes.c_int, [ctypes.POINTER(SngNoiseSpec), c_float_p, c_float_p, ctypes.c_int32,
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, c_float_p]),
    "sng_graph_create_policy_noise": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.POINTER(SngInfo), ctypes.c_int, ctypes.c_int32,
                                                     ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "sng_replay_create": (ctypes.c_int, [_H, ctypes.POINTER(SngReplaySpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_replay_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, _S]),
    "sng_replay_size": (ctypes.c_int64, [ctypes.c_void_p]),
    "sng_replay_state": (ctypes.c_int, [ctypes.c_void_p, c_int32_p, c_int32_p]),
    "sng_replay_sample": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(SngReplayBatch), _S]),
    "sng_replay_get_counter": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "sng_replay_set_counter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "sng_replay_destroy": (None, [ctypes.c_void_p]),
    "sng_replay_host_indices": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "sng_critic_create": (ctypes.c_int, [_H, ctypes.POINTER(SngCriticSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_critic_set_weights": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngMlpWeights), _S]),
    "sng_critic_q": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, _S]),
    "sng_critic_targets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                          ctypes.c_void_p, _S]),
    "sng_critic_destroy": (None, [ctypes.c_void_p]),
    "sng_critic_host_q": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SngCriticSpec),
                                         ctypes.POINTER(SngMlpWeights), ctypes.c_int64, c_float_p, c_float_p, c_float_p]),
    "sng_critic_host_targets": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(SngCriticSpec),
                                               ctypes.POINTER(SngMlpWeights), ctypes.POINTER(SngMlpNetSpec),
                                               ctypes.POINTER(SngMlpWeights), ctypes.c_int64, c_float_p, c_float_p,
                                               c_float_p, ctypes.c_double, c_float_p, ctypes.c_int, c_float_p]),
    "sng_policy_actions_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, _S]),
    "sng_learner_create": (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(SngLearnerSpec), ctypes.POINTER(ctypes.c_void_p)]),
    "sng_learner_update": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, _S]),
    "sng_learner_arrays": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(SngNetArrays)]),
    "sng_learner_last": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngLearnerLast)]),
    "sng_learner_get_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "sng_learner_set_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngLearnerState), _S]),
    "sng_learner_get_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SngLearnerState),
                                             ctypes.POINTER(ctypes.c_int64), _S]),
    "sng_learner_destroy": (None, [ctypes.c_void_p]),
    "sng_learner_host_update": (ctypes.c_int, [ctypes.POINTER(SngMlpNetSpec), ctypes.POINTER(SngCriticSpec),
                                               ctypes.POINTER(SngLearnerSpec), ctypes.POINTER(SngLearnerState),
                                               ctypes.c_int64, c_float_p, c_float_p, c_float_p, c_float_p,
                                               ctypes.POINTER(SngLearnerTrace)]),
    "sng_host_generate_scenarios": (ctypes.c_int, [ctypes.POINTER(SngConfig), ctypes.c_int64, ctypes.c_uint64,
                                                   ctypes.c_int32, c_double_p, c_double_p, c_double_p, c_double_p,
                                                   c_int32_p, c_int32_p, ctypes.c_int32, c_double_p]),
    "sng_host_threads": (ctypes.c_int32, []),
    "sng_get_day_counter": (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_uint64), _S]),
    "sng_bandwidth_probe": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), _S]),
    "sng_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "sng_comm_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_void_p)]),
    "sng_allgather_returns": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _S]),
    "sng_comm_destroy": (None, [ctypes.c_void_p]),
    "sng_comm_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
}

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def lib():
    """Load libsng.so (raises NativeLibraryMissing when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C smart-nanogrid-gym_amd/csrc` (there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                # additions to the ABI (sng_graph_step_nodes) keep its version: an older build lacks the symbol
                raise NativeLibraryMissing(f"{LIB_PATH} does not export {name}: it is an older build of the "
                                           "library, rebuild it (make -C smart-nanogrid-gym_amd/csrc)") from None
            fn.restype = res
            fn.argtypes = args
        if L.sng_abi_version() != ABI_VERSION:
            raise NativeLibraryMissing("libsng.so ABI version mismatch")
        _lib = L
    return _lib


class NativeError(RuntimeError):
    pass


def graph_describe(g):
    """sng_graph_describe's text for a graph handle: one line per captured node."""
    n = lib().sng_graph_describe(g, None, 0)
    if n < 0:
        raise NativeError(f"libsng error {n}: sng_graph_describe")
    buf = ctypes.create_string_buffer(n + 1)
    if lib().sng_graph_describe(g, buf, len(buf)) != n:
        raise NativeError("sng_graph_describe: the graph changed between two calls")
    return buf.value.decode()


def check(rc, handle=None):
    if rc != SNG_OK:
        msg = lib().sng_last_error(handle)
        raise NativeError(f"libsng error {rc}: {msg.decode() if msg else ''}")


def load_irradiance():
    import numpy as np
    return np.fromfile(IRRADIANCE_FILE, dtype="<f8")
