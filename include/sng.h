/*
 * sng.h -- C ABI of the MI355X-native batched SmartNanogridEnv (libsng.so).
 *
 * Drop-in boundary for the reference's step()/reset() hot path.  The reference
 * (Dellintel98/smart-nanogrid-gym, pure Python) has no FFI of its own; its
 * plugin surface is the gym.Env it registers as 'SmartNanogridEnv-v0'
 * (smart_nanogrid_gym/__init__.py:4-8).  Each entry point below names the
 * reference interface it replaces.  The Python mirror of that interface
 * (smart-nanogrid-gym_amd/smart_nanogrid_gym/) binds these symbols with ctypes;
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Plain C types only.  Device buffers are raw device pointers (e.g. a torch
 *     tensor's data_ptr()); `stream` is an opaque hipStream_t (NULL = default).
 *   - Every call returns SNG_OK (0) or a negative SngStatus; the message is in
 *     sng_last_error(env) (or sng_last_error(NULL) for sng_create failures).
 *   - All calls on one handle must come from one host thread at a time.
 *   - Layouts at the boundary: actions float32 [num_envs][act_dim] row-major,
 *     observations float32 [num_envs][obs_dim] row-major, reward float64
 *     [num_envs], done uint8 [num_envs] -- exactly the per-env arrays the
 *     reference returns, stacked.
 */
#ifndef SNG_H
#define SNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNG_ABI_VERSION 10

typedef enum SngStatus {
    SNG_OK = 0,
    SNG_ERR_INVALID_ARGUMENT = -1,   /* ValueError in the reference */
    SNG_ERR_UNSUPPORTED = -2,        /* configuration the reference cannot run either */
    SNG_ERR_HIP = -3,                /* HIP runtime failure */
    SNG_ERR_STATE = -4,              /* call out of order (e.g. step before reset) */
    SNG_ERR_OUT_OF_MEMORY = -5
} SngStatus;

/* vehicle_uncharged_penalty_mode, charging_station.py:50-60 */
typedef enum SngPenaltyMode {
    SNG_PENALTY_NONE = 0,            /* 'no_penalty' */
    SNG_PENALTY_ON_DEPARTURE = 1,    /* 'on_departure' */
    SNG_PENALTY_SPARSE = 2,          /* 'sparse' */
    SNG_PENALTY_DENSE = 3            /* 'dense' */
} SngPenaltyMode;

/* How sng_reset draws the new day's vehicles. */
typedef enum SngRngMode {
    /* MT19937 streams identical to the reference's global RNGs: environment i
     * reproduces `np.random.seed(seed + i); random.seed(seed + i)` followed by the
     * reference's reset()/step() sequence (charging_station.py:200-279,
     * smart_nanogrid_environment.py:181,349).  The streams live and are drawn on the device. */
    SNG_RNG_REFERENCE = 0,
    /* Counter-based hash streams on the GPU: same distributions, different draws (the arrival
     * SoC is drawn as a float32 value).  Fully device-resident; graph-capturable.  Each device
     * reset draws a new day of the handle's day counter, which the day's first step advances. */
    SNG_RNG_DEVICE = 1
} SngRngMode;

/* Per-env flag bits reported by sng_read_errors / SngInfo.flags. */
#define SNG_FLAG_SUMMARY_WORDS 1024   /* SngInfo.flag_summary's words */
#define SNG_FLAG_NEGATIVE_DEMAND  0x1u  /* ValueError, central_management_system.py:158-159 */
#define SNG_FLAG_CHARGING_MODE    0x2u  /* ValueError, charger.py:88/138, battery_energy_storage_system.py:74/106 */
#define SNG_FLAG_BESS_SOC_ABOVE_1 0x4u  /* ValueError, penaliser.py:110-111 */
#define SNG_FLAG_V2X_BREAKPOINT   0x8u  /* breakpoint(), central_management_system.py:160-165 (not an error) */

/* Constructor keyword arguments of SmartNanogridEnv (smart_nanogrid_environment.py:32-34)
 * plus the module constants the reference hard-codes, with the reference's values as
 * defaults (sng_config_defaults). */
typedef struct SngConfig {
    int32_t abi_version;                     /* = SNG_ABI_VERSION */
    int32_t number_of_chargers;              /* N (1..128) */
    double time_interval_hours;              /* set_time_interval(), :125-138 ('1h' -> 1.0) */
    int32_t price_model;                     /* accountant.py:58-101, 0..4 */
    int32_t pv_system_available;             /* pv_system_available_in_model */
    int32_t battery_system_available;        /* battery_system_available_in_model */
    int32_t vehicle_to_everything;           /* vehicle_to_everything */
    int32_t different_vehicle_capacities;    /* enable_different_vehicle_battery_capacities */
    int32_t requested_state_of_charge;       /* enable_requested_state_of_charge */
    int32_t charging_mode_bounded;           /* charging_mode == 'bounded' */
    int32_t penalty_mode;                    /* SngPenaltyMode */
    int32_t numpy_legacy_promotion;          /* 1: NumPy<2 float64 EV power (the recorded KATs) */
    double grid_cost_weight;                 /* accountant.py:35 -> 0.75 */
    double battery_penalty_weight;           /* penaliser.py:181 -> 0.8 */
    double selling_price_coefficient;        /* accountant.py:6 -> 0.8 */
    /* BESS, central_management_system.py:35 */
    double bess_capacity_kwh;                /* 80 */
    double bess_initial_soc;                 /* 0.5 */
    double bess_max_charging_kw;             /* 44 */
    double bess_max_discharging_kw;          /* 44 */
    double bess_charging_efficiency;         /* 0.95 */
    double bess_discharging_efficiency;      /* 0.95 */
    double bess_depth_of_discharge;          /* 0.15 */
    /* EV charger, charger.py:20-23 */
    double ev_max_power_kw;                  /* 22 */
    double ev_efficiency;                    /* 0.95 */
    /* PV input: per-minute irradiance (W/m^2), solar_irradiance.mat['irradiance'] */
    const double *irradiance_per_minute;
    int64_t irradiance_minutes;
    /* Kernel tuning: GPU lanes per environment in the step kernel (0 = automatic; 1, 2, 4). */
    int32_t step_lanes_per_env;
    /* Build-defined generalisation (no reference oracle, default off):
     * extended_day = 1 allows days longer than 24 steps (dt < 1 h): per-charger arrays get
     * T+1 slots, prices come from the per-step tariff loop (accountant.py:61-68).
     * pv_noise / price_noise = sigma > 0 scale every PV / price table entry an env uses on a day
     * by 1 + sigma*z, z in [-1, 1) from a counter-based hash of (env seed, day, k). */
    int32_t extended_day;
    int32_t reserved0;
    double pv_noise;
    double price_noise;
} SngConfig;

typedef struct SngDims {
    int32_t obs_dim;        /* smart_nanogrid_environment.py:90-96 */
    int32_t act_dim;        /* :101-118 */
    int32_t timesteps;      /* 24 / dt */
    int32_t number_of_chargers;
    int64_t num_envs;
    int32_t step_lanes_per_env;   /* lanes per env the step kernel runs with (SngConfig 0 = default) */
    int32_t slots;                /* per-charger scenario array length: 25, or T+1 with extended_day */
} SngDims;

/* Optional per-step diagnostics: device pointers, each [num_envs]; NULL = not written.
 * Names follow the results dict of CentralManagementSystem.manage_nanogrid
 * (central_management_system.py:128-155). */
typedef struct SngInfo {
    double *grid_power;                  /* 'Grid power' */
    double *total_charging_power;        /* 'Total charging power' */
    double *total_discharging_power;     /* 'Total discharging power' */
    double *battery_state_of_charge;     /* 'Battery state of charge' */
    double *total_vehicle_penalty;       /* 'Total vehicle penalty' */
    double *total_battery_penalty;       /* 'Total battery penalty' */
    double *grid_energy_cost;            /* 'Grid energy cost' */
    double *total_cost;                  /* 'Total cost' */
    double *utilized_solar_energy;       /* 'Utilized solar energy' */
    double *battery_power_value;         /* 'Battery power value' */
    double *battery_calculated_power;    /* 'Battery calculated power value' */
    double *nonexistent_vehicle_penalty; /* 'DisCharging nonexistent vehicles penalty' */
    double *initial_battery_soc;         /* 'Initial battery state of charge' */
    uint32_t *flags;                     /* SNG_FLAG_* raised by this step */
    double *episode_return;              /* accumulated: += reward (zeroed by every reset) */
    /* per charger, [num_envs][N] (row-major, env-major); NULL = not written */
    double *charger_power;               /* 'Charger power values' (charging_station.py:282-299) */
    double *vehicle_soc;                 /* SOC[c, t] after the step (charger.py:37-56/:86/:136) */
    /* device u32 [SNG_FLAG_SUMMARY_WORDS], NULL = not written: OR of the SNG_FLAG_* any env raised since the
     * caller last zeroed it, spread over SNG_FLAG_SUMMARY_WORDS words (the envs of one wavefront share a
     * word: word (first env of the wavefront / 32) mod SNG_FLAG_SUMMARY_WORDS), touched only when a flag is
     * raised, one atomic per wavefront.  A caller that watches these words instead of `flags` spares the step
     * its per-env flag store, and reads which envs raised what with sng_read_errors(clear = 1) only when a
     * word is non-zero.  (One shared word made every flagged wavefront's atomic wait on the same address: a
     * V2X station, which flags most envs every step, took ~10 us more per step at 65,536 envs.) */
    uint32_t *flag_summary;
} SngInfo;

/* A scenario in the reference's own layout (ChargingStation after
 * generate_new_initial_values / load_initial_values, charging_station.py:119-186):
 * per env and charger, 25-slot arrays plus padded arrival/departure lists (-1 = none). */
typedef struct SngScenario {
    int32_t slots;                 /* 25 (charger.py:16-19); T+1 with extended_day */
    int32_t max_vehicles;          /* padded list length */
    const double *soc;             /* [num_envs][N][slots]  'SOC' */
    const double *occupancy;       /* [num_envs][N][slots]  'Charger_occupancy' */
    const double *capacity;        /* [num_envs][N][slots]  'Vehicle_capacities' */
    const double *requested_soc;   /* [num_envs][N][slots]  'Requested_SOC' */
    const int32_t *arrivals;       /* [num_envs][N][max_vehicles]  'Arrivals' */
    const int32_t *departures;     /* [num_envs][N][max_vehicles]  'Departures' */
    const double *pv_ratio;        /* [num_envs] random_pv_shift_ratio */
} SngScenario;

typedef struct SngEnv SngEnv;
typedef struct SngGraph SngGraph;

int32_t sng_abi_version(void);
/* The library's build id: the first 12 hex digits of the SHA-256 of its sources (csrc/Makefile).  The
 * measurements committed under profiles/ name the build they were taken on by this id. */
const char *sng_build_id(void);

/* Fill `cfg` with the reference's defaults (N=8, '1h', b-pv, bounded, sparse). */
void sng_config_defaults(SngConfig *cfg);

/* SmartNanogridEnv.__init__ (smart_nanogrid_environment.py:32-120) for num_envs
 * independent environments on HIP device `device`.  Builds the PV/price tables
 * (pv_system_manager.py:10-91, accountant.py:48-101), allocates device state.
 * The BESS starts at bess_initial_soc and, as in the reference, is NOT reset by
 * sng_reset (central_management_system.py:93-94). */
int sng_create(const SngConfig *cfg, int device, int64_t num_envs, uint64_t seed, SngEnv **out);
void sng_destroy(SngEnv *env);
const char *sng_last_error(const SngEnv *env);
int sng_get_dims(const SngEnv *env, SngDims *out);
int sng_get_timestep(const SngEnv *env);

/* Global index of this handle's env 0 when one population of envs is sharded over several
 * GPUs/processes: env i then draws the streams of global env offset+i (reference RNG:
 * seed + offset + i; device RNG: hash-stream key of global env offset + i), so a sharded run reproduces the
 * single-GPU run bit for bit.  Call before reset. */
int sng_set_env_offset(SngEnv *env, int64_t offset);

/* SmartNanogridEnv.reset() (smart_nanogrid_environment.py:311-351) with generate_new_initial_values=True:
 * a new day for every env (charging_station.py:152-186), timestep 0, the t=0 observation into
 * obs[num_envs][obs_dim].  SNG_RNG_REFERENCE draws the days on the device too: numpy's and Python's
 * MT19937 stream of every env live there (ref_day2_kernel draws a day, the t = 0 observation's kernel the
 * PV ratio), and the next day's stream blocks are prepared on a side stream while this day is stepped.  Host
 * threads (the CPUs of sched_getaffinity, capped by SNG_HOST_THREADS / OMP_NUM_THREADS) only seed Python's
 * streams, once per seeding, and encode the injected days of sng_reset_from_scenario. */
int sng_reset(SngEnv *env, int rng_mode, float *obs, void *stream);

/* reset(generate_new_initial_values=False) (smart_nanogrid_environment.py:347-357): replays the day this
 * handle last generated with sng_reset, as ChargingStation.load_initial_values (charging_station.py:
 * 119-136) re-reads the initial_values.json the generation wrote (:185-186): arrivals, departures, SoC,
 * occupancy and capacities as generated, Requested_SOC left at the 0 clear_initialisation_variables
 * (:138-150) wrote (so no vehicle penalty), a new PV ratio (:349 -- reference RNG: each env's Python
 * stream, after the owed day-end draw; device RNG: a replay stream), BESS carried over.
 * SNG_ERR_STATE if nothing was generated yet or an injected day (sng_reset_from_scenario) replaced it. */
int sng_reset_replay(SngEnv *env, float *obs, void *stream);

/* Start a day from given days in the reference's layout (host memory): the recorded KAT days, or
 * days exported with sng_get_scenario.  scenario->pv_ratio may be NULL: each env then draws its ratio
 * from its Python stream (smart_nanogrid_environment.py:349) as a reset does; the day-end draw the
 * last step owes (:181) is consumed either way once the streams exist. */
int sng_reset_from_scenario(SngEnv *env, const SngScenario *scenario, float *obs, void *stream);

/* Reseed: env i draws the streams of seed + global index i from the next reset on (reference RNG:
 * np.random.seed / random.seed of that value; device RNG: the hash streams of that seed, from day 0).
 * The loaded day stays loaded.  Synchronises `stream`. */
int sng_set_seed(SngEnv *env, uint64_t seed, void *stream);

/* SmartNanogridEnv.step(actions) (smart_nanogrid_environment.py:140-188) for every env:
 * one fused kernel.  reward = -total cost (f64), done = 1 at the end of the day.
 * `info` may be NULL.  Asynchronous on `stream`. */
int sng_step(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
             const SngInfo *info, void *stream);

/* sng_step with the actions in host memory and the outputs returned to host memory: the one-env gym path
   (smart_nanogrid_environment.py:140-188 as SB3's DummyVecEnv and solvers/evaluator.py:13-24 drive it: one
   step per call, results on the host).  actions [E][act_dim] f32, obs [E][obs_dim] f32, reward [E] f64,
   done [E] u8 and step_flags [E] u32 (each env's SNG_FLAG_* bits raised in this step; the sticky per-env flags
   and the flag summary are updated as by sng_step) are ordinary host memory of the caller.  The step kernel
   reads the actions from and writes the outputs to a per-handle block of mapped host memory, so the call is
   one kernel dispatch and one wait on `stream` (synchronous: returns when the outputs are in the caller's
   arrays).  info as sng_step, except that SngInfo.flags must be null.  Meant for small batches; a large one
   belongs on sng_step with device buffers. */
int sng_step_host(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done, uint32_t *step_flags,
                  const SngInfo *info, void *stream);

/* The kernel name (as rocprofv3 reports it) of the step kernel sng_step would launch next with this
 * `info` (NULL allowed): "void sng::step_lean_kernel<N, PK, REQ>" for stations of N in {1,2,4,8,10,16}
 * chargers stepped with one lane per env, no diagnostics, NumPy-2 promotion, a power-of-two dt,
 * bounded charging and no stochastic profiles; "void sng::step_kernel<NC, L, DIAG, FAST, PK>" otherwise. */
int sng_step_kernel_name(const SngEnv *env, const SngInfo *info, char *buf, int32_t len);

/* Sticky per-env error flags (SNG_FLAG_*), copied to host after the work queued on `stream`;
 * synchronises that stream only. */
int sng_read_errors(SngEnv *env, uint32_t *host_flags, int clear, void *stream);

/* State access (host arrays of num_envs doubles; [num_envs][N] for the vehicle SoC), ordered after the
 * work queued on `stream`; each synchronises that stream only.  Attribute reads of the reference's
 * components: battery_energy_storage_system.py:108-109, random_pv_shift_ratio, charger.py:16. */
int sng_get_battery_soc(SngEnv *env, double *host_soc, void *stream);
int sng_set_battery_soc(SngEnv *env, const double *host_soc, void *stream);
int sng_get_pv_ratio(SngEnv *env, double *host_ratio, void *stream);
int sng_get_vehicle_soc(SngEnv *env, double *host_soc, void *stream);   /* SOC[c, t] of the last step */
int sng_set_vehicle_soc(SngEnv *env, const double *host_soc, void *stream);

/* Checkpoint / resume of the whole simulation: EV SoC [N][E], BESS SoC and the
 * day's initial SoC (central_management_system.py:93-94), PV ratio, t = 0 penalty, sticky flags, the
 * loaded day (timeline, requested-SoC stream, profile factors), the timestep, the device day counter,
 * the replay bookkeeping, the reference RNG streams when they exist, and -- when episode_return is
 * given (device [num_envs] f64, e.g. SngInfo.episode_return) -- the running day returns.  The blob is
 * host memory of sng_state_size bytes; sng_set_state accepts only a blob of a handle with the same
 * configuration, num_envs and ABI.  Both synchronise `stream`. */
int sng_state_size(const SngEnv *env, int with_episode_return, size_t *bytes);
int sng_get_state(SngEnv *env, void *host_buf, size_t bytes, const double *episode_return, void *stream);
int sng_set_state(SngEnv *env, const void *host_buf, size_t bytes, double *episode_return, void *stream);

/* The current day of envs [first, first + count) in the reference's initial_values.json layout
 * (ChargingStation.generated_initial_values_json, charging_station.py:164-191), decoded from the device
 * timeline -- for host-generated, device-generated and injected days alike.
 * soc / occupancy / capacity / requested_soc: host [count][N][slots]; arrivals / departures: host
 * [count][N][max_vehicles], -1 padded (n_vehicles[count][N] holds the full counts); pv_ratio: [count].
 * 'SOC' holds the arrival SoCs and the recorded SOC[c, t] of empty chargers (the slots a step
 * reads); Requested_SOC is exact when requested SoC is enabled or any penalised value differs
 * from 1.0, and 1.0 on occupied slots otherwise (0 everywhere on a replayed day).  Valid after a reset
 * until the next reset; synchronises `stream`. */
int sng_get_scenario(SngEnv *env, int64_t first, int64_t count, int32_t max_vehicles, double *soc,
                     double *occupancy, double *capacity, double *requested_soc, int32_t *arrivals,
                     int32_t *departures, int32_t *n_vehicles, double *pv_ratio, void *stream);

/* Constant tables as built at create (host copies; n = 2*T). */
int sng_get_tables(const SngEnv *env, double *irr, double *irr_max, double *pv_power, double *price,
                   double *price_max, int32_t *n);

/* `days` full days captured as one hipGraph: ([device-RNG reset] + the day's T steps) x days.
 * actions holds T consecutive [num_envs][act_dim] blocks (reused every day); obs/reward/done
 * are overwritten every step (but see SNG_GRAPH_TRAJECTORY); info may be NULL.  Replays draw new days each time.
 * Because every step's actions are known at capture and envs never interact, a day's T steps are one
 * graph node where the step plan has a day kernel: each wavefront steps its envs through the whole day with
 * SoC, BESS SoC and the day return in registers, and still stores every step's observation, reward, done and
 * flags.  The plans with a day kernel (csrc/sng_step_plan.h, day_kernel_of):
 *   - the lean family's (step_lean_kernel's stations: 1, 2, 4, 8 or 16 chargers, or 10 with V2X; no stochastic
 *     profiles, no diagnostics, NumPy-2 promotion, a power-of-two dt), for device-RNG days and for
 *     reference-RNG, injected and replayed days alike: day_lean_kernel;
 *   - packed device-RNG days of the 10-charger station without V2X or stochastic profiles: day_wide_kernel,
 *     which keeps only the last step's outputs, so not with SNG_GRAPH_TRAJECTORY.
 * What is in memory after the graph has run is bit for bit what T step nodes leave; only the intermediate
 * SoC / BESS SoC / day return of steps before the last are never written.  Every other plan (50 chargers, the
 * general kernel's stations, any SngInfo diagnostics), and SNG_GRAPH_STEP_NODES, captures T dependent step
 * nodes.
 * SNG_GRAPH_TRAJECTORY keeps every step of every captured day instead of overwriting one block: obs is then
 * [days][T + 1][num_envs][obs_dim] f32, reward [days][T][num_envs] f64 and done [days][T][num_envs] u8.  Block
 * [d][0] of obs is day d's t = 0 observation: the graph's reset writes it with SNG_GRAPH_RESET, a steps-only
 * graph leaves it to the caller.  Step t writes obs[d][t + 1], reward[d][t] and done[d][t]; day_returns and info
 * are as without the flag.
 * flags: SNG_GRAPH_*; days > 1 needs SNG_GRAPH_RESET.
 * day_returns (device [days][num_envs] f64, may be NULL): day d's returns accumulate into row
 * d instead of info->episode_return, so a replay leaves every day's returns for one
 * collective per replay (bench.py gathers them over RCCL while the next replay runs).
 * Without SNG_GRAPH_RESET the graph steps the day that is loaded at launch, from t = 0: device-RNG days,
 * host-RNG / injected days and replayed days are stepped with different encodings (sng_layout.h:
 * packed records, requested-SoC stream, cleared Requested_SOC, day-counter ownership), so launching a
 * steps-only graph over a day of another encoding than at capture, or after t = 0, fails with
 * SNG_ERR_STATE.
 * A reset graph of two or more days without SNG_GRAPH_TRAJECTORY, at the stations whose day measured shorter that
 * way (csrc/sng_graph_form.h, reset_overlapped: 10 chargers without V2X or stochastic profiles), generates day
 * d + 1 while day d is stepped: the generator nodes sit on a parallel branch
 * of the graph and write every other day into a second set of day buffers the handle allocates for this (about
 * the size of one packed day).  The days drawn, the outputs, the day returns and the state the graph leaves --
 * the last day is always in the handle's own buffers -- are bit for bit those of the serial chain; only the
 * t = 0 observation of each day, which step 0 overwrites in the same block, is never written.  Parallel branches
 * need the process's default of 4 hardware queues.  SNG_GRAPH_SERIAL_RESET captures the serial chain (every
 * day's generator, then its steps); SNG_GRAPH_OVERLAPPED_RESET overlaps at every station whose device reset is
 * one launch (about 60 chargers), also where the serial chain measured no slower and is the default (the lean
 * stations, 50 chargers).  The serial flag wins over it, and so do one day and a kept trajectory.
 * The default station -- 10 chargers, 1 h steps, PV, BESS, bounded charging, no V2X, no requested SoC, no stochastic
 * profiles, NumPy-2 promotion -- steps its generated days with day_station_kernel, day_wide_kernel with those
 * switches fixed at compile time (csrc/sng_step_plan.h, day_station_fixed); the results are the same bit for bit.
 * SNG_GRAPH_GENERIC_DAY captures day_wide_kernel there too. */
#define SNG_GRAPH_RESET 1        /* start every day with a device-RNG reset */
#define SNG_GRAPH_STEP_NODES 2   /* one graph node per step even where a day kernel exists (A/B, tests) */
#define SNG_GRAPH_TRAJECTORY 4   /* obs / reward / done hold every step of every day (shapes above) */
#define SNG_GRAPH_SERIAL_RESET 8 /* no generator beside the previous day's steps (A/B, tests) */
#define SNG_GRAPH_OVERLAPPED_RESET 16 /* ... and beside them at every station whose reset is one launch (A/B, tests) */
#define SNG_GRAPH_POLICY_FUSED 32 /* sng_graph_create_policy: the fused day wherever it is compiled (A/B, tests) */
#define SNG_GRAPH_GENERIC_DAY 64 /* day_wide_kernel also where the station-fixed day kernel would run (A/B, tests) */
int sng_graph_create(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
                     const SngInfo *info, int flags, int32_t days, double *day_returns, SngGraph **out);
int sng_graph_launch(SngGraph *graph, void *stream);
/* The kernel of the graph's day-kernel nodes as rocprofv3 names it, e.g. "void sng::day_station_kernel<10, 2>" or
 * "void sng::day_wide_kernel<10, 2, false, false>"; an empty string for step nodes and for a policy graph. */
int sng_graph_day_kernel_name(const SngGraph *graph, char *buf, int32_t len);
/* Graph nodes that step one day: 1 with the day kernel, else T; a policy graph's node form has 2T (-1 for NULL). */
int sng_graph_step_nodes(const SngGraph *graph);
/* 1: the graph generates day d + 1 beside day d's steps (above); 0: the serial chain (-1 for NULL). */
int sng_graph_reset_overlapped(const SngGraph *graph);
/* The captured graph as text, one line per node in hipGraphGetNodes order: "<index> <type>", for a kernel node its name
 * (hipKernelNameRefByPtr), "grid=(x,y,z) block=(x,y,z) lds=<dynamic LDS bytes>", and "deps=[...]", the indices of the
 * nodes it depends on, ascending.  Returns the text's length without its NUL (buf holds the text when that is below
 * len; else call again with more room), or a negative SNG_ERR_* code.  For tests and A/B tools: what a capture made. */
int sng_graph_describe(const SngGraph *graph, char *buf, int64_t len);
/* Kernel-time probe: runs `days` device-RNG days eagerly (as the graph does) and returns the
 * device time (ms) of every step kernel, ms[days*T], from HIP start/stop events attached to
 * each dispatch (hipExtLaunchKernel: the dispatch's own begin/end timestamps), and, when reset_ms
 * is not NULL, of every day's device reset, reset_ms[days] (the one-launch generator the same way;
 * wide stations' generator + profile + observe0 launches between recorded events).  ms = NULL: the
 * days are launched without per-dispatch events (back to back, for a caller's own timing).  Synchronises. */
int sng_time_step_kernels(SngEnv *env, const float *actions, float *obs, double *reward, uint8_t *done,
                          const SngInfo *info, int32_t days, float *ms, float *reset_ms, void *stream);
void sng_graph_destroy(SngGraph *graph);

/* ---------------------------------------------------------------------------------------------
 * Policy in the loop: the actor of the reference's own workload, PPO("MlpPolicy", env)
 * (solvers/RL/ppo_train.py:92), evaluated on the device between steps, so a day whose step t + 1 actions depend on
 * step t's observation runs without a torch kernel in between.
 *
 * The actor's arithmetic is one contract, the same on the host (sng_policy_host_actions) and on the device.  x is
 * an env's observation row; weights are in torch's nn.Linear layout [out][in]; every layer's output j is the
 * k-ordered float32 fmaf chain started from the bias:
 *     h = b[j];  for k = 0 .. K-1:  h = fmaf(in[k], W[j][k], h)
 * Two hidden layers of 64 units with tanh or relu (relu(h) = h > 0 ? h : 0); the output layer has no activation and
 * gives the mean; a = mean + noise (one float32 add) when a noise block is given, else the mean; `a` is what is
 * stored as the step's action, and the env is stepped with min(max(a, low), high) when the spec has clip bounds,
 * else with a.  With relu the device reproduces the host bit for bit; with tanh up to the device's tanhf.
 * Another hidden width returns SNG_ERR_UNSUPPORTED; non-finite weights are refused at upload
 * (SNG_ERR_INVALID_ARGUMENT); what non-finite observations give is unspecified. */
typedef struct SngMlpSpec {
    int32_t obs_dim, act_dim;
    int32_t hidden;                 /* 64 */
    int32_t activation;             /* 0 tanh, 1 relu */
    const float *clip_low, *clip_high;   /* host [act_dim]; both NULL = no clip */
} SngMlpSpec;
typedef struct SngMlpWeights {      /* host memory, [out][in] and [out] */
    const float *w1, *b1;           /* [64][obs_dim], [64] */
    const float *w2, *b2;           /* [64][64], [64] */
    const float *w3, *b3;           /* [act_dim][64], [act_dim] */
} SngMlpWeights;
typedef struct SngPolicy SngPolicy;

/* An actor for `env`: spec->obs_dim and act_dim must be the env's.  Its weights are zero until
 * sng_policy_set_weights.  A policy must outlive the graphs created with it and be destroyed before its env. */
int sng_policy_create(SngEnv *env, const SngMlpSpec *spec, SngPolicy **out);
/* Upload into the policy's device image, asynchronously on `stream`.  Captured graphs read that image, so new
 * weights between two launches change the next launch without a recapture (one PPO iteration). */
int sng_policy_set_weights(SngPolicy *policy, const SngMlpWeights *weights, void *stream);
/* One launch (policy_kernel) over the env's num_envs rows: obs [num_envs][obs_dim], noise [num_envs][act_dim] or
 * NULL, actions [num_envs][act_dim] (a), env_actions [num_envs][act_dim] or NULL (what sng_step is to be given);
 * device pointers.  Works at every station.  Asynchronous on `stream`. */
int sng_policy_actions(SngPolicy *policy, const float *obs, const float *noise, float *actions, float *env_actions,
                       void *stream);
void sng_policy_destroy(SngPolicy *policy);

/* sng_graph_create with the policy in the loop: every step's actions are the actor's answer to the observation the
 * step before it (or the day's reset) wrote.  noise holds T consecutive [num_envs][act_dim] blocks reused every
 * day, or is NULL.  flags, days, day_returns, info and obs / reward / done are sng_graph_create's, the steps-only
 * rules (the loaded day's encoding, t = 0) included; a steps-only graph reads the day's t = 0 observation from obs
 * (block [0][0] with SNG_GRAPH_TRAJECTORY), where the reset or the caller left it.  actions_out receives a: one block
 * [num_envs][act_dim] that every step overwrites, or [days][T][num_envs][act_dim] with SNG_GRAPH_TRAJECTORY.
 * The form of a day is decided per plan in csrc/sng_graph_form.h (policy_day_form).  Node form: T x (policy_kernel
 * node, step node), the step nodes being those of sng_graph_create; sng_graph_step_nodes reports 2T.  Fused form: one
 * node a day, day_lean_policy_kernel, the lean day kernel with the actor between its steps (one wavefront per 64
 * envs, the observation and the actions never leave LDS between the actor and the step); sng_graph_step_nodes
 * reports 1.  The fused form exists for the plans with a lean day kernel; it is a plan's default only where its day
 * measured shorter than the node form's (nowhere in this build: DESIGN.md section 4.6, profiles/policy_day_ab.txt),
 * and SNG_GRAPH_POLICY_FUSED takes it wherever it exists.  SNG_GRAPH_STEP_NODES and SngInfo diagnostics force the
 * node form.  Both forms leave the same bytes.  Policy graphs capture the serial chain: sng_graph_reset_overlapped
 * gives 0, whatever the reset flags. */
int sng_graph_create_policy(SngEnv *env, SngPolicy *policy, const float *noise, float *obs, float *actions_out,
                            double *reward, uint8_t *done, const SngInfo *info, int flags, int32_t days,
                            double *day_returns, SngGraph **out);

/* Host only: the actor's contract on the CPU (csrc/sng_policy_host.h, mlp_actor_host) over `rows` rows of host
 * memory.  noise and env_actions may be NULL.  Validates as sng_policy_create and sng_policy_set_weights do. */
int sng_policy_host_actions(const SngMlpSpec *spec, const SngMlpWeights *w, int64_t rows, const float *obs,
                            const float *noise, float *actions, float *env_actions);

/* ---------------------------------------------------------------------------------------------
 * Actors of any width, and the squashed output: SB3's DDPG / TD3 actor (solvers/RL/ddpg_train.py;
 * Linear(O, 400) - ReLU - Linear(400, 300) - ReLU - Linear(300, A) - Tanh, rescaled into the action Box), SAC's
 * 256-256 and a PPO actor with its own net_arch.
 *
 * The contract is SngMlpSpec's, with two hidden widths of their own: every layer's output j is the k-ordered float32
 * fmaf chain started from the bias, over the layer's real K inputs.  The device (policy_net_kernel, on the f32-input
 * MFMA, whose result is that chain) may append zero-input, zero-weight terms after a chain's last real term, and a
 * chain with such terms gives +0 where the chain without them gives -0: that sign of a zero is the only bit the
 * padding can change, so device and host are compared by value (==), and with relu hidden layers they are equal
 * that way; with tanh they are equal up to the device's tanhf.
 *
 * output = SNG_MLP_OUT_MEAN: as SngMlpSpec -- a = mean (+ noise), and the env is stepped with min(max(a, low), high)
 * where bounds are given, else with a.
 * output = SNG_MLP_OUT_SQUASH: s = tanh(mean); with noise s = min(max(s + noise, -1), 1) (SB3's _sample_action: the
 * noise is added and clipped in the [-1, 1] domain); a = s is what is stored; and the env is stepped with SB3's
 * unscale_action as numpy evaluates it in float32,
 *     env = low[j] + ((0.5f * (s + 1.0f)) * d[j]),   d[j] = high[j] - low[j] (float32, computed once per policy),
 * the product and the sum each rounded on their own (no fused multiply-add).  low / high are the action Box and
 * must be finite.
 *
 * Refusals: a hidden width outside 8 .. 512, an act_dim above 64 (the kernel keeps two output tiles of 32: stations
 * of up to 63 chargers with a battery, 64 without; the message names act_dim), or a combination of widths and obs_dim
 * whose LDS tiles do not fit a compute unit's 160 KB (the message names the sizes), is SNG_ERR_UNSUPPORTED -- every
 * pair of widths up to 512 fits at stations of up to 50 chargers (obs_dim 109).  sng_policy_net_host_actions refuses
 * the same specs, although the host model itself has no such limits.  Dims that are not the env's, a bad activation or output,
 * bounds that are unordered, half given or (SQUASH) missing or not finite, and non-finite weights are
 * SNG_ERR_INVALID_ARGUMENT. */
#define SNG_MLP_OUT_MEAN   0   /* as SngMlpSpec: a = mean (+ noise); env action = clip(a) where bounds are given */
#define SNG_MLP_OUT_SQUASH 1   /* s = tanh(mean); with noise s = min(max(s + noise, -1), 1); a = s is stored;
                                  env action = low + (0.5f * (s + 1.0f)) * (high - low)                          */
typedef struct SngMlpNetSpec {
    int32_t obs_dim, act_dim;
    int32_t hidden1, hidden2;      /* each 8 .. 512, any integer */
    int32_t activation;            /* hidden layers: 0 tanh, 1 relu */
    int32_t output;                /* SNG_MLP_OUT_* */
    const float *low, *high;       /* host [act_dim]: MEAN: clip bounds or both NULL; SQUASH: the Box, required */
} SngMlpNetSpec;
/* An actor of that net for `env`.  SngMlpWeights holds w1 [hidden1][obs_dim], w2 [hidden2][hidden1] and
 * w3 [act_dim][hidden2] with their biases.  The policy that comes back is sng_policy_create's in every other call:
 * sng_policy_set_weights, sng_policy_actions (one policy_net_kernel launch; a 64-64 MEAN net runs that kernel too),
 * sng_graph_create_policy and sng_policy_destroy.  Its captured days are always in node form, T x
 * (policy_net_kernel node, step node): SNG_GRAPH_POLICY_FUSED is accepted and gives nodes
 * (csrc/sng_graph_form.h, policy_net_day_form). */
int sng_policy_create_net(SngEnv *env, const SngMlpNetSpec *spec, SngPolicy **out);
/* Host only: that contract on the CPU (csrc/sng_policy_net_host.h, mlp_net_host), over the chains' real terms.
 * For a 64-64 MEAN spec it gives what sng_policy_host_actions gives.  Validates as sng_policy_create_net and
 * sng_policy_set_weights do. */
int sng_policy_net_host_actions(const SngMlpNetSpec *spec, const SngMlpWeights *w, int64_t rows, const float *obs,
                                const float *noise, float *actions, float *env_actions);

/* ---------------------------------------------------------------------------------------------
 * The rest of a PPO rollout: critic values, log-probabilities and generalised advantage estimates of the days a
 * policy graph with SNG_GRAPH_TRAJECTORY left, in one launch.  With them a caller holds everything SB3's RolloutBuffer
 * holds (observations, actions, rewards, episode starts, values, log-probs, advantages, returns) as device arrays.
 * The contract is engine-independent, as SngMlpSpec's: one arithmetic, on the host (sng_ppo_host_finish,
 * csrc/sng_ppo_host.h) and on the device (rollout_gae_kernel, csrc/sng_ppo.h); with relu the device reproduces the host
 * bit for bit, with tanh the values up to the device's tanhf and the rest exactly, given those values.
 *
 * Value net: the second net of SB3's ActorCriticPolicy (mlp_extractor.value_net.{0,2}, value_net), 64-64 with the
 * actor's activation.  Its arithmetic is SngMlpSpec's with act_dim = 1, no noise and no clip: every output is the
 * k-ordered float32 fmaf chain started from the bias, and V is the output layer's one chain.  SngMlpWeights holds
 * w3 [1][64] and b3 [1].
 *
 * GAE: numpy's float32 evaluation of RolloutBuffer.compute_returns_and_advantage, per env and per day, walking
 * t = T-1 .. 0 with gae = 0.0f before t = T-1; every operation is rounded on its own (no fused multiply-add):
 *     g  = (float)gamma                      gl = (float)((double)gamma * (double)gae_lambda)
 *     r  = (float)reward[d][t][e]            nn = 1.0f - (float)done[d][t][e]
 *     delta = ((r + ((g * V[d][t+1][e]) * nn)) - V[d][t][e])
 *     gae   = delta + ((gl * nn) * gae)
 *     advantages[d][t][e] = gae              returns[d][t][e] = gae + V[d][t][e]
 * V[d][T] is the value of obs[d][T] (SB3's last_values, with buffer_size = T).  done is terminal (the env reports no
 * truncation), so there is no bootstrap through it; days are independent scans, which with the env's own done (1 at
 * every day's last step) is SB3's one scan over days * T steps.  gamma and gae_lambda must be finite and in [0, 1].
 *
 * Log-probability of the sampled action under SB3's DiagGaussianDistribution, from the noise the actor added
 * (a = mean + noise): inv_std[j] = 1.0f / expf(log_std[j]) is computed once on the host when the weights are uploaded
 * and stored in the device image next to log_std[j]; per row, in j order, every operation rounded on its own:
 *     lp = 0.0f;  for j:  z = noise[t][e][j] * inv_std[j]
 *                         lp = lp + ((((-0.5f * z) * z) - log_std[j]) - 0.91893853f)
 * noise is sng_graph_create_policy's block [T][num_envs][act_dim], reused every day; logp is [days][T][num_envs] all
 * the same.  A NULL noise or a NULL logp skips the stage.
 *
 * Non-finite value weights and a non-finite log_std are refused at upload, a gamma or gae_lambda outside [0, 1] (or
 * NaN), days < 1 and a NULL required pointer at the call: SNG_ERR_INVALID_ARGUMENT, the reason in sng_last_error. */
typedef struct SngPpo SngPpo;
typedef struct SngPpoRollout {          /* device pointers (host pointers for sng_ppo_host_finish) */
    int32_t days;
    double gamma, gae_lambda;
    const float *obs;                   /* [days][T+1][num_envs][obs_dim] */
    const double *reward;               /* [days][T][num_envs] */
    const uint8_t *done;                /* [days][T][num_envs] */
    const float *noise;                 /* [T][num_envs][act_dim] or NULL */
    float *values;                      /* [days][T+1][num_envs] */
    float *advantages, *returns;        /* [days][T][num_envs] */
    float *logp;                        /* [days][T][num_envs] or NULL */
} SngPpoRollout;
/* A head for `env` (its obs_dim, act_dim, T and num_envs); activation: 0 tanh, 1 relu.  The value net's weights and
 * log_std are zero until sng_ppo_set_weights.  Destroyed before its env, as a policy is. */
int sng_ppo_create(SngEnv *env, int32_t activation, SngPpo **out);
/* Upload into the head's device image, asynchronously on `stream`: new weights between two sng_ppo_finish calls
 * change the next one.  log_std: host [act_dim], or NULL for zeros (SB3's log_std_init). */
int sng_ppo_set_weights(SngPpo *ppo, const SngMlpWeights *value_net, const float *log_std, void *stream);
/* One launch (rollout_gae_kernel), asynchronous on `stream`: no synchronisation and no allocation.  Launched after a
 * day graph on the same stream it finishes that graph's trajectory.  At most 65535 days in one call (more is
 * SNG_ERR_INVALID_ARGUMENT; the host entry point has no such limit). */
int sng_ppo_finish(SngPpo *ppo, const SngPpoRollout *rollout, void *stream);
/* Host only: the same contract on host arrays.  values_given != 0: `values` is read, not computed (obs and value_net
 * may then be NULL).  Validates as sng_ppo_set_weights and sng_ppo_finish do. */
int sng_ppo_host_finish(int32_t obs_dim, int32_t act_dim, int32_t activation, int32_t T, int64_t E,
                        const SngMlpWeights *value_net, const float *log_std, const SngPpoRollout *host_arrays,
                        int values_given);
void sng_ppo_destroy(SngPpo *ppo);

/* ---------------------------------------------------------------------------------------------
 * The same for a value net of any two hidden widths: the critic of PPO("MlpPolicy", env,
 * policy_kwargs=dict(net_arch=...)), beside an actor made by sng_policy_create_net (or the 64-64 one: SB3's
 * dict(pi=..., vf=...) lets the two differ).
 *
 * The contract.  Values are SngMlpNetSpec's arithmetic with act_dim = 1, SNG_MLP_OUT_MEAN, no noise and no clip:
 * every layer's output is the k-ordered float32 fmaf chain started from the bias over the layer's real K inputs, and V
 * is the output layer's one chain.  Its host model is mlp_net_host (csrc/sng_policy_net_host.h) on a NetImage packed
 * for (obs_dim, 1, hidden1, hidden2); the head's device image is that NetImage followed by log_std | inv_std as the
 * section above lays them out (csrc/sng_ppo_net_host.h).  The device (value_net_kernel, csrc/sng_ppo_net.h, on the
 * f32-input MFMA) may append zero-input, zero-weight terms after a chain's last real term, which can turn a -0 into
 * +0 and nothing else, so values are compared by value (==): with relu they are equal, with tanh equal up to the
 * device's tanhf.  GAE and the log-probability are exactly the formulas of the section above, each operation rounded
 * on its own (gae_scan_kernel); given the stored values they are bitwise the host's.  noise [T][num_envs][act_dim] is
 * reused every day; a NULL noise or a NULL logp skips the stage and leaves logp untouched.
 *
 * Refusals.  A hidden width outside 8 .. 512, or widths and an obs_dim whose LDS tiles do not fit a compute unit's
 * 160 KB (net_spec_check's rule for act_dim = 1; the message names the sizes: every pair of widths up to 512 fits
 * at stations of up to 50 chargers), or an act_dim above 255, is SNG_ERR_UNSUPPORTED.  A bad activation, non-finite
 * weights or log_std, a gamma or gae_lambda outside [0, 1], days < 1 and NULL required pointers are
 * SNG_ERR_INVALID_ARGUMENT.  In one sng_ppo_finish of a net head the days are rows of gae_scan_kernel's grid, and with
 * the log-probability stage the T steps are T more: days (+ T with noise and logp) is at most 65535, and the
 * days * (T + 1) * num_envs / 64 workgroups of value_net_kernel at most 2^31 - 1 (a grid's x dimension); more is
 * SNG_ERR_INVALID_ARGUMENT with the reason.  The host entry point refuses the same specs and has no launch limits. */
typedef struct SngPpoNetSpec {
    int32_t hidden1, hidden2;      /* each 8 .. 512, any integer */
    int32_t activation;            /* hidden layers: 0 tanh, 1 relu */
} SngPpoNetSpec;
/* A head of that value net for `env`.  SngMlpWeights holds w1 [hidden1][obs_dim], w2 [hidden2][hidden1] and
 * w3 [1][hidden2] with their biases.  The handle that comes back is sng_ppo_create's in every other call:
 * sng_ppo_set_weights (new weights between two sng_ppo_finish calls change the next one), sng_ppo_destroy, and
 * sng_ppo_finish, which for a net head is two launches on `stream`, value_net_kernel then gae_scan_kernel, with no
 * allocation and no synchronisation.  A (64, 64) net head runs these kernels too, not rollout_gae_kernel. */
int sng_ppo_create_net(SngEnv *env, const SngPpoNetSpec *spec, SngPpo **out);
/* Host only: the net head's contract on host arrays, as sng_ppo_host_finish is the 64-64 head's (values_given != 0:
 * `values` is read, not computed; obs and value_net may then be NULL).  For a (64, 64) spec it gives what
 * sng_ppo_host_finish gives.  Validates as sng_ppo_create_net, sng_ppo_set_weights and sng_ppo_finish do. */
int sng_ppo_net_host_finish(int32_t obs_dim, int32_t act_dim, const SngPpoNetSpec *spec, int32_t T, int64_t E,
                            const SngMlpWeights *value_net, const float *log_std,
                            const SngPpoRollout *host_arrays, int values_given);

/* ---------------------------------------------------------------------------------------------
 * Action noise: the exploration noise a policy graph's actor adds, drawn by the library -- the sample of PPO's
 * Gaussian head, SB3's NormalActionNoise, and SB3's OrnsteinUhlenbeckActionNoise (DDPG: solvers/RL/ddpg_train.py:111
 * trains with sigma = 0.5 and mean 0).  A source has one kernel (action_noise_kernel, csrc/sng_noise.h) and a host model
 * (sng_noise_host_fill) compiled from the same text (csrc/sng_noise_host.h), which the kernel reproduces bit for bit:
 * every operation is an integer operation, an fmaf, or a float32 add / multiply rounded on its own.
 *
 * Stream.  The variate of (seed, global env ge = env offset + e, action j, counter c, step t) comes from the hash
 *     h = mix32(key + t * 0x9e3779b9u)
 * with mix32 the device generator's ("triple32") and key a stream_key-style mix of (seed, ge, 0x6e7a0000 | j, c) in
 * which all 64 bits of ge and of c take part (noise_key); j < 256.  So a sharded population draws what one population
 * draws, and a block depends on nothing but its counter.
 *
 * Standard normal z from h, without a transcendental: sign = h >> 31, u = max(h & 0x7fffffff, 1), p = (u + 0.5) 2^-32
 * in (0, 0.5); octave k = 30 - msb(u) (31 of them); the bits below u's leading one, left-aligned, give a 2-bit
 * sub-segment and a 24-bit fraction x in [0, 1); r = max(fmaf(fmaf(fmaf(c3, x, c2), x, c1), x, c0), 2^-32) with the
 * segment's four float32 coefficients from a table [31][4][4] fitted against float64 -ndtri(p) (tools/fit_noise_table.py);
 * z = sign ? -r : r.  |z - ndtri| <= 2^-18 (measured 2.2e-6), |z| <= 6.17, z is never 0.
 *
 * Kinds, per action j with mu[j] and scale[j] (scale >= 0):
 *   SNG_NOISE_GAUSSIAN   n[t] = mu[j] + scale[j] * z[t]          (PPO: scale = exp(log_std); NormalActionNoise)
 *   SNG_NOISE_OU         x = 0 at every block's start (SB3 resets the process at an episode's end); for t = 0 .. T-1
 *                        x = (x + ((theta * (mu[j] - x)) * dt)) + (sd[j] * z[t]),   n[t] = x,
 *                        sd[j] = (float)(scale[j] * sqrt(dt)) formed in double at upload; theta and dt are used as
 *                        float32 (SB3's defaults: theta 0.15, dt 1e-2).
 *
 * Counter.  A source owns a uint64 on the device (not the env's day counter, and not in a checkpoint blob): a fill of
 * `days` blocks [T][num_envs][act_dim] uses counters c, c + 1, .., and a one-thread kernel behind the fill adds `days`.
 *
 * Refusals (SNG_ERR_INVALID_ARGUMENT, the message names the value): a kind that is neither, an act_dim outside
 * 1 .. 255 or not the env's, non-finite mu / scale / theta / dt, a negative scale (or dt, for OU), days < 1, NULL
 * required pointers. */
#define SNG_NOISE_GAUSSIAN 0
#define SNG_NOISE_OU       1
typedef struct SngNoiseSpec {
    int32_t kind;                   /* SNG_NOISE_* */
    int32_t act_dim;                /* the env's, 1 .. 255 */
    uint64_t seed;
    double theta, dt;               /* SNG_NOISE_OU; finite for both kinds */
} SngNoiseSpec;
typedef struct SngNoise SngNoise;

/* A source for `env` (its act_dim, T and num_envs), counter 0, mu and scale zero until sng_noise_set_params.  Destroyed
 * before its env and after the graphs created with it. */
int sng_noise_create(SngEnv *env, const SngNoiseSpec *spec, SngNoise **out);
/* Upload mu (host [act_dim], or NULL for zeros) and scale (host [act_dim]), asynchronously on `stream`: fills and
 * captured graphs read the uploaded image, so new values between two launches change the next launch without a
 * recapture, as weights do. */
int sng_noise_set_params(SngNoise *noise, const float *mu, const float *scale, void *stream);
/* `days` blocks into out (device [days][T][num_envs][act_dim] f32): the fill launch and the counter's bump, asynchronous
 * on `stream`, with no allocation and no synchronisation.  The env offset is read when the call is enqueued. */
int sng_noise_fill(SngNoise *noise, float *out, int32_t days, void *stream);
/* The counter the next fill starts from, for checkpoints; both synchronise `stream`. */
int sng_noise_get_counter(SngNoise *noise, uint64_t *out, void *stream);
int sng_noise_set_counter(SngNoise *noise, uint64_t counter, void *stream);
void sng_noise_destroy(SngNoise *noise);
/* Host only: the blocks a source with this spec, mu (NULL: zeros) and scale gives envs env_offset .. env_offset + E - 1
 * from `counter` on, into out (host [days][T][E][act_dim]).  Validates as the device calls do. */
int sng_noise_host_fill(const SngNoiseSpec *spec, const float *mu, const float *scale, int32_t T, int64_t E,
                        int64_t env_offset, uint64_t counter, int32_t days, float *out);
/* sng_graph_create_policy with a source in the place of the caller's noise: the graph's first nodes are one fill of all
 * `days` blocks into noise_out (device [days][T][num_envs][act_dim]) and the counter's bump, on the serial chain, and
 * day d's actor reads block d -- in the node form and in the fused form alike -- so every day explores with its own
 * sample and every replay draws new days.  Everything else is sng_graph_create_policy's, whose own one-block behaviour
 * is unchanged. */
int sng_graph_create_policy_noise(SngEnv *env, SngPolicy *policy, SngNoise *noise_source, float *noise_out, float *obs,
                                  float *actions_out, double *reward, uint8_t *done, const SngInfo *info, int flags,
                                  int32_t days, double *day_returns, SngGraph **out);

/* ---------------------------------------------------------------------------------------------
 * The off-policy side of DDPG / TD3 (solvers/RL/ddpg_train.py): a replay ring of whole days, its sampler, the critic
 * Q(s, a) and the TD targets -- everything between "a closed-loop day ended" and "the caller holds a minibatch and its
 * targets", on the device, each with an exact host model (csrc/sng_ddpg_host.h).  The gradient step and the polyak
 * update follow below (sng_learner_create); a caller who keeps them in torch uploads the weights they give, as with PPO.
 *
 * Replay ring.  capacity_days slots, each one day of a policy graph's SNG_GRAPH_TRAJECTORY outputs, in device storage
 * the caller provides at create and keeps alive until destroy (as a graph's outputs are the caller's):
 *     obs     [capacity_days][T + 1][num_envs][obs_dim] f32
 *     actions [capacity_days][T][num_envs][act_dim]     f32   the stored a: for a squashed actor the [-1, 1] action,
 *                                                             which is what SB3's ReplayBuffer stores
 *     reward  [capacity_days][T][num_envs]              f32   (float)reward: SB3's buffer is float32
 *     done    [capacity_days][T][num_envs]              u8
 * A push of `days` days (1 <= days <= capacity_days; more is refused) writes slots head, head + 1, .. (mod
 * capacity_days) in one launch, then head advances by days (mod capacity_days) and filled = min(filled + days,
 * capacity_days); both start at 0.  Transition i < n = filled * T * num_envs is
 *     (slot, t, e) = (i / (T * num_envs), (i / num_envs) % T, i % num_envs)
 * in physical slot order.  Its next observation is obs[slot][t + 1][e]; for t = T - 1 that is the day's terminal
 * observation, which the trajectory holds in block T (the next day's reset is in the next slot's block 0).  done is
 * terminal (the env reports no truncation), so there is no timeout mask.
 *
 * Sampling law, in integer operations only, so the device equals the host (sng_replay_host_indices) bit for bit.  Row b
 * of the sample with counter c takes
 *     key = mix32(mix32(day_key(seed, c) ^ lo32(off)) ^ (hi32(off) * 0x85ebca6b + 0x72730000 * 0xc2b2ae35 + 0x27d4eb2f))
 *     kb  = mix32(mix32(key ^ lo32(b)) ^ (hi32(b) * 0x85ebca6b + 0x165667b1))
 *     h   = (uint64)mix32(kb + 0x9e3779b9) << 32 | mix32(kb + 2 * 0x9e3779b9)
 *     index = (h * n) >> 64        the high word of the 128-bit product; the bias is below n / 2^64
 * with mix32 and day_key the action noise's (noise_mix32, noise_day_key), off the env offset when the call is enqueued
 * and 0x72730000 the sampler's own domain tag.  One text is compiled for both sides.  The counter is a host-side
 * uint64 of the handle, 0 at create, read by a sample call and bumped by one per sample call; sng_replay_get_counter /
 * sng_replay_set_counter read and set it without touching the device.  A sample captured into the caller's own graph
 * therefore repeats itself: its counter was baked into the captured launch.
 *
 * Sample output: SB3's ReplayBufferSamples as dense device arrays -- obs [batch][obs_dim], actions [batch][act_dim],
 * next_obs [batch][obs_dim], reward [batch] f32, done [batch] f32 (0.0 / 1.0) and, where given, index [batch] i64.
 * Sampling an empty ring or batch < 1 is refused.
 *
 * Critic.  Q(s, a) is SngMlpNetSpec's arithmetic with obs_dim := obs_dim + act_dim, act_dim := 1, SNG_MLP_OUT_MEAN, no
 * noise and no clip, on the input row x = [obs row | action row]: every output is the k-ordered float32 fmaf chain
 * started from the bias; SngMlpWeights holds w1 [hidden1][obs_dim + act_dim], w2 [hidden2][hidden1], w3 [1][hidden2].
 * The device (q_net_kernel, csrc/sng_ddpg.h: policy_net_kernel's trunk with its rows staged from two arrays) may append
 * zero terms to a chain, so device and host are compared by value (==), as value_net_kernel's values are: equal with
 * relu, equal up to the device's tanhf with tanh.  The refusals are net_spec_check's for that input width, and the
 * message names the sizes: widths outside 8 .. 512 and LDS tiles above a compute unit's 160 KB are SNG_ERR_UNSUPPORTED
 * (at 50 chargers the input width is 160: 400-300 needs 147,968 B and fits, 512-512 needs 172,544 B and does not).
 *
 * TD target: SB3's TD3.train with n_critics = 1 and no target-policy noise, each float32 operation rounded on its own:
 *     a' = the target actor's stored action for next_obs   (SNG_MLP_OUT_SQUASH: tanh(mean); no noise)
 *     q' = Q_target(next_obs, a')
 *     nn = 1.0f - done;   y = reward + ((nn * (float)gamma) * q')
 * gamma must be finite and in [0, 1].  Given the device's a' the device's y equals the host's by value with relu.
 *
 * Every device call below is asynchronous on `stream`, and none allocates or synchronises after create.  Row counts and
 * offsets are 64-bit.  Handles are destroyed before their env. */
typedef struct SngReplaySpec {
    int32_t capacity_days;          /* >= 1 */
    uint64_t seed;                  /* of the sampler's streams */
    float *obs, *actions, *reward;  /* device storage, shapes above */
    uint8_t *done;
} SngReplaySpec;
typedef struct SngReplayBatch {     /* device pointers */
    float *obs, *actions, *next_obs;    /* [batch][obs_dim], [batch][act_dim], [batch][obs_dim] */
    float *reward, *done;               /* [batch] */
    int64_t *index;                     /* [batch] or NULL */
} SngReplayBatch;
typedef struct SngReplay SngReplay;
int sng_replay_create(SngEnv *env, const SngReplaySpec *spec, SngReplay **out);
/* `days` days of a trajectory -- obs [days][T + 1][num_envs][obs_dim], actions [days][T][num_envs][act_dim], reward f64
 * and done u8 [days][T][num_envs], device pointers -- into the ring: one launch (replay_push_kernel). */
int sng_replay_push(SngReplay *ring, int32_t days, const float *obs, const float *actions, const double *reward,
                    const uint8_t *done, void *stream);
/* filled * T * num_envs: the transitions a sample draws from (with NULL: 0) */
int64_t sng_replay_size(const SngReplay *ring);
/* The slot the next pushed day goes to, and the slots that hold a day. */
int sng_replay_state(const SngReplay *ring, int32_t *head, int32_t *filled);
/* One launch (replay_sample_kernel) with the handle's counter, which is then bumped. */
int sng_replay_sample(SngReplay *ring, int64_t batch, const SngReplayBatch *out, void *stream);
int sng_replay_get_counter(const SngReplay *ring, uint64_t *out);
int sng_replay_set_counter(SngReplay *ring, uint64_t counter);
void sng_replay_destroy(SngReplay *ring);
/* Host only: the `batch` indices a sample with this seed, env offset and counter draws from n transitions. */
int sng_replay_host_indices(uint64_t seed, int64_t env_offset, uint64_t counter, uint64_t n, int64_t batch,
                            int64_t *out);

typedef struct SngCriticSpec {
    int32_t hidden1, hidden2;      /* each 8 .. 512, any integer */
    int32_t activation;            /* hidden layers: 0 tanh, 1 relu */
} SngCriticSpec;
typedef struct SngCritic SngCritic;
/* A critic for `env` (its obs_dim and act_dim); the weights are zero until sng_critic_set_weights. */
int sng_critic_create(SngEnv *env, const SngCriticSpec *spec, SngCritic **out);
/* Upload into the critic's device image, asynchronously on `stream`: new weights between two calls change the next. */
int sng_critic_set_weights(SngCritic *critic, const SngMlpWeights *weights, void *stream);
/* obs [rows][obs_dim], actions [rows][act_dim] -> out [rows]: one launch (q_net_kernel). */
int sng_critic_q(SngCritic *critic, int64_t rows, const float *obs, const float *actions, float *out, void *stream);
/* The TD targets of `rows` transitions: two launches, the target actor (policy_net_kernel) over next_obs into
 * next_actions [rows][act_dim], which is written, then q_net_kernel with the target stage over (next_obs, next_actions)
 * and reward / done [rows] f32 into y [rows].  actor_target is a policy made by sng_policy_create_net for the same env. */
int sng_critic_targets(SngCritic *q_target, SngPolicy *actor_target, int64_t rows, const float *next_obs,
                       const float *reward, const float *done, double gamma, float *next_actions, float *y,
                       void *stream);
void sng_critic_destroy(SngCritic *critic);
/* Host only: the same contracts on host arrays.  Validate as the device calls do.  next_actions_given != 0:
 * next_actions is read, not computed (actor_spec and actor_weights may then be NULL). */
int sng_critic_host_q(int32_t obs_dim, int32_t act_dim, const SngCriticSpec *spec, const SngMlpWeights *weights,
                      int64_t rows, const float *obs, const float *actions, float *out);
int sng_critic_host_targets(int32_t obs_dim, int32_t act_dim, const SngCriticSpec *spec, const SngMlpWeights *weights,
                            const SngMlpNetSpec *actor_spec, const SngMlpWeights *actor_weights, int64_t rows,
                            const float *next_obs, const float *reward, const float *done, double gamma,
                            float *next_actions, int next_actions_given, float *y);
/* sng_policy_actions over `rows` rows instead of the env's num_envs: one policy_net_kernel launch.  A policy not made
 * by sng_policy_create_net is refused (SNG_ERR_UNSUPPORTED). */
int sng_policy_actions_rows(SngPolicy *policy, int64_t rows, const float *obs, const float *noise, float *actions,
                            float *env_actions, void *stream);

/* ---------------------------------------------------------------------------------------------
 * DDPG's gradient step: one SB3 TD3.train iteration as DDPG runs it (one critic, policy_delay = 1, no target noise)
 * on the device -- both nets' forward and backward passes, Adam, the polyak update of both targets and the repacking
 * of the four handles' device images -- as plain launches on one stream, with no synchronisation and no host weight
 * traffic.  The host model is csrc/sng_ddpg_learn_host.h, whose header comment lists every expression; the device
 * (csrc/sng_ddpg_learn.h, on the f32-input MFMA) gives the same values (==, the sign of a zero apart) given the
 * device's own a_pi = tanhf(mean), which the host model takes as an input.
 *
 * The learner owns, as plain row-major float32 device arrays in torch's [out][in] layout: the master weights of the
 * actor, the critic and their targets (taken from host arrays by sng_learner_set_state), Adam's two moments and the
 * last update's gradients of actor and critic, and the last update's q, dq, a_pi, q_pi [rows] and two losses.
 *
 * sng_learner_update(rows, obs, actions, y):
 *   1. critic: q = Q(s, a); loss = mean((q - y)^2), dq[b] = (2 (q[b] - y[b])) / (float)rows; backward; Adam on the
 *      critic's masters; polyak of the target critic; both critics' images repacked.
 *   2. actor, on the critic as updated: a_pi = tanhf(mean(s)); q_pi = Q(s, a_pi); loss = -mean(q_pi), dq_pi[b] =
 *      -(1 / (float)rows); backward through the critic's data path to the action columns of its input, through
 *      1 - a_pi^2, and through the actor; Adam on the actor's masters; polyak of the target actor; both actors' images
 *      repacked.  The next launch of a graph captured with the actor acts with the new weights.
 * Forward outputs are the k-ordered fmaf chains from the bias of SngMlpNetSpec; a data gradient dIn[b][i] is the fmaf
 * chain over the layer's outputs j ascending of dOut[b][j] * W[j][i], from 0, masked by the relu (In[b][i] > 0); a
 * weight gradient dW[j][i] is the fmaf chain over the rows b ascending of dOut[b][j] * In[b][i], from 0, and db[j] the
 * same ordered sum of dOut[b][j].  Segment law: the rows are cut into segments of SNG_LEARNER_SEGMENT; each segment is
 * a chain of its own from 0 and the partials are added in ascending segment order (g = p0; g = g + p1; ...); rows <=
 * SNG_LEARNER_SEGMENT is one chain.  No float atomics anywhere: nothing depends on scheduling.
 *
 * Adam (torch.optim.Adam, no weight decay, no amsgrad) on an element, each float32 operation rounded on its own, the
 * divisions and the square root correctly rounded.  t = 1, 2, .. is a host integer of the handle; with the doubles of
 * the spec
 *     step_size = (float)(lr / (1 - beta1^t)),  bc2_sqrt = (float)sqrt(1 - beta2^t)
 *     m = (float)beta1 * m + (float)(1 - beta1) * g
 *     v = (float)beta2 * v + ((float)(1 - beta2) * g) * g
 *     p = p - step_size * (m / (sqrt(v) / bc2_sqrt + (float)eps))
 * Polyak: target = (float)(1 - tau) * target + (float)tau * p, on the p just updated.  Losses: the row-ordered float32
 * sums (s = s + d * d; s = s + q_pi; segments as for the weight gradients) divided by (float)rows, the actor's negated.
 *
 * Refusals, the reason in sng_last_error: hidden activations other than relu and an actor that is not
 * sng_policy_create_net's with SNG_MLP_OUT_SQUASH are SNG_ERR_UNSUPPORTED; nets whose widths or activations differ
 * from their targets', handles of another env, rows < 1 or rows > SNG_LEARNER_MAX_ROWS, non-finite hyper-parameters,
 * tau outside [0, 1], lr <= 0, betas outside [0, 1), eps < 0 and NULL pointers are SNG_ERR_INVALID_ARGUMENT.  The four
 * handles must outlive the learner.  The workspace grows (the old block freed and a new one allocated, which
 * synchronises) only when an update has more rows than every update before it; the pointers sng_learner_last gave
 * before are then invalid, and if that allocation fails sng_learner_last refuses (SNG_ERR_STATE) until an update
 * succeeds.  Losses: the sums follow the segment law too.  While a learner lives, its masters are the weights:
 * sng_policy_set_weights / sng_critic_set_weights on one of its four handles changes that handle's image only until
 * the next update overwrites it (load the learner with sng_learner_set_state instead).  An update that fails at a
 * launch (SNG_ERR_HIP) returns at once: launches before it are queued, the critic may have been stepped without the
 * actor, and the step count is not advanced; restore a known state with sng_learner_set_state. */
#define SNG_LEARNER_SEGMENT 1024     /* rows of one chain of a weight gradient */
#define SNG_LEARNER_MAX_ROWS 65536
typedef struct SngLearnerSpec {
    double actor_lr, critic_lr;     /* > 0 */
    double tau;                     /* [0, 1] */
    double beta1, beta2, eps;       /* Adam's */
} SngLearnerSpec;
typedef struct SngNetArrays {       /* a net's six arrays: w1 [h1][in], b1, w2 [h2][h1], b2, w3 [out][h2], b3 */
    float *w1, *b1, *w2, *b2, *w3, *b3;
} SngNetArrays;
enum {                              /* sng_learner_arrays' `which` */
    SNG_LEARNER_ACTOR = 0, SNG_LEARNER_CRITIC = 1, SNG_LEARNER_ACTOR_TARGET = 2, SNG_LEARNER_CRITIC_TARGET = 3,
    SNG_LEARNER_ACTOR_M = 4, SNG_LEARNER_ACTOR_V = 5, SNG_LEARNER_CRITIC_M = 6, SNG_LEARNER_CRITIC_V = 7,
    SNG_LEARNER_ACTOR_GRAD = 8, SNG_LEARNER_CRITIC_GRAD = 9, SNG_LEARNER_ARRAYS = 10
};
typedef struct SngLearnerState {    /* host arrays: the masters, the targets, Adam's moments and the step count */
    SngNetArrays actor, critic, actor_target, critic_target;
    SngNetArrays actor_m, actor_v, critic_m, critic_v;
    int64_t step;
} SngLearnerState;
typedef struct SngLearnerLast {     /* the last update's outputs: device pointers (sng_learner_last) */
    int64_t rows;
    float *q, *dq, *a_pi, *q_pi;    /* [rows], [rows], [rows][act_dim], [rows] */
    float *critic_loss, *actor_loss;    /* one float each */
} SngLearnerLast;
typedef struct SngLearnerTrace {    /* sng_learner_host_update's outputs: host arrays, each may be NULL */
    float *q, *dq, *q_pi;           /* [rows] */
    SngNetArrays critic_grad, actor_grad;
    float *critic_loss, *actor_loss;
} SngLearnerTrace;
typedef struct SngLearner SngLearner;
/* A learner over four handles of `env`; the masters, targets and moments are zero and the step count 0 until
 * sng_learner_set_state. */
int sng_learner_create(SngEnv *env, SngPolicy *actor, SngPolicy *actor_target, SngCritic *critic,
                       SngCritic *critic_target, const SngLearnerSpec *spec, SngLearner **out);
/* One update on obs [rows][obs_dim], actions [rows][act_dim] and y [rows] (device pointers), asynchronous on `stream`. */
int sng_learner_update(SngLearner *learner, int64_t rows, const float *obs, const float *actions, const float *y,
                       void *stream);
/* The device arrays of one of the ten nets' worth of arrays above; they live as long as the learner. */
int sng_learner_arrays(SngLearner *learner, int which, SngNetArrays *out);
/* The last update's outputs; the pointers change when the workspace grows. */
int sng_learner_last(SngLearner *learner, SngLearnerLast *out);
int sng_learner_get_step(const SngLearner *learner, int64_t *out);
/* Masters, targets, moments and the step count from / to host arrays.  set_state also repacks the four handles' device
 * images from the new masters.  Both synchronise `stream`. */
int sng_learner_set_state(SngLearner *learner, const SngLearnerState *state, void *stream);
int sng_learner_get_state(SngLearner *learner, const SngLearnerState *state_out, int64_t *step_out, void *stream);
void sng_learner_destroy(SngLearner *learner);
/* Host only: the host model of one update on host arrays; `state` is updated in place, a_pi [rows][act_dim] is read
 * (the device's, or any stand-in for tanh(mean)).  Validates as the device calls do. */
int sng_learner_host_update(const SngMlpNetSpec *actor_spec, const SngCriticSpec *critic_spec,
                            const SngLearnerSpec *spec, SngLearnerState *state, int64_t rows, const float *obs,
                            const float *actions, const float *y, const float *a_pi, const SngLearnerTrace *trace);

/* Host-only entry points (no GPU needed): the reference-RNG scenario generator, for
 * checking against numpy/Python streams on CPU.  Outputs in SngScenario layout for
 * `num_envs` envs seeded seed+i; `episode` = number of days already drawn. */
int sng_host_generate_scenarios(const SngConfig *cfg, int64_t num_envs, uint64_t seed, int32_t episodes,
                                double *soc, double *occupancy, double *capacity, double *requested_soc,
                                int32_t *arrivals, int32_t *departures, int32_t max_vehicles,
                                double *pv_ratio);

/* Host threads the reference-RNG generator and the scenario encoder use (see sng_reset). */
int32_t sng_host_threads(void);

/* The device day counter: the number of device-RNG days this handle has started (the next device
 * reset draws day *out).  Synchronises `stream`. */
int sng_get_day_counter(SngEnv *env, uint64_t *out, void *stream);

/* Diagnostics: the measured bandwidth ceiling of device `device` for a step-sized launch.  One float4
 * copy kernel reads read_bytes and writes write_bytes (nontemporal stores, the step kernel's policy) per
 * dispatch; *dispatch_us = mean device time of `reps` dispatches each between its own start/stop events,
 * *back_to_back_us = mean start-to-start time of `reps` dispatches queued back to back (as a graph runs
 * them).  Allocates and frees its buffers; synchronises `stream`.  No reference counterpart. */
int sng_bandwidth_probe(int device, int64_t read_bytes, int64_t write_bytes, int32_t reps, float *dispatch_us,
                        float *back_to_back_us, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU exchange: one process per GPU, each with its contiguous env shard
 * (sng_set_env_offset); once per simulated day the per-env returns are all-gathered over RCCL
 * (xGMI within a node).  No per-step communication.  RCCL is loaded at the first call
 * (dlopen librccl.so.1).  Rank 0 makes the id with sng_comm_unique_id and hands it to every rank
 * (file, socket, MPI ...); each rank then calls sng_comm_create with it. */
#define SNG_COMM_ID_BYTES 128
typedef struct SngComm SngComm;
int sng_comm_unique_id(uint8_t *id /* [SNG_COMM_ID_BYTES] */);
int sng_comm_create(int device, int nranks, int rank, const uint8_t *id, SngComm **out);
/* local: device [count] f64 of this rank; global: device [nranks * count] f64, rank-major (= global
 * env order for equal contiguous shards).  Asynchronous on `stream`. */
int sng_allgather_returns(SngComm *comm, const double *local, double *global, int64_t count, void *stream);
void sng_comm_destroy(SngComm *comm);
const char *sng_comm_last_error(const SngComm *comm);   /* NULL: the calling thread's last create error */

#ifdef __cplusplus
}
#endif

#endif /* SNG_H */
