// sng_launch.h -- what the host translation units (through sng_env.h) call in sng_kernels.hip: the launch
// wrappers; the kernels they launch live in the headers that file includes.  They all include it, so a changed
// signature is a compile error in one of them; default arguments live here only.  Launches only: what a plan's
// graph looks like is answered by sng_graph_form.h, before anything is launched.
#pragma once
#include <hip/hip_runtime.h>

#include "sng_ddpg_host.h"
#include "sng_ddpg_learn_host.h"
#include "sng_graph_form.h"
#include "sng_layout.h"
#include "sng_noise_host.h"
#include "sng_policy_host.h"
#include "sng_policy_net_host.h"
#include "sng_ppo_host.h"
#include "sng_ppo_net_host.h"

namespace sng {

// a pointer a kernel may read or write 16 bytes a lane through
inline bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15u) == 0; }

// ev_start / ev_stop (both or neither): stamped with the dispatch's own begin / end, the kernel's device time
hipError_t launch_step(const Params &p, const DeviceState &s, const InfoPtrs &info, const Tables &tab,
                       const float *act, float *obs, double *reward, uint8_t *done, int64_t E, int t, int vec_io,
                       hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// Steps t0 .. t0 + nt - 1 of the loaded day in one launch (sng_step_day.h) of the day kernel `node` names, which
// graph_form decided (DAY_KERNEL_LEAN, DAY_KERNEL_WIDE or DAY_KERNEL_STATION); `act` is step t0's block of nt
// consecutive [E][act_dim] blocks.  hipErrorNotSupported for any other node and for a node that is not the plan's
// (day_kernel_of; the station kernel: day_station_fixed).
// obs_step / out_step: floats from one step's observation block to the next and elements from one step's reward
// and done block to the next, when every step's outputs are kept (`trajectory`, which only the lean day kernel
// can do: sng_step_plan.h day_kernel_of); 0: every step overwrites the same blocks.
hipError_t launch_day(DayNode node, const Params &p, const DeviceState &s, const InfoPtrs &info, const float *act,
                      float *obs, double *reward, uint8_t *done, int64_t E, int t0, int nt, int vec_io, hipStream_t stream,
                      int64_t obs_step = 0, int64_t out_step = 0);
hipError_t launch_observe0(const Params &p, const DeviceState &s, float *obs, double *ep_return, int64_t E,
                           int vec_io, hipStream_t stream, int mode, int64_t replay, const RefStreams *ps = nullptr,
                           int py = 0);
hipError_t launch_generate(const Params &p, const DeviceState &s, uint64_t seed, int64_t E, int i4, int i10, int i1,
                           float *obs, double *ep_return, int vec_io, hipStream_t stream,
                           hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, int day_delta = 0,
                           size_t min_lds = 0);
hipError_t launch_profiles(const Params &p, const DeviceState &s, int64_t E, hipStream_t stream);
hipError_t launch_bump_day(const DeviceState &s, hipStream_t stream, uint64_t amount = 1);
hipError_t launch_probe_copy(const void *in, void *out, int64_t nr, int64_t nw, hipStream_t stream, hipEvent_t a,
                             hipEvent_t b);
hipError_t launch_ref_seed(const RefStreams &rs, uint64_t seed0, int64_t E, hipStream_t stream);
hipError_t launch_mt_prepare(const RefStreams &rs, int64_t E, hipStream_t stream);
hipError_t launch_ref_day(const Params &p, const DeviceState &s, const RefStreams &rs, int64_t E, int i4, int i10,
                          int i1, bool prepare, hipStream_t stream);
// The MLP actor over E rows (sng_policy.h, policy_kernel): img is the device image `m` describes; noise and
// env_actions may be null.
hipError_t launch_policy(const float *img, const PolicyImage &m, const float *obs, const float *noise, float *actions,
                         float *env_actions, int64_t E, hipStream_t stream);
// The MLP actor of any width over E rows (sng_policy_net.h, policy_net_kernel): img is the device image `m` describes;
// noise and env_actions may be null.
hipError_t launch_policy_net(const float *img, const NetImage &m, const float *obs, const float *noise, float *actions,
                             float *env_actions, int64_t E, hipStream_t stream);
// The policy kernels' dynamic-LDS limit, raised once (stations above 45 chargers need more than 64 KB); called by
// sng_policy_create so that no capture is the first to ask.
hipError_t policy_kernels_init();
// A whole day with the actor between the steps in one launch (sng_policy.h, day_lean_policy_kernel), where graph_form
// decided DAY_POLICY_FUSED (hipErrorInvalidDeviceFunction for a plan without that kernel).  noise: T blocks or null;
// obs0: the day's t = 0 observation block; obs, reward, done: step 0's blocks, obs_step / out_step as launch_day's;
// actions_out: step 0's block of a, act_step floats to the next step's (0: one block).
hipError_t launch_policy_day(const Params &p, const DeviceState &s, const InfoPtrs &info, const float *img,
                             const PolicyImage &m, const float *noise, const float *obs0, float *obs,
                             float *actions_out, double *reward, uint8_t *done, int64_t E, int vec_io,
                             hipStream_t stream, int64_t obs_step, int64_t out_step, int64_t act_step);
// What finishes a PPO rollout (sng_ppo.h, rollout_gae_kernel): values, advantages, returns and, with noise and logp
// both given, log-probabilities of `r`'s days of T steps of E envs; img is the device image `m` describes.
hipError_t launch_rollout_gae(const float *img, const PpoImage &m, const SngPpoRollout &r, int64_t E, int T,
                              hipStream_t stream);
// rollout_gae_kernel's dynamic-LDS limit, raised once; called by sng_ppo_create so that no capture is the first to ask.
hipError_t ppo_kernels_init();
// A net head's finish (sng_ppo_net.h): value_net_kernel over the days * (T + 1) * E observation rows, then
// gae_scan_kernel; img is the device image `m` describes.  hipErrorInvalidValue for what sng_ppo_finish refuses.
hipError_t launch_ppo_net(const float *img, const PpoNetImage &m, const SngPpoRollout &r, int64_t E, int T,
                          hipStream_t stream);
// value_net_kernel's dynamic-LDS limit, raised once; called by sng_ppo_create_net so that no capture is the first to ask.
hipError_t ppo_net_kernels_init();
// A noise source's fill (sng_noise.h, action_noise_kernel) of `days` blocks [T][E][act_dim] into out, from the counter's
// value on, and the one-thread kernel that adds `days` to the counter behind it; params is the device image
// noise_pack_params fills.
hipError_t launch_noise_fill(const SngNoiseSpec &spec, const float *params, uint64_t *counter, int64_t env_offset,
                             float *out, int32_t days, int T, int64_t E, hipStream_t stream);
// A replay ring's push (sng_ddpg.h, replay_push_kernel): the segments replay_push_args lists, in one launch.
hipError_t launch_replay_push(const PushArgs &a, hipStream_t stream);
// A ring's sample (replay_sample_kernel): `batch` rows of the n transitions of days of T steps of E envs, with the
// sample's key (replay_sample_key).
hipError_t launch_replay_sample(const ReplayStorage &ring, const SngReplayBatch &out, uint32_t key, uint64_t n, int T,
                                int64_t E, int O, int A, int64_t batch, hipStream_t stream);
// Q over `rows` rows (q_net_kernel): img is the critic's device image `m` describes (m.O = O + the action width); with
// reward and done the TD targets with g = (float)gamma instead.  hipErrorInvalidValue for what critic_spec_check and the
// entry points refuse.
hipError_t launch_q_net(const float *img, const NetImage &m, int O, const float *obs, const float *actions,
                        const float *reward, const float *done, float g, float *out, int64_t rows, hipStream_t stream);
// q_net_kernel's dynamic-LDS limit, raised once; called by sng_critic_create so that no capture is the first to ask.
hipError_t critic_kernels_init();
// A learner's launches (sng_ddpg_learn.h; the structs are sng_ddpg_learn_host.h's): x = [obs | actions]; one matrix
// product with its epilogue (a LearnEpilogue); a loss and its gradient over the rows; a net's Adam step, polyak blend
// and repack, or with adam = false the repack alone.  hipErrorInvalidValue for what sng_learner_update refuses.
hipError_t launch_learn_concat(const float *obs, const float *actions, float *x, int64_t rows, int O, int A,
                               hipStream_t stream);
hipError_t launch_learn_gemm(const LearnGemm &g, int epilogue, hipStream_t stream);
hipError_t launch_learn_loss(bool actor, const float *q, const float *y, float *dq, float *loss, int64_t rows,
                             hipStream_t stream);
hipError_t launch_learn_step(const LearnStep &s, bool adam, hipStream_t stream);

}  // namespace sng
