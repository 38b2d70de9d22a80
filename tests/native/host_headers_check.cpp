// The library's host-only headers, included with nothing but include/ and csrc/ on the include path and no
// ROCm: tests/test_host_day_cpu.py compiles this file with g++ -std=c++17 -Wall -Werror -fsyntax-only, which
// fails as soon as one of them reaches for hip/hip_runtime.h.
#include "sng_graph_form.h"
#include "sng_host_day.h"
#include "sng_host_pool.h"
#include "sng_host_tables.h"
#include "sng_noise_host.h"
#include "sng_policy_host.h"
#include "sng_policy_net_host.h"
#include "sng_ppo_host.h"
#include "sng_ppo_net_host.h"
#include "sng_state_format.h"
#include "sng_step_plan.h"

int main() { return 0; }
