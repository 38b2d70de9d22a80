# The library's sources and its build id, shared by csrc/Makefile and tools/diag/Makefile (tools/diag/variant.sh
# copies csrc/ whole, so this fragment travels with a variant's sources).
SNG_SRCS := sng_kernels.hip sng_api.cpp sng_state.cpp sng_graph.cpp sng_policy.cpp sng_ppo.cpp sng_noise.cpp sng_ddpg.cpp sng_ddpg_learn.cpp sng_comm.cpp
# every header of the directory this fragment lies in, sorted: a new header is in the build id and in make's
# dependencies without being listed anywhere
SNG_HDRS := $(sort $(notdir $(wildcard $(dir $(lastword $(MAKEFILE_LIST)))*.h)))
# $(call sng_build_id,<csrc directory>,<compile flags>): the first 12 hex digits of the SHA-256 of every source
# of the library, the compile flags and the compiler's version line (the same sources built with
# other flags or another ROCm are another binary).  The committed measurements under profiles/ are keyed by
# it (bench.py looks them up by the loaded library's id).
sng_build_id = $(shell (cd $(1) && cat $(SNG_SRCS) $(SNG_HDRS) $(ROOT)/include/sng.h; echo '$(2)'; \
                        $(HIPCC) --version 2>/dev/null | head -1) | sha256sum | cut -c1-12)
