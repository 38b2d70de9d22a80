// sng_ppo_net_host.h -- the PPO head with a value net of any two hidden widths, in host form (include/sng.h,
// sng_ppo_create_net): the validation of an SngPpoNetSpec, the head's device image and the contract's arithmetic on
// the CPU.  Nothing is computed here that another header does not state already: the value path is mlp_net_host
// (sng_policy_net_host.h) on a NetImage packed by net_pack for (obs_dim, 1, hidden1, hidden2), the advantages are
// ppo_gae_host and the log-probabilities ppo_logp_host (sng_ppo_host.h), which read log_std / inv_std through the
// GaussHead laid out behind the NetImage.  value_net_kernel and gae_scan_kernel (sng_ppo_net.h) reproduce
// it by value with relu and up to the device's tanhf with tanh.  Host only, no HIP: it compiles with plain g++
// (tests/native/ppo_net_host_check.cpp runs it against naive loops); build with -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "sng.h"
#include "sng_policy_net_host.h"
#include "sng_ppo_host.h"

namespace sng {

// The device image, in floats: the value net's NetImage (A = 1, the mean output, no bounds), then the Gaussian head
// (sng_ppo_host.h, GaussHead), as in a PpoImage.
struct PpoNetImage {
    NetImage v;
    GaussHead head;
    size_t floats = 0;
};

// gae_scan_kernel stages 64 noise rows of (act_dim | 1) floats in at most 64 KB of LDS
constexpr int kPpoNetMaxAct = 255;

inline SngMlpNetSpec ppo_net_value_spec(int O, const SngPpoNetSpec &s) {
    return SngMlpNetSpec{O, 1, s.hidden1, s.hidden2, s.activation, SNG_MLP_OUT_MEAN, nullptr, nullptr};
}

inline PpoNetImage ppo_net_image(int O, int A, const SngPpoNetSpec &s) {
    PpoNetImage m;
    m.v = net_image(O, 1, s.hidden1, s.hidden2, s.activation, SNG_MLP_OUT_MEAN, false);
    m.head = gauss_head(A, m.v.floats, &m.floats);
    return m;
}

// SNG_OK, or the status sng_ppo_create_net and sng_ppo_net_host_finish return with `why`: ppo_dims_check's refusals,
// then net_spec_check's for the value net (act_dim = 1): widths outside 8 .. 512 and LDS tiles that do not fit a
// compute unit are SNG_ERR_UNSUPPORTED with the sizes in the message.
inline int ppo_net_spec_check(const SngPpoNetSpec *s, int O, int A, std::string *why) {
    if (!s) {
        if (why) *why = "null ppo net spec";
        return SNG_ERR_INVALID_ARGUMENT;
    }
    if (int rc = ppo_dims_check(O, A, s->activation, why)) return rc;
    if (A > kPpoNetMaxAct) {   // far above any station's (129 at 128 chargers with a battery)
        if (why) *why = "ppo act_dim " + std::to_string(A) + " is above " + std::to_string(kPpoNetMaxAct) +
                        ", the widest noise tile of gae_scan_kernel";
        return SNG_ERR_UNSUPPORTED;
    }
    const SngMlpNetSpec v = ppo_net_value_spec(O, *s);
    if (int rc = net_spec_check(&v, 0, 0, why)) {
        if (why) *why = "ppo value net: " + *why;
        return rc;
    }
    return SNG_OK;
}

// The value net's weights as mlp_weights_check refuses them, and log_std.
inline int ppo_net_weights_check(int O, int A, const SngPpoNetSpec &s, const SngMlpWeights *w, const float *log_std,
                                 std::string *why) {
    if (int rc = mlp_weights_check(O, s.hidden1, s.hidden2, 1, "value net", w, why)) return rc;
    return ppo_log_std_check(A, log_std, why);
}

// The image of a head without a value net (zero weights): for a caller that brings its own values.
inline void ppo_net_pack_log_std(const PpoNetImage &m, const float *log_std, float *img) {
    ppo_pack_log_std(m.head, m.floats, log_std, img);   // zeros the whole image first
}

// The value net and log_std (null: zeros) into `img` (PpoNetImage::floats floats).
inline void ppo_net_pack(const PpoNetImage &m, const SngPpoNetSpec &s, const SngMlpWeights &w, const float *log_std,
                         float *img) {
    ppo_net_pack_log_std(m, log_std, img);
    net_pack(m.v, ppo_net_value_spec(m.v.O, s), w, img);   // rewrites the NetImage's floats only
}

// obs [days][T + 1][E][O] -> values [days][T + 1][E]: mlp_net_host with one action, no noise and no clip, over the
// days * (T + 1) * E rows as one flat batch
inline void ppo_net_values_host(const PpoNetImage &m, const float *img, int32_t days, int32_t T, int64_t E,
                                const float *obs, float *values) {
    mlp_net_host(m.v, img, (int64_t)days * (int64_t)(T + 1) * E, obs, nullptr, values, nullptr);
}

// The rows of the device's value launch and its workgroups of kNetRows rows; a grid's x dimension holds 2^31 - 1.
constexpr int64_t kPpoNetMaxBlocks = 2147483647;
inline int64_t ppo_net_rows(int32_t days, int32_t T, int64_t E) { return (int64_t)days * (int64_t)(T + 1) * E; }
inline int64_t ppo_net_blocks(int64_t rows) { return (rows + kNetRows - 1) / kNetRows; }

}  // namespace sng
