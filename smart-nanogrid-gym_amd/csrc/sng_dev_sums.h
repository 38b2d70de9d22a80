// sng_dev_sums.h -- numpy's pairwise sum, the order the reference adds the charging powers in
// (charging_station.py:293-294): fed one element at a time (PairwiseSum) or over a compacted row in LDS
// (pairwise_row, pairwise_row_c).  Needs nothing but the HIP runtime header.
#pragma once

namespace sng {

// ---------------------------------------------------------------------------------
// numpy pairwise_sum (loops_utils.h.src) for n <= 128, fed one element at a time in
// array order (used for N > 16; smaller N use the LDS-compacted form below).
// ---------------------------------------------------------------------------------
struct PairwiseSum {
    double r[8];
    double b[8];
    int n;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            r[q] = 0.0;
            b[q] = 0.0;
        }
        n = 0;
    }
    __device__ __forceinline__ void push(double x) {
        const int j = n & 7;
#pragma unroll
        for (int q = 0; q < 8; ++q) b[q] = (q == j) ? x : b[q];
        ++n;
        if ((n & 7) == 0) {
            const bool first = (n == 8);
#pragma unroll
            for (int q = 0; q < 8; ++q) r[q] = first ? b[q] : r[q] + b[q];
        }
    }
    __device__ __forceinline__ double result() const {
        const int tail = n & 7;
        double res = (n < 8) ? 0.0 : ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < tail) res += b[q];
        return res;
    }
};

// The same sum over a compacted array the lane has written to its own LDS row:
// n < 8 is the sequential sum `seq` the caller kept on the fly (adding the skipped +0.0
// terms is exact); otherwise 8 accumulators over full blocks, pairwise tree, sequential tail.
__device__ __forceinline__ double pairwise_row(const double *row, int n, double seq) {
    if (n < 8) return seq;
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = row[j];
    const int full = n - (n & 7);
    for (int i = 8; i < full; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += row[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = full; i < n; ++i) res += row[i];
    return res;
}

// The same for a row of at most NC <= 16 entries: every slot is read in one batch of LDS reads
// (slots at or past n hold stale values and are selected away), so the sequential tail costs
// no LDS round trip per element.
template <int NC>
__device__ __forceinline__ double pairwise_row_c(const double *row, int n, double seq) {
    static_assert(NC >= 1 && NC <= 16, "one 8-block plus tail, or two full blocks at 16");
    if constexpr (NC < 8) {
        return seq;
    } else {
        if (n < 8) return seq;
        double r[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) r[j] = row[j];
        if (NC == 16 && n == 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += r[(j + 8) % NC];
            return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        }
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = 8; i < NC; ++i) res = (i < n) ? res + r[i] : res;
        return res;
    }
}

}  // namespace sng
