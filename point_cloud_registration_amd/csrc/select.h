// An exact order statistic of float64 keys on the device (select.hip; include/pcr.h: "adaptive pass", pcr_order_statistic):
// the k-th smallest key among those < +inf, the number of keys <= it, and -- for the adaptive pass of match_pass.h -- the
// robust scale taken from it.  A most-significant-digit radix select over the ordered 64-bit pattern of a key: 8 digits of 8
// bits, per digit one histogram launch (LDS integer atomics per block, integer adds into the state's histogram of that digit:
// exact in any order) and one launch of one block that picks the digit and narrows the prefix.  No float atomics, nothing that
// depends on the grid, nothing that waits on the host.
#pragma once

#include <stdint.h>

#include "pcr_internal.h"

#define PCR_SELECT_DIGITS 8
#define PCR_SELECT_BINS 256
// the histogram grid: ceil(n / 256) blocks of 256 lanes, at most this many -- a lane's second key lies one stride of
// PCR_SELECT_MAX_BLOCKS * 256 = 262144 keys behind its first
#define PCR_SELECT_MAX_BLOCKS 1024

// The device state block of one selection: zeroed (hipMemsetAsync) before the first launch
struct SelectState {
    unsigned long long hist[PCR_SELECT_DIGITS][PCR_SELECT_BINS];   // one histogram per digit: no re-zeroing between the rounds
    unsigned long long prefix;     // the digits chosen so far, at their place in the ordered pattern
    unsigned long long rank;       // 1-based rank of the wanted key among the keys that share the prefix
    unsigned long long below;      // keys ordered before every key that shares the prefix
    unsigned long long m;          // keys < +inf
    unsigned long long k;          // the rank asked for: given, or max(1, floor(quantile * m))
    unsigned long long n_le;       // keys <= tau
    double tau;                    // the k-th smallest key; +inf for m = 0
    double c, c2;                  // factor * sqrt(tau) and c * c, taken once, by the last launch; 0 under PCR_ROBUST_TRIM
    // What the reduce behind the selection reads (match_pass.h: AdaptiveSide) -- the variants of the adaptive pass as
    // data, so that the reduce takes them as it takes a caller's RobustK:
    //   an M-estimator            w = (kind, c, c2)
    //   ... whose c2 is not > 0   w = (HUBER, 0, 0): s <= 0 ? 1 : 0 / sqrt(s), the limit of every kernel for c -> 0
    //   PCR_ROBUST_TRIM           w = (HUBER, 0, +inf): s <= +inf, weight exactly 1 (over what pcr_select_drop_launch left)
    double w_c, w_c2;
    int w_kind;
    int kind;                      // PCR_ROBUST_HUBER .. PCR_ROBUST_TRIM, as asked for
};

// The selection over n >= 1 keys on the device, queued on the context's stream behind whatever wrote the keys.
//   k_fixed >= 1: the rank;  k_fixed == 0: k = max(1, floor(quantile * m)), the product taken once in float64 on the device
//   kind, factor: c = kind == PCR_ROBUST_TRIM ? 0 : factor * sqrt(tau)
//   stats_or_null: 5 doubles on the device, (tau, c, n_le, k, m) -- (+inf, 0, 0, 0, 0) for m = 0
pcr_status pcr_select_launch(pcr_context *ctx, const double *keys, int64_t n, double quantile, int64_t k_fixed, int kind, double factor,
                             SelectState *st, double *stats_or_null);
// behind it: idx[i] = none wherever not (keys[i] <= tau) -- the entries of a match list that a trim drops; the compare reads the
// STORED key, so exactly n_le entries with a key stay
pcr_status pcr_select_drop_launch(pcr_context *ctx, const double *keys, int64_t n, const SelectState *st, uint32_t *idx, uint32_t none);
