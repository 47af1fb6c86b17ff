// The host's half of the expected hexamer counts of the sequence-bias correction (DESIGN.md section 4,
// "Sequence bias"): the abundances as 96-bit fixed-point weights.  Plain C++, no GPU: skm_bias_correct and
// skm_bias_correct_many (skm_abi_index.hip) and skm_bias_fixed_weights (libseekmer_host.so) all call this one function.
#pragma once
#include <cmath>
#include <cstdint>

namespace skm {

constexpr double BIAS_FIXED_ONE = 0x1p94;

// total = sum_t tpm_t n_t, added in transcript order.  False when the total is not finite or 2^94 / total is not:
// the abundances cannot be scaled.  The caller has checked that every tpm_t is finite and not negative and every
// n_t is not negative.
inline bool bias_fixed_total(const double *tpm, const int32_t *windows, int64_t n_tx, double *total_out)
{
    double total = 0.0;
    for (int64_t t = 0; t < n_tx; ++t) total += tpm[t] * (double)windows[t];
    *total_out = total;
    return total == 0.0 || !(std::isinf(total) || std::isinf(BIAS_FIXED_ONE / total));
}

// W_t = round(tpm_t * 2^94 / total) < 2^95 for a total that bias_fixed_total accepted, cut into three 32-bit limbs,
// lowest first: limbs[k * n_tx + t] (a limb's sum over 2^31 windows stays below 2^63: no carries on the device).  A
// transcript without windows gets limbs 0 (its weight is never added, whatever it is), and so does every
// transcript when the total is 0.
inline void bias_fixed_limbs(const double *tpm, const int32_t *windows, int64_t n_tx, double total, unsigned long long *limbs)
{
    for (int64_t i = 0; i < 3 * n_tx; ++i) limbs[i] = 0;
    if (!(total > 0.0)) return;
    for (int64_t t = 0; t < n_tx; ++t) {
        if (windows[t] == 0) continue;
        const double w = tpm[t] * (BIAS_FIXED_ONE / total);           // (a double at or above 2^52 is a whole number)
        // clamped as a double, before the conversion: one transcript may hold everything with the scale rounded up
        const unsigned __int128 fixed = w >= 0x1p95 ? ((unsigned __int128)1 << 95) - 1
                                                    : (unsigned __int128)(w < 0x1p52 ? w + 0.5 : w);
        for (int k = 0; k < 3; ++k) limbs[k * n_tx + t] = (unsigned long long)(fixed >> (32 * k)) & 0xffffffffULL;
    }
}

// both: false, with nothing but *total_out written, for a total that cannot be scaled
inline bool bias_fixed_weights(const double *tpm, const int32_t *windows, int64_t n_tx, unsigned long long *limbs,
                               double *total_out)
{
    if (!bias_fixed_total(tpm, windows, n_tx, total_out)) return false;
    bias_fixed_limbs(tpm, windows, n_tx, *total_out, limbs);
    return true;
}

}  // namespace skm
