// skm_bias_fixed_weights: the fixed-point weights of the sequence-bias correction on the host alone (tests, and
// callers that want to see what the device is handed).  The arithmetic is skm_bias_weights.h's.
#include "../../include/seekmer_hip.h"
#include "skm_bias_weights.h"

extern "C" int skm_bias_fixed_weights(const double *tpm, const int32_t *windows, int64_t n_tx, uint64_t *limbs_out,
                                      double *total_out)
{
    if (n_tx < 0 || !total_out || (n_tx && (!tpm || !windows || !limbs_out))) return SKM_ERR_ARG;
    for (int64_t t = 0; t < n_tx; ++t)
        if (!(tpm[t] >= 0.0) || std::isinf(tpm[t]) || windows[t] < 0) return SKM_ERR_ARG;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "limbs are 64-bit words");
    return skm::bias_fixed_weights(tpm, windows, n_tx, reinterpret_cast<unsigned long long *>(limbs_out), total_out)
               ? SKM_OK : SKM_ERR_ARG;
}
