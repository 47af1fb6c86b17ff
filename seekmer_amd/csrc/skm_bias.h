// Sequence-bias correction (--bias): the structs and launchers of skm_bias.hip.  DESIGN.md section 4,
// "Sequence bias", states the model; tests/bias_reference.py restates it in numpy.
#pragma once
#include "skm_device.h"

namespace skm {

constexpr int BIAS_HEXAMER = 6;
constexpr int BIAS_BINS = 4096;                   // 4^6 hexamers, first base in the top two bits
constexpr int BIAS_LIMBS = 3;                     // E in 96-bit fixed point: three 32-bit limbs a weight, summed apart

// samples whose b tables a block of the many-sample lengths kernel holds in LDS (32 KB each): 1, 2 or 4.  A
// tuning build sets it (scripts/build_variant.sh NAME "-DSKM_BIAS_LENGTHS_G=4" skm_bias.hip); DESIGN.md section 4,
// "Sequence bias", has the measurement behind the default.
#ifndef SKM_BIAS_LENGTHS_G
#define SKM_BIAS_LENGTHS_G 1
#endif
constexpr int BIAS_LENGTHS_G = SKM_BIAS_LENGTHS_G;
static_assert(BIAS_LENGTHS_G == 1 || BIAS_LENGTHS_G == 2 || BIAS_LENGTHS_G == 4, "G x 32 KB of LDS: 1, 2 or 4");
constexpr int64_t BIAS_MANY_MAX_GROUP = 32768;    // samples of one launch at most (a grid dimension holds 65535)

// What the pool is rebuilt from, kept on the host by skm_index_create until the pool has been built: of
// every contig its place in the pooled bases and its slice of the target rows (entry, offset).
struct PoolContig {
    int64_t target_offset;
    int32_t offset, length, target_count, pad;
};

// The transcripts' own sequences in HBM: transcript t owns the words tx_word[t] .. tx_word[t + 1) of
// `codes` (32 bases per u64, first base in the top two bits) and of `known` (bit 31 - i of a word =
// base 32 w + i is covered by a target row); every transcript starts a word, one pad word closes both
// arrays, and bits beyond a transcript's length are zero.
struct TxPool {
    uint64_t *codes;
    uint32_t *known;
    const int64_t *tx_word;       // [n_tx + 1]
    const int32_t *tx_len;        // [n_tx]
    int64_t n_tx, n_words;
};

// Scatter the contigs' bases through their target rows into the (zeroed) pool: row (e, o) of a contig of
// length L with bases S writes T_e[o .. o + L) = S for e >= 0 and T_~e[o + 25 - L .. o + 25) = revcomp(S)
// for e < 0.  Rows that overlap write the same bases: the words are OR-ed together.  *bad_rows counts the
// rows that name no transcript or leave its length; they write nothing.
void launch_bias_pool_scatter(const uint64_t *seq2, const PoolContig *contigs, int64_t n_contigs, const Coord *targets,
                              const TxPool &pool, unsigned long long *bad_rows, hipStream_t stream);
// tx_windows[t] = n_t: the positions p <= len_t - 6 whose six bases are all known
void launch_bias_windows(const TxPool &pool, int32_t *tx_windows, hipStream_t stream);
// observed[h] += 1 for every record of a mapped batch whose tuple (after the strand filter) is not empty,
// at the hexamer of the first six bases of mate 1 (or the single read) -- unless one of the six is not an
// upper-case A, C, G or T (the record's bit plane says so)
void launch_bias_observed(const uint32_t *records, int record_words, int words_per_read, int paired,
                          const unsigned long long *rec_tuple, const int32_t *rec_unit, int64_t n_units,
                          unsigned long long *observed, hipStream_t stream);
// expected[k][h] += limb k of W_t for every window of every transcript (tx_weight[k][n_tx], limbs below 2^32,
// lowest first; expected[BIAS_LIMBS][4096]): at h+ (strand none, fr) and at h- (none, rf).  Integer adds only, so
// the result does not depend on the grid or on the order of arrival; a limb's sum stays below 2^63 for up to
// 2^31 additions, and no carry is needed until the three sums are put together
void launch_bias_expected(const TxPool &pool, const unsigned long long *tx_weight, int strand,
                          unsigned long long *expected, int blocks, hipStream_t stream);
// one block: with e[h] the value of the three limb sums, expected_out[h] = e[h] * scale, b[h] = ((O[h] + 1) /
// (sum O + 4096)) / (e[h] / sum e) where e[h] > 0, 1 elsewhere, and 1 everywhere when either sum is 0
void launch_bias_weights(const unsigned long long *observed, const unsigned long long *expected, double scale,
                         double *expected_out, double *b, hipStream_t stream);
// eff_out[t] = eff[t] * ((sum over the windows of t of s+ b[h+] + s- b[h-]) / n_t), eff[t] where n_t = 0;
// one wave per transcript, its sum in a fixed order
void launch_bias_lengths(const TxPool &pool, const int32_t *tx_windows, const double *b, int strand, const double *eff,
                         double *eff_out, int blocks, hipStream_t stream);
// The same three for n samples in one launch each (skm_bias_correct_many); every row has the bits of the call above
// on that row alone.  tx_weight[n][BIAS_LIMBS][n_tx], expected[n][BIAS_LIMBS][4096] (zeroed), observed[n][4096],
// scale[n], expected_out[n][4096], b[n][4096], eff[n][n_tx], eff_out[n][n_tx]; n <= BIAS_MANY_MAX_GROUP.
void launch_bias_expected_many(const TxPool &pool, const unsigned long long *tx_weight, int64_t n, int strand,
                               unsigned long long *expected, int blocks, hipStream_t stream);
void launch_bias_weights_many(const unsigned long long *observed, const unsigned long long *expected, const double *scale,
                              int64_t n, double *expected_out, double *b, hipStream_t stream);
void launch_bias_lengths_many(const TxPool &pool, const int32_t *tx_windows, const double *b, int64_t n, int strand,
                              const double *eff, double *eff_out, int blocks, hipStream_t stream);

}  // namespace skm
