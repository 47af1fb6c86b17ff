// skm_packed_gather (include/seekmer_hip.h): selected reads of packed pieces written as one new piece.  The
// demultiplexer's host half: after the units of a chunk have been grouped by cell on the GPU, each mate's reads
// are moved once, in that order, into one piece whose sub-ranges are the cells' segments.  Memory-bound work
// (32 bytes of codes per 100-base read), one pass, no allocation.
#include "../../include/seekmer_hip.h"

#include <algorithm>
#include <cstring>

namespace {

// the exception entry of read r of a piece, or -1 (exception_reads ascend)
int64_t exception_of(const skm_packed_reads &p, uint32_t r)
{
    const uint32_t *first = p.exception_reads, *last = first + p.n_exceptions;
    const uint32_t *at = std::lower_bound(first, last, r);
    return at != last && *at == r ? at - first : -1;
}

}  // namespace

extern "C" int skm_packed_gather(const skm_packed_reads *sources, int64_t n_sources, const int32_t *order,
                                 int64_t count, int32_t code_words, uint64_t *codes, uint32_t *lengths,
                                 uint32_t *exception_reads, uint32_t *exception_masks, int64_t cap_exceptions,
                                 int64_t *n_exceptions)
{
    if (n_sources < 0 || count < 0 || count >= (1LL << 31) || code_words < 0 || !n_exceptions || (n_sources && !sources) ||
        (count && !order) || (codes && count && !lengths))
        return SKM_ERR_ARG;
    int64_t total = 0;
    for (int64_t s = 0; s < n_sources; ++s) {
        const skm_packed_reads &p = sources[s];
        if (p.n_reads < 0 || p.code_words < 0 || p.code_words > code_words || p.read_stride < p.code_words ||
            p.n_exceptions < 0 || (p.n_reads && p.code_words && !p.codes) || (p.n_reads && !p.lengths && p.uniform_len < 0) ||
            (p.n_exceptions && (!p.exception_reads || !p.exception_masks)))
            return SKM_ERR_ARG;
        total += p.n_reads;
    }
    int64_t n_exc = 0;
    int64_t s = 0, base = 0;                  // the source that holds the read looked at last (orders are mostly runs)
    for (int64_t i = 0; i < count; ++i) {
        const int64_t at = order[i];
        if (at < 0 || at >= total) return SKM_ERR_ARG;
        while (at < base) base -= sources[--s].n_reads;
        while (at >= base + sources[s].n_reads) base += sources[s++].n_reads;
        const skm_packed_reads &p = sources[s];
        const int64_t r = at - base;
        if (codes) {
            uint64_t *to = codes + i * code_words;
            if (p.code_words) memcpy(to, p.codes + r * p.read_stride, (size_t)p.code_words * 8);
            for (int32_t w = p.code_words; w < code_words; ++w) to[w] = 0;
            lengths[i] = p.lengths ? p.lengths[r] : (uint32_t)p.uniform_len;
        }
        if (p.n_exceptions) {
            const int64_t e = exception_of(p, (uint32_t)r);
            if (e >= 0) {
                if (codes && n_exc < cap_exceptions) {
                    if (!exception_reads || !exception_masks) return SKM_ERR_ARG;
                    exception_reads[n_exc] = (uint32_t)i;
                    uint32_t *to = exception_masks + n_exc * code_words;
                    memcpy(to, p.exception_masks + e * p.code_words, (size_t)p.code_words * 4);
                    for (int32_t w = p.code_words; w < code_words; ++w) to[w] = 0;
                }
                ++n_exc;
            }
        }
    }
    *n_exceptions = n_exc;
    return codes && n_exc > cap_exceptions ? SKM_ERR_STATE : SKM_OK;
}
