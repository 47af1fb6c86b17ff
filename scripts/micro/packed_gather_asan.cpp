// skm_packed_gather under AddressSanitizer + UBSan, as a program of its own (CPU only, no GPU, no Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       scripts/micro/packed_gather_asan.cpp seekmer_amd/csrc/skm_packed_gather.cpp -o /tmp/packed_gather_asan
//   /tmp/packed_gather_asan
// Pieces of every shape the tests use (strided codes, ragged and uniform lengths, with and without exceptions,
// an empty piece, different widths), orders that permute, repeat and span them, exact-size output arrays (so a
// write past any of them is caught), and every result compared with a plain loop.
#include "seekmer_hip.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

struct Piece {
    std::vector<uint64_t> codes;
    std::vector<uint32_t> lengths, exception_reads, exception_masks;
    skm_packed_reads raw{};
};

static Piece make(std::mt19937_64 &rng, int64_t n, int32_t code_words, int64_t stride, bool uniform, int every)
{
    Piece p;
    p.codes.resize((size_t)(n ? (n - 1) * stride + code_words : 0));      // (exactly what the struct promises)
    for (auto &w : p.codes) w = rng();
    p.lengths.resize((size_t)n);
    for (auto &l : p.lengths) l = uniform ? 32u * code_words - 3 : 1 + (uint32_t)(rng() % (32u * code_words));
    for (int64_t r = 0; every && r < n; r += every) {
        p.exception_reads.push_back((uint32_t)r);
        for (int32_t w = 0; w < code_words; ++w) p.exception_masks.push_back((uint32_t)rng());
    }
    p.raw.code_words = code_words; p.raw.n_reads = n; p.raw.read_stride = stride;
    p.raw.uniform_len = uniform && n ? p.lengths[0] : -1;
    p.raw.codes = p.codes.data();
    p.raw.lengths = uniform && n ? nullptr : p.lengths.data();
    p.raw.n_exceptions = (int64_t)p.exception_reads.size();
    p.raw.exception_reads = p.exception_reads.empty() ? nullptr : p.exception_reads.data();
    p.raw.exception_masks = p.exception_masks.empty() ? nullptr : p.exception_masks.data();
    return p;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

int main()
{
    std::mt19937_64 rng(7);
    std::vector<Piece> pieces;
    pieces.push_back(make(rng, 37, 2, 2, false, 5));
    pieces.push_back(make(rng, 1, 3, 4, true, 1));
    pieces.push_back(make(rng, 0, 3, 3, true, 0));
    pieces.push_back(make(rng, 64, 1, 6, true, 3));
    pieces.push_back(make(rng, 20, 3, 3, false, 0));
    std::vector<skm_packed_reads> sources;
    std::vector<int64_t> base{0};
    for (auto &p : pieces) { sources.push_back(p.raw); base.push_back(base.back() + p.raw.n_reads); }
    const int64_t total = base.back();
    const int32_t code_words = 3;
    for (int round = 0; round < 200; ++round) {
        const int64_t count = round == 0 ? 0 : (int64_t)(rng() % (2 * total));
        std::vector<int32_t> order((size_t)count);
        for (auto &o : order) o = (int32_t)(rng() % total);
        if (round == 1) { order.resize((size_t)total); for (int64_t i = 0; i < total; ++i) order[i] = (int32_t)i; }
        const int64_t n = (int64_t)order.size();
        int64_t n_exc = -1;
        CHECK(skm_packed_gather(sources.data(), (int64_t)sources.size(), order.data(), n, code_words, nullptr, nullptr, nullptr,
                                nullptr, 0, &n_exc) == SKM_OK);
        std::vector<uint64_t> codes((size_t)(n * code_words));
        std::vector<uint32_t> lengths((size_t)n), reads((size_t)n_exc), masks((size_t)(n_exc * code_words));
        int64_t again = -1;
        if (n_exc)
            CHECK(skm_packed_gather(sources.data(), (int64_t)sources.size(), order.data(), n, code_words, codes.data(), lengths.data(),
                                    reads.data(), masks.data(), n_exc - 1, &again) == SKM_ERR_STATE && again == n_exc);
        CHECK(skm_packed_gather(sources.data(), (int64_t)sources.size(), order.data(), n, code_words, codes.data(), lengths.data(),
                                reads.data(), masks.data(), n_exc, &again) == SKM_OK && again == n_exc);
        int64_t e = 0;
        for (int64_t i = 0; i < n; ++i) {
            size_t s = 0;
            while (order[i] >= base[s + 1]) ++s;
            const Piece &p = pieces[s];
            const int64_t r = order[i] - base[s];
            for (int32_t w = 0; w < code_words; ++w)
                CHECK(codes[i * code_words + w] == (w < p.raw.code_words ? p.codes[r * p.raw.read_stride + w] : 0));
            CHECK(lengths[i] == p.lengths[r]);
            for (size_t k = 0; k < p.exception_reads.size(); ++k)
                if (p.exception_reads[k] == (uint32_t)r) {
                    CHECK(e < n_exc && reads[e] == (uint32_t)i);
                    for (int32_t w = 0; w < code_words; ++w)
                        CHECK(masks[e * code_words + w] == (w < p.raw.code_words ? p.exception_masks[k * p.raw.code_words + w] : 0));
                    ++e;
                }
        }
        CHECK(e == n_exc);
    }
    int32_t outside = (int32_t)total;
    int64_t n_exc = 0;
    CHECK(skm_packed_gather(sources.data(), (int64_t)sources.size(), &outside, 1, code_words, nullptr, nullptr, nullptr, nullptr, 0,
                            &n_exc) == SKM_ERR_ARG);
    puts("skm_packed_gather: ok");
    return 0;
}
