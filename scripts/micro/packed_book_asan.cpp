// The packed pieces' book (seekmer_amd/csrc/skm_packed_book.h) under AddressSanitizer + UBSan, as a program of its
// own (CPU only, no GPU, no Python; tests/test_packed_book_host.py builds and runs it):
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -Iseekmer_amd/csrc scripts/micro/packed_book_asan.cpp -o /tmp/packed_book_asan
//   ASAN_OPTIONS=detect_leaks=1 /tmp/packed_book_asan
// With fixed seeds a book with a run cap of 7 units goes through random sequences of inserts (ascending, out of
// order, overlapping replacements), cuts, find_run -> segments(mark) -> consume, segments of a bare list, and
// drop_all, single-ended and paired, with units 0 to 40, pieces of 1 to 9 units, 1 to 3 code words, ragged and
// uniform lengths and about one read in three an exception.  After every operation the book is compared with a
// model that holds, for each stream and unit, the pushed piece and the index inside it, or nothing.  The "device"
// arrays are host blocks of exactly the pushed sizes that hold known values, so a segment's addresses are followed
// as well as compared, and every block has a deleter that counts.
#include "skm_packed_book.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using namespace skm::abi;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

namespace {

constexpr int64_t RUN_CAP = 7, MAX_FIRST = 40, MAX_LEN = 9, UNITS = MAX_FIRST + MAX_LEN + 1;

struct Pushed {                          // a piece as it was pushed (no hold on the block: the lists alone keep it alive)
    int64_t origin, n;
    int cw;
    int64_t uniform_len;
    char *block;
    uint64_t *codes;
    uint32_t *lengths, *exc_reads_dev, *exc_masks;
    std::vector<uint32_t> exc;
};
struct Cell { int piece = -1; int64_t index = 0; };

std::set<char *> live;                   // blocks whose deleter has not run
std::vector<Pushed> pushed;
Cell model[2][UNITS];
int64_t model_dropped = 0;
// how often the branches worth reaching were reached
int64_t seen_split = 0, seen_replace = 0, seen_out_of_order = 0, seen_cut_inside = 0, seen_capped = 0, seen_exc_offset = 0,
        seen_gap_end = 0, seen_runs = 0;

uint64_t code_value(size_t id, int64_t i, int w) { return (uint64_t)id * 1000003u + (uint64_t)i * 131u + (uint64_t)w; }
uint32_t length_value(size_t id, int64_t i) { return (uint32_t)(id * 977u + (uint64_t)i * 7u + 1u); }
uint32_t mask_value(size_t id, int64_t e, int w) { return (uint32_t)(id * 31u + (uint64_t)e * 17u + (uint64_t)w + 5u); }

PackedPiece make_piece(std::mt19937_64 &rng, int64_t first, int64_t n, int cw, bool uniform)
{
    Pushed p{};
    const size_t id = pushed.size();
    p.origin = first; p.n = n; p.cw = cw;
    p.uniform_len = uniform ? 32 * cw - 3 : -1;
    for (int64_t i = 0; i < n; ++i) if (rng() % 3 == 0) p.exc.push_back((uint32_t)i);
    const size_t codes_bytes = (size_t)n * cw * 8, len_bytes = uniform ? 0 : (size_t)n * 4, exc_bytes = p.exc.size() * 4;
    p.block = new char[codes_bytes + len_bytes + exc_bytes + p.exc.size() * cw * 4];
    CHECK(live.insert(p.block).second);
    p.codes = (uint64_t *)p.block;
    p.lengths = uniform ? nullptr : (uint32_t *)(p.block + codes_bytes);
    p.exc_reads_dev = (uint32_t *)(p.block + codes_bytes + len_bytes);
    p.exc_masks = (uint32_t *)(p.block + codes_bytes + len_bytes + exc_bytes);
    for (int64_t i = 0; i < n; ++i) {
        for (int w = 0; w < cw; ++w) p.codes[i * cw + w] = code_value(id, i, w);
        if (!uniform) p.lengths[i] = length_value(id, i);
    }
    for (size_t e = 0; e < p.exc.size(); ++e) {
        p.exc_reads_dev[e] = p.exc[e];
        for (int w = 0; w < cw; ++w) p.exc_masks[e * cw + w] = mask_value(id, (int64_t)e, w);
    }
    PackedPiece piece;
    piece.first = piece.origin = first;
    piece.n = n;
    piece.cw = cw;
    piece.uniform_len = p.uniform_len;
    piece.block = std::shared_ptr<char>(p.block, [](char *q) { CHECK(live.erase(q) == 1); delete[] q; });
    piece.codes = p.codes;
    piece.lengths = p.lengths;
    piece.exc_reads_dev = p.exc_reads_dev;
    piece.exc_masks = p.exc_masks;
    piece.exc_reads = p.exc;
    pushed.push_back(std::move(p));
    return piece;
}

bool covered(int stream, int64_t u) { return u >= 0 && u < UNITS && model[stream][u].piece >= 0; }

// lists: ascending, disjoint, no empty piece, exactly the model's units; dropped count; live blocks
void verify(const PackedBook &book)
{
    std::set<char *> referenced;
    for (int s = 0; s < 2; ++s) {
        int64_t cursor = -1, units = 0, in_model = 0;
        for (const PackedPiece &piece : book.pending[s]) {
            CHECK(piece.n > 0);
            CHECK(piece.first >= cursor && piece.first >= 0 && piece.first + piece.n <= UNITS);
            cursor = piece.first + piece.n;
            for (int64_t u = piece.first; u < cursor; ++u) {
                const Cell cell = model[s][u];
                CHECK(cell.piece >= 0);
                const Pushed &p = pushed[(size_t)cell.piece];
                CHECK(piece.origin == p.origin && u - piece.origin == cell.index);
                CHECK(piece.block.get() == p.block);       // (a head and a tail of one piece: one block)
                CHECK(piece.codes == p.codes && piece.lengths == p.lengths && piece.exc_reads_dev == p.exc_reads_dev
                      && piece.exc_masks == p.exc_masks && piece.cw == p.cw && piece.uniform_len == p.uniform_len
                      && piece.exc_reads == p.exc);
            }
            units += piece.n;
            referenced.insert(piece.block.get());
        }
        for (int64_t u = 0; u < UNITS; ++u) in_model += covered(s, u);
        CHECK(units == in_model);
    }
    CHECK(referenced == live);
    CHECK(book.dropped == model_dropped);
    CHECK(book.empty() == live.empty());
}

// the segments of stream `s` in [lo, hi): ascending, disjoint, exactly the model's units there (`tiles`: all of them,
// exactly once), with the addresses and the exceptions of the pieces as pushed
void check_segments(const std::vector<PackedSegment> &segments, int s, int64_t lo, int64_t hi, bool tiles)
{
    int64_t cursor = lo, units = 0, in_model = 0;
    for (const PackedSegment &seg : segments) {
        if (seg.mate != s) continue;
        CHECK(seg.n > 0 && seg.first >= cursor && seg.first + seg.n <= hi);
        if (tiles) CHECK(seg.first == cursor);
        cursor = seg.first + seg.n;
        units += seg.n;
        const Cell head = model[s][seg.first];
        CHECK(head.piece >= 0);
        const Pushed &p = pushed[(size_t)head.piece];
        CHECK(seg.cw == p.cw);
        CHECK(seg.uniform_len == (uint32_t)(p.uniform_len < 0 ? 0 : p.uniform_len));
        CHECK((seg.lengths == nullptr) == (p.uniform_len >= 0));
        for (int64_t u = seg.first; u < cursor; ++u) {
            const Cell cell = model[s][u];
            CHECK(cell.piece == head.piece && cell.index == head.index + (u - seg.first));
            CHECK(seg.codes + (u - seg.first) * seg.cw == p.codes + cell.index * p.cw);
            for (int w = 0; w < seg.cw; ++w)
                CHECK(seg.codes[(u - seg.first) * seg.cw + w] == code_value((size_t)cell.piece, cell.index, w));
            if (seg.lengths) {
                CHECK(seg.lengths + (u - seg.first) == p.lengths + cell.index);
                CHECK(seg.lengths[u - seg.first] == length_value((size_t)cell.piece, cell.index));
            }
        }
        CHECK(seg.exc_base == head.index);
        int64_t before = 0, inside = 0;
        for (uint32_t e : p.exc) {
            before += (int64_t)e < head.index;
            inside += (int64_t)e >= head.index && (int64_t)e < head.index + seg.n;
        }
        CHECK(seg.n_exc == inside);
        CHECK(seg.exc_reads == p.exc_reads_dev + before);
        CHECK(seg.exc_masks == p.exc_masks + before * p.cw);
        for (int64_t k = 0; k < seg.n_exc; ++k) {
            CHECK(seg.exc_reads[k] == p.exc[(size_t)(before + k)]);
            CHECK((int64_t)seg.exc_reads[k] >= seg.exc_base && (int64_t)seg.exc_reads[k] < seg.exc_base + seg.n);
            for (int w = 0; w < seg.cw; ++w) CHECK(seg.exc_masks[k * seg.cw + w] == mask_value((size_t)head.piece, before + k, w));
        }
        seen_exc_offset += before > 0 && inside > 0;
    }
    for (int64_t u = lo; u < hi; ++u) in_model += covered(s, u);
    CHECK(units == in_model);
    if (tiles) CHECK(cursor == hi && units == hi - lo);
}

// the lowest unit that every stream covers, and on while the coverage is contiguous, up to the cap
bool model_run(int streams, int64_t *lo, int64_t *hi)
{
    auto all = [&](int64_t u) { return covered(0, u) && (streams == 1 || covered(1, u)); };
    int64_t u = 0;
    while (u < UNITS && !all(u)) ++u;
    if (u == UNITS) return false;
    *lo = *hi = u;
    while (*hi < UNITS && all(*hi) && *hi - *lo < RUN_CAP) ++*hi;
    return true;
}

void model_clear_from(int s, int64_t from, bool count)
{
    for (int64_t u = std::max<int64_t>(from, 0); u < UNITS; ++u) {
        if (count && covered(s, u)) model_dropped += 1;
        model[s][u] = Cell{};
    }
}

void insert(PackedBook &book, std::mt19937_64 &rng, int s, int64_t first, int64_t n)
{
    const int cw = 1 + (int)(rng() % 3);
    PackedPiece piece = make_piece(rng, first, n, cw, rng() % 2 == 0);
    bool overlap = false, behind = false;
    for (int64_t u = first; u < first + n; ++u) overlap = overlap || covered(s, u);
    for (int64_t u = first + n; u < UNITS; ++u) behind = behind || covered(s, u);
    CHECK(book.overlaps(s, first, n) == overlap);
    if (overlap) { model_clear_from(s, first, false); ++seen_replace; }     // (a replacement counts nothing as dropped)
    else seen_out_of_order += behind;
    for (int64_t i = 0; i < n; ++i) model[s][first + i] = Cell{(int)pushed.size() - 1, i};
    book.insert(s, std::move(piece));
}

void sequence(uint64_t seed, bool paired, int n_ops)
{
    std::mt19937_64 rng(seed);
    const int streams = paired ? 2 : 1;
    {
        PackedBook book(RUN_CAP);
        CHECK(book.max_run == RUN_CAP && book.paired == -1 && book.dropped == 0 && book.empty());
        book.paired = paired ? 1 : 0;
        for (auto &row : model) for (auto &cell : row) cell = Cell{};
        model_dropped = 0;
        pushed.clear();
        for (int op = 0; op < n_ops; ++op) {
            const int kind = (int)(rng() % 20);
            const int s = (int)(rng() % (uint64_t)streams);
            if (kind < 6) {                           // an ascending insert: behind everything the stream holds
                int64_t end = 0;
                for (int64_t u = 0; u < UNITS; ++u) if (covered(s, u)) end = u + 1;
                if (rng() % 4 == 0) end += 1 + (int64_t)(rng() % 3);          // (with a gap now and then)
                if (end <= MAX_FIRST) insert(book, rng, s, end, 1 + (int64_t)(rng() % MAX_LEN));
            } else if (kind < 10) {                   // anywhere: out of order, into a gap, or over what is there
                insert(book, rng, s, (int64_t)(rng() % (MAX_FIRST + 1)), 1 + (int64_t)(rng() % MAX_LEN));
            } else if (kind < 12) {                   // a cut
                const int64_t from = (int64_t)(rng() % (MAX_FIRST + 2));
                seen_cut_inside += from > 0 && covered(s, from) && covered(s, from - 1)
                                   && model[s][from].piece == model[s][from - 1].piece;
                model_clear_from(s, from, true);
                book.truncate(s, from, true);
            } else if (kind < 18) {                   // what the worker does: a run, its segments, and the run consumed
                int64_t lo = -1, hi = -1, want_lo = -1, want_hi = -1;
                const bool found = book.find_run(&lo, &hi), want = model_run(streams, &want_lo, &want_hi);
                CHECK(found == want);
                if (found) {
                    CHECK(lo == want_lo && hi == want_hi && hi > lo && hi - lo <= RUN_CAP);
                    ++seen_runs;
                    if (hi - lo == RUN_CAP) {
                        bool more = covered(0, hi) && (streams == 1 || covered(1, hi));
                        seen_capped += more;
                    } else {
                        seen_gap_end += 1;
                    }
                    std::vector<PackedSegment> segments;
                    int max_cw = 1, want_cw = 1;
                    for (int t = 0; t < streams; ++t) book.segments(t, lo, hi, true, &segments, &max_cw);
                    for (const PackedSegment &seg : segments) want_cw = std::max(want_cw, seg.cw);
                    CHECK(max_cw == want_cw);
                    for (int t = 0; t < streams; ++t) {
                        check_segments(segments, t, lo, hi, true);
                        CHECK(book.in_flight_from(t, hi - 1) && !book.in_flight_from(t, UNITS));
                    }
                    for (int t = 0; t < streams; ++t) {
                        seen_split += lo > 0 && covered(t, lo - 1) && covered(t, hi)
                                      && model[t][lo - 1].piece == model[t][hi].piece;
                        for (int64_t u = lo; u < hi; ++u) model[t][u] = Cell{};
                        book.consume(t, lo, hi);
                        CHECK(!book.in_flight_from(t, -1));
                    }
                }
            } else if (kind < 19) {                   // segments of a list that no run was found in (the sample set's use)
                const int64_t lo = (int64_t)(rng() % UNITS), hi = lo + (int64_t)(rng() % (uint64_t)(UNITS - lo + 1));
                std::vector<PackedSegment> segments;
                int max_cw = 1;
                PackedBook::segments(book.pending[s], s, lo, hi, false, &segments, &max_cw);
                check_segments(segments, s, lo, hi, false);
                CHECK(!book.in_flight_from(s, -1));
            } else if (rng() % 3 == 0) {              // nothing more can be mapped
                for (int t = 0; t < 2; ++t) model_clear_from(t, 0, true);
                book.drop_all();
                CHECK(live.empty());
            }
            verify(book);
        }
    }
    CHECK(live.empty());                              // the book has gone: so has every block
}

}  // namespace

int main()
{
    for (uint64_t seed = 1; seed <= 3000; ++seed) {
        sequence(seed, false, 60);
        sequence(seed + 1000000, true, 90);
    }
    CHECK(seen_runs > 1000 && seen_split > 0 && seen_replace > 0 && seen_out_of_order > 0 && seen_cut_inside > 0
          && seen_capped > 0 && seen_gap_end > 0 && seen_exc_offset > 0);
    printf("runs %lld, capped %lld, pieces split in two %lld, replacements %lld, out of order %lld, cuts inside a piece %lld, "
           "segments behind earlier exceptions %lld\n", (long long)seen_runs, (long long)seen_capped, (long long)seen_split,
           (long long)seen_replace, (long long)seen_out_of_order, (long long)seen_cut_inside, (long long)seen_exc_offset);
    printf("ok\n");
    return 0;
}
