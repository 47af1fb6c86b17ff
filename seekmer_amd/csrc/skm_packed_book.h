// The book of the packed pieces: which reads, pushed as 2-bit code words (skm_mapper_push_packed), wait in HBM for
// their mates, which run of units every stream covers, what a mapped run, a cut or an overlapping piece leaves of a
// piece, and where a segment's codes and exceptions start.  It decides which reads meet as mates.  Host arithmetic
// only: the device pointers are plain pointers that nothing here follows, and the header needs the standard library
// alone, so scripts/micro/packed_book_asan.cpp checks it against a per-unit model on a CPU.
// The book has no mutex of its own: every call is made with the feed's queue mutex (skm_mapper::Feed::q_mu) held.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <memory>
#include <utility>
#include <vector>

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

constexpr int64_t PACKED_MIN_UNITS = 1 << 15;      // smaller runs wait for more (or for a flush)
constexpr int64_t PACKED_MAX_UNITS = 1 << 21;      // one launch

struct PackedPiece {
    int64_t first = 0, n = 0;             // units [first, first + n) of the stream (what is left of the piece)
    int64_t origin = 0;                   // first_read of the piece as pushed: the arrays start there
    int cw = 1;
    int64_t uniform_len = -1;
    std::shared_ptr<char> block;          // one HBM allocation: codes | lengths | exception reads | masks
    uint64_t *codes = nullptr;            // [n as pushed][cw]
    uint32_t *lengths = nullptr;          // or NULL (uniform_len)
    uint32_t *exc_reads_dev = nullptr, *exc_masks = nullptr;
    std::vector<uint32_t> exc_reads;      // host copy (indices relative to origin), for cutting runs
    bool in_job = false;
};

struct PackedSegment {               // part of one piece inside a run
    int mate;
    int64_t first, n;                // units
    const uint64_t *codes;
    const uint32_t *lengths;
    int cw;
    uint32_t uniform_len;
    const uint32_t *exc_reads, *exc_masks;   // device, already offset to the segment's first exception
    int64_t n_exc;
    int64_t exc_base;                // index (relative to the piece as pushed) of the segment's first read
};

// One ascending list of pieces per stream, until the worker maps a run of units that every stream covers.
struct PackedBook {
    explicit PackedBook(int64_t max_run_units = PACKED_MAX_UNITS) : max_run(max_run_units) {}

    std::deque<PackedPiece> pending[2];
    int paired = -1;                          // -1 until the first piece
    int64_t dropped = 0;                      // reads that never got a mate
    const int64_t max_run;                    // units of one run at the most

    bool empty() const { return pending[0].empty() && pending[1].empty(); }

    // the first run of units that every stream covers: [*lo, *hi), at most max_run
    bool find_run(int64_t *lo, int64_t *hi) const
    {
        const auto &a = pending[0];
        if (a.empty()) return false;
        if (paired != 1) {
            *lo = a.front().first;
            *hi = *lo;
            for (const auto &piece : a) {
                if (piece.first != *hi) break;
                *hi += piece.n;
                if (*hi - *lo >= max_run) { *hi = *lo + max_run; break; }
            }
            return *hi > *lo;
        }
        const auto &b = pending[1];
        size_t i = 0, j = 0;
        bool open = false;
        while (i < a.size() && j < b.size()) {
            const int64_t from = std::max(a[i].first, b[j].first);
            const int64_t to = std::min(a[i].first + a[i].n, b[j].first + b[j].n);
            if (from < to) {
                if (!open) { *lo = from; *hi = to; open = true; }
                else if (from == *hi) *hi = to;
                else break;
                if (*hi - *lo >= max_run) { *hi = *lo + max_run; break; }
            }
            if (a[i].first + a[i].n <= b[j].first + b[j].n) ++i; else ++j;
        }
        return open;
    }

    // forget units [lo, hi) of a stream: they have been mapped.  What a piece holds before `lo` (reads whose
    // mates have not arrived yet) and after `hi` stays, sharing the block.
    void consume(int stream, int64_t lo, int64_t hi)
    {
        auto &list = pending[stream];
        std::deque<PackedPiece> kept;
        for (auto &piece : list) {
            piece.in_job = false;
            const int64_t end = piece.first + piece.n;
            if (end <= lo || piece.first >= hi) { kept.push_back(std::move(piece)); continue; }
            if (piece.first < lo) {
                PackedPiece head = piece;
                head.n = lo - piece.first;
                kept.push_back(std::move(head));
            }
            if (end > hi) {
                PackedPiece tail = piece;
                tail.first = hi;
                tail.n = end - hi;
                kept.push_back(std::move(tail));
            }
        }
        list.swap(kept);
    }

    // nothing more can be mapped: reads without a mate go
    void drop_all()
    {
        for (auto &list : pending) {
            for (auto &piece : list) dropped += piece.n;
            list.clear();
        }
    }

    // the parts of a stream's pieces that lie in units [lo, hi), as segments of a launch (also for a list of
    // pieces that no book holds: the sample set's chunks)
    static void segments(std::deque<PackedPiece> &pieces, int mate, int64_t lo, int64_t hi, bool mark_in_job,
                         std::vector<PackedSegment> *segments, int *max_cw)
    {
        for (auto &piece : pieces) {
            const int64_t from = std::max(lo, piece.first), to = std::min(hi, piece.first + piece.n);
            if (from >= to) continue;
            if (mark_in_job) piece.in_job = true;
            PackedSegment seg{};
            seg.mate = mate;
            seg.first = from;
            seg.n = to - from;
            const int64_t skip = from - piece.origin;
            seg.codes = piece.codes + skip * piece.cw;
            seg.lengths = piece.lengths ? piece.lengths + skip : nullptr;
            seg.cw = piece.cw;
            seg.uniform_len = (uint32_t)std::max<int64_t>(piece.uniform_len, 0);
            const auto e0 = std::lower_bound(piece.exc_reads.begin(), piece.exc_reads.end(), (uint32_t)skip);
            const auto e1 = std::lower_bound(piece.exc_reads.begin(), piece.exc_reads.end(), (uint32_t)(skip + seg.n));
            seg.n_exc = e1 - e0;
            const int64_t at = e0 - piece.exc_reads.begin();
            seg.exc_reads = piece.exc_reads_dev + at;
            seg.exc_masks = piece.exc_masks + at * piece.cw;
            seg.exc_base = skip;
            *max_cw = std::max(*max_cw, piece.cw);
            segments->push_back(seg);
        }
    }
    void segments(int stream, int64_t lo, int64_t hi, bool mark_in_job, std::vector<PackedSegment> *out, int *max_cw)
    {
        segments(pending[stream], stream, lo, hi, mark_in_job, out, max_cw);
    }

    // is a piece of the stream that reaches past `from` being mapped
    bool in_flight_from(int stream, int64_t from) const
    {
        for (const auto &other : pending[stream])
            if (other.in_job && other.first + other.n > from) return true;
        return false;
    }

    // drop what the stream holds at or behind `from`; a cut counts what goes as reads that never got a mate, a
    // piece that replaces them does not
    void truncate(int stream, int64_t from, bool count_dropped)
    {
        auto &list = pending[stream];
        int64_t gone = 0;
        while (!list.empty() && list.back().first >= from) { gone += list.back().n; list.pop_back(); }
        if (!list.empty() && list.back().first + list.back().n > from) {
            gone += list.back().first + list.back().n - from;
            list.back().n = from - list.back().first;
        }
        if (count_dropped) dropped += gone;
    }

    bool overlaps(int stream, int64_t first, int64_t n) const
    {
        for (const auto &other : pending[stream])
            if (other.first < first + n && first < other.first + other.n) return true;
        return false;
    }

    // a piece joins its stream where its first unit puts it; one that overlaps what the stream holds replaces
    // the reads from its first one on
    void insert(int stream, PackedPiece &&held)
    {
        auto &list = pending[stream];
        if (overlaps(stream, held.first, held.n)) {
            truncate(stream, held.first, false);
            list.push_back(std::move(held));
        } else {
            size_t at = list.size();
            while (at > 0 && list[at - 1].first > held.first) --at;
            list.insert(list.begin() + (long)at, std::move(held));
        }
    }
};

}  // namespace abi
}  // namespace skm
