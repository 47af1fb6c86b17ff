// The sample-set handle of the C ABI glue with the types of its members, for the units that look into it
// (skm_abi_samples.hip, which owns it, skm_abi_genes.hip and skm_abi_quant.hip), and the call that makes its tables
// by sample.
#pragma once
#include "skm_abi_mapper.h"
#include "skm_packed_book.h"

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

struct SetChunk {                        // the reads of one added segment where they lie in HBM
    std::deque<PackedPiece> pieces[2];         // packed form: one piece per mate, numbered by the sample's units
    std::shared_ptr<char> ascii;         // ASCII form: one block, offsets | bases
    const uint8_t *bases = nullptr;      // biased: read r of the segment = bases[offsets[r] .. offsets[r + 1])
    const int64_t *offsets = nullptr;    // [reads + 1], as the caller gave them
    int64_t origin = 0;                  // the sample's unit of the segment's first read
    int max_len = 0;
    std::shared_ptr<uint32_t> umis;      // a set that keeps UMIs: umis[u - umi_origin] of the segment's unit u, in HBM
    int64_t umi_origin = 0;
};
struct SetQueued { int32_t sample; int64_t first, n; std::shared_ptr<SetChunk> data; };   // what is left of a segment
struct SetPart { int32_t sample; int64_t first, n, at; std::shared_ptr<SetChunk> data; }; // units [first, first + n) of
                                                                                         // the sample at place `at` of a launch

// which units of which sample the set's unit numbers are: one entry per part of every launch, in launch
// order, so `global` ascends and the entries tile [0, units)
struct SetLog {
    std::vector<int64_t> global, local;
    std::vector<int32_t> sample;
    int64_t units = 0;
    void append(const std::vector<SetPart> &parts)
    {
        for (const SetPart &part : parts) {
            global.push_back(units + part.at);
            local.push_back(part.first);
            sample.push_back(part.sample);
        }
        if (!parts.empty()) units += parts.back().at + parts.back().n;
    }
};

}  // namespace abi
}  // namespace skm

struct skm_sample_set {
    skm_sample_set(skm_mapper *mapper, int paired_) : m(mapper), paired(paired_) {}
    ~skm_sample_set();
    Own<skm_mapper *, skm_mapper_destroy> m;      // (declared first: given up last)
    const int paired;
    int64_t max_units = PACKED_MAX_UNITS;         // of one launch (SKM_SAMPLE_SET_MAX_UNITS)
    std::mutex copy_mu;                           // one adder copies at a time
    Stream copy_stream;
    std::shared_ptr<std::atomic<int64_t>> bytes = std::make_shared<std::atomic<int64_t>>(0);
    DBuf<int32_t> seg_table;                      // the segments of the launch under way: first units | samples
    // one fragment-length histogram per sample (skm_sample_set_keep_histograms): [rows][2000], rows >= the
    // largest sample a launch has held + 1, every word up to hist.cap counted or zero; touched under m->mu
    bool keep_hist = false;
    DBuf<unsigned long long> hist;
    // one row of observed hexamers per sample (skm_sample_set_keep_bias): [rows][4096], kept as `hist` is
    bool keep_bias = false;
    DBuf<unsigned long long> bias_rows;
    // UMI collapse (skm_sample_set_keep_umis; skm_umi.hip): the molecule set -- umi_n_slots slots, a power of two,
    // sized ahead of every launch to at least twice (molecules so far + the launch's records) --, its counters,
    // the units removed per sample (rows kept as `hist` is) and the segments' UMIs of the launch under way;
    // touched under m->mu.  SKM_TEST_UMI_SLOTS: the set starts at that many slots and grows only when a launch
    // finds it full.  umi_mismatches (skm_sample_set_set_umi_mismatches, under mu like umi_bases): 1 = resolve also
    // removes a unit that an earlier unit with a UMI one substitution away precedes; umi_near = those removed so.
    int umi_bases = 0;                            // 0: the set keeps no UMIs
    int umi_mismatches = 0;
    int64_t umi_near = 0;
    DBuf<UmiSlot> umi_slots;
    uint64_t umi_n_slots = 0, umi_test_slots = 0;
    int64_t umi_entries = 0;
    DBuf<unsigned long long> umi_ctl, umi_removed;
    DBuf<UmiSegment> umi_segs;
    // ---- under mu
    std::mutex mu;
    std::condition_variable work_cv, done_cv;
    std::deque<SetQueued> queue;
    int64_t queued_units = 0;
    std::vector<int64_t> sample_units;            // units added per sample = where its next segment must begin
    SetLog log;
    bool busy = false, stop = false, worker_started = false;
    int flush = 0;
    int error = SKM_OK;                           // the first failed launch: the set stays failed
    std::string error_msg;
    std::thread worker;
    // the tables by sample, made by the first reader after the last launch
    struct View {
        bool valid = false;
        std::vector<int64_t> start, len, count, local, order, sample_class_offsets, sample_rows, sample_aligned;
        std::vector<int64_t> units;               // sample_units as the view was made, all of them mapped, less `removed`
        std::vector<int64_t> removed;             // the units UMI collapse has removed, per sample (zeros without it)
        std::vector<int32_t> arena;
        // the classes where class_compact and sample_assign left them in HBM (registry order), kept with the view
        // for the calls that pass over the table on the device (skm_sample_set_gene_counts)
        DBuf<int64_t> d_start, d_len;
        DBuf<double> d_count;
        DBuf<int32_t> d_sample;
    } view;
};

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// (defined in skm_abi_samples.hip) waits for the set's launches and makes s->view if it is not valid; `hold` then holds s->mu
int set_view(skm_sample_set *s, std::unique_lock<std::mutex> &hold);

}  // namespace abi
}  // namespace skm
