// C ABI of libseekmer_hip.so: the sample sets -- the queue of added segments, the worker that cuts it into
// launches of the set's mapper, the tables by sample (set_view) and the host-only plan / split of a launch log.
#include "skm_abi_samples.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace skm;
using namespace skm::abi;

// ------------------------------------------------------------------ sample sets
// Many small samples through ONE mapper: their units share launches and the class table, in which a
// class is (sample, tuple) -- skm_samples.hip.  The set owns a mapper (its table, batch buffers, stream)
// and drives map_batch_resident itself: added segments wait in HBM in a queue, one worker cuts the
// front of the queue into launches and logs which units of which sample every launch held.
namespace {

// the next launch: whole segments from the front of the queue, the last one cut where the launch is full
int64_t set_cut_launch(std::deque<SetQueued> &queue, int64_t max_units, std::vector<SetPart> *parts)
{
    int64_t n_units = 0;
    parts->clear();
    while (!queue.empty() && n_units < max_units && (int)parts->size() < SAMPLE_LAUNCH_SEGMENTS) {
        SetQueued &front = queue.front();
        const int64_t take = std::min(front.n, max_units - n_units);
        parts->push_back(SetPart{front.sample, front.first, take, n_units, front.data});
        n_units += take;
        if (take == front.n) queue.pop_front();
        else { front.first += take; front.n -= take; }
    }
    return n_units;
}

// classes by (sample, first-seen unit inside the sample): order[k] = the class in place k,
// sample_class_offsets[i] = place of sample i's first class
void set_split_order(int64_t n_samples, int64_t n_classes, const int32_t *class_sample, const int64_t *class_local,
                     int64_t *order, int64_t *sample_class_offsets)
{
    std::iota(order, order + n_classes, (int64_t)0);
    std::sort(order, order + n_classes, [&](int64_t a, int64_t b) {
        return class_sample[a] != class_sample[b] ? class_sample[a] < class_sample[b] : class_local[a] < class_local[b];
    });
    std::fill(sample_class_offsets, sample_class_offsets + n_samples + 1, (int64_t)0);
    for (int64_t k = 0; k < n_classes; ++k) sample_class_offsets[class_sample[k] + 1]++;
    for (int64_t i = 0; i < n_samples; ++i) sample_class_offsets[i + 1] += sample_class_offsets[i];
}

constexpr int64_t SET_MAX_SAMPLES = 1 << 24;
constexpr int64_t SET_MAX_HIST_SAMPLES = 1 << 16;   // with a histogram per sample: rows of 16 KB by sample NUMBER, 1 GiB at most
constexpr int64_t SET_MAX_BIAS_SAMPLES = 1 << 15;   // counting hexamers: rows of 32 KB (4096 x u64) by sample NUMBER, 1 GiB at most
constexpr int64_t SET_MAX_QUEUED = 4 * PACKED_MAX_UNITS;     // units that may wait in HBM before an adder waits

// the molecule set in `n_slots` slots (a power of two): a fresh set, or the molecules of the old one rehashed
// (m->mu is held; the stream drains before the old slots go back to the pool)
int set_umi_grow(skm_sample_set *s, uint64_t n_slots)
{
    skm_mapper *m = s->m;
    if (n_slots > (1ULL << 36)) return fail(SKM_ERR_STATE, "a molecule set of %llu slots", (unsigned long long)n_slots);
    DBuf<UmiSlot> fresh;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });
    if (fresh.ensure((size_t)n_slots) != SKM_OK) {
        const std::string why = last_message();
        return fail(SKM_ERR_HIP, "UMI collapse: no device memory for a molecule set of %llu slots, %llu MB (64 bytes a molecule "
                    "at load 1/2; %lld molecules so far): %s", (unsigned long long)n_slots,
                    (unsigned long long)(n_slots * sizeof(UmiSlot) >> 20), (long long)s->umi_entries, why.c_str());
    }
    const UmiSet to{fresh.p, n_slots - 1, s->umi_ctl.p, m->error.p};
    if (s->umi_n_slots) launch_umi_rehash(UmiSet{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p}, to, m->stream);
    else launch_umi_init(to, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    s->umi_slots = std::move(fresh);
    s->umi_n_slots = n_slots;
    return SKM_OK;
}

// room for `rows` rows of `width` words on `stream`: what was held stays, what the buffer gains is zero
int set_grow_rows(DBuf<unsigned long long> &buf, size_t rows, size_t width, hipStream_t stream)
{
    const size_t held = buf.cap;
    SKM_TRY(buf.ensure(rows * width, true, stream));
    if (buf.cap > held) HIP_TRY(hipMemsetAsync(buf.p + held, 0, (buf.cap - held) * sizeof(unsigned long long), stream));
    return SKM_OK;
}

int set_launch(skm_sample_set *s, const std::vector<SetPart> &parts, int64_t n_units, int64_t global_first)
{
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int mates = s->paired ? 2 : 1;
    const int n_parts = (int)parts.size();
    if (n_parts > SAMPLE_LAUNCH_SEGMENTS) return fail(SKM_ERR_STATE, "%d segments in one launch", n_parts);
    std::vector<int32_t> table(2 * (size_t)n_parts);
    std::vector<UmiSegment> umi_segments;         // (a set that keeps UMIs)
    std::vector<PackedSegment> segments;          // `first` = place in the launch
    int max_cw = 0, max_len = 0;
    int32_t largest = 0;                          // sample of the launch
    for (int i = 0; i < n_parts; ++i) {
        const SetPart &part = parts[i];
        table[i] = (int32_t)part.at;
        table[n_parts + i] = part.sample;
        largest = std::max(largest, part.sample);
        if (part.data->ascii) { max_len = std::max(max_len, part.data->max_len); continue; }
        for (int mate = 0; mate < mates; ++mate) {
            const size_t from = segments.size();
            PackedBook::segments(part.data->pieces[mate], mate, part.first, part.first + part.n, false, &segments, &max_cw);
            for (size_t k = from; k < segments.size(); ++k) segments[k].first += part.at - part.first;
        }
    }
    max_len = std::max(max_len, max_cw * 32);
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (`table` is read by a queued copy)
    SKM_TRY(s->seg_table.ensure(2 * SAMPLE_LAUNCH_SEGMENTS));
    HIP_TRY(hipMemcpyAsync(s->seg_table.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    const SampleSalt salt{s->seg_table.p, s->seg_table.p + n_parts, n_parts};
    const RecordStage fill = [&](uint32_t *records, int words, int record_words) -> int {
        packed_unpack(segments, 0, mates, records, words, record_words, m->error.p, m->stream);
        for (const SetPart &part : parts) {
            if (!part.data->ascii) continue;
            launch_pack_reads(part.data->bases, part.data->offsets + (part.first - part.data->origin) * mates, part.n * mates,
                              words, record_words, records + part.at * mates * (int64_t)record_words, m->stream);
        }
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    // room for the rows of this launch's samples, the new ones zero
    if (s->keep_hist) SKM_TRY(set_grow_rows(s->hist, (size_t)largest + 1, MAX_FRAGMENT_LENGTH, m->stream));
    if (s->keep_bias) SKM_TRY(set_grow_rows(s->bias_rows, (size_t)largest + 1, BIAS_BINS, m->stream));
    // UMI collapse: the launch's segments with their UMIs, room in the molecule set, rows of removed[]; then claim and
    // resolve between the strand filter and everything that counts
    const BatchStage collapse = [&](const MapBatch &b) -> int {
        for (;;) {
            const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p};
            HIP_TRY(hipMemsetAsync(s->umi_ctl.p + UMI_CTL_LOST, 0, sizeof(unsigned long long), m->stream));
            launch_umi_claim(set, b, salt, s->umi_segs.p, m->stream);
            HIP_TRY(hipGetLastError());
            if (!s->umi_test_slots) break;        // (sized ahead: a full set is reported after the launch)
            unsigned long long *lost = m->pinned + 48;
            HIP_TRY(hipMemcpyAsync(lost, s->umi_ctl.p + UMI_CTL_LOST, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
            HIP_TRY(hipStreamSynchronize(m->stream));
            if (*lost == 0) break;
            // full under test: four times the slots, and the pass again -- find-or-claim and a minimum, so a
            // record that had its turn changes nothing by a second one
            SKM_TRY(set_umi_grow(s, s->umi_n_slots * 4));
        }
        const UmiSet set{s->umi_slots.p, s->umi_n_slots - 1, s->umi_ctl.p, m->error.p};
        launch_umi_resolve(set, b, salt, s->umi_segs.p, s->umi_removed.p, s->umi_bases, s->umi_mismatches, m->stream);
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    if (s->umi_bases) {
        umi_segments.reserve(n_parts);
        for (const SetPart &part : parts) {
            if (!part.data->umis) return fail(SKM_ERR_STATE, "a segment without UMIs in a set that keeps them");
            umi_segments.push_back(UmiSegment{part.first, part.data->umis.get() + (part.first - part.data->umi_origin)});
        }
        SKM_TRY(s->umi_segs.ensure(SAMPLE_LAUNCH_SEGMENTS));
        HIP_TRY(hipMemcpyAsync(s->umi_segs.p, umi_segments.data(), umi_segments.size() * sizeof(UmiSegment), hipMemcpyHostToDevice, m->stream));
        SKM_TRY(set_grow_rows(s->umi_removed, (size_t)largest + 1, 1, m->stream));
        if (!s->umi_ctl.p) {
            SKM_TRY(s->umi_ctl.ensure(UMI_CTL_WORDS));
            HIP_TRY(hipMemsetAsync(s->umi_ctl.p, 0, UMI_CTL_WORDS * sizeof(unsigned long long), m->stream));
        }
        uint64_t want = s->umi_test_slots ? s->umi_test_slots : 1024;
        if (!s->umi_test_slots)
            while (want < 2 * (uint64_t)(s->umi_entries + n_units)) want *= 2;
        if (s->umi_n_slots == 0 || (!s->umi_test_slots && want > s->umi_n_slots)) SKM_TRY(set_umi_grow(s, want));
    }
    SKM_TRY(map_batch_resident(m, nullptr, nullptr, n_units, s->paired, max_len, global_first, &fill, &salt,
                               s->keep_bias ? s->bias_rows.p : nullptr, s->umi_bases ? &collapse : nullptr));
    if (s->umi_bases) {                           // (the stream has drained)
        unsigned long long *ctl = m->pinned + 48;
        HIP_TRY(hipMemcpyAsync(ctl, s->umi_ctl.p, UMI_CTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        if (ctl[UMI_CTL_LOST])
            return fail(SKM_ERR_STATE, "the molecule set of %llu slots was full for %llu records", (unsigned long long)s->umi_n_slots,
                        ctl[UMI_CTL_LOST]);
        s->umi_entries = (int64_t)ctl[UMI_CTL_ENTRIES];
        s->umi_near = (int64_t)ctl[UMI_CTL_NEAR];
    }
    if (s->keep_hist) {
        // the spans of the attempt that stood (an overflowing entry arena runs the map kernel again), after
        // the pair rule; they stay until this mapper's next launch, which the set's worker starts after this one
        if (!m->last_spans) return fail(SKM_ERR_STATE, "a set that keeps histograms mapped without spans");
        launch_sample_fld(m->unit_begin.p, m->unit_end.p, n_units, salt, s->hist.p, m->stream);
        HIP_TRY(hipGetLastError());
    }
    return SKM_OK;
}

void set_worker(skm_sample_set *s)
{
    for (;;) {
        std::vector<SetPart> parts;
        int64_t n_units = 0, global_first = 0;
        {
            std::unique_lock<std::mutex> hold(s->mu);
            s->work_cv.wait(hold, [&] {
                return s->stop || (!s->queue.empty()
                                   && (s->error != SKM_OK || s->flush || s->queued_units >= std::min(PACKED_MIN_UNITS, s->max_units)));
            });
            if (s->stop || s->error != SKM_OK) {          // nothing more is mapped: what waits goes
                s->queue.clear();
                s->queued_units = 0;
                s->done_cv.notify_all();
                if (s->stop) return;
                continue;
            }
            n_units = set_cut_launch(s->queue, s->max_units, &parts);
            s->queued_units -= n_units;
            global_first = s->log.units;
            s->log.append(parts);
            s->view.valid = false;
            s->busy = true;
        }
        const int rc = set_launch(s, parts, n_units, global_first);
        const std::string message = rc != SKM_OK ? last_message() : std::string();
        if (rc != SKM_OK) (void)hipStreamSynchronize(s->m->stream);   // (before the parts' blocks go back to the pool)
        parts.clear();
        {
            std::lock_guard<std::mutex> hold(s->mu);
            if (rc != SKM_OK) { s->error = rc; s->error_msg = message; }
            s->busy = false;
        }
        s->done_cv.notify_all();
    }
}

// (before the copy) the caller's arguments, and room in the queue
int set_admit(skm_sample_set *s, int64_t sample, int64_t first_unit, int64_t n_units)
{
    if (sample < 0 || sample >= SET_MAX_SAMPLES) return fail(SKM_ERR_ARG, "sample %lld outside [0, 2^24)", (long long)sample);
    if (first_unit < 0 || n_units < 0 || n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "bad unit range");
    SKM_TRY(set_device(s->m->ix->device));
    std::unique_lock<std::mutex> hold(s->mu);
    if (s->keep_hist && sample >= SET_MAX_HIST_SAMPLES)
        return fail(SKM_ERR_ARG, "sample %lld: a set that keeps a histogram per sample numbers its samples below %lld",
                    (long long)sample, (long long)SET_MAX_HIST_SAMPLES);
    if (s->keep_bias && sample >= SET_MAX_BIAS_SAMPLES)
        return fail(SKM_ERR_ARG, "sample %lld: a set that counts hexamers per sample numbers its samples below %lld",
                    (long long)sample, (long long)SET_MAX_BIAS_SAMPLES);
    s->done_cv.wait(hold, [&] { return s->error != SKM_OK || s->queued_units <= SET_MAX_QUEUED; });
    if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
    return SKM_OK;
}

// (after the copy) the segment joins the queue if it begins where the sample's units so far end
int set_enqueue(skm_sample_set *s, int64_t sample, int64_t first_unit, int64_t n_units, std::shared_ptr<SetChunk> data)
{
    {
        std::lock_guard<std::mutex> hold(s->mu);
        if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
        if ((int64_t)s->sample_units.size() <= sample) s->sample_units.resize((size_t)sample + 1, 0);
        if (first_unit != s->sample_units[sample])
            return fail(SKM_ERR_STATE, "sample %lld: a segment from unit %lld after %lld units (segments are added in order)",
                        (long long)sample, (long long)first_unit, (long long)s->sample_units[sample]);
        s->sample_units[sample] += n_units;
        s->view.valid = false;
        if (n_units == 0) return SKM_OK;
        s->queue.push_back(SetQueued{(int32_t)sample, first_unit, n_units, std::move(data)});
        s->queued_units += n_units;
        if (!s->worker_started) {
            s->worker = std::thread(set_worker, s);
            s->worker_started = true;
        }
    }
    s->work_cv.notify_all();
    return SKM_OK;
}

// `hold` (s->mu) is taken here, when everything added has been mapped, and stays taken for the caller's
// reading: from that moment no segment joins the queue (an adder waits in set_enqueue), so what the caller
// reads, the log and the units per sample describe the same units.
// set_view: the tables by sample (s->view), made once after the last launch.
int set_hold(skm_sample_set *s, std::unique_lock<std::mutex> &hold)
{
    hold = std::unique_lock<std::mutex>(s->mu);
    s->flush++;
    s->work_cv.notify_all();
    s->done_cv.wait(hold, [&] { return !s->busy && s->queue.empty(); });
    s->flush--;
    if (s->error != SKM_OK) { set_message(s->error_msg); return s->error; }
    return SKM_OK;
}

// wait until everything added has been mapped; the set's failure, if it has one
int set_wait(skm_sample_set *s)
{
    std::unique_lock<std::mutex> hold;
    return set_hold(s, hold);
}

// (s->mu held) a sample has units: the set's modes can no longer change
bool set_has_units(const skm_sample_set *s)
{
    for (const int64_t units : s->sample_units)
        if (units) return true;
    return false;
}

// rows [0, n_samples) of `width` words of a buffer kept by sample, on the mapper's stream (s->mu held, m->mu taken here)
int set_download_rows(skm_sample_set *s, const DBuf<unsigned long long> &buf, int64_t width, int64_t n_samples, int64_t *out)
{
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // (a sample that no launch has held -- no units -- may lie past the buffer: its row is zero)
    const int64_t rows = std::min<int64_t>(n_samples, (int64_t)buf.cap / width);
    std::fill(out + rows * width, out + n_samples * width, (int64_t)0);
    if (rows) {
        HIP_TRY(hipMemcpyAsync(out, buf.p, (size_t)(rows * width) * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    return SKM_OK;
}

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

int set_view(skm_sample_set *s, std::unique_lock<std::mutex> &hold)
{
    SKM_TRY(set_hold(s, hold));
    if (s->view.valid) return SKM_OK;
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used, n_samples = (int64_t)s->sample_units.size();
    const int64_t n_log = (int64_t)s->log.global.size();
    skm_sample_set::View &v = s->view;
    v.start.assign(C, 0); v.len.assign(C, 0); v.count.assign(C, 0); v.local.assign(C, 0); v.order.assign(C, 0);
    v.arena.assign((size_t)std::max<int64_t>(M, 1), 0);
    v.sample_class_offsets.assign(n_samples + 1, 0);
    v.sample_rows.assign(n_samples, 0); v.sample_aligned.assign(n_samples, 0);
    v.units = s->sample_units;
    v.removed.assign(n_samples, 0);
    int64_t removed_total = 0;
    if (s->umi_bases && s->umi_removed.cap && n_samples) {      // (a sample that no launch has held may lie past the rows)
        const int64_t rows = std::min<int64_t>(n_samples, (int64_t)s->umi_removed.cap);
        HIP_TRY(hipMemcpyAsync(v.removed.data(), s->umi_removed.p, (size_t)rows * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        for (int64_t i = 0; i < n_samples; ++i) {
            if (v.removed[i] < 0 || v.removed[i] > v.units[i])
                return fail(SKM_ERR_STATE, "sample %lld: %lld of %lld units removed", (long long)i, (long long)v.removed[i], (long long)v.units[i]);
            v.units[i] -= v.removed[i];               // a removed unit was never in the files
            removed_total += v.removed[i];
        }
    }
    std::vector<int32_t> cls_sample(C);
    if (C) {
        if (n_log == 0) return fail(SKM_ERR_STATE, "classes without a launch");
        DBuf<int64_t> &d_off = v.d_start, &d_len = v.d_len; DBuf<double> &d_cnt = v.d_count; DBuf<int32_t> &d_sample = v.d_sample;
        DBuf<int64_t> d_local, d_log; DBuf<unsigned long long> d_fs; DBuf<int32_t> d_log_sample;
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
        SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
        SKM_TRY(d_sample.ensure(C)); SKM_TRY(d_local.ensure(C)); SKM_TRY(d_log.ensure(2 * n_log)); SKM_TRY(d_log_sample.ensure(n_log));
        HIP_TRY(hipMemcpyAsync(d_log.p, s->log.global.data(), n_log * 8, hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(d_log.p + n_log, s->log.local.data(), n_log * 8, hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(d_log_sample.p, s->log.sample.data(), n_log * 4, hipMemcpyHostToDevice, m->stream));
        launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
        launch_sample_assign(d_log.p, d_log.p + n_log, d_log_sample.p, n_log, d_fs.p, C, d_sample.p, d_local.p, m->stream);
        HIP_TRY(hipGetLastError());
        std::vector<double> cnt(C);
        HIP_TRY(hipMemcpyAsync(v.start.data(), d_off.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(v.len.data(), d_len.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(cls_sample.data(), d_sample.p, C * 4, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(v.local.data(), d_local.p, C * 8, hipMemcpyDeviceToHost, m->stream));
        if (M) HIP_TRY(hipMemcpyAsync(v.arena.data(), m->arena.p, (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        drain.dismiss();
        for (int64_t k = 0; k < C; ++k) {
            if (cls_sample[k] < 0 || cls_sample[k] >= n_samples || v.start[k] < 0)
                return fail(SKM_ERR_STATE, "class %lld of the shared table belongs to no sample", (long long)k);
            v.count[k] = (int64_t)cnt[k];
            v.sample_rows[cls_sample[k]] += v.len[k];
            v.sample_aligned[cls_sample[k]] += v.count[k];
        }
    }
    set_split_order(n_samples, C, cls_sample.data(), v.local.data(), v.order.data(), v.sample_class_offsets.data());
    // (units_s - aligned_s is each sample's unaligned count; their sum is what the table counted -- less the units
    // that UMI collapse removed, which reached class counting looking unaligned)
    int64_t unaligned = 0;
    for (int64_t i = 0; i < n_samples; ++i) {
        if (v.sample_aligned[i] > v.units[i]) return fail(SKM_ERR_STATE, "sample %lld counts more units than it has", (long long)i);
        unaligned += v.units[i] - v.sample_aligned[i];
    }
    if (m->host_totals_valid && unaligned != (int64_t)m->host_unaligned - removed_total)
        return fail(SKM_ERR_STATE, "the samples' unaligned units (%lld) are not the table's (%llu less %lld removed)", (long long)unaligned,
                    m->host_unaligned, (long long)removed_total);
    v.valid = true;
    return SKM_OK;
}

}  // namespace abi
}  // namespace skm

skm_sample_set::~skm_sample_set()
{
    (void)hipSetDevice(m->ix->device);
    if (worker_started) {
        { std::lock_guard<std::mutex> hold(mu); stop = true; }
        work_cv.notify_all();
        worker.join();                     // (finishes the launch under way; what waits is dropped)
    }
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
}

extern "C" int skm_sample_set_create(skm_index *ix, int paired, skm_sample_set **out)
{
    if (!ix || !out) return fail(SKM_ERR_ARG, "NULL argument");
    skm_mapper *mapper = nullptr;
    SKM_TRY(skm_mapper_create(ix, &mapper));
    std::unique_ptr<skm_sample_set> s(new skm_sample_set(mapper, paired ? 1 : 0));
    HIP_TRY(hipStreamCreateWithFlags(s->copy_stream.out(), hipStreamNonBlocking));
    if (const char *v = getenv("SKM_SAMPLE_SET_MAX_UNITS"))
        if (atoll(v) > 0) s->max_units = std::min<int64_t>(atoll(v), PACKED_MAX_UNITS);
    if (const char *v = getenv("SKM_TEST_UMI_SLOTS")) {          // test hook: a molecule set that has to grow under a launch
        const long long n = atoll(v);
        if (n < 2 || n > (1LL << 30) || (n & (n - 1)))
            return fail(SKM_ERR_ARG, "SKM_TEST_UMI_SLOTS must be a power of two from 2 to 2^30, not '%s'", v);
        s->umi_test_slots = (uint64_t)n;
    }
    *out = s.release();
    return SKM_OK;
}

extern "C" int skm_sample_set_destroy(skm_sample_set *s)
{
    delete s;
    return SKM_OK;
}

extern "C" int skm_sample_set_set_strand(skm_sample_set *s, int mode)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    {
        std::lock_guard<std::mutex> hold(s->mu);
        if (set_has_units(s)) return fail(SKM_ERR_STATE, "the strand mode can only change on an empty sample set");
    }
    return skm_mapper_set_strand(s->m, mode);
}

extern "C" int skm_sample_set_set_length_weights(skm_sample_set *s, const double *p)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    return skm_mapper_set_length_weights(s->m, p);
}

extern "C" int skm_sample_set_keep_histograms(skm_sample_set *s, int enable)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::lock_guard<std::mutex> hold(s->mu);
    if (set_has_units(s)) return fail(SKM_ERR_STATE, "histograms per sample can only be switched on an empty sample set");
    if (!enable && s->umi_bases) return fail(SKM_ERR_STATE, "a set that keeps UMIs keeps its histograms per sample");
    SKM_TRY(skm_mapper_keep_spans(s->m, enable));
    s->keep_hist = enable != 0;
    return SKM_OK;
}

extern "C" int skm_sample_set_keep_bias(skm_sample_set *s, int enable)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::lock_guard<std::mutex> hold(s->mu);
    if (set_has_units(s)) return fail(SKM_ERR_STATE, "hexamer counts per sample can only be switched on an empty sample set");
    s->keep_bias = enable != 0;
    return SKM_OK;
}

extern "C" int skm_sample_set_keep_umis(skm_sample_set *s, int umi_bases)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    if (umi_bases < 0 || umi_bases > 16) return fail(SKM_ERR_ARG, "UMIs of %d bases: 1 to 16 are possible (0: none)", umi_bases);
    std::lock_guard<std::mutex> hold(s->mu);
    if (!s->sample_units.empty()) return fail(SKM_ERR_STATE, "UMIs can only be switched before the set's first segment");
    if (umi_bases && !s->keep_hist)
        return fail(SKM_ERR_STATE, "a set that keeps UMIs keeps a histogram per sample: call skm_sample_set_keep_histograms(set, 1) "
                    "first (the pooled histogram is counted inside the map kernel and cannot leave a unit out)");
    s->umi_bases = umi_bases;
    if (!umi_bases) s->umi_mismatches = 0;
    return SKM_OK;
}

extern "C" int skm_sample_set_set_umi_mismatches(skm_sample_set *s, int mismatches)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    if (mismatches != 0 && mismatches != 1) return fail(SKM_ERR_ARG, "%d UMI mismatches: 0 or 1 are possible", mismatches);
    std::lock_guard<std::mutex> hold(s->mu);
    if (!s->umi_bases) return fail(SKM_ERR_STATE, "the set keeps no UMIs: call skm_sample_set_keep_umis first");
    if (!s->sample_units.empty()) return fail(SKM_ERR_STATE, "UMI mismatches can only be switched before the set's first segment");
    s->umi_mismatches = mismatches;
    return SKM_OK;
}

namespace {

int set_umi_bases(skm_sample_set *s)
{
    std::lock_guard<std::mutex> hold(s->mu);
    return s->umi_bases;
}

int set_add_packed(skm_sample_set *s, int64_t sample, int64_t first_unit, const skm_packed_reads *mate1,
                   const skm_packed_reads *mate2, const uint32_t *umis)
{
    if ((mate2 != nullptr) != (s->paired != 0)) return fail(SKM_ERR_ARG, "a %s set takes %s", s->paired ? "paired" : "single-ended",
                                                           s->paired ? "both mates" : "mate 1 alone");
    const int64_t n = mate1->n_reads;
    if (mate2 && mate2->n_reads != n) return fail(SKM_ERR_ARG, "%lld reads of mate 1, %lld of mate 2", (long long)n, (long long)mate2->n_reads);
    SKM_TRY(set_admit(s, sample, first_unit, n));
    auto data = std::make_shared<SetChunk>();
    if (n) {
        const skm_packed_reads *mates[2] = {mate1, mate2};
        for (int k = 0; k < (s->paired ? 2 : 1); ++k) SKM_TRY(packed_check_arrays(mates[k]));
        std::lock_guard<std::mutex> copying(s->copy_mu);
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(s->copy_stream); });   // (the caller's arrays, the blocks)
        for (int k = 0; k < (s->paired ? 2 : 1); ++k) {
            skm_packed_reads piece = *mates[k];
            piece.first_read = first_unit;             // (numbered by the sample's units)
            PackedPiece held;
            SKM_TRY(packed_upload(&piece, s->bytes, s->copy_stream, &held));
            data->pieces[k].push_back(std::move(held));
        }
        if (umis) {                                    // the UMIs go with the chunk
            std::shared_ptr<char> block;
            SKM_TRY(packed_block((int64_t)packed_round((size_t)n * 4), s->bytes, &block));
            data->umis = std::shared_ptr<uint32_t>(block, (uint32_t *)block.get());
            data->umi_origin = first_unit;
            HIP_TRY(hipMemcpyAsync(block.get(), umis, (size_t)n * 4, hipMemcpyHostToDevice, s->copy_stream));
        }
        drain.dismiss();
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    return set_enqueue(s, sample, first_unit, n, std::move(data));
}

}  // namespace

extern "C" int skm_sample_set_add_packed(skm_sample_set *s, int64_t sample, int64_t first_unit,
                                         const skm_packed_reads *mate1, const skm_packed_reads *mate2)
{
    if (!s || !mate1) return fail(SKM_ERR_ARG, "NULL argument");
    if (set_umi_bases(s)) return fail(SKM_ERR_ARG, "a set that keeps UMIs takes its reads with them: skm_sample_set_add_packed_umis");
    return set_add_packed(s, sample, first_unit, mate1, mate2, nullptr);
}

extern "C" int skm_sample_set_add_packed_umis(skm_sample_set *s, int64_t sample, int64_t first_unit, const skm_packed_reads *mate1,
                                              const skm_packed_reads *mate2, const uint32_t *umis)
{
    if (!s || !mate1) return fail(SKM_ERR_ARG, "NULL argument");
    const int umi_bases = set_umi_bases(s);
    if (!umi_bases) return fail(SKM_ERR_ARG, "the set keeps no UMIs: call skm_sample_set_keep_umis before the first segment");
    if (mate1->n_reads > 0 && !umis) return fail(SKM_ERR_ARG, "NULL UMIs");
    if (umi_bases < 16)
        for (int64_t u = 0; u < mate1->n_reads; ++u)
            if (umis[u] >> (2 * umi_bases)) return fail(SKM_ERR_ARG, "UMI %lld (%u) does not fit %d bases", (long long)u, umis[u], umi_bases);
    return set_add_packed(s, sample, first_unit, mate1, mate2, mate1->n_reads > 0 ? umis : nullptr);
}

extern "C" int skm_sample_set_add_batch(skm_sample_set *s, int64_t sample, int64_t first_unit, const char *bases,
                                        const int64_t *offsets, int64_t n_units)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    if (set_umi_bases(s)) return fail(SKM_ERR_ARG, "a set that keeps UMIs takes its reads with them: skm_sample_set_add_packed_umis");
    if (n_units > 0 && (!bases || !offsets)) return fail(SKM_ERR_ARG, "NULL reads");
    SKM_TRY(set_admit(s, sample, first_unit, n_units));
    auto data = std::make_shared<SetChunk>();
    if (n_units) {
        const int64_t n_reads = s->paired ? 2 * n_units : n_units;
        int64_t longest = 0;
        for (int64_t r = 0; r < n_reads; ++r) {
            if (offsets[r + 1] < offsets[r]) return fail(SKM_ERR_ARG, "offsets are not monotone");
            longest = std::max(longest, offsets[r + 1] - offsets[r]);
        }
        if (longest > (1 << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
        const int64_t n_bytes = offsets[n_reads] - offsets[0];
        const size_t offsets_bytes = packed_round((size_t)(n_reads + 1) * 8);
        const int64_t block_bytes = (int64_t)(offsets_bytes + (size_t)n_bytes + 64);     // (the pack kernel reads 32 bytes at a time)
        SKM_TRY(packed_block(block_bytes, s->bytes, &data->ascii));
        char *raw = data->ascii.get();
        data->offsets = (const int64_t *)raw;
        data->bases = (const uint8_t *)raw + offsets_bytes - offsets[0];
        data->origin = first_unit;
        data->max_len = (int)longest;
        std::lock_guard<std::mutex> copying(s->copy_mu);
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(s->copy_stream); });
        HIP_TRY(hipMemcpyAsync(raw, offsets, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, s->copy_stream));
        if (n_bytes)
            HIP_TRY(hipMemcpyAsync(raw + offsets_bytes, bases + offsets[0], (size_t)n_bytes, hipMemcpyHostToDevice, s->copy_stream));
        drain.dismiss();
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    }
    return set_enqueue(s, sample, first_unit, n_units, std::move(data));
}

extern "C" int skm_sample_set_sync(skm_sample_set *s)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    return set_wait(s);
}

extern "C" int skm_sample_set_map_relaunches(skm_sample_set *s, int64_t *count)
{
    if (!s || !count) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_wait(s));
    return skm_mapper_map_relaunches(s->m, count);
}

extern "C" int skm_sample_set_summary(skm_sample_set *s, int64_t cap_samples, int64_t *n_samples, int64_t *summary)
{
    if (!s || !n_samples || cap_samples < 0 || (cap_samples && !summary)) return fail(SKM_ERR_ARG, "bad argument");
    if (cap_samples == 0) {                               // (the number alone: nothing is waited for)
        std::lock_guard<std::mutex> counting(s->mu);
        *n_samples = (int64_t)s->sample_units.size();
        return SKM_OK;
    }
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    *n_samples = (int64_t)v.units.size();
    for (int64_t i = 0; i < std::min(cap_samples, *n_samples); ++i) {
        summary[4 * i + 0] = v.sample_class_offsets[i + 1] - v.sample_class_offsets[i];
        summary[4 * i + 1] = v.sample_rows[i];
        summary[4 * i + 2] = v.units[i] - v.sample_aligned[i];
        summary[4 * i + 3] = v.units[i];
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_export(skm_sample_set *s, int64_t *sample_class_offsets, int64_t *class_offsets,
                                     int32_t *class_targets, int64_t *class_counts, int64_t *first_seen)
{
    if (!s) return fail(SKM_ERR_ARG, "NULL sample set");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    if (sample_class_offsets) std::copy(v.sample_class_offsets.begin(), v.sample_class_offsets.end(), sample_class_offsets);
    if (class_offsets) class_offsets[0] = 0;
    int64_t pos = 0;
    for (size_t k = 0; k < v.order.size(); ++k) {
        const int64_t c = v.order[k];
        if (class_targets) memcpy(class_targets + pos, v.arena.data() + v.start[c], (size_t)v.len[c] * 4);
        pos += v.len[c];
        if (class_offsets) class_offsets[k + 1] = pos;
        if (class_counts) class_counts[k] = v.count[c];
        if (first_seen) first_seen[k] = v.local[c];
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_histogram(skm_sample_set *s, int64_t *fld)
{
    if (!s || !fld) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_wait(s));
    return skm_mapper_export(s->m, nullptr, nullptr, nullptr, nullptr, fld);
}

extern "C" int skm_sample_set_histograms(skm_sample_set *s, int64_t cap_samples, int64_t *fld)
{
    if (!s || cap_samples < 0 || (cap_samples && !fld)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_hold(s, hold));
    if (!s->keep_hist)
        return fail(SKM_ERR_STATE, "the set keeps no histogram per sample: call skm_sample_set_keep_histograms(set, 1) before adding");
    const int64_t n_samples = (int64_t)s->sample_units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    return set_download_rows(s, s->hist, MAX_FRAGMENT_LENGTH, n_samples, fld);
}

extern "C" int skm_sample_set_bias_observed(skm_sample_set *s, int64_t cap_samples, int64_t *out)
{
    if (!s || cap_samples < 0 || (cap_samples && !out)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_hold(s, hold));
    if (!s->keep_bias)
        return fail(SKM_ERR_STATE, "the set does not count hexamers: call skm_sample_set_keep_bias(set, 1) before adding");
    const int64_t n_samples = (int64_t)s->sample_units.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    if (n_samples == 0) return SKM_OK;
    return set_download_rows(s, s->bias_rows, BIAS_BINS, n_samples, out);
}

extern "C" int skm_sample_set_umi_removed(skm_sample_set *s, int64_t cap_samples, int64_t *removed)
{
    if (!s || cap_samples < 0 || (cap_samples && !removed)) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    const int64_t n_samples = (int64_t)v.removed.size();
    if (cap_samples < n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)n_samples);
    std::copy(v.removed.begin(), v.removed.end(), removed);
    return SKM_OK;
}

extern "C" int skm_sample_set_umi_near_removed(skm_sample_set *s, int64_t *n)
{
    if (!s || !n) return fail(SKM_ERR_ARG, "bad argument");
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_hold(s, hold));                   // (every launch has read its counters back)
    std::lock_guard<std::mutex> lock(s->m->mu);
    *n = s->umi_near;
    return SKM_OK;
}

extern "C" int skm_sample_set_plan(int64_t n_segments, const int32_t *sample, const int64_t *n_units, int64_t max_units,
                                   int64_t cap_entries, int64_t *n_entries, int64_t *entry_global, int64_t *entry_local,
                                   int32_t *entry_sample)
{
    if (n_segments < 0 || max_units < 1 || cap_entries < 0 || !n_entries || (n_segments && (!sample || !n_units)))
        return fail(SKM_ERR_ARG, "bad argument");
    std::deque<SetQueued> queue;
    std::unordered_map<int32_t, int64_t> next;
    for (int64_t i = 0; i < n_segments; ++i) {
        if (sample[i] < 0 || n_units[i] < 0) return fail(SKM_ERR_ARG, "bad segment %lld", (long long)i);
        if (n_units[i]) queue.push_back(SetQueued{sample[i], next[sample[i]], n_units[i], nullptr});
        next[sample[i]] += n_units[i];
    }
    SetLog log;
    std::vector<SetPart> parts;
    while (!queue.empty()) {
        set_cut_launch(queue, max_units, &parts);
        log.append(parts);
    }
    *n_entries = (int64_t)log.global.size();
    if (*n_entries > cap_entries) return SKM_OK;       // (the caller sizes its arrays and asks again)
    if (*n_entries && (!entry_global || !entry_local || !entry_sample)) return fail(SKM_ERR_ARG, "NULL entry arrays");
    std::copy(log.global.begin(), log.global.end(), entry_global);
    std::copy(log.local.begin(), log.local.end(), entry_local);
    std::copy(log.sample.begin(), log.sample.end(), entry_sample);
    return SKM_OK;
}

extern "C" int skm_sample_set_split(int64_t n_entries, const int64_t *entry_global, const int64_t *entry_local,
                                    const int32_t *entry_sample, int64_t n_samples, int64_t n_classes,
                                    const int64_t *first_seen, int32_t *class_sample, int64_t *class_local, int64_t *order,
                                    int64_t *sample_class_offsets)
{
    if (n_entries < 0 || n_samples < 0 || n_classes < 0 || !sample_class_offsets
            || (n_entries && (!entry_global || !entry_local || !entry_sample))
            || (n_classes && (!first_seen || !class_sample || !class_local || !order)))
        return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (n_entries == 0 || entry_global[0] != 0)) return fail(SKM_ERR_ARG, "the log does not start at unit 0");
    for (int64_t i = 0; i < n_entries; ++i)
        if (entry_sample[i] < 0 || entry_sample[i] >= n_samples || (i && entry_global[i] <= entry_global[i - 1]))
            return fail(SKM_ERR_ARG, "bad log entry %lld", (long long)i);
    for (int64_t k = 0; k < n_classes; ++k) {
        if (first_seen[k] < 0) return fail(SKM_ERR_ARG, "negative first-seen unit");
        const int64_t e = segment_find(entry_global, n_entries, first_seen[k]);
        class_sample[k] = entry_sample[e];
        class_local[k] = entry_local[e] + (first_seen[k] - entry_global[e]);
    }
    set_split_order(n_samples, n_classes, class_sample, class_local, order, sample_class_offsets);
    return SKM_OK;
}
