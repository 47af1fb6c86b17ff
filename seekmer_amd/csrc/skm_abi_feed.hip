// C ABI of libseekmer_hip.so (declared in include/seekmer_hip.h): the mapper's feed -- how reads reach the
// map/class stage of skm_abi.hip.  The staging lanes of the host batches, the packed pieces (their book-keeping
// is skm_packed_book.h) and the one worker that maps both through map_batch_resident.  Everything here runs
// under skm_mapper::feed.q_mu; the worker takes `mu` for the batch or run it maps, and for nothing else.
#include "skm_abi_mapper.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace skm;
using namespace skm::abi;

namespace {

// ---- host batches: staging lanes and the mapping worker --------------------------------
int run_job(skm_mapper *m, const skm_mapper::Job &job)
{
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    skm_mapper::Lane &lane = m->feed.lanes[job.lane];
    const int64_t n_reads = job.paired ? 2 * job.n_units : job.n_units;
    // longest read and monotonicity from the offsets in HBM (the lane's copy is complete)
    SKM_TRY(m->feed.scan_out.ensure(2));
    HIP_TRY(hipMemsetAsync(m->feed.scan_out.p, 0, 16, m->stream));
    launch_offsets_scan(lane.offsets.p, n_reads, job.offset_base, m->feed.scan_out.p, m->stream);   // (and rebases them to 0)
    HIP_TRY(hipGetLastError());
    unsigned long long *scan = m->pinned + 40;
    HIP_TRY(hipMemcpyAsync(scan, m->feed.scan_out.p, 16, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (scan[1]) return fail(SKM_ERR_ARG, "offsets are not monotone (%llu descents)", scan[1]);
    if (scan[0] > (1ULL << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
    return map_batch_resident(m, lane.bases.p, lane.offsets.p, job.n_units, job.paired, (int)scan[0],
                              job.first_unit);
}

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// ---- packed pieces ----------------------------------------------------------------------

// the read records of a launch's packed segments (`first_unit`: the unit that stands at record 0)
void packed_unpack(const std::vector<PackedSegment> &segments, int64_t first_unit, int mates, uint32_t *records, int words,
                   int record_words, int *error, hipStream_t stream)
{
    for (const PackedSegment &seg : segments) {
        uint32_t *dst = records + ((seg.first - first_unit) * mates + seg.mate) * (int64_t)record_words;
        launch_unpack_reads(seg.codes, seg.cw, seg.cw, seg.lengths, seg.uniform_len, seg.n, words, dst,
                            (int64_t)mates * record_words, error, stream);
        if (seg.n_exc)
            launch_unpack_exceptions(seg.exc_reads, seg.exc_masks, seg.n_exc, seg.cw, seg.exc_base, words, dst,
                                     (int64_t)mates * record_words, stream);
    }
}

}  // namespace abi
}  // namespace skm

namespace {

int run_packed_job(skm_mapper *m, int64_t lo, int64_t hi, int paired, const std::vector<PackedSegment> &segments,
                   int max_cw)
{
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int mates = paired ? 2 : 1;
    if (!m->packed_sized && m->expected_units > 0) {
        // Runs grow with what has arrived (a few ten thousand units, then hundreds of thousands, then
        // PACKED_MAX_UNITS): sized run by run, every batch buffer is allocated three or four times in
        // a sample's first milliseconds.  Size them for the largest run of the announced sample once.
        const int64_t most = std::max<int64_t>(hi - lo, std::min(m->expected_units, PACKED_MAX_UNITS));
        const int words = max_cw + 1, record_words = ((3 * words + 1 + 15) / 16) * 16;
        SKM_TRY(m->records.ensure((size_t)most * mates * record_words + 16));
        SKM_TRY(m->rec_unit.ensure(most)); SKM_TRY(m->rec_tuple.ensure(most));
        SKM_TRY(m->unit_slot.ensure(most)); SKM_TRY(m->rec_key.ensure(most));
        SKM_TRY(m->unit_entries.ensure((size_t)most * 8 + (size_t)m->ix->cu_count * MAP_BLOCKS_PER_CU * (MAP_THREADS / 64) * 2048 + 4096));
        if (m->host_classes == 0) SKM_TRY(table_reserve_for_sample(m, m->expected_units));
        m->packed_sized = true;
    }
    const RecordStage fill = [&](uint32_t *records, int words, int record_words) -> int {
        packed_unpack(segments, lo, mates, records, words, record_words, m->error.p, m->stream);
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    return map_batch_resident(m, nullptr, nullptr, hi - lo, paired, max_cw * 32, lo, &fill);
}

void worker_main(skm_mapper *m)
{
    skm_mapper::Feed &f = m->feed;
    for (;;) {
        skm_mapper::Job job;
        bool packed = false;
        int64_t lo = 0, hi = 0;
        int paired = 0, max_cw = 1;
        std::vector<PackedSegment> segments;
        {
            std::unique_lock<std::mutex> hold(f.q_mu);
            for (;;) {
                if (!f.jobs.empty()) break;
                if (f.job_error != SKM_OK && !f.book.empty()) {
                    f.book.drop_all();          // after a failure the table is not to be trusted
                    f.done_cv.notify_all();
                }
                // (a pusher that waits at the byte limit may be the only one who could make the run
                // longer: its presence maps whatever run there is, as a flush does)
                if (f.book.find_run(&lo, &hi)
                        && (hi - lo >= PACKED_MIN_UNITS || f.packed_flush || f.packed_waiters || f.stop)) {
                    packed = true;
                    break;
                }
                if (f.stop) {                   // stop requested and nothing left to map
                    f.book.drop_all();
                    return;
                }
                f.q_cv.wait(hold);
            }
            if (!packed) {
                job = f.jobs.front();
                f.jobs.pop_front();
            } else {
                paired = f.book.paired == 1;
                for (int s = 0; s < (paired ? 2 : 1); ++s)
                    f.book.segments(s, lo, hi, true, &segments, &max_cw);
                f.packed_busy = true;
            }
        }
        int rc = SKM_OK;
        std::string message;
        if (packed) {
            rc = run_packed_job(m, lo, hi, paired, segments, max_cw);
            if (rc != SKM_OK) {
                message = last_message();
                // kernels that read the pieces' blocks may still be queued: nothing is handed back
                // to the pool (and from there to the next pusher's copy) before the stream has drained
                (void)hipStreamSynchronize(m->stream);
            }
            {
                std::lock_guard<std::mutex> hold(f.q_mu);
                f.record_failure(rc, 0, message);         // (reported by every wait)
                for (int s = 0; s < (paired ? 2 : 1); ++s) f.book.consume(s, lo, hi);
                f.packed_busy = false;
            }
            f.done_cv.notify_all();
            continue;
        }
        bool skip;
        {
            std::lock_guard<std::mutex> hold(f.q_mu);
            skip = f.job_error != SKM_OK;         // after a failure the table is not to be trusted
        }
        if (!skip) {
            rc = run_job(m, job);
            if (rc != SKM_OK) message = last_message();  // (this thread's message)
        }
        {
            std::lock_guard<std::mutex> hold(f.q_mu);
            f.record_failure(rc, job.ticket, message);
            f.lanes[job.lane].busy = false;
            f.done_ticket = job.ticket;
        }
        f.done_cv.notify_all();
    }
}

// (q_mu held) the worker starts with the first batch or piece
void ensure_worker(skm_mapper *m)
{
    if (m->feed.worker_started) return;
    m->feed.worker = std::thread(worker_main, m);
    m->feed.worker_started = true;
}

}  // namespace

void skm_mapper::Feed::record_failure(int rc, uint64_t ticket, const std::string &message)
{
    if (rc == SKM_OK || job_error != SKM_OK) return;
    job_error = rc;
    job_error_ticket = ticket;
    job_error_msg = message;
}

void skm_mapper::Feed::shutdown()
{
    if (!worker_started) return;
    { std::lock_guard<std::mutex> hold(q_mu); stop = true; }
    q_cv.notify_all();
    worker.join();                     // (finishes what is queued)
}

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// wait until every queued batch up to `ticket` has been mapped (0 = all of them AND every packed
// read whose mate has arrived; reads still without one keep waiting in HBM -- another thread may be
// about to push their mates -- until skm_mapper_reset / _clear / _destroy); reports (and, with
// `consume`, forgets) the first failure among them
int wait_jobs(skm_mapper *m, uint64_t ticket, bool consume)
{
    skm_mapper::Feed &f = m->feed;
    std::unique_lock<std::mutex> hold(f.q_mu);
    const uint64_t upto = ticket ? ticket : f.next_ticket - 1;
    f.done_cv.wait(hold, [&] { return f.done_ticket >= upto; });
    if (ticket == 0 && (f.packed_busy || !f.book.empty())) {
        f.packed_flush++;
        f.q_cv.notify_all();
        f.done_cv.wait(hold, [&] {
            int64_t lo, hi;
            return !f.packed_busy && (f.job_error != SKM_OK || !f.book.find_run(&lo, &hi));
        });
        f.packed_flush--;
    }
    if (f.job_error != SKM_OK && f.job_error_ticket <= upto) {
        const int rc = f.job_error;
        const std::string message = f.job_error_msg;
        if (consume) { f.job_error = SKM_OK; f.job_error_ticket = 0; f.job_error_msg.clear(); }
        set_message(message);
        return rc;
    }
    return SKM_OK;
}

}  // namespace abi
}  // namespace skm

namespace {

// offsets == nullptr: every read is `uniform_len` bases long (the offsets are then made on the device)
int submit_batch(skm_mapper *m, const char *bases, const int64_t *offsets, int64_t uniform_len, int64_t n_units,
                 int paired, int64_t first_unit, uint64_t *ticket_out)
{
    if (!m || n_units < 0 || (!offsets && uniform_len < 0)) return fail(SKM_ERR_ARG, "bad argument");
    if (n_units > 0 && !bases) return fail(SKM_ERR_ARG, "bases is NULL");
    if (n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "more than 2^31 - 1 units in one batch");
    if (!offsets && uniform_len > (1 << 20)) return fail(SKM_ERR_ARG, "read longer than 2^20 bases");
    SKM_TRY(set_device(m->ix->device));
    skm_mapper::Feed &f = m->feed;
    const int64_t n_reads = paired ? 2 * n_units : n_units;
    const int64_t first_byte = offsets ? offsets[0] : 0;
    const int64_t n_bytes = offsets ? offsets[n_reads] - offsets[0] : n_reads * uniform_len;
    if (n_bytes < 0) return fail(SKM_ERR_ARG, "offsets are not monotone");
    // a free lane (at most N_LANES batches are in HBM at a time: one being mapped, others copied)
    int li = -1;
    {
        std::unique_lock<std::mutex> hold(f.q_mu);
        ensure_worker(m);
        f.done_cv.wait(hold, [&] {
            for (int i = 0; i < skm_mapper::N_LANES; ++i) if (!f.lanes[i].busy) { li = i; return true; }
            return false;
        });
        f.lanes[li].busy = true;
    }
    skm_mapper::Lane &lane = f.lanes[li];
    auto release = on_exit([&]() {
        { std::lock_guard<std::mutex> hold(f.q_mu); lane.busy = false; }
        f.done_cv.notify_all();
    });
    if (!lane.stream) HIP_TRY(hipStreamCreateWithFlags(lane.stream.out(), hipStreamNonBlocking));
    SKM_TRY(lane.bases.ensure((size_t)n_bytes + 64));
    SKM_TRY(lane.offsets.ensure((size_t)n_reads + 1));
    // pinned sources go over the link at full rate and asynchronously; pageable ones are staged
    // by the runtime.  Either way the source is free again when this call returns.
    if (n_bytes)
        HIP_TRY(hipMemcpyAsync(lane.bases.p, bases + first_byte, (size_t)n_bytes, hipMemcpyHostToDevice, lane.stream));
    if (offsets)
        HIP_TRY(hipMemcpyAsync(lane.offsets.p, offsets, (size_t)(n_reads + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                               lane.stream));
    else
        launch_offsets_uniform(lane.offsets.p, n_reads, uniform_len, lane.stream);
    HIP_TRY(hipStreamSynchronize(lane.stream));
    uint64_t ticket;
    {
        std::lock_guard<std::mutex> hold(f.q_mu);
        ticket = f.next_ticket++;
        f.jobs.push_back(skm_mapper::Job{li, n_units, paired, first_byte, first_unit, ticket});
    }
    release.dismiss();
    f.q_cv.notify_one();
    if (ticket_out) *ticket_out = ticket;
    return SKM_OK;
}

}  // namespace

extern "C" int skm_mapper_map_batch_async(skm_mapper *m, const char *bases, const int64_t *offsets,
                                          int64_t n_units, int paired, int64_t first_unit)
{
    if (!offsets) return fail(SKM_ERR_ARG, "offsets is NULL");
    return submit_batch(m, bases, offsets, -1, n_units, paired, first_unit, nullptr);
}

extern "C" int skm_mapper_map_batch_uniform_async(skm_mapper *m, const char *bases, int32_t read_len,
                                                  int64_t n_units, int paired, int64_t first_unit)
{
    if (read_len < 0) return fail(SKM_ERR_ARG, "negative read length");
    return submit_batch(m, bases, nullptr, read_len, n_units, paired, first_unit, nullptr);
}

extern "C" int skm_mapper_map_batch(skm_mapper *m, const char *bases, const int64_t *offsets,
                                    int64_t n_units, int paired)
{
    uint64_t ticket = 0;
    if (!offsets) return fail(SKM_ERR_ARG, "offsets is NULL");
    SKM_TRY(submit_batch(m, bases, offsets, -1, n_units, paired, -1, &ticket));
    return wait_jobs(m, ticket, true);
}

extern "C" int skm_mapper_expect_units(skm_mapper *m, int64_t n_units)
{
    if (!m || n_units < 0) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lock(m->mu);          // (run_packed_job reads them under it)
    m->expected_units = n_units;
    m->packed_sized = false;
    return SKM_OK;
}

extern "C" int skm_mapper_sync(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    return wait_jobs(m, 0, true);
}

namespace {

// A piece on its way into the mapper: `stage` checks it, waits at the byte limit, takes a block of HBM
// and QUEUES the copies on the mapper's copy stream (*staged = false: a cut or an empty piece, dealt
// with on the spot); `commit` -- once the copies have completed -- makes the piece visible to the worker.
int packed_stage(skm_mapper *m, const skm_packed_reads *piece, int paired, PackedPiece *out, bool *staged);
int packed_commit(skm_mapper *m, PackedPiece &&held, int stream_index);

// A piece's one HBM block: codes | lengths | exception reads | exception bit planes
int64_t packed_block_bytes(const skm_packed_reads *piece)
{
    const size_t n = (size_t)piece->n_reads, cw = (size_t)piece->code_words, n_exc = (size_t)piece->n_exceptions;
    return (int64_t)(packed_round(n * cw * 8) + (piece->uniform_len >= 0 ? 0 : packed_round(n * 4)) + packed_round(n_exc * 4)
                     + packed_round(n_exc * cw * 4) + 256);
}

}  // namespace

extern "C" int skm_mapper_push_packed(skm_mapper *m, const skm_packed_reads *piece, int paired)
{
    if (!m || !piece) return fail(SKM_ERR_ARG, "NULL argument");
    PackedPiece held;
    bool staged = false;
    SKM_TRY(packed_stage(m, piece, paired, &held, &staged));
    if (!staged) return SKM_OK;
    HIP_TRY(hipStreamSynchronize(m->feed.packed_stream));   // (the caller's arrays are free again)
    return packed_commit(m, std::move(held), piece->stream);
}

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// the arrays of a piece that holds reads
int packed_check_arrays(const skm_packed_reads *piece)
{
    const int64_t n = piece->n_reads;
    const int cw = piece->code_words;
    if (cw < 1 || cw > (1 << 15) || piece->read_stride < cw || !piece->codes) return fail(SKM_ERR_ARG, "bad code words");
    if (piece->uniform_len < 0 && !piece->lengths) return fail(SKM_ERR_ARG, "lengths is NULL");
    if (piece->uniform_len > 32LL * cw) return fail(SKM_ERR_ARG, "reads of %lld bases in %d code words", (long long)piece->uniform_len, cw);
    const int64_t n_exc = piece->n_exceptions;
    if (n_exc < 0 || n_exc > n || (n_exc > 0 && (!piece->exception_reads || !piece->exception_masks)))
        return fail(SKM_ERR_ARG, "bad exception list");
    for (int64_t e = 0; e < n_exc; ++e)
        if (piece->exception_reads[e] >= (uint64_t)n || (e && piece->exception_reads[e] <= piece->exception_reads[e - 1]))
            return fail(SKM_ERR_ARG, "exception reads must ascend and lie inside the piece");
    return SKM_OK;
}

// `bytes` of HBM from the pool, counted in *counter while the block lives
int packed_block(int64_t bytes, const std::shared_ptr<std::atomic<int64_t>> &counter, std::shared_ptr<char> *block)
{
    char *raw = nullptr;
    HIP_TRY(pool_alloc((void **)&raw, (size_t)bytes));
    counter->fetch_add(bytes);       // (the counter outlives its owner if a block does)
    *block = std::shared_ptr<char>(raw, [counter, bytes](char *q) { pool_free(q); counter->fetch_sub(bytes); });
    return SKM_OK;
}

// take the block (counted in *counter while it lives) and QUEUE the copies of the piece's arrays on `stream`
int packed_upload(const skm_packed_reads *piece, const std::shared_ptr<std::atomic<int64_t>> &counter, hipStream_t stream,
                  PackedPiece *out)
{
    const int64_t n = piece->n_reads, n_exc = piece->n_exceptions;
    const int cw = piece->code_words;
    const bool uniform = piece->uniform_len >= 0;
    const size_t codes_bytes = packed_round((size_t)n * cw * 8);
    const size_t len_bytes = uniform ? 0 : packed_round((size_t)n * 4);
    const size_t exc_bytes = packed_round((size_t)n_exc * 4);
    PackedPiece &held = *out;
    SKM_TRY(packed_block(packed_block_bytes(piece), counter, &held.block));
    char *raw = held.block.get();
    held.first = held.origin = piece->first_read;
    held.n = n;
    held.cw = cw;
    held.uniform_len = uniform ? piece->uniform_len : -1;
    held.codes = (uint64_t *)raw;
    held.lengths = uniform ? nullptr : (uint32_t *)(raw + codes_bytes);
    held.exc_reads_dev = (uint32_t *)(raw + codes_bytes + len_bytes);
    held.exc_masks = (uint32_t *)(raw + codes_bytes + len_bytes + exc_bytes);
    if (n_exc) held.exc_reads.assign(piece->exception_reads, piece->exception_reads + n_exc);
    if (piece->read_stride == cw)
        HIP_TRY(hipMemcpyAsync(held.codes, piece->codes, (size_t)n * cw * 8, hipMemcpyHostToDevice, stream));
    else
        HIP_TRY(hipMemcpy2DAsync(held.codes, (size_t)cw * 8, piece->codes, (size_t)piece->read_stride * 8, (size_t)cw * 8,
                                 (size_t)n, hipMemcpyHostToDevice, stream));
    if (!uniform) HIP_TRY(hipMemcpyAsync(held.lengths, piece->lengths, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    if (n_exc) {
        HIP_TRY(hipMemcpyAsync(held.exc_reads_dev, piece->exception_reads, (size_t)n_exc * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(held.exc_masks, piece->exception_masks, (size_t)n_exc * cw * 4, hipMemcpyHostToDevice, stream));
    }
    return SKM_OK;
}

}  // namespace abi
}  // namespace skm

namespace {

int packed_stage(skm_mapper *m, const skm_packed_reads *piece, int paired, PackedPiece *out, bool *staged)
{
    *staged = false;
    skm_mapper::Feed &f = m->feed;
    const int64_t n = piece->n_reads;
    const int cw = piece->code_words;
    if (n < 0 || n >= (1LL << 31) || piece->first_read < 0) return fail(SKM_ERR_ARG, "bad piece: %lld reads from %lld", (long long)n, (long long)piece->first_read);
    if (piece->stream < 0 || piece->stream > (paired ? 1 : 0)) return fail(SKM_ERR_ARG, "stream %d of a %s sample", piece->stream, paired ? "paired" : "single-ended");
    if (n == 0 && cw == SKM_PACKED_CUT) {
        // a cut: the stream's reads from first_read on are dropped (the longer file of a pair of
        // files, seekmer/common.py:180-197: zip() ends at the shorter one).  The run the worker may
        // be mapping from the same piece ends where both streams had reads, i.e. at or below the cut.
        std::unique_lock<std::mutex> hold(f.q_mu);
        const int64_t from = piece->first_read;
        f.done_cv.wait(hold, [&] { return !f.packed_busy || !f.book.in_flight_from(piece->stream, from); });
        f.book.truncate(piece->stream, from, true);
        return SKM_OK;
    }
    if (n == 0) return SKM_OK;
    SKM_TRY(packed_check_arrays(piece));
    SKM_TRY(set_device(m->ix->device));
    {
        std::lock_guard<std::mutex> hold(f.q_mu);
        if (f.book.paired >= 0 && f.book.paired != (paired ? 1 : 0) && (!f.book.empty() || f.packed_busy))
            return fail(SKM_ERR_STATE, "paired and single-ended pieces in one run");
        f.book.paired = paired ? 1 : 0;
        if (!f.packed_stream) HIP_TRY(hipStreamCreateWithFlags(f.packed_stream.out(), hipStreamNonBlocking));
    }
    const int64_t block_bytes = packed_block_bytes(piece);
    {
        std::unique_lock<std::mutex> hold(f.q_mu);
        auto may_go = [&] {
            if (f.packed_bytes->load() + block_bytes <= f.packed_max_pending || f.job_error != SKM_OK) return true;
            int64_t lo, hi;
            return !(f.packed_busy || f.book.find_run(&lo, &hi));         // nothing the worker could free
        };
        if (!may_go()) {
            f.packed_waiters++;                   // the worker now maps runs below PACKED_MIN_UNITS too
            f.q_cv.notify_all();
            f.done_cv.wait(hold, may_go);
            f.packed_waiters--;
        }
    }
    SKM_TRY(packed_upload(piece, f.packed_bytes, f.packed_stream, out));
    *staged = true;
    return SKM_OK;
}

int packed_commit(skm_mapper *m, PackedPiece &&held, int stream_index)
{
    skm_mapper::Feed &f = m->feed;
    {
        std::unique_lock<std::mutex> hold(f.q_mu);
        ensure_worker(m);
        // a piece that overlaps what its stream holds replaces the reads from its first one on
        if (f.book.overlaps(stream_index, held.first, held.n)) {
            // a piece the worker is mapping from right now (the longer file of a pair of unequal
            // length: its leftover reads are what this piece replaces): the run in flight ends where
            // both streams had reads, so waiting for it leaves only the leftover to cut off -- the
            // outcome does not depend on when the worker took the run
            f.done_cv.wait(hold, [&] { return !f.packed_busy || !f.book.in_flight_from(stream_index, held.first); });
            for (const auto &other : f.book.pending[stream_index])
                if (other.first < held.first && other.first + other.n > held.first && other.in_job)
                    return fail(SKM_ERR_STATE, "a piece replaces reads that are being mapped");
        }
        f.book.insert(stream_index, std::move(held));     // (whether it still overlaps is asked again in there)
    }
    f.q_cv.notify_all();
    return SKM_OK;
}

}  // namespace

extern "C" int skm_mapper_map_packed_source(skm_mapper *m, skm_packed_source next, void *context, int paired,
                                            int64_t *n_pieces)
{
    if (!m || !next) return fail(SKM_ERR_ARG, "NULL argument");
    if (n_pieces) *n_pieces = 0;
    // The copy of piece k runs while the source is asked for piece k + 1 (a source keeps a piece's
    // arrays valid through ONE more call, include/seekmer_hip.h): the drain loop -- one thread --
    // paid every piece's copy time in full before (524 pieces x 25 us of a 42 ms pass).
    SKM_TRY(set_device(m->ix->device));
    hipEvent_t copied[2] = {nullptr, nullptr};
    PackedPiece waiting;
    bool have_waiting = false;
    auto undo = on_exit([&]() {
        // (an early return with a copy still queued: its block goes back to the pool with `waiting`)
        if (have_waiting) (void)hipStreamSynchronize(m->feed.packed_stream);
        for (auto &e : copied) pool_event_release(e, false);
    });
    for (auto &e : copied) HIP_TRY(pool_event_acquire(&e, false));
    int waiting_stream = 0, turn = 0;
    auto land = [&]() -> int {                   // the piece whose copy was queued a call ago joins its stream
        if (!have_waiting) return SKM_OK;
        have_waiting = false;
        HIP_TRY(hipEventSynchronize(copied[turn ^ 1]));
        return packed_commit(m, std::move(waiting), waiting_stream);
    };
    for (;;) {
        skm_packed_reads piece;
        memset(&piece, 0, sizeof(piece));
        const int rc = next(context, &piece);
        if (rc != SKM_OK) { (void)land(); return fail(rc, "the source of packed reads failed (%d)", rc); }
        if (piece.n_reads == 0 && piece.code_words != SKM_PACKED_CUT) return land();
        if (piece.n_reads == 0) SKM_TRY(land());         // a cut applies behind everything that came before it
        PackedPiece held;
        bool staged = false;
        const int staged_rc = packed_stage(m, &piece, paired, &held, &staged);
        if (staged_rc != SKM_OK) { (void)land(); return staged_rc; }
        if (staged) HIP_TRY(hipEventRecord(copied[turn], m->feed.packed_stream));
        SKM_TRY(land());
        if (staged) {
            waiting = std::move(held);
            waiting_stream = piece.stream;
            have_waiting = true;
            turn ^= 1;
        }
        if (n_pieces) ++*n_pieces;
    }
}
