// C ABI of libseekmer_hip.so (declared in include/seekmer_hip.h): the mapper -- its class table,
// map_batch_resident, its settings, and the calls that read, merge and clear the table: everything that runs
// under `mu`.  How reads reach it (the staging lanes and packed pieces with their worker) is skm_abi_feed.hip.
// No torch types, no exceptions across the boundary.
#include "skm_abi_mapper.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace skm;
using namespace skm::abi;

// ------------------------------------------------------------------- mapper
namespace {

void bind_table(skm_mapper *m, uint64_t n_slots)
{
    m->t.slots = m->slots.p;
    m->t.slot_mask = n_slots - 1;
    m->t.arena = m->arena.p;
    m->t.arena_capacity = (int64_t)m->arena.cap;
    m->t.arena_cursor = m->counters.p + CTR_ARENA;
    m->t.n_classes = m->counters.p + CTR_CLASSES;
    m->t.n_unaligned = m->counters.p + CTR_UNALIGNED;
    m->t.n_units = m->counters.p + CTR_UNITS;
    m->t.global_fld = m->counters.p + CTR_FLD;
    m->t.class_list = m->class_list.p;
    m->t.class_list_capacity = (int64_t)m->class_list.cap;
    m->t.n_listed = m->counters.p + CTR_LISTED;
    m->t.n_deferred = m->counters.p + CTR_DEFERRED;
    m->t.arena_committed = m->counters.p + CTR_COMMITTED;
    m->t.error = m->error.p;
}

int table_reset(skm_mapper *m, uint64_t n_slots)
{
    SKM_TRY(m->slots.ensure(n_slots));
    SKM_TRY(m->arena.ensure(1 << 20));
    SKM_TRY(m->class_list.ensure(1 << 16));
    SKM_TRY(m->counters.ensure(CTR_WORDS));
    SKM_TRY(m->error.ensure(1));
    HIP_TRY(hipMemsetAsync(m->counters.p, 0, CTR_WORDS * sizeof(unsigned long long), m->stream));
    HIP_TRY(hipMemsetAsync(m->error.p, 0, sizeof(int), m->stream));
    bind_table(m, n_slots);
    launch_class_init(m->t, m->stream);
    HIP_TRY(hipGetLastError());
    m->host_classes = 0;
    m->host_arena_used = 0;
    m->host_units = m->host_unaligned = 0;
    m->host_totals_valid = true;
    m->units_done = 0;
    m->first_seen_bound = 0;
    return SKM_OK;
}

// make the class table at least `want_slots` big (power of two), moving its
// entries; the registry (and, for a batch in flight, the unit -> slot map) is
// redirected through a forwarding array
int table_grow(skm_mapper *m, uint64_t want_slots, int64_t units_in_flight)
{
    uint64_t n_slots = m->t.slot_mask + 1;
    uint64_t need = n_slots;
    while (need < want_slots) need <<= 1;
    if (need == n_slots) return SKM_OK;
    if (units_in_flight > 0) m->deferred_grows += 1;
    DBuf<ClassSlot> new_slots;
    DBuf<int64_t> forward;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    SKM_TRY(new_slots.ensure(need));
    SKM_TRY(forward.ensure(n_slots));
    ClassTable to = m->t;
    to.slots = new_slots.p;
    to.slot_mask = need - 1;
    launch_class_init(to, m->stream);
    launch_class_rehash(m->t, to, forward.p, m->stream);
    unsigned long long listed = 0;
    HIP_TRY(hipMemcpyAsync(&listed, m->counters.p + CTR_LISTED, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    launch_slot_remap(m->class_list.p, (int64_t)listed, forward.p, m->stream);
    launch_slot_remap(m->unit_slot.p, units_in_flight, forward.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    m->slots = std::move(new_slots);
    bind_table(m, need);
    return SKM_OK;
}

// Size the table for a batch of `n_units`: classes are far fewer than units in
// practice (0.09 per pair at 10 M pairs), so reserve for one new class per 8
// units at load <= 0.5 and let the bounded probe defer the rest.
int table_reserve(skm_mapper *m, int64_t n_units)
{
    const double expect = (double)m->host_classes + (double)n_units / 8.0 + 1024.0;
    uint64_t want = 1 << 16;
    while ((double)want * 0.5 < expect) want <<= 1;
    if (!m->test_class_slots) SKM_TRY(table_grow(m, want, 0));
    // registry and arena can never need more than one entry per unit / id of the batch
    SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_units + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    return SKM_OK;
}

int read_error(skm_mapper *m)
{
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, m->error.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (err == SKM_ERR_COLLISION)
        return fail(SKM_ERR_COLLISION, "two different class tuples share a 64-bit key");
    if (err) return fail(err, "class table kernel reported error %d", err);
    return SKM_OK;
}

}  // namespace

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// What skm_mapper_expect_units announced (0: nothing): the table and the batch buffers are sized for
// it once instead of growing step by step under the first runs of a sample.
int table_reserve_for_sample(skm_mapper *m, int64_t sample_units)
{
    // (a hint, possibly a wild one: what it reserves is bounded -- 2^26 classes, 2 GB of table -- and
    // a sample that needs more grows the table as before)
    const double expect = (double)m->host_classes + (double)std::min<int64_t>(sample_units, 1LL << 29) / 8.0 + 1024.0;
    uint64_t want = 1 << 16;
    while ((double)want * 0.5 < expect && want < (1ULL << 26)) want <<= 1;
    if (!m->test_class_slots) SKM_TRY(table_grow(m, want, 0));
    SKM_TRY(m->class_list.ensure((size_t)(expect + 1024.0), true, m->stream));
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + (int64_t)(expect * 6.0) + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    return SKM_OK;
}

int map_batch_resident(skm_mapper *m, const uint8_t *d_bases, const int64_t *d_offsets,
                       int64_t n_units, int paired, int max_len, int64_t first_unit,
                       const RecordStage *fill_records, const SampleSalt *salt,
                       unsigned long long *sample_bias_rows, const BatchStage *collapse)
{
    const int64_t unit_base = first_unit >= 0 ? first_unit : m->units_done;
    skm_index *ix = m->ix;
    const int64_t n_reads = paired ? 2 * n_units : n_units;
    const int words = (max_len + 31) / 32 + 1;
    m->last_units = n_units;
    m->last_ids = 0;
    m->last_reads = 0;
    if (n_units == 0) return SKM_OK;

    const int record_words = ((3 * words + 1 + 15) / 16) * 16;      // 64-byte records
    SKM_TRY(m->records.ensure((size_t)n_reads * record_words + 16));
    m->last_reads = n_reads;
    m->last_words = words;
    m->last_record_words = record_words;
    if (n_units >= (1LL << 31)) return fail(SKM_ERR_ARG, "more than 2^31 - 1 units in one batch");
    if (m->keep_spans) {
        SKM_TRY(m->unit_begin.ensure(n_units));
        SKM_TRY(m->unit_end.ensure(n_units));
        SKM_TRY(m->unit_anchor.ensure(n_units));
    }
    m->last_spans = m->keep_spans;
    SKM_TRY(m->rec_unit.ensure(n_units));
    SKM_TRY(m->rec_tuple.ensure(n_units));
    SKM_TRY(m->unit_slot.ensure(n_units));
    SKM_TRY(m->rec_key.ensure(n_units));

    SKM_TRY(m->batch_ctl.ensure(BC_WORDS));

    // launch geometry: persistent blocks of 256 lanes, each with its kernel's unit contexts in LDS (just
    // under 40 KB -> 4 blocks per CU).  The packed contexts where the launch's bounds allow them, the
    // wide ones otherwise (map_geometry); the relaunch after an arena overflow is the same launch again.
    const MapGeometry geometry = map_geometry(n_units, max_len, ix->d.max_target_count, ix->cu_count,
                                              m->test_map_blocks, m->test_map_layout);
    if (geometry.packed < 0)
        return fail(SKM_ERR_ARG, "SKM_TEST_MAP_LAYOUT=packed: reads of %d bases or lists of %d targets do not fit",
                    max_len, (int)ix->d.max_target_count);
    const int64_t CONTEXTS = geometry.contexts;
    const int64_t blocks = geometry.blocks;
    m->last_map_packed = geometry.packed;
    m->last_map_contexts = geometry.contexts;
    // per context: mask extension words (live + staging, two mates) for slices > 64 targets
    const int64_t ext_words = std::max<int64_t>(0, (ix->d.max_target_count + 63) / 64 - 1);
    SKM_TRY(m->workspace.ensure((size_t)(blocks * CONTEXTS * 4 * ext_words * 2 + 16)));
    m->grid_blocks = (int)blocks;
    {   // the kernel addresses a block's records with 32-bit byte offsets
        const int64_t per_block = (n_units + blocks - 1) / blocks;
        if (per_block * (paired ? 2 : 1) * (int64_t)record_words * 4 >= (1LL << 32))
            return fail(SKM_ERR_ARG, "batch of %lld units with %d-base reads is too large for one launch",
                        (long long)n_units, max_len);
    }
    // entry arena: ~8 ids per unit plus one 2048-id slice of slack per wave
    SKM_TRY(m->unit_entries.ensure((size_t)n_units * 8 + (size_t)blocks * (MAP_THREADS / 64) * MAP_ARENA_CHUNK + 4096));

    MapBatch b{};
    b.records = m->records.p;
    b.n_units = n_units;
    b.words_per_read = words;
    b.record_words = record_words;
    b.paired = paired;
    b.workspace = m->workspace.p;
    b.unit_begin = m->unit_begin.p;
    b.unit_end = m->unit_end.p;
    b.unit_anchor = m->unit_anchor.p;
    b.keep_spans = m->keep_spans ? 1 : 0;
    b.rec_unit = m->rec_unit.p;
    b.rec_tuple = m->rec_tuple.p;
    b.rec_key = m->rec_key.p;
    b.ids_cursor = m->batch_ctl.p + BC_IDS;
    b.fld = m->batch_ctl.p + BC_FLD;
    b.stats = m->batch_ctl.p + BC_STATS;
    for (int i = 0; i < 8; ++i) b.vote[i] = m->vote[i];

    HIP_TRY(hipEventRecord(m->ev[0], m->stream));
    if (fill_records) SKM_TRY((*fill_records)(m->records.p, words, record_words));
    else launch_pack_reads(d_bases, d_offsets, n_reads, words, record_words, m->records.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev[1], m->stream));
    unsigned long long ids = 0;
    // A launch whose ids outgrow the arena stores none of the tuples that do not fit and is run again
    // in a larger one.  A wave takes max(its emission, MAP_ARENA_CHUNK) ids per grab and gives up what is
    // left of a chunk that the next emission does not fit, so the cursor of such a launch depends on
    // how the finished units happened to meet in emission waves, which differs from launch to launch:
    // it bounds no later launch of the same kind.  The relaunch therefore takes exactly what each
    // emission writes (ids_chunk = 0).  Its cursor is the sum of the batch's tuple lengths whatever the
    // grouping, and that sum is at most the first launch's cursor, because every emission of the first
    // launch lay wholly inside a chunk of its own wave and the chunks are disjoint.  An arena of the
    // first cursor's size cannot overflow a second time.
    for (int attempt = 0; attempt < 2; ++attempt) {
        b.unit_entries = m->unit_entries.p;
        b.ids_capacity = (int64_t)m->unit_entries.cap;
        b.ids_chunk = attempt == 0 ? MAP_ARENA_CHUNK : 0;
        HIP_TRY(hipMemsetAsync(m->batch_ctl.p, 0, BC_WORDS * sizeof(unsigned long long), m->stream));
        launch_map_units(ix->d, b, m->grid_blocks, m->want_stats, geometry.packed == 1, m->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(m->ev[2], m->stream));
        unsigned long long *cursor_and_flag = m->pinned + 32;
        HIP_TRY(hipMemcpyAsync(cursor_and_flag, b.ids_cursor, 16, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        ids = cursor_and_flag[0];
        if (cursor_and_flag[1]) return fail(SKM_ERR_STATE, "map kernel: the in-kernel scheduler stalled");
        if ((int64_t)ids <= b.ids_capacity) break;
        if (attempt == 1) return fail(SKM_ERR_STATE, "entry arena overflow");
        SKM_TRY(m->unit_entries.ensure((size_t)ids));
        m->map_relaunches += 1;
    }
    m->last_ids = (int64_t)ids;
    if (m->want_stats) {
        unsigned long long st[48];
        HIP_TRY(hipMemcpy(st, b.stats, sizeof(st), hipMemcpyDeviceToHost));
        for (int i = 0; i < 48; ++i) m->stats_total[i] += st[i];
    }
    // strand-specific library: the records keep the entries of its orientation (nothing is
    // launched unstranded)
    if (m->strand != SKM_STRAND_NONE) {
        launch_strand_filter(b, m->strand, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (collapse) SKM_TRY((*collapse)(b));
    if (m->bias) {             // --bias: the first hexamers of the units that are still aligned
        launch_bias_observed(m->records.p, record_words, words, paired, m->rec_tuple.p, m->rec_unit.p, n_units,
                             m->bias_observed.p, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (salt && sample_bias_rows) {   // a sample set that counts: the same rule, by the unit's sample
        launch_sample_bias(b, *salt, sample_bias_rows, m->stream);
        HIP_TRY(hipGetLastError());
    }
    if (salt) {
        launch_sample_salt(b, *salt, m->error.p, m->stream);
        HIP_TRY(hipGetLastError());
    }

    // class counting
    SKM_TRY(table_reserve(m, n_units));
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + (int64_t)ids + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    // A large batch on an empty table goes in two waves of records: once the classes of the first
    // quarter are committed, most records of the rest land on a committed class and are verified
    // inside class_insert (the slot's tuple word came with the probe); class_verify's second random
    // pass over the table is left with the first wave and the records of classes new in the second.
    const bool two_waves = m->host_classes == 0 && n_units >= (1 << 21);
    for (int pass = 0;; ++pass) {
        // insert (with the commit of the new classes) -> totals -> verify: one pipeline, one
        // synchronisation; the optimistic case needs a single pass
        HIP_TRY(hipMemsetAsync(m->counters.p + CTR_DEFERRED, 0, 8, m->stream));
        // (wave borders in sixteenths of the batch; SKM_CLASS_WAVES="2,8" etc. is a tuning aid)
        int cuts[8] = {4, 16, 16, 16, 16, 16, 16, 16};
        int n_waves = two_waves && pass == 0 ? 2 : 1;
#ifdef SKM_TUNING                                    // (tuning builds only: scripts/build_variant.sh)
        if (n_waves > 1)
            if (const char *e = getenv("SKM_CLASS_WAVES")) {
                int parsed[8], n = 0;
                bool ok = true;
                for (const char *c = e; *c && n < 7;) {
                    parsed[n] = atoi(c);
                    ok = ok && parsed[n] >= 1 && parsed[n] <= 16 && (n == 0 || parsed[n] > parsed[n - 1]);
                    ++n;
                    while (*c && *c != ',') ++c;
                    if (*c == ',') ++c;
                }
                if (ok && n > 0) {                 // strictly ascending sixteenths, else ignored
                    if (parsed[n - 1] < 16) parsed[n++] = 16;
                    for (int i = 0; i < n; ++i) cuts[i] = parsed[i];
                    n_waves = n;
                }
            }
#endif
        for (int wave = 0; wave < n_waves; ++wave) {
            const int64_t w0 = n_waves == 1 || wave == 0 ? 0 : n_units * cuts[wave - 1] / 16;
            const int64_t w1 = n_waves == 1 ? n_units : n_units * cuts[wave] / 16;
            MapBatch part = b;                   // records [w0, w1) of the batch
            part.rec_unit += w0; part.rec_key += w0; part.rec_tuple += w0;
            part.n_units = w1 - w0;
            launch_class_insert(m->t, part, unit_base, m->unit_slot.p + w0, pass > 0, pass == 0 && wave == 0, m->stream);
            launch_class_verify(m->t, part, m->unit_slot.p + w0, m->stream);
        }
        HIP_TRY(hipGetLastError());
        if (pass == 0) HIP_TRY(hipEventRecord(m->ev[3], m->stream));
        HIP_TRY(hipMemcpyAsync(m->pinned, m->counters.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(m->pinned + 16, m->error.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        const int err = *reinterpret_cast<int *>(m->pinned + 16);
        if (err == SKM_ERR_COLLISION)
            return fail(SKM_ERR_COLLISION, collapse ? "two different class tuples, or two different molecules, share a 64-bit key"
                                                    : "two different class tuples share a 64-bit key");
        if (err == SKM_ERR_ARG) return fail(SKM_ERR_ARG, "a packed read is longer than its code words hold");
        if (err) return fail(err, "class table kernel reported error %d", err);
        m->host_arena_used = (int64_t)m->pinned[CTR_ARENA];
        m->host_classes = (int64_t)m->pinned[CTR_CLASSES];
        m->host_units = m->pinned[CTR_UNITS];
        m->host_unaligned = m->pinned[CTR_UNALIGNED];
        m->host_totals_valid = true;
        if (m->pinned[CTR_LISTED] != m->pinned[CTR_CLASSES])
            return fail(SKM_ERR_STATE, "class registry out of step (%llu listed, %llu classes)",
                        m->pinned[CTR_LISTED], m->pinned[CTR_CLASSES]);
        if (m->pinned[CTR_DEFERRED] == 0) break;
        if (pass > 40) return fail(SKM_ERR_STATE, "class table cannot absorb the batch");
        // too full for bounded probing: grow 4x (its classes move along), retry the deferred units
        SKM_TRY(table_grow(m, (m->t.slot_mask + 1) * 4, n_units));
    }
    // keep the load below 0.5 for the next batch
    if ((uint64_t)m->host_classes * 2 > m->t.slot_mask + 1)
        SKM_TRY(table_grow(m, (m->t.slot_mask + 1) * 2, 0));
    m->units_done += n_units;
    m->first_seen_bound = std::max(m->first_seen_bound, std::max(m->units_done, unit_base + n_units));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[0], m->ev[1])); m->t_pack_ns += ms * 1e6;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[1], m->ev[2])); m->t_map_ns += ms * 1e6;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev[2], m->ev[3])); m->t_class_ns += ms * 1e6;
    m->batches += 1;
    return SKM_OK;
}

}  // namespace abi
}  // namespace skm

extern "C" int skm_mapper_create(skm_index *ix, skm_mapper **out)
{
    if (!ix || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(set_device(ix->device));
    std::unique_ptr<skm_mapper> m(new skm_mapper(ix));     // (any early return below: nothing is left behind)
    HIP_TRY(pool_stream_acquire(m->stream.out()));
    for (auto &e : m->ev) HIP_TRY(hipEventCreate(e.out()));
    HIP_TRY(hipHostMalloc((void **)m->pinned.out(), 64 * sizeof(unsigned long long)));
    if (const char *v = getenv("SKM_MAP_STATS")) m->want_stats = v[0] == '2' ? 2 : 1;
    if (const char *v = getenv("SKM_TEST_PACKED_MAX_PENDING"))      // test hook: the pushers' byte limit
        if (atoll(v) > 0) m->feed.packed_max_pending = atoll(v);
    if (const char *v = getenv("SKM_MAP_VOTE"))          // tuning aid: "start,lookup,merge,left,right,emit,scan"
        sscanf(v, "%d,%d,%d,%d,%d,%d,%d", &m->vote[0], &m->vote[1], &m->vote[2], &m->vote[3], &m->vote[4],
               &m->vote[5], &m->vote[6]);
    HIP_TRY(hipStreamCreateWithFlags(m->feed.packed_stream.out(), hipStreamNonBlocking));   // (10 ms: not at the first piece's push)
    uint64_t first_slots = 1 << 16;
    if (const char *v = getenv("SKM_TEST_CLASS_SLOTS")) {        // test hook: a table that has to grow under a batch
        const long long n = atoll(v);
        if (n < 2 || n > (1LL << 30) || (n & (n - 1)))
            return fail(SKM_ERR_ARG, "SKM_TEST_CLASS_SLOTS must be a power of two from 2 to 2^30, not '%s'", v);
        first_slots = (uint64_t)n;
        m->test_class_slots = true;
    }
    if (const char *v = getenv("SKM_TEST_MAP_BLOCKS")) {         // test hook: few blocks, so that contexts are refilled
        const long long n = atoll(v);
        if (n < 1 || n > (1LL << 30))
            return fail(SKM_ERR_ARG, "SKM_TEST_MAP_BLOCKS must be a number from 1 to 2^30, not '%s'", v);
        m->test_map_blocks = (int)n;
    }
    if (const char *v = getenv("SKM_TEST_MAP_LAYOUT")) {         // test hook: the map kernel of every launch
        if (!strcmp(v, "wide")) m->test_map_layout = MAP_LAYOUT_WIDE;
        else if (!strcmp(v, "packed")) m->test_map_layout = MAP_LAYOUT_PACKED;   // (a launch that does not fit fails)
        else return fail(SKM_ERR_ARG, "SKM_TEST_MAP_LAYOUT must be 'wide' or 'packed', not '%s'", v);
    }
    SKM_TRY(table_reset(m.get(), first_slots));
    HIP_TRY(hipStreamSynchronize(m->stream));
    *out = m.release();                                     // (the caller's handle from here on)
    return SKM_OK;
}

skm_mapper::~skm_mapper()
{
    (void)hipSetDevice(ix->device);
    feed.shutdown();
    // every stream drains before the members -- buffers, pieces, streams, events -- free themselves
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto &lane : feed.lanes)
        if (lane.stream) (void)hipStreamSynchronize(lane.stream);
    if (feed.packed_stream) (void)hipStreamSynchronize(feed.packed_stream);
}

extern "C" int skm_mapper_destroy(skm_mapper *m)
{
    delete m;
    return SKM_OK;
}

extern "C" int skm_mapper_map_batch_device(skm_mapper *m, const void *d_bases, const void *d_offsets,
                                           int64_t n_units, int paired, int32_t max_read_len)
{
    if (!m || !d_offsets || n_units < 0 || max_read_len < 0)
        return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    return map_batch_resident(m, (const uint8_t *)d_bases, (const int64_t *)d_offsets, n_units,
                              paired, max_read_len);
}

extern "C" int skm_mapper_last_batch(skm_mapper *m, int32_t *begin, int32_t *end,
                                     int32_t *anchor_entry, int32_t *anchor_offset, int32_t *counts,
                                     int32_t *entries, int64_t cap_entries, int64_t *n_entries)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t n = m->last_units;
    if (n_entries) *n_entries = 0;
    if (n == 0) return SKM_OK;
    if ((begin || end || anchor_entry || anchor_offset) && !m->last_spans)
        return fail(SKM_ERR_STATE, "the spans of the last batch were not kept: call skm_mapper_keep_spans(mapper, 1) before mapping");
    if (begin) HIP_TRY(hipMemcpy(begin, m->unit_begin.p, n * 4, hipMemcpyDeviceToHost));
    if (end) HIP_TRY(hipMemcpy(end, m->unit_end.p, n * 4, hipMemcpyDeviceToHost));
    if (anchor_entry || anchor_offset) {
        std::vector<Coord> a(n);
        HIP_TRY(hipMemcpy(a.data(), m->unit_anchor.p, n * sizeof(Coord), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            if (anchor_entry) anchor_entry[i] = a[i].entry;
            if (anchor_offset) anchor_offset[i] = a[i].offset;
        }
    }
    if (!counts && !entries && !n_entries) return SKM_OK;
    // the records of the batch (emission order) -> per unit
    std::vector<int32_t> unit(n);
    std::vector<unsigned long long> tuple(n);
    HIP_TRY(hipMemcpy(unit.data(), m->rec_unit.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tuple.data(), m->rec_tuple.p, n * 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> cnt(n, 0);
    std::vector<int64_t> off(n, 0);
    std::vector<char> seen(n, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t u = unit[r];
        if (u < 0 || u >= n || seen[u]) return fail(SKM_ERR_STATE, "record %lld names unit %lld", (long long)r, (long long)u);
        seen[u] = 1;
        cnt[u] = (int32_t)(tuple[r] >> 40);
        off[u] = (int64_t)(tuple[r] & ((1ULL << 40) - 1));
    }
    if (counts) memcpy(counts, cnt.data(), n * 4);
    if (n_entries) {
        int64_t total = 0;
        for (int64_t u = 0; u < n; ++u) total += cnt[u];
        *n_entries = total;           // the arena itself has per-wave slack
    }
    if (entries) {
        std::vector<int32_t> raw((size_t)std::max<int64_t>(m->last_ids, 1));
        if (m->last_ids)
            HIP_TRY(hipMemcpy(raw.data(), m->unit_entries.p, (size_t)m->last_ids * 4, hipMemcpyDeviceToHost));
        int64_t pos = 0;
        for (int64_t u = 0; u < n; ++u) {
            for (int i = 0; i < cnt[u]; ++i)
                if (pos + i < cap_entries) entries[pos + i] = raw[off[u] + i];
            pos += cnt[u];
        }
    }
    return SKM_OK;
}

extern "C" int skm_mapper_copy_records(skm_mapper *m, int64_t first_read, int64_t n_reads, uint32_t *out,
                                       int32_t *record_words, int32_t *words_per_read)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    if (m->last_reads == 0) return fail(SKM_ERR_STATE, "no batch has been mapped since the handle was made or reset");
    if (first_read < 0 || n_reads < 0 || first_read > m->last_reads || n_reads > m->last_reads - first_read)
        return fail(SKM_ERR_ARG, "reads %lld .. +%lld of a batch of %lld", (long long)first_read, (long long)n_reads,
                    (long long)m->last_reads);
    if (record_words) *record_words = m->last_record_words;
    if (words_per_read) *words_per_read = m->last_words;
    if (out && n_reads) {
        HIP_TRY(hipStreamSynchronize(m->stream));
        HIP_TRY(hipMemcpy(out, m->records.p + first_read * (int64_t)m->last_record_words,
                          (size_t)n_reads * m->last_record_words * 4, hipMemcpyDeviceToHost));
    }
    return SKM_OK;
}

extern "C" int skm_pack_stage_reads(int32_t words_per_read, int32_t *reads_per_block)
{
    if (words_per_read < 1 || !reads_per_block) return fail(SKM_ERR_ARG, "bad argument");
    *reads_per_block = pack_stage_reads(words_per_read);
    return SKM_OK;
}

extern "C" int skm_map_geometry(int64_t n_units, int32_t max_read_len, int32_t max_target_count, int32_t cu_count,
                                int32_t block_cap, int32_t *packed, int32_t *contexts, int64_t *blocks)
{
    if (n_units < 0 || max_read_len < 0 || max_target_count < 0 || cu_count < 1 || block_cap < 0 || !packed || !contexts || !blocks)
        return fail(SKM_ERR_ARG, "bad argument");
    const MapGeometry g = map_geometry(n_units, max_read_len, max_target_count, cu_count, block_cap, MAP_LAYOUT_AUTO);
    *packed = g.packed;
    *contexts = g.contexts;
    *blocks = g.blocks;
    return SKM_OK;
}

extern "C" int skm_mapper_map_layout(skm_mapper *m, int32_t *packed, int32_t *contexts, int32_t *blocks)
{
    if (!m || !packed || !contexts || !blocks) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->last_map_packed < 0) return fail(SKM_ERR_STATE, "no batch has been mapped yet");
    *packed = m->last_map_packed;
    *contexts = m->last_map_contexts;
    *blocks = m->grid_blocks;
    return SKM_OK;
}

extern "C" int skm_mapper_keep_spans(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    m->keep_spans = enable != 0;
    return SKM_OK;
}

extern "C" int skm_mapper_set_strand(skm_mapper *m, int mode)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    if (mode != SKM_STRAND_NONE && mode != SKM_STRAND_FR && mode != SKM_STRAND_RF)
        return fail(SKM_ERR_ARG, "unknown strand mode %d", mode);
    (void)wait_jobs(m, 0, false);
    bool queued;
    {
        std::lock_guard<std::mutex> hold(m->feed.q_mu);
        queued = !m->feed.jobs.empty() || m->feed.packed_busy || !m->feed.book.empty();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    if (queued || m->units_done != 0)
        return fail(SKM_ERR_STATE, "the strand mode can only change on an empty mapper (new, or after "
                                   "skm_mapper_reset / skm_mapper_clear)");
    m->strand = mode;
    return SKM_OK;
}

extern "C" int skm_mapper_set_bias(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    bool queued;
    {
        std::lock_guard<std::mutex> hold(m->feed.q_mu);
        queued = !m->feed.jobs.empty() || m->feed.packed_busy || !m->feed.book.empty();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    if (queued || m->units_done != 0)
        return fail(SKM_ERR_STATE, "hexamer counting can only change on an empty mapper (new, or after "
                                   "skm_mapper_reset / skm_mapper_clear)");
    if (enable) {
        SKM_TRY(set_device(m->ix->device));
        SKM_TRY(m->bias_observed.ensure(BIAS_BINS));
        HIP_TRY(hipMemsetAsync(m->bias_observed.p, 0, BIAS_BINS * sizeof(unsigned long long), m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    m->bias = enable != 0;
    return SKM_OK;
}

extern "C" int skm_mapper_bias_observed(skm_mapper *m, int64_t out[4096])
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->bias) return fail(SKM_ERR_STATE, "this mapper does not count hexamers: call skm_mapper_set_bias(mapper, 1) before mapping");
    SKM_TRY(set_device(m->ix->device));
    HIP_TRY(hipMemcpy(out, m->bias_observed.p, BIAS_BINS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return SKM_OK;
}

namespace skm {
namespace abi __attribute__((visibility("hidden"))) {

// the weights of a fragment-length model: every one finite and >= 0 (checked on the host, before any device work)
bool length_weights_valid(const double *p, int64_t count)
{
    for (int64_t i = 0; i < count; ++i)
        if (!(p[i] >= 0.0) || std::isinf(p[i])) return false;
    return true;
}

}  // namespace abi
}  // namespace skm

extern "C" int skm_mapper_set_length_weights(skm_mapper *m, const double *p)
{
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    if (p && !length_weights_valid(p, MAX_FRAGMENT_LENGTH))
        return fail(SKM_ERR_ARG, "a fragment-length weight is negative or not finite");
    SKM_TRY(wait_jobs(m, 0, false));
    std::lock_guard<std::mutex> lock(m->mu);
    if (!p) {
        m->use_length_weights = false;
        return SKM_OK;
    }
    SKM_TRY(set_device(m->ix->device));
    SKM_TRY(m->length_weights.ensure(MAX_FRAGMENT_LENGTH));
    // (no quantification call is under way: they hold mu until their stream has drained)
    HIP_TRY(hipMemcpy(m->length_weights.p, p, MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
    m->use_length_weights = true;
    return SKM_OK;
}

extern "C" int skm_mapper_summary(skm_mapper *m, int64_t summary[4])
{
    if (!m || !summary) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));
    summary[0] = (int64_t)ctr[CTR_CLASSES];
    summary[1] = (int64_t)ctr[CTR_ARENA];
    summary[2] = (int64_t)ctr[CTR_UNALIGNED];
    summary[3] = (int64_t)ctr[CTR_UNITS];
    return SKM_OK;
}

extern "C" int skm_mapper_export(skm_mapper *m, int64_t *class_offsets, int32_t *class_targets,
                                 int64_t *class_counts, int64_t *first_seen, int64_t *fld)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    if (fld)
        HIP_TRY(hipMemcpy(fld, m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8, hipMemcpyDeviceToHost));
    if (!class_offsets && !class_targets && !class_counts && !first_seen) return SKM_OK;
    const int64_t C = m->host_classes, M = m->host_arena_used;
    if (class_offsets) class_offsets[0] = 0;
    if (C == 0) return SKM_OK;
    DBuf<int64_t> d_off, d_len; DBuf<double> d_cnt; DBuf<unsigned long long> d_fs;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
    SKM_TRY(d_off.ensure(C)); SKM_TRY(d_len.ensure(C)); SKM_TRY(d_cnt.ensure(C)); SKM_TRY(d_fs.ensure(C));
    launch_class_compact(m->t, C, d_off.p, d_len.p, d_cnt.p, d_fs.p, m->stream);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> off(C), len(C);
    std::vector<double> cnt(C);
    std::vector<unsigned long long> fs(C);
    std::vector<int32_t> arena((size_t)std::max<int64_t>(M, 1));
    HIP_TRY(hipMemcpyAsync(off.data(), d_off.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(len.data(), d_len.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(fs.data(), d_fs.p, C * 8, hipMemcpyDeviceToHost, m->stream));
    if (M) HIP_TRY(hipMemcpyAsync(arena.data(), m->arena.p, (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    drain.dismiss();
    // Counter insertion order under -j1 = ascending first-seen unit (mapper.py:88)
    std::vector<int64_t> order(C);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return fs[a] < fs[b]; });
    int64_t pos = 0;
    for (int64_t k = 0; k < C; ++k) {
        const int64_t c = order[k];
        if (class_targets)
            memcpy(class_targets + pos, arena.data() + off[c], (size_t)len[c] * 4);
        pos += len[c];
        if (class_offsets) class_offsets[k + 1] = pos;
        if (class_counts) class_counts[k] = (int64_t)cnt[c];
        if (first_seen) first_seen[k] = (int64_t)fs[c];
    }
    return SKM_OK;
}

extern "C" int skm_mapper_merge(skm_mapper *m, int64_t n_classes, const int64_t *class_offsets,
                                const int32_t *class_targets, const int64_t *class_counts,
                                const int64_t *first_seen, int64_t unaligned, const int64_t *fld)
{
    if (!m || n_classes < 0 || unaligned < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (!class_offsets || !class_targets || !class_counts || !first_seen))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    m->host_totals_valid = false;             // (the totals change on the device below)
    SKM_TRY(set_device(m->ix->device));
    std::vector<unsigned long long> add(CTR_WORDS, 0);
    int64_t units = unaligned;
    for (int64_t c = 0; c < n_classes; ++c) units += class_counts[c];
    add[CTR_UNALIGNED] = (unsigned long long)unaligned;
    add[CTR_UNITS] = (unsigned long long)units;
    if (fld) for (int i = 0; i < MAX_FRAGMENT_LENGTH; ++i) add[CTR_FLD + i] = (unsigned long long)fld[i];
    if (n_classes) {
        const int64_t M = class_offsets[n_classes];
        {   // foreign classes may all be new: size for them at load <= 0.5, unbounded probes
            uint64_t want = 1 << 16;
            while ((double)want * 0.5 < (double)(m->host_classes + n_classes + 1024)) want <<= 1;
            SKM_TRY(table_grow(m, want, 0));
            SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_classes + 1024), true, m->stream));
        }
        SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + M + 1024), true, m->stream));
        bind_table(m, m->t.slot_mask + 1);
        DBuf<int64_t> d_off, d_cnt, d_fs; DBuf<int32_t> d_ids;
        auto drain = on_exit([&]() { (void)hipStreamSynchronize(m->stream); });   // (an early return: before they go)
        SKM_TRY(d_off.ensure(n_classes + 1)); SKM_TRY(d_cnt.ensure(n_classes));
        SKM_TRY(d_fs.ensure(n_classes)); SKM_TRY(d_ids.ensure(std::max<int64_t>(M, 1)));
        HIP_TRY(hipMemcpy(d_off.p, class_offsets, (n_classes + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_cnt.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_fs.p, first_seen, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(d_ids.p, class_targets, M * 4, hipMemcpyHostToDevice));
        launch_class_merge(m->t, n_classes, d_off.p, d_ids.p, d_cnt.p, d_fs.p, m->stream);
        HIP_TRY(hipGetLastError());
        unsigned long long ctr[8];
        HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
        SKM_TRY(read_error(m));
        drain.dismiss();                      // (read_error has synchronised the stream)
        m->host_arena_used = (int64_t)ctr[CTR_ARENA];
        m->host_classes = (int64_t)ctr[CTR_CLASSES];
    }
    // totals and histogram only once the classes are in: a failed merge leaves them untouched
    std::vector<unsigned long long> cur(CTR_WORDS);
    HIP_TRY(hipMemcpy(cur.data(), m->counters.p, CTR_WORDS * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < CTR_WORDS; ++i) cur[i] += add[i];
    HIP_TRY(hipMemcpy(m->counters.p, cur.data(), CTR_WORDS * 8, hipMemcpyHostToDevice));
    m->units_done += units;
    for (int64_t c = 0; c < n_classes; ++c)
        m->first_seen_bound = std::max(m->first_seen_bound, first_seen[c] + 1);
    m->first_seen_bound = std::max(m->first_seen_bound, m->units_done);
    return SKM_OK;
}

// The table where it lies (SURVEY 8(e).1 without the host: the hand-over between GPUs is then a
// copy of these arrays over xGMI, ncclSend / ncclRecv or a peer copy, and a merge by key).
extern "C" int skm_mapper_device_table(skm_mapper *m, skm_device_table *out)
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    memset(out, 0, sizeof(*out));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const int64_t C = (int64_t)ctr[CTR_CLASSES];
    out->device = m->ix->device;
    out->n_classes = C;
    out->n_ids = (int64_t)ctr[CTR_ARENA];
    out->unaligned = (int64_t)ctr[CTR_UNALIGNED];
    out->units = (int64_t)ctr[CTR_UNITS];
    out->first_seen_bound = m->first_seen_bound;
    out->fld = (const uint64_t *)(m->counters.p + CTR_FLD);
    out->ids = m->arena.p;
    if (C == 0) return SKM_OK;
    SKM_TRY(m->view_start.ensure(C)); SKM_TRY(m->view_len.ensure(C));
    SKM_TRY(m->view_count.ensure(C)); SKM_TRY(m->view_first_seen.ensure(C));
    launch_class_compact(m->t, C, m->view_start.p, m->view_len.p, m->view_count.p, m->view_first_seen.p, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    out->class_start = m->view_start.p;
    out->class_len = m->view_len.p;
    out->class_count = m->view_count.p;
    out->first_seen = (const uint64_t *)m->view_first_seen.p;
    return SKM_OK;
}

extern "C" int skm_mapper_merge_device(skm_mapper *m, const skm_device_table *table)
{
    if (!m || !table || table->n_classes < 0 || table->n_ids < 0 || table->unaligned < 0 || table->units < 0)
        return fail(SKM_ERR_ARG, "bad argument");
    if (table->n_classes && (!table->class_start || !table->class_len || !table->class_count || !table->first_seen || !table->ids))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    if (table->device != m->ix->device)
        return fail(SKM_ERR_ARG, "the table lies on GPU %d, the mapper on GPU %d: copy it over first", table->device, m->ix->device);
    SKM_TRY(wait_jobs(m, 0, false));
    std::lock_guard<std::mutex> lock(m->mu);
    m->host_totals_valid = false;
    SKM_TRY(set_device(m->ix->device));
    const int64_t n_classes = table->n_classes;
    {   // foreign classes may all be new: size for them at load <= 0.5, unbounded probes
        uint64_t want = 1 << 16;
        while ((double)want * 0.5 < (double)(m->host_classes + n_classes + 1024)) want <<= 1;
        SKM_TRY(table_grow(m, want, 0));
        SKM_TRY(m->class_list.ensure((size_t)(m->host_classes + n_classes + 1024), true, m->stream));
    }
    SKM_TRY(m->arena.ensure((size_t)(m->host_arena_used + table->n_ids + 1024), true, m->stream));
    bind_table(m, m->t.slot_mask + 1);
    if (n_classes) {
        launch_class_merge_device(m->t, n_classes, table->class_start, table->class_len, table->ids, table->class_count,
                                  (const unsigned long long *)table->first_seen, m->stream);
        HIP_TRY(hipGetLastError());
        SKM_TRY(read_error(m));
    }
    // totals and histogram only once the classes are in: a failed merge leaves them untouched (the
    // hand-over of a table happens once per sample: the launch boundary is on no hot path)
    launch_class_add_totals(m->t, (unsigned long long)table->unaligned, (unsigned long long)table->units,
                            (const unsigned long long *)table->fld, m->stream);
    HIP_TRY(hipGetLastError());
    unsigned long long ctr[8];
    HIP_TRY(hipMemcpyAsync(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->host_arena_used = (int64_t)ctr[CTR_ARENA];
    m->host_classes = (int64_t)ctr[CTR_CLASSES];
    m->host_units = ctr[CTR_UNITS];
    m->host_unaligned = ctr[CTR_UNALIGNED];
    m->host_totals_valid = true;
    m->units_done += table->units;
    m->first_seen_bound = std::max(m->first_seen_bound, std::max(table->first_seen_bound, m->units_done));
    return SKM_OK;
}

extern "C" int skm_mapper_clear(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, true);            // (a failed queued batch is forgotten with the table)
    {
        std::lock_guard<std::mutex> hold(m->feed.q_mu);      // (and packed reads that never got a mate)
        m->feed.book.drop_all();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // MapResult.clear only clears the counter (mapper.py:143-145): the FLD stays
    std::vector<unsigned long long> fld(MAX_FRAGMENT_LENGTH);
    HIP_TRY(hipMemcpy(fld.data(), m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8, hipMemcpyDeviceToHost));
    SKM_TRY(table_reset(m, m->t.slot_mask + 1));
    HIP_TRY(hipMemcpyAsync(m->counters.p + CTR_FLD, fld.data(), MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return SKM_OK;
}

extern "C" int skm_mapper_reset(skm_mapper *m)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, true);            // (a failed queued batch is forgotten with the table)
    {
        std::lock_guard<std::mutex> hold(m->feed.q_mu);      // (and packed reads that never got a mate)
        m->feed.book.drop_all();
    }
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    SKM_TRY(table_reset(m, m->t.slot_mask + 1));
    if (m->bias) HIP_TRY(hipMemsetAsync(m->bias_observed.p, 0, BIAS_BINS * sizeof(unsigned long long), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));         // (readers of the table use streams of their own)
    m->last_units = 0;
    m->last_ids = 0;
    m->last_reads = 0;
    return SKM_OK;
}

extern "C" int skm_mapper_timing(skm_mapper *m, double stats[8])
{
    if (!m || !stats) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    stats[0] = m->t_pack_ns; stats[1] = m->t_map_ns; stats[2] = m->t_class_ns;
    stats[3] = m->batches; stats[4] = (double)m->units_done;
    stats[5] = m->t_em_ns; stats[6] = m->em_iters; stats[7] = (double)m->deferred_grows;
    return SKM_OK;
}

extern "C" int skm_mapper_map_relaunches(skm_mapper *m, int64_t *count)
{
    if (!m || !count) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    *count = m->map_relaunches;
    return SKM_OK;
}

// access counters of the STATS build of the map kernel (SKM_MAP_STATS=1):
// [0]=reads [1]=read bases [2]=lookups [3]=slots [4]=contig reads [5]=targets
// copied [6]=targets merged [7]=8-base fetches [8]=merges [9]=tuple ids
extern "C" int skm_mapper_access_stats(skm_mapper *m, int64_t out[48])
{
    if (!m || !out) return fail(SKM_ERR_ARG, "NULL argument");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    for (int i = 0; i < 48; ++i) out[i] = (int64_t)m->stats_total[i];
    return SKM_OK;
}

extern "C" int skm_mapper_set_stats(skm_mapper *m, int enable)
{
    if (!m) return fail(SKM_ERR_ARG, "NULL mapper");
    (void)wait_jobs(m, 0, false);
    std::lock_guard<std::mutex> lock(m->mu);
    m->want_stats = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    for (auto &v : m->stats_total) v = 0;
    return SKM_OK;
}
