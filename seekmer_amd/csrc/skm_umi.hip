// UMI collapse ("UMI collapse"): inside one cell of a pooled run a unit whose UMI and class
// an earlier unit of the cell has already shown is a PCR duplicate and is removed as if it had never been read.
//
// (a) umi_window_kernel.  One lane per barcode read, grid-stride.  The UMI is bases [start, start + L), L <= 16, of
// the barcode read: 2 L code bits cut out of the one or two 64-bit code words that hold them (BarcodeWindows, the
// upload of barcode_assign_kernel: only the window's words go up), the exception planes scattered into one dense
// "clean" word per read by barcode_clean_kernel.  A window that the read does not hold, or that holds a position
// other than an upper-case ACGT, has no UMI: the unit belongs to no cell (cell[u] = -1) and is counted.
//
// (b) the molecule set of a sample set: an open-addressing table in HBM, linear probing, at most half full, that
// lives as long as the set.  A slot is one 32-byte sector: tag (a 64-bit mix of the salted class key and the UMI,
// 0 = empty), class key, UMI, the smallest sample-local unit number seen of the molecule, and one word that says the
// molecule's first unit was removed for a neighbour (`dropped`, below; read by skm_molecules.hip alone).  Between the strand
// filter and everything that counts (hexamers, classes, fragment lengths) every launch runs
//   claim   -- every record with a tuple finds or claims its molecule's slot (atomicCAS on the tag; the claimant
//              stores key and UMI with plain stores) and lowers min_unit to its own unit (atomicMin);
//   resolve -- a launch of its own, so that everything claim stored is visible: every such record finds its slot
//              again, compares key and UMI in FULL (a mismatch is a collision of two molecules' tags and fails the
//              call: exact or fail, like the class table) and, if min_unit is not its own unit, removes itself:
//              key 0, tuple length 0, a span that gives no fragment length -- from here on an unaligned unit,
//              which the set subtracts again (removed[sample]).  With one mismatch allowed (umi_resolve_kernel<true>)
//              the first unit of a molecule also looks up its 3 L one-substitution neighbours and removes itself
//              when one of them has a smaller min_unit -- and then marks its molecule's slot `dropped`: no unit of
//              the molecule is left; it reads the set only, with plain loads, for the same
//              reason: claim has finished.  The units removed by a neighbour alone are counted in ctl[UMI_CTL_NEAR].
// Units of earlier launches have smaller local numbers (a sample's segments are added in order), so an entry of an
// earlier launch always wins; inside a launch the minimum does not depend on the order of arrival.  No lane waits
// for another; nothing a lane stores with a plain store is read in the same launch.
//   Every index is bounded before use: slots by the mask, segments by the bisection over the launch's table,
// a unit's UMI inside its segment's array, removed[] by the rows the host has made for the launch's samples.
#include "../../include/seekmer_hip.h"
#include "skm_kernels.h"

#include <algorithm>

namespace skm {

namespace {

__global__ void __launch_bounds__(256)
umi_window_kernel(BarcodeWindows w, int L, int32_t *__restrict__ cell, uint32_t *__restrict__ umi,
                  unsigned long long *n_unreadable)
{
    __shared__ unsigned int s_unreadable;
    if (threadIdx.x == 0) s_unreadable = 0;
    __syncthreads();
    const uint32_t window_bits = ~(~0u >> L);                 // (L <= 16)
    const bool two_words = w.offset + L > 32;
    unsigned int unreadable = 0;
    for (int64_t u = blockIdx.x * 256LL + threadIdx.x; u < w.n_reads; u += gridDim.x * 256LL) {
        const int64_t len = w.lengths ? (int64_t)w.lengths[u] : w.uniform_len;
        bool readable = !(w.words == 0 || len < (int64_t)w.start + L || (two_words && w.words < 2));     // else short
        uint32_t value = 0;
        if (readable) {
            const uint64_t *c = w.codes + u * w.words;
            uint64_t high = c[0] << (2 * w.offset);
            if (two_words) high |= c[1] >> (64 - 2 * w.offset);       // (offset > 0 here)
            value = (uint32_t)(high >> (64 - 2 * L));
            readable = (~w.clean[u] & window_bits) == 0;
        }
        umi[u] = readable ? value : 0u;
        if (!readable) {
            if (cell) cell[u] = -1;
            ++unreadable;
        }
    }
    if (unreadable) atomicAdd(&s_unreadable, unreadable);
    __syncthreads();
    if (threadIdx.x == 0 && s_unreadable) atomicAdd(n_unreadable, (unsigned long long)s_unreadable);
}

__global__ void __launch_bounds__(256)
umi_init_kernel(UmiSlot *slots, uint64_t n_slots)
{
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_slots; i += gridDim.x * 256ULL) {
        slots[i].tag = 0;
        slots[i].class_key = 0;
        slots[i].umi = 0;
        slots[i].dropped = 0;
        slots[i].min_unit = ~0ULL;
    }
}

// what a record is to the molecule set: its sample, the salted key of its class, its UMI, its sample-local unit
struct UmiRecord {
    uint64_t key, tag;
    int64_t local;
    uint32_t umi;
    int32_t sample;
};

// (key != 0: the record has a tuple.)  A salted key or a tag of 0 cannot be stored: `zero` is raised instead
__device__ __forceinline__ UmiRecord umi_record(uint64_t key, int64_t unit, const int32_t *s_first, const int32_t *s_sample,
                                                const UmiSegment *__restrict__ segs, int n_segments, bool &zero)
{
    UmiRecord r;
    const int64_t seg = segment_find(s_first, n_segments, unit);
    const int64_t at = unit - s_first[seg];
    const UmiSegment here = segs[seg];
    r.sample = s_sample[seg];
    r.key = sample_key(key, (uint32_t)r.sample);
    r.umi = here.umi[at];
    r.local = here.local_first + at;
    r.tag = umi_tag(r.key, r.umi);
    zero |= r.key == 0 || r.tag == 0;
    return r;
}

// Records are taken UMI_WIDTH at a time per lane, their home slots fetched before any is looked at (as
// class_insert_kernel does): the kernel is one random 32-byte sector per record, and the chain record -> slot ->
// atomic of one record runs under the chains of the others.  The probe reads are plain loads: a tag never changes
// once set, and a stale "empty" only costs the CAS that then reports the real tag -- device-scope atomics are
// served at the memory side of the fabric (the XCDs' L2s are not coherent), so every one avoided is a fabric
// request less.  For the same reason a record whose unit is not below the min_unit it read leaves it alone: the
// word only ever decreases, so a stale value is too large and the atomic is merely sent where it was not needed.
constexpr int UMI_WIDTH = 4;

__global__ void __launch_bounds__(256)
umi_claim_kernel(UmiSet t, const int32_t *__restrict__ rec_unit, const uint64_t *__restrict__ rec_key, int64_t n_records,
                 const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_sample,
                 const UmiSegment *__restrict__ segs, int n_segments)
{
    __shared__ int32_t s_first[SAMPLE_LAUNCH_SEGMENTS], s_sample[SAMPLE_LAUNCH_SEGMENTS];
    __shared__ unsigned int s_claimed, s_lost;
    for (int i = threadIdx.x; i < n_segments; i += blockDim.x) { s_first[i] = seg_first[i]; s_sample[i] = seg_sample[i]; }
    if (threadIdx.x == 0) { s_claimed = 0; s_lost = 0; }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t n_slots = t.slot_mask + 1;
    unsigned int claimed = 0, lost = 0;
    bool zero = false;
    for (int64_t r0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r0 < n_records; r0 += UMI_WIDTH * stride) {
        UmiRecord rec[UMI_WIDTH];
        bool live[UMI_WIDTH];
        unsigned long long home_tag[UMI_WIDTH], home_min[UMI_WIDTH];
#pragma unroll
        for (int k = 0; k < UMI_WIDTH; ++k) {
            const int64_t r = r0 + k * stride;
            const uint64_t key = r < n_records ? rec_key[r] : 0;
            live[k] = key != 0;
            rec[k] = UmiRecord{};
            if (live[k]) {
                bool bad = false;
                rec[k] = umi_record(key, rec_unit[r], s_first, s_sample, segs, n_segments, bad);
                zero |= bad;
                live[k] = !bad;
            }
        }
#pragma unroll
        for (int k = 0; k < UMI_WIDTH; ++k) {
            const UmiSlot *home = &t.slots[rec[k].tag & t.slot_mask];      // (a record that is not live: slot 0, unused)
            home_tag[k] = home->tag;
            home_min[k] = home->min_unit;
        }
#pragma unroll
        for (int k = 0; k < UMI_WIDTH; ++k) {
            if (!live[k]) continue;
            uint64_t slot = rec[k].tag & t.slot_mask;
            bool found = false;
            unsigned long long seen = ~0ULL;
            for (uint64_t n = 0; n < n_slots; ++n) {
                unsigned long long cur = n ? t.slots[slot].tag : home_tag[k];
                seen = n ? t.slots[slot].min_unit : home_min[k];
                if (cur == 0) {
                    cur = atomicCAS(&t.slots[slot].tag, 0ULL, (unsigned long long)rec[k].tag);
                    if (cur == 0) {                   // the claimant: nobody reads these two before the next launch
                        t.slots[slot].class_key = rec[k].key;
                        t.slots[slot].umi = rec[k].umi;
                        ++claimed;
                        cur = rec[k].tag;
                    }
                    seen = ~0ULL;
                }
                if (cur == rec[k].tag) { found = true; break; }
                slot = (slot + 1) & t.slot_mask;
            }
            if (!found) { ++lost; continue; }         // the set is full: the host grows it (tests) or fails
            if (seen > (unsigned long long)rec[k].local) atomicMin(&t.slots[slot].min_unit, (unsigned long long)rec[k].local);
        }
    }
    if (claimed) atomicAdd(&s_claimed, claimed);
    if (lost) atomicAdd(&s_lost, lost);
    if (zero) atomicExch(t.error, SKM_ERR_COLLISION);
    __syncthreads();
    if (threadIdx.x == 0 && s_claimed) atomicAdd(t.ctl + UMI_CTL_ENTRIES, (unsigned long long)s_claimed);
    if (threadIdx.x == 0 && s_lost) atomicAdd(t.ctl + UMI_CTL_LOST, (unsigned long long)s_lost);
}

// A block takes UMI_RESOLVE_RUN consecutive records, 256 at a time.  Neighbouring records are mostly one sample's
// (sample_bias_kernel says why): a tile whose records with a tuple all belong to one sample (a block-wide vote)
// counts its removals in LDS, and the block adds them to removed[sample] when that sample changes and at the end;
// a mixed tile adds straight to HBM.  Integer adds: any order gives the same counts.
constexpr int UMI_RESOLVE_RUN = 1024;

// The neighbour step (skm_sample_set_set_umi_mismatches(set, 1); DESIGN.md section 4, "UMI mismatches").  A record
// that is the first unit of its own molecule is still removed when one of the 3 L molecules (same salted class key,
// UMI one substitution away) is in the set with a min_unit below the record's unit: an EARLIER unit of the cell showed
// a UMI at distance 1, whether or not that unit stayed itself -- so one lane decides from the set alone, waits for
// nobody and stores nothing into the set.  Everything claim stored (tags by CAS, keys and UMIs by plain stores,
// min_unit by atomicMin), in this launch and in every one before it, is visible: resolve is a launch of its own, and
// claim of the same launch has finished -- also where the test hook grew the set and claimed again.  So all reads
// here are plain loads, and a min_unit is final for every unit below the launch's end: a later launch only brings
// larger units, which never decide about this record.
//   The 3 L probe chains of a record are independent random 32-byte sectors: UMI_NEAR_WIDTH home slots (two
// positions' three substitutions) are fetched whole before any is looked at, as umi_claim_kernel does with its
// records; a chain that goes past its home slot walks on alone (at load 1/2 mostly inside the 128-byte line its
// home slot brought).  A probe ends at an empty slot, at a slot with the neighbour's tag, or after n_slots steps.
// A tag match whose key or UMI differs is another molecule with the neighbour's tag: the neighbour itself cannot
// be stored beside it, so it is not in the set -- no collision is raised for a molecule no record has shown (the
// records of a real collision report it themselves above).  A neighbour whose tag is 0 cannot be stored: skipped.
//   Bounds: shifts are 2 * position <= 30 (L <= 16), slots go through the mask, walks end after n_slots steps.
constexpr int UMI_NEAR_WIDTH = 6;

// true: an earlier unit of the record's cell and class has a UMI one substitution away
__device__ __forceinline__ bool umi_near_earlier(const UmiSet &t, const UmiRecord &rec, int L, uint64_t n_slots)
{
    const unsigned long long mine = (unsigned long long)rec.local;
    bool earlier = false;
    for (int p = 0; p < L && !earlier; p += UMI_NEAR_WIDTH / 3) {
        uint32_t near[UMI_NEAR_WIDTH], home_umi[UMI_NEAR_WIDTH];
        uint64_t tag[UMI_NEAR_WIDTH];
        unsigned long long home_tag[UMI_NEAR_WIDTH], home_key[UMI_NEAR_WIDTH], home_min[UMI_NEAR_WIDTH];
#pragma unroll
        for (int k = 0; k < UMI_NEAR_WIDTH; ++k) {
            const int at = p + k / 3;                                  // the position, counted from the UMI's last base
            near[k] = rec.umi ^ ((uint32_t)(k % 3 + 1) << (2 * (at & 15)));
            tag[k] = at < L ? umi_tag(rec.key, near[k]) : 0;           // (0: nothing to look for)
        }
#pragma unroll
        for (int k = 0; k < UMI_NEAR_WIDTH; ++k) {
            const UmiSlot *home = &t.slots[tag[k] & t.slot_mask];      // (tag 0: slot 0, unused)
            home_tag[k] = home->tag;
            home_key[k] = home->class_key;
            home_umi[k] = home->umi;
            home_min[k] = home->min_unit;
        }
#pragma unroll
        for (int k = 0; k < UMI_NEAR_WIDTH; ++k) {
            if (tag[k] == 0) continue;
            if (home_tag[k] == tag[k]) {
                earlier |= home_key[k] == rec.key && home_umi[k] == near[k] && home_min[k] < mine;
                continue;
            }
            unsigned long long cur = home_tag[k];
            uint64_t slot = tag[k] & t.slot_mask;
            for (uint64_t n = 1; cur != tag[k] && cur != 0 && n < n_slots; ++n) {
                slot = (slot + 1) & t.slot_mask;
                cur = t.slots[slot].tag;
            }
            if (cur != tag[k]) continue;
            const UmiSlot *entry = &t.slots[slot];
            earlier |= entry->class_key == rec.key && entry->umi == near[k] && entry->min_unit < mine;
        }
    }
    return earlier;
}

// NEAR: with the neighbour step, and then with one more argument, the bases of a UMI; without it the kernel has the
// arguments and the code it always had
template <bool NEAR, typename... Bases>
__global__ void __launch_bounds__(256)
umi_resolve_kernel(UmiSet t, MapBatch b, const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_sample,
                   const UmiSegment *__restrict__ segs, int n_segments, unsigned long long *__restrict__ removed, Bases... bases)
{
    static_assert(sizeof...(Bases) == (NEAR ? 1 : 0), "the UMI's length goes with the neighbour step");
    const int L = (0 + ... + bases);
    __shared__ int32_t s_first[SAMPLE_LAUNCH_SEGMENTS], s_sample[SAMPLE_LAUNCH_SEGMENTS];
    __shared__ unsigned int s_removed, s_near;    // (s_near: touched by the neighbour form alone, the other has none)
    __shared__ int32_t s_ref;
    for (int i = threadIdx.x; i < n_segments; i += blockDim.x) { s_first[i] = seg_first[i]; s_sample[i] = seg_sample[i]; }
    if (threadIdx.x == 0) s_removed = 0;
    if constexpr (NEAR) { if (threadIdx.x == 0) s_near = 0; }
    __syncthreads();
    const int64_t run_first = (int64_t)blockIdx.x * UMI_RESOLVE_RUN;
    const int64_t run_end = run_first + UMI_RESOLVE_RUN < b.n_units ? run_first + UMI_RESOLVE_RUN : b.n_units;
    const uint64_t n_slots = t.slot_mask + 1;
    int64_t held = -1;                            // the sample whose removals s_removed counts (block-uniform)
    auto flush = [&]() {                          // (called by the whole block)
        __syncthreads();
        if (threadIdx.x == 0 && s_removed) {
            atomicAdd(&removed[held], (unsigned long long)s_removed);
            s_removed = 0;
        }
        __syncthreads();
    };
    int fault = 0;
    unsigned int near = 0;                        // removed by a neighbour alone
    for (int64_t tile = run_first; tile < run_end; tile += blockDim.x) {
        const int64_t r = tile + threadIdx.x;
        const uint64_t key = r < run_end ? b.rec_key[r] : 0;
        const bool mine = key != 0;
        const int32_t unit = mine ? b.rec_unit[r] : 0;
        UmiRecord rec{};
        bool zero = false;
        if (mine) rec = umi_record(key, unit, s_first, s_sample, segs, n_segments, zero);
        if (threadIdx.x == 0) s_ref = -1;         // (the vote of the tile before lies behind everyone's read of it)
        __syncthreads();
        if (mine) s_ref = rec.sample;             // (any of the tile's samples: the vote says whether it is the only one)
        __syncthreads();
        const int32_t ref = s_ref;
        const bool one_sample = __syncthreads_and(!mine || rec.sample == ref) != 0;      // block-uniform
        if (one_sample && ref >= 0 && held != ref) {
            if (held >= 0) flush();
            held = ref;
        }
        if (!mine) continue;
        if (zero) { fault = SKM_ERR_COLLISION; continue; }
        uint64_t slot = rec.tag & t.slot_mask;
        bool found = false;
        for (uint64_t n = 0; n < n_slots; ++n) {
            const unsigned long long cur = t.slots[slot].tag;
            if (cur == rec.tag) { found = true; break; }
            if (cur == 0) break;
            slot = (slot + 1) & t.slot_mask;
        }
        if (!found) { fault = SKM_ERR_STATE; continue; }              // (claim has reported it: the set was full)
        const UmiSlot entry = t.slots[slot];
        if (entry.class_key != rec.key || entry.umi != rec.umi) { fault = SKM_ERR_COLLISION; continue; }
        if (entry.min_unit == (unsigned long long)rec.local) {        // the molecule's first unit stays
            if (!NEAR) continue;
            if (!umi_near_earlier(t, rec, L, n_slots)) continue;      // ... unless an earlier unit was one substitution away
            ++near;
            // none of the molecule's units stays now (the others left for this one).  This lane alone stores the word,
            // nobody reads it in this launch, and later launches bring larger units only: final.
            if constexpr (NEAR) t.slots[slot].dropped = 1;
        }
        b.rec_key[r] = 0;
        b.rec_tuple[r] &= (1ULL << 40) - 1;       // tuple length 0: unaligned to everything that follows
        if (b.keep_spans) { b.unit_begin[unit] = 0; b.unit_end[unit] = -K; }             // fragment length rule: 0, not counted
        if (one_sample) atomicAdd(&s_removed, 1u);
        else atomicAdd(&removed[rec.sample], 1ULL);
    }
    if (held >= 0) flush();
    if (fault) atomicExch(t.error, fault);
    if constexpr (NEAR) {
        if (near) atomicAdd(&s_near, near);
        __syncthreads();
        if (threadIdx.x == 0 && s_near) atomicAdd(t.ctl + UMI_CTL_NEAR, (unsigned long long)s_near);
    }
}

// one lane per old slot: the 32 bytes move to the slot their tag finds in the new table
__global__ void __launch_bounds__(256)
umi_rehash_kernel(UmiSet from, UmiSet to)
{
    const uint64_t n_from = from.slot_mask + 1, n_to = to.slot_mask + 1;
    bool lost = false;
    for (uint64_t i = blockIdx.x * 256ULL + threadIdx.x; i < n_from; i += gridDim.x * 256ULL) {
        const UmiSlot entry = from.slots[i];
        if (entry.tag == 0) continue;
        uint64_t slot = entry.tag & to.slot_mask;
        bool placed = false;
        for (uint64_t n = 0; n < n_to; ++n) {
            if (atomicCAS(&to.slots[slot].tag, 0ULL, entry.tag) == 0ULL) { placed = true; break; }
            slot = (slot + 1) & to.slot_mask;
        }
        if (!placed) { lost = true; continue; }
        to.slots[slot].class_key = entry.class_key;
        to.slots[slot].umi = entry.umi;
        to.slots[slot].dropped = entry.dropped;
        to.slots[slot].min_unit = entry.min_unit;
    }
    if (lost) atomicExch(to.error, SKM_ERR_STATE);
}

unsigned umi_grid(int64_t n)
{
    return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 2048);
}

}  // namespace

void launch_umi_windows(const BarcodeWindows &w, int length, int32_t *cell, uint32_t *umi, unsigned long long *n_unreadable,
                        hipStream_t stream)
{
    if (w.n_reads <= 0) return;
    hipLaunchKernelGGL(umi_window_kernel, dim3(umi_grid(w.n_reads)), dim3(256), 0, stream, w, length, cell, umi, n_unreadable);
}

void launch_umi_init(const UmiSet &t, hipStream_t stream)
{
    hipLaunchKernelGGL(umi_init_kernel, dim3(umi_grid((int64_t)(t.slot_mask + 1))), dim3(256), 0, stream, t.slots, t.slot_mask + 1);
}

void launch_umi_claim(const UmiSet &t, const MapBatch &b, const SampleSalt &salt, const UmiSegment *segs, hipStream_t stream)
{
    if (b.n_units <= 0 || salt.n_segments <= 0) return;
    const int64_t lanes = (b.n_units + UMI_WIDTH - 1) / UMI_WIDTH;
    hipLaunchKernelGGL(umi_claim_kernel, dim3(umi_grid(lanes)), dim3(256), 0, stream, t, b.rec_unit, b.rec_key, b.n_units,
                       salt.seg_first, salt.seg_sample, segs, (int)salt.n_segments);
}

void launch_umi_resolve(const UmiSet &t, const MapBatch &b, const SampleSalt &salt, const UmiSegment *segs,
                        unsigned long long *removed, int umi_bases, int mismatches, hipStream_t stream)
{
    if (b.n_units <= 0 || salt.n_segments <= 0) return;
    const int64_t blocks = (b.n_units + UMI_RESOLVE_RUN - 1) / UMI_RESOLVE_RUN;       // (at most 2^21 units a launch)
    if (mismatches)
        hipLaunchKernelGGL((umi_resolve_kernel<true, int>), dim3((unsigned)blocks), dim3(256), 0, stream, t, b, salt.seg_first,
                           salt.seg_sample, segs, (int)salt.n_segments, removed, std::min(std::max(umi_bases, 0), 16));
    else
        hipLaunchKernelGGL(umi_resolve_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, t, b, salt.seg_first,
                           salt.seg_sample, segs, (int)salt.n_segments, removed);
}

void launch_umi_rehash(const UmiSet &from, const UmiSet &to, hipStream_t stream)
{
    launch_umi_init(to, stream);
    hipLaunchKernelGGL(umi_rehash_kernel, dim3(umi_grid((int64_t)(from.slot_mask + 1))), dim3(256), 0, stream, from, to);
}

}  // namespace skm
