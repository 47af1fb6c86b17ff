// C ABI of libseekmer_hip.so: quantification -- effective lengths, the skm_quant handle and the EM drivers,
// bootstrap and blend, the sample sets' shared EM launches, and RCCL with the skm_comm handle.
#include "skm_abi_samples.h"

#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

using namespace skm;
using namespace skm::abi;

// The whole table's transcript-major rows as their readers get them (QuantRowsHolder::get)
struct QuantRowsView {
    int64_t n_rows;
    const int64_t *row_start;     // [n_rows + 1]
    const int32_t *row_tx;        // [n_rows]
    const int32_t *tx_cls;        // [M]
    const int64_t *tx_row;        // [T + 1]
    unsigned int *arrivals;       // [T], zero between steps (EmProblem::arrivals)
};

// The rows of a handle, built when a reader first asks (the tile EM reads none of them: a handle whose table is
// tiles alone never builds them).  Nothing but get() reaches the arrays, so every reader goes through it.
class QuantRowsHolder {
public:
    // the rows, built now if they are not (the pair sort and the row kernels on the handle's stream, the cleared
    // arrival counters with them).  The caller holds the handle's mutex (or owns the handle alone) and has set
    // the device.
    int get(skm_quant *q, QuantRowsView &view);
    bool built() const { return built_; }
    void reset() { built_ = false; n_rows_ = 0; }      // (the class table changes: the set driver's next group)
private:
    DBuf<int64_t> row_start_, tx_row_;
    DBuf<int32_t> tx_cls_, row_tx_;
    DBuf<unsigned int> arrivals_;
    int64_t n_rows_ = 0;
    bool built_ = false;
};

struct skm_quant {
    ~skm_quant()                              // (the buffers go once the stream has drained)
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    int device = 0;
    PoolStream stream;
    PoolTimingEvent ev[2];
    PoolEvent chunk_ev[2];
    PoolPinned pinned;                        // host-pinned readback of the control block
    std::mutex mu;
    int64_t n_tx = 0, n_classes = 0, n_ids = 0;
    DBuf<int64_t> cls_offset;
    DBuf<int32_t> ids, perm;                      // perm[k] = caller's index of internal class k
    QuantRowsHolder rows;                         // the transcript-major rows, on first use
    DBuf<double> cls_count, cls_count_saved, inner, row_sum;
    DBuf<double> eff_len, x0, x1, acc, part_max;
    DBuf<unsigned int> part_flags;
    DBuf<unsigned long long> ctl, cum;
    DBuf<unsigned int> tile_total;            // scratch of the tiled multinomial draw
    DBuf<double> x_start, boot_out;           // bootstrap: the common start vector, the replicates' results
    // working set of the batched EM (skm_em_batch.hip): eight problems of this class structure side by side
    struct Batch {
        DBuf<double> cls_count, inner, row_sum, x0, x1, part_max;
        DBuf<unsigned int> part_flags;
        DBuf<unsigned long long> ctl, mgr;
        DBuf<double> counts_all;              // [group][C] class counts of a group of problems (internal class order)
        DBuf<double> totals;                  // [group][2] their sums (pairs, as launch_np_sum_many leaves them)
        DBuf<int64_t> iters;                  // [group] their step counts
    } batch;
    // the component tiles of the class table (EmTiles, skm_kernels.h): built with the class views
    struct Tiles {
        DBuf<int64_t> tile_tx, tile_cls, cls_pair, tx_pair;
        DBuf<int32_t> tx_list, cls_list, tx_label, tx_tile, cls_tile;
        DBuf<int32_t> order;                  // [T + 1] the tiles by descending pair count: the launch order
        DBuf<uint16_t> cls_tx, tx_cls;
        DBuf<double> snap, step_max;          // snap: [EM_CHUNK_MAX][T] every step's abundances of the chunk in flight
        DBuf<unsigned int> step_flags;
        // the components above the capacity as an EM problem beside the tiles (QuantResidual)
        struct Residual {
            int64_t n_classes = 0, n_ids = 0, n_rows = 0;
            DBuf<int64_t> cls_offset, row_start, tx_row;
            DBuf<int32_t> ids, cls_src, row_tx, tx_cls;
            DBuf<double> cls_count, inner, row_sum;
            bool built = false;
        } residual;
        bool built = false;                   // the set-up has run
        int64_t n_tiles = 0, n_oversize = 0;  // n_oversize: components above the tile capacity (then the tiles are not used)
    } tiles;
    double n_total = 0;
    bool n_total_reduced = false;             // n_total already is the sum over all ranks
    // RCCL communicator (borrowed from an skm_comm), loaded lazily
    void *comm = nullptr;
    int rank = 0, world = 1;
    double t_em_ns = 0, iters_total = 0, launches = 0;
};

struct skm_comm {
    int device = 0;
    void *comm = nullptr;
    int rank = 0, world = 1;
};

// ------------------------------------------------------------ quantification
extern "C" int skm_effective_lengths(int device, const int64_t *fld, const double *lengths,
                                     int64_t n_tx, double *out)
{
    if (!fld || !lengths || !out || n_tx < 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(check_device(device));
    SKM_TRY(set_device(device));
    if (n_tx == 0) return SKM_OK;
    DBuf<unsigned long long> d_fld; DBuf<double> d_len, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_fld.ensure(MAX_FRAGMENT_LENGTH)); SKM_TRY(d_len.ensure(n_tx)); SKM_TRY(d_out.ensure(n_tx));
    HIP_TRY(hipMemcpy(d_fld.p, fld, MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len.p, lengths, n_tx * 8, hipMemcpyHostToDevice));
    launch_effective_lengths(d_fld.p, d_len.p, n_tx, d_out.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, n_tx * 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copy home has waited for the kernel)
    return SKM_OK;
}

namespace {

// rows per group of n > 0 rows of 2000 words in, n_tx > 0 words out: 256 MB of output rows and of input rows
// at most (16 777 rows: one launch's gridDim.y holds them); SKM_EFF_MANY_GROUP (tests): fewer
int64_t effective_lengths_group(int64_t n, int64_t n_tx)
{
    int64_t group = std::min<int64_t>((int64_t)(1LL << 25) / n_tx, (int64_t)(1LL << 25) / MAX_FRAGMENT_LENGTH);
    if (const char *v = getenv("SKM_EFF_MANY_GROUP"))
        if (atoll(v) > 0) group = std::min<int64_t>(group, atoll(v));
    return std::max<int64_t>(1, std::min(group, n));
}

// out[n][n_tx] from n > 0 rows of 2000 words (histograms or weights, 8 bytes a word: what `launch` takes), n_tx > 0:
// groups of rows, so that the rows staged in HBM, in and out, stay within 256 MB each (as many_rows_in); the lengths
// go up once.  The device is set.
template <class Row>
int effective_lengths_grouped(int64_t n, const Row *rows, const double *lengths, int64_t n_tx, double *out,
                              void (*launch)(const Row *, int64_t, const double *, int64_t, double *, hipStream_t))
{
    const int64_t group = effective_lengths_group(n, n_tx);
    DBuf<Row> d_rows; DBuf<double> d_len, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_rows.ensure((size_t)group * MAX_FRAGMENT_LENGTH)); SKM_TRY(d_len.ensure(n_tx)); SKM_TRY(d_out.ensure((size_t)(group * n_tx)));
    HIP_TRY(hipMemcpy(d_len.p, lengths, n_tx * 8, hipMemcpyHostToDevice));
    for (int64_t first = 0; first < n; first += group) {
        const int64_t here = std::min(group, n - first);
        HIP_TRY(hipMemcpy(d_rows.p, rows + first * MAX_FRAGMENT_LENGTH, (size_t)here * MAX_FRAGMENT_LENGTH * 8, hipMemcpyHostToDevice));
        launch(d_rows.p, here, d_len.p, n_tx, d_out.p, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + first * n_tx, d_out.p, (size_t)(here * n_tx) * 8, hipMemcpyDeviceToHost));
    }
    drain.dismiss();                          // (the copies home have waited for the kernels)
    return SKM_OK;
}

}  // namespace

// One row of effective lengths per histogram (the counts go to the device as the unsigned words the kernel reads).
extern "C" int skm_effective_lengths_many(int device, int64_t n, const int64_t *fld, const double *lengths,
                                          int64_t n_tx, double *out)
{
    if (n < 0 || n_tx < 0 || (n && (!fld || (n_tx && (!lengths || !out))))) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(check_device(device));
    SKM_TRY(set_device(device));
    if (n == 0 || n_tx == 0) return SKM_OK;
    return effective_lengths_grouped(n, (const unsigned long long *)fld, lengths, n_tx, out, launch_effective_lengths_many);
}

// The same rule for n rows of given weights, grouped as the histograms above.
extern "C" int skm_effective_lengths_weights(int device, int64_t n, const double *p, const double *lengths,
                                             int64_t n_tx, double *out)
{
    if (n < 0 || n_tx < 0 || !p || !lengths || !out) return fail(SKM_ERR_ARG, "bad argument");
    if (!length_weights_valid(p, n * MAX_FRAGMENT_LENGTH))
        return fail(SKM_ERR_ARG, "a fragment-length weight is negative or not finite");
    SKM_TRY(check_device(device));
    SKM_TRY(set_device(device));
    if (n == 0 || n_tx == 0) return SKM_OK;
    return effective_lengths_grouped(n, p, lengths, n_tx, out, launch_effective_lengths_weights);
}

namespace {

// SKM_EM_NO_COMPONENTS (tuning aid, looked up at every use so that one process can compare both forms):
// no component tiles are built, and an EM run steps the whole table with two launches per step
bool em_components_enabled() { return getenv("SKM_EM_NO_COMPONENTS") == nullptr; }
// what an EM run needs besides the handle's own state to step tiles: one rank (the all-reduce of several
// sits inside every step) and the fused rows + finalize launch (the unfused finalize walks every transcript)
bool em_tiles_possible(bool several_ranks)
{
    static const bool unfused = getenv("SKM_EM_UNFUSED") != nullptr;
    return !several_ranks && !unfused && em_components_enabled();
}

// several_ranks: the handle gets a communicator right after this call; the tiles, which only a one-rank EM
// can use, are then neither given room here nor built by quant_finish_setup
int quant_alloc(skm_quant *q, int device, int64_t n_tx, int64_t n_classes, int64_t n_ids, bool several_ranks = false)
{
    STALE_CHECK("quant_alloc entry");
    q->device = device;
    q->n_tx = n_tx;
    q->n_classes = n_classes;
    q->n_ids = n_ids;
    HIP_TRY(pool_stream_acquire(q->stream.out()));
    for (auto &e : q->ev) HIP_TRY(pool_event_acquire(e.out(), true));
    for (auto &e : q->chunk_ev) HIP_TRY(pool_event_acquire(e.out(), false));
    HIP_TRY(pool_pinned_acquire((void **)q->pinned.out()));
    const size_t C = (size_t)std::max<int64_t>(n_classes, 1), M = (size_t)std::max<int64_t>(n_ids, 1);
    const size_t T = (size_t)std::max<int64_t>(n_tx, 1);
    const size_t R = (size_t)quant_rows_upper_bound(n_tx, n_ids);
    SKM_TRY(q->cls_offset.ensure(C + 1));
    SKM_TRY(q->cls_count.ensure(C));
    SKM_TRY(q->inner.ensure(C));
    SKM_TRY(q->ids.ensure(M));
    SKM_TRY(q->perm.ensure(C));
    SKM_TRY(q->row_sum.ensure(R));
    SKM_TRY(q->eff_len.ensure(T));
    SKM_TRY(q->x0.ensure(T));
    SKM_TRY(q->x1.ensure(T));
    SKM_TRY(q->acc.ensure(T));
    SKM_TRY(q->ctl.ensure(EM_CTL_WORDS + EM_JUDGE_WORDS));       // (the tile judge's words lie behind the control block)
    SKM_TRY(q->part_max.ensure(EM_FINAL_BLOCKS));
    SKM_TRY(q->part_flags.ensure(EM_FINAL_BLOCKS));
    if (em_tiles_possible(several_ranks)) {
        auto &t = q->tiles;
        SKM_TRY(t.tile_tx.ensure(T + 2)); SKM_TRY(t.tile_cls.ensure(T + 2));
        SKM_TRY(t.cls_pair.ensure(C + 1)); SKM_TRY(t.tx_pair.ensure(T + 1));
        SKM_TRY(t.tx_list.ensure(T)); SKM_TRY(t.cls_list.ensure(C));
        SKM_TRY(t.tx_label.ensure(T)); SKM_TRY(t.tx_tile.ensure(T)); SKM_TRY(t.cls_tile.ensure(C));
        SKM_TRY(t.cls_tx.ensure(M)); SKM_TRY(t.tx_cls.ensure(M));
        SKM_TRY(t.order.ensure(T + 1));
    }
    STALE_CHECK("quant_alloc exit");
    return SKM_OK;
}

QuantBuild quant_build_view(skm_quant *q)
{
    QuantBuild b{};
    b.n_tx = q->n_tx;
    b.n_classes = q->n_classes;
    b.n_ids = q->n_ids;
    b.cls_offset = q->cls_offset.p;
    b.ids = q->ids.p;
    b.cls_count = q->cls_count.p;
    if (q->tiles.tile_tx.p) {                      // (quant_alloc made room for the tiles)
        auto &t = q->tiles;
        b.tile_tx = t.tile_tx.p; b.tile_cls = t.tile_cls.p;
        b.tx_list = t.tx_list.p; b.cls_list = t.cls_list.p;
        b.cls_pair = t.cls_pair.p; b.tx_pair = t.tx_pair.p;
        b.tile_cls_tx = t.cls_tx.p; b.tile_tx_cls = t.tx_cls.p;
        b.tx_label = t.tx_label.p; b.tx_tile = t.tx_tile.p; b.cls_tile = t.cls_tile.p;
        b.tile_order = t.order.p;
    }
    return b;
}

}  // namespace

int QuantRowsHolder::get(skm_quant *q, QuantRowsView &view)
{
    if (!built_) {
        const size_t M = (size_t)std::max<int64_t>(q->n_ids, 1), T = (size_t)std::max<int64_t>(q->n_tx, 1);
        const size_t R = (size_t)quant_rows_upper_bound(q->n_tx, q->n_ids);
        SKM_TRY(tx_cls_.ensure(M));
        SKM_TRY(tx_row_.ensure(T + 1));
        SKM_TRY(row_start_.ensure(R + 1));
        SKM_TRY(row_tx_.ensure(R));
        SKM_TRY(arrivals_.ensure(T));
        HIP_TRY(hipMemsetAsync(arrivals_.p, 0, T * sizeof(unsigned int), q->stream));
        const QuantBuild b = quant_build_view(q);
        QuantRows r{};
        r.tx_cls = tx_cls_.p; r.tx_row = tx_row_.p; r.row_start = row_start_.p; r.row_tx = row_tx_.p;
        r.n_rows_cap = (int64_t)std::min(row_tx_.cap, row_start_.cap - 1);
        const int64_t n = quant_rows_build(b, r, q->stream);
        if (n < 0) return fail(SKM_ERR_HIP, "building the transcript-major rows failed (%lld): %s", (long long)n, quant_setup_failure());
        n_rows_ = n;
        built_ = true;
    }
    view.n_rows = n_rows_;
    view.row_start = row_start_.p; view.row_tx = row_tx_.p; view.tx_cls = tx_cls_.p; view.tx_row = tx_row_.p;
    view.arrivals = arrivals_.p;
    return SKM_OK;
}

namespace {

int quant_finish_setup(skm_quant *q, const ClassTable *table, int64_t units_seen = -1)
{
    STALE_CHECK("quant_finish_setup");
    QuantBuild b = quant_build_view(q);
    b.first_seen_bound = units_seen > 0 ? units_seen : 0;      // first-seen values are unit indices below this
    q->rows.reset();
    const int rc = quant_setup(table, b, q->perm.p, q->stream);
    if (rc < 0) return fail(SKM_ERR_HIP, "building the class views failed (%d): %s", rc, quant_setup_failure());
    if (b.tile_tx) {
        q->tiles.built = true;
        q->tiles.n_tiles = b.tile_info[0];
        q->tiles.n_oversize = b.tile_info[1];
        if (q->tiles.n_tiles > 0) {
            SKM_TRY(q->tiles.step_max.ensure((size_t)(EM_CHUNK_MAX * q->tiles.n_tiles)));
            SKM_TRY(q->tiles.step_flags.ensure((size_t)(EM_CHUNK_MAX * q->tiles.n_tiles)));
            SKM_TRY(q->tiles.snap.ensure((size_t)EM_CHUNK_MAX * (size_t)q->n_tx));
        }
        if (q->tiles.n_oversize > 0 && q->tiles.n_tiles > 0) {
            // tiles AND components above the capacity: those become the residual problem (a table that
            // is one such component has no tiles and keeps the whole-table EM as it is)
            // (the residual is cut out of the whole table's rows: this handle builds them now)
            auto &r = q->tiles.residual;
            QuantRowsView rv{};
            SKM_TRY(q->rows.get(q, rv));
            QuantRows whole{};
            whole.tx_cls = const_cast<int32_t *>(rv.tx_cls); whole.tx_row = const_cast<int64_t *>(rv.tx_row);
            whole.row_start = const_cast<int64_t *>(rv.row_start); whole.row_tx = const_cast<int32_t *>(rv.row_tx);
            whole.n_rows_cap = rv.n_rows;
            int64_t counts[3] = {0, 0, 0};
            if (quant_residual_count(b, whole, counts, q->stream))
                return fail(SKM_ERR_HIP, "sizing the residual EM problem failed: %s", quant_setup_failure());
            r.n_classes = counts[0]; r.n_ids = counts[1]; r.n_rows = counts[2];
            SKM_TRY(r.cls_offset.ensure((size_t)r.n_classes + 1)); SKM_TRY(r.ids.ensure((size_t)std::max<int64_t>(r.n_ids, 1)));
            SKM_TRY(r.cls_src.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.row_start.ensure((size_t)r.n_rows + 1)); SKM_TRY(r.row_tx.ensure((size_t)std::max<int64_t>(r.n_rows, 1)));
            SKM_TRY(r.tx_cls.ensure((size_t)std::max<int64_t>(r.n_ids, 1))); SKM_TRY(r.tx_row.ensure((size_t)q->n_tx + 1));
            SKM_TRY(r.cls_count.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.inner.ensure((size_t)std::max<int64_t>(r.n_classes, 1)));
            SKM_TRY(r.row_sum.ensure((size_t)std::max<int64_t>(r.n_rows, 1)));
            QuantResidual out{};
            out.n_classes = r.n_classes; out.n_ids = r.n_ids; out.n_rows = r.n_rows;
            out.cls_offset = r.cls_offset.p; out.ids = r.ids.p; out.cls_src = r.cls_src.p;
            out.row_start = r.row_start.p; out.row_tx = r.row_tx.p; out.tx_cls = r.tx_cls.p; out.tx_row = r.tx_row.p;
            if (quant_residual_build(b, whole, out, q->stream))
                return fail(SKM_ERR_HIP, "building the residual EM problem failed: %s", quant_setup_failure());
            r.built = true;
        }
    }
    return SKM_OK;
}

// ---- RCCL through dlopen: the library is only needed for N > 1
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;      // (table hand-over; optional)
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
};
struct UniqueId { char internal[128]; };
typedef int (*comm_init_fn)(void **, int, UniqueId, int);
Rccl g_rccl;
comm_init_fn g_comm_init = nullptr;

int load_rccl()
{
    if (g_rccl.lib) return SKM_OK;
    void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(SKM_ERR_COMM, "cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(lib, "ncclGetUniqueId");
    g_comm_init = (comm_init_fn)dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(lib, "ncclCommDestroy");
    g_rccl.CommCount = (int (*)(void *, int *))dlsym(lib, "ncclCommCount");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(lib, "ncclGetErrorString");
    g_rccl.Send = (int (*)(const void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclSend");
    g_rccl.Recv = (int (*)(void *, size_t, int, int, void *, hipStream_t))dlsym(lib, "ncclRecv");
    g_rccl.GroupStart = (int (*)())dlsym(lib, "ncclGroupStart");
    g_rccl.GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
    if (!g_rccl.GetUniqueId || !g_comm_init || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(SKM_ERR_COMM, "librccl.so lacks a required symbol");
    g_rccl.lib = lib;
    return SKM_OK;
}

constexpr int NCCL_FLOAT64 = 8, NCCL_UINT64 = 5, NCCL_INT32 = 2, NCCL_SUM = 0;

#define NCCL_TRY(call)                                                                   \
    do {                                                                                 \
        int r_ = (call);                                                                 \
        if (r_ != 0)                                                                     \
            return fail(SKM_ERR_COMM, "%s failed: %s", #call,                            \
                        g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?");        \
    } while (0)

EmProblem em_problem(skm_quant *q, double rel_tol, double x_floor, int64_t max_iters,
                     int64_t fixed_iters)
{
    EmProblem p{};
    p.n_tx = q->n_tx;
    p.n_classes = q->n_classes;
    p.cls_offset = q->cls_offset.p;
    p.ids = q->ids.p;
    p.cls_count = q->cls_count.p;
    p.inner = q->inner.p;
    p.row_sum = q->row_sum.p;
    p.eff_len = q->eff_len.p;
    p.x[0] = q->x0.p;
    p.x[1] = q->x1.p;
    p.acc = q->acc.p;
    p.n_total = q->n_total;
    p.rel_tol = rel_tol;
    p.x_floor = x_floor;
    p.ctl = q->ctl.p;
    p.part_max = q->part_max.p;
    p.part_flags = q->part_flags.p;
    p.max_iters = max_iters;
    p.fixed_iters = fixed_iters;
    static const bool unfused = getenv("SKM_EM_UNFUSED") != nullptr;     // tuning aid: rows and finalize as two launches
    p.fused = q->comm || unfused ? 0 : 1;      // (several ranks: the all-reduce sits between rows and finalize)
    return p;
}

// the whole table's rows into the problem, for the kernels that step the whole table (built now if no reader
// has asked before); em_problem leaves them out: the tile EM of a table without a residual reads none
int em_problem_rows(skm_quant *q, EmProblem &p)
{
    QuantRowsView rv{};
    SKM_TRY(q->rows.get(q, rv));
    p.n_rows = rv.n_rows;
    p.row_start = rv.row_start; p.row_tx = rv.row_tx; p.tx_cls = rv.tx_cls; p.tx_row = rv.tx_row;
    p.arrivals = rv.arrivals;
    return SKM_OK;
}

// one rank, every component within the tile capacity: the EM runs tile by tile in LDS (em_run_tiles)
bool em_uses_tiles(const skm_quant *q)
{
    return em_tiles_possible(q->comm != nullptr) && q->tiles.built && q->tiles.n_tiles > 0 &&
           (q->tiles.n_oversize == 0 || q->tiles.residual.built);
}

// The host one chunk of steps ahead of the device.  enqueue(slot) queues a chunk and, behind it, the copy
// of what the host reads about it to q->pinned + 8 * slot; chunk i + 1 is already queued when the host
// waits for chunk i's words, so the GPU never idles at a check-point (a converged EM turns at most one
// chunk of launches into no-ops).  Returns once stopped(words) says so, with the look-ahead chunk still
// queued and `words` those of the chunk that stopped.
template <class Enqueue, class Stopped>
int em_run_chunks_ahead(skm_quant *q, unsigned long long (&words)[8], Enqueue enqueue, Stopped stopped)
{
    auto enqueue_chunk = [&](int slot) -> int {
        SKM_TRY(enqueue(slot));
        HIP_TRY(hipEventRecord(q->chunk_ev[slot], q->stream));
        return SKM_OK;
    };
    SKM_TRY(enqueue_chunk(0));
    for (int slot = 0;; slot ^= 1) {
        SKM_TRY(enqueue_chunk(slot ^ 1));                 // stay one chunk ahead
        HIP_TRY(hipEventSynchronize(q->chunk_ev[slot]));
        memcpy(words, q->pinned + 8 * slot, sizeof(words));
        if (stopped(words)) return SKM_OK;
    }
}
bool em_ctl_done(const unsigned long long *ctl) { return ctl[CTL_DONE] != 0; }

// The component form of em_run's loop (after its preamble: control block cleared, ev[0] recorded).  Every
// chunk is ONE launch that steps all the tiles `chunk` times in LDS and leaves every step's abundances in
// the snapshot buffer -- the next chunk starts from the last of them -- and judges the chunk's steps in order
// itself (beside a residual problem: that problem's judge does).  The host stays one chunk ahead as before;
// the look-ahead chunk that finds the EM stopped (at step K) copies the tiles' entries of step K from the snapshots to x[K & 1],
// where the callers look for the result: no step runs twice and the stop costs no launch of its own.
int em_run_tiles(skm_quant *q, const EmProblem &p, int64_t chunk, int64_t *iters_out)
{
    auto &t = q->tiles;
    EmTiles tl{};
    tl.n_tiles = t.n_tiles;
    tl.tile_tx = t.tile_tx.p; tl.tile_cls = t.tile_cls.p;
    tl.tx_list = t.tx_list.p; tl.cls_list = t.cls_list.p;
    tl.cls_pair = t.cls_pair.p; tl.tx_pair = t.tx_pair.p;
    tl.cls_tx = t.cls_tx.p; tl.tx_cls = t.tx_cls.p;
    tl.step_max = t.step_max.p; tl.step_flags = t.step_flags.p;
    tl.snap = t.snap.p;
    // SKM_EM_TILE_ORDER (tuning aid, looked up at every run as SKM_EM_NO_COMPONENTS is): `identity` launches the
    // tiles in tile order, `reverse` smallest first; unset: largest first.  The results are the same bits.
    tl.order = t.order.p;
    if (const char *form = getenv("SKM_EM_TILE_ORDER")) {
        if (!strcmp(form, "identity")) tl.order = nullptr;
        else if (!strcmp(form, "reverse")) tl.order_reversed = 1;
        else return fail(SKM_ERR_ARG, "SKM_EM_TILE_ORDER is identity or reverse, not '%s'", form);
    }
    // With components above the capacity the residual problem runs beside the tiles, step by step with
    // the whole-table kernels on its own classes and rows (its transcripts' entries of x0 / x1; the
    // tiles' entries are the tiles' alone), and ITS judge takes the tiles' partials of the step along.
    const bool mixed = t.n_oversize > 0;
    // Tiles alone: the chunk launch judges its own steps (the workgroup that finishes last does), one launch a chunk.
    if (!mixed && !SKM_EM_JUDGE_LAUNCH) tl.judge = q->ctl.p + EM_CTL_WORDS;
    EmProblem pr = p;
    if (mixed) {
        auto &r = t.residual;
        pr.n_classes = r.n_classes; pr.n_rows = r.n_rows;
        pr.cls_offset = r.cls_offset.p; pr.ids = r.ids.p; pr.cls_count = r.cls_count.p; pr.inner = r.inner.p;
        pr.row_start = r.row_start.p; pr.row_tx = r.row_tx.p; pr.tx_cls = r.tx_cls.p; pr.tx_row = r.tx_row.p;
        pr.row_sum = r.row_sum.p;
        pr.fused = 1;
        pr.extra_max = t.step_max.p; pr.extra_flags = t.step_flags.p; pr.n_extra = t.n_tiles;
        launch_permute_f64(q->cls_count.p, r.cls_src.p, r.n_classes, r.cls_count.p, false, q->stream);   // (set_counts may have changed them)
    }
    int64_t queued = 0;
    auto enqueue_chunk = [&](int slot) -> int {
        launch_em_local_chunk(p, tl, queued == 0 ? q->x0.p : t.snap.p + (chunk - 1) * q->n_tx, (int)chunk, queued * chunk, q->stream);
        if (mixed) {
            pr.extra_first = queued * chunk;
            for (int64_t i = 0, k = queued * chunk; i < chunk; ++i, ++k) {
                launch_em_inner(pr, (int)(k & 1), i > 0, k, q->stream);
                launch_em_rows_finalize(pr, (int)(k & 1), q->stream);
            }
            launch_em_decide(pr, (queued + 1) * chunk, q->stream);
            q->launches += 2 * chunk + 2;
        } else {
#if SKM_EM_JUDGE_LAUNCH
            launch_em_local_decide(p, tl, queued * chunk, (int)chunk, q->stream);
            q->launches += 1;
#endif
            q->launches += 1;
        }
        ++queued;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, q->ctl.p, 8 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long ctl[8] = {0};
    SKM_TRY(em_run_chunks_ahead(q, ctl, enqueue_chunk, em_ctl_done));
    // (a tile above the capacity cannot come out of the set-up; the kernel that meets one leaves it alone,
    // says so here and stops the run rather than going on with abundances nobody stepped)
    if (ctl[CTL_TILE_FAULT]) {
        HIP_TRY(hipStreamSynchronize(q->stream));
        return fail(SKM_ERR_STATE, "a component tile exceeds the tile capacity: the class views of this handle are damaged");
    }
    // (the look-ahead chunk, queued above, is the copy of step `steps` of the tiles to x[steps & 1])
    const int64_t steps = (int64_t)ctl[CTL_ITERS];
    HIP_TRY(hipEventRecord(q->ev[1], q->stream));
    HIP_TRY(hipEventSynchronize(q->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
    q->t_em_ns += ms * 1e6;
    q->iters_total += (double)steps;
    if (iters_out) *iters_out = steps;
    if (ctl[CTL_UNDEFINED]) return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
    return SKM_OK;
}

// runs the EM from the abundance already in q->x0; result left in x[iters & 1]
int em_run(skm_quant *q, double rel_tol, double x_floor, int64_t max_iters, int64_t fixed_iters,
           int64_t *iters_out, int64_t chunk_steps = 16)
{
    // n = class_count.sum() over ALL ranks (infer.py:152)
    double n_total = q->n_total;
    if (q->comm && !q->n_total_reduced) {
        HIP_TRY(hipMemcpyAsync(q->acc.p, &n_total, 8, hipMemcpyHostToDevice, q->stream));
        NCCL_TRY(g_rccl.AllReduce(q->acc.p, q->acc.p, 1, NCCL_FLOAT64, NCCL_SUM, q->comm, q->stream));
        HIP_TRY(hipMemcpyAsync(&n_total, q->acc.p, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
    }
    EmProblem p = em_problem(q, rel_tol, x_floor, max_iters, fixed_iters);
    p.n_total = n_total;
    const int64_t chunk = fixed_iters > 0 ? std::min<int64_t>(fixed_iters, chunk_steps) : chunk_steps;
    const bool by_tiles = em_uses_tiles(q) && chunk <= EM_CHUNK_MAX;
    // (the rows: for the whole-table steps, and beside tiles for the residual's launches, whose arrival counters
    // are the whole table's -- built with the residual at the set-up)
    if (!by_tiles || q->tiles.n_oversize > 0) SKM_TRY(em_problem_rows(q, p));
    // (with the control block the tile judge's words behind it: a run that ended in a tile fault or an error
    // leaves nothing there)
    HIP_TRY(hipMemsetAsync(q->ctl.p, 0, (EM_CTL_WORDS + EM_JUDGE_WORDS) * sizeof(unsigned long long), q->stream));
    int64_t k = 0;
    HIP_TRY(hipEventRecord(q->ev[0], q->stream));
    if (by_tiles) return em_run_tiles(q, p, chunk, iters_out);
    // Steps are enqueued in chunks, the control block copied to pinned memory behind each (em_run_chunks_ahead).
    static const bool unfused_rows = getenv("SKM_EM_UNFUSED") != nullptr;
    auto enqueue_chunk = [&](int slot) -> int {
        for (int64_t i = 0; i < chunk; ++i, ++k) {
            // (the first step of a chunk follows the chunk-end em_decide: already judged)
            launch_em_inner(p, (int)(k & 1), i > 0, k, q->stream);
            if (q->comm) {
                // rows -> this rank's numerators (one launch, or two with SKM_EM_UNFUSED), summed over
                // the ranks, then the finalize on every rank alike
                if (unfused_rows) {
                    launch_em_rows(p, (int)(k & 1), q->stream);
                    launch_em_rows_to_acc(p, q->stream);
                } else {
                    launch_em_rows_acc(p, (int)(k & 1), q->stream);
                }
                NCCL_TRY(g_rccl.AllReduce(q->acc.p, q->acc.p, (size_t)q->n_tx, NCCL_FLOAT64, NCCL_SUM,
                                          q->comm, q->stream));
                launch_em_finalize(p, (int)(k & 1), true, q->stream);
            } else if (p.fused) {
                launch_em_rows_finalize(p, (int)(k & 1), q->stream);     // (rows + finalize: one launch)
            } else {
                launch_em_rows(p, (int)(k & 1), q->stream);
                launch_em_finalize(p, (int)(k & 1), false, q->stream);
            }
            q->launches += q->comm ? (unfused_rows ? 4 : 3) : (p.fused ? 2 : 3);
        }
        launch_em_decide(p, k, q->stream);
        q->launches += 1;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, q->ctl.p, 8 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long ctl[8] = {0};
    SKM_TRY(em_run_chunks_ahead(q, ctl, enqueue_chunk, em_ctl_done));
    HIP_TRY(hipStreamSynchronize(q->stream));             // drain the look-ahead chunk (no-ops)
    HIP_TRY(hipEventRecord(q->ev[1], q->stream));
    HIP_TRY(hipEventSynchronize(q->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
    q->t_em_ns += ms * 1e6;
    q->iters_total += (double)ctl[CTL_ITERS];
    if (iters_out) *iters_out = (int64_t)ctl[CTL_ITERS];
    if (ctl[CTL_UNDEFINED]) return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
    return SKM_OK;
}

}  // namespace

namespace {

// numpy.sum of a contiguous f8 array on the host, bit for bit (blocks of 8192, pairwise inside;
// see np_sum_blocks_kernel): n = class_count.sum() of infer.py:152 for counts that are not
// integers (blended single-cell tables, impute.py:248-252)
double np_pairwise_host(const double *a, int64_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_host(a, n2) + np_pairwise_host(a + n2, n - n2);
}

double np_sum_host(const double *a, int64_t n)
{
    double acc = 0.0;
    for (int64_t i = 0; i < n; i += 8192) acc += np_pairwise_host(a + i, std::min<int64_t>(8192, n - i));
    return acc;
}

}  // namespace

extern "C" int skm_quant_create(int device, int64_t n_tx, int64_t n_classes,
                                const int64_t *class_offsets, const int32_t *class_targets,
                                const double *class_counts, skm_quant **out)
{
    if (!out || n_tx <= 0 || n_classes < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_classes && (!class_offsets || !class_targets || !class_counts))
        return fail(SKM_ERR_ARG, "NULL class arrays");
    SKM_TRY(check_device(device));
    const int64_t M = n_classes ? class_offsets[n_classes] - class_offsets[0] : 0;
    for (int64_t c = 0; c < n_classes; ++c)
        if (class_offsets[c + 1] < class_offsets[c]) return fail(SKM_ERR_ARG, "class offsets are not monotone");
    const double total = np_sum_host(class_counts, n_classes);
    for (int64_t j = 0; j < M; ++j) {
        const int32_t t = class_targets[class_offsets[0] + j];
        if (t < 0 || t >= n_tx) return fail(SKM_ERR_ARG, "class target %d outside [0, n_tx)", t);
    }
    SKM_TRY(set_device(device));
    std::unique_ptr<skm_quant> q(new skm_quant());     // (any early return below: nothing is left behind)
    SKM_TRY(quant_alloc(q.get(), device, n_tx, n_classes, M));
    std::vector<int64_t> rebased(n_classes + 1, 0);
    for (int64_t c = 0; c <= n_classes && n_classes; ++c) rebased[c] = class_offsets[c] - class_offsets[0];
    HIP_TRY(hipMemcpy(q->cls_offset.p, rebased.data(), (n_classes + 1) * 8, hipMemcpyHostToDevice));
    if (n_classes) {
        HIP_TRY(hipMemcpy(q->cls_count.p, class_counts, n_classes * 8, hipMemcpyHostToDevice));
        if (M) HIP_TRY(hipMemcpy(q->ids.p, class_targets + class_offsets[0], M * 4, hipMemcpyHostToDevice));
    }
    q->n_total = total;
    SKM_TRY(quant_finish_setup(q.get(), nullptr));
    *out = q.release();                                 // (the caller's handle from here on)
    return SKM_OK;
}

extern "C" int skm_quant_create_from_mapper(skm_mapper *m, int64_t n_tx, skm_quant **out)
{
    if (!m || !out || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used;
    std::unique_ptr<skm_quant> q(new skm_quant());     // (any early return below: nothing is left behind)
    SKM_TRY(quant_alloc(q.get(), m->ix->device, n_tx, C, M));
    unsigned long long ctr[4];
    HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));
    q->n_total = (double)(ctr[CTR_UNITS] - ctr[CTR_UNALIGNED]);
    SKM_TRY(quant_finish_setup(q.get(), &m->t, m->first_seen_bound));
    *out = q.release();                                 // (the caller's handle from here on)
    return SKM_OK;
}

// One sample from the resident class table to TPM without leaving the device:
// fragment-length histogram (all-reduced over the ranks of `comm`) -> effective
// lengths (mapper.py:134-141) -> start vector 1/l normalised with numpy's sum
// (infer.py:116-119) -> EM to the stop rule (:133-168) -> TPM scaling (:127-129).
extern "C" int skm_quant_infer(skm_mapper *m, skm_comm *comm, const double *lengths, int64_t n_tx,
                               double rel_tol, double x_floor, int64_t max_iters,
                               double *tpm, double *effective_lengths, int64_t *iters)
{
    if (!m || !lengths || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(wait_jobs(m, 0, false));           // queued host batches first
    std::lock_guard<std::mutex> lock(m->mu);
    if (comm && comm->device != m->ix->device)
        return fail(SKM_ERR_ARG, "communicator and mapper live on different GPUs");
    SKM_TRY(set_device(m->ix->device));
    const int64_t C = m->host_classes, M = m->host_arena_used;
    // SKM_TRACE_INFER=1: host wall time between the phases below, on stderr (tuning aid)
    static const bool trace = getenv("SKM_TRACE_INFER") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[skm_quant_infer] %-12s %8.1f us\n", what,
                std::chrono::duration<double, std::micro>(now - t_last).count());
        t_last = now;
    };
    // (the scratch is declared before the handle: the handle's destructor drains the stream first)
    DBuf<unsigned long long> fld;
    DBuf<double> sums;
    std::unique_ptr<skm_quant> q(new skm_quant());
    SKM_TRY(quant_alloc(q.get(), m->ix->device, n_tx, C, M, comm != nullptr));
    if (comm) { q->comm = comm->comm; q->rank = comm->rank; q->world = comm->world; }
    lap("alloc");
    const int64_t n_blocks = (n_tx + 8191) / 8192;
    SKM_TRY(fld.ensure(MAX_FRAGMENT_LENGTH + 1));
    SKM_TRY(sums.ensure(n_blocks + 2));
    double *const total = sums.p + n_blocks;          // [0] sum, [1] sum / divisor
    unsigned long long ctr[4] = {0, 0, m->host_unaligned, m->host_units};
    if (!m->host_totals_valid)
        HIP_TRY(hipMemcpy(ctr, m->counters.p, sizeof(ctr), hipMemcpyDeviceToHost));   // (mapper stream is idle)
    unsigned long long aligned = ctr[CTR_UNITS] - ctr[CTR_UNALIGNED];
    HIP_TRY(hipMemcpyAsync(fld.p, m->counters.p + CTR_FLD, MAX_FRAGMENT_LENGTH * 8,
                           hipMemcpyDeviceToDevice, q->stream));
    if (q->comm) {
        // merge_fragment_lengths over the ranks, and with it (word 2000 of the same
        // collective) n = class_count.sum() of infer.py:152 over ALL ranks.  Whether there
        // is anything to quantify (infer.py:106-107 tests the merged table) must be decided
        // on the global sum: a rank whose shard produced no class still has to take part
        // in every collective of the EM below, with empty class views.
        q->pinned[32] = aligned;
        HIP_TRY(hipMemcpyAsync(fld.p + MAX_FRAGMENT_LENGTH, q->pinned + 32, 8, hipMemcpyHostToDevice, q->stream));
        NCCL_TRY(g_rccl.AllReduce(fld.p, fld.p, MAX_FRAGMENT_LENGTH + 1, NCCL_UINT64, NCCL_SUM, q->comm,
                                  q->stream));
        HIP_TRY(hipMemcpyAsync(q->pinned + 32, fld.p + MAX_FRAGMENT_LENGTH, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        aligned = q->pinned[32];
        q->n_total_reduced = true;
        // test hook: "the other ranks aligned this many units" -- a rank whose own shard produced no
        // class (C == 0) then goes through the set-up and every collective of the EM with empty
        // class views, a state one rank cannot reach by itself (tests/test_gpu_parity.py)
        if (const char *v = getenv("SKM_TEST_ALIGNED_GLOBAL")) aligned += strtoull(v, nullptr, 10);
    }
    q->n_total = (double)aligned;
    HIP_TRY(hipMemcpyAsync(q->x1.p, lengths, n_tx * 8, hipMemcpyHostToDevice, q->stream));
    if (m->use_length_weights)                 // a fragment-length model: the same on every rank
        launch_effective_lengths_weights(m->length_weights.p, 1, q->x1.p, n_tx, q->eff_len.p, q->stream);
    else
        launch_effective_lengths(fld.p, q->x1.p, n_tx, q->eff_len.p, q->stream);
    // (the effective lengths go home at the end, with the TPM: a copy to pageable memory holds the
    // host up, and the kernels that follow are not launched meanwhile)
    // quantify(): no class -> zeros (infer.py:106-107); over several ranks "no class anywhere"
    // is "no aligned unit anywhere" (every aligned unit belongs to a class)
    if (q->comm ? aligned == 0 : C == 0) {
        if (effective_lengths)
            HIP_TRY(hipMemcpyAsync(effective_lengths, q->eff_len.p, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        if (tpm) memset(tpm, 0, (size_t)n_tx * 8);
        if (iters) *iters = 0;
        return SKM_OK;
    }
    launch_reciprocal(q->eff_len.p, n_tx, q->x0.p, q->stream);
    launch_np_sum(q->x0.p, n_tx, 1.0, sums.p, total, q->stream);
    launch_divide(q->x0.p, n_tx, total, false, 0.0, q->stream);
    lap("start vector");
    SKM_TRY(quant_finish_setup(q.get(), &m->t, m->first_seen_bound));
    lap("setup");
    if (trace) fprintf(stderr, "[skm_quant_infer] %lld classes, %lld transcripts, rows %s\n", (long long)C, (long long)n_tx,
                       q->rows.built() ? "built" : "not built");
    int64_t it = 0;
    SKM_TRY(em_run(q.get(), rel_tol, x_floor, max_iters, 0, &it));
    lap("em");
    m->t_em_ns += q->t_em_ns;
    m->em_iters += (double)it;
    double *const x = (it & 1) ? q->x1.p : q->x0.p;
    launch_np_sum(x, n_tx, 1000000.0, sums.p, total, q->stream);
    launch_divide(x, n_tx, total + 1, true, 0.001, q->stream);
    launch_np_sum(x, n_tx, 1000000.0, sums.p, total, q->stream);
    launch_divide(x, n_tx, total + 1, false, 0.0, q->stream);
    HIP_TRY(hipGetLastError());
    if (tpm) HIP_TRY(hipMemcpyAsync(tpm, x, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
    if (effective_lengths)
        HIP_TRY(hipMemcpyAsync(effective_lengths, q->eff_len.p, n_tx * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    lap("tpm");
    if (iters) *iters = it;
    q.reset();
    lap("destroy");
    return SKM_OK;
}

extern "C" int skm_quant_destroy(skm_quant *q)
{
    if (!q) return SKM_OK;
    STALE_CHECK("quant_destroy entry");
    delete q;
    STALE_CHECK("quant_destroy exit");
    return SKM_OK;
}

extern "C" int skm_quant_em(skm_quant *q, double *x, const double *l, double rel_tol, double x_floor,
                            int64_t max_iters, int64_t fixed_iters, int64_t *iters)
{
    if (!q || !x || !l) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    HIP_TRY(hipMemcpyAsync(q->x0.p, x, q->n_tx * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->eff_len.p, l, q->n_tx * 8, hipMemcpyHostToDevice, q->stream));
    int64_t it = 0;
    SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, fixed_iters, &it));
    HIP_TRY(hipMemcpy(x, (it & 1) ? q->x1.p : q->x0.p, q->n_tx * 8, hipMemcpyDeviceToHost));
    if (iters) *iters = it;
    return SKM_OK;
}

extern "C" int skm_quant_components(skm_quant *q, int64_t info[8], int32_t *tx_label, int32_t *tx_tile,
                                    int32_t *class_tile)
{
    if (!q || !info) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    const auto &t = q->tiles;
    info[0] = t.built ? 1 : 0;
    info[1] = t.n_tiles;
    info[2] = t.n_oversize;
    info[3] = em_uses_tiles(q) ? 1 : 0;
    info[4] = EM_TILE_PAIRS; info[5] = EM_TILE_CLASSES; info[6] = EM_TILE_TX; info[7] = EM_TILE_SEGMENT;
    if (!t.built) {
        if (tx_label || tx_tile || class_tile) return fail(SKM_ERR_ARG, "no component tiles were built for this handle");
        return SKM_OK;
    }
    HIP_TRY(hipStreamSynchronize(q->stream));
    if (tx_label) HIP_TRY(hipMemcpy(tx_label, t.tx_label.p, q->n_tx * 4, hipMemcpyDeviceToHost));
    if (tx_tile) HIP_TRY(hipMemcpy(tx_tile, t.tx_tile.p, q->n_tx * 4, hipMemcpyDeviceToHost));
    if (class_tile && q->n_classes) {
        // internal (locality) order -> the caller's class order
        std::vector<int32_t> tile(q->n_classes), perm(q->n_classes);
        HIP_TRY(hipMemcpy(tile.data(), t.cls_tile.p, q->n_classes * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(perm.data(), q->perm.p, q->n_classes * 4, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < q->n_classes; ++k) class_tile[perm[k]] = tile[k];
    }
    return SKM_OK;
}

extern "C" int skm_quant_rows_built(skm_quant *q, int *built)
{
    if (!q || !built) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    *built = q->rows.built() ? 1 : 0;
    return SKM_OK;
}

extern "C" int skm_quant_tile_arrays(skm_quant *q, int64_t *tile_tx, int64_t *tile_cls, int32_t *tx_list, int32_t *cls_list,
                                     int64_t *tx_pair, int64_t *cls_pair, uint16_t *cls_tx, uint16_t *tx_cls, int32_t *order,
                                     int32_t *perm)
{
    if (!q) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    const auto &t = q->tiles;
    if (!t.built) return fail(SKM_ERR_ARG, "no component tiles were built for this handle");
    HIP_TRY(hipStreamSynchronize(q->stream));
    const int64_t S = t.n_tiles, T = q->n_tx, C = q->n_classes, M = q->n_ids;
    auto home = [](void *to, const void *from, int64_t bytes) {
        return to && bytes > 0 ? hipMemcpy(to, from, (size_t)bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIP_TRY(home(tile_tx, t.tile_tx.p, (S + 1) * 8)); HIP_TRY(home(tile_cls, t.tile_cls.p, (S + 1) * 8));
    HIP_TRY(home(tx_list, t.tx_list.p, T * 4)); HIP_TRY(home(cls_list, t.cls_list.p, C * 4));
    HIP_TRY(home(tx_pair, t.tx_pair.p, (T + 1) * 8)); HIP_TRY(home(cls_pair, t.cls_pair.p, (C + 1) * 8));
    HIP_TRY(home(cls_tx, t.cls_tx.p, M * 2)); HIP_TRY(home(tx_cls, t.tx_cls.p, M * 2));
    HIP_TRY(home(order, t.order.p, S * 4)); HIP_TRY(home(perm, q->perm.p, C * 4));
    return SKM_OK;
}

extern "C" int skm_device_np_sum_probe(int device, const double *values, int64_t n, double *sum)
{
    SKM_TRY(check_device(device));
    if (n < 0 || n >= (1LL << 31) || !sum || (n && !values)) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(set_device(device));
    DBuf<double> d_values, d_sums, d_out;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(nullptr); });     // (an early return: before they go)
    SKM_TRY(d_values.ensure(std::max<int64_t>(n, 1))); SKM_TRY(d_sums.ensure((n + 8191) / 8192 + 1)); SKM_TRY(d_out.ensure(2));
    if (n) HIP_TRY(hipMemcpy(d_values.p, values, n * 8, hipMemcpyHostToDevice));
    launch_np_sum(d_values.p, n, 1.0, d_sums.p, d_out.p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(sum, d_out.p, 8, hipMemcpyDeviceToHost));
    drain.dismiss();                          // (the copy home has waited for the kernels)
    return SKM_OK;
}

extern "C" int skm_quant_set_counts(skm_quant *q, const double *class_counts)
{
    if (!q || (!class_counts && q->n_classes)) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    const double total = np_sum_host(class_counts, q->n_classes);
    if (q->n_classes) {
        // caller's class order -> internal (locality) order
        SKM_TRY(q->cls_count_saved.ensure(q->n_classes));
        HIP_TRY(hipMemcpyAsync(q->cls_count_saved.p, class_counts, q->n_classes * 8, hipMemcpyHostToDevice, q->stream));
        launch_permute_f64(q->cls_count_saved.p, q->perm.p, q->n_classes, q->cls_count.p, false, q->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(q->stream));
    }
    q->n_total = total;
    return SKM_OK;
}

namespace {

// ---- many EM problems on ONE class structure: the group loop that `-b N` (bootstrap_impl), K count
// vectors of the caller's (skm_quant_em_many) and the second round of `impute` (skm_quant_em_blend)
// share.  The callers differ in where a problem's class counts come from, and say so with
//     fill(first, n, rows, totals): queue on the handle's stream whatever leaves rows[i][C] (device,
//     INTERNAL class order) = the class counts of problems first + i, i < n, and totals[2 i] (device;
//     pairs, as launch_np_sum_many leaves them) = their sums as numpy adds them up in the caller's order.
// Problem b starts from x0, runs the EM of seekmer/infer.py:133-168 to its stopping rule and leaves
// out[b][T]: the raw result, or with `tpm` what quantify() makes of it (infer.py:127-129).  The caller
// holds q->mu, has set the device and has checked its arguments; C > 0.  On every exit the handle
// holds the class counts and the total it came with.
//   batched: EM_BATCH problems side by side with the device refilling the places (skm_em_batch.hip);
//   otherwise (resampled counts wanted, a step cap set, a communicator attached: its collectives
//   must stay matched) one problem after the other through the single-problem EM.
//   slot_cap > 0 (tests): at most that many problems per group.
template <class Fill>
int em_group_run(skm_quant *q, int64_t n_problems, Fill &&fill, bool batched, int64_t slot_cap, const double *x0,
                 const double *l, double rel_tol, double x_floor, int64_t max_iters, double *out, int64_t *iters_out,
                 bool tpm)
{
    const int64_t C = q->n_classes, T = q->n_tx;
    skm_quant::Batch &w = q->batch;
    // the problems' results stay in HBM and come back in groups (one copy per group, not one per problem)
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(n_problems, (int64_t)(1LL << 28) / T));
    const int64_t by_counts = std::max<int64_t>(1, (int64_t)((1LL << 31) / (8 * std::max<int64_t>(C, 1))));
    int64_t slots = batched ? std::max<int64_t>(1, std::min(group, by_counts)) : 1;
    if (slot_cap > 0) slots = std::min(slots, slot_cap);
    SKM_TRY(q->cls_count_saved.ensure(C));
    SKM_TRY(q->x_start.ensure(T));
    SKM_TRY(q->boot_out.ensure((size_t)(slots * T)));
    SKM_TRY(w.totals.ensure((size_t)(2 * slots)));
    HIP_TRY(hipMemcpyAsync(q->cls_count_saved.p, q->cls_count.p, C * 8, hipMemcpyDeviceToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->eff_len.p, l, T * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->x_start.p, x0, T * 8, hipMemcpyHostToDevice, q->stream));
    const double saved_total = q->n_total;
    int rc = SKM_OK;
    DBuf<double> sums;                               // (before `restore`: freed after the stream has drained)
    auto restore = on_exit([&]() {                   // every exit: the handle holds its own counts again
        (void)hipMemcpyAsync(q->cls_count.p, q->cls_count_saved.p, C * 8, hipMemcpyDeviceToDevice, q->stream);
        (void)hipStreamSynchronize(q->stream);
        q->n_total = saved_total;
    });
    // One problem the careful way (host-checked chunks of the single-problem EM): its counts straight
    // into the handle's, EM from x_start, result to `dst` (HBM).
    auto problem_checked = [&](int64_t b, int64_t *it_out, double *dst) -> int {
        SKM_TRY(fill(b, (int64_t)1, q->cls_count.p, w.totals.p));
        HIP_TRY(hipGetLastError());
        double total = 0.0;
        HIP_TRY(hipMemcpyAsync(&total, w.totals.p, 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipMemcpyAsync(q->x0.p, q->x_start.p, T * 8, hipMemcpyDeviceToDevice, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        q->n_total = total;
        SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, 0, it_out, 8));
        HIP_TRY(hipMemcpyAsync(dst, (*it_out & 1) ? q->x1.p : q->x0.p, T * 8, hipMemcpyDeviceToDevice, q->stream));
        if (iters_out) iters_out[b] = *it_out;
        return SKM_OK;
    };
    // infer.py:127-129 on `count` results in HBM (TPM scaling with numpy's sums), when TPM is asked for
    auto scale = [&](double *results, int64_t count) -> int {
        if (!tpm || count <= 0) return SKM_OK;
        const int64_t n_blocks = (T + 8191) / 8192;
        SKM_TRY(sums.ensure((size_t)(count * (n_blocks + 2))));
        double *const totals = sums.p + count * n_blocks;            // (sum, sum / 1e6) per problem
        launch_np_sum_many(results, T, count, T, 1000000.0, sums.p, totals, q->stream);
        launch_divide_many(results, T, count, T, totals + 1, true, 0.001, q->stream);
        launch_np_sum_many(results, T, count, T, 1000000.0, sums.p, totals, q->stream);
        launch_divide_many(results, T, count, T, totals + 1, false, 0.0, q->stream);
        HIP_TRY(hipGetLastError());
        return SKM_OK;
    };
    auto send_home = [&](int64_t first, int64_t count) -> int {     // boot_out[0 .. count) = problems first ..
        if (count <= 0) return SKM_OK;
        SKM_TRY(scale(q->boot_out.p, count));
        HIP_TRY(hipMemcpyAsync(out + first * T, q->boot_out.p, (size_t)count * T * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        return SKM_OK;
    };
    if (!batched) {
        for (int64_t b = 0; b < n_problems; ++b) {
            int64_t it = 0;
            SKM_TRY(problem_checked(b, &it, q->boot_out.p));
            SKM_TRY(send_home(b, 1));
        }
        return rc;
    }
    // EM_BATCH problems sit side by side in the batched EM (skm_em_batch.hip) and THE DEVICE keeps the
    // working set full: the class counts of a whole group of problems are made first (HBM has the
    // room: 8 MB per problem at a million classes), and after every step two small launches take
    // the results of the problems that have latched their stopping rule and put the next ones in
    // their places (launch_em_batch_manage) -- no host look between steps; the host queues steps
    // and reads now and then how many problems have finished.  (Through round 3's first half the
    // host looked every four steps and refilled: ~100 looks and a fifth of the phase's wall time in
    // gaps.)  Step counts have a long tail (most replicates of the 20 M-pair table stop near 30
    // steps, one in six needs 60-90): problems that wait for the slowest of a fixed group of eight
    // waste half the working set's steps.  Every problem still runs the single-problem EM's steps bit
    // for bit, whoever its neighbours are and whenever it starts.
    QuantRowsView rows{};                                        // (the batched EM steps the whole table)
    SKM_TRY(q->rows.get(q, rows));
    SKM_TRY(w.cls_count.ensure((size_t)C * EM_BATCH)); SKM_TRY(w.inner.ensure((size_t)C * EM_BATCH));
    SKM_TRY(w.row_sum.ensure((size_t)std::max<int64_t>(rows.n_rows, 1) * EM_BATCH));
    SKM_TRY(w.x0.ensure((size_t)T * EM_BATCH)); SKM_TRY(w.x1.ensure((size_t)T * EM_BATCH));
    SKM_TRY(w.part_max.ensure((size_t)EM_FINAL_BLOCKS * EM_BATCH));
    SKM_TRY(w.part_flags.ensure((size_t)EM_FINAL_BLOCKS * EM_BATCH));
    SKM_TRY(w.ctl.ensure(32 + EM_BATCH));                        // (the places' totals lie behind the control block)
    SKM_TRY(w.mgr.ensure(64));
    SKM_TRY(w.counts_all.ensure((size_t)slots * C));
    SKM_TRY(w.iters.ensure((size_t)slots));
    EmBatchProblem p{};
    p.n_tx = T; p.n_classes = C; p.n_rows = rows.n_rows;
    p.cls_offset = q->cls_offset.p; p.ids = q->ids.p; p.row_start = rows.row_start; p.row_tx = rows.row_tx;
    p.tx_cls = rows.tx_cls; p.tx_row = rows.tx_row; p.eff_len = q->eff_len.p;
    p.cls_count = w.cls_count.p; p.inner = w.inner.p; p.row_sum = w.row_sum.p;
    p.x[0] = w.x0.p; p.x[1] = w.x1.p;
    p.place_total = reinterpret_cast<double *>(w.ctl.p + 32);
    p.rel_tol = rel_tol; p.x_floor = x_floor;
    p.ctl = w.ctl.p; p.part_max = w.part_max.p; p.part_flags = w.part_flags.p;
    p.managed = 1;
    p.mgr = w.mgr.p;
    p.iters_out = w.iters.p;
    p.fused = getenv("SKM_EM_UNFUSED") ? 0 : 1;
    p.arrivals = rows.arrivals;
    int64_t chunk = 16;                                          // steps queued between two looks at the progress
    if (const char *e = getenv("SKM_BOOTSTRAP_CHUNK")) chunk = std::max<int64_t>(1, atoll(e));   // (tests)
    unsigned long long *const look = q->pinned + 64;             // 64 + 8 words of the pinned block
    std::vector<int64_t> iters_host((size_t)slots);
    std::vector<double> totals_host((size_t)(2 * slots));        // (what the tail hands to the single-problem EM)
    for (int64_t w0 = 0; w0 < n_problems; w0 += slots) {
        const int64_t n = std::min(n_problems, w0 + slots) - w0;
        SKM_TRY(fill(w0, n, w.counts_all.p, w.totals.p));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(totals_host.data(), w.totals.p, (size_t)(2 * n) * 8, hipMemcpyDeviceToHost, q->stream));
        launch_em_batch_manage_init(p, w.mgr.p, look, n, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, q->stream);
        HIP_TRY(hipGetLastError());
        for (int64_t k = 0;;) {
            for (int64_t i = 0; i < chunk; ++i, ++k) {
                launch_em_batch_step(p, k, q->stream);        // (its first kernel also plans for what has stopped)
                launch_em_batch_manage(p, w.mgr.p, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, w.iters.p, k, true,
                                       q->stream);
            }
            // before the host looks, the last pass is judged too (otherwise only the next step's first
            // kernel would) and what it stops is taken: a place that is still occupied then is running
            launch_em_batch_decide(p, k, q->stream);
            launch_em_batch_manage(p, w.mgr.p, w.counts_all.p, w.totals.p, q->x_start.p, q->boot_out.p, w.iters.p, k - 1, false,
                                   q->stream);
            q->launches += 4 * chunk + 3;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(look, w.mgr.p, 24 * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipMemcpyAsync(look + 24, w.ctl.p, 8 * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipStreamSynchronize(q->stream));
            const unsigned long long *const all_done = look + 24;   // (the head of the control block, behind mgr's words)
            if (look[MGR_UNDEFINED])
                return fail(SKM_ERR_UNDEFINED, "no abundance above x_floor: numpy raises on max() of an empty selection");
            if (all_done[BCTL_ALL_DONE]) break;                  // every problem of the group has finished
            if (k > (1LL << 24)) return fail(SKM_ERR_STATE, "the batched EM does not stop");
            // The tail: nothing left to put in, a few problems still running.  A step of the
            // working set costs the same however many places are live (~5 single-problem steps), so
            // the last three or fewer go on one by one in the single-problem EM, from where they are.
            int live = 0;
            for (int r = 0; r < EM_BATCH; ++r) live += look[MGR_REP + r] != 0;
            if (look[MGR_NEXT] >= look[MGR_COUNT] && live <= 3) {
                for (int r = 0; r < EM_BATCH; ++r) {
                    if (look[MGR_REP + r] == 0) continue;
                    const int64_t rep = (int64_t)look[MGR_REP + r] - 1, since = (int64_t)look[MGR_SINCE + r];
                    launch_em_batch_take(p.x[k & 1], T, r, q->x0.p, q->stream);
                    launch_em_batch_take(w.cls_count.p, C, r, q->cls_count.p, q->stream);
                    HIP_TRY(hipGetLastError());
                    q->n_total = totals_host[(size_t)(2 * rep)];
                    int64_t more = 0;
                    SKM_TRY(em_run(q, rel_tol, x_floor, max_iters, 0, &more, 8));
                    HIP_TRY(hipMemcpyAsync(q->boot_out.p + rep * T, (more & 1) ? q->x1.p : q->x0.p, (size_t)T * 8,
                                           hipMemcpyDeviceToDevice, q->stream));
                    const int64_t steps = k - since + more;
                    HIP_TRY(hipMemcpyAsync(w.iters.p + rep, &steps, 8, hipMemcpyHostToDevice, q->stream));
                    HIP_TRY(hipStreamSynchronize(q->stream));      // (`steps` lives on this frame)
                    q->iters_total -= (double)more;                // (em_run has counted its own; the sum below counts all)
                }
                break;
            }
        }
        HIP_TRY(hipMemcpyAsync(iters_host.data(), w.iters.p, (size_t)n * 8, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipStreamSynchronize(q->stream));
        for (int64_t i = 0; i < n; ++i) {
            if (iters_out) iters_out[w0 + i] = iters_host[(size_t)i];
            q->iters_total += (double)iters_host[(size_t)i];
        }
        SKM_TRY(send_home(w0, n));
    }
    return rc;
}

// Replicate b of the call (b = 0 .. n_boot - 1) is replicate number rep_first + b * rep_step of the
// `-b N` run: its draw depends on (seed, that number) alone, so a rank's share of the replicates
// gives the same results as the one-GPU loop, replicate by replicate.
int bootstrap_impl(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                   const double *l, double rel_tol, double x_floor, int64_t max_iters,
                   double *out, int64_t *counts_out, int64_t *iters_out, bool tpm,
                   int64_t rep_first = 0, int64_t rep_step = 1)
{
    if (!q || !x0 || !l || !out || n_boot < 0 || rep_first < 0 || rep_step < 1) return fail(SKM_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    // (seekmer/infer.py:108-111 resamples the table of the WHOLE sample: a handle that holds one
    // rank's share of the classes -- a communicator of several ranks attached -- cannot)
    if (q->comm && q->world > 1)
        return fail(SKM_ERR_STATE, "bootstraps resample the merged class table: detach the communicator "
                                   "(skm_quant_set_comm(quant, NULL)) and give every rank the merged table");
    auto number = [&](int64_t b) { return (uint64_t)(rep_first + b * rep_step); };
    const int64_t C = q->n_classes;
    if (C == 0) return fail(SKM_ERR_STATE, "no classes to resample");
    // integer cumulative counts of the observed table
    SKM_TRY(q->cum.ensure(C));
    SKM_TRY(q->tile_total.ensure(4096));
    SKM_TRY(q->inner.ensure(C));
    std::vector<double> cnt(C);
    HIP_TRY(hipMemcpyAsync(cnt.data(), q->cls_count.p, C * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    std::vector<unsigned long long> cum(C);
    unsigned long long run = 0;
    for (int64_t c = 0; c < C; ++c) { run += (unsigned long long)cnt[c]; cum[c] = run; }
    if (run >= (1ULL << 32)) return fail(SKM_ERR_STATE, "more than 2^32 - 1 units to resample");
    HIP_TRY(hipMemcpyAsync(q->cum.p, cum.data(), C * 8, hipMemcpyHostToDevice, q->stream));
    const int64_t n_draws = (int64_t)run;            // n = class_count.sum(), infer.py:109
    // (a resample keeps the total: the same for every replicate; filled once, never changed while the
    // call runs, so the copies out of it need no synchronisation of their own)
    const std::vector<double> totals((size_t)(2 * std::max<int64_t>(n_boot, 1)), (double)n_draws);
    // a group's counts: one multinomial draw per replicate, straight into its row
    auto draw = [&](int64_t first, int64_t n, double *rows, double *totals_dev) -> int {
        for (int64_t i = 0; i < n; ++i)
            if (!launch_multinomial(q->cum.p, C, n_draws, seed, number(first + i), q->tile_total.p, rows + (size_t)i * C, 1,
                                    q->stream))
                return fail(SKM_ERR_STATE, "class table too large to resample (%lld classes)", (long long)C);
        HIP_TRY(hipGetLastError());
        for (int64_t i = 0; i < n && counts_out; ++i) {
            // internal (locality) class order -> caller's order; the counts fit a double exactly
            launch_permute_f64(rows + (size_t)i * C, q->perm.p, C, q->inner.p, true, q->stream);
            std::vector<double> as_double(C);
            HIP_TRY(hipMemcpyAsync(as_double.data(), q->inner.p, C * 8, hipMemcpyDeviceToHost, q->stream));
            HIP_TRY(hipStreamSynchronize(q->stream));
            for (int64_t c = 0; c < C; ++c) counts_out[(first + i) * C + c] = (int64_t)as_double[c];
        }
        HIP_TRY(hipMemcpyAsync(totals_dev, totals.data(), (size_t)(2 * n) * 8, hipMemcpyHostToDevice, q->stream));
        return SKM_OK;
    };
    // With the resampled counts wanted, a step cap set or a communicator attached (its collectives
    // must stay matched) every replicate goes the careful way.
    const bool batched = !counts_out && !q->comm && max_iters <= 0;
    return em_group_run(q, n_boot, draw, batched, 0, x0, l, rel_tol, x_floor, max_iters, out, iters_out, tpm);
}

// Rows of class counts in the caller's order, `produce`d piece by piece into a staging buffer, on their
// way into a group of em_group_run: the sum of each row as numpy adds it up (what skm_quant_set_counts
// computes on the host), then the row in the internal (locality) class order.  A piece is at most
// 256 MB, so neither side holds a second copy of a whole group and the caller's rows need not be
// page-locked.  The staging buffers belong to the call (ManyStage: sized before anything is queued, given
// back to the pool when the call ends), not to the handle, which may live long (infer._quant_for).
int64_t many_piece(int64_t n_classes, int64_t n_rows)
{
    return std::max<int64_t>(1, std::min<int64_t>(n_rows, (int64_t)(1LL << 25) / std::max<int64_t>(n_classes, 1)));
}

struct ManyStage {
    DBuf<double> rows, sums;
    int reserve(int64_t n_classes, int64_t n_rows)
    {
        const int64_t piece = many_piece(n_classes, n_rows);
        SKM_TRY(rows.ensure((size_t)(piece * n_classes)));
        SKM_TRY(sums.ensure((size_t)(piece * ((n_classes + 8191) / 8192))));
        return SKM_OK;
    }
};

template <class Produce>
int many_rows_in(skm_quant *q, ManyStage &stage, int64_t first, int64_t n, double *rows, double *totals,
                 int64_t n_rows_of_call, Produce &&produce)
{
    const int64_t C = q->n_classes, piece = many_piece(C, n_rows_of_call);
    for (int64_t i0 = 0; i0 < n; i0 += piece) {
        const int64_t m = std::min(piece, n - i0);
        SKM_TRY(produce(first + i0, m, stage.rows.p));
        launch_np_sum_many(stage.rows.p, C, m, C, 1.0, stage.sums.p, totals + 2 * i0, q->stream);
        launch_permute_rows_f64(stage.rows.p, q->perm.p, C, m, rows + (size_t)i0 * C, q->stream);
        HIP_TRY(hipGetLastError());
    }
    return SKM_OK;
}

// what the two entry points below check alike, before the handle is touched
int many_check(const skm_quant *q, int64_t n_sets, const double *x0, const double *l, const double *out, bool sources)
{
    if (!q || n_sets < 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_sets > 0 && (!x0 || !l || !out || !sources)) return fail(SKM_ERR_ARG, "NULL argument");
    return SKM_OK;
}

int many_state_check(const skm_quant *q)
{
    // (one rank's share of the classes is not the table the caller's counts belong to)
    if (q->comm && q->world > 1)
        return fail(SKM_ERR_STATE, "bootstraps resample the merged class table: detach the communicator "
                                   "(skm_quant_set_comm(quant, NULL)) and give every rank the merged table");
    if (q->n_classes == 0) return fail(SKM_ERR_STATE, "no classes to quantify");
    return SKM_OK;
}

int64_t many_slot_cap()
{
    const char *e = getenv("SKM_EM_MANY_SLOTS");                  // (tests: several groups from a few problems)
    return e ? std::max<int64_t>(1, atoll(e)) : 0;
}

}  // namespace

extern "C" int skm_quant_em_many(skm_quant *q, int64_t n_sets, const double *counts, const double *x0, const double *l,
                                 double rel_tol, double x_floor, int tpm, double *out, int64_t *iters_out)
{
    SKM_TRY(many_check(q, n_sets, x0, l, out, counts != nullptr));
    if (n_sets == 0) return SKM_OK;                               // (nothing to do, with or without a GPU)
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    SKM_TRY(many_state_check(q));
    const int64_t C = q->n_classes;
    ManyStage stage;                                              // (before the guard: freed after the stream has drained)
    SKM_TRY(stage.reserve(C, n_sets));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(q->stream); });
    auto upload = [&](int64_t first, int64_t m, double *stage) -> int {
        HIP_TRY(hipMemcpyAsync(stage, counts + (size_t)first * C, (size_t)m * C * 8, hipMemcpyHostToDevice, q->stream));
        return SKM_OK;
    };
    auto fill = [&](int64_t first, int64_t n, double *rows, double *totals) -> int {
        return many_rows_in(q, stage, first, n, rows, totals, n_sets, upload);
    };
    return em_group_run(q, n_sets, fill, !q->comm, many_slot_cap(), x0, l, rel_tol, x_floor, 0, out, iters_out, tpm != 0);
}

extern "C" int skm_quant_em_blend(skm_quant *q, int64_t n_cells, const int32_t *class_cell, const double *weight,
                                  const double *cell_total, const double *x0, const double *l, double rel_tol,
                                  double x_floor, int tpm, double *out, int64_t *iters_out, double *counts_out)
{
    SKM_TRY(many_check(q, n_cells, x0, l, out, class_cell && weight && cell_total));
    if (n_cells == 0) return SKM_OK;                              // (nothing to do, with or without a GPU)
    int n_dev = 0;
    SKM_TRY(skm_device_count(&n_dev));
    std::lock_guard<std::mutex> lock(q->mu);
    SKM_TRY(set_device(q->device));
    SKM_TRY(many_state_check(q));
    const int64_t C = q->n_classes;
    for (int64_t k = 0; k < C; ++k)
        if (class_cell[k] < 0 || class_cell[k] >= n_cells)
            return fail(SKM_ERR_ARG, "class_cell[%lld] = %d outside [0, n_cells)", (long long)k, (int)class_cell[k]);
    ManyStage stage;
    SKM_TRY(stage.reserve(C, n_cells));
    // what the kernel reads: the handle's own counts in the caller's class order, the class -> cell map,
    // the weights and the cells' totals (declared before the guard: freed after the stream has drained)
    DBuf<double> own, weight_dev, total_dev;
    DBuf<int32_t> cell_dev;
    SKM_TRY(own.ensure(C)); SKM_TRY(cell_dev.ensure(C));
    SKM_TRY(weight_dev.ensure((size_t)(n_cells * n_cells))); SKM_TRY(total_dev.ensure((size_t)n_cells));
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(q->stream); });
    launch_permute_f64(q->cls_count.p, q->perm.p, C, own.p, true, q->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cell_dev.p, class_cell, C * 4, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(weight_dev.p, weight, (size_t)(n_cells * n_cells) * 8, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(total_dev.p, cell_total, (size_t)n_cells * 8, hipMemcpyHostToDevice, q->stream));
    auto blend = [&](int64_t first, int64_t m, double *stage) -> int {
        launch_blend_counts(own.p, cell_dev.p, weight_dev.p, total_dev.p, n_cells, first, m, C, stage, q->stream);
        HIP_TRY(hipGetLastError());
        if (counts_out)
            HIP_TRY(hipMemcpyAsync(counts_out + (size_t)first * C, stage, (size_t)m * C * 8, hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    auto fill = [&](int64_t first, int64_t n, double *rows, double *totals) -> int {
        return many_rows_in(q, stage, first, n, rows, totals, n_cells, blend);
    };
    return em_group_run(q, n_cells, fill, !q->comm, many_slot_cap(), x0, l, rel_tol, x_floor, 0, out, iters_out, tpm != 0);
}

extern "C" int skm_quant_bootstrap(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                                   const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                   double *out, int64_t *counts_out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, counts_out, iters_out, false);
}

extern "C" int skm_quant_bootstrap_tpm(skm_quant *q, int64_t n_boot, uint64_t seed, const double *x0,
                                       const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                       double *out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, nullptr, iters_out, true);
}

extern "C" int skm_quant_bootstrap_share_tpm(skm_quant *q, int64_t n_boot, int64_t first, int64_t step, uint64_t seed,
                                             const double *x0, const double *l, double rel_tol, double x_floor,
                                             int64_t max_iters, double *out, int64_t *iters_out)
{
    return bootstrap_impl(q, n_boot, seed, x0, l, rel_tol, x_floor, max_iters, out, nullptr, iters_out, true, first, step);
}

// ---- many class tables over the same transcripts in shared EM launches (skm_em_set.hip) ------------
// The tables of a GROUP are stacked into one block-diagonal problem on a handle of the call's own (class
// views without component tiles: quant_alloc's several_ranks switch), set up once by quant_setup and
// stepped by the segmented kernels until every slot has met its own stopping rule.  A group holds as
// many consecutive tables as keep
//   - slots * T below 2^31 (stacked transcript ids are int32) and the classes and pairs below 2^31,
//   - slots at most SET_QUANT_MAX_SLOTS (gridDim.y) and at most SKM_SET_QUANT_GROUP (tests),
//   - set_quant_bytes(), an estimate of the group's buffers and of the set-up's scratch, within
//     SET_QUANT_GROUP_BYTES (2 GiB); a single table above that still runs, as a group of its own.
// The next group reuses the buffers (they are sized for the largest group before the first runs).
namespace {

constexpr int64_t SET_QUANT_MAX_SLOTS = 32768;
constexpr int64_t SET_QUANT_GROUP_BYTES = 1LL << 31;

int64_t set_quant_bytes(int64_t slots, int64_t n_tx, int64_t n_classes, int64_t n_ids)
{
    return slots * n_tx * 96 + n_classes * 64 + n_ids * 24;
}

int64_t set_quant_slot_cap()
{
    const char *e = getenv("SKM_SET_QUANT_GROUP");                // (looked up at every call)
    const int64_t asked = e ? atoll(e) : 0;
    return asked > 0 ? std::min(asked, SET_QUANT_MAX_SLOTS) : SET_QUANT_MAX_SLOTS;
}

// group g = tables [first[g], first[g + 1]); `first` ends with n_tables
void set_quant_cut(int64_t n_tables, int64_t n_tx, const int64_t *table_classes, const int64_t *table_ids, int64_t max_slots,
                   std::vector<int64_t> *first)
{
    first->assign(1, 0);
    int64_t slots = 0, classes = 0, ids = 0;
    for (int64_t i = 0; i < n_tables; ++i) {
        const bool fits = slots < max_slots && (slots + 1) * n_tx < (1LL << 31) && classes + table_classes[i] < (1LL << 31)
                          && ids + table_ids[i] < (1LL << 31)
                          && set_quant_bytes(slots + 1, n_tx, classes + table_classes[i], ids + table_ids[i]) <= SET_QUANT_GROUP_BYTES;
        if (slots > 0 && !fits) {
            first->push_back(i);
            slots = classes = ids = 0;
        }
        ++slots; classes += table_classes[i]; ids += table_ids[i];
    }
    if (n_tables > 0) first->push_back(n_tables);
}

struct SetQuantRun {
    // (the scratch before the handle: the handle's destructor, which runs first, drains the stream)
    DBuf<EmSetSlot> slots;
    DBuf<unsigned long long> running;
    DBuf<double> out, sums;
    std::unique_ptr<skm_quant> q;
    int64_t n_tx = 0;
};

// room for the largest group of the cut
int set_quant_open(SetQuantRun &run, int device, int64_t n_tx, const std::vector<int64_t> &first, const int64_t *table_classes,
                   const int64_t *table_ids)
{
    int64_t slots = 1, classes = 0, ids = 0;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        int64_t c = 0, m = 0;
        for (int64_t i = first[g]; i < first[g + 1]; ++i) { c += table_classes[i]; m += table_ids[i]; }
        slots = std::max(slots, first[g + 1] - first[g]);
        classes = std::max(classes, c);
        ids = std::max(ids, m);
    }
    if (slots * n_tx >= (1LL << 31)) return fail(SKM_ERR_ARG, "%lld transcripts: stacked ids do not fit 32 bits", (long long)n_tx);
    run.n_tx = n_tx;
    run.q.reset(new skm_quant());
    SKM_TRY(quant_alloc(run.q.get(), device, slots * n_tx, classes, ids, true));
    SKM_TRY(run.slots.ensure((size_t)slots));
    SKM_TRY(run.running.ensure(2));
    SKM_TRY(run.out.ensure((size_t)(slots * n_tx)));
    SKM_TRY(run.sums.ensure((size_t)(slots * ((n_tx + 8191) / 8192 + 2))));
    return SKM_OK;
}

// One group of n tables.  The caller has queued on the handle's stream whatever fills, for the stacked
// problem: cls_offset [C + 1] (from 0), ids [M] (slot s's ids + s T), cls_count [C] -- classes table by
// table in each table's own order --, eff_len and x0 [n][T].  slot_classes / slot_total: classes and sum
// of the class counts of every table.  out [n][T] and iters [n] (host) get what skm_quant_create +
// skm_quant_em give for each table alone; tpm: scaled as quantify() scales (infer.py:127-129).
int set_quant_group(SetQuantRun &run, int64_t n, const int64_t *slot_classes, const double *slot_total, int64_t C, int64_t M,
                    double rel_tol, double x_floor, int64_t max_iters, bool tpm, double *out, int64_t *iters, int64_t first_table)
{
    skm_quant *q = run.q.get();
    const int64_t T = run.n_tx;
    // (on every way out, the failing ones too: copies from the callers' and this function's pageable staging
    // vectors may still be queued, and those vectors go before the handle's destructor drains the stream)
    struct Drain { hipStream_t stream; ~Drain() { (void)hipStreamSynchronize(stream); } } drain{q->stream};
    if (C == 0) {                                                 // (quantify(): no class -> zeros, infer.py:106-107)
        HIP_TRY(hipStreamSynchronize(q->stream));
        if (out) std::fill(out, out + n * T, 0.0);
        for (int64_t i = 0; i < n && iters; ++i) iters[i] = 0;
        return SKM_OK;
    }
    q->n_tx = n * T; q->n_classes = C; q->n_ids = M;
    SKM_TRY(quant_finish_setup(q, nullptr));
    // every transcript has its rows, slot s those of transcripts [s T, (s + 1) T)
    QuantRowsView rows{};                                         // (the set EM steps the stacked table whole)
    SKM_TRY(q->rows.get(q, rows));
    std::vector<int64_t> row_cut((size_t)n + 1);
    HIP_TRY(hipMemcpy2DAsync(row_cut.data(), 8, rows.tx_row, (size_t)T * 8, 8, (size_t)n + 1, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    std::vector<EmSetSlot> slots((size_t)n);
    int64_t cls = 0, largest_classes = 0, largest_rows = 0;
    for (int64_t i = 0; i < n; ++i) {
        EmSetSlot &d = slots[(size_t)i];
        d.cls_first = cls; d.cls_end = cls += slot_classes[i];
        d.row_first = row_cut[(size_t)i]; d.row_end = row_cut[(size_t)i + 1];
        if (d.row_end - d.row_first < T || d.row_end > rows.n_rows)
            return fail(SKM_ERR_STATE, "the stacked class views give table %lld rows [%lld, %lld)", (long long)(first_table + i),
                        (long long)d.row_first, (long long)d.row_end);
        d.n_total = slot_total[i];
        d.done = slot_classes[i] == 0 ? 1 : 0;
        d.iters = 0; d.undefined = 0;
        if (slot_classes[i]) {
            largest_classes = std::max(largest_classes, slot_classes[i]);
            largest_rows = std::max(largest_rows, d.row_end - d.row_first);
        }
    }
    if (cls != C) return fail(SKM_ERR_STATE, "the tables of the group hold %lld classes, not %lld", (long long)cls, (long long)C);
    EmSetProblem p{};
    p.cls_offset = q->cls_offset.p; p.ids = q->ids.p; p.cls_count = q->cls_count.p; p.inner = q->inner.p;
    p.row_start = rows.row_start; p.row_tx = rows.row_tx; p.tx_cls = rows.tx_cls; p.tx_row = rows.tx_row;
    p.row_sum = q->row_sum.p; p.eff_len = q->eff_len.p; p.x[0] = q->x0.p; p.x[1] = q->x1.p;
    p.rel_tol = rel_tol; p.x_floor = x_floor; p.max_iters = max_iters;
    p.slots = run.slots.p; p.n_slots = (int)n;
    p.n_parts = em_set_parts(largest_rows);
    SKM_TRY(q->part_max.ensure((size_t)(n * p.n_parts)));
    SKM_TRY(q->part_flags.ensure((size_t)(n * p.n_parts)));
    p.part_max = q->part_max.p; p.part_flags = q->part_flags.p;
    p.arrivals = rows.arrivals;
    HIP_TRY(hipMemcpyAsync(run.slots.p, slots.data(), (size_t)n * sizeof(EmSetSlot), hipMemcpyHostToDevice, q->stream));
    // Steps are queued in chunks with the host one chunk ahead, as em_run does; what the host reads at a
    // chunk's end is the number of slots still running.
    const int64_t chunk = 16;
    int64_t k = 0;
    auto enqueue_chunk = [&](int slot) -> int {
        if (k > (1LL << 24)) return fail(SKM_ERR_STATE, "the EM of the stacked tables does not stop");
        HIP_TRY(hipMemsetAsync(run.running.p + slot, 0, 8, q->stream));
        for (int64_t i = 0; i < chunk; ++i, ++k) launch_em_set_step(p, largest_classes, k, i > 0, q->stream);
        launch_em_set_decide(p, k, run.running.p + slot, q->stream);
        q->launches += 2 * chunk + 1;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q->pinned + 8 * slot, run.running.p + slot, 8, hipMemcpyDeviceToHost, q->stream));
        return SKM_OK;
    };
    unsigned long long look[8];                           // ([0]: slots still running)
    SKM_TRY(em_run_chunks_ahead(q, look, enqueue_chunk, [](const unsigned long long *w) { return w[0] == 0; }));
    HIP_TRY(hipMemcpyAsync(slots.data(), run.slots.p, (size_t)n * sizeof(EmSetSlot), hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));             // (with it the look-ahead chunk: no-ops)
    for (int64_t i = 0; i < n; ++i) {
        if (slots[(size_t)i].undefined)
            return fail(SKM_ERR_UNDEFINED, "table %lld: no abundance above x_floor: numpy raises on max() of an empty selection",
                        (long long)(first_table + i));
        if (iters) iters[i] = (int64_t)slots[(size_t)i].iters;
        q->iters_total += (double)slots[(size_t)i].iters;
    }
    launch_em_set_result(run.slots.p, (int)n, q->x0.p, q->x1.p, T, run.out.p, q->stream);
    if (tpm) {
        double *const totals = run.sums.p + n * ((T + 8191) / 8192);  // (sum, sum / 1e6) per table
        launch_np_sum_many(run.out.p, T, n, T, 1000000.0, run.sums.p, totals, q->stream);
        launch_divide_many(run.out.p, T, n, T, totals + 1, true, 0.001, q->stream);
        launch_np_sum_many(run.out.p, T, n, T, 1000000.0, run.sums.p, totals, q->stream);
        launch_divide_many(run.out.p, T, n, T, totals + 1, false, 0.0, q->stream);
        for (int64_t i = 0; i < n; ++i)                   // (quantify() does not scale the zeros of a table without classes)
            if (slot_classes[i] == 0) HIP_TRY(hipMemsetAsync(run.out.p + i * T, 0, (size_t)T * 8, q->stream));
    }
    HIP_TRY(hipGetLastError());
    if (out) HIP_TRY(hipMemcpyAsync(out, run.out.p, (size_t)(n * T) * 8, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    return SKM_OK;
}

}  // namespace

extern "C" int skm_set_quant_groups(int64_t n_tables, int64_t n_tx, const int64_t *table_classes, const int64_t *table_ids,
                                    int64_t max_slots, int64_t *n_groups, int64_t *group_first)
{
    if (n_tables < 0 || n_tx <= 0 || max_slots < 1 || !n_groups || (n_tables && (!table_classes || !table_ids || !group_first)))
        return fail(SKM_ERR_ARG, "bad argument");
    for (int64_t i = 0; i < n_tables; ++i)
        if (table_classes[i] < 0 || table_ids[i] < 0) return fail(SKM_ERR_ARG, "negative size of table %lld", (long long)i);
    std::vector<int64_t> first;
    set_quant_cut(n_tables, n_tx, table_classes, table_ids, std::min(max_slots, SET_QUANT_MAX_SLOTS), &first);
    *n_groups = (int64_t)first.size() - 1;
    if (n_tables) std::copy(first.begin(), first.end(), group_first);
    return SKM_OK;
}

extern "C" int skm_quant_em_tables(int device, int64_t n_tx, int64_t n_tables, const int64_t *table_class_offsets,
                                   const int64_t *class_offsets, const int32_t *class_targets, const double *class_counts,
                                   const double *x0, const double *l, double rel_tol, double x_floor, int64_t max_iters,
                                   int tpm, double *out, int64_t *iters)
{
    if (n_tables < 0 || n_tx <= 0) return fail(SKM_ERR_ARG, "bad argument");
    if (n_tables == 0) return SKM_OK;                             // (nothing to do, with or without a GPU)
    if (!table_class_offsets || !x0 || !l || !out) return fail(SKM_ERR_ARG, "NULL argument");
    if (table_class_offsets[0] < 0) return fail(SKM_ERR_ARG, "negative class offset");
    for (int64_t s = 0; s < n_tables; ++s)
        if (table_class_offsets[s + 1] < table_class_offsets[s]) return fail(SKM_ERR_ARG, "table offsets are not monotone");
    const int64_t c_lo = table_class_offsets[0], c_hi = table_class_offsets[n_tables];
    if (c_hi > c_lo && (!class_offsets || !class_targets || !class_counts)) return fail(SKM_ERR_ARG, "NULL class arrays");
    for (int64_t c = c_lo; c < c_hi; ++c)
        if (class_offsets[c + 1] < class_offsets[c] || class_offsets[c] < 0) return fail(SKM_ERR_ARG, "class offsets are not monotone");
    if (c_hi > c_lo)
        for (int64_t j = class_offsets[c_lo]; j < class_offsets[c_hi]; ++j)
            if (class_targets[j] < 0 || class_targets[j] >= n_tx)
                return fail(SKM_ERR_ARG, "class target %d outside [0, n_tx)", (int)class_targets[j]);
    std::vector<int64_t> classes((size_t)n_tables), ids((size_t)n_tables), first;
    std::vector<double> total((size_t)n_tables);
    // A class without a tuple entry adds its count to the table's total and nothing else: no transcript's
    // sum reads it (skm_quant_create keeps it, with the key of no transcript).  In the stacked order that key
    // would put it behind the classes of EVERY table, outside its own table's range, so such classes are left
    // out of the stacked problem; the total still counts them.  A table of nothing but such classes has no
    // defined problem and no place here.
    for (int64_t s = 0; s < n_tables; ++s) {
        const int64_t a = table_class_offsets[s], b = table_class_offsets[s + 1];
        int64_t named = 0;
        for (int64_t c = a; c < b; ++c) named += class_offsets[c + 1] > class_offsets[c];
        if (b > a && named == 0) return fail(SKM_ERR_ARG, "table %lld: none of its %lld classes names a transcript", (long long)s, (long long)(b - a));
        classes[(size_t)s] = named;
        ids[(size_t)s] = b > a ? class_offsets[b] - class_offsets[a] : 0;
        total[(size_t)s] = b > a ? np_sum_host(class_counts + a, b - a) : 0.0;     // (as skm_quant_create)
    }
    SKM_TRY(check_device(device));
    SKM_TRY(set_device(device));
    set_quant_cut(n_tables, n_tx, classes.data(), ids.data(), set_quant_slot_cap(), &first);
    std::vector<int64_t> offsets;                                 // (staging, declared before the run: its handle's destructor,
    std::vector<int32_t> stacked;                                 //  which drains the stream, then runs before they go)
    std::vector<double> counts;
    SetQuantRun run;
    SKM_TRY(set_quant_open(run, device, n_tx, first, classes.data(), ids.data()));
    skm_quant *q = run.q.get();
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int64_t t0 = first[g], n = first[g + 1] - t0;
        int64_t C = 0, M = 0;
        for (int64_t s = 0; s < n; ++s) { C += classes[(size_t)(t0 + s)]; M += ids[(size_t)(t0 + s)]; }
        if (C) {
            offsets.resize((size_t)C + 1);
            counts.resize((size_t)C);
            stacked.resize((size_t)M);
            int64_t k = 0, j_out = 0;
            for (int64_t s = 0; s < n; ++s) {
                const int32_t base = (int32_t)(s * n_tx);
                for (int64_t c = table_class_offsets[t0 + s]; c < table_class_offsets[t0 + s + 1]; ++c) {
                    if (class_offsets[c + 1] == class_offsets[c]) continue;
                    offsets[(size_t)k] = j_out;
                    counts[(size_t)k++] = class_counts[c];
                    for (int64_t j = class_offsets[c]; j < class_offsets[c + 1]; ++j) stacked[(size_t)j_out++] = class_targets[j] + base;
                }
            }
            offsets[(size_t)C] = j_out;
            if (k != C || j_out != M) return fail(SKM_ERR_STATE, "stacked %lld classes and %lld ids of %lld and %lld", (long long)k, (long long)j_out, (long long)C, (long long)M);
            HIP_TRY(hipMemcpyAsync(q->cls_offset.p, offsets.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_count.p, counts.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->ids.p, stacked.data(), (size_t)M * 4, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->x0.p, x0 + t0 * n_tx, (size_t)(n * n_tx) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->eff_len.p, l + t0 * n_tx, (size_t)(n * n_tx) * 8, hipMemcpyHostToDevice, q->stream));
        }
        SKM_TRY(set_quant_group(run, n, classes.data() + t0, total.data() + t0, C, M, rel_tol, x_floor, max_iters, tpm != 0,
                                out + t0 * n_tx, iters ? iters + t0 : nullptr, t0));
    }
    return SKM_OK;
}

extern "C" int skm_sample_set_quantify(skm_sample_set *s, const double *lengths, int64_t n_tx, double rel_tol, double x_floor,
                                       int64_t max_iters, int64_t cap_samples, int64_t *n_samples, double *tpm,
                                       double *effective_lengths, int64_t *iters)
{
    if (!s || !lengths || !n_samples || n_tx <= 0 || cap_samples < 0 || (cap_samples && !tpm))
        return fail(SKM_ERR_ARG, "bad argument");
    {
        std::lock_guard<std::mutex> counting(s->mu);              // (before any device work)
        *n_samples = (int64_t)s->sample_units.size();
    }
    if (cap_samples < *n_samples) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)*n_samples);
    if (*n_samples == 0) return SKM_OK;
    std::unique_lock<std::mutex> hold;
    SKM_TRY(set_view(s, hold));
    const skm_sample_set::View &v = s->view;
    const int64_t S = (int64_t)v.units.size();
    *n_samples = S;
    if (cap_samples < S) return fail(SKM_ERR_ARG, "room for %lld samples of %lld", (long long)cap_samples, (long long)S);
    skm_mapper *m = s->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SKM_TRY(set_device(m->ix->device));
    // a tuple's ids index the stacked abundance vectors: none may lie outside the caller's transcripts
    for (size_t k = 0; k < v.order.size(); ++k) {
        const int64_t c = v.order[k];
        if (v.len[c] <= 0) return fail(SKM_ERR_STATE, "class %lld of the set has no tuple", (long long)c);   // (it would leave its sample's range)
        for (int64_t j = 0; j < v.len[c]; ++j)
            if (v.arena[(size_t)(v.start[c] + j)] < 0 || v.arena[(size_t)(v.start[c] + j)] >= n_tx)
                return fail(SKM_ERR_ARG, "the set's classes name transcript %d: not below n_tx = %lld", (int)v.arena[(size_t)(v.start[c] + j)],
                            (long long)n_tx);
    }
    std::vector<int64_t> classes((size_t)S), ids((size_t)S), first;
    std::vector<double> total((size_t)S);
    for (int64_t i = 0; i < S; ++i) {
        classes[(size_t)i] = v.sample_class_offsets[(size_t)i + 1] - v.sample_class_offsets[(size_t)i];
        ids[(size_t)i] = v.sample_rows[(size_t)i];
        total[(size_t)i] = (double)v.sample_aligned[(size_t)i];   // n = its aligned units
    }
    set_quant_cut(S, n_tx, classes.data(), ids.data(), set_quant_slot_cap(), &first);
    // the class tuples stay where the mapper left them: a group's are gathered from the table's arena into
    // the stacked problem on the device, by the classes' places there -- a few words per class from the host
    DBuf<double> lengths_dev;
    DBuf<unsigned long long> hist;
    DBuf<int64_t> src, dst;
    DBuf<int32_t> add;
    std::vector<int64_t> h_src, h_dst;                            // (staging, before the run: see skm_quant_em_tables)
    std::vector<int32_t> h_add;
    std::vector<double> h_count;
    SetQuantRun run;
    SKM_TRY(set_quant_open(run, m->ix->device, n_tx, first, classes.data(), ids.data()));
    skm_quant *q = run.q.get();
    int64_t slots_max = 1, classes_max = 1;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        slots_max = std::max(slots_max, first[g + 1] - first[g]);
        classes_max = std::max(classes_max, v.sample_class_offsets[(size_t)first[g + 1]] - v.sample_class_offsets[(size_t)first[g]]);
    }
    SKM_TRY(lengths_dev.ensure((size_t)n_tx));
    SKM_TRY(src.ensure((size_t)classes_max)); SKM_TRY(dst.ensure((size_t)classes_max + 1)); SKM_TRY(add.ensure((size_t)classes_max));
    if (s->keep_hist) SKM_TRY(hist.ensure((size_t)slots_max * MAX_FRAGMENT_LENGTH));
    HIP_TRY(hipStreamSynchronize(m->stream));                     // (the table, the arena and the histograms are final)
    HIP_TRY(hipMemcpyAsync(lengths_dev.p, lengths, (size_t)n_tx * 8, hipMemcpyHostToDevice, q->stream));
    const int64_t hist_rows = (int64_t)(s->hist.cap / MAX_FRAGMENT_LENGTH);     // (a sample past them has an empty histogram)
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int64_t t0 = first[g], n = first[g + 1] - t0;
        const int64_t k0 = v.sample_class_offsets[(size_t)t0], C = v.sample_class_offsets[(size_t)(t0 + n)] - k0;
        h_src.resize((size_t)C); h_dst.resize((size_t)C + 1); h_add.resize((size_t)C); h_count.resize((size_t)C);
        int64_t M = 0;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = v.sample_class_offsets[(size_t)(t0 + i)]; k < v.sample_class_offsets[(size_t)(t0 + i) + 1]; ++k) {
                const int64_t c = v.order[(size_t)k];
                h_src[(size_t)(k - k0)] = v.start[(size_t)c];
                h_dst[(size_t)(k - k0)] = M;
                h_add[(size_t)(k - k0)] = (int32_t)(i * n_tx);
                h_count[(size_t)(k - k0)] = (double)v.count[(size_t)c];
                M += v.len[(size_t)c];
            }
        h_dst[(size_t)C] = M;
        if (m->use_length_weights) {              // a fragment-length model: one row for every sample
            launch_effective_lengths_weights(m->length_weights.p, 1, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
            launch_repeat_row(q->eff_len.p, n_tx, n, q->stream);
        } else if (s->keep_hist) {
            const int64_t have = std::max<int64_t>(0, std::min(n, hist_rows - t0));
            HIP_TRY(hipMemsetAsync(hist.p, 0, (size_t)n * MAX_FRAGMENT_LENGTH * 8, q->stream));
            if (have) HIP_TRY(hipMemcpyAsync(hist.p, s->hist.p + t0 * MAX_FRAGMENT_LENGTH, (size_t)have * MAX_FRAGMENT_LENGTH * 8,
                                             hipMemcpyDeviceToDevice, q->stream));
            launch_effective_lengths_many(hist.p, n, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
        } else {
            launch_effective_lengths(m->counters.p + CTR_FLD, lengths_dev.p, n_tx, q->eff_len.p, q->stream);
            launch_repeat_row(q->eff_len.p, n_tx, n, q->stream);
        }
        if (effective_lengths)
            HIP_TRY(hipMemcpyAsync(effective_lengths + t0 * n_tx, q->eff_len.p, (size_t)(n * n_tx) * 8, hipMemcpyDeviceToHost, q->stream));
        if (C) {
            // the start vector of skm_quant_infer, per sample: reciprocal, numpy's sum, divide
            double *const totals = run.sums.p + n * ((n_tx + 8191) / 8192);
            launch_reciprocal(q->eff_len.p, n * n_tx, q->x0.p, q->stream);
            launch_np_sum_many(q->x0.p, n_tx, n, n_tx, 1.0, run.sums.p, totals, q->stream);
            launch_divide_many(q->x0.p, n_tx, n, n_tx, totals, false, 0.0, q->stream);
            HIP_TRY(hipMemcpyAsync(src.p, h_src.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(dst.p, h_dst.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(add.p, h_add.data(), (size_t)C * 4, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_offset.p, h_dst.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, q->stream));
            HIP_TRY(hipMemcpyAsync(q->cls_count.p, h_count.data(), (size_t)C * 8, hipMemcpyHostToDevice, q->stream));
            launch_stack_tuples(src.p, dst.p, add.p, C, m->arena.p, q->ids.p, q->stream);
            HIP_TRY(hipGetLastError());
        }
        SKM_TRY(set_quant_group(run, n, classes.data() + t0, total.data() + t0, C, M, rel_tol, x_floor, max_iters, true,
                                tpm + t0 * n_tx, iters ? iters + t0 : nullptr, t0));
    }
    return SKM_OK;
}

extern "C" int skm_quant_timing(skm_quant *q, double timing[4])
{
    if (!q || !timing) return fail(SKM_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(q->mu);
    timing[0] = q->t_em_ns; timing[1] = q->iters_total; timing[2] = q->launches; timing[3] = 0;
    return SKM_OK;
}

// ---------------------------------------------------------------- multi-GPU
extern "C" int skm_comm_unique_id(void *id128)
{
    if (!id128) return fail(SKM_ERR_ARG, "NULL argument");
    SKM_TRY(load_rccl());
    NCCL_TRY(g_rccl.GetUniqueId(id128));
    return SKM_OK;
}

extern "C" int skm_comm_create(int device, const void *id128, int rank, int world, skm_comm **out)
{
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return fail(SKM_ERR_ARG, "bad argument");
    SKM_TRY(check_device(device));
    SKM_TRY(set_device(device));
    SKM_TRY(load_rccl());
    UniqueId id;
    memcpy(&id, id128, sizeof(id));
    skm_comm *c = new skm_comm();
    c->device = device;
    c->rank = rank;
    c->world = world;
    int r = g_comm_init(&c->comm, world, id, rank);
    if (r != 0) {
        delete c;
        return fail(SKM_ERR_COMM, "ncclCommInitRank failed: %s",
                    g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    }
    *out = c;
    return SKM_OK;
}

extern "C" int skm_comm_count(skm_comm *c, int *count)
{
    if (!c || !count) return fail(SKM_ERR_ARG, "NULL argument");
    if (!g_rccl.CommCount) return fail(SKM_ERR_COMM, "librccl.so lacks ncclCommCount");
    NCCL_TRY(g_rccl.CommCount(c->comm, count));
    return SKM_OK;
}

// SURVEY 8(e).1 over xGMI: a mapper's table goes from GPU to GPU as it lies in HBM
// (skm_mapper_device_table's arrays, ncclSend / ncclRecv) and is merged by key on the receiving GPU
// (class_merge_kernel over the received arrays): no host copy, no host sort.  One call does both
// directions so that a rank may pair a send with a receive (two ranks swapping, or -- the one-GPU
// test -- a rank sending to itself): first the sizes (a header of eight words), then the arrays.
extern "C" int skm_mapper_exchange_tables(skm_mapper *send, int send_to, skm_mapper *recv, int recv_from, skm_comm *comm)
{
    if (!comm || (!send && !recv)) return fail(SKM_ERR_ARG, "NULL argument");
    if ((send && send_to < 0) || (recv && recv_from < 0) || send_to >= comm->world || recv_from >= comm->world)
        return fail(SKM_ERR_ARG, "peer rank outside the communicator");
    if ((send && send->ix->device != comm->device) || (recv && recv->ix->device != comm->device))
        return fail(SKM_ERR_ARG, "communicator and mapper live on different GPUs");
    SKM_TRY(load_rccl());
    if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
        return fail(SKM_ERR_COMM, "librccl.so lacks ncclSend / ncclRecv");
    SKM_TRY(set_device(comm->device));
    skm_device_table out{};
    if (send) SKM_TRY(skm_mapper_device_table(send, &out));            // (waits for what the mapper has queued)
    PoolStream stream;
    HIP_TRY(pool_stream_acquire(stream.out()));
    DBuf<unsigned long long> header, fld, first_seen;
    DBuf<int64_t> start, len;
    DBuf<double> count;
    DBuf<int32_t> ids;
    auto drain = on_exit([&]() { (void)hipStreamSynchronize(stream); });      // (every exit: before they go)
    SKM_TRY(header.ensure(16));
    unsigned long long words[16] = {(unsigned long long)out.n_classes, (unsigned long long)out.n_ids,
                                    (unsigned long long)out.unaligned, (unsigned long long)out.units,
                                    (unsigned long long)out.first_seen_bound, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(header.p, words, 8 * 8, hipMemcpyHostToDevice, stream));
    // (a group that has been started is always ended, whatever a call inside it returned)
    auto grouped = [&](const std::function<int()> &calls) -> int {
        NCCL_TRY(g_rccl.GroupStart());
        const int rc = calls();
        const int end = g_rccl.GroupEnd();
        if (rc != SKM_OK) return rc;
        NCCL_TRY(end);
        return SKM_OK;
    };
    SKM_TRY(grouped([&]() -> int {
        if (send) NCCL_TRY(g_rccl.Send(header.p, 8, NCCL_UINT64, send_to, comm->comm, stream));
        if (recv) NCCL_TRY(g_rccl.Recv(header.p + 8, 8, NCCL_UINT64, recv_from, comm->comm, stream));
        return SKM_OK;
    }));
    HIP_TRY(hipMemcpyAsync(words + 8, header.p + 8, 8 * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    skm_device_table in{};
    in.device = comm->device;
    if (recv) {
        in.n_classes = (int64_t)words[8]; in.n_ids = (int64_t)words[9];
        in.unaligned = (int64_t)words[10]; in.units = (int64_t)words[11]; in.first_seen_bound = (int64_t)words[12];
        if (in.n_classes < 0 || in.n_ids < 0 || in.n_classes >= (1LL << 40) || in.n_ids >= (1LL << 40))
            return fail(SKM_ERR_COMM, "received a table header that makes no sense");
        SKM_TRY(start.ensure(std::max<int64_t>(in.n_classes, 1))); SKM_TRY(len.ensure(std::max<int64_t>(in.n_classes, 1)));
        SKM_TRY(count.ensure(std::max<int64_t>(in.n_classes, 1))); SKM_TRY(first_seen.ensure(std::max<int64_t>(in.n_classes, 1)));
        SKM_TRY(ids.ensure(std::max<int64_t>(in.n_ids, 1))); SKM_TRY(fld.ensure(MAX_FRAGMENT_LENGTH));
    }
    SKM_TRY(grouped([&]() -> int {
    if (send) {
        if (out.n_classes) {
            NCCL_TRY(g_rccl.Send(out.class_start, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.class_len, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.class_count, (size_t)out.n_classes, NCCL_FLOAT64, send_to, comm->comm, stream));
            NCCL_TRY(g_rccl.Send(out.first_seen, (size_t)out.n_classes, NCCL_UINT64, send_to, comm->comm, stream));
        }
        if (out.n_ids) NCCL_TRY(g_rccl.Send(out.ids, (size_t)out.n_ids, NCCL_INT32, send_to, comm->comm, stream));
        NCCL_TRY(g_rccl.Send(out.fld, MAX_FRAGMENT_LENGTH, NCCL_UINT64, send_to, comm->comm, stream));
    }
    if (recv) {
        if (in.n_classes) {
            NCCL_TRY(g_rccl.Recv(start.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(len.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(count.p, (size_t)in.n_classes, NCCL_FLOAT64, recv_from, comm->comm, stream));
            NCCL_TRY(g_rccl.Recv(first_seen.p, (size_t)in.n_classes, NCCL_UINT64, recv_from, comm->comm, stream));
        }
        if (in.n_ids) NCCL_TRY(g_rccl.Recv(ids.p, (size_t)in.n_ids, NCCL_INT32, recv_from, comm->comm, stream));
        NCCL_TRY(g_rccl.Recv(fld.p, MAX_FRAGMENT_LENGTH, NCCL_UINT64, recv_from, comm->comm, stream));
    }
    return SKM_OK;
    }));
    HIP_TRY(hipStreamSynchronize(stream));
    if (!recv) return SKM_OK;
    in.class_start = start.p; in.class_len = len.p; in.class_count = count.p;
    in.first_seen = (const uint64_t *)first_seen.p; in.ids = ids.p; in.fld = (const uint64_t *)fld.p;
    return skm_mapper_merge_device(recv, &in);
}

extern "C" int skm_comm_destroy(skm_comm *c)
{
    if (!c) return SKM_OK;
    (void)hipSetDevice(c->device);
    if (c->comm && g_rccl.CommDestroy) NCCL_TRY(g_rccl.CommDestroy(c->comm));
    delete c;
    return SKM_OK;
}

extern "C" int skm_quant_set_comm(skm_quant *q, skm_comm *c)
{
    if (!q) return fail(SKM_ERR_ARG, "NULL quant");
    std::lock_guard<std::mutex> lock(q->mu);
    if (c && c->device != q->device) return fail(SKM_ERR_ARG, "communicator and quant live on different GPUs");
    q->comm = c ? c->comm : nullptr;
    q->rank = c ? c->rank : 0;
    q->world = c ? c->world : 1;
    return SKM_OK;
}
