// skm_barcode_census_* (the host glue of cell discovery in skm_abi_cells.hip, with the pool) under AddressSanitizer + UBSan,
// as a program of its own: CPU only, no GPU, no Python.  The HIP runtime calls the glue makes are stand-ins over
// host memory (below); the launchers are sequential CPU versions with the same table layout and probing
// (census_host_asan_kernels.hip).  From the repository's root:
//   F="--offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer"
//   hipcc $F -c seekmer_amd/csrc/skm_abi_cells.hip -o /tmp/ca_cells.o && hipcc $F -c seekmer_amd/csrc/skm_abi_core.hip -o /tmp/ca_core.o
//   hipcc $F -c seekmer_amd/csrc/skm_pool.hip -o /tmp/ca_pool.o
//   hipcc $F -Iinclude -Iseekmer_amd/csrc -c scripts/micro/census_host_asan_kernels.hip -o /tmp/ca_kernels.o
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -c scripts/micro/census_host_asan.cpp -o /tmp/ca_main.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined -o /tmp/census_host_asan /tmp/ca_main.o /tmp/ca_cells.o /tmp/ca_core.o \
//       /tmp/ca_pool.o /tmp/ca_kernels.o -Wl,--unresolved-symbols=ignore-all -ldl -lpthread
//   (only the units the census glue needs: skm_abi_cells.hip and, for the error message and set_device, skm_abi_core.hip.
//   The flag stays: the cells unit also holds the barcode, UMI-window and unit-grouping glue and the core unit the
//   gather probe, whose five launchers the stand-ins do not define and the program never calls)
//   ASAN_OPTIONS=detect_leaks=0 /tmp/census_host_asan        (the pool parks its blocks for the life of the process: no leak)
// 120 censuses: L in {1, 5, 16, 31, 32} x start in {0, 3, 20, 40}, ragged and uniform pieces (every other uniform piece
// without a lengths array), strided codes, empty pieces, exception planes, SKM_TEST_CENSUS_SLOTS unset, 2 and 64; size,
// ranked (exact-size arrays, order and sum checked) and pick with a cap that is too small and then exact.
#include "seekmer_hip.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>
static int run(int L, int start, bool uniform, int pieces, int stride_extra, const char *slots)
{
    if (slots) setenv("SKM_TEST_CENSUS_SLOTS", slots, 1); else unsetenv("SKM_TEST_CENSUS_SLOTS");
    std::mt19937_64 rng(L * 131 + start * 7 + pieces);
    skm_barcode_census *c = nullptr;
    if (skm_barcode_census_create(0, L, &c) != 0) { printf("create: %s\n", skm_last_error()); return 1; }
    int64_t stats[3] = {0, 0, 0}, total = 0;
    for (int p = 0; p < pieces; ++p) {
        const int64_t n = p % 7 == 3 ? 0 : 50 + (int64_t)(rng() % 400);
        const int words = (start + L + 10 + 31) / 32, stride = words + stride_extra;
        std::vector<uint64_t> codes((size_t)(n * stride) + 1);
        std::vector<uint32_t> lengths((size_t)n + 1), er, em;
        for (int64_t r = 0; r < n; ++r) {
            for (int k = 0; k < words; ++k) codes[r * stride + k] = (rng() % 5 == 0 ? ~0ULL : rng() % 3 == 0 ? 0ULL : rng()) & (rng() % 4 ? ~0ULL : 0xFFFF0000FFFFFFFFULL);
            lengths[r] = uniform ? (uint32_t)(start + L + 4) : (uint32_t)(rng() % (start + L + 11));
            if (rng() % 9 == 0) { er.push_back((uint32_t)r); for (int k = 0; k < words; ++k) em.push_back((uint32_t)rng() | (rng() % 2 ? ~0u : 0u)); }
        }
        skm_packed_reads reads{};
        reads.code_words = words; reads.n_reads = n; reads.read_stride = stride; reads.first_read = total;
        reads.uniform_len = uniform ? start + L + 4 : -1;
        reads.codes = codes.data(); reads.lengths = uniform && p % 2 ? nullptr : lengths.data();
        reads.n_exceptions = (int64_t)er.size(); reads.exception_reads = er.data(); reads.exception_masks = em.data();
        if (skm_barcode_census_add(c, &reads, start, stats) != 0) { printf("add: %s\n", skm_last_error()); return 1; }
        total += n;
    }
    int64_t distinct = 0, counted = 0;
    if (skm_barcode_census_size(c, &distinct, &counted) != 0) return 1;
    if (stats[0] + stats[1] + stats[2] != total || counted != stats[0]) { printf("stats do not add up\n"); return 1; }
    std::vector<uint64_t> keys((size_t)distinct + 1); std::vector<int64_t> counts((size_t)distinct + 1);
    if (skm_barcode_census_ranked(c, distinct, keys.data(), counts.data()) != 0) { printf("ranked: %s\n", skm_last_error()); return 1; }
    int64_t sum = 0;
    for (int64_t i = 0; i < distinct; ++i) {
        sum += counts[i];
        if (i && (counts[i] > counts[i - 1] || (counts[i] == counts[i - 1] && keys[i] <= keys[i - 1]))) { printf("not ranked at %lld\n", (long long)i); return 1; }
    }
    if (sum != counted) { printf("ranked counts %lld, counted %lld\n", (long long)sum, (long long)counted); return 1; }
    for (int64_t expect : {1LL, 150LL, 100000LL})
        for (int drop : {1, 0}) {
            int64_t info[6] = {0};
            int code = skm_barcode_census_pick(c, expect, drop, 1, keys.data(), counts.data(), info);      // a cap that is mostly too small
            if (distinct == 0) { if (code == 0) return 1; continue; }
            if (code != 0 && info[5] <= 1) { printf("pick: %s\n", skm_last_error()); return 1; }
            std::vector<uint64_t> pk((size_t)info[5]); std::vector<int64_t> pc((size_t)info[5]);
            if (skm_barcode_census_pick(c, expect, drop, info[5], pk.data(), pc.data(), info) != 0) { printf("pick: %s\n", skm_last_error()); return 1; }
            if (info[5] != info[3] - info[4] || (!drop && info[4])) return 1;
        }
    printf("L %2d start %2d %s pieces %2d stride+%d slots %-5s: %lld reads, %lld counted, %lld distinct\n", L, start, uniform ? "uniform" : "ragged ",
           pieces, stride_extra, slots ? slots : "-", (long long)total, (long long)counted, (long long)distinct);
    return skm_barcode_census_destroy(c);
}
int main()
{
    for (const char *slots : {(const char *)nullptr, "2", "64"})
        for (int L : {1, 5, 16, 31, 32})
            for (int start : {0, 3, 20, 40})
                for (int uniform : {0, 1})
                    if (run(L, start, uniform, L % 2 ? 9 : 3, start % 3, slots)) return 1;
    skm_barcode_census *c = nullptr;
    if (skm_barcode_census_create(0, 0, &c) == 0 || skm_barcode_census_create(0, 33, &c) == 0) return 1;
    puts("done");
    return 0;
}

// ---- stand-ins for the HIP runtime calls of the glue: device memory is host memory
#include <cstdlib>
#include <cstring>
#include <cstddef>
extern "C" {
int hipGetDeviceCount(int *n) { *n = 1; return 0; }
int hipSetDevice(int) { return 0; }
int hipGetDevice(int *d) { *d = 0; return 0; }
int hipMalloc(void **p, size_t n) { *p = malloc(n); return *p ? 0 : 2; }
int hipFree(void *p) { free(p); return 0; }
int hipMemcpy(void *d, const void *s, size_t n, int) { memcpy(d, s, n); return 0; }
int hipMemcpyAsync(void *d, const void *s, size_t n, int, void *) { memcpy(d, s, n); return 0; }
int hipMemset(void *d, int v, size_t n) { memset(d, v, n); return 0; }
int hipMemsetAsync(void *d, int v, size_t n, void *) { memset(d, v, n); return 0; }
int hipStreamSynchronize(void *) { return 0; }
int hipDeviceSynchronize() { return 0; }
int hipGetLastError() { return 0; }
const char *hipGetErrorString(int) { return "shim"; }
}
extern "C" {
int hipEventCreate(void **) { return 1; }
int hipEventCreateWithFlags(void **, unsigned) { return 1; }
int hipEventDestroy(void *) { return 0; }
int hipEventElapsedTime(float *, void *, void *) { return 1; }
int hipEventRecord(void *, void *) { return 1; }
int hipEventSynchronize(void *) { return 1; }
int hipHostFree(void *p) { free(p); return 0; }
int hipHostMalloc(void **p, size_t n, unsigned) { *p = malloc(n); return 0; }
int hipGetDevicePropertiesR0600(void *, int) { return 1; }
int hipMemcpy2DAsync(void *, size_t, const void *, size_t, size_t, size_t, int, void *) { return 1; }
int hipStreamCreate(void **) { return 1; }
int hipStreamCreateWithFlags(void **, unsigned) { return 1; }
int hipStreamDestroy(void *) { return 0; }
}
