// mcq_build.hip -- GPU construction of the feature -> locations table from reference sequences
// (row f2 of SURVEY.md section 8): mcq_build_table / mcq_db_build of include/mcq.h.
//
// Restates the reference's build-side insertion (add_all_window_sketches,
// src/sketch_database.h:1079-1097, with target t sketched on rank t % P, :540-542): every window of
// every target is sketched (same kernel as the query path, through mcq_sketch); per (feature,
// virtual rank) only the first max_locs = 254 locations in (target, window) order survive
// (:1090-1092); the table is the union of the P rank tables, lists in (target, window) order.
//
// Only the public C ABI of mcq_stages.hip and mcq_table.hip is used from here (mcq_count_windows, mcq_sketch,
// mcq_db_create), plus rocPRIM's radix sort for the two global sorts -- a plain library sort of
// ~3e8 pairs, run once per database, outside any timed region.
#include <cstring>
#include <chrono>
#include <cstdio>
#include <hip/hip_runtime.h>
#include <memory>
#include <rocprim/rocprim.hpp>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcq.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {
thread_local std::string g_berr;
int bfail(int code, const std::string& m) { g_berr = m; return code; }
#define BCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return bfail(MCQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define MCHK(expr) do { int r_ = (expr); if (r_ != MCQ_OK) return r_; } while (0)

// n elements of T from hipMalloc (never fewer than one), behind a move-only owner whose destructor gives them back: every way
// out of a function frees.  What the handles of this unit keep lives in these; the temporaries of a build come from Scratch.
template <class T> struct Dev {
    T* p = nullptr;
    Dev() = default;
    Dev(Dev&& o) noexcept : p(o.release()) {}
    Dev& operator=(Dev&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    ~Dev() { reset(); }
    hipError_t alloc(u64 n) { reset(); return hipMalloc(&p, (n ? n : 1) * sizeof(T)); }
    T* get() const { return p; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }
};
// The same from the device's default memory pool, in stream 0: what a handle gathers over several calls and then hands to a
// pipeline whose temporaries come from that pool (Scratch below) -- given back, its memory serves the pipeline's next buffer instead
// of being unmapped by a hipFree in the middle of a build.
template <class T> struct PoolDev {
    T* p = nullptr;
    PoolDev() = default;
    PoolDev(PoolDev&& o) noexcept : p(o.release()) {}
    PoolDev& operator=(PoolDev&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    ~PoolDev() { reset(); }
    hipError_t alloc(u64 n) { reset(); return hipMallocAsync((void**)&p, (n ? n : 1) * sizeof(T), 0); }
    T* get() const { return p; }
    void reset() { if (p) (void)hipFreeAsync(p, 0); p = nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }
};
// a half-built handle: freed by its own *_free / mcq_db_destroy unless released into *out
template <class H, int (*Free)(H*)> struct HandleFree { void operator()(H* h) const { (void)Free(h); } };
typedef std::unique_ptr<mcq_table, HandleFree<mcq_table, mcq_table_free>> TablePtr;
typedef std::unique_ptr<mcq_parts, HandleFree<mcq_parts, mcq_parts_free>> PartsPtr;
typedef std::unique_ptr<mcq_parts_builder, HandleFree<mcq_parts_builder, mcq_parts_builder_free>> BuilderPtr;
typedef std::unique_ptr<mcq_db, HandleFree<mcq_db, mcq_db_destroy>> DbPtr;

// Temporaries of one build come from the device's default memory pool with its release threshold lifted, so a buffer
// freed by one phase is handed to the next without unmapping and remapping HBM (hipMalloc / hipFree of tens of GB were
// most of the build time of a 16 Gbp input).  The destructor frees what an error path left behind, restores the
// threshold and trims the pool, so nothing stays reserved after the call.
struct Scratch {
    hipMemPool_t pool = nullptr;
    uint64_t old_threshold = 0;
    std::vector<void*> live;
    hipError_t init(int device) {
        hipError_t e = hipDeviceGetDefaultMemPool(&pool, device);
        if (e != hipSuccess) return e;
        e = hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, &old_threshold);
        if (e != hipSuccess) return e;
        uint64_t keep = ~0ull;
        return hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    template <class T> hipError_t get(T** p, u64 bytes) {
        void* q = nullptr;
        hipError_t e = hipMallocAsync(&q, bytes ? bytes : 1, 0);
        if (e == hipSuccess) { live.push_back(q); *p = static_cast<T*>(q); }
        return e;
    }
    void put(void* p) {
        if (!p) return;
        for (size_t i = 0; i < live.size(); ++i) if (live[i] == p) { live[i] = live.back(); live.pop_back(); break; }
        (void)hipFreeAsync(p, 0);
    }
    ~Scratch() {
        for (void* p : live) (void)hipFreeAsync(p, 0);
        (void)hipStreamSynchronize(0);
        if (pool) {
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &old_threshold);
            (void)hipMemPoolTrimTo(pool, 0);
        }
    }
};

const u32 TB = 256;
inline dim3 grid_for(u64 n) { u64 g = (n + TB - 1) / TB; return dim3((u32)(g < (1u << 22) ? (g ? g : 1) : (1u << 22))); }

// target of global window w: last t with win_off[t] <= w
__device__ __forceinline__ u32 target_of(const u64* win_off, u32 n_targets, u64 w) {
    u32 lo = 0, hi = n_targets;
    while (hi - lo > 1) { u32 mid = (lo + hi) >> 1; if (win_off[mid] <= w) lo = mid; else hi = mid; }
    return lo;
}

// slot i = window i / s, sketch position i % s  ->  key = feature * P + (target % P), value = global window
__global__ void k_make_pairs(const u32* feat, u64 n_slots, u32 s, const u64* win_off, u32 n_targets, u32 P, u64* key, u32* val) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const u32 f = feat[i];
        const u64 w = i / s;
        if (f == 0xFFFFFFFFu) { key[i] = ~0ull; val[i] = 0; continue; }
        const u32 t = target_of(win_off, n_targets, w);
        key[i] = (u64)f * P + (t % P);
        val[i] = (u32)w;
    }
}
// head[i] = 1 where a new key group starts (sorted keys)
__global__ void k_heads(const u64* key, u64 n, u32* head) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
__global__ void k_group_start(const u32* head, const u64* gid_excl, u64 n, u64* gstart) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) if (head[i]) gstart[gid_excl[i]] = i;
}
// keep the first max_locs entries of every (feature, rank) group
__global__ void k_keep(const u64* key, const u32* head, const u64* gid_excl, const u64* gstart, u64 n, u32 max_locs, u32* keep) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 g = gid_excl[i] + head[i] - 1;          // heads before me, plus my own, minus one
        keep[i] = (key[i] != ~0ull && (i - gstart[g]) < max_locs) ? 1u : 0u;
    }
}
__global__ void k_compact(const u64* key, const u32* val, const u32* keep, const u64* pos, u64 n, u32 P, u64* out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (keep[i]) out[pos[i]] = ((key[i] / P) << 32) | val[i];               // (feature << 32) | global window
}
// -remove-overpopulated-features: entries of features with more than `limit` locations are dropped
__global__ void k_keep_small(const u64* fw, const u32* head, const u64* kid_excl, const u64* first, u64 n, u64 n_keys, u64 limit, u32* keep) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 kx = kid_excl[i] + head[i] - 1;
        const u64 end = (kx + 1 < n_keys) ? first[kx + 1] : n;
        keep[i] = (end - first[kx] <= limit) ? 1u : 0u;
    }
}
__global__ void k_first_of_key(const u32* head, const u64* kid_excl, u64 n, u64* first) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) if (head[i]) first[kid_excl[i]] = i;
}
__global__ void k_compact_u64(const u64* in, const u32* keep, const u64* pos, u64 n, u64* out) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) if (keep[i]) out[pos[i]] = in[i];
}
__global__ void k_feat_heads(const u64* fw, u64 n, u32* head) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        head[i] = (i == 0 || (fw[i] >> 32) != (fw[i - 1] >> 32)) ? 1u : 0u;
}
__global__ void k_emit(const u64* fw, const u32* head, const u64* kid_excl, u64 n, u64 n_keys, const u64* win_off, u32 n_targets,
                       u32* keys, u64* list_off, u64* locs) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 w = fw[i] & 0xFFFFFFFFull;
        const u32 t = target_of(win_off, n_targets, w);
        locs[i] = ((u64)t << 32) | (w - win_off[t]);
        if (head[i]) { keys[kid_excl[i]] = (u32)(fw[i] >> 32); list_off[kid_excl[i]] = i; }
        if (i == 0) list_off[n_keys] = n;
    }
}

// exclusive sum scan u32 -> u64 via rocPRIM (out has n entries; total returned through *total on the host)
int excl_scan(const u32* in, u64* out, u64 n, u64* total) {
    if (n == 0) { *total = 0; return MCQ_OK; }
    size_t tmp = 0;
    auto first = rocprim::make_transform_iterator(in, [] __device__(u32 x) { return (u64)x; });
    BCHK(rocprim::exclusive_scan(nullptr, tmp, first, out, (u64)0, n, rocprim::plus<u64>()));
    Dev<char> t;
    BCHK(t.alloc(tmp));
    BCHK(rocprim::exclusive_scan(t.get(), tmp, first, out, (u64)0, n, rocprim::plus<u64>()));
    u64 last_out = 0; u32 last_in = 0;
    BCHK(hipMemcpy(&last_out, out + n - 1, 8, hipMemcpyDeviceToHost));
    BCHK(hipMemcpy(&last_in, in + n - 1, 4, hipMemcpyDeviceToHost));
    *total = last_out + last_in;
    return MCQ_OK;
}
}  // namespace

struct mcq_table {            // device arrays, freed with the handle (mcq_table_free)
    u64 n_keys = 0, n_locs = 0;
    Dev<u32> keys; Dev<u64> list_off, locs;
    Dev<u64> win_off; u32 n_targets = 0;
    int device = 0;
};

extern "C" const char* mcq_build_last_error(void) { return g_berr.c_str(); }

extern "C" int mcq_table_free(mcq_table* t) {
    if (!t) return MCQ_OK;
    (void)hipSetDevice(t->device);
    delete t;
    return MCQ_OK;
}
extern "C" int mcq_table_info(const mcq_table* t, uint64_t* n_keys, uint64_t* n_locs, const uint32_t** keys,
                              const uint64_t** list_off, const uint64_t** locs, const uint64_t** win_off) {
    if (!t) return bfail(MCQ_E_ARG, "null argument");
    if (n_keys) *n_keys = t->n_keys;
    if (n_locs) *n_locs = t->n_locs;
    if (keys) *keys = t->keys.get();
    if (list_off) *list_off = t->list_off.get();
    if (locs) *locs = t->locs.get();
    if (win_off) *win_off = t->win_off.get();
    return MCQ_OK;
}

// ---- the pipeline behind both forms of the build -----------------------------------------------------------------
// (feature * P + rank, global window) pairs in (target, window) order -> stable sort by key, first max_locs of every
// (feature, rank) group, lists of a feature merged over the ranks into (target, window) order, optionally
// -remove-overpopulated-features; leaves fw[0..n_kept) = (feature << 32) | global window sorted, head[i] = 1 where a
// feature's list starts, kid[i] = exclusive count of heads, n_keys.  Takes over key / val (both from tmpbuf).
struct Lists { u64* fw = nullptr; u32* head = nullptr; u64* kid = nullptr; u64 n_kept = 0, n_keys = 0; };
template <class Phase>
static int sort_truncate(Scratch& tmpbuf, u64* key, u32* val, u64 n, u32 P, u32 max_locs, bool remove_overpop, Lists& L, Phase phase) {
    u64* key2 = nullptr; u32* val2 = nullptr;
    BCHK(tmpbuf.get(&key2, (n ? n : 1) * 8)); BCHK(tmpbuf.get(&val2, (n ? n : 1) * 4));
    if (n) {
        // keys are feature * P + rank < 2^32 * P: only these bits take part in the sort
        u32 key_bits = 32; while (key_bits < 64 && (((u64)P - 1) >> (key_bits - 32))) ++key_bits;
        size_t tmp = 0;
        BCHK(rocprim::radix_sort_pairs(nullptr, tmp, key, key2, val, val2, n, 0, key_bits));
        void* t = nullptr; BCHK(tmpbuf.get(&t, tmp ? tmp : 1));
        BCHK(rocprim::radix_sort_pairs(t, tmp, key, key2, val, val2, n, 0, key_bits));
        BCHK(hipDeviceSynchronize());
        tmpbuf.put(t);
    }
    tmpbuf.put(key); tmpbuf.put(val);
    phase("sort by (feature, rank)");

    // rank inside each group, keep the first max_locs
    u32 *head = nullptr, *keep = nullptr; u64 *gid = nullptr, *gstart = nullptr, *pos = nullptr;
    BCHK(tmpbuf.get(&head, (n ? n : 1) * 4)); BCHK(tmpbuf.get(&keep, (n ? n : 1) * 4));
    BCHK(tmpbuf.get(&gid, (n ? n : 1) * 8)); BCHK(tmpbuf.get(&pos, (n ? n : 1) * 8));
    u64 n_groups = 0, n_kept = 0;
    if (n) hipLaunchKernelGGL(k_heads, grid_for(n), dim3(TB), 0, 0, key2, n, head);
    MCHK(excl_scan(head, gid, n, &n_groups));
    BCHK(tmpbuf.get(&gstart, (n_groups ? n_groups : 1) * 8));
    if (n) {
        hipLaunchKernelGGL(k_group_start, grid_for(n), dim3(TB), 0, 0, head, gid, n, gstart);
        hipLaunchKernelGGL(k_keep, grid_for(n), dim3(TB), 0, 0, key2, head, gid, gstart, n, max_locs, keep);
    }
    MCHK(excl_scan(keep, pos, n, &n_kept));
    u64* fw = nullptr;
    BCHK(tmpbuf.get(&fw, (n_kept ? n_kept : 1) * 8));
    if (n) hipLaunchKernelGGL(k_compact, grid_for(n), dim3(TB), 0, 0, key2, val2, keep, pos, n, P, fw);
    BCHK(hipDeviceSynchronize());
    tmpbuf.put(key2); tmpbuf.put(val2); tmpbuf.put(keep); tmpbuf.put(gid); tmpbuf.put(gstart); tmpbuf.put(pos);
    phase("truncate to max_locs");

    // merge the virtual ranks' lists of a feature into (target, window) order
    if (P > 1 && n_kept) {
        u64* fw2 = nullptr; BCHK(tmpbuf.get(&fw2, n_kept * 8));
        size_t tmp = 0;
        BCHK(rocprim::radix_sort_keys(nullptr, tmp, fw, fw2, n_kept, 0, 64));
        void* t = nullptr; BCHK(tmpbuf.get(&t, tmp ? tmp : 1));
        BCHK(rocprim::radix_sort_keys(t, tmp, fw, fw2, n_kept, 0, 64));
        BCHK(hipDeviceSynchronize());
        tmpbuf.put(t); tmpbuf.put(fw);
        fw = fw2;
    }
    phase("merge ranks");
    u64* kid = nullptr; u64 n_keys = 0;
    tmpbuf.put(head);
    BCHK(tmpbuf.get(&head, (n_kept ? n_kept : 1) * 4)); BCHK(tmpbuf.get(&kid, (n_kept ? n_kept : 1) * 8));
    if (n_kept) hipLaunchKernelGGL(k_feat_heads, grid_for(n_kept), dim3(TB), 0, 0, fw, n_kept, head);
    MCHK(excl_scan(head, kid, n_kept, &n_keys));
    if (remove_overpop && n_kept && max_locs > 1) {
        u64 *first = nullptr, *pos2 = nullptr, *fw2 = nullptr; u32* keep2 = nullptr; u64 n2 = 0;
        BCHK(tmpbuf.get(&first, (n_keys ? n_keys : 1) * 8)); BCHK(tmpbuf.get(&pos2, n_kept * 8)); BCHK(tmpbuf.get(&keep2, n_kept * 4));
        hipLaunchKernelGGL(k_first_of_key, grid_for(n_kept), dim3(TB), 0, 0, head, kid, n_kept, first);
        hipLaunchKernelGGL(k_keep_small, grid_for(n_kept), dim3(TB), 0, 0, fw, head, kid, first, n_kept, n_keys, (u64)max_locs - 1, keep2);
        MCHK(excl_scan(keep2, pos2, n_kept, &n2));
        BCHK(tmpbuf.get(&fw2, (n2 ? n2 : 1) * 8));
        hipLaunchKernelGGL(k_compact_u64, grid_for(n_kept), dim3(TB), 0, 0, fw, keep2, pos2, n_kept, fw2);
        BCHK(hipDeviceSynchronize());
        tmpbuf.put(first); tmpbuf.put(pos2); tmpbuf.put(keep2); tmpbuf.put(fw);
        fw = fw2; n_kept = n2;
        if (n_kept) hipLaunchKernelGGL(k_feat_heads, grid_for(n_kept), dim3(TB), 0, 0, fw, n_kept, head);
        MCHK(excl_scan(head, kid, n_kept, &n_keys));
    }
    L.fw = fw; L.head = head; L.kid = kid; L.n_kept = n_kept; L.n_keys = n_keys;
    return MCQ_OK;
}

// What mcq_build_table ends in, for a pass of the range build (the one-piece builds keep the text they have): keys, offsets and
// (target, window) locations of T (win_off and n_targets are set) from the sorted lists; gives fw / head / kid back to tmpbuf.
static int emit_table(Scratch& tmpbuf, mcq_table& T, const Lists& L) {
    T.n_keys = L.n_keys; T.n_locs = L.n_kept;
    BCHK(T.keys.alloc(L.n_keys)); BCHK(T.list_off.alloc(L.n_keys + 1));
    BCHK(T.locs.alloc(L.n_kept));
    if (L.n_kept) hipLaunchKernelGGL(k_emit, grid_for(L.n_kept), dim3(TB), 0, 0, (const u64*)L.fw, (const u32*)L.head, (const u64*)L.kid, L.n_kept, L.n_keys,
                                     (const u64*)T.win_off.get(), T.n_targets, T.keys.get(), T.list_off.get(), T.locs.get());
    else BCHK(hipMemset(T.list_off.get(), 0, 8));
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    tmpbuf.put(L.fw); tmpbuf.put(L.head); tmpbuf.put(L.kid);
    return MCQ_OK;
}

struct PhaseTrace {
    bool on; std::chrono::steady_clock::time_point last;
    PhaseTrace() : on(getenv("MCQ_BUILD_TRACE") != nullptr), last(std::chrono::steady_clock::now()) {}
    void operator()(const char* name) {        // MCQ_BUILD_TRACE=1: phase times on stderr (adds a device synchronisation per phase)
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mcq_build] %-28s %8.3f s\n", name, std::chrono::duration<double>(now - last).count());
        last = now;
    }
};

// a key-less handle carries the sketching parameters of a build; null (and the error text set) when they are refused
static DbPtr make_sketch_handle(const mcq_build_desc* d) {
    mcq_db_desc sd; std::memset(&sd, 0, sizeof(sd));
    sd.k = d->k; sd.sketch_size = d->sketch_size; sd.winlen = d->winlen; sd.winstride = d->winstride;
    const u64 zero = 0; sd.list_off = &zero; sd.n_shards = 1; sd.device = d->device;
    mcq_db* sk = nullptr;
    if (mcq_db_create(&sd, &sk) != MCQ_OK) { bfail(MCQ_E_ARG, std::string("sketch parameters: ") + mcq_last_error()); return DbPtr(); }
    return DbPtr(sk);
}

extern "C" int mcq_build_table(const mcq_build_desc* d, mcq_table** out) {
    if (!d || !out || !d->seq_off || (d->n_targets && !d->bases)) return bfail(MCQ_E_ARG, "null argument");
    if (d->n_targets < 1) return bfail(MCQ_E_ARG, "no targets");
    const u32 P = d->emulate_ranks ? d->emulate_ranks : 1;
    const u32 max_locs = d->max_locs ? d->max_locs : 254;
    BCHK(hipSetDevice(d->device));
    Scratch tmpbuf;
    BCHK(tmpbuf.init(d->device));
    const bool dev = (d->flags & MCQ_DEVICE_PTRS) != 0;
    const u32 nt = d->n_targets;
    PhaseTrace phase;

    // inputs on the device
    const char* bases = d->bases; const u64* seq_off = d->seq_off;
    char* t_bases = nullptr; u64* t_off = nullptr;
    if (!dev) {
        const u64 nb = d->seq_off[nt];
        BCHK(tmpbuf.get(&t_bases, nb ? nb : 1)); BCHK(tmpbuf.get(&t_off, (u64)(nt + 1) * 8));
        if (nb) BCHK(hipMemcpy(t_bases, d->bases, nb, hipMemcpyHostToDevice));
        BCHK(hipMemcpy(t_off, d->seq_off, (u64)(nt + 1) * 8, hipMemcpyHostToDevice));
        bases = t_bases; seq_off = t_off;
    }
    DbPtr sk = make_sketch_handle(d);
    if (!sk) return MCQ_E_ARG;

    TablePtr T(new mcq_table());
    T->device = d->device; T->n_targets = nt;
    BCHK(T->win_off.alloc((u64)nt + 1));
    u64* const win_off = T->win_off.get();
    mcq_batch b; b.n_seqs = nt; b.bases = bases; b.seq_off = seq_off; b.paired = 0; b.flags = MCQ_DEVICE_PTRS;
    MCHK(mcq_count_windows(sk.get(), &b, win_off, nullptr));
    u64 n_win = 0;
    BCHK(hipMemcpy(&n_win, win_off + nt, 8, hipMemcpyDeviceToHost));
    if (n_win >= (1ull << 32)) return bfail(MCQ_E_UNSUPPORTED, "more than 2^32 windows");
    const u32 s = d->sketch_size;
    const u64 n = n_win * s;
    u32 *feat = nullptr, *nfeat = nullptr;
    BCHK(tmpbuf.get(&feat, (n ? n : 1) * 4)); BCHK(tmpbuf.get(&nfeat, (n_win ? n_win : 1) * 4));
    MCHK(mcq_sketch(sk.get(), &b, win_off, feat, nfeat, nullptr));
    BCHK(hipDeviceSynchronize());
    sk.reset();
    tmpbuf.put(nfeat);
    phase("windows + sketches");

    // (feature * P + rank, global window) in window order
    u64* key = nullptr; u32* val = nullptr;
    BCHK(tmpbuf.get(&key, (n ? n : 1) * 8)); BCHK(tmpbuf.get(&val, (n ? n : 1) * 4));
    if (n) hipLaunchKernelGGL(k_make_pairs, grid_for(n), dim3(TB), 0, 0, feat, n, s, win_off, nt, P, key, val);
    tmpbuf.put(feat);
    phase("pairs");
    Lists L;
    MCHK(sort_truncate(tmpbuf, key, val, n, P, max_locs, (d->flags & MCQ_BUILD_REMOVE_OVERPOPULATED) != 0, L, phase));
    // keys, offsets, (target, window) locations
    T->n_keys = L.n_keys; T->n_locs = L.n_kept;
    BCHK(T->keys.alloc(L.n_keys)); BCHK(T->list_off.alloc(L.n_keys + 1));
    BCHK(T->locs.alloc(L.n_kept));
    if (L.n_kept) hipLaunchKernelGGL(k_emit, grid_for(L.n_kept), dim3(TB), 0, 0, L.fw, L.head, L.kid, L.n_kept, L.n_keys, win_off, nt, T->keys.get(), T->list_off.get(), T->locs.get());
    else BCHK(hipMemset(T->list_off.get(), 0, 8));
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    tmpbuf.put(L.fw); tmpbuf.put(L.head); tmpbuf.put(L.kid);
    phase("emit keys / offsets / locations");
    if (t_bases) tmpbuf.put(t_bases);
    if (t_off) tmpbuf.put(t_off);
    *out = T.release();
    return MCQ_OK;
}

// ---- the build in parts: tables whose one-piece temporaries do not fit (RefSeq scale) -------------------------------
// The features are cut into R ranges of h2(feature) (sub-ranges of the shard's range when the table is sharded: the same
// hash as mcq_owner, so a part never crosses a shard).  Pass p sketches every target again (the sketch is the cheap part:
// ~40 Gbp/s), in chunks of whole targets, keeps the features of range p -- flags, scan, scatter: (target, window) order is
// kept, which the stable sort relies on -- and runs the pipeline above on them; what is left of a pass is its part of the
// table in the form the query side stores: keys, list lengths, 32-bit global-window words.
struct mcq_parts {
    int device = 0; u32 n_targets = 0;
    u32 k = 0, s = 0, winlen = 0, winstride = 0;      // what the handle sketches QUERIES with
    u32 tgt_winstride = 0;            // window stride of the targets (range width of the candidates); 0 = winstride
    u64 n_windows = 0;
    Dev<u32> tgt_windows;     // device [n_targets]
    struct Part { Dev<u32> keys, list_len, locs; };
    std::vector<Part> own;            // the arrays of every part ...
    std::vector<mcq_db_part> parts;   // ... and what mcq_db_create_parts reads of them (filled by emit_part)
    u64 n_keys = 0, n_locs = 0, bytes = 0;
};
namespace {
__device__ __forceinline__ u32 tmh_dev(u32 x) {        // thomas_mueller_hash (src/hash_int.h:39-45), as mcq_owner
    x = ((x >> 16) ^ x) * 0x45d9f3bu; x = ((x >> 16) ^ x) * 0x45d9f3bu; return (x >> 16) ^ x;
}
__global__ void k_part_flags(const u32* feat, u64 n, u32 n_ranges, u32 range, u32* flag) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u32 f = feat[i];
        flag[i] = (f != 0xFFFFFFFFu && (u32)(((u64)tmh_dev(f) * n_ranges) >> 32) == range) ? 1u : 0u;
    }
}
// chunk slot i = window w0 + i / s; kept slots go to key / val at cursor + pos[i]
__global__ void k_part_scatter(const u32* feat, const u32* flag, const u64* pos, u64 n, u32 s, u64 w0, const u64* win_off, u32 n_targets, u32 P,
                               u64 cursor, u64 cap, u64* key, u32* val) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (!flag[i]) continue;
        const u64 o = cursor + pos[i];
        if (o >= cap) continue;                       // (reported by the host from the counts)
        const u64 w = w0 + i / s;
        const u32 t = P > 1 ? target_of(win_off, n_targets, w) : 0u;
        key[o] = (u64)feat[i] * P + (P > 1 ? t % P : 0u);
        val[o] = (u32)w;
    }
}
__global__ void k_shift_off(const u64* in, u64 n, u64 base, u64* out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] - base;
}
__global__ void k_windows_of(const u64* win_off, u32 n_targets, u32* out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_targets) out[i] = (u32)(win_off[i + 1] - win_off[i]);
}
// part arrays from the sorted lists: the key of every list and the words themselves (lengths: k_part_first + k_part_len)
__global__ void k_emit_part(const u64* fw, const u32* head, const u64* kid, u64 n, u32* keys, u32* locs) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        locs[i] = (u32)fw[i];
        if (head[i]) keys[kid[i]] = (u32)(fw[i] >> 32);
    }
}
__global__ void k_part_first(const u32* head, const u64* kid, u64 n, u64* first) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) if (head[i]) first[kid[i]] = i;
}
__global__ void k_part_len(const u64* first, u64 n_keys, u64 n, u32* list_len) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_keys) list_len[i] = (u32)(((i + 1 < n_keys) ? first[i + 1] : n) - first[i]);
}
}  // namespace

extern "C" int mcq_parts_free(mcq_parts* p) {
    if (!p) return MCQ_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return MCQ_OK;
}
extern "C" int mcq_parts_info(const mcq_parts* p, uint64_t* n_keys, uint64_t* n_locs, uint64_t* n_windows, uint32_t* n_parts, uint64_t* bytes) {
    if (!p) return bfail(MCQ_E_ARG, "null argument");
    if (n_keys) *n_keys = p->n_keys;
    if (n_locs) *n_locs = p->n_locs;
    if (n_windows) *n_windows = p->n_windows;
    if (n_parts) *n_parts = (u32)p->parts.size();
    if (bytes) *bytes = p->bytes;
    return MCQ_OK;
}

// One part of R from sorted lists (fw / head / kid as sort_truncate leaves them, all null for an empty range): keys, list lengths
// and words, owned by R from the first allocation on.  Gives fw / head / kid back to tmpbuf.
static int emit_part(Scratch& tmpbuf, mcq_parts& R, u64* fw, u32* head, u64* kid, u64 n_locs, u64 n_keys) {
    R.own.emplace_back();
    mcq_parts::Part& o = R.own.back();
    BCHK(o.keys.alloc(n_keys)); BCHK(o.list_len.alloc(n_keys)); BCHK(o.locs.alloc(n_locs));
    mcq_db_part q; q.n_keys = n_keys; q.n_locs = n_locs; q.keys = o.keys.get(); q.list_len = o.list_len.get(); q.locs = o.locs.get();
    R.parts.push_back(q);
    if (n_locs) {
        u64* first = nullptr;
        BCHK(tmpbuf.get(&first, (n_keys ? n_keys : 1) * 8));
        hipLaunchKernelGGL(k_part_first, grid_for(n_locs), dim3(TB), 0, 0, (const u32*)head, (const u64*)kid, n_locs, first);
        hipLaunchKernelGGL(k_part_len, grid_for(n_keys), dim3(TB), 0, 0, (const u64*)first, n_keys, n_locs, o.list_len.get());
        hipLaunchKernelGGL(k_emit_part, grid_for(n_locs), dim3(TB), 0, 0, (const u64*)fw, (const u32*)head, (const u64*)kid, n_locs, o.keys.get(), o.locs.get());
        BCHK(hipDeviceSynchronize());
        BCHK(hipGetLastError());
        tmpbuf.put(first);
    }
    tmpbuf.put(fw); tmpbuf.put(head); tmpbuf.put(kid);
    R.n_keys += n_keys; R.n_locs += n_locs; R.bytes += n_keys * 8 + n_locs * 4;
    return MCQ_OK;
}

// ---- one pass over the sequences for one feature range: what mcq_build_parts and mcq_range_build_next share ----
// The windows of every target (device: win_off, host: h_win) and the chunks of whole targets the sequences are sketched in
// (MCQ_BUILD_CHUNK_WINDOWS: tuning knob / test hook).
struct RangePlan {
    std::vector<u64> h_win; std::vector<u32> cut; u64 largest = 0, n_win = 0;
    u64 chunk_bytes(u32 s) const { return largest * s * 16 + largest * 4; }     // feat, flag, pos of a chunk's slots; nfeat
};
static int plan_ranges(mcq_db* sk, const mcq_build_desc* d, u64* win_off, RangePlan& pl) {
    const u32 nt = d->n_targets;
    mcq_batch b; b.n_seqs = nt; b.bases = d->bases; b.seq_off = d->seq_off; b.paired = 0; b.flags = MCQ_DEVICE_PTRS; b.n_bases = 0;
    MCHK(mcq_count_windows(sk, &b, win_off, nullptr));
    pl.h_win.resize((size_t)nt + 1);
    BCHK(hipMemcpy(pl.h_win.data(), win_off, (u64)(nt + 1) * 8, hipMemcpyDeviceToHost));
    pl.n_win = pl.h_win[nt];
    if (pl.n_win >= 0xFFFFFFFFull) return bfail(MCQ_E_UNSUPPORTED, "2^32 - 1 windows or more");
    u64 chunk_win = 1ull << 24;
    if (const char* e = getenv("MCQ_BUILD_CHUNK_WINDOWS")) chunk_win = std::max<u64>(1, strtoull(e, nullptr, 10));
    pl.cut.assign(1, 0u);
    pl.largest = 0;
    for (u32 t = 0; t < nt;) {
        u32 e = t + 1;
        while (e < nt && pl.h_win[e + 1] - pl.h_win[t] <= chunk_win) ++e;
        pl.largest = std::max(pl.largest, pl.h_win[e] - pl.h_win[t]);
        pl.cut.push_back(e); t = e;
    }
    return MCQ_OK;
}
// what one pass may keep in flight: a third of the free memory without the chunk's buffers, at least 1 GiB
static int pass_budget(u64 chunk_bytes, u64* budget) {
    size_t mem_free = 0, mem_total = 0;
    BCHK(hipMemGetInfo(&mem_free, &mem_total));
    *budget = mem_free / 3 > chunk_bytes + (1ull << 30) ? mem_free / 3 - chunk_bytes : (1ull << 30);
    return MCQ_OK;
}
// the buffers of one chunk: sketches, features per window, range flags and their scan, the chunk's own window offsets
struct ChunkBufs {
    u32 *feat = nullptr, *nfeat = nullptr, *flag = nullptr; u64 *pos = nullptr, *woff = nullptr;
    int get(Scratch& tmpbuf, u64 largest, u32 s, u32 nt) {
        BCHK(tmpbuf.get(&feat, std::max<u64>(1, largest * s) * 4)); BCHK(tmpbuf.get(&nfeat, std::max<u64>(1, largest) * 4));
        BCHK(tmpbuf.get(&flag, std::max<u64>(1, largest * s) * 4)); BCHK(tmpbuf.get(&pos, std::max<u64>(1, largest * s) * 8));
        BCHK(tmpbuf.get(&woff, ((u64)nt + 1) * 8));
        return MCQ_OK;
    }
    void put(Scratch& tmpbuf) { tmpbuf.put(feat); tmpbuf.put(nfeat); tmpbuf.put(flag); tmpbuf.put(pos); tmpbuf.put(woff); }
};
// Range `range` of n_ranges: every target is sketched again, chunk by chunk; the slots whose feature falls into the range are kept
// (flags, scan, scatter: (target, window) order stays) in pair arrays that start with room for `cap` pairs (MCQ_BUILD_PART_CAP: test
// hook) and grow; sort_truncate leaves the range's lists in L.
template <class Phase>
static int range_pass(Scratch& tmpbuf, mcq_db* sk, const mcq_build_desc* d, const u64* win_off, const RangePlan& pl, const ChunkBufs& cb,
                      u32 n_ranges, u32 range, u64 cap, Lists& L, Phase& phase) {
    const u32 P = d->emulate_ranks ? d->emulate_ranks : 1, max_locs = d->max_locs ? d->max_locs : 254;
    const u32 nt = d->n_targets, s = d->sketch_size;
    u64* key = nullptr; u32* val = nullptr;
    u64 cap_p = cap;
    if (const char* e = getenv("MCQ_BUILD_PART_CAP")) cap_p = std::max<u64>(1, strtoull(e, nullptr, 10));      // test hook: start small, grow
    BCHK(tmpbuf.get(&key, cap_p * 8)); BCHK(tmpbuf.get(&val, cap_p * 4));
    u64 cursor = 0;
    for (size_t c = 0; c + 1 < pl.cut.size(); ++c) {
        const u32 t0 = pl.cut[c], t1 = pl.cut[c + 1];
        const u64 w0 = pl.h_win[t0], nw = pl.h_win[t1] - w0, ns = nw * s;
        if (!nw) continue;
        hipLaunchKernelGGL(k_shift_off, dim3((t1 - t0 + 1 + TB - 1) / TB), dim3(TB), 0, 0, (const u64*)(win_off + t0), (u64)(t1 - t0) + 1, w0, cb.woff);
        mcq_batch b; b.n_seqs = t1 - t0; b.bases = d->bases; b.seq_off = d->seq_off + t0; b.paired = 0; b.flags = MCQ_DEVICE_PTRS; b.n_bases = 0;
        MCHK(mcq_sketch(sk, &b, cb.woff, cb.feat, cb.nfeat, nullptr));
        hipLaunchKernelGGL(k_part_flags, grid_for(ns), dim3(TB), 0, 0, (const u32*)cb.feat, ns, n_ranges, range, cb.flag);
        u64 kept = 0;
        MCHK(excl_scan(cb.flag, cb.pos, ns, &kept));
        if (cursor + kept > cap_p) {
            // more than the even share + 3 %: real data is not uniform -- features that repeat millions of times (low-complexity
            // minimisers, rRNA, IS copies) all land in ONE range before the 254-per-feature limit applies.  The pair arrays of
            // this range grow (half again, at least what is needed) instead of failing (until r04: MCQ_E_CAPACITY and the advice
            // to ask for more parts, which shrinks the cap as well)
            const u64 ncap = std::max<u64>(cursor + kept, cap_p + cap_p / 2);
            u64* key2 = nullptr; u32* val2 = nullptr;
            BCHK(tmpbuf.get(&key2, ncap * 8)); BCHK(tmpbuf.get(&val2, ncap * 4));
            if (cursor) { BCHK(hipMemcpyAsync(key2, key, cursor * 8, hipMemcpyDeviceToDevice, 0)); BCHK(hipMemcpyAsync(val2, val, cursor * 4, hipMemcpyDeviceToDevice, 0)); }
            BCHK(hipStreamSynchronize(0));
            tmpbuf.put(key); tmpbuf.put(val);
            key = key2; val = val2; cap_p = ncap;
        }
        hipLaunchKernelGGL(k_part_scatter, grid_for(ns), dim3(TB), 0, 0, (const u32*)cb.feat, (const u32*)cb.flag, (const u64*)cb.pos, ns, s, w0,
                           win_off, nt, P, cursor, cap_p, key, val);
        cursor += kept;
    }
    BCHK(hipDeviceSynchronize());
    phase("  sketch + keep the range's features");
    return sort_truncate(tmpbuf, key, val, cursor, P, max_locs, (d->flags & MCQ_BUILD_REMOVE_OVERPOPULATED) != 0, L, phase);
}

extern "C" int mcq_build_parts(const mcq_build_desc* d, mcq_parts** out) {
    if (!d || !out || !d->seq_off || (d->n_targets && !d->bases)) return bfail(MCQ_E_ARG, "null argument");
    if (d->n_targets < 1) return bfail(MCQ_E_ARG, "no targets");
    if (!(d->flags & MCQ_DEVICE_PTRS)) return bfail(MCQ_E_ARG, "mcq_build_parts takes device pointers (the sequences of such a table do not fit a staging copy)");
    const u32 n_shards = d->n_shards ? d->n_shards : 1;
    if (d->shard_id >= n_shards) return bfail(MCQ_E_ARG, "shard_id >= n_shards");
    BCHK(hipSetDevice(d->device));
    Scratch tmpbuf;
    BCHK(tmpbuf.init(d->device));
    const u32 nt = d->n_targets, s = d->sketch_size;
    PhaseTrace phase;
    DbPtr sk = make_sketch_handle(d);
    if (!sk) return MCQ_E_ARG;

    PartsPtr R(new mcq_parts());
    R->device = d->device; R->n_targets = nt; R->k = d->k; R->s = s; R->winlen = d->winlen; R->winstride = d->winstride;

    // windows of every target, chunks of whole targets for the sketch
    u64* win_off = nullptr;
    BCHK(tmpbuf.get(&win_off, (u64)(nt + 1) * 8));
    RangePlan plan;
    MCHK(plan_ranges(sk.get(), d, win_off, plan));
    const u64 n_win = plan.n_win;
    R->n_windows = n_win;
    BCHK(R->tgt_windows.alloc(nt));
    hipLaunchKernelGGL(k_windows_of, dim3((nt + TB - 1) / TB), dim3(TB), 0, 0, (const u64*)win_off, nt, R->tgt_windows.get());
    phase("windows");

    // number of parts: what one pass keeps in flight (44 B per pair at its peak, plus the chunk's buffers) against a third of the
    // free memory (MCQ_BUILD_PARTS: tuning knob / test hook)
    const u64 n_slots_mine = (n_win * s + n_shards - 1) / n_shards;
    u64 budget = 0;
    MCHK(pass_budget(plan.chunk_bytes(s), &budget));
    u32 n_parts = (u32)std::max<u64>(1, (n_slots_mine * 44 + budget - 1) / budget);
    if (const char* e = getenv("MCQ_BUILD_PARTS")) n_parts = (u32)std::max<u64>(1, strtoull(e, nullptr, 10));
    if ((u64)n_parts * n_shards > (1u << 20)) return bfail(MCQ_E_UNSUPPORTED, "too many parts");
    const u32 n_ranges = n_parts * n_shards;
    // a range's share of the slots to start with: the hash spreads distinct features evenly (3 % and 2^20 slack; a range that holds
    // more -- repeats -- grows, see range_pass)
    const u64 cap = (u64)((double)n_slots_mine / n_parts * 1.03) + (1ull << 20);

    ChunkBufs cb;
    MCHK(cb.get(tmpbuf, plan.largest, s, nt));
    for (u32 p = 0; p < n_parts; ++p) {
        Lists L;
        MCHK(range_pass(tmpbuf, sk.get(), d, win_off, plan, cb, n_ranges, d->shard_id * n_parts + p, cap, L, phase));
        MCHK(emit_part(tmpbuf, *R, L.fw, L.head, L.kid, L.n_kept, L.n_keys));
        phase("  part emitted");
    }
    cb.put(tmpbuf); tmpbuf.put(win_off);
    *out = R.release();
    return MCQ_OK;
}

// ---- the build in ranges that keeps (target, window) lists: one mcq_table per feature range (mcq_range_build_* of include/mcq.h) ----
// The ranges and the pass are those of mcq_build_parts (range_pass); a range ends in k_emit, as mcq_build_table does, so its table
// has the rank structure that mcq_table_rank_split and mcq_table_shard_records need.  The handle keeps the windows of the targets,
// the chunk cuts, the sketching handle and, as the one call of mcq_build_parts does for all its parts, ONE Scratch and one set of
// chunk buffers for all its passes: what a pass gives back serves the next one, and the pool is trimmed once, when the handle goes.
struct mcq_range_build {
    mcq_build_desc d;                 // (bases and seq_off stay the caller's, on the device)
    u32 n_ranges = 1, next = 0;
    DbPtr sk;
    Dev<u64> win_off;                 // device [n_targets + 1]
    RangePlan plan;
    u64 cap = 0;                      // pairs a pass makes room for to start with
    Scratch tmpbuf;                   // the temporaries of every pass (what an error leaves in it goes with the handle)
    ChunkBufs cb;
};
typedef std::unique_ptr<mcq_range_build, HandleFree<mcq_range_build, mcq_range_build_free>> RangeBuildPtr;

extern "C" int mcq_range_build_free(mcq_range_build* b) {
    if (!b) return MCQ_OK;
    (void)hipSetDevice(b->d.device);
    delete b;
    return MCQ_OK;
}

extern "C" int mcq_range_build_create(const mcq_build_desc* d, uint32_t n_ranges, mcq_range_build** out) {
    if (!d || !out || !d->seq_off || (d->n_targets && !d->bases)) return bfail(MCQ_E_ARG, "null argument");
    if (d->n_targets < 1) return bfail(MCQ_E_ARG, "no targets");
    if (!(d->flags & MCQ_DEVICE_PTRS)) return bfail(MCQ_E_ARG, "mcq_range_build_create takes device pointers (as mcq_build_parts)");
    if (d->n_shards > 1) return bfail(MCQ_E_ARG, "mcq_range_build_* builds the whole table (n_shards must be 0 or 1)");
    if (n_ranges > (1u << 20)) return bfail(MCQ_E_UNSUPPORTED, "too many ranges (at most 2^20)");
    BCHK(hipSetDevice(d->device));
    RangeBuildPtr b(new mcq_range_build());
    b->d = *d;
    b->sk = make_sketch_handle(d);
    if (!b->sk) return MCQ_E_ARG;
    BCHK(b->win_off.alloc((u64)d->n_targets + 1));
    MCHK(plan_ranges(b->sk.get(), d, b->win_off.get(), b->plan));
    const u64 n_slots = b->plan.n_win * d->sketch_size;
    if (!n_ranges) {
        // per pair of a range: 44 B of the pass at its peak, the range's table (12 B per key, 8 B per location: at most one key and
        // one location per pair) and the record block of the largest rank (21 B per key, 8 B per location: all of them, at worst) --
        // 93 B, against what mcq_build_parts allows one pass
        u64 budget = 0;
        MCHK(pass_budget(b->plan.chunk_bytes(d->sketch_size), &budget));
        const u64 r = std::max<u64>(1, (n_slots * (44 + 20 + 29) + budget - 1) / budget);
        if (r > (1u << 20)) return bfail(MCQ_E_UNSUPPORTED, "too many ranges (at most 2^20)");
        n_ranges = (u32)r;
    }
    b->n_ranges = n_ranges;
    b->cap = (u64)((double)n_slots / n_ranges * 1.03) + (1ull << 20);
    BCHK(b->tmpbuf.init(d->device));
    MCHK(b->cb.get(b->tmpbuf, b->plan.largest, d->sketch_size, d->n_targets));
    BCHK(hipDeviceSynchronize());
    *out = b.release();
    return MCQ_OK;
}

extern "C" int mcq_range_build_info(const mcq_range_build* b, uint32_t* n_ranges, uint32_t* next_range, uint64_t* n_windows) {
    if (!b) return bfail(MCQ_E_ARG, "null argument");
    if (n_ranges) *n_ranges = b->n_ranges;
    if (next_range) *next_range = b->next;
    if (n_windows) *n_windows = b->plan.n_win;
    return MCQ_OK;
}

extern "C" int mcq_range_build_tgt_windows(const mcq_range_build* b, uint32_t* out) {
    if (!b || !out) return bfail(MCQ_E_ARG, "null argument");
    for (u32 t = 0; t < b->d.n_targets; ++t) out[t] = (u32)(b->plan.h_win[t + 1] - b->plan.h_win[t]);
    return MCQ_OK;
}

extern "C" int mcq_range_build_next(mcq_range_build* b, mcq_table** out) {
    if (!b || !out) return bfail(MCQ_E_ARG, "null argument");
    *out = nullptr;
    if (b->next >= b->n_ranges) return MCQ_OK;
    BCHK(hipSetDevice(b->d.device));
    PhaseTrace phase;
    const u32 nt = b->d.n_targets;
    TablePtr T(new mcq_table());
    T->device = b->d.device; T->n_targets = nt;
    BCHK(T->win_off.alloc((u64)nt + 1));
    BCHK(hipMemcpy(T->win_off.get(), b->win_off.get(), ((u64)nt + 1) * 8, hipMemcpyDeviceToDevice));
    Lists L;
    MCHK(range_pass(b->tmpbuf, b->sk.get(), &b->d, b->win_off.get(), b->plan, b->cb, b->n_ranges, b->next, b->cap, L, phase));
    MCHK(emit_table(b->tmpbuf, *T, L));
    phase("  range emitted");
    ++b->next;
    *out = T.release();
    return MCQ_OK;
}


// ---- parts from streamed (feature, target, window) triples: the reference's shard files without a host-side union --------------
// (include/mcq.h, mcq_parts_builder_*; the host side is mcq_refdb_open_meta + mcq_shard_stream_* of include/mcq_host.h.)
// A chunk of triples becomes (feature << 32 | global window) words on the device and is scattered to the buffer of its feature-hash
// range -- the ranges of mcq_build_parts, sub-ranges of this shard's range: foreign features are dropped --; finish() sorts
// every range (that is the merge of the reference's P per-rank lists of a feature into (target, window) order: each is
// already truncated to 254 per rank, src/sketch_database.h:1090-1092) and cuts it into keys / list lengths / words.
struct mcq_parts_builder {
    int device = 0; u32 nt = 0, n_ranges = 1, n_shards = 1, shard_id = 0;
    u32 k = 0, s = 0, winlen = 0, winstride = 0, tgt_winstride = 0;
    Dev<u32> tgt_windows;             // device [nt] (moves into the parts)
    Dev<u32> gw_off;                  // device [nt + 1]
    u64 n_windows = 0;
    std::vector<Dev<u64>> buf; std::vector<u64> cnt, cap;
    Dev<u64*> d_buf;                  // device copy of the buffer pointers
    Dev<unsigned long long> d_cur;    // device write cursors [n_ranges]
    Dev<u32> d_hist;                  // device [n_ranges + 1]: chunk histogram, [n_ranges] = bad triples
    Dev<u32> d_feat, d_tgt, d_win; u64 stage_cap = 0;
    u64 n_added = 0, n_kept = 0;
    u32 keep_first = 0, remove_above = 0;       // the query-time bucket rules (mcq_parts_builder_set_bucket_limit); both 0: off
    u64 n_shrunk = 0, n_removed = 0;            // ... buckets they shrank / removed so far
    Dev<char> limit_scratch; u64 limit_scratch_bytes = 0;     // ... and their scratch: there only once a rule is set, grows with the chunks
};
namespace {
__global__ void k_gwoff(const u32* tgt_windows, u32 nt, u32* gw_off) {       // (one thread: nt is at most a few 1e5)
    if (blockIdx.x || threadIdx.x) return;
    u64 acc = 0;
    for (u32 t = 0; t < nt; ++t) { gw_off[t] = (u32)acc; acc += tgt_windows[t]; }
    gw_off[nt] = (u32)acc;
}
// range of every triple of a chunk (0xFFFFFFFF: another shard's feature) and the chunk's histogram
__global__ void k_triple_range(const u32* feat, const u32* tgt, const u32* win, u64 n, u32 n_ranges, u32 n_shards, u32 shard_id,
                               const u32* tgt_windows, u32 nt, u32* rng, u32* hist) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u32 f = feat[i];
        const u32 r = (u32)(((u64)tmh_dev(f) * ((u64)n_ranges * n_shards)) >> 32);
        u32 mine = (r / n_ranges == shard_id) ? r - shard_id * n_ranges : 0xFFFFFFFFu;
        if (f == 0xFFFFFFFFu || tgt[i] >= nt || win[i] >= tgt_windows[tgt[i]]) { mine = 0xFFFFFFFFu; atomicAdd(&hist[n_ranges], 1u); }
        rng[i] = mine;
        if (mine != 0xFFFFFFFFu) atomicAdd(&hist[mine], 1u);
    }
}
__global__ void k_triple_scatter(const u32* feat, const u32* tgt, const u32* win, const u32* rng, u64 n, const u32* gw_off,
                                 u64* const* bufs, unsigned long long* cur) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u32 lane = threadIdx.x & 63;
    for (u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n; i0 += stride) {       // (whole waves iterate together)
        const u64 i = i0 + lane;
        const u32 r = i < n ? rng[i] : 0xFFFFFFFFu;
        unsigned long long todo = __ballot(r != 0xFFFFFFFFu);
        while (todo) {                                        // one atomic per distinct range among the wave's triples
            const u32 rr = __shfl(r, (int)__builtin_ctzll(todo), 64);
            const unsigned long long mm = __ballot(r == rr);
            unsigned long long base = 0;
            if (lane == (u32)__builtin_ctzll(mm)) base = atomicAdd(&cur[rr], (unsigned long long)__builtin_popcountll(mm));
            base = __shfl(base, (int)__builtin_ctzll(mm), 64);
            if (r == rr) bufs[rr][base + __builtin_popcountll(mm & ((1ull << lane) - 1))] = ((u64)feat[i] << 32) | (u64)(gw_off[tgt[i]] + win[i]);
            todo &= ~mm;
        }
    }
}
}  // namespace

extern "C" int mcq_parts_builder_free(mcq_parts_builder* b) {
    if (!b) return MCQ_OK;
    (void)hipSetDevice(b->device);
    delete b;
    return MCQ_OK;
}

extern "C" int mcq_parts_builder_create(const mcq_parts_builder_desc* d, mcq_parts_builder** out) {
    if (!d || !out || !d->tgt_windows || d->n_targets < 1) return bfail(MCQ_E_ARG, "null argument");
    const u32 n_shards = d->n_shards ? d->n_shards : 1;
    if (d->shard_id >= n_shards) return bfail(MCQ_E_ARG, "shard_id >= n_shards");
    BCHK(hipSetDevice(d->device));
    BuilderPtr b(new mcq_parts_builder());
    b->device = d->device; b->nt = d->n_targets; b->n_shards = n_shards; b->shard_id = d->shard_id;
    b->k = d->k; b->s = d->sketch_size; b->winlen = d->winlen; b->winstride = d->winstride; b->tgt_winstride = d->tgt_winstride;
    u64 total = 0;
    for (u32 t = 0; t < d->n_targets; ++t) total += d->tgt_windows[t];
    if (total >= 0xFFFFFFFFull) return bfail(MCQ_E_UNSUPPORTED, "2^32 - 1 windows or more");
    b->n_windows = total;
    BCHK(b->tgt_windows.alloc(d->n_targets));
    BCHK(hipMemcpy(b->tgt_windows.get(), d->tgt_windows, (u64)d->n_targets * 4, hipMemcpyHostToDevice));
    BCHK(b->gw_off.alloc((u64)d->n_targets + 1));
    hipLaunchKernelGGL(k_gwoff, dim3(1), dim3(1), 0, 0, (const u32*)b->tgt_windows.get(), d->n_targets, b->gw_off.get());
    // ranges: what the sort of one range needs at its peak (~30 B per location: the words twice, heads, key ids) against a
    // quarter of the free memory, from the caller's estimate of the locations this shard will receive
    size_t mem_free = 0, mem_total = 0;
    BCHK(hipMemGetInfo(&mem_free, &mem_total));
    const u64 expect = d->expected_locations / n_shards + 1;
    u32 n_ranges = (u32)std::max<u64>(1, (expect * 30 + mem_free / 4 - 1) / (mem_free / 4 ? mem_free / 4 : 1));
    if (d->n_ranges) n_ranges = d->n_ranges;
    if (const char* e = getenv("MCQ_BUILD_PARTS")) n_ranges = (u32)std::max<u64>(1, strtoull(e, nullptr, 10));      // (test hook, as mcq_build_parts)
    if ((u64)n_ranges * n_shards > (1u << 20)) return bfail(MCQ_E_UNSUPPORTED, "too many ranges");
    b->n_ranges = n_ranges;
    b->buf.resize(n_ranges); b->cnt.assign(n_ranges, 0); b->cap.assign(n_ranges, 0);
    BCHK(b->d_buf.alloc(n_ranges));
    BCHK(b->d_cur.alloc(n_ranges));
    BCHK(b->d_hist.alloc((u64)n_ranges + 1));
    BCHK(hipDeviceSynchronize());
    *out = b.release();
    return MCQ_OK;
}

extern "C" int mcq_parts_builder_add(mcq_parts_builder* b, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n, uint32_t flags) {
    if (!b || (n && (!feat || !tgt || !win))) return bfail(MCQ_E_ARG, "null argument");
    if (!n) return MCQ_OK;
    if (n >= (1ull << 31)) return bfail(MCQ_E_ARG, "a chunk holds fewer than 2^31 triples");
    BCHK(hipSetDevice(b->device));
    const u32 *df = feat, *dt = tgt, *dw = win;
    const bool limit = b->keep_first || b->remove_above;       // (the rules compact in place: a device chunk is copied to the stage first)
    if (!(flags & MCQ_DEVICE_PTRS) || limit) {
        const hipMemcpyKind kind = (flags & MCQ_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (n > b->stage_cap) {
            b->d_feat.reset(); b->d_tgt.reset(); b->d_win.reset(); b->stage_cap = 0;      // (all three go before the larger ones come)
            BCHK(b->d_feat.alloc(n)); BCHK(b->d_tgt.alloc(n)); BCHK(b->d_win.alloc(n));
            b->stage_cap = n;
        }
        df = b->d_feat.get(); dt = b->d_tgt.get(); dw = b->d_win.get();
        BCHK(hipMemcpyAsync(b->d_feat.get(), feat, n * 4, kind, 0));
        BCHK(hipMemcpyAsync(b->d_tgt.get(), tgt, n * 4, kind, 0));
        BCHK(hipMemcpyAsync(b->d_win.get(), win, n * 4, kind, 0));
    }
    const u64 n_given = n;
    if (limit) {                                                // every (feature, rank) bucket of the chunk, before anything else sees it
        const u64 need = mcq_bucket_limit_scratch_bytes(n);
        if (need > b->limit_scratch_bytes) {
            b->limit_scratch.reset(); b->limit_scratch_bytes = 0;
            BCHK(b->limit_scratch.alloc(need));
            b->limit_scratch_bytes = need;
        }
        uint64_t c[3] = {0, 0, 0};                              // kept, buckets shrunk, buckets removed
        if (mcq_bucket_limit_ws(b->d_feat.get(), b->d_tgt.get(), b->d_win.get(), n, b->keep_first, b->remove_above, b->device, nullptr,
                                b->limit_scratch.get(), b->limit_scratch_bytes, c) != MCQ_OK) return bfail(MCQ_E_HIP, std::string("mcq_bucket_limit_ws: ") + mcq_last_error());
        BCHK(hipStreamSynchronize(0));                          // (the counts arrive in stream order)
        if (c[0] > n) return bfail(MCQ_E_HIP, "mcq_bucket_limit_ws: more triples kept than given");
        b->n_shrunk += c[1]; b->n_removed += c[2];
        n = c[0];
        if (!n) { b->n_added += n_given; return MCQ_OK; }
    }
    Dev<u32> rng_buf;
    BCHK(rng_buf.alloc(n));
    u32* const rng = rng_buf.get();
    BCHK(hipMemsetAsync(b->d_hist.get(), 0, ((u64)b->n_ranges + 1) * 4, 0));
    hipLaunchKernelGGL(k_triple_range, grid_for(n), dim3(TB), 0, 0, df, dt, dw, n, b->n_ranges, b->n_shards, b->shard_id,
                       (const u32*)b->tgt_windows.get(), b->nt, rng, b->d_hist.get());
    std::vector<u32> hist(b->n_ranges + 1);
    BCHK(hipMemcpy(hist.data(), b->d_hist.get(), hist.size() * 4, hipMemcpyDeviceToHost));
    if (hist[b->n_ranges]) return bfail(MCQ_E_ARG, std::to_string(hist[b->n_ranges]) + " triples name a target or a window the database does not have");
    // room in every range's buffer (grown by half when it runs out: a copy of what is there)
    bool moved = false;
    for (u32 r = 0; r < b->n_ranges; ++r) {
        const u64 need = b->cnt[r] + hist[r];
        if (need <= b->cap[r]) continue;
        const u64 ncap = std::max<u64>(need + need / 2, 1u << 20);
        Dev<u64> nb;
        BCHK(nb.alloc(ncap));
        if (b->cnt[r]) BCHK(hipMemcpy(nb.get(), b->buf[r].get(), b->cnt[r] * 8, hipMemcpyDeviceToDevice));
        b->buf[r] = std::move(nb);                               // (frees the old one)
        b->cap[r] = ncap; moved = true;
    }
    if (moved) {
        std::vector<u64*> ptrs(b->n_ranges);
        for (u32 r = 0; r < b->n_ranges; ++r) ptrs[r] = b->buf[r].get();
        BCHK(hipMemcpy(b->d_buf.get(), ptrs.data(), (u64)b->n_ranges * 8, hipMemcpyHostToDevice));
    }
    BCHK(hipMemcpy(b->d_cur.get(), b->cnt.data(), (u64)b->n_ranges * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_triple_scatter, grid_for(n), dim3(TB), 0, 0, df, dt, dw, (const u32*)rng, n, (const u32*)b->gw_off.get(), (u64* const*)b->d_buf.get(), b->d_cur.get());
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    for (u32 r = 0; r < b->n_ranges; ++r) { b->cnt[r] += hist[r]; b->n_kept += hist[r]; }
    b->n_added += n_given;
    return MCQ_OK;
}

extern "C" int mcq_parts_builder_set_bucket_limit(mcq_parts_builder* b, uint32_t keep_first, uint32_t remove_above) {
    if (!b) return bfail(MCQ_E_ARG, "null argument");
    if (keep_first > 255) return bfail(MCQ_E_ARG, "keep_first must be in 0..255");
    b->keep_first = keep_first; b->remove_above = remove_above;
    return MCQ_OK;
}

extern "C" int mcq_parts_builder_bucket_counts(const mcq_parts_builder* b, uint64_t* n_shrunk, uint64_t* n_removed) {
    if (!b || !n_shrunk || !n_removed) return bfail(MCQ_E_ARG, "null argument");
    *n_shrunk = b->n_shrunk; *n_removed = b->n_removed;
    return MCQ_OK;
}

extern "C" int mcq_parts_builder_finish(mcq_parts_builder* b, mcq_parts** out) {
    if (!b || !out) return bfail(MCQ_E_ARG, "null argument");
    BCHK(hipSetDevice(b->device));
    Scratch tmpbuf;
    BCHK(tmpbuf.init(b->device));
    PhaseTrace phase;
    PartsPtr R(new mcq_parts());
    R->device = b->device; R->n_targets = b->nt; R->k = b->k; R->s = b->s; R->winlen = b->winlen; R->winstride = b->winstride;
    R->tgt_winstride = b->tgt_winstride;
    R->n_windows = b->n_windows; R->tgt_windows = std::move(b->tgt_windows);
    b->d_feat.reset(); b->d_tgt.reset(); b->d_win.reset(); b->stage_cap = 0;
    b->limit_scratch.reset(); b->limit_scratch_bytes = 0;
    for (u32 r = 0; r < b->n_ranges; ++r) {
        const u64 n = b->cnt[r];
        u64* fw = nullptr; u32* head = nullptr; u64* kid = nullptr; u64 n_keys = 0;
        if (n) {
            BCHK(tmpbuf.get(&fw, n * 8));
            size_t tmp = 0;
            BCHK(rocprim::radix_sort_keys(nullptr, tmp, b->buf[r].get(), fw, n, 0, 64));
            void* t = nullptr; BCHK(tmpbuf.get(&t, tmp ? tmp : 1));
            BCHK(rocprim::radix_sort_keys(t, tmp, b->buf[r].get(), fw, n, 0, 64));
            BCHK(hipDeviceSynchronize());
            tmpbuf.put(t);
            b->buf[r].reset(); b->cap[r] = 0;                    // (sorted into fw: the range's buffer goes before its part comes)
            BCHK(tmpbuf.get(&head, n * 4)); BCHK(tmpbuf.get(&kid, n * 8));
            hipLaunchKernelGGL(k_feat_heads, grid_for(n), dim3(TB), 0, 0, (const u64*)fw, n, head);
            MCHK(excl_scan(head, kid, n, &n_keys));
        }
        MCHK(emit_part(tmpbuf, *R, fw, head, kid, n, n_keys));   // (an empty range is a part of its own: no keys, one-element arrays)
        phase("  range sorted + emitted");
    }
    *out = R.release();
    mcq_parts_builder_free(b);
    return MCQ_OK;
}

// ---- a table extended by new sequences: `modify` (mcq_table_extend_* of include/mcq.h) ------------------------------------------
// What the database holds arrives as the triples of its shard files and becomes the pairs of the pipeline above, appended in
// the order given: a (feature, rank) group lies in one file, inside one key record, so it stays in the order of its bucket.
// finish() sketches the new sequences, makes their pairs with target ids and global windows that go on behind the old ones,
// puts them behind the old pairs and runs sort_truncate: the stable sort keeps the old entries of a group first, the cut at
// max_locs is the reference's bucket limit on an append (src/sketch_database.h:1090-1092).
struct mcq_table_extend {
    int device = 0; u32 k = 0, s = 0, winlen = 0, winstride = 0, P = 1, max_locs = 254, flags = 0;
    u32 n_old = 0; u64 n_old_win = 0;
    Dev<u32> tgt_windows;             // device [n_old]
    Dev<u64> win_off;                 // device [n_old + 1]: first global window of every old target
    PoolDev<u64> key; PoolDev<u32> val; u64 n = 0, cap = 0;     // the old pairs
    Dev<u32> d_feat, d_tgt, d_win; u64 stage_cap = 0;
    Dev<u32> d_bad;                   // triples of a chunk that name nothing the database has
};
typedef std::unique_ptr<mcq_table_extend, HandleFree<mcq_table_extend, mcq_table_extend_free>> ExtendPtr;
namespace {
__global__ void k_win_off(const u32* tgt_windows, u32 nt, u64* win_off) {      // (one thread, as k_gwoff)
    if (blockIdx.x || threadIdx.x) return;
    u64 acc = 0;
    for (u32 t = 0; t < nt; ++t) { win_off[t] = acc; acc += tgt_windows[t]; }
    win_off[nt] = acc;
}
// triple i of a chunk -> pair at + i (the caller has made room for the whole chunk)
__global__ void k_triple_pairs(const u32* feat, const u32* tgt, const u32* win, u64 n, const u32* tgt_windows, const u64* win_off, u32 nt, u32 P,
                               u64* key, u32* val, u32* bad) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u32 f = feat[i], t = tgt[i], w = win[i];
        if (f == 0xFFFFFFFFu || t >= nt || w >= tgt_windows[t]) { key[i] = ~0ull; val[i] = 0; atomicAdd(bad, 1u); continue; }
        key[i] = (u64)f * P + (t % P);
        val[i] = (u32)(win_off[t] + w);
    }
}
// k_make_pairs for sequences that go on behind others: win_off counts from the first new window, target ids from tgt_base,
// global windows from win_base (a kernel of its own: the from-scratch build keeps the one it has)
__global__ void k_make_pairs_after(const u32* feat, u64 n_slots, u32 s, const u64* win_off, u32 n_targets, u32 P, u32 tgt_base, u64 win_base,
                                   u64* key, u32* val) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const u32 f = feat[i];
        const u64 w = i / s;
        if (f == 0xFFFFFFFFu) { key[i] = ~0ull; val[i] = 0; continue; }
        const u32 t = tgt_base + target_of(win_off, n_targets, w);
        key[i] = (u64)f * P + (t % P);
        val[i] = (u32)(win_base + w);
    }
}
__global__ void k_shift_up(const u64* in, u64 n, u64 base, u64* out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + base;
}
}  // namespace

extern "C" int mcq_table_extend_free(mcq_table_extend* x) {
    if (!x) return MCQ_OK;
    (void)hipSetDevice(x->device);
    delete x;
    (void)hipStreamSynchronize(0);                              // (the pair buffer goes back to the pool in stream 0)
    return MCQ_OK;
}

extern "C" int mcq_table_extend_create(const mcq_table_extend_desc* d, mcq_table_extend** out) {
    if (!d || !out || (d->n_old_targets && !d->old_tgt_windows)) return bfail(MCQ_E_ARG, "null argument");
    if (d->flags & ~(uint32_t)MCQ_BUILD_REMOVE_OVERPOPULATED) return bfail(MCQ_E_ARG, "flags other than MCQ_BUILD_REMOVE_OVERPOPULATED");
    u64 total = 0;
    for (u32 t = 0; t < d->n_old_targets; ++t) total += d->old_tgt_windows[t];
    if (total >= (1ull << 32)) return bfail(MCQ_E_UNSUPPORTED, "more than 2^32 windows");
    if (d->expected_old_locations >= (1ull << 40)) return bfail(MCQ_E_UNSUPPORTED, "2^40 locations or more: the one-piece pipeline does not hold them");
    {   // the sketch parameters are refused here, before the database is read
        mcq_build_desc bd; std::memset(&bd, 0, sizeof(bd));
        bd.k = d->k; bd.sketch_size = d->sketch_size; bd.winlen = d->winlen; bd.winstride = d->winstride; bd.device = d->device;
        BCHK(hipSetDevice(d->device));
        if (!make_sketch_handle(&bd)) return MCQ_E_ARG;
    }
    ExtendPtr x(new mcq_table_extend());
    x->device = d->device; x->k = d->k; x->s = d->sketch_size; x->winlen = d->winlen; x->winstride = d->winstride;
    x->P = d->n_ranks ? d->n_ranks : 1; x->max_locs = d->max_locs ? d->max_locs : 254; x->flags = d->flags;
    x->n_old = d->n_old_targets; x->n_old_win = total;
    BCHK(x->tgt_windows.alloc(x->n_old)); BCHK(x->win_off.alloc((u64)x->n_old + 1)); BCHK(x->d_bad.alloc(1));
    if (x->n_old) BCHK(hipMemcpy(x->tgt_windows.get(), d->old_tgt_windows, (u64)x->n_old * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_win_off, dim3(1), dim3(1), 0, 0, (const u32*)x->tgt_windows.get(), x->n_old, x->win_off.get());
    x->cap = d->expected_old_locations;
    BCHK(x->key.alloc(x->cap)); BCHK(x->val.alloc(x->cap));
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    *out = x.release();
    return MCQ_OK;
}

extern "C" int mcq_table_extend_add(mcq_table_extend* x, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n, uint32_t flags) {
    if (!x || (n && (!feat || !tgt || !win))) return bfail(MCQ_E_ARG, "null argument");
    if (!n) return MCQ_OK;
    if (n >= (1ull << 31)) return bfail(MCQ_E_ARG, "a chunk holds fewer than 2^31 triples");
    BCHK(hipSetDevice(x->device));
    if (x->n + n > x->cap) {
        // more than the caller expected: room for this chunk and a sixteenth more, the pairs so far copied over
        const u64 ncap = x->n + n + std::max<u64>(x->cap / 16, 1u << 20);
        PoolDev<u64> nk; PoolDev<u32> nv;
        BCHK(nk.alloc(ncap)); BCHK(nv.alloc(ncap));
        if (x->n) {
            BCHK(hipMemcpyAsync(nk.get(), x->key.get(), x->n * 8, hipMemcpyDeviceToDevice, 0));
            BCHK(hipMemcpyAsync(nv.get(), x->val.get(), x->n * 4, hipMemcpyDeviceToDevice, 0));
        }
        x->key = std::move(nk); x->val = std::move(nv);           // (gives the old ones back, behind the copies in stream 0)
        x->cap = ncap;
    }
    const u32 *df = feat, *dt = tgt, *dw = win;
    if (!(flags & MCQ_DEVICE_PTRS)) {
        if (n > x->stage_cap) {
            x->d_feat.reset(); x->d_tgt.reset(); x->d_win.reset(); x->stage_cap = 0;      // (all three go before the larger ones come)
            BCHK(x->d_feat.alloc(n)); BCHK(x->d_tgt.alloc(n)); BCHK(x->d_win.alloc(n));
            x->stage_cap = n;
        }
        df = x->d_feat.get(); dt = x->d_tgt.get(); dw = x->d_win.get();
        BCHK(hipMemcpyAsync(x->d_feat.get(), feat, n * 4, hipMemcpyHostToDevice, 0));
        BCHK(hipMemcpyAsync(x->d_tgt.get(), tgt, n * 4, hipMemcpyHostToDevice, 0));
        BCHK(hipMemcpyAsync(x->d_win.get(), win, n * 4, hipMemcpyHostToDevice, 0));
    }
    BCHK(hipMemsetAsync(x->d_bad.get(), 0, 4, 0));
    hipLaunchKernelGGL(k_triple_pairs, grid_for(n), dim3(TB), 0, 0, df, dt, dw, n, (const u32*)x->tgt_windows.get(), (const u64*)x->win_off.get(),
                       x->n_old, x->P, x->key.get() + x->n, x->val.get() + x->n, x->d_bad.get());
    u32 bad = 0;
    BCHK(hipMemcpy(&bad, x->d_bad.get(), 4, hipMemcpyDeviceToHost));      // (waits for the kernel: the caller's buffers are free again)
    BCHK(hipGetLastError());
    if (bad) return bfail(MCQ_E_ARG, std::to_string(bad) + " triples name a target or a window the database does not have");
    x->n += n;
    return MCQ_OK;
}

extern "C" int mcq_table_extend_finish(mcq_table_extend* x, const char* bases, const uint64_t* seq_off, uint32_t n_new_targets, uint32_t flags,
                                       mcq_table** out) {
    if (!x || !out || (n_new_targets && (!seq_off || !bases))) return bfail(MCQ_E_ARG, "null argument");
    const u32 nn = n_new_targets;
    if ((u64)x->n_old + nn >= 0xFFFFFFFFull) return bfail(MCQ_E_UNSUPPORTED, "more targets than a 32-bit target id holds");
    BCHK(hipSetDevice(x->device));
    Scratch tmpbuf;
    BCHK(tmpbuf.init(x->device));
    PhaseTrace phase;
    x->d_feat.reset(); x->d_tgt.reset(); x->d_win.reset(); x->stage_cap = 0;
    const u32 nt = x->n_old + nn, s = x->s;

    TablePtr T(new mcq_table());
    T->device = x->device; T->n_targets = nt;
    BCHK(T->win_off.alloc((u64)nt + 1));
    u64* const win_off = T->win_off.get();
    BCHK(hipMemcpy(win_off, x->win_off.get(), ((u64)x->n_old + 1) * 8, hipMemcpyDeviceToDevice));

    // the new sequences: windows and sketches, counted from their own first window
    u64 n_new_win = 0;
    u32* feat = nullptr; u64* new_off = nullptr;
    char* t_bases = nullptr; u64* t_off = nullptr;
    if (nn) {
        if (!(flags & MCQ_DEVICE_PTRS)) {
            const u64 nb = seq_off[nn];
            BCHK(tmpbuf.get(&t_bases, nb ? nb : 1)); BCHK(tmpbuf.get(&t_off, (u64)(nn + 1) * 8));
            if (nb) BCHK(hipMemcpy(t_bases, bases, nb, hipMemcpyHostToDevice));
            BCHK(hipMemcpy(t_off, seq_off, (u64)(nn + 1) * 8, hipMemcpyHostToDevice));
            bases = t_bases; seq_off = t_off;
        }
        mcq_build_desc bd; std::memset(&bd, 0, sizeof(bd));
        bd.k = x->k; bd.sketch_size = s; bd.winlen = x->winlen; bd.winstride = x->winstride; bd.device = x->device;
        DbPtr sk = make_sketch_handle(&bd);
        if (!sk) return MCQ_E_ARG;
        BCHK(tmpbuf.get(&new_off, (u64)(nn + 1) * 8));
        mcq_batch b; b.n_seqs = nn; b.bases = bases; b.seq_off = seq_off; b.paired = 0; b.flags = MCQ_DEVICE_PTRS; b.n_bases = 0;
        MCHK(mcq_count_windows(sk.get(), &b, new_off, nullptr));
        BCHK(hipMemcpy(&n_new_win, new_off + nn, 8, hipMemcpyDeviceToHost));
        if (x->n_old_win + n_new_win >= (1ull << 32)) return bfail(MCQ_E_UNSUPPORTED, "more than 2^32 windows");
        u32* nfeat = nullptr;
        BCHK(tmpbuf.get(&feat, std::max<u64>(1, n_new_win * s) * 4)); BCHK(tmpbuf.get(&nfeat, std::max<u64>(1, n_new_win) * 4));
        MCHK(mcq_sketch(sk.get(), &b, new_off, feat, nfeat, nullptr));
        hipLaunchKernelGGL(k_shift_up, dim3((nn + 1 + TB - 1) / TB), dim3(TB), 0, 0, (const u64*)new_off, (u64)nn + 1, x->n_old_win, win_off + x->n_old);
        BCHK(hipDeviceSynchronize());
        tmpbuf.put(nfeat);
    }
    phase("windows + sketches (new)");

    // old pairs, then the new ones, in one buffer of the pipeline's own kind
    const u64 n_new = n_new_win * s, n = x->n + n_new;
    u64* key = nullptr; u32* val = nullptr;
    BCHK(tmpbuf.get(&key, (n ? n : 1) * 8)); BCHK(tmpbuf.get(&val, (n ? n : 1) * 4));
    if (x->n) {
        BCHK(hipMemcpyAsync(key, x->key.get(), x->n * 8, hipMemcpyDeviceToDevice, 0));
        BCHK(hipMemcpyAsync(val, x->val.get(), x->n * 4, hipMemcpyDeviceToDevice, 0));
    }
    if (n_new) hipLaunchKernelGGL(k_make_pairs_after, grid_for(n_new), dim3(TB), 0, 0, (const u32*)feat, n_new, s, (const u64*)new_off, nn, x->P,
                                  x->n_old, x->n_old_win, key + x->n, val + x->n);
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    x->key.reset(); x->val.reset(); x->cap = 0; x->n = 0;        // (the pipeline owns the pairs from here on: an error below ends the extension)
    if (feat) tmpbuf.put(feat);
    if (new_off) tmpbuf.put(new_off);
    if (t_bases) tmpbuf.put(t_bases);
    if (t_off) tmpbuf.put(t_off);
    phase("pairs (old + new)");
    Lists L;
    MCHK(sort_truncate(tmpbuf, key, val, n, x->P, x->max_locs, (x->flags & MCQ_BUILD_REMOVE_OVERPOPULATED) != 0, L, phase));
    // keys, offsets, (target, window) locations over all targets (as mcq_build_table ends, whose text stays what it was)
    T->n_keys = L.n_keys; T->n_locs = L.n_kept;
    BCHK(T->keys.alloc(L.n_keys)); BCHK(T->list_off.alloc(L.n_keys + 1));
    BCHK(T->locs.alloc(L.n_kept));
    if (L.n_kept) hipLaunchKernelGGL(k_emit, grid_for(L.n_kept), dim3(TB), 0, 0, L.fw, L.head, L.kid, L.n_kept, L.n_keys, win_off, nt, T->keys.get(), T->list_off.get(), T->locs.get());
    else BCHK(hipMemset(T->list_off.get(), 0, 8));
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    tmpbuf.put(L.fw); tmpbuf.put(L.head); tmpbuf.put(L.kid);
    phase("emit keys / offsets / locations");
    *out = T.release();
    mcq_table_extend_free(x);
    return MCQ_OK;
}

extern "C" int mcq_db_from_parts(const mcq_parts* p, const uint32_t* tgt2tax, uint32_t n_shards, uint32_t shard_id, uint32_t flags, mcq_db** out) {
    if (!p || !tgt2tax || !out) return bfail(MCQ_E_ARG, "null argument");
    BCHK(hipSetDevice(p->device));
    Dev<u32> t2t;
    if (!(flags & MCQ_DEVICE_PTRS)) {
        BCHK(t2t.alloc(p->n_targets));
        BCHK(hipMemcpy(t2t.get(), tgt2tax, (u64)p->n_targets * 4, hipMemcpyHostToDevice));
    }
    mcq_db_desc c; std::memset(&c, 0, sizeof(c));
    c.k = p->k; c.sketch_size = p->s; c.winlen = p->winlen; c.winstride = p->winstride; c.tgt_winstride = p->tgt_winstride ? p->tgt_winstride : p->winstride;
    c.n_targets = p->n_targets; c.tgt2tax = t2t.get() ? t2t.get() : tgt2tax; c.tgt_windows = p->tgt_windows.get();
    c.n_shards = n_shards ? n_shards : 1; c.shard_id = shard_id; c.device = p->device;
    c.flags = MCQ_DEVICE_PTRS | (flags & (MCQ_DB_SLOTS_16 | MCQ_DB_BUCKETS_64));
    const int rc = mcq_db_create_parts(&c, p->parts.data(), (u32)p->parts.size(), out);
    if (rc != MCQ_OK) g_berr = mcq_last_error();
    return rc;
}

extern "C" int mcq_db_build(const mcq_build_desc* d, mcq_db** out) {
    if (!d || !out) return bfail(MCQ_E_ARG, "null argument");
    // in parts when the one-piece temporaries (~60 B per feature slot of the sequences) would not leave room for the table --
    // or when asked to (MCQ_BUILD_PARTS: test hook); needs the sequences in device memory.
    // The two routes must not give different location WORDS for the same data when the words travel (a sharded table: the home
    // rank decodes what the owners send with its own tables): with n_shards > 1 the route is chosen by the size of the data alone
    // (not by what this rank happens to have free), and both routes give the global-window form over the true window counts of
    // the targets.  (A one-rank table keeps the faster bit fields where they fit, and the memory-driven choice.)
    const bool sharded = d->n_shards > 1;
    if ((d->flags & MCQ_DEVICE_PTRS) && !(d->flags & MCQ_DB_LOCS_64) && d->seq_off && d->n_targets) {
        bool in_parts = getenv("MCQ_BUILD_PARTS") != nullptr;
        if (!in_parts) {
            u64 ends[1] = {0};
            BCHK(hipSetDevice(d->device));
            BCHK(hipMemcpy(ends, d->seq_off + d->n_targets, 8, hipMemcpyDeviceToHost));
            const u64 slots = ends[0] / (d->winstride ? d->winstride : 1) * d->sketch_size;
            if (sharded) in_parts = slots * 60 > (96ull << 30);
            else {
                size_t mem_free = 0, mem_total = 0;
                BCHK(hipMemGetInfo(&mem_free, &mem_total));
                in_parts = slots * 60 > mem_free / 2;
            }
        }
        if (in_parts) {
            mcq_parts* built = nullptr;
            MCHK(mcq_build_parts(d, &built));
            PartsPtr parts(built);
            return mcq_db_from_parts(parts.get(), d->tgt2tax, d->n_shards, d->shard_id, d->flags & (MCQ_DEVICE_PTRS | MCQ_DB_SLOTS_16 | MCQ_DB_BUCKETS_64), out);
        }
    }
    mcq_table* built = nullptr;
    MCHK(mcq_build_table(d, &built));
    TablePtr T(built);
    Dev<u32> t2t, tw;
    BCHK(t2t.alloc(d->n_targets));
    BCHK(hipMemcpy(t2t.get(), d->tgt2tax, (u64)d->n_targets * 4, (d->flags & MCQ_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    mcq_db_desc c; std::memset(&c, 0, sizeof(c));
    c.k = d->k; c.sketch_size = d->sketch_size; c.winlen = d->winlen; c.winstride = d->winstride; c.tgt_winstride = d->winstride;
    c.n_targets = d->n_targets; c.n_keys = T->n_keys; c.n_locs = T->n_locs;
    c.keys = T->keys.get(); c.list_off = T->list_off.get(); c.locs = T->locs.get(); c.tgt2tax = t2t.get();
    c.n_shards = d->n_shards ? d->n_shards : 1; c.shard_id = d->shard_id; c.flags = MCQ_DEVICE_PTRS | (d->flags & (MCQ_DB_LOCS_64 | MCQ_DB_LOCS_GW | MCQ_DB_SLOTS_16 | MCQ_DB_BUCKETS_64)); c.device = d->device;
    // the true window counts of the targets (what the parts route defines its words by), and for a sharded table that form
    BCHK(tw.alloc(d->n_targets));
    hipLaunchKernelGGL(k_windows_of, dim3((d->n_targets + TB - 1) / TB), dim3(TB), 0, 0, (const u64*)T->win_off.get(), d->n_targets, tw.get());
    c.tgt_windows = tw.get();
    if (sharded && !(d->flags & MCQ_DB_LOCS_64)) c.flags |= MCQ_DB_LOCS_GW;
    const int rc = mcq_db_create(&c, out);
    if (rc != MCQ_OK) g_berr = mcq_last_error();
    return rc;                                                   // (tw, t2t and the table go in that order, as they always did)
}

// ---- one reference rank's table out of the union table (mcq_table_rank_split of include/mcq.h) ----------------------------------
// The reference's rank r holds the targets with tgt % P == r (src/sketch_database.h:540-542), so its table is the union table with
// every other target's locations taken out and the keys that lose their whole list dropped.  The per-(feature, rank) limit and
// -remove-overpopulated-features were applied when the union was built.  Count per key, two scans, scatter: lists keep their
// (target, window) order, keys their order, nothing is written through an atomic.
// A group of 16 lanes works on one key (lists are short: a few locations on average, at most 254 x P), four keys per wave; a group
// reads 16 consecutive locations per step.  All loops are uniform over the wave (the ballots need every lane): the trip count is
// the longest of the wave's four lists.
namespace {
const u32 SPLIT_GROUP = 16;
struct SplitKey { u64 kx, beg; u32 len, steps; };
// key of this lane's group in the wave's round `base` and the wave-uniform number of 16-location steps
__device__ __forceinline__ SplitKey split_key(const u64* list_off, u64 n_keys, u64 base, u32 lane) {
    SplitKey s; s.kx = base + lane / SPLIT_GROUP; s.beg = 0; s.len = 0;
    if (s.kx < n_keys) { s.beg = list_off[s.kx]; s.len = (u32)(list_off[s.kx + 1] - s.beg); }
    u32 m = s.len;
    m = max(m, (u32)__shfl_xor((int)m, 16, 64));
    m = max(m, (u32)__shfl_xor((int)m, 32, 64));
    s.steps = (m + SPLIT_GROUP - 1) / SPLIT_GROUP;
    return s;
}
__global__ void __launch_bounds__(256) k_split_count(const u64* list_off, const u64* locs, u64 n_keys, u32 P, u32 rank, u32* cnt, u32* alive) {
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP, shift = lane - sub;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const SplitKey s = split_key(list_off, n_keys, base, lane);
        u32 n = 0;
        for (u32 i = 0; i < s.steps; ++i) {
            const u32 j = i * SPLIT_GROUP + sub;
            const bool mine = j < s.len && (u32)(locs[s.beg + j] >> 32) % P == rank;
            n += (u32)__builtin_popcountll((__ballot(mine) >> shift) & 0xFFFFull);
        }
        if (sub == 0 && s.kx < n_keys) { cnt[s.kx] = n; alive[s.kx] = n ? 1u : 0u; }
    }
}
__global__ void __launch_bounds__(256) k_split_scatter(const u32* keys, const u64* list_off, const u64* locs, u64 n_keys, u32 P, u32 rank,
                                                      const u32* alive, const u64* key_pos, const u64* loc_pos, u64 n_keys_out, u64 n_locs_out,
                                                      u32* okeys, u64* ooff, u64* olocs) {
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP, shift = lane - sub;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) ooff[n_keys_out] = n_locs_out;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const SplitKey s = split_key(list_off, n_keys, base, lane);
        const bool live = s.kx < n_keys && alive[s.kx];
        const u64 out = live ? loc_pos[s.kx] : 0;
        if (live && sub == 0) { const u64 ko = key_pos[s.kx]; if (ko < n_keys_out) { okeys[ko] = keys[s.kx]; ooff[ko] = out; } }
        u32 done = 0;
        for (u32 i = 0; i < s.steps; ++i) {
            const u32 j = i * SPLIT_GROUP + sub;
            u64 w = 0;
            bool mine = false;
            if (live && j < s.len) { w = locs[s.beg + j]; mine = (u32)(w >> 32) % P == rank; }
            const u32 bits = (u32)((__ballot(mine) >> shift) & 0xFFFFull);
            const u64 o = out + done + (u32)__builtin_popcount(bits & ((1u << sub) - 1u));
            if (mine && o < n_locs_out) olocs[o] = w;
            done += (u32)__builtin_popcount(bits);
        }
    }
}
}  // namespace

// ---- what the two filters of a table share (this one and -remove-ambig-features below) ----
// *out = t without some of its locations and without the keys that lose their whole list; win_off is t's.  count(grid, cnt, alive)
// enqueues the kernel that writes what every key keeps (cnt[key] locations, alive[key] = 0 / 1), scatter(grid, alive, key_pos,
// loc_pos, n_keys_out, n_locs_out, keys, list_off, locs) the one that writes the output from the two scans; neither is called
// for a table without keys.
template <class Count, class Scatter>
static int filter_table(const mcq_table* t, Count count, Scatter scatter, mcq_table** out, uint64_t* n_kept_keys) {
    const u64 nk = t->n_keys;
    TablePtr R(new mcq_table());
    R->device = t->device; R->n_targets = t->n_targets;
    BCHK(R->win_off.alloc((u64)t->n_targets + 1));
    BCHK(hipMemcpy(R->win_off.get(), t->win_off.get(), ((u64)t->n_targets + 1) * 8, hipMemcpyDeviceToDevice));
    Dev<u32> cnt, alive; Dev<u64> key_pos, loc_pos;
    BCHK(cnt.alloc(nk)); BCHK(alive.alloc(nk)); BCHK(key_pos.alloc(nk)); BCHK(loc_pos.alloc(nk));
    const dim3 grid = grid_for((nk + 3) / 4 * 64);               // four keys per wave of 64 lanes
    u64 n_keys_out = 0, n_locs_out = 0;
    if (nk) count(grid, cnt.get(), alive.get());
    MCHK(excl_scan(cnt.get(), loc_pos.get(), nk, &n_locs_out));
    MCHK(excl_scan(alive.get(), key_pos.get(), nk, &n_keys_out));
    R->n_keys = n_keys_out; R->n_locs = n_locs_out;
    BCHK(R->keys.alloc(n_keys_out)); BCHK(R->list_off.alloc(n_keys_out + 1)); BCHK(R->locs.alloc(n_locs_out));
    if (nk) scatter(grid, (const u32*)alive.get(), (const u64*)key_pos.get(), (const u64*)loc_pos.get(), n_keys_out, n_locs_out,
                    R->keys.get(), R->list_off.get(), R->locs.get());
    else BCHK(hipMemset(R->list_off.get(), 0, 8));
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    *n_kept_keys = n_keys_out;
    *out = R.release();
    return MCQ_OK;
}

extern "C" int mcq_table_rank_split(const mcq_table* t, uint32_t n_ranks, uint32_t rank, mcq_table** out) {
    if (!t || !out) return bfail(MCQ_E_ARG, "null argument");
    if (n_ranks < 1 || rank >= n_ranks) return bfail(MCQ_E_ARG, "rank >= n_ranks");
    BCHK(hipSetDevice(t->device));
    const u64 nk = t->n_keys;
    const u32* keys = t->keys.get(); const u64 *list_off = t->list_off.get(), *locs = t->locs.get();
    u64 n_kept = 0;
    return filter_table(t,
        [&](dim3 grid, u32* cnt, u32* alive) {
            hipLaunchKernelGGL(k_split_count, grid, dim3(TB), 0, 0, list_off, locs, nk, n_ranks, rank, cnt, alive);
        },
        [&](dim3 grid, const u32* alive, const u64* key_pos, const u64* loc_pos, u64 n_keys_out, u64 n_locs_out, u32* okeys, u64* ooff, u64* olocs) {
            hipLaunchKernelGGL(k_split_scatter, grid, dim3(TB), 0, 0, keys, list_off, locs, nk, n_ranks, rank, alive, key_pos, loc_pos,
                               n_keys_out, n_locs_out, okeys, ooff, olocs);
        }, out, &n_kept);
}

// ---- one rank's key records as the bytes of its shard file (mcq_table_shard_records of include/mcq.h) --------------------------------
// The rank split above, ending in file bytes instead of a table: for every key with at least one location of the rank, in key
// order, `u32 key, u8 n, u64 n, u32 tgt[n], u64 n, u32 win[n]` -- 21 + 8 n bytes, little-endian, nothing aligned (what
// mcq_refdb_write_shard of the host library writes per key; hash_multimap::serialize, src/hash_multimap.h).  Same traversal: a group of
// 16 lanes per key, four keys per wave, trip counts uniform over the wave.  The count pass leaves n and the bytes of every key (0 or
// 21 + 8 n) and raises a flag word for a list that an 8-bit count does not hold; a 64-bit scan of the bytes gives every record its
// place; the emit pass writes the record's fixed fields from the group's first lane and the two columns at ballot-prefix positions.
// No atomics.  Every field is written byte by byte: the target column starts at byte 13 of a record and the window column at
// 21 + 4 n, records follow each other without padding, so no field has an alignment to rely on -- and the disk, not this kernel,
// bounds the phase.
namespace {
__device__ __forceinline__ void put_le(unsigned char* p, u64 v, u32 n_bytes) {
    for (u32 i = 0; i < n_bytes; ++i) p[i] = (unsigned char)(v >> (8 * i));
}
__global__ void __launch_bounds__(256) k_rec_count(const u64* list_off, const u64* locs, u64 n_keys, u32 P, u32 rank, u32* cnt, u32* bytes, u32* too_long) {
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP, shift = lane - sub;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const SplitKey s = split_key(list_off, n_keys, base, lane);
        u32 n = 0;
        for (u32 i = 0; i < s.steps; ++i) {
            const u32 j = i * SPLIT_GROUP + sub;
            const bool mine = j < s.len && (u32)(locs[s.beg + j] >> 32) % P == rank;
            n += (u32)__builtin_popcountll((__ballot(mine) >> shift) & 0xFFFFull);
        }
        if (sub == 0 && s.kx < n_keys) {
            cnt[s.kx] = n; bytes[s.kx] = n ? 21u + 8u * n : 0u;
            if (n > 255u) *too_long = 1u;                        // (every writer stores the same word)
        }
    }
}
__global__ void __launch_bounds__(256) k_rec_emit(const u32* keys, const u64* list_off, const u64* locs, u64 n_keys, u32 P, u32 rank,
                                                 const u32* cnt, const u64* byte_pos, u64 n_bytes, unsigned char* out) {
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP, shift = lane - sub;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const SplitKey s = split_key(list_off, n_keys, base, lane);
        const u32 n = s.kx < n_keys ? cnt[s.kx] : 0u;
        const u64 at = n ? byte_pos[s.kx] : 0;
        const bool live = n && at + 21 + 8ull * n <= n_bytes;   // (the whole record lies inside the buffer, or nothing of it is written)
        unsigned char* const rec = out + at;
        if (live && sub == 0) {
            put_le(rec, keys[s.kx], 4); put_le(rec + 4, n, 1); put_le(rec + 5, n, 8);
            put_le(rec + 13 + 4ull * n, n, 8);
        }
        u32 done = 0;
        for (u32 i = 0; i < s.steps; ++i) {
            const u32 j = i * SPLIT_GROUP + sub;
            u64 w = 0;
            bool mine = false;
            if (live && j < s.len) { w = locs[s.beg + j]; mine = (u32)(w >> 32) % P == rank; }
            const u32 bits = (u32)((__ballot(mine) >> shift) & 0xFFFFull);
            const u32 o = done + (u32)__builtin_popcount(bits & ((1u << sub) - 1u));
            if (mine && o < n) { put_le(rec + 13 + 4ull * o, w >> 32, 4); put_le(rec + 21 + 4ull * n + 4ull * o, w & 0xFFFFFFFFull, 4); }
            done += (u32)__builtin_popcount(bits);
        }
    }
}
}  // namespace

extern "C" int mcq_table_shard_records(const mcq_table* t, uint32_t n_ranks, uint32_t rank, void* out, uint64_t cap_bytes,
                                       uint64_t* n_bytes, uint64_t* n_keys, uint64_t* n_locs) {
    if (!t || !n_bytes || !n_keys || !n_locs) return bfail(MCQ_E_ARG, "null argument");
    if (n_ranks < 1 || rank >= n_ranks) return bfail(MCQ_E_ARG, "rank >= n_ranks");
    *n_bytes = *n_keys = *n_locs = 0;
    const u64 nk = t->n_keys;
    if (!nk) return MCQ_OK;
    BCHK(hipSetDevice(t->device));
    Dev<u32> cnt, bytes, too_long; Dev<u64> byte_pos, loc_pos;
    BCHK(cnt.alloc(nk)); BCHK(bytes.alloc(nk)); BCHK(too_long.alloc(1)); BCHK(byte_pos.alloc(nk)); BCHK(loc_pos.alloc(nk));
    BCHK(hipMemset(too_long.get(), 0, 4));
    const dim3 grid = grid_for((nk + 3) / 4 * 64);               // four keys per wave of 64 lanes
    hipLaunchKernelGGL(k_rec_count, grid, dim3(TB), 0, 0, (const u64*)t->list_off.get(), (const u64*)t->locs.get(), nk, n_ranks, rank,
                       cnt.get(), bytes.get(), too_long.get());
    u64 total_bytes = 0, total_locs = 0;
    MCHK(excl_scan(bytes.get(), byte_pos.get(), nk, &total_bytes));
    MCHK(excl_scan(cnt.get(), loc_pos.get(), nk, &total_locs));       // (for its total)
    loc_pos.reset();
    u32 flagged = 0;
    BCHK(hipMemcpy(&flagged, too_long.get(), 4, hipMemcpyDeviceToHost));
    BCHK(hipGetLastError());
    if (flagged) return bfail(MCQ_E_UNSUPPORTED, "a list has more than 255 locations of the rank (bucket size type is uint8, src/config.h:77)");
    *n_bytes = total_bytes; *n_locs = total_locs; *n_keys = (total_bytes - 8 * total_locs) / 21;
    if (!out) return MCQ_OK;
    if (cap_bytes < total_bytes) return bfail(MCQ_E_CAPACITY, "the buffer holds " + std::to_string(cap_bytes) + " bytes, the records need " + std::to_string(total_bytes));
    if (total_bytes) hipLaunchKernelGGL(k_rec_emit, grid, dim3(TB), 0, 0, (const u32*)t->keys.get(), (const u64*)t->list_off.get(), (const u64*)t->locs.get(), nk,
                                        n_ranks, rank, (const u32*)cnt.get(), (const u64*)byte_pos.get(), total_bytes, (unsigned char*)out);
    BCHK(hipDeviceSynchronize());
    BCHK(hipGetLastError());
    return MCQ_OK;
}

// ---- -remove-ambig-features: keys whose list names more than max_keys distinct clades (mcq_table_remove_ambiguous of include/mcq.h) ----
// remove_ambiguous_features (src/sketch_database.h:428-470) over the union table: a feature goes when the targets of its list have more
// than max_keys distinct values of tgt_key[target] (the target's ancestor at the rank, "none" being one value; the target itself for
// rank sequence).  Same traversal as the rank split above: a group of 16 lanes per key, four keys per wave, 16 consecutive locations
// per step, trip counts uniform over the wave; a count pass (alive, surviving length = the whole list or nothing), the two scans, a
// scatter pass that copies the lists of the keys that stay.  No atomics, nothing comes back to the host per key.
//   max_keys = 1 (the default): a list is ambiguous as soon as one key differs from that of its first location -- one ballot per step.
//   max_keys > 1: the group keeps the distinct keys it has seen in LDS, max_keys + 1 words per group (at most 256: 16 KB per block of
//   16 groups).  A list is sorted by (target, window), so the locations of one target are a run: only the first location of a run is
//   a candidate (equal keys of DIFFERENT targets are not adjacent and are found by the set).  A candidate scans the set; candidates
//   that are not in it are made unique among the 16 lanes by shuffles (only in steps where some group of the wave has two of them),
//   then appended at ballot-prefix positions.  The count saturates at max_keys + 1, where the group stops looking.
namespace {
__device__ __forceinline__ u32 ambig_key(const u32* tgt_key, u32 n_targets, u64 loc) {
    const u32 t = (u32)(loc >> 32);
    return t < n_targets ? tgt_key[t] : 0u;
}
template <bool ONE>
__global__ void __launch_bounds__(256) k_ambig_count(const u64* list_off, const u64* locs, u64 n_keys, const u32* tgt_key, u32 n_targets,
                                                    u32 max_keys, u32* cnt, u32* alive) {
    extern __shared__ u32 s_seen[];                              // [blockDim.x / 16][max_keys + 1]; not used by ONE
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP, shift = lane - sub;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    const u32 cap = max_keys + 1;
    u32* seen = s_seen + (threadIdx.x / SPLIT_GROUP) * cap;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const SplitKey s = split_key(list_off, n_keys, base, lane);
        bool ambiguous = false;
        if (ONE) {
            u32 first = 0;
            for (u32 i = 0; i < s.steps; ++i) {
                const u32 j = i * SPLIT_GROUP + sub;
                const bool valid = j < s.len;
                const u32 k = valid ? ambig_key(tgt_key, n_targets, locs[s.beg + j]) : 0u;
                if (i == 0) first = (u32)__shfl((int)k, (int)shift, 64);
                ambiguous |= ((__ballot(valid && k != first) >> shift) & 0xFFFFull) != 0;
                if (!__ballot(!ambiguous && (i + 1) * SPLIT_GROUP < s.len)) break;       // (uniform) no group of the wave has anything left to learn
            }
        } else {
            u32 n = 0, last_t = 0xFFFFFFFFu;                     // distinct keys so far; target of the location before this step's first
            for (u32 i = 0; i < s.steps; ++i) {
                const u32 j = i * SPLIT_GROUP + sub;
                const bool valid = j < s.len;
                const u64 w = valid ? locs[s.beg + j] : 0;
                const u32 t = (u32)(w >> 32);
                const u32 k = valid ? ambig_key(tgt_key, n_targets, w) : 0u;
                const u32 before = (u32)__shfl((int)t, (int)((lane + 63) & 63), 64);
                bool cand = valid && n < cap && t != (sub ? before : last_t);
                last_t = (u32)__shfl((int)t, (int)(shift + SPLIT_GROUP - 1), 64);
                if (cand) for (u32 q = 0; q < n; ++q) if (seen[q] == k) { cand = false; break; }
                bool fresh = cand;
                const u32 bits = (u32)((__ballot(cand) >> shift) & 0xFFFFull);
                if (__ballot((bits & (bits - 1)) != 0)) {        // some group has two candidates: the lowest lane of every key stays
                    for (u32 d = 1; d < SPLIT_GROUP; ++d) {
                        const u32 ko = (u32)__shfl((int)k, (int)((lane + 64 - d) & 63), 64);
                        const int co = __shfl((int)cand, (int)((lane + 64 - d) & 63), 64);
                        if (sub >= d && co && ko == k) fresh = false;
                    }
                }
                const u32 add = (u32)((__ballot(fresh) >> shift) & 0xFFFFull);
                const u32 at = n + (u32)__builtin_popcount(add & ((1u << sub) - 1u));
                if (fresh && at < cap) seen[at] = k;
                n = min(n + (u32)__builtin_popcount(add), cap);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the group's next step reads what this one wrote
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (!__ballot(n < cap && (i + 1) * SPLIT_GROUP < s.len)) break;
            }
            ambiguous = n > max_keys;
        }
        if (sub == 0 && s.kx < n_keys) { const bool stays = s.len && !ambiguous; cnt[s.kx] = stays ? s.len : 0u; alive[s.kx] = stays ? 1u : 0u; }
    }
}
__global__ void __launch_bounds__(256) k_ambig_scatter(const u32* keys, const u64* list_off, const u64* locs, u64 n_keys, const u32* alive,
                                                      const u64* key_pos, const u64* loc_pos, u64 n_keys_out, u64 n_locs_out,
                                                      u32* okeys, u64* ooff, u64* olocs) {
    const u32 lane = threadIdx.x & 63, sub = lane % SPLIT_GROUP;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) ooff[n_keys_out] = n_locs_out;
    for (u64 base = wave * 4; base < n_keys; base += n_waves * 4) {
        const u64 kx = base + lane / SPLIT_GROUP;
        if (kx >= n_keys || !alive[kx]) continue;
        const u64 beg = list_off[kx], out = loc_pos[kx];
        const u32 len = (u32)(list_off[kx + 1] - beg);
        if (sub == 0) { const u64 ko = key_pos[kx]; if (ko < n_keys_out) { okeys[ko] = keys[kx]; ooff[ko] = out; } }
        for (u32 j = sub; j < len; j += SPLIT_GROUP) if (out + j < n_locs_out) olocs[out + j] = locs[beg + j];
    }
}
}  // namespace

extern "C" int mcq_table_remove_ambiguous(const mcq_table* t, const uint32_t* tgt_key, uint32_t n_targets, uint32_t max_keys, uint32_t flags,
                                          mcq_table** out, uint64_t* n_removed) {
    if (!t || !tgt_key || !out || !n_removed) return bfail(MCQ_E_ARG, "null argument");
    if (n_targets != t->n_targets) return bfail(MCQ_E_ARG, "n_targets is not the table's (" + std::to_string(t->n_targets) + ")");
    if (max_keys < 1 || max_keys > 255) return bfail(MCQ_E_ARG, "max_keys must be 1..255");
    BCHK(hipSetDevice(t->device));
    const u64 nk = t->n_keys;
    const u32* keys = t->keys.get(); const u64 *list_off = t->list_off.get(), *locs = t->locs.get();
    Dev<u32> d_key;
    const u32* keyp = tgt_key;
    if (!(flags & MCQ_DEVICE_PTRS)) {
        BCHK(d_key.alloc(n_targets));
        BCHK(hipMemcpy(d_key.get(), tgt_key, (u64)n_targets * 4, hipMemcpyHostToDevice));
        keyp = d_key.get();
    }
    u64 n_kept = 0;
    MCHK(filter_table(t,
        [&](dim3 grid, u32* cnt, u32* alive) {
            if (max_keys == 1)
                hipLaunchKernelGGL(k_ambig_count<true>, grid, dim3(TB), 0, 0, list_off, locs, nk, keyp, n_targets, max_keys, cnt, alive);
            else
                hipLaunchKernelGGL(k_ambig_count<false>, grid, dim3(TB), (TB / SPLIT_GROUP) * (max_keys + 1) * 4, 0, list_off, locs, nk,
                                   keyp, n_targets, max_keys, cnt, alive);
        },
        [&](dim3 grid, const u32* alive, const u64* key_pos, const u64* loc_pos, u64 n_keys_out, u64 n_locs_out, u32* okeys, u64* ooff, u64* olocs) {
            hipLaunchKernelGGL(k_ambig_scatter, grid, dim3(TB), 0, 0, keys, list_off, locs, nk, alive, key_pos, loc_pos,
                               n_keys_out, n_locs_out, okeys, ooff, olocs);
        }, out, &n_kept));
    *n_removed = nk - n_kept;
    return MCQ_OK;
}

extern "C" int mcq_table_tgt_windows(const mcq_table* t, uint32_t* out) {
    if (!t || !out) return bfail(MCQ_E_ARG, "null argument");
    BCHK(hipSetDevice(t->device));
    std::vector<u64> w((size_t)t->n_targets + 1);
    BCHK(hipMemcpy(w.data(), t->win_off.get(), w.size() * 8, hipMemcpyDeviceToHost));
    for (u32 i = 0; i < t->n_targets; ++i) out[i] = (u32)(w[i + 1] - w[i]);
    return MCQ_OK;
}
