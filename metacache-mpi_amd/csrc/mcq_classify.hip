// mcq_classify.hip -- classification and per-taxon read counts on the device (include/mcq.h: mcq_taxonomy_*, mcq_classify).
//
// k_classify: one thread per query, 256 per workgroup, a grid of the resident workgroups looping over the batch in chunks
// of 256 queries.  Per chunk the workgroup stages its (taxon, hits) pairs into LDS from 16-B loads of consecutive
// candidates (the chunk's candidate lists are one contiguous range: every load instruction covers 1 KiB), then every
// thread classifies its query from LDS as mcq_refdb_classify does (src/classification.cpp:235-265): the threshold
// (float)(h0 - hits_min) * frac as one fp32 multiply, the ranked LCA (src/taxonomy.h:531-537) over the device lineage
// table, whose rows are read only for candidates above the threshold.
// Counting: per workgroup an LDS table taxon -> count (4096 slots, open addressing); a key that finds no slot within
// 16 probes goes to global memory directly, one 64-bit atomic per distinct key of the wave.  At the end every occupied
// slot is one global 64-bit atomic: a taxon that holds every read costs one atomic per workgroup, not one per read.
// Integer counts make the result independent of the order of the adds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>

#include "mcq_classify.hpp"
#include "mcq_classify_one.hpp"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kNumRanks = mcq::kClsNumRanks;
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr int kThreads = 256;
constexpr int kMaxCand = 16;
constexpr int kTableLog2 = 12;
constexpr u32 kTable = 1u << kTableLog2;
constexpr int kProbes = 16;

struct ClassifyArgs {
    const uint4* cands;           // [n * max_cand] {tax, hits, win_beg, win_end}
    const u32* n_cand;            // [n]
    u64 n;
    u32 max_cand;
    mcq::ClassifyRules rules;     // lineage table, ranks and the options: what classify_one (mcq_classify_one.hpp) reads
    u32* best;                    // [n] or null
    unsigned long long* counts;   // [n_taxa + 1] or null
};

template <bool COUNT>
__global__ __launch_bounds__(kThreads) void k_classify(ClassifyArgs a) {
    extern __shared__ uint2 s_cand[];                 // [kThreads * max_cand]: the chunk's (tax, hits) pairs (8 KiB at max_cand 4)
    __shared__ u32 s_key[COUNT ? kTable : 1];
    __shared__ u32 s_cnt[COUNT ? kTable : 1];
    const u32 tid = threadIdx.x, lane = tid & 63;
    if (COUNT) {
        for (u32 i = tid; i < kTable; i += kThreads) { s_key[i] = kNone; s_cnt[i] = 0; }
    }
    const u32 mc = a.max_cand;
    for (u64 base = (u64)blockIdx.x * kThreads; base < a.n; base += (u64)gridDim.x * kThreads) {
        const u32 nq = (u32)min<u64>(kThreads, a.n - base);
        __syncthreads();                                              // (the previous chunk's pairs are read; the table is set up)
        const uint4* src = a.cands + base * mc;
        for (u32 u = tid; u < nq * mc; u += kThreads) {
            const uint4 v = src[u];
            s_cand[u] = make_uint2(v.x, v.y);
        }
        __syncthreads();
        u32 key = kNone;
        if (tid < nq) {
            const u64 q = base + tid;
            const u32 n = min(a.n_cand[q], mc);
            const u32 b = mcq::classify_one(&s_cand[tid * mc], n, a.rules);
            if (a.best) a.best[q] = b;
            key = b == kNone ? a.rules.n_taxa : b;
        }
        if (COUNT) {
            bool pending = false;
            if (key != kNone) {
                const u32 h = (key * 0x9E3779B1u) >> (32 - kTableLog2);
                pending = true;
                for (int p = 0; p < kProbes; ++p) {
                    const u32 slot = (h + (u32)p) & (kTable - 1);
                    const u32 prev = atomicCAS(&s_key[slot], kNone, key);
                    if (prev == kNone || prev == key) { atomicAdd(&s_cnt[slot], 1u); pending = false; break; }
                }
            }
            // table full around this key: one global atomic per distinct key of the wave
            u64 todo = __ballot(pending);
            while (todo) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const u32 lk = __shfl(key, leader);
                const u64 same = __ballot(pending && key == lk);
                if ((int)lane == leader) atomicAdd(&a.counts[lk], (unsigned long long)__popcll(same));
                if (pending && key == lk) pending = false;
                todo &= ~same;
            }
        }
    }
    if (COUNT) {
        __syncthreads();
        for (u32 i = tid; i < kTable; i += kThreads)
            if (s_key[i] != kNone && s_cnt[i]) atomicAdd(&a.counts[s_key[i]], (unsigned long long)s_cnt[i]);
    }
}

}  // namespace

extern "C" int mcq_taxonomy_create(const uint32_t* lineage, const uint8_t* rank, uint32_t n_taxa, int32_t device, mcq_taxonomy** out) {
    if (!lineage || !rank || !out) return mcq::set_error(MCQ_E_ARG, "null argument");
    if (n_taxa < 1 || n_taxa >= (1u << 31)) return mcq::set_error(MCQ_E_ARG, "n_taxa must be 1 .. 2^31 - 1");
    // every index the kernel may follow must lie inside the table
    for (u64 i = 0; i < (u64)n_taxa * kNumRanks; ++i)
        if (lineage[i] != kNone && lineage[i] >= n_taxa) return mcq::set_error(MCQ_E_ARG, "lineage entry outside the taxa");
    if (hipSetDevice(device) != hipSuccess) return mcq::set_error(MCQ_E_HIP, "hipSetDevice failed");
    mcq_taxonomy* tx = new mcq_taxonomy();
    tx->device = device; tx->n_taxa = n_taxa;
    const u64 lb = (u64)n_taxa * kNumRanks * 4;
    if (hipMalloc(&tx->lineage, lb) != hipSuccess || hipMalloc(&tx->rank, n_taxa) != hipSuccess ||
        hipMemcpy(tx->lineage, lineage, lb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tx->rank, rank, n_taxa, hipMemcpyHostToDevice) != hipSuccess) {
        mcq_taxonomy_destroy(tx);
        return mcq::set_error(MCQ_E_HIP, "allocating / copying the lineage table failed");
    }
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) n_cu = 256;
    for (int m = 1; m <= kMaxCand; ++m) {                 // resident workgroups per max_cand (the staging area grows with it)
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_classify<true>, kThreads, (size_t)m * kThreads * 8) != hipSuccess || per_cu < 1) per_cu = 2;
        tx->grid[m] = (u32)(per_cu * n_cu);
    }
    *out = tx;
    return MCQ_OK;
}

extern "C" int mcq_taxonomy_destroy(mcq_taxonomy* tx) {
    if (!tx) return MCQ_OK;
    (void)hipSetDevice(tx->device);
    if (tx->lineage) (void)hipFree(tx->lineage);
    if (tx->rank) (void)hipFree(tx->rank);
    delete tx;
    return MCQ_OK;
}

int mcq::check_classify_opts(const mcq_classify_opts* o) {
    if (!o) return set_error(MCQ_E_ARG, "classify opts is null");
    if (o->flags) return set_error(MCQ_E_ARG, "unknown bits in mcq_classify_opts.flags");
    return MCQ_OK;
}

extern "C" int mcq_classify(const mcq_taxonomy* tx, const mcq_result* cands, uint64_t n_queries, uint32_t max_cand,
                            const mcq_classify_opts* opts, uint32_t* best, uint64_t* counts, void* stream) {
    if (!tx || !cands) return mcq::set_error(MCQ_E_ARG, "null argument");
    int rc = mcq::check_classify_opts(opts);
    if (rc) return rc;
    if (!(cands->flags & MCQ_DEVICE_PTRS)) return mcq::set_error(MCQ_E_ARG, "mcq_classify takes the device result (MCQ_DEVICE_PTRS)");
    if (max_cand < 1 || max_cand > kMaxCand) return mcq::set_error(MCQ_E_UNSUPPORTED, "max_cand must be in 1..16");
    if (n_queries == 0 || (!best && !counts)) return MCQ_OK;
    if (!cands->cands || !cands->n_cand) return mcq::set_error(MCQ_E_ARG, "null candidate buffers");
    if (hipSetDevice(tx->device) != hipSuccess) return mcq::set_error(MCQ_E_HIP, "hipSetDevice failed");
    ClassifyArgs a;
    a.cands = reinterpret_cast<const uint4*>(cands->cands); a.n_cand = cands->n_cand; a.n = n_queries; a.max_cand = max_cand;
    a.rules.lineage = tx->lineage; a.rules.rank = tx->rank; a.rules.n_taxa = tx->n_taxa;
    a.rules.hits_min = opts->hits_min; a.rules.frac = opts->hits_diff_fraction; a.rules.highest = opts->highest_rank;
    a.best = best; a.counts = reinterpret_cast<unsigned long long*>(counts);
    const u32 grid = (u32)std::min<u64>(tx->grid[max_cand], (n_queries + kThreads - 1) / kThreads);
    const size_t lds = (size_t)max_cand * kThreads * 8;
    if (counts) hipLaunchKernelGGL(k_classify<true>, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_classify<false>, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mcq::set_error(MCQ_E_HIP, (std::string("k_classify: ") + hipGetErrorString(e)).c_str());
    return MCQ_OK;
}
