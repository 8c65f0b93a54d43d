#pragma once
// mcq_classify_one.hpp -- the classification of ONE candidate list on the device, shared by k_classify (mcq_classify.hip: the
// candidates of a query batch) and k_mg_finish (mcq_merge.hip: the merged lists of result files): one text for both.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcq {

constexpr uint32_t kClsNumRanks = 21;
constexpr uint32_t kClsNone = 0xFFFFFFFFu;

struct ClassifyRules {
    const uint32_t* lineage;      // [n_taxa * 21]
    const uint8_t* rank;          // [n_taxa]
    uint32_t n_taxa;
    uint32_t hits_min;
    float frac;
    uint32_t highest;
};

__device__ __forceinline__ bool cls_valid_key(uint32_t key, uint32_t n_taxa) { return key != kClsNone && (key & 0x7FFFFFFFu) < n_taxa; }

// mcq_refdb_classify (csrc/host/mcq_host.cpp) on the (tax, hits) pairs c[0 .. n)
__device__ inline uint32_t classify_one(const uint2* c, uint32_t n, const ClassifyRules& a) {
    if (n == 0 || !cls_valid_key(c[0].x, a.n_taxa)) return kClsNone;
    const uint32_t h0 = c[0].y;
    if (h0 < a.hits_min) return kClsNone;
    uint32_t lca = c[0].x & 0x7FFFFFFFu;
    const float thr = h0 > a.hits_min ? __fmul_rn(__uint2float_rn(h0 - a.hits_min), a.frac) : 0.0f;
    for (uint32_t i = 1; i < n; ++i) {
        if (!(__uint2float_rn(c[i].y) > thr)) break;
        uint32_t r = kClsNone;
        if (cls_valid_key(c[i].x, a.n_taxa)) {
            const uint32_t* la = a.lineage + (uint64_t)lca * kClsNumRanks;
            const uint32_t* lb = a.lineage + (uint64_t)(c[i].x & 0x7FFFFFFFu) * kClsNumRanks;
            for (uint32_t j = 0; j < kClsNumRanks; ++j) {
                const uint32_t x = la[j];
                if (x != kClsNone && x == lb[j]) { r = x; break; }
            }
        }
        lca = r;
        if (lca == kClsNone || a.rank[lca] > a.highest) return kClsNone;
    }
    return a.rank[lca] <= a.highest ? lca : kClsNone;
}

}  // namespace mcq
