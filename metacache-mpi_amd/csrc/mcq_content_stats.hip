// mcq_content_stats.hip -- content statistics of a database over chunks of (feature, target, window) triples
// (mcq_content_stats_* of include/mcq.h).
//
// What `metacache_mpi info DB statistics` reports about a table's buckets (print_content_properties, src/sketch_database.h:1205-1237:
// location_list_size_statistics pushes every bucket's size into a statistics_accumulator, src/stat_combined.h) needs, per bucket
// of `len` locations, 1, len, len^2, len^3 and the maximum; a histogram of the sizes and the locations of every target come from the
// same pass.  A chunk is what mcq_shard_stream_next hands out -- whole key records of one shard file --, so a maximal run of equal
// features is one bucket of one rank, as in mcq_bucket_limit.hip, whose tile shape this unit follows.
//
// Shape: memory-bound, 8 B read per triple (feat, tgt; win is not read), one launch over tiles of CS_TILE triples.
//   k_cs_add   the run heads of the tile as a bit mask in LDS (one ballot per 64 triples); the tile's last run is followed behind the
//              tile by the first wave, 64 triples a step.  Only a run's first triple contributes: from its run length (the next head
//              above it by a bit scan) it adds 1, len, len^2, len^3, the maximum and one histogram bin.  The five numbers are reduced
//              in the wave by shuffles, then over the waves in LDS; bins 1..4 (nearly every bucket of a real table) are counted by
//              ballot and popcount, the others by LDS atomics into the workgroup's 256 bins.  One ordinary atomic per non-zero counter
//              and bin per workgroup goes to the chunk's 64-bit counters.
//              Targets: inside a bucket the file's locations come in build order, so equal targets are neighbours: a wave's 64
//              targets are cut into stretches of equal neighbours by a ballot, each stretch's first lane adds its length (a popcount)
//              with one atomic.  A target >= n_targets adds nothing and leaves the smallest such triple index in the error word.
// The chunk's counters are zeroed before and copied to the host after every launch and summed there, so a chunk with a bad target
// changes no total; its additions to the target counts are taken back by the same kernel run with `undo` (it subtracts what the first
// run added and touches nothing else).  All sums are integers; every store is a plain store or a vector atomic.
#include "mcq_internal.hpp"

namespace {
constexpr u32 CS_TB = 256;                 // threads per workgroup: 4 waves
constexpr u32 CS_TILE = 2048;              // triples per workgroup: every wave takes 512 contiguous ones, 64 a step
constexpr u32 CS_WORDS = CS_TILE / 64;     // head words per tile
constexpr u32 CS_WAVES = CS_TB / 64;
constexpr u32 CS_WAVE_SPAN = CS_TILE / CS_WAVES;
constexpr u32 CS_SMALL = 4;                // bins 1..CS_SMALL are counted by ballot
// the chunk's counters: [0] buckets, [1] locations, [2] sum of len^2, [3] sum of len^3, [4] largest len, [5 + s] hist[s], [CS_ERR] the
// smallest index of a triple whose target is out of range (~0: none)
constexpr u32 CS_HIST = 5;
constexpr u32 CS_ERR = CS_HIST + 256;
constexpr u32 CS_WORDS_ALL = CS_ERR + 1;

__device__ inline u64 cs_wave_sum(u64 v) { for (u32 d = 32; d; d >>= 1) v += __shfl_xor(v, (int)d, 64); return v; }
__device__ inline u64 cs_wave_max(u64 v) { for (u32 d = 32; d; d >>= 1) { const u64 o = __shfl_xor(v, (int)d, 64); v = o > v ? o : v; } return v; }

__global__ __launch_bounds__(CS_TB) void k_cs_add(const u32* __restrict__ feat, const u32* __restrict__ tgt, u64 n, u32 n_targets, int undo,
                                                   unsigned long long* __restrict__ counters, unsigned long long* __restrict__ tgt_cnt) {
    __shared__ unsigned long long heads[CS_WORDS];     // bit j of word w: triple w * 64 + j of the tile starts a run
    __shared__ u64 fwd_s;                               // triples of the tile's last run behind the tile
    __shared__ u32 hist[256];
    __shared__ u64 part[CS_WAVES][5];
    const u64 t0 = (u64)blockIdx.x * CS_TILE;
    const u64 t1 = (t0 + CS_TILE < n) ? t0 + CS_TILE : n;     // (t0 < n: the grid has ceil(n / CS_TILE) workgroups)
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    hist[threadIdx.x] = 0;
    // the run heads of the tile, and the targets' counts
    for (u32 it = 0; it < CS_WAVE_SPAN / 64; ++it) {
        const u64 i = t0 + wave * CS_WAVE_SPAN + it * 64 + lane;
        const bool valid = i < t1;
        if (!undo) {
            const bool head = valid && (i == 0 || feat[i - 1] != feat[i]);
            const unsigned long long m = __ballot(head);
            if (lane == 0) heads[wave * (CS_WAVE_SPAN / 64) + it] = m;
        }
        const u32 t = valid ? tgt[i] : 0u;
        const u32 prev = __shfl_up(t, 1, 64);
        const bool first = valid && (lane == 0 || t != prev);          // first lane of a stretch of equal neighbours
        const unsigned long long vm = __ballot(valid), fm = __ballot(first);
        if (first) {
            const unsigned long long above = lane == 63 ? 0ull : fm & (~0ull << (lane + 1));
            const unsigned long long upto = above ? (1ull << (u32)__builtin_ctzll(above)) - 1ull : ~0ull;    // lanes below the next stretch
            const unsigned long long cnt = (u32)__builtin_popcountll(vm & upto & (~0ull << lane));
            if (t < n_targets) atomicAdd(&tgt_cnt[t], undo ? 0ull - cnt : cnt);
            else if (!undo) atomicMin(&counters[CS_ERR], (unsigned long long)i);
        }
    }
    if (undo) return;                                   // (the whole grid: no barrier was passed)
    // the tile's last run, followed behind the tile by the first wave
    if (wave == 0) {
        const u32 fl = feat[t1 - 1];
        u64 fwd = 0;
        for (u64 j = t1; j < n;) {                      // triples j, j + 1, ... equal to the tile's last
            const bool eq = (j + lane < n) && feat[j + lane] == fl;
            const unsigned long long m = __ballot(eq);
            if (m == ~0ull) { fwd += 64; j += 64; continue; }
            fwd += (u32)__builtin_ctzll(~m);
            break;
        }
        if (lane == 0) fwd_s = fwd;
    }
    __syncthreads();
    u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0, mx = 0;
    u32 small[CS_SMALL] = {0, 0, 0, 0};                 // (the same in every lane of the wave)
    for (u32 it = 0; it < CS_WAVE_SPAN / 64; ++it) {
        const u32 w = wave * (CS_WAVE_SPAN / 64) + it;
        const u64 i = t0 + (u64)w * 64 + lane;
        u64 len = 0;
        if ((heads[w] >> lane) & 1ull) {                // (a head bit implies i < t1)
            // end (exclusive): the nearest head above it; none in the tile: the run goes on fwd_s triples behind it
            unsigned long long m = lane == 63 ? 0ull : heads[w] & (~0ull << (lane + 1));
            u32 ww = w;
            while (!m && ww + 1 < CS_WORDS) m = heads[++ww];
            const u64 end = m ? t0 + (u64)ww * 64 + (u32)__builtin_ctzll(m) : t1 + fwd_s;
            len = end - i;
            s0 += 1; s1 += len; s2 += len * len; s3 += len * len * len;
            mx = len > mx ? len : mx;
            if (len > CS_SMALL) atomicAdd(&hist[len < 255 ? (u32)len : 255u], 1u);
        }
        for (u32 b = 0; b < CS_SMALL; ++b) small[b] += (u32)__builtin_popcountll(__ballot(len == b + 1));
    }
    s0 = cs_wave_sum(s0); s1 = cs_wave_sum(s1); s2 = cs_wave_sum(s2); s3 = cs_wave_sum(s3); mx = cs_wave_max(mx);
    if (lane == 0) {
        part[wave][0] = s0; part[wave][1] = s1; part[wave][2] = s2; part[wave][3] = s3; part[wave][4] = mx;
        for (u32 b = 0; b < CS_SMALL; ++b) if (small[b]) atomicAdd(&hist[b + 1], small[b]);
    }
    __syncthreads();
    const u32 h = hist[threadIdx.x];
    if (h) atomicAdd(&counters[CS_HIST + threadIdx.x], (unsigned long long)h);
    if (threadIdx.x < 4) {
        u64 v = 0;
        for (u32 q = 0; q < CS_WAVES; ++q) v += part[q][threadIdx.x];
        if (v) atomicAdd(&counters[threadIdx.x], (unsigned long long)v);
    } else if (threadIdx.x == 4) {
        u64 v = 0;
        for (u32 q = 0; q < CS_WAVES; ++q) v = part[q][4] > v ? part[q][4] : v;
        if (v) atomicMax(&counters[4], (unsigned long long)v);
    }
}
}  // namespace

// The handle owns every byte the calls use: the chunk's counters, the targets' counts, a staging copy of feat and tgt for host pointers
// (grown to the largest chunk seen) and the pinned words the counters come back through.  Plain hipMalloc, nothing per chunk.
struct mcq_content_stats {
    int device = 0;
    u32 n_targets = 0;
    hipStream_t stream = nullptr;
    mcq_content_totals tot;
    u64 st_cap = 0;
    Dev<unsigned long long> counters, tgt_cnt;
    Dev<u32> st_feat, st_tgt;
    Pinned<unsigned long long> h_counters;
};

extern "C" int mcq_content_stats_create(uint32_t n_targets, mcq_content_stats** out) {
    if (!out) return fail(MCQ_E_ARG, "null argument");
    *out = nullptr;
    if (!n_targets) return fail(MCQ_E_ARG, "mcq_content_stats_create: n_targets must be at least 1");
    std::unique_ptr<mcq_content_stats> h(new mcq_content_stats());
    HIPCHK(hipGetDevice(&h->device));
    h->n_targets = n_targets;
    memset(&h->tot, 0, sizeof(h->tot));
    HIPCHK(h->counters.alloc(CS_WORDS_ALL));
    HIPCHK(h->tgt_cnt.alloc(n_targets));
    HIPCHK(h->h_counters.alloc(CS_WORDS_ALL));
    HIPCHK(hipMemset(h->tgt_cnt.get(), 0, (u64)n_targets * 8));
    *out = h.release();
    return MCQ_OK;
}

extern "C" int mcq_content_stats_set_stream(mcq_content_stats* h, void* stream) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    h->stream = (hipStream_t)stream;
    return MCQ_OK;
}

extern "C" int mcq_content_stats_add(mcq_content_stats* h, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n, uint32_t flags) {
    (void)win;
    if (!h) return fail(MCQ_E_ARG, "null argument");
    if (!n) return MCQ_OK;
    if (!feat || !tgt) return fail(MCQ_E_ARG, "null argument");
    if (n >= (1ull << 40)) return fail(MCQ_E_UNSUPPORTED, "a chunk holds fewer than 2^40 triples");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const u32 *df = feat, *dt = tgt;
    if (!(flags & MCQ_DEVICE_PTRS)) {
        if (n > h->st_cap) {
            h->st_cap = 0;
            HIPCHK(h->st_feat.alloc(n)); HIPCHK(h->st_tgt.alloc(n));
            h->st_cap = n;
        }
        HIPCHK(hipMemcpyAsync(h->st_feat.get(), feat, n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->st_tgt.get(), tgt, n * 4, hipMemcpyHostToDevice, s));
        df = h->st_feat.get(); dt = h->st_tgt.get();
    }
    const u32 n_tiles = (u32)((n + CS_TILE - 1) / CS_TILE);
    unsigned long long* c = h->h_counters.get();
    HIPCHK(hipMemsetAsync(h->counters.get(), 0, CS_ERR * 8, s));
    HIPCHK(hipMemsetAsync(h->counters.get() + CS_ERR, 0xFF, 8, s));
    hipLaunchKernelGGL(k_cs_add, dim3(n_tiles), dim3(CS_TB), 0, s, df, dt, (u64)n, h->n_targets, 0, h->counters.get(), h->tgt_cnt.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c, h->counters.get(), CS_WORDS_ALL * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (c[CS_ERR] != ~0ull) {
        // a target out of range: nothing of this chunk stays -- the totals were not touched yet, the targets' counts are taken back
        const u64 bad = c[CS_ERR] < n ? c[CS_ERR] : 0;
        u32 t = 0;
        hipLaunchKernelGGL(k_cs_add, dim3(n_tiles), dim3(CS_TB), 0, s, df, dt, (u64)n, h->n_targets, 1, h->counters.get(), h->tgt_cnt.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&t, dt + bad, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return fail(MCQ_E_ARG, "mcq_content_stats_add: triple " + std::to_string(bad) + " of the chunk names target " + std::to_string(t) +
                               ", the handle has " + std::to_string(h->n_targets) + " targets");
    }
    mcq_content_totals& T = h->tot;
    T.n_buckets += c[0]; T.n_locations += c[1]; T.sum2 += c[2]; T.sum3 += c[3];
    if (c[4] > T.max_size) T.max_size = c[4];
    for (u32 b = 0; b < 256; ++b) T.hist[b] += c[CS_HIST + b];
    return MCQ_OK;
}

extern "C" int mcq_content_stats_totals(mcq_content_stats* h, mcq_content_totals* out) {
    if (!h || !out) return fail(MCQ_E_ARG, "null argument");
    *out = h->tot;
    return MCQ_OK;
}

extern "C" int mcq_content_stats_target_locations(mcq_content_stats* h, uint64_t* out) {
    if (!h || !out) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, h->tgt_cnt.get(), (u64)h->n_targets * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MCQ_OK;
}

extern "C" int mcq_content_stats_reset(mcq_content_stats* h) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    memset(&h->tot, 0, sizeof(h->tot));
    return MCQ_OK;
}

extern "C" int mcq_content_stats_free(mcq_content_stats* h) {
    delete h;
    return MCQ_OK;
}
