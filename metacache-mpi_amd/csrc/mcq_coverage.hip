// mcq_coverage.hip -- breadth of coverage per reference sequence, accumulated over all batches of a run on the device
// (mcq_coverage_* of include/mcq.h).
//
// mcq_target_hits leaves, per query and slot, the window range of the read's candidate on the slot's target and the read's matches
// on every window of it.  This unit keeps what a whole input adds up to and nothing per read: one bit per (target, window) -- set once
// some read had a match there --, and per target the number of (query, slot) entries and the sum of their matches.  A target's
// segment of the bitmap starts on a 32-bit word: word_off[t + 1] = word_off[t] + ceil(windows[t] / 32).
//
// Shape: memory-bound, one launch over the flattened counts array, 4 B read per word of it, CV_TB consecutive words per workgroup,
// so a wave's loads are one contiguous 256 B stretch whatever range_cap is (3 for a read of 150 bases, hundreds for a long read).
//   k_cv_add   a thread owns word e = slot * range_cap + i.  It reads its slot's range (16 B; the threads of a slot read the same
//              ones), and if i < n_win the count -- the words from n_win on are never loaded.  A count > 0 tests the window's bitmap
//              word and issues the atomic OR only when the bit is missing: coverage saturates, and once it has, a batch costs loads
//              only.  The counts of a slot are summed by a segmented scan over the wave (slots are contiguous in e); the last lane of
//              every stretch adds its sum to hits[tgt] with one atomic, the thread with i == 0 adds 1 to queries[tgt].
//              A slot whose target is not below n_targets, whose range ends behind windows[tgt], or that is wider than range_cap is
//              skipped as a whole and counted once in out_of_range: no word outside a target's segment is ever addressed.
//   k_cv_read  one wave per target: the set bits of its segment (bits from windows[t] on are never set), and the target's three numbers
//              as one mcq_target_coverage.
// All sums are integers, so they do not depend on the order of the adds; every store is a plain store or a vector atomic.
#include "mcq_internal.hpp"

namespace {
constexpr u32 CV_TB = 256;                 // threads per workgroup: 4 waves, 256 consecutive words of counts

__device__ inline u64 cv_wave_sum32(u32 v) { u64 s = v; for (u32 d = 32; d; d >>= 1) s += __shfl_xor(s, (int)d, 64); return s; }

__global__ __launch_bounds__(CV_TB) void k_cv_add(const uint4* __restrict__ ranges, const u32* __restrict__ counts, u64 n_rows, u32 range_cap,
                                                   const u32* __restrict__ windows, const u64* __restrict__ word_off, u32 n_targets,
                                                   u32* __restrict__ bitmap, unsigned long long* __restrict__ queries,
                                                   unsigned long long* __restrict__ hits, unsigned long long* __restrict__ out_of_range) {
    const u32 lane = threadIdx.x & 63;
    // the workgroup's first word lies in row row0 (one 64-bit division, the same in every thread); the rest is 32-bit arithmetic
    const u64 e0 = (u64)blockIdx.x * CV_TB;
    const u64 row0 = e0 / range_cap;
    const u32 r = (u32)(e0 - row0 * range_cap) + threadIdx.x;          // < range_cap + CV_TB
    const u64 row = row0 + r / range_cap;
    const u32 i = r % range_cap;
    u32 c = 0, tgt = MCQ_TARGET_UNUSED;
    if (row < n_rows) {
        const uint4 rg = ranges[row];                                   // tgt, hits, win_beg, n_win
        if (rg.x != MCQ_TARGET_UNUSED && rg.w != 0) {
            const bool inside = rg.x < n_targets && rg.w <= range_cap && (u64)rg.z + rg.w <= windows[rg.x < n_targets ? rg.x : 0];
            if (!inside) {
                if (i == 0) atomicAdd(out_of_range, 1ull);
            } else {
                tgt = rg.x;
                if (i == 0) atomicAdd(&queries[tgt], 1ull);
                if (i < rg.w) {
                    c = counts[row * range_cap + i];
                    if (c) {
                        const u32 win = rg.z + i;                       // < windows[tgt]
                        u32* w = bitmap + word_off[tgt] + (win >> 5);
                        const u32 bit = 1u << (win & 31);
                        if (!(*w & bit)) atomicOr(w, bit);
                    }
                }
            }
        }
    }
    // the sums of the rows that cross this wave: a segmented inclusive scan (equal rows are neighbours), then the last lane of a stretch
    u64 s = c;
    for (u32 d = 1; d < 64; d <<= 1) {
        const u64 os = __shfl_up(s, d, 64);
        const u64 orow = __shfl_up(row, d, 64);
        if (lane >= d && orow == row) s += os;
    }
    const u64 nrow = __shfl_down(row, 1, 64);
    if ((lane == 63 || nrow != row) && tgt != MCQ_TARGET_UNUSED && s) atomicAdd(&hits[tgt], (unsigned long long)s);
}

__global__ __launch_bounds__(CV_TB) void k_cv_read(const u32* __restrict__ bitmap, const u64* __restrict__ word_off, u32 n_targets,
                                                    const unsigned long long* __restrict__ queries, const unsigned long long* __restrict__ hits,
                                                    mcq_target_coverage* __restrict__ out) {
    const u32 lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * (CV_TB / 64) + (threadIdx.x >> 6);
    if (t >= n_targets) return;                                         // (whole waves: no barrier below)
    const u64 w0 = word_off[t], w1 = word_off[t + 1];
    u32 n = 0;
    for (u64 w = w0 + lane; w < w1; w += 64) n += (u32)__builtin_popcount(bitmap[w]);
    const u64 covered = cv_wave_sum32(n);                               // <= windows[t] < 2^32
    if (lane == 0) { out[t].hits = hits[t]; out[t].queries = queries[t]; out[t].windows_covered = (u32)covered; out[t].reserved = 0; }
}
}  // namespace

// The handle owns every byte the calls use.  The bitmap has one guard word in front and one behind (zero, never addressed:
// mcq_coverage_bitmap hands them out with the rest, and a test looks at them).
struct mcq_coverage {
    int device = 0;
    u32 n_targets = 0;
    u64 n_words = 0;                       // words of all segments, guards not counted
    Dev<u32> windows, bitmap;
    Dev<u64> word_off;
    Dev<unsigned long long> counters;      // queries[n_targets], hits[n_targets], out_of_range
    Dev<mcq_target_coverage> out;
};

namespace {
int cv_zero(mcq_coverage* h, hipStream_t s) {
    HIPCHK(hipMemsetAsync(h->bitmap.get(), 0, (h->n_words + 2) * 4, s));
    HIPCHK(hipMemsetAsync(h->counters.get(), 0, (2 * (u64)h->n_targets + 1) * 8, s));
    return MCQ_OK;
}
}  // namespace

extern "C" int mcq_coverage_create(const uint32_t* windows, uint32_t n_targets, int32_t device, mcq_coverage** out) {
    if (!out) return fail(MCQ_E_ARG, "null argument");
    *out = nullptr;
    if (!windows || !n_targets) return fail(MCQ_E_ARG, "mcq_coverage_create: windows of at least one target");
    std::vector<u64> off((size_t)n_targets + 1, 0);
    for (u32 t = 0; t < n_targets; ++t) off[t + 1] = off[t] + ((u64)windows[t] + 31) / 32;
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<mcq_coverage> h(new mcq_coverage());
    h->device = device; h->n_targets = n_targets; h->n_words = off[n_targets];
    HIPCHK(h->windows.alloc(n_targets));
    HIPCHK(h->word_off.alloc((u64)n_targets + 1));
    HIPCHK(h->bitmap.alloc(h->n_words + 2));
    HIPCHK(h->counters.alloc(2 * (u64)n_targets + 1));
    HIPCHK(h->out.alloc(n_targets));
    HIPCHK(hipMemcpy(h->windows.get(), windows, (u64)n_targets * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->word_off.get(), off.data(), ((u64)n_targets + 1) * 8, hipMemcpyHostToDevice));
    if (int rc = cv_zero(h.get(), nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    *out = h.release();
    return MCQ_OK;
}

extern "C" int mcq_coverage_add(mcq_coverage* h, const mcq_target_range* ranges, const uint32_t* counts, uint64_t n_queries,
                                uint32_t n_slots, uint32_t range_cap, void* stream) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    if (n_slots < 1 || range_cap < 1 || range_cap > (1u << 31)) return fail(MCQ_E_ARG, "mcq_coverage_add: n_slots at least 1, range_cap 1..2^31");
    if (n_queries == 0) return MCQ_OK;
    if (!ranges || !counts) return fail(MCQ_E_ARG, "null argument");
    if ((uintptr_t)ranges & 15) return fail(MCQ_E_ARG, "mcq_coverage_add: ranges must be 16-byte aligned");
    if (n_queries > (1ull << 40) / n_slots) return fail(MCQ_E_UNSUPPORTED, "mcq_coverage_add: a batch holds at most 2^40 slots");
    const u64 n_rows = n_queries * n_slots;
    const u64 blocks = (n_rows * range_cap + CV_TB - 1) / CV_TB;
    if (blocks > 0x7FFFFFFFull) return fail(MCQ_E_UNSUPPORTED, "mcq_coverage_add: a batch holds fewer than 2^39 count words");
    HIPCHK(hipSetDevice(h->device));
    unsigned long long* q = h->counters.get();
    hipLaunchKernelGGL(k_cv_add, dim3((u32)blocks), dim3(CV_TB), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(ranges), counts, n_rows,
                       range_cap, h->windows.get(), h->word_off.get(), h->n_targets, h->bitmap.get() + 1, q, q + h->n_targets, q + 2 * (u64)h->n_targets);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_coverage_read(mcq_coverage* h, mcq_target_coverage* host_out, uint64_t* out_of_range, void* stream) {
    if (!h || !host_out) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long* q = h->counters.get();
    const u32 per = CV_TB / 64;
    hipLaunchKernelGGL(k_cv_read, dim3((h->n_targets + per - 1) / per), dim3(CV_TB), 0, s, h->bitmap.get() + 1, h->word_off.get(), h->n_targets,
                       q, q + h->n_targets, h->out.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_out, h->out.get(), (u64)h->n_targets * sizeof(mcq_target_coverage), hipMemcpyDeviceToHost, s));
    if (out_of_range) HIPCHK(hipMemcpyAsync(out_of_range, q + 2 * (u64)h->n_targets, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MCQ_OK;
}

extern "C" uint64_t mcq_coverage_bitmap_words(const mcq_coverage* h) { return h ? h->n_words + 2 : 0; }

extern "C" int mcq_coverage_bitmap(mcq_coverage* h, uint32_t* host_words, uint64_t* host_word_off, void* stream) {
    if (!h || !host_words) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host_words, h->bitmap.get(), (h->n_words + 2) * 4, hipMemcpyDeviceToHost, s));
    if (host_word_off) HIPCHK(hipMemcpyAsync(host_word_off, h->word_off.get(), ((u64)h->n_targets + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MCQ_OK;
}

extern "C" int mcq_coverage_reset(mcq_coverage* h, void* stream) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    return cv_zero(h, (hipStream_t)stream);
}

extern "C" int mcq_coverage_free(mcq_coverage* h) {
    delete h;
    return MCQ_OK;
}
