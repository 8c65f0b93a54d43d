// mcq_align.hip -- semi-global alignment of every query of a batch against one subject each (mcq_align): what the reference's
// make_semi_global_alignment (src/classification.cpp:77-103) computes for `-align`, bit for bit -- align_semi_global with
// default_alignment_scheme (src/alignment.h), both orientations of mate 1, the score-only passes of mate 2, the comparison of the two
// sums as std::size_t, and the backtrace of the winner.
//
// One wavefront per query, a grid of resident waves that stride over the jobs, no workgroup barrier.  The dynamic programme runs as a
// skewed sweep: lane l owns AL_W adjacent subject columns, and at step t it works query row t - l, so the cell to the left of its strip
// (row t - l, lane l - 1's last column) was finished one step earlier and arrives by a one-lane wave shift; the diagonal neighbour is
// that same value one step older.  Inside a strip the columns resolve left to right in registers.  A subject wider than 64 x AL_W
// columns is worked panel by panel; the last column of a panel waits in LDS (one 16-bit score per query row) for lane 0 of the next.
// Score-only passes keep nothing else.  The pass that is traced back packs the predecessors at 2 bits per cell, one 16-bit word per
// lane and step, into LDS when rows x strips fits AL_LDS_WORDS, else into the wave's area of the workspace's scratch memory.  Mate 1's
// two score passes run first, so only the winner is traced.  The walk back is lane 0's serial chase: once to learn the length, once
// more to write the two strings front to back.  The oriented query and the subject are staged in LDS for the sweep and the walk.
// AL_W = 8 was chosen from the register count alone; nothing here is tuned.
#include "mcq_internal.hpp"

#include <atomic>

namespace {

constexpr u32 AL_W = 8;                         // subject columns per lane: one u16 of predecessors per lane and step
constexpr u32 AL_PANEL = 64 * AL_W;             // columns one sweep covers
constexpr u32 AL_LDS_WORDS = 10240;             // predecessor words (u16) a wave keeps in LDS: 20 KiB -- 150 rows x 59 strips fit
constexpr u64 AL_SCRATCH_BUDGET = 256ull << 20; // bytes of scratch a workspace holds once a call needs any: 128 areas of the largest matrix the
                                                // capacities allow; a call that needs scratch divides it among its waves
static_assert(AL_W * 2 == 16, "a lane's predecessors of one row fill one 16-bit word");
static_assert(MCQ_ALIGN_MAX_SUBJECT % AL_W == 0, "the subject capacity is a whole number of strips");

struct AlArgs {
    const char* subjects;
    const mcq_align_job* jobs;
    u32 max_query, max_subject, text_cap;
    mcq_alignment* out;
    char* out_query; char* out_subject;
    unsigned short* scratch;     // [grid * scratch_words] of the workspace's area, or null: every job of the call fits LDS
    u64 scratch_words;           // per wave
};

__device__ __forceinline__ u32 al_complement(u32 c) {
    switch (c) {
        case 'A': return 'T'; case 'a': return 't';
        case 'C': return 'G'; case 'c': return 'g';
        case 'G': return 'C'; case 'g': return 'c';
        case 'T': return 'A'; case 't': return 'a';
        default: return c;
    }
}

// the oriented mate into LDS
__device__ __forceinline__ void al_stage_query(const char* __restrict__ bases, u64 off, u32 len, bool reverse, unsigned char* s_q, u32 lane) {
    for (u32 i = lane; i < len; i += 64)
        s_q[i] = reverse ? (unsigned char)al_complement((unsigned char)bases[off + (len - 1 - i)]) : (unsigned char)bases[off + i];
    wave_sync();
}

// end-cell candidates in the order the reference visits them: 0 the corner, then rows 1 .. lq-1 of the last column, then columns
// 1 .. ls-1 of the last row; the first of the largest wins (every later one must be strictly greater)
__device__ __forceinline__ u64 al_key(int v, u32 order) {
    return ((u64)(u32)(v + 0x40000000) << 32) | (u64)(0xFFFFFFFFu - order);
}

// One pass over the score matrix of s_q[0, lq) against s_sub[0, ls), lq, ls >= 1.  Returns, wave-uniform, the key of the end cell.
// TRACE: the predecessors go to P[(row - 1) * nstrips + strip].
template <bool TRACE, class PT>
__device__ __forceinline__ u64 al_pass(const unsigned char* s_q, u32 lq, const unsigned char* s_sub, u32 ls, short* s_bnd,
                                       PT* P, u32 nstrips, u32 lane) {
    u64 best = 0;
    const u32 npanels = (ls + AL_PANEL - 1) / AL_PANEL;
    for (u32 p = 0; p < npanels; ++p) {
        const u32 c0 = p * AL_PANEL + lane * AL_W;              // my columns: c0 + j + 1 (1-based), j < AL_W
        const u32 cols = ls - p * AL_PANEL < AL_PANEL ? ls - p * AL_PANEL : AL_PANEL;
        const u32 lanes_used = (cols + AL_W - 1) / AL_W;
        u32 sc[AL_W];
#pragma unroll
        for (u32 j = 0; j < AL_W; ++j) sc[j] = c0 + j < ls ? (u32)s_sub[c0 + j] : 0x100u + j;     // behind the end: equals no base
        int h[AL_W];
#pragma unroll
        for (u32 j = 0; j < AL_W; ++j) h[j] = 0;                // row 0
        const u32 jl = ls - 1 - c0;                             // < AL_W on the lane that owns the last column
        int left_prev = 0;                                      // the cell left of my strip in the row above
        int carry = 0;                                          // my last column in the row I worked last
        const u32 nsteps = lq + lanes_used - 1;
        for (u32 t = 0; t < nsteps; ++t) {
            int from_left = __shfl_up(carry, 1, 64);
            const u32 i = t - lane + 1;                         // my row (1-based); wraps for lanes that have not started
            const bool act = lane <= t && i <= lq && lane < lanes_used;
            if (lane == 0) from_left = (p != 0 && act) ? (int)s_bnd[i] : 0;
            if (act) {
                const u32 qc = s_q[i - 1];
                int diag = left_prev, left = from_left;
                u32 pw = 0;
#pragma unroll
                for (u32 j = 0; j < AL_W; ++j) {
                    int d = diag + (qc == sc[j] ? 2 : -1);
                    u32 pr = 1;
                    const int a = h[j] - 1;
                    if (a > d) { d = a; pr = 2; }
                    const int l = left - 1;
                    if (l > d) { d = l; pr = 3; }
                    diag = h[j]; h[j] = d; left = d;
                    pw |= pr << (2 * j);
                }
                left_prev = from_left;
                carry = h[AL_W - 1];
                if (lane == 63 && p + 1 < npanels) s_bnd[i] = (short)carry;
                if (TRACE) P[(u64)(i - 1) * nstrips + (p * 64 + lane)] = (PT)pw;      // lane < lanes_used: the strip exists
                if (jl < AL_W) {
                    int v = 0;
#pragma unroll
                    for (u32 j = 0; j < AL_W; ++j) v = j == jl ? h[j] : v;
                    const u64 k = al_key(v, i == lq ? 0u : i);
                    best = k > best ? k : best;
                }
                if (i == lq) {
#pragma unroll
                    for (u32 j = 0; j < AL_W; ++j) {
                        const u32 c = c0 + j + 1;
                        if (c < ls) { const u64 k = al_key(h[j], lq + c); best = k > best ? k : best; }
                    }
                }
            }
        }
        wave_sync();                                            // the boundary column is complete before the next panel reads it
    }
    return wave_max(best);
}

__device__ __forceinline__ int al_key_score(u64 key) { return (int)((u32)(key >> 32) - 0x40000000u); }

template <class PT>
__device__ __forceinline__ u32 al_pred(const PT* P, u32 nstrips, u32 i, u32 c) {
    if (i == 0 || c == 0) return 0;
    return ((u32)P[(u64)(i - 1) * nstrips + (c - 1) / AL_W] >> (2 * ((c - 1) % AL_W))) & 3u;
}

// the reference's do-while from the end cell (bq, bs); WRITE: the pairs go to oq / os back to front, the last one at L - 1
template <bool WRITE, class PT>
__device__ __forceinline__ u32 al_walk(const PT* P, u32 nstrips, u32 bq, u32 bs, const unsigned char* s_q, const unsigned char* s_sub,
                                       char* oq, char* os, u32 L) {
    u32 i = bq, c = bs, n = 0;
    u32 pred = al_pred(P, nstrips, i, c);
    do {
        char a = '_', b = '_';
        if (pred == 1) { --i; --c; a = (char)s_q[i]; b = (char)s_sub[c]; }
        else if (pred == 2) { --i; a = (char)s_q[i]; }
        else if (pred == 3) { --c; b = (char)s_sub[c]; }
        if (WRITE) { oq[L - 1 - n] = a; os[L - 1 - n] = b; }
        ++n;
        pred = al_pred(P, nstrips, i, c);
    } while (pred != 0);
    return n;
}

template <class PT>
__device__ __forceinline__ u32 al_trace(const unsigned char* s_q, u32 lq, const unsigned char* s_sub, u32 ls, short* s_bnd, PT* P,
                                        u32 nstrips, u32 lane, char* oq, char* os, u32 text_cap) {
    const u64 key = al_pass<true>(s_q, lq, s_sub, ls, s_bnd, P, nstrips, lane);
    wave_sync();                                                // the predecessors are in place for lane 0
    const u32 order = 0xFFFFFFFFu - (u32)key;
    const u32 bq = (order == 0 || order >= lq) ? lq : order;
    const u32 bs = order >= lq ? order - lq : ls;
    u32 L = 0;
    if (lane == 0) {
        L = al_walk<false>(P, nstrips, bq, bs, s_q, s_sub, oq, os, 0u);
        if (L <= text_cap) al_walk<true>(P, nstrips, bq, bs, s_q, s_sub, oq, os, L);     // (L <= lq + ls <= text_cap)
        else L = 0;
    }
    return __builtin_amdgcn_readfirstlane(L);
}

__global__ __launch_bounds__(64) void k_align(BatchDev b, AlArgs a) {
    __shared__ unsigned short s_pred[AL_LDS_WORDS];
    __shared__ unsigned char s_q[MCQ_ALIGN_MAX_QUERY];
    __shared__ unsigned char s_sub[MCQ_ALIGN_MAX_SUBJECT];
    __shared__ short s_bnd[MCQ_ALIGN_MAX_QUERY + 1];
    const u32 lane = threadIdx.x;
    for (u64 q = blockIdx.x; q < b.nq; q += gridDim.x) {
        const mcq_align_job job = a.jobs[q];
        int score = 0; u32 L = 0, rev = 0, st = 0;
        if (job.on) {
            const u64 sa = b.paired ? 2 * q : q;
            u64 o0, e0, o1 = 0, e1 = 0;
            seq_bounds(b.seq_off, b.ranges, sa, o0, e0);
            if (b.paired) seq_bounds(b.seq_off, b.ranges, sa + 1, o1, e1);
            const u64 l1 = e0 - o0, l2 = e1 - o1;
            if (l1 > a.max_query || l2 > a.max_query) st |= MCQ_ALIGN_QUERY_LONG;
            if (job.sub_len > a.max_subject) st |= MCQ_ALIGN_SUBJECT_LONG;
            if (st == 0) {
                const u32 lq = (u32)l1, lq2 = (u32)l2, ls = job.sub_len;
                char* oq = a.out_query + q * (u64)a.text_cap;
                char* os = a.out_subject + q * (u64)a.text_cap;
                for (u32 i = lane; i < ls; i += 64) s_sub[i] = (unsigned char)a.subjects[job.sub_off + i];
                wave_sync();
                // the two sums, as std::size_t: a negative score sign-extends.  s1f / s1r: mate 1's own scores, one of which is printed
                int s1f = 0, s1r = 0;
                u64 sum_f = 0, sum_r = 0;
                if (lq > 0 && ls > 0) {
                    al_stage_query(b.bases, o0, lq, false, s_q, lane);
                    s1f = al_key_score(al_pass<false>(s_q, lq, s_sub, ls, s_bnd, (unsigned short*)nullptr, 0u, lane));
                    wave_sync();
                    al_stage_query(b.bases, o0, lq, true, s_q, lane);
                    s1r = al_key_score(al_pass<false>(s_q, lq, s_sub, ls, s_bnd, (unsigned short*)nullptr, 0u, lane));
                    wave_sync();
                    sum_f = (u64)(long long)s1f; sum_r = (u64)(long long)s1r;
                }
                if (lq2 > 0 && ls > 0) {                        // (an empty second mate is not aligned; against an empty subject it scores 0)
                    al_stage_query(b.bases, o1, lq2, false, s_q, lane);
                    sum_f += (u64)(long long)al_key_score(al_pass<false>(s_q, lq2, s_sub, ls, s_bnd, (unsigned short*)nullptr, 0u, lane));
                    wave_sync();
                    al_stage_query(b.bases, o1, lq2, true, s_q, lane);
                    sum_r += (u64)(long long)al_key_score(al_pass<false>(s_q, lq2, s_sub, ls, s_bnd, (unsigned short*)nullptr, 0u, lane));
                    wave_sync();
                }
                rev = sum_f > sum_r ? 0u : 1u;
                score = rev ? s1r : s1f;
                if (lq == 0 || ls == 0) {                       // nothing to relax: the corner, score 0, predecessor none -> one pair of gaps
                    if (lane == 0) { oq[0] = '_'; os[0] = '_'; }
                    L = 1;
                } else {
                    al_stage_query(b.bases, o0, lq, rev != 0, s_q, lane);
                    const u32 nstrips = (ls + AL_W - 1) / AL_W;
                    if ((u64)lq * nstrips <= AL_LDS_WORDS) {
                        L = al_trace(s_q, lq, s_sub, ls, s_bnd, s_pred, nstrips, lane, oq, os, a.text_cap);
                    } else {                                    // lq <= max_query, ls <= max_subject: the host gave every wave max_query x strips(max_subject) words
                        unsigned short* P = a.scratch + (u64)blockIdx.x * a.scratch_words;
                        L = al_trace(s_q, lq, s_sub, ls, s_bnd, P, nstrips, lane, oq, os, a.text_cap);
                    }
                }
                wave_sync();
            }
        }
        if (lane == 0) {
            mcq_alignment r;
            r.score = score; r.length = L; r.reverse = rev; r.status = st;
            a.out[q] = r;
        }
        wave_sync();                                            // the next query stages into the same LDS
    }
}

}  // namespace

// workgroups of k_align a device holds at once (asked once per device)
static u32 al_resident_blocks(int device) {
    static std::atomic<u32> cached[64];
    const bool slot = device >= 0 && device < 64;
    if (slot) { const u32 c = cached[device].load(std::memory_order_relaxed); if (c) return c; }
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_align, 64, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 1;
    const u32 n = (u32)per_cu * (u32)cus;
    if (slot) cached[device].store(n, std::memory_order_relaxed);
    return n;
}

extern "C" int mcq_align(mcq_ws* ws, const mcq_batch* in, const char* subjects, const mcq_align_job* jobs,
                         uint32_t max_query, uint32_t max_subject, mcq_alignment* out,
                         char* out_query, char* out_subject, uint32_t text_cap, void* stream) {
    if (!ws || !in || !subjects || !jobs || !out || !out_query || !out_subject) return fail(MCQ_E_ARG, "null argument");
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "mcq_align takes device pointers (MCQ_DEVICE_PTRS)");
    if (in->flags & MCQ_BATCH_PACKED) return fail(MCQ_E_UNSUPPORTED, "mcq_align compares raw characters: a packed batch (MCQ_BATCH_PACKED) has lost their case");
    if (in->flags & ~(u32)(MCQ_DEVICE_PTRS | MCQ_BATCH_RANGES)) return fail(MCQ_E_ARG, "unknown batch flag");
    if (max_query > MCQ_ALIGN_MAX_QUERY) return fail(MCQ_E_ARG, "max_query exceeds MCQ_ALIGN_MAX_QUERY = " + std::to_string(MCQ_ALIGN_MAX_QUERY));
    if (max_subject > MCQ_ALIGN_MAX_SUBJECT) return fail(MCQ_E_ARG, "max_subject exceeds MCQ_ALIGN_MAX_SUBJECT = " + std::to_string(MCQ_ALIGN_MAX_SUBJECT));
    if (text_cap < 1 || (u64)text_cap < (u64)max_query + max_subject) return fail(MCQ_E_ARG, "text_cap must be at least max_query + max_subject and at least 1");
    HIPCHK(hipSetDevice(ws->device));
    BatchDev b;
    int rc = batch_dev(in, in->bases, in->seq_off, b);
    if (rc) return rc;
    if (b.nq > ws->max_queries) return fail(MCQ_E_ARG, "batch has more queries than the workspace allows");
    if (b.nq == 0) return MCQ_OK;
    if (!in->bases || !in->seq_off) return fail(MCQ_E_ARG, "null argument");
    AlArgs a;
    a.subjects = subjects; a.jobs = jobs; a.max_query = max_query; a.max_subject = max_subject; a.text_cap = text_cap;
    a.out = out; a.out_query = out_query; a.out_subject = out_subject; a.scratch = nullptr; a.scratch_words = 0;
    u32 grid = (u32)std::min<u64>(b.nq, al_resident_blocks(ws->device));
    const u64 words = (u64)max_query * ((max_subject + AL_W - 1) / AL_W);       // the largest predecessor matrix the bounds allow
    if (words > AL_LDS_WORDS) {
        // the scratch is made once, by the first call that needs any, at its full size: no later call allocates, whatever its bounds
        const u64 total = AL_SCRATCH_BUDGET / sizeof(unsigned short);
        static_assert((u64)MCQ_ALIGN_MAX_QUERY * (MCQ_ALIGN_MAX_SUBJECT / AL_W) <= AL_SCRATCH_BUDGET / sizeof(unsigned short), "the scratch holds the largest matrix");
        if (ws->align_scratch_words == 0) {
            HIPCHK(ws->align_scratch.alloc(total));
            ws->align_scratch_words = total;
        }
        grid = (u32)std::min<u64>(grid, ws->align_scratch_words / words);      // >= 1: words <= the largest matrix
        a.scratch = ws->align_scratch.get(); a.scratch_words = words;
    }
    hipLaunchKernelGGL(k_align, dim3(grid), dim3(64), 0, (hipStream_t)stream, b, a);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}
