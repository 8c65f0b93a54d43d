// mcq_all_hits.hip -- all hits of a read (mcq_all_hits_count, mcq_all_hits): the read's sorted match list (rows 1-8, what merge_sort
// returns at src/querying.h:88-106) run-length compressed: one entry per distinct (target, window) in ascending order with its
// multiplicity.  What the reference prints under -allhits (show_matches, src/printing.cpp:365-416).
//
// Two calls.  mcq_all_hits_count sketches and probes every query (one wavefront per query) and leaves the exclusive prefix sums of
// the queries' location counts in loc_off: a query's location count bounds its distinct entries, so [loc_off[q], loc_off[q + 1]) is
// its segment of the entry array.  mcq_all_hits sketches and probes again, checks every query's count against its segment BEFORE a
// word of it is stored, sorts the table's own location words (every form sorts like (target, window)) and expands them only on
// output.  The tiers, by the size T of the segment:
//   T <= MCQ_ALL_HITS_REG_MAX    one wavefront; the words sit in LDS and are sorted in registers, one per lane
//   T <= MCQ_ALL_HITS_WAVE_MAX   one wavefront; sorted in LDS
//   T <= max_locs_per_query      a workgroup of four wavefronts (a launch of its own that skips every other query); the words are
//                                gathered into the END of the query's own segment (an entry has 12 bytes, a word 4 or 8) and sorted
//                                there; the entries are then written from the front of the segment, 256 words at a time, each chunk
//                                read whole before its entries are stored -- after J of T words at most J entries exist, and
//                                12 J <= (12 - w) T + w J for J <= T, so no entry reaches a word that is still to be read.
// A query is answered by exactly one of the two launches, which also writes its n_hits and status.  The sort is a bitonic network whose
// comparators all point the same way (a flip stage, then half-cleaners), so a list of any length is sorted as if padded with the
// largest word and no padding is stored.  It and the run-length pass are private to this unit; geometry, sketch and probe are the
// shared device functions.
#include "mcq_internal.hpp"

namespace {

constexpr u32 AH_REG_MAX = MCQ_ALL_HITS_REG_MAX;
constexpr u32 AH_WAVE_MAX = MCQ_ALL_HITS_WAVE_MAX;
constexpr u32 AH_WALK_MAX = 32;                       // longer lists are copied by the whole wave
constexpr u32 AH_BLOCK_WAVES = 4;
static_assert(AH_REG_MAX == 64 && AH_WAVE_MAX >= 64, "the register tier is one word per lane");

struct AhArgs {
    const u64* loc_off;      // [nq + 1]
    u32* hits;               // [cap * 3]
    u64 cap;
    u32* n_hits;             // [nq]
    u32* status;             // [nq]
    u32 lmax;                // the workspace's max_locs_per_query
};

__device__ __forceinline__ u64 ah_bcast64(u64 v, u32 src_lane) {
    return ((u64)bcast((u32)(v >> 32), src_lane) << 32) | bcast((u32)v, src_lane);
}
__device__ __forceinline__ u32 ah_pow2ceil(u32 x) { return x <= 1 ? 1u : 1u << (32 - __builtin_clz(x - 1)); }

// Rows 1-7 of one read by the NW waves of a workgroup: wave `wave` takes every NW-th group of windows (as many windows as give at
// most 64 features), probes one feature per lane and adds the lists' lengths to *s_total, which also hands out the lists' places.
// With dst: a list that ends at or before `limit` is copied to its place (the order of the lists does not matter: they are sorted).
template <class KeyT, int BSH>
__device__ __forceinline__ void ah_rows(const DbDev& db, const BatchDev& b, u64 o0, u64 l1, u64 o1, u64 l2, u32 wave, u32 NW, u32 lane,
                                        u32* sk_tmp, u32* feat, unsigned long long* s_total, KeyT* dst, u64 limit) {
    const u32 nw1 = num_windows(l1, db.winlen, db.winstride), nw2 = b.paired ? num_windows(l2, db.winlen, db.winstride) : 0;
    const u32 nw = nw1 + nw2;
    const u32 per = db.s < 64 ? 64 / db.s : 1;
    const u32 ngroups = (nw + per - 1) / per;
    const KeyT* __restrict__ L = reinterpret_cast<const KeyT*>(db.locs);
    for (u32 g = wave; g < ngroups; g += NW) {
        const u32 w0 = g * per, w1 = w0 + per < nw ? w0 + per : nw;
        u32 nfeat = 0;
        for (u32 w = w0; w < w1; ++w) {
            const bool m2 = w >= nw1;
            u64 beg; u32 wl;
            window_of(m2 ? l2 : l1, db.winlen, db.winstride, m2 ? w - nw1 : w, beg, wl);
            nfeat += wave_sketch_b(b, (m2 ? o1 : o0) + beg, wl, db.k, db.s, lane, sk_tmp, feat + nfeat);
        }
        const u32 f = lane < nfeat ? feat[lane] : MCQ_EMPTY;
        u64 off; u32 len;
        probe<BSH>(db, f, off, len);
        const u32 incl = wave_incl_scan_dpp(len);
        const u32 total = bcast(incl, 63);
        wave_sync();                                    // feat[] is consumed
        if (total == 0) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(s_total, (unsigned long long)total);
        base = ah_bcast64(base, 0);
        if (!dst) continue;
        const u64 pos = base + (incl - len);
        const bool fits = len > 0 && pos + len <= limit;
        if (fits && len <= AH_WALK_MAX)
            for (u32 i = 0; i < len; ++i) dst[pos + i] = L[off + i];
        u64 m = __ballot(fits && len > AH_WALK_MAX);
        while (m) {
            const u32 src = (u32)__builtin_ctzll(m);
            m &= m - 1;
            const u64 o = ah_bcast64(off, src), p = ah_bcast64(pos, src);
            const u32 n = bcast(len, src);
            for (u32 i = lane; i < n; i += 64) dst[p + i] = L[o + i];
        }
    }
}

// buf[0, n) ascending, any n, by G threads.  Level k merges sorted blocks of k / 2: the flip stage pairs i with its mirror image in
// the block of k, the stages behind it are half-cleaners.  Every comparator puts the smaller word at the smaller index, so words
// behind n that were the largest would never move: their comparators are left out.
template <class KeyT, class Sync>
__device__ __forceinline__ void ah_sort(KeyT* buf, u32 n, u32 tid, u32 G, Sync sync) {
    const u32 np = ah_pow2ceil(n);
    for (u32 k = 2; k <= np; k <<= 1) {
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (u32 t = tid; t < (np >> 1); t += G) {
                const u32 i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const u32 l = flip ? (i ^ (k - 1)) : (i | j);
                if (l < n) {
                    const KeyT x = buf[i], y = buf[l];
                    if (x > y) { buf[i] = y; buf[l] = x; }
                }
            }
            sync();
        }
    }
}

// Sorted words keys[0, T) -> one entry (tgt, win, hits) per run of equal words at out, by the NW waves of a workgroup; returns the
// number of entries.  A run's LAST word writes its entry: the entry's index is the number of run heads up to there, its count the
// distance to the last head.  A chunk of 64 NW words is read whole (with the word in front of it carried in a register) before one
// of its entries is stored, so out may be the memory the words lie in (see the file header).
template <class KeyT, u32 NW, class LF, class Sync>
__device__ __forceinline__ u32 ah_emit(const KeyT* keys, u32 T, u32* out, const LF& lf, u32 tid, u32* s_w, Sync sync) {
    constexpr u32 G = 64 * NW;
    const u32 lane = tid & 63, wave = tid >> 6;
    u32 n_out = 0, head_carry = 0;                      // head_carry: 1 + index of the last run head of the chunks so far
    KeyT last = 0;
    for (u32 base = 0; base < T; base += G) {
        const u32 j = base + tid;
        const bool in = j < T;
        const u32 e = (base + G < T ? base + G : T) - 1;
        const KeyT k = in ? keys[j] : (KeyT)0;
        const KeyT kp = (in && tid > 0) ? keys[j - 1] : last;
        const KeyT kn = (j + 1 < T) ? keys[j + 1] : (KeyT)0;
        const KeyT new_last = keys[e];
        const bool head = in && (j == 0 || k != kp);
        const bool tail = in && (j + 1 == T || k != kn);
        const u64 hm = __ballot(head);
        const u32 hrank = lane_rank(hm) + (head ? 1u : 0u);
        const u32 hpos = wave_incl_max_dpp(head ? j + 1 : 0u);
        u32 cnt_before = 0, max_before = 0, cnt_all = (u32)__builtin_popcountll(hm), max_all = bcast(hpos, 63);
        if constexpr (NW > 1) {
            if (lane == 0) { s_w[wave] = cnt_all; s_w[NW + wave] = max_all; }
            sync();
            cnt_all = 0; max_all = 0;
            for (u32 w = 0; w < NW; ++w) {
                const u32 c = s_w[w], m = s_w[NW + w];
                if (w < wave) { cnt_before += c; max_before = m > max_before ? m : max_before; }
                cnt_all += c; max_all = m > max_all ? m : max_all;
            }
        } else
            sync();
        if (tail) {
            u32 hp = hpos > max_before ? hpos : max_before;
            hp = hp > head_carry ? hp : head_carry;     // >= 1: word 0 is a head
            u32 t; KeyT tb;
            lf.locate(k, t, tb);
            u32* o = out + 3 * (u64)(n_out + cnt_before + hrank - 1);
            o[0] = t; o[1] = (u32)(k - tb); o[2] = j + 2 - hp;
        }
        n_out += cnt_all;
        head_carry = max_all > head_carry ? max_all : head_carry;
        last = new_last;
        sync();
    }
    return n_out;
}

// what one query's status is once its locations are counted
__device__ __forceinline__ u32 ah_status(bool too_long, u64 real, bool seg_ok, u64 T, u64 seg_end, const AhArgs& a) {
    u32 st = 0;
    if (too_long || real > a.lmax) st |= (u32)MCQ_ALL_HITS_LOCS;
    if (!too_long && (!seg_ok || real != T || (T > 0 && seg_end > a.cap))) st |= (u32)MCQ_ALL_HITS_SEGMENT;
    return st;
}

template <int BSH>
__global__ __launch_bounds__(64) void k_all_hits_count(DbDev db, BatchDev b, u64* cnt) {
    __shared__ u32 sk_tmp[64];
    __shared__ u32 feat[64];
    __shared__ unsigned long long s_total;
    const u32 lane = threadIdx.x;
    for (u64 q = blockIdx.x; q < b.nq; q += gridDim.x) {
        const u64 sa = b.paired ? 2 * q : q;
        u64 o0, e0, o1, e1;
        seq_bounds(b.seq_off, b.ranges, sa, o0, e0);
        if (b.paired) seq_bounds(b.seq_off, b.ranges, sa + 1, o1, e1); else { o1 = e0; e1 = e0; }
        const u64 l1 = e0 - o0, l2 = e1 - o1;
        if (lane == 0) s_total = 0;
        wave_sync();
        if (((l1 | l2) >> 31) == 0)
            ah_rows<u32, BSH>(db, b, o0, l1, o1, l2, 0, 1, lane, sk_tmp, feat, &s_total, nullptr, 0);
        wave_sync();
        if (lane == 0) cnt[q] = s_total;
        wave_sync();
    }
}

template <class KeyT, bool GW, int BSH>
__global__ __launch_bounds__(64) void k_all_hits_wave(DbDev db, BatchDev b, AhArgs a, GwDev gwd) {
    __shared__ KeyT keys[AH_WAVE_MAX];
    __shared__ u32 sk_tmp[64];
    __shared__ u32 feat[64];
    __shared__ unsigned long long s_total;
    const u32 lane = threadIdx.x;
    const auto lf = loc_format<KeyT, GW>(db, gwd);
    for (u64 q = blockIdx.x; q < b.nq; q += gridDim.x) {
        const u64 sb = a.loc_off[q], se = a.loc_off[q + 1];
        const bool seg_ok = se >= sb;
        const u64 T64 = seg_ok ? se - sb : 0;
        if (T64 > AH_WAVE_MAX) continue;                // k_all_hits_block's
        const u64 sa = b.paired ? 2 * q : q;
        u64 o0, e0, o1, e1;
        seq_bounds(b.seq_off, b.ranges, sa, o0, e0);
        if (b.paired) seq_bounds(b.seq_off, b.ranges, sa + 1, o1, e1); else { o1 = e0; e1 = e0; }
        const u64 l1 = e0 - o0, l2 = e1 - o1;
        const bool too_long = ((l1 | l2) >> 31) != 0;
        if (lane == 0) s_total = 0;
        wave_sync();
        if (!too_long) ah_rows<KeyT, BSH>(db, b, o0, l1, o1, l2, 0, 1, lane, sk_tmp, feat, &s_total, keys, T64);
        wave_sync();
        const u32 st = ah_status(too_long, s_total, seg_ok, T64, se, a);
        u32 n = 0;
        if (st == 0 && T64 > 0) {
            const u32 T = (u32)T64;
            if (T <= AH_REG_MAX) {
                KeyT r[1];
                r[0] = lane < T ? keys[lane] : ~(KeyT)0;
                wave_regsort<KeyT, 1>(r, lane);
                keys[lane] = r[0];
                wave_sync();
            } else
                ah_sort(keys, T, lane, 64u, [] { wave_sync(); });
            n = ah_emit<KeyT, 1>(keys, T, a.hits + 3 * sb, lf, lane, nullptr, [] { wave_sync(); });
        }
        if (lane == 0) { a.n_hits[q] = n; a.status[q] = st; }
        wave_sync();                                    // the next query writes keys[] and s_total
    }
}

template <class KeyT, bool GW, int BSH>
__global__ __launch_bounds__(64 * AH_BLOCK_WAVES) void k_all_hits_block(DbDev db, BatchDev b, AhArgs a, GwDev gwd) {
    __shared__ u32 sk_tmp[AH_BLOCK_WAVES][64];
    __shared__ u32 feat[AH_BLOCK_WAVES][64];
    __shared__ u32 s_w[2 * AH_BLOCK_WAVES];
    __shared__ unsigned long long s_total;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto lf = loc_format<KeyT, GW>(db, gwd);
    for (u64 q = blockIdx.x; q < b.nq; q += gridDim.x) {
        const u64 sb = a.loc_off[q], se = a.loc_off[q + 1];
        if (se < sb || se - sb <= AH_WAVE_MAX) continue;            // k_all_hits_wave's
        const u64 T64 = se - sb;
        const u64 sa = b.paired ? 2 * q : q;
        u64 o0, e0, o1, e1;
        seq_bounds(b.seq_off, b.ranges, sa, o0, e0);
        if (b.paired) seq_bounds(b.seq_off, b.ranges, sa + 1, o1, e1); else { o1 = e0; e1 = e0; }
        const u64 l1 = e0 - o0, l2 = e1 - o1;
        const bool too_long = ((l1 | l2) >> 31) != 0;
        // ---- count first: nothing is stored into a segment that is not this query's location count
        if (tid == 0) s_total = 0;
        __syncthreads();
        if (!too_long) ah_rows<KeyT, BSH>(db, b, o0, l1, o1, l2, wave, AH_BLOCK_WAVES, lane, sk_tmp[wave], feat[wave], &s_total, nullptr, 0);
        __syncthreads();
        const u32 st = ah_status(too_long, s_total, true, T64, se, a);
        u32 n = 0;
        if (st == 0) {                                  // (workgroup-uniform)
            const u32 T = (u32)T64;                     // <= lmax <= 2^30
            u32* seg = a.hits + 3 * sb;
            // the words at the end of the segment, rounded down to a word's alignment (entries are 4-byte aligned)
            const uintptr_t kaddr = ((uintptr_t)seg + (12 - sizeof(KeyT)) * T64) & ~(uintptr_t)(sizeof(KeyT) - 1);
            KeyT* keys = reinterpret_cast<KeyT*>(kaddr);
            __syncthreads();
            if (tid == 0) s_total = 0;
            __syncthreads();
            ah_rows<KeyT, BSH>(db, b, o0, l1, o1, l2, wave, AH_BLOCK_WAVES, lane, sk_tmp[wave], feat[wave], &s_total, keys, T64);
            __syncthreads();
            ah_sort(keys, T, tid, 64u * AH_BLOCK_WAVES, [] { __syncthreads(); });
            n = ah_emit<KeyT, AH_BLOCK_WAVES>(keys, T, seg, lf, tid, s_w, [] { __syncthreads(); });
        }
        if (tid == 0) { a.n_hits[q] = n; a.status[q] = st; }
        __syncthreads();
    }
}

// workgroups of `kern` a device holds at once
template <class K>
u32 ah_resident_blocks(K kern, int threads, int device) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 1;
    return (u32)per_cu * (u32)cus;
}

int ah_batch(const char* who, const mcq_db* db, const mcq_ws* ws, const mcq_batch* in, BatchDev& b) {
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, std::string(who) + " takes device pointers (MCQ_DEVICE_PTRS)");
    if (in->flags & ~(u32)(MCQ_DEVICE_PTRS | MCQ_BATCH_RANGES | MCQ_BATCH_PACKED)) return fail(MCQ_E_ARG, "unknown batch flag");
    if (db->device != ws->device) return fail(MCQ_E_ARG, "workspace and table live on different devices");
    HIPCHK(hipSetDevice(db->device));
    int rc = batch_dev(in, in->bases, in->seq_off, b);
    if (rc) return rc;
    if (b.nq > ws->max_queries) return fail(MCQ_E_ARG, "batch has more queries than the workspace allows");
    return MCQ_OK;
}

}  // namespace

extern "C" int mcq_all_hits_count(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, uint64_t* loc_off, void* stream) {
    if (!db || !ws || !in || !loc_off) return fail(MCQ_E_ARG, "null argument");
    BatchDev b;
    int rc = ah_batch("mcq_all_hits_count", db, ws, in, b);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (b.nq == 0) { HIPCHK(hipMemsetAsync(loc_off, 0, sizeof(u64), st)); return MCQ_OK; }
    const DbDev d = db->d;
    const int device = db->device;
    with_layout(db, [&](auto bsh) {
        auto kern = k_all_hits_count<decltype(bsh)::value>;
        const u32 grid = (u32)std::min<u64>(b.nq, ah_resident_blocks(kern, 64, device));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, st, d, b, loc_off);
        return 0;
    });
    HIPCHK(hipGetLastError());
    // in place: every count is read by the thread that then writes its sum
    rc = device_exclusive_scan<u64>(loc_off, loc_off, b.nq, st, 256);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_all_hits(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const uint64_t* loc_off, mcq_hit* hits, uint64_t cap,
                            uint32_t* n_hits, uint32_t* status, void* stream) {
    if (!db || !ws || !in || !loc_off || !hits || !n_hits || !status) return fail(MCQ_E_ARG, "null argument");
    if ((uintptr_t)hits & 3u) return fail(MCQ_E_ARG, "hits must be 4-byte aligned");
    BatchDev b;
    int rc = ah_batch("mcq_all_hits", db, ws, in, b);
    if (rc) return rc;
    if (b.nq == 0) return MCQ_OK;
    AhArgs a;
    a.loc_off = loc_off; a.hits = reinterpret_cast<u32*>(hits); a.cap = cap; a.n_hits = n_hits; a.status = status; a.lmax = ws->sc.lmax;
    hipStream_t st = (hipStream_t)stream;
    const DbDev d = db->d; const GwDev g = db->g;
    const int device = db->device;
    with_loc_form(db, [&](auto lf) {
        using LF = decltype(lf);
        with_layout(db, [&](auto bsh) {
            auto kw = k_all_hits_wave<typename LF::Key, LF::gw, decltype(bsh)::value>;
            auto kb = k_all_hits_block<typename LF::Key, LF::gw, decltype(bsh)::value>;
            const u32 gw_ = (u32)std::min<u64>(b.nq, ah_resident_blocks(kw, 64, device));
            const u32 gb_ = (u32)std::min<u64>(b.nq, ah_resident_blocks(kb, 64 * AH_BLOCK_WAVES, device));
            hipLaunchKernelGGL(kw, dim3(gw_), dim3(64), 0, st, d, b, a, g);
            hipLaunchKernelGGL(kb, dim3(gb_), dim3(64 * AH_BLOCK_WAVES), 0, st, d, b, a, g);
            return 0;
        });
        return 0;
    });
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}
