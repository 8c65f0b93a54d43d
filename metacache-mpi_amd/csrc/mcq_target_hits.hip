// mcq_target_hits.hip -- per-target window hit lists of a batch (mcq_target_hits, mcq_target_slots): what the reference's
// matches_per_target::insert keeps of a read (src/matches_per_target.h:111-155) for the targets the caller names.
//
// The query kernels hold a read's match list in registers and LDS and give out candidates only; after a fold even the window
// range of a candidate is (0,0).  This unit answers, for up to MCQ_TARGET_HITS_MAX_SLOTS targets per query, the question the
// table of -hits-per-seq asks: the read's per-target candidate on that target (for_all_contiguous_window_ranges,
// src/candidates.h:118-180 -- the first strictly best contiguous range of at most numWindows windows) and the number of the
// read's matches on every window of that range.
//
// One wavefront per query, grid-stride.  Rows 1-6 as in the query kernels and with their device functions (the read is sketched
// window by window, any number of windows; one table probe per lane).  Row 7 differs: a location is kept only when its target is one
// of the query's slot targets.  A target owns one interval of location words in every location form -- [tgt << wb, +2^wb) for the bit
// fields, [gw_off[tgt], gw_off[tgt + 1]) for the global-window index -- so the test is two compares of the word against a row of LDS,
// made per location before anything is stored, and it needs no target lookup (LocGW::locate) at all.  Lists are sorted like
// (target, window): a list of more than TH_WALK_MAX locations is not walked but searched for every slot's interval.
// What survives goes into a table of distinct (slot, window) keys in LDS whose multiplicities are the per-window counts; the distinct
// keys are sorted (in registers up to 64 of them, else a bitonic network over the table's words), their multiplicities summed up
// front to back, and the best range of a slot is then a closed form per right end: S(j) = P[j] - P[l(j) - 1], l(j) the first key of
// the slot not more than numWindows - 1 windows left of key j; the first j with the largest S(j) is the reference's candidate.
// All three location forms and both bucket layouts take this one path.  The distinct-key table, the register sort of 32-bit words and
// the weighted sweep of the query kernels are private to their unit and built around the top lists they feed; this kernel emits ranges
// and windows instead and has its own, smaller forms of the three.
#include "mcq_internal.hpp"

#include <atomic>

namespace {

constexpr u32 TH_KEYS = MCQ_TARGET_HITS_MAX_KEYS;
constexpr u32 TH_HT = 2 * TH_KEYS;                     // words of the distinct-key table: load factor <= 1/2 (+ 63 keys, see th_insert)
constexpr u32 TH_HT_SMALL = 256;                      // ... of a read that can have at most 128 keys (one group of features, few locations)
constexpr u32 TH_WIN_BITS = 28;                       // key = slot << 28 | window inside the target
constexpr u32 TH_WALK_MAX = 16;                       // longer lists are searched per slot instead of walked
constexpr unsigned long long TH_EMPTY = ~0ull;
static_assert((TH_HT & (TH_HT - 1)) == 0 && TH_HT > TH_KEYS + 64, "the table holds MCQ_TARGET_HITS_MAX_KEYS keys and one more wave of inserts");

struct ThArgs {
    const u32* targets;      // [nq * n_slots]
    u32 n_slots;
    u32 range_cap;
    u64 insert_size_max;
    u32* ranges;             // [nq * n_slots * 4]
    u32* counts;             // [nq * n_slots * range_cap]
    u32* status;             // [nq]
};

// one location that lies on slot `slot`, window `win` of its target: count it in the distinct-key table
__device__ __forceinline__ void th_insert(unsigned long long* tab, u32 ht_mask, u32* s_nd, u32* s_flags, u32 slot, u64 win) {
    if (win >> TH_WIN_BITS) { atomicOr(s_flags, (u32)MCQ_TARGET_HITS_WINDOW); return; }
    const u32 key = (slot << TH_WIN_BITS) | (u32)win;
    u32 i = ((key * 0x9E3779B1u) >> 12) & ht_mask;
    for (u32 n = 0; n <= ht_mask; ++n) {
        unsigned long long e = ((volatile unsigned long long*)tab)[i];
        if (e == TH_EMPTY) {
            // (lanes that pass this test together may take the table to TH_KEYS + 63 keys: it has room for them, and the caller
            // reports every query that ends above TH_KEYS, so the outcome does not depend on the interleaving)
            if (*(volatile u32*)s_nd >= TH_KEYS) { atomicOr(s_flags, (u32)MCQ_TARGET_HITS_KEYS); return; }
            const unsigned long long old = atomicCAS(&tab[i], TH_EMPTY, ((unsigned long long)key << 32) | 1ull);
            if (old == TH_EMPTY) { atomicAdd(s_nd, 1u); return; }
            e = old;
        }
        if ((u32)(e >> 32) == key) { atomicAdd(&tab[i], 1ull); return; }      // (a read has fewer than 2^32 locations: the count stays in its half)
        i = (i + 1) & ht_mask;
    }
    atomicOr(s_flags, (u32)MCQ_TARGET_HITS_KEYS);
}

// first index in [a, e) whose key (upper half of the table word) is >= key; e if there is none
__device__ __forceinline__ u32 th_lower_bound(const unsigned long long* tab, u32 a, u32 e, u64 key) {
    while (a < e) {
        const u32 mid = (a + e) >> 1;
        if ((tab[mid] >> 32) < key) a = mid + 1; else e = mid;
    }
    return a;
}

// one list: keep the locations that lie on a slot target
template <class KeyT>
__device__ __forceinline__ void th_walk(const DbDev& db, u64 off, u32 len, u32 n_slots, const u64* s_lo, const u64* s_hi,
                                        unsigned long long* tab, u32 ht_mask, u32* s_nd, u32* s_flags) {
    const KeyT* __restrict__ L = reinterpret_cast<const KeyT*>(db.locs) + off;
    if (len <= TH_WALK_MAX) {
        for (u32 i = 0; i < len; ++i) {
            const u64 wd = L[i];
            for (u32 s = 0; s < n_slots; ++s) {
                const u64 lo = s_lo[s], hi = s_hi[s];
                if (wd >= lo && wd <= hi) th_insert(tab, ht_mask, s_nd, s_flags, s, wd - lo);
            }
        }
    } else {
        for (u32 s = 0; s < n_slots; ++s) {
            const u64 lo = s_lo[s], hi = s_hi[s];
            if (lo > hi) continue;
            u32 a = 0, e = len;
            while (a < e) {
                const u32 mid = (a + e) >> 1;
                if ((u64)L[mid] < lo) a = mid + 1; else e = mid;
            }
            for (; a < len; ++a) {
                const u64 wd = L[a];
                if (wd > hi) break;
                th_insert(tab, ht_mask, s_nd, s_flags, s, wd - lo);
            }
        }
    }
}

template <class KeyT, bool GW, int BSH>
__global__ __launch_bounds__(64) void k_target_hits(DbDev db, BatchDev b, ThArgs a, CountersDev* ctr, GwDev gwd) {
    __shared__ unsigned long long tab[TH_HT];
    __shared__ u32 sk_tmp[64];
    __shared__ u32 feat[64];
    __shared__ u64 s_lo[MCQ_TARGET_HITS_MAX_SLOTS], s_hi[MCQ_TARGET_HITS_MAX_SLOTS];
    __shared__ u32 s_nd, s_flags;
    const u32 lane = threadIdx.x;
    const u32 n_slots = a.n_slots;
    for (u64 q = blockIdx.x; q < b.nq; q += gridDim.x) {
        // ---- the read and its slots
        const u64 sa = b.paired ? 2 * q : q;
        u64 o0, e0, o1, e1;
        seq_bounds(b.seq_off, b.ranges, sa, o0, e0);
        if (b.paired) seq_bounds(b.seq_off, b.ranges, sa + 1, o1, e1); else { o1 = e0; e1 = e0; }
        const u64 l1 = e0 - o0, l2 = e1 - o1;
        const u32 numWindows = range_width(l1 + l2, a.insert_size_max, db.tgt_winstride, db.magic_tgt_stride);
        const u32 my_tgt = lane < n_slots ? a.targets[q * n_slots + lane] : MCQ_EMPTY;
        u64 lo = 1, hi = 0;                                 // an empty interval: unused slot, or no such target
        if (my_tgt != MCQ_EMPTY && my_tgt < db.n_targets) {
            if constexpr (GW) {
                const u32 w0 = gwd.off[my_tgt], w1 = gwd.off[my_tgt + 1];
                if (w1 > w0) { lo = w0; hi = w1 - 1; }
            } else {
                lo = (u64)my_tgt << db.wb; hi = lo | ((1ull << db.wb) - 1);
            }
        }
        if (lane < MCQ_TARGET_HITS_MAX_SLOTS) { s_lo[lane] = lo; s_hi[lane] = hi; }
        if (lane == 0) { s_nd = 0; s_flags = 0; }
        const bool any_slot = __ballot(lo <= hi) != 0;
        u32 st = 0;
        if (numWindows > a.range_cap) st |= MCQ_TARGET_HITS_RANGE;
        if (((l1 | l2) >> 31) != 0) st |= MCQ_TARGET_HITS_WINDOW;
        wave_sync();
        u32 D = 0;
        if (st == 0 && any_slot) {
            // ---- rows 1-7: sketch window by window, probe a group of up to 64 features at a time, keep the slot targets' locations
            const u32 nw1 = num_windows(l1, db.winlen, db.winstride), nw2 = b.paired ? num_windows(l2, db.winlen, db.winstride) : 0;
            const u32 nw = nw1 + nw2;
            const bool single = (u64)nw * db.s <= 64;       // one group: the table is sized once its locations are counted
            u32 ht_mask = TH_HT - 1;
            if (!single) {
                for (u32 i = lane; i < TH_HT; i += 64) tab[i] = TH_EMPTY;
                wave_sync();
            }
            u32 nfeat = 0;
            for (u32 w = 0; w < nw; ++w) {
                const bool m2 = w >= nw1;
                u64 beg; u32 wl;
                window_of(m2 ? l2 : l1, db.winlen, db.winstride, m2 ? w - nw1 : w, beg, wl);
                nfeat += wave_sketch_b(b, (m2 ? o1 : o0) + beg, wl, db.k, db.s, lane, sk_tmp, feat + nfeat);
                if (nfeat + db.s <= 64 && w + 1 < nw) continue;
                const u32 f = lane < nfeat ? feat[lane] : MCQ_EMPTY;
                u64 off; u32 len;
                probe<BSH>(db, f, off, len);
                if (single) {
                    const u32 T = bcast(wave_incl_scan_dpp(len), 63);
                    if ((u64)T * n_slots <= TH_HT_SMALL / 2) ht_mask = TH_HT_SMALL - 1;
                    for (u32 i = lane; i <= ht_mask; i += 64) tab[i] = TH_EMPTY;
                }
                wave_sync();                                // feat[] is consumed, the table is clear
                th_walk<KeyT>(db, off, len, n_slots, s_lo, s_hi, tab, ht_mask, &s_nd, &s_flags);
                wave_sync();
                nfeat = 0;
            }
            st |= s_flags;
            D = s_nd;
            if (D > TH_KEYS) st |= MCQ_TARGET_HITS_KEYS;
            if (st == 0 && D > 0) {
                // ---- the distinct keys to the front (in place: writes trail reads), sorted, their counts summed front to back
                u32 nd = 0;
                for (u32 base = 0; base <= ht_mask; base += 64) {
                    const unsigned long long e = tab[base + lane];
                    const u64 m = __ballot(e != TH_EMPTY);
                    wave_sync();
                    if (e != TH_EMPTY) tab[nd + lane_rank(m)] = e;
                    nd += (u32)__builtin_popcountll(m);
                    wave_sync();
                }
                D = nd;
                if (D <= 64) {
                    u64 r[1];
                    r[0] = lane < D ? (u64)tab[lane] : ~0ull;
                    wave_regsort<u64, 1>(r, lane);
                    tab[lane] = r[0];
                } else {
                    const u32 n2 = 1u << (32 - __builtin_clz(D - 1));      // 64 < D <= TH_KEYS: n2 <= TH_HT
                    for (u32 i = D + lane; i < n2; i += 64) tab[i] = TH_EMPTY;
                    wave_sync();
                    bitonic_sort(tab, n2, lane, 64u, [] { wave_sync(); });
                }
                wave_sync();
                u32 carry = 0;
                for (u32 base = 0; base < D; base += 64) {
                    const u32 j = base + lane;
                    const unsigned long long e = j < D ? tab[j] : 0ull;
                    const u32 incl = wave_incl_scan_dpp(j < D ? (u32)e : 0u) + carry;
                    if (j < D) tab[j] = (e & 0xFFFFFFFF00000000ull) | incl;
                    carry = bcast(incl, 63);
                }
                wave_sync();
            }
        }
        if (st != 0) D = 0;
        // ---- per slot: the best range and its windows
        for (u32 s = 0; s < n_slots; ++s) {
            const u32 tgt = a.targets[q * n_slots + s];
            u32* rg = a.ranges + (q * n_slots + s) * 4;
            u32 hits = 0, win_beg = 0, n_win = 0, lj = 0;
            if (D > 0 && tgt != MCQ_EMPTY) {
                const u64 k0 = (u64)s << TH_WIN_BITS;
                const u32 sb = th_lower_bound(tab, 0, D, k0), se = th_lower_bound(tab, sb, D, k0 + (1ull << TH_WIN_BITS));
                // S(j) for every right end j of the slot; the first j with the largest S(j) wins (strict > in the reference's loop)
                unsigned long long best = 0;
                for (u32 j = sb + lane; j < se; j += 64) {
                    const u64 key = tab[j] >> 32;
                    const u64 win = key - k0;
                    const u64 lowkey = win >= numWindows ? key - (numWindows - 1) : k0;
                    const u32 l = th_lower_bound(tab, sb, j, lowkey);
                    const u32 S = (u32)tab[j] - (l > 0 ? (u32)tab[l - 1] : 0u);
                    const unsigned long long c = ((unsigned long long)S << 32) | (0xFFFFFFFFu - j);
                    best = c > best ? c : best;
                }
                best = wave_max((u64)best);
                if (best != 0) {
                    const u32 j = 0xFFFFFFFFu - (u32)best;
                    const u64 key = tab[j] >> 32;
                    const u64 win = key - k0;
                    const u64 lowkey = win >= numWindows ? key - (numWindows - 1) : k0;
                    lj = th_lower_bound(tab, sb, j, lowkey);
                    hits = (u32)(best >> 32);
                    win_beg = (u32)((tab[lj] >> 32) - k0);
                    n_win = (u32)win - win_beg + 1;                  // <= numWindows <= range_cap
                    // every window of the range: its key's multiplicity, 0 where the read has no match
                    u32* cn = a.counts + (q * n_slots + s) * (u64)a.range_cap;
                    for (u32 i = lane; i < n_win; i += 64) {
                        const u64 wk = k0 + win_beg + i;
                        const u32 p = th_lower_bound(tab, lj, j + 1, wk);
                        u32 c = 0;
                        if (p <= j && (tab[p] >> 32) == wk) c = (u32)tab[p] - (p > 0 ? (u32)tab[p - 1] : 0u);
                        cn[i] = c;
                    }
                }
            }
            if (lane == 0) { rg[0] = tgt; rg[1] = hits; rg[2] = win_beg; rg[3] = n_win; }
        }
        if (lane == 0) {
            a.status[q] = st;
            if (st != 0) atomicAdd(&ctr->err_count, 1u);
        }
        wave_sync();                                        // the next query clears the table and the slot rows
    }
}

// slot targets of a batch from its device results: the sequence-level candidates with hits >= hits_min, in list order
__global__ void k_target_slots(const u32* __restrict__ cands, const u32* __restrict__ ncand, u64 nq, u32 max_cand, u32 hits_min,
                               const u32* __restrict__ tax2tgt, u32 n_taxa, u32* __restrict__ targets, u32 n_slots) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const u32 n = ncand[q] < max_cand ? ncand[q] : max_cand;
    u32 used = 0;
    for (u32 i = 0; i < n && used < n_slots; ++i) {
        const u32 tax = cands[(q * max_cand + i) * 4], hits = cands[(q * max_cand + i) * 4 + 1];
        if (!(tax & 0x80000000u) || tax == MCQ_EMPTY || hits < hits_min) continue;
        const u32 idx = tax & 0x7FFFFFFFu;
        const u32 tgt = idx < n_taxa ? tax2tgt[idx] : MCQ_EMPTY;
        if (tgt != MCQ_EMPTY) targets[q * n_slots + used++] = tgt;
    }
    for (; used < n_slots; ++used) targets[q * n_slots + used] = MCQ_EMPTY;
}

// workgroups of k_target_hits<KeyT, GW, BSH> a device holds at once: asked once per instantiation and device, as the other launch
// paths size their grids when the workspace is made
template <class KeyT, bool GW, int BSH>
u32 th_resident_blocks(int device) {
    static std::atomic<u32> cached[64];
    const bool slot = device >= 0 && device < 64;
    if (slot) { const u32 c = cached[device].load(std::memory_order_relaxed); if (c) return c; }
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_target_hits<KeyT, GW, BSH>, 64, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 1;
    const u32 n = (u32)per_cu * (u32)cus;
    if (slot) cached[device].store(n, std::memory_order_relaxed);
    return n;
}

}  // namespace

extern "C" uint32_t mcq_target_hits_range_cap(const mcq_db* db, uint64_t longest_query, uint64_t insert_size_max) {
    if (!db) return 0;
    const u64 m = longest_query > insert_size_max ? longest_query : insert_size_max;
    return (u32)(2 + m / db->d.tgt_winstride);          // Geom::range_width (src/classification.cpp:217-219)
}

extern "C" int mcq_target_hits(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const uint32_t* targets, uint32_t n_slots,
                               uint64_t insert_size_max, uint32_t range_cap, mcq_target_range* out_ranges, uint32_t* out_counts,
                               uint32_t* status, void* stream) {
    if (!db || !ws || !in || !targets || !out_ranges || !out_counts || !status) return fail(MCQ_E_ARG, "null argument");
    if (n_slots < 1 || n_slots > MCQ_TARGET_HITS_MAX_SLOTS) return fail(MCQ_E_ARG, "n_slots must be 1.." + std::to_string(MCQ_TARGET_HITS_MAX_SLOTS));
    if (range_cap < 1) return fail(MCQ_E_ARG, "range_cap must be at least 1");
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "mcq_target_hits takes device pointers (MCQ_DEVICE_PTRS)");
    if (in->flags & ~(u32)(MCQ_DEVICE_PTRS | MCQ_BATCH_RANGES | MCQ_BATCH_PACKED)) return fail(MCQ_E_ARG, "unknown batch flag");
    if (db->device != ws->device) return fail(MCQ_E_ARG, "workspace and table live on different devices");
    HIPCHK(hipSetDevice(db->device));
    BatchDev b;
    int rc = batch_dev(in, in->bases, in->seq_off, b);
    if (rc) return rc;
    if (b.nq > ws->max_queries) return fail(MCQ_E_ARG, "batch has more queries than the workspace allows");
    if (b.nq == 0) return MCQ_OK;
    ThArgs a;
    a.targets = targets; a.n_slots = n_slots; a.range_cap = range_cap; a.insert_size_max = insert_size_max;
    a.ranges = reinterpret_cast<u32*>(out_ranges); a.counts = out_counts; a.status = status;
    hipStream_t st = (hipStream_t)stream;
    const DbDev d = db->d; const GwDev g = db->g; CountersDev* ctr = ws->ctr.get();
    const int device = db->device;
    with_loc_form(db, [&](auto lf) {
        using LF = decltype(lf);
        with_layout(db, [&](auto bsh) {
            auto kern = k_target_hits<typename LF::Key, LF::gw, decltype(bsh)::value>;
            const u32 grid = (u32)std::min<u64>(b.nq, th_resident_blocks<typename LF::Key, LF::gw, decltype(bsh)::value>(device));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, st, d, b, a, ctr, g);
            return 0;
        });
        return 0;
    });
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_target_slots(const mcq_result* cands, uint64_t n_queries, uint32_t max_cand, uint32_t hits_min,
                                const uint32_t* tax2tgt, uint32_t n_taxa, uint32_t* targets, uint32_t n_slots, void* stream) {
    if (!cands || !cands->cands || !cands->n_cand || !tax2tgt || !targets) return fail(MCQ_E_ARG, "null argument");
    if (!(cands->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "mcq_target_slots takes device results (MCQ_DEVICE_PTRS)");
    if (n_slots < 1 || n_slots > MCQ_TARGET_HITS_MAX_SLOTS || max_cand < 1) return fail(MCQ_E_ARG, "n_slots must be 1..16, max_cand at least 1");
    if (n_queries == 0) return MCQ_OK;
    hipLaunchKernelGGL(k_target_slots, dim3((u32)((n_queries + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const u32*>(cands->cands), cands->n_cand, n_queries, max_cand, hits_min, tax2tgt, n_taxa, targets, n_slots);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}
