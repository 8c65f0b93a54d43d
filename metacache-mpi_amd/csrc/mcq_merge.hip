// mcq_merge.hip -- the reference's `merge` of query result files on the device (mcq_merge_*, include/mcq.h): what read_results
// (src/mode_merge.cpp:209-264) and best_distinct_matches_in_contiguous_window_ranges::insert (src/candidates.h:236-285) do token by
// token on one thread, for text that has the strict form, and classify() (src/classification.cpp:235-265) of the merged lists.
//
// The handle owns, per query, a candidate list (a count and max_cand (taxon index, hits) pairs, sorted by hits descending) and the
// reference of its header token (file ordinal, byte offset in that file, length), and one counter of items whose taxid the taxonomy
// does not have.  A mapping line `id \t|\t header \t|\t ... \t|\t taxid:hits,taxid:hits \t|\t ...` touches the list of query id alone:
// every item goes through the reference's insert in item order, so the lists are a function of the order of the lines per query --
// chunks of one file in file order and files in merge order on ONE stream give the reference's lists.
//
// THE STRICT FORM (what makes a parse line by line see the records the reference's token stream sees).  A chunk is strict when
// every line of it
//   - begins with '#' (a comment: skipped whatever it holds and however long it is), or
//   - is 1-18 decimal digits (the query id, 1 .. n_queries), then `\t|\t`, then the header column, whose first byte begins a
//     non-empty token that ends at the first blank (space, TAB, VT, FF, CR); then the columns up to `top_hits`, each ended by
//     `\t|\t`, with no '|' anywhere else in front of the top_hits column (tophits_column of them are passed in all); then the
//     top_hits column: empty, or items `taxid:hits` -- taxid 1-18 digits, hits 1-9 digits -- split by single ',', at most
//     MCQ_MERGE_MAX_ITEMS of them; then a TAB.  What follows that TAB is not looked at (a CR included);
//   - is at most MCQ_MERGE_MAX_LINE bytes long with its LF (the chunk's last line may lack the LF and then counts as if it had it);
// and no query id occurs twice in the chunk.  An empty line is not strict.
//
// A chunk (whole lines of one file, in device memory) goes through these launches on the caller's stream:
//   k_mg_count   newlines per 4 KiB tile (16-B loads), then an exclusive scan: the line index of every tile's first line
//   k_mg_parse   one workgroup per tile stages the tile and MCQ_MERGE_MAX_LINE bytes behind it in LDS with 16-B loads, numbers the
//                line starts of the tile (wave scan + carry, the pattern of k_am_parse), then one lane per line checks the form in
//                LDS and binary-searches every taxid in the sorted id array; the taxon is replaced by its ancestor at the merge
//                rank where it has one.  Per line it leaves the query, the header reference and the items in scratch; any
//                violation sets the chunk's status word.  Nothing of the handle's state is touched.
//   k_mg_claim   (only if the status word is clear) every line claims its query for this chunk; a second claim sets the status word
//   k_mg_apply   (only if still clear) the lane that owns a line runs the reference's insert over its items on the query's list
// The call waits for its stream twice: behind the scan, for the number of lines (it sizes the scratch of the lines, 28 B per line, and
// the grids of claim and apply; the items take 2 B of scratch per byte of text), and at its end, for the status word.  So two chunks
// never overlap on the device: a caller with two buffers overlaps only its reading of the next chunk with this call.
// Text at any address: a 16-B piece that is not aligned is two aligned 16-B loads and a shift (mg_load16).
// Stores are plain C++ and vector atomics.
#include "mcq_internal.hpp"
#include "mcq_classify_one.hpp"

namespace {

constexpr u32 MG_TILE = 4096;                          // bytes of text per workgroup
constexpr u32 MG_MAX_LINE = MCQ_MERGE_MAX_LINE;        // a strict line with its '\n' is no longer than this
constexpr u32 MG_LDS = MG_TILE + MG_MAX_LINE;          // a line that starts in the tile and is strict ends inside this
constexpr u32 MG_TILE_LINES = MG_TILE / 2 + 1;         // ("#\n") more line starts than this in a tile: some line is empty
constexpr u32 MG_NONE = 0xFFFFFFFFu;
constexpr u32 MG_MAX_CAND = 16;
constexpr u32 MG_RANKS = mcq::kClsNumRanks;
static_assert(MG_LDS % 16 == 0 && MG_TILE == 256 * 16 && MG_MAX_LINE <= 256 * 16, "one or two 16-B loads per thread cover tile and tail");

struct MgTax {
    const int64_t* id_sorted; const u32* id_taxon; u64 n_ids;       // taxid -> taxon index
    const u32* lineage; const uint8_t* rank; u32 n_taxa;
    u32 merge_below;                                                // 0: keep the taxon
};
// the lines of one call in scratch: line l names query q[l] (MG_NONE: a comment) and holds the items [item0[l], item0[l] + its count)
struct MgLines {
    u64 n_lines;                                                    // (chunk: its newlines, + 1 for a last line without one)
    u32* q; u64* item0; u32* cnt;                                   // cnt null: the count is item0[l + 1] - item0[l]
    u64* hdr_off; u32* hdr_len;
    u32* item_tax; u32* item_hits;
    u64 line_cap;
    u32* status;                                                    // != 0: not strict / an id twice
    u32 file_ordinal;
};
struct MgChunk {
    const char* text; u64 n;
    u64 n_tiles; const u64* tile_off;                               // [n_tiles + 1] newlines before each tile
    u64 chunk_offset;                                               // of the chunk's first byte in its file
    u64 n_queries; u32 tophits_column;
};
struct MgState {
    u32* cnt; uint2* pairs; u32 max_cand;                           // [n_queries], [n_queries * max_cand] (taxon, hits)
    u32* hdr_file; u64* hdr_off; u32* hdr_len;                      // [n_queries]; hdr_len 0 = none yet
    unsigned long long* unknown;                                    // items whose taxid the taxonomy does not have
    u32* claim; u32 epoch;                                          // [n_queries]: the last call that touched the query
};

// bit j = byte j of the 16 is '\n' (exact per-byte zero detection, as am_newlines of mcq_accmap.hip)
__device__ __forceinline__ u32 mg_newlines(const uint4 v) {
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u32 mask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32 m = w[i] ^ 0x0A0A0A0Au;
        const u32 z = ~(((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u;
        mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * i);
    }
    return mask;
}
// text[base .. base + 16), 0 behind the end of the chunk: one aligned 16-B load, or, where text + base is not aligned, the two aligned
// 16-B pieces it lies in and a shift.  A piece is loaded only if it holds a byte of the chunk, so every load stays in the chunk's pages.
__device__ __forceinline__ uint4 mg_load16(const char* __restrict__ text, u64 base, u64 n) {
    if (base >= n) return make_uint4(0, 0, 0, 0);
    const uintptr_t a = reinterpret_cast<uintptr_t>(text) + base;
    const u32 mis = (u32)(a & 15);
    const uint4* p = reinterpret_cast<const uint4*>(a - mis);
    const uint4 lo = p[0];
    u32 w[4] = {lo.x, lo.y, lo.z, lo.w};
    if (mis) {
        const uint4 hi = base + (16 - mis) < n ? p[1] : make_uint4(0, 0, 0, 0);
        const u32 v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const u32 k = mis >> 2, sh = (mis & 3) * 8;
#pragma unroll
        for (u32 i = 0; i < 4; ++i) {
            u32 x = 0, y = 0;
#pragma unroll
            for (u32 j = 0; j < 4; ++j) if (k == j) { x = v[i + j]; y = v[i + j + 1]; }   // (no indexed registers)
            w[i] = sh ? (x >> sh) | (y << (32 - sh)) : x;
        }
    }
    const u64 left = n - base;
    if (left < 16) {
#pragma unroll
        for (u32 i = 0; i < 4; ++i) {
            const u32 keep = left > 4 * i ? (u32)(left - 4 * i) : 0u;        // bytes of word i inside the chunk
            if (keep < 4) w[i] &= keep ? (1u << (8 * keep)) - 1u : 0u;
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(256) void k_mg_count(const char* text, u64 n, u64* tile_cnt) {
    __shared__ u32 s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * MG_TILE + (u64)threadIdx.x * 16;
    u32 c = base < n ? (u32)__builtin_popcount(mg_newlines(mg_load16(text, base, n))) : 0u;     // (the 0 fill is no newline)
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_c;
}

// taxon_with_id, then the ancestor at the merge rank if there is one (src/candidates.h:242-245); MG_NONE: no such taxid
__device__ __forceinline__ u32 mg_taxon(const MgTax& T, int64_t taxid) {
    u64 lo = 0, hi = T.n_ids;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (T.id_sorted[mid] < taxid) lo = mid + 1; else hi = mid; }
    if (lo >= T.n_ids || T.id_sorted[lo] != taxid) return MG_NONE;
    u32 t = T.id_taxon[lo];
    if (T.merge_below > 0) {
        const u32 a = T.lineage[(u64)t * MG_RANKS + T.merge_below];
        if (a != MG_NONE) t = a;
    }
    return t;
}

__device__ __forceinline__ bool mg_digit(unsigned char c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool mg_blank(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

__global__ __launch_bounds__(256) void k_mg_parse(MgTax T, MgChunk C, MgLines L) {
    __shared__ uint4 s_text4[MG_LDS / 16];
    __shared__ unsigned short s_start[MG_TILE_LINES + 1];
    __shared__ u32 s_w[4];
    unsigned char* s_text = reinterpret_cast<unsigned char*>(s_text4);
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 tile0 = (u64)blockIdx.x * MG_TILE;
    // the tile and what may hold the end of its last line, 16 B per load
    const uint4 mine = mg_load16(C.text, tile0 + (u64)tid * 16, C.n);
    s_text4[tid] = mine;
    if (tid < MG_MAX_LINE / 16) s_text4[256 + tid] = mg_load16(C.text, tile0 + MG_TILE + (u64)tid * 16, C.n);
    const bool tile_at_line_start = tile0 == 0 || C.text[tile0 - 1] == '\n';
    __syncthreads();
    // line starts among my 16 bytes: behind every newline, inside the chunk
    const u64 base = tile0 + (u64)tid * 16;
    const u32 nlm = mg_newlines(mine);
    const u32 valid = base >= C.n ? 0u : (C.n - base >= 16 ? 0xFFFFu : (1u << (u32)(C.n - base)) - 1u);
    const u32 prev = tid == 0 ? (u32)tile_at_line_start : (u32)(s_text[tid * 16 - 1] == '\n');
    const u32 lsm = ((nlm << 1) | prev) & valid;
    const u32 c = (u32)__builtin_popcount(lsm);
    const u32 incl = wave_incl_scan_dpp(c);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u32 woff = 0, total = 0;
    for (u32 w = 0; w < 4; ++w) { if (w < wave) woff += s_w[w]; total += s_w[w]; }
    if (total > MG_TILE_LINES) { if (tid == 0) *L.status = 1; return; }       // (uniform: an empty line among them)
    u32 at = woff + incl - c;
    for (u32 m = lsm; m; m &= m - 1) s_start[at++] = (unsigned short)(tid * 16 + (u32)__builtin_ctz(m));
    __syncthreads();
    const u64 line0 = C.tile_off[blockIdx.x] + (tile_at_line_start ? 0 : 1);  // index of the tile's first line start
    bool bad = false;
    for (u32 j = tid; j < total; j += 256) {
        const u32 p = s_start[j];
        const u64 li = line0 + j;
        if (li >= L.line_cap) { bad = true; continue; }
        const u64 left = C.n - (tile0 + p);                                   // (>= 1)
        const u32 scan = left < MG_MAX_LINE ? (u32)left : MG_MAX_LINE;
        const unsigned char* s = s_text + p;
        if (s[0] == '#') { L.q[li] = MG_NONE; continue; }
        u32 i = 0;
        u64 id = 0;
        while (i < scan && i < 18 && mg_digit(s[i])) { id = id * 10 + (u64)(s[i] - '0'); ++i; }
        bool ok = i > 0 && id >= 1 && id <= C.n_queries && i + 3 <= scan && s[i] == '\t' && s[i + 1] == '|' && s[i + 2] == '\t';
        if (!ok) { bad = true; continue; }
        i += 3;
        const u32 hbeg = i;
        while (i < scan && !mg_blank(s[i]) && s[i] != '|') ++i;
        const u32 hlen = i - hbeg;
        ok = hlen > 0;
        for (u32 pipes = 1; ok && pipes < C.tophits_column; ++pipes) {        // every further column ends in \t|\t
            const u32 col = i;                                                // (the header column: behind its token)
            while (i < scan && s[i] != '|' && s[i] != '\n') ++i;
            ok = i > col && i + 1 < scan && s[i] == '|' && s[i - 1] == '\t' && s[i + 1] == '\t';   // (its own TAB, not the last separator's)
            i += 2;
        }
        ok = ok && i < scan;
        // the top_hits column: item k of the line goes to slot item0 + k; items lie at least 4 bytes apart, so the slots of two lines
        // never meet and (n_bytes / 4 + 1) slots hold every item of the chunk
        const u64 item0 = (tile0 + p + i) >> 2;
        u32 n_items = 0;
        if (ok && s[i] == '\t') {
            ++i;
        } else {
            while (ok) {
                u32 d = 0;
                u64 taxid = 0;
                while (i < scan && d < 18 && mg_digit(s[i])) { taxid = taxid * 10 + (u64)(s[i] - '0'); ++i; ++d; }
                if (d == 0 || i >= scan || s[i] != ':') { ok = false; break; }
                ++i;
                u32 e = 0, hits = 0;
                while (i < scan && e < 9 && mg_digit(s[i])) { hits = hits * 10 + (u32)(s[i] - '0'); ++i; ++e; }
                if (e == 0 || i >= scan || (s[i] != ',' && s[i] != '\t') || n_items == MCQ_MERGE_MAX_ITEMS) { ok = false; break; }
                L.item_tax[item0 + n_items] = mg_taxon(T, (int64_t)taxid);
                L.item_hits[item0 + n_items] = hits;
                ++n_items;
                if (s[i++] == '\t') break;
            }
        }
        if (ok) {                                                             // the line's length with its LF
            while (i < scan && s[i] != '\n') ++i;
            ok = i < scan || left < MG_MAX_LINE;
        }
        if (!ok) { bad = true; continue; }
        L.q[li] = (u32)(id - 1);
        L.item0[li] = item0;
        L.cnt[li] = n_items;
        L.hdr_off[li] = C.chunk_offset + tile0 + p + hbeg;
        L.hdr_len[li] = hlen;
    }
    if (bad) *L.status = 1;
}

// the lines of mcq_merge_lines: taxid -> taxon for every item (in place of what k_mg_parse does while it reads)
__global__ __launch_bounds__(256) void k_mg_lookup(MgTax T, const int64_t* taxid, u32* item_tax, u64 n_items) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < n_items) item_tax[k] = mg_taxon(T, taxid[k]);
}

__device__ __forceinline__ u64 mg_n_lines(const MgLines& L) { return L.n_lines < L.line_cap ? L.n_lines : L.line_cap; }

__global__ __launch_bounds__(256) void k_mg_claim(MgLines L, MgState S) {
    if (*L.status) return;
    const u64 li = (u64)blockIdx.x * 256 + threadIdx.x;
    if (li >= mg_n_lines(L)) return;
    const u32 q = L.q[li];
    if (q != MG_NONE && atomicExch(&S.claim[q], S.epoch) == S.epoch) *L.status = 2;
}

// best_distinct_matches_in_contiguous_window_ranges::insert (src/candidates.h:236-285) on the list l[0 .. n) of capacity max_cand
__device__ __forceinline__ u32 mg_insert(uint2* l, u32 n, u32 max_cand, u32 tax, u32 hits, bool sequence_level) {
    if (!sequence_level) {                                        // above sequence level a taxon occurs once
        u32 i = 0;
        while (i < n && l[i].x != tax) ++i;
        if (i < n) {
            if (hits > l[i].y) {                                  // more hits: ahead of the smaller entries, behind the equal ones
                while (i > 0 && l[i - 1].y < hits) { l[i] = l[i - 1]; --i; }
                l[i] = make_uint2(tax, hits);
            }
            return n;
        }
    }
    u32 j = 0;                                                    // upper_bound by hits descending: behind equal hits
    while (j < n && l[j].y >= hits) ++j;
    if (j == n && n >= max_cand) return n;
    const u32 nn = n < max_cand ? n + 1 : max_cand;
    for (u32 k = nn - 1; k > j; --k) l[k] = l[k - 1];
    l[j] = make_uint2(tax, hits);
    return nn;
}

__global__ __launch_bounds__(256) void k_mg_apply(MgLines L, MgState S, const uint8_t* rank) {
    if (*L.status) return;
    const u64 li = (u64)blockIdx.x * 256 + threadIdx.x;
    if (li >= mg_n_lines(L)) return;
    const u32 q = L.q[li];
    if (q == MG_NONE) return;
    if (S.hdr_len[q] == 0 && L.hdr_len[li] != 0) { S.hdr_file[q] = L.file_ordinal; S.hdr_off[q] = L.hdr_off[li]; S.hdr_len[q] = L.hdr_len[li]; }
    const u64 item0 = L.item0[li];
    const u64 n_items = L.cnt ? (u64)L.cnt[li] : L.item0[li + 1] - item0;
    uint2* l = S.pairs + (u64)q * S.max_cand;
    u32 n = S.cnt[q], unknown = 0;
    for (u64 k = 0; k < n_items; ++k) {
        const u32 tax = L.item_tax[item0 + k];
        if (tax == MG_NONE) { ++unknown; continue; }
        n = mg_insert(l, n, S.max_cand, tax, L.item_hits[item0 + k], rank[tax] == 0);
    }
    S.cnt[q] = n;
    if (unknown) atomicAdd(S.unknown, (unsigned long long)unknown);
}

// classify() of every merged list, one thread per query; counts: one 64-bit atomic per distinct taxon of the wave
__global__ __launch_bounds__(256) void k_mg_finish(MgState S, u64 n_queries, mcq::ClassifyRules R, u32* best, unsigned long long* counts) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    bool pending = q < n_queries;
    u32 key = MG_NONE;
    if (pending) {
        const u32 n = min(S.cnt[q], S.max_cand);
        const u32 b = mcq::classify_one(S.pairs + q * S.max_cand, n, R);
        if (best) best[q] = b;
        key = b == MG_NONE ? R.n_taxa : b;
    }
    if (!counts) return;
    u64 todo = __ballot(pending);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const u32 lk = __shfl(key, leader);
        const u64 same = __ballot(pending && key == lk);
        if ((int)lane == leader) atomicAdd(&counts[lk], (unsigned long long)__popcll(same));
        if (pending && key == lk) pending = false;
        todo &= ~same;
    }
}

template <class T> struct DevArr {
    T* p = nullptr; u64 cap = 0;
    ~DevArr() { if (p) (void)hipFree(p); }
    int grow(u64 n) {
        if (n <= cap && p) return MCQ_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        HIPCHK(hipMalloc((void**)&p, std::max<u64>(1, n) * sizeof(T)));
        cap = n;
        return MCQ_OK;
    }
};

}  // namespace

struct mcq_merge {
    int device = 0;
    const mcq_taxonomy* tx = nullptr;
    u64 n_ids = 0, n_queries = 0;
    u32 max_cand = 0, merge_below = 0, epoch = 0;
    DevArr<int64_t> id_sorted, taxid;
    DevArr<u32> id_taxon, cnt, hdr_file, hdr_len, claim, status;
    DevArr<uint2> pairs;
    DevArr<u64> hdr_off, tile_cnt, tile_off, line_item0, line_hdr_off;
    DevArr<u32> line_q, line_cnt, line_hdr_len, item_tax, item_hits;
    DevArr<unsigned long long> unknown;

    MgTax tax() const {
        MgTax T; T.id_sorted = id_sorted.p; T.id_taxon = id_taxon.p; T.n_ids = n_ids; T.lineage = tx->lineage; T.rank = tx->rank;
        T.n_taxa = tx->n_taxa; T.merge_below = merge_below;
        return T;
    }
    MgState state() {
        MgState S; S.cnt = cnt.p; S.pairs = pairs.p; S.max_cand = max_cand; S.hdr_file = hdr_file.p; S.hdr_off = hdr_off.p;
        S.hdr_len = hdr_len.p; S.unknown = unknown.p; S.claim = claim.p; S.epoch = epoch;
        return S;
    }
    // a new claim word for the next call (0 is what the array is cleared to)
    int next_epoch(hipStream_t st) {
        if (++epoch == 0) { HIPCHK(hipMemsetAsync(claim.p, 0, (size_t)std::max<u64>(1, n_queries) * 4, st)); epoch = 1; }
        return MCQ_OK;
    }
};

extern "C" int mcq_merge_create(const mcq_taxonomy* tx, const int64_t* taxid_sorted, const uint32_t* taxid_taxon, uint64_t n_ids,
                                uint64_t n_queries, uint32_t max_cand, uint32_t merge_below_rank, int device, mcq_merge** out) {
    if (!tx || !out || (n_ids && (!taxid_sorted || !taxid_taxon))) return fail(MCQ_E_ARG, "null argument");
    if (max_cand < 1 || max_cand > MG_MAX_CAND) return fail(MCQ_E_UNSUPPORTED, "max_cand must be in 1..16");
    if (merge_below_rank >= MG_RANKS) return fail(MCQ_E_ARG, "merge_below_rank must be a rank below 21");
    if (n_queries >= (1ull << 32) - 1) return fail(MCQ_E_UNSUPPORTED, "fewer than 2^32 - 1 queries");
    if (tx->device != device) return fail(MCQ_E_ARG, "the taxonomy lives on another device");
    for (u64 k = 0; k < n_ids; ++k) {
        if (k && taxid_sorted[k - 1] >= taxid_sorted[k]) return fail(MCQ_E_ARG, "the taxon ids must ascend strictly");
        if (taxid_taxon[k] >= tx->n_taxa) return fail(MCQ_E_ARG, "a taxon index outside the taxonomy");
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<mcq_merge> h(new mcq_merge());
    h->device = device; h->tx = tx; h->n_ids = n_ids; h->n_queries = n_queries; h->max_cand = max_cand; h->merge_below = merge_below_rank;
    const u64 nq = std::max<u64>(1, n_queries);
    int rc;
    if ((rc = h->id_sorted.grow(n_ids)) || (rc = h->id_taxon.grow(n_ids)) || (rc = h->cnt.grow(nq)) || (rc = h->pairs.grow(nq * max_cand)) ||
        (rc = h->hdr_file.grow(nq)) || (rc = h->hdr_off.grow(nq)) || (rc = h->hdr_len.grow(nq)) || (rc = h->claim.grow(nq)) ||
        (rc = h->status.grow(1)) || (rc = h->unknown.grow(1))) return rc;
    if (n_ids) {
        HIPCHK(hipMemcpy(h->id_sorted.p, taxid_sorted, n_ids * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->id_taxon.p, taxid_taxon, n_ids * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(h->cnt.p, 0, nq * 4));
    HIPCHK(hipMemset(h->pairs.p, 0, nq * max_cand * 8));
    HIPCHK(hipMemset(h->hdr_file.p, 0, nq * 4));
    HIPCHK(hipMemset(h->hdr_off.p, 0, nq * 8));
    HIPCHK(hipMemset(h->hdr_len.p, 0, nq * 4));
    HIPCHK(hipMemset(h->claim.p, 0, nq * 4));
    HIPCHK(hipMemset(h->unknown.p, 0, 8));
    *out = h.release();
    return MCQ_OK;
}

extern "C" int mcq_merge_chunk(mcq_merge* h, const char* text, uint64_t n_bytes, uint32_t file_ordinal, uint64_t chunk_offset,
                               uint32_t tophits_column, int32_t* strict, void* stream) {
    if (!h || !strict || (n_bytes && !text)) return fail(MCQ_E_ARG, "null argument");
    if (n_bytes >= (1ull << 32)) return fail(MCQ_E_UNSUPPORTED, "a chunk holds fewer than 2^32 bytes");
    if (tophits_column < 2) return fail(MCQ_E_ARG, "top_hits is column 2 or later (column 0 is query_id, column 1 the header)");
    if (chunk_offset + n_bytes < chunk_offset) return fail(MCQ_E_ARG, "chunk_offset + n_bytes overflows");
    *strict = 1;
    if (!n_bytes) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const u64 n_tiles = (n_bytes + MG_TILE - 1) / MG_TILE, item_cap = n_bytes / 4 + 1;
    int rc;
    if ((rc = h->tile_cnt.grow(n_tiles)) || (rc = h->tile_off.grow(n_tiles + 1)) || (rc = h->next_epoch(st))) return rc;
    HIPCHK(hipMemsetAsync(h->status.p, 0, 4, st));
    hipLaunchKernelGGL(k_mg_count, dim3((u32)n_tiles), dim3(256), 0, st, text, n_bytes, h->tile_cnt.p);
    if ((rc = device_exclusive_scan<u64>((const u64*)h->tile_cnt.p, h->tile_off.p, n_tiles, st, 256))) return rc;
    // the number of lines sizes the scratch of the lines and the grids of claim and apply: one wait more, on 9 bytes
    u64 newlines = 0;
    char last = 0;
    HIPCHK(hipMemcpyAsync(&newlines, h->tile_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&last, text + (n_bytes - 1), 1, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const u64 line_cap = newlines + (last != '\n' ? 1 : 0);
    if (line_cap > n_bytes / 2 + 1) { *strict = 0; return MCQ_OK; }          // (a line has two bytes at least: some line is empty)
    if ((rc = h->line_q.grow(line_cap)) || (rc = h->line_item0.grow(line_cap)) || (rc = h->line_cnt.grow(line_cap)) ||
        (rc = h->line_hdr_off.grow(line_cap)) || (rc = h->line_hdr_len.grow(line_cap)) || (rc = h->item_tax.grow(item_cap)) ||
        (rc = h->item_hits.grow(item_cap))) return rc;
    MgChunk C; C.text = text; C.n = n_bytes; C.n_tiles = n_tiles; C.tile_off = h->tile_off.p; C.chunk_offset = chunk_offset;
    C.n_queries = h->n_queries; C.tophits_column = tophits_column;
    MgLines L; L.n_lines = line_cap; L.q = h->line_q.p; L.item0 = h->line_item0.p; L.cnt = h->line_cnt.p;
    L.hdr_off = h->line_hdr_off.p; L.hdr_len = h->line_hdr_len.p; L.item_tax = h->item_tax.p; L.item_hits = h->item_hits.p;
    L.line_cap = line_cap; L.status = h->status.p; L.file_ordinal = file_ordinal;
    hipLaunchKernelGGL(k_mg_parse, dim3((u32)n_tiles), dim3(256), 0, st, h->tax(), C, L);
    const u32 line_blocks = (u32)((line_cap + 255) / 256);
    hipLaunchKernelGGL(k_mg_claim, dim3(line_blocks), dim3(256), 0, st, L, h->state());
    hipLaunchKernelGGL(k_mg_apply, dim3(line_blocks), dim3(256), 0, st, L, h->state(), (const uint8_t*)h->tx->rank);
    HIPCHK(hipGetLastError());
    u32 status = 0;
    HIPCHK(hipMemcpyAsync(&status, h->status.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *strict = status ? 0 : 1;
    return MCQ_OK;
}

extern "C" int mcq_merge_lines(mcq_merge* h, const uint32_t* line_query, const uint64_t* item_off, const int64_t* taxid,
                               const uint32_t* hits, const uint64_t* header_off, const uint32_t* header_len, uint64_t n_lines,
                               uint32_t file_ordinal, uint32_t flags, void* stream) {
    if (!h || !item_off || (n_lines && (!line_query || !header_off || !header_len))) return fail(MCQ_E_ARG, "null argument");
    if (flags) return fail(MCQ_E_ARG, "mcq_merge_lines takes host arrays (flags 0)");
    if (item_off[0] != 0) return fail(MCQ_E_ARG, "item_off[0] must be 0");
    for (u64 l = 0; l < n_lines; ++l) {
        if (item_off[l + 1] < item_off[l]) return fail(MCQ_E_ARG, "item_off must not decrease");
        if (line_query[l] >= h->n_queries) return fail(MCQ_E_ARG, "a line names a query the handle does not have");
    }
    const u64 n_items = item_off[n_lines];
    if (n_items && (!taxid || !hits)) return fail(MCQ_E_ARG, "null argument");
    if (!n_lines) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = h->line_q.grow(n_lines)) || (rc = h->line_item0.grow(n_lines + 1)) || (rc = h->line_hdr_off.grow(n_lines)) ||
        (rc = h->line_hdr_len.grow(n_lines)) || (rc = h->item_tax.grow(n_items)) || (rc = h->item_hits.grow(n_items)) ||
        (rc = h->taxid.grow(n_items)) || (rc = h->next_epoch(st))) return rc;
    HIPCHK(hipMemsetAsync(h->status.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(h->line_q.p, line_query, n_lines * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->line_item0.p, item_off, (n_lines + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->line_hdr_off.p, header_off, n_lines * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->line_hdr_len.p, header_len, n_lines * 4, hipMemcpyHostToDevice, st));
    if (n_items) {
        HIPCHK(hipMemcpyAsync(h->taxid.p, taxid, n_items * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->item_hits.p, hits, n_items * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mg_lookup, dim3((u32)((n_items + 255) / 256)), dim3(256), 0, st, h->tax(), (const int64_t*)h->taxid.p, h->item_tax.p, n_items);
    }
    MgLines L; L.n_lines = n_lines; L.q = h->line_q.p; L.item0 = h->line_item0.p; L.cnt = nullptr;
    L.hdr_off = h->line_hdr_off.p; L.hdr_len = h->line_hdr_len.p; L.item_tax = h->item_tax.p; L.item_hits = h->item_hits.p;
    L.line_cap = n_lines; L.status = h->status.p; L.file_ordinal = file_ordinal;
    const u32 line_blocks = (u32)((n_lines + 255) / 256);
    hipLaunchKernelGGL(k_mg_claim, dim3(line_blocks), dim3(256), 0, st, L, h->state());
    hipLaunchKernelGGL(k_mg_apply, dim3(line_blocks), dim3(256), 0, st, L, h->state(), (const uint8_t*)h->tx->rank);
    HIPCHK(hipGetLastError());
    u32 status = 0;
    HIPCHK(hipMemcpyAsync(&status, h->status.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                             // (the host arrays are free again; the lines are applied)
    if (status) return fail(MCQ_E_ARG, "a query occurs twice in one mcq_merge_lines call: nothing was applied (cut the call there)");
    return MCQ_OK;
}

extern "C" int mcq_merge_finish(mcq_merge* h, const mcq_classify_opts* opts, uint32_t* best, uint64_t* counts, void* stream) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    int rc = mcq::check_classify_opts(opts);
    if (rc) return rc;
    if (h->n_queries == 0 || (!best && !counts)) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    mcq::ClassifyRules R;
    R.lineage = h->tx->lineage; R.rank = h->tx->rank; R.n_taxa = h->tx->n_taxa;
    R.hits_min = opts->hits_min; R.frac = opts->hits_diff_fraction; R.highest = opts->highest_rank;
    hipLaunchKernelGGL(k_mg_finish, dim3((u32)((h->n_queries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->state(), h->n_queries, R,
                       best, reinterpret_cast<unsigned long long*>(counts));
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_merge_lists(mcq_merge* h, uint32_t* n_cand, uint32_t* pairs, uint64_t* n_unknown) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    if (n_cand && h->n_queries) HIPCHK(hipMemcpy(n_cand, h->cnt.p, h->n_queries * 4, hipMemcpyDeviceToHost));
    if (pairs && h->n_queries) HIPCHK(hipMemcpy(pairs, h->pairs.p, h->n_queries * h->max_cand * 8, hipMemcpyDeviceToHost));
    if (n_unknown) HIPCHK(hipMemcpy(n_unknown, h->unknown.p, 8, hipMemcpyDeviceToHost));
    return MCQ_OK;
}

extern "C" int mcq_merge_headers(mcq_merge* h, uint32_t* file, uint64_t* offset, uint32_t* length) {
    if (!h) return fail(MCQ_E_ARG, "null argument");
    if (!h->n_queries) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    if (file) HIPCHK(hipMemcpy(file, h->hdr_file.p, h->n_queries * 4, hipMemcpyDeviceToHost));
    if (offset) HIPCHK(hipMemcpy(offset, h->hdr_off.p, h->n_queries * 8, hipMemcpyDeviceToHost));
    if (length) HIPCHK(hipMemcpy(length, h->hdr_len.p, h->n_queries * 4, hipMemcpyDeviceToHost));
    return MCQ_OK;
}

extern "C" int mcq_merge_free(mcq_merge* h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;
    return MCQ_OK;
}
