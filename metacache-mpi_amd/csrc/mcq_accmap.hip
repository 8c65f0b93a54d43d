// mcq_accmap.hip -- the join of *.accession2taxid text against the names of a database's targets (mcq_accmap_*, include/mcq.h):
// what rank_targets_with_mapping_file (src/mode_build.cpp:248-312) does line by line with three map lookups, for text that has
// the strict four-column form.  A line `acc \t accver \t taxid \t gi` names at most one target: the one named exactly accver, else
// the first name strictly greater than acc if it begins with acc (taxon_with_similar_name, src/sketch_database.h:631-639), else
// the one named exactly gi; an unranked target takes the taxid of the FIRST line that names it, in (file ordinal, line number) order.
//
// A chunk (whole lines of one file, in device memory) goes through five launches on the caller's stream:
//   k_am_count   newlines per 4 KiB tile (16-B loads), then an exclusive scan: the line index of every tile's first line
//   k_am_parse   one workgroup per tile stages the tile and AM_MAX_LINE bytes behind it in LDS with 16-B loads, numbers the line
//                starts of the tile (wave scan + carry, as k_fq_ranges / k_rd_lines do), then one lane per line splits and checks the
//                fields in LDS and binary-searches the sorted names (global memory, read-mostly: offsets and blob stay in L2) up to
//                three times.  Per line it leaves the target (or none) and the taxid in scratch; any violation of the strict form
//                sets the chunk's status word.  Nothing of the handle's state is touched.
//   k_am_claim   (only if the status word is clear) 64-bit atomicMin of (file_ordinal << 40 | line_no) into the target's key
//   k_am_write   (only if clear) the line whose key stands in the target's key word writes its taxid
// A target that an earlier line of any chunk has won holds a smaller key and is left alone; a chunk fed out of order replaces a
// larger key and overwrites the taxid.  The result is a function of the set of (ordinal, line, text) alone, never of scheduling.
// The status word is read back at the end of the call: the call returns when the chunk is applied (or found not strict).
// A handle made by mcq_accmap_create_rule with MCQ_ACCMAP_RULE_ACC / _ACCVER / _GI joins on ONE column instead: a line names the name
// equal to its field 0 / 1 / 3 and no other (what `annotate` does with its std::map, src/mode_annotate.cpp:181-229); the strict form,
// the claim and the write are the same.
// Stores are plain C++ and vector atomics.
#include "mcq_internal.hpp"

namespace {

constexpr u32 AM_TILE = 4096;                          // bytes of text per workgroup
constexpr u32 AM_MAX_LINE = MCQ_ACCMAP_MAX_LINE;       // a strict line with its '\n' is no longer than this
constexpr u32 AM_LDS = AM_TILE + AM_MAX_LINE;          // a line that starts in the tile and is strict ends inside this
constexpr u32 AM_MIN_LINE = 8;                         // "a\tb\t1\tc\n"
constexpr u32 AM_TILE_LINES = AM_TILE / AM_MIN_LINE + 1;   // more line starts than this in a tile: some line is too short to be strict
constexpr u32 AM_NONE = 0xFFFFFFFFu;
constexpr u64 AM_NO_KEY = ~0ull;
static_assert(AM_LDS % 16 == 0 && AM_TILE == 256 * 16, "one 16-B load per thread covers the tile");

struct AmNames {
    const unsigned char* blob; const u64* off; const u32* target; u64 n;     // sorted bytewise (unsigned), then by length
    const unsigned char* unranked; u32 n_targets;
};
struct AmChunk {
    const char* text; u64 n;              // the chunk
    u64 n_tiles; const u64* tile_off;     // [n_tiles + 1] newlines before each tile
    u32* line_tgt; u64* line_tax; u64 line_cap;
    u32* status;                          // != 0: not strict
    u64 key0;                             // file_ordinal << 40 | first_line_no
};

// bit j = byte j of the 16 is '\n' (exact per-byte zero detection, as fq_newline_mask)
__device__ __forceinline__ u32 am_newlines(const uint4 v) {
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
// text[base .. base + 16) as one 16-B load where it is aligned and inside the chunk, byte by byte at the ragged ends; 0 behind the end
__device__ __forceinline__ uint4 am_load16(const char* __restrict__ text, u64 base, u64 n) {
    if (base + 16 <= n && ((reinterpret_cast<uintptr_t>(text) + base) & 15) == 0) return *reinterpret_cast<const uint4*>(text + base);
    u32 w[4] = {0, 0, 0, 0};
    for (u32 j = 0; j < 16; ++j)
        if (base + j < n) w[j >> 2] |= (u32)(unsigned char)text[base + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(256) void k_am_count(const char* text, u64 n, u64* tile_cnt) {
    __shared__ u32 s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * AM_TILE + (u64)threadIdx.x * 16;
    u32 c = base < n ? (u32)__builtin_popcount(am_newlines(am_load16(text, base, n))) : 0u;     // (the 0 fill is no newline)
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_c;
}

// name k against the field s[0 .. len) in LDS: < 0, 0, > 0 as std::string::compare (unsigned bytes, then length)
__device__ __forceinline__ int am_cmp(const AmNames& N, u64 k, const unsigned char* s, u32 len) {
    const u64 b = N.off[k], nl = N.off[k + 1] - b;
    const u32 m = nl < len ? (u32)nl : len;
    const unsigned char* __restrict__ p = N.blob + b;
    for (u32 i = 0; i < m; ++i) {
        const int d = (int)p[i] - (int)s[i];
        if (d) return d;
    }
    return nl < len ? -1 : (nl > len ? 1 : 0);
}
// the name equal to the field: its index, or n
__device__ __forceinline__ u64 am_find(const AmNames& N, const unsigned char* s, u32 len) {
    u64 lo = 0, hi = N.n;                                       // first name >= field
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (am_cmp(N, mid, s, len) < 0) lo = mid + 1; else hi = mid; }
    return (lo < N.n && am_cmp(N, lo, s, len) == 0) ? lo : N.n;
}
// taxon_with_similar_name: the first name > field, if its first len bytes are the field; else n
__device__ __forceinline__ u64 am_similar(const AmNames& N, const unsigned char* s, u32 len) {
    u64 lo = 0, hi = N.n;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (am_cmp(N, mid, s, len) <= 0) lo = mid + 1; else hi = mid; }
    if (lo >= N.n) return N.n;
    const u64 b = N.off[lo], nl = N.off[lo + 1] - b;
    if (nl < len) return N.n;
    for (u32 i = 0; i < len; ++i) if (N.blob[b + i] != s[i]) return N.n;
    return lo;
}

// RULE: MCQ_ACCMAP_RULE_TARGETS (the three lookups of a build's post-mapping) or _ACC / _ACCVER / _GI (the name equal to field 0 / 1 /
// 3 and nothing else: the exact-column join of `annotate`).  A compile-time axis: the default rule's instantiation is the code it was.
template <u32 RULE>
__global__ __launch_bounds__(256) void k_am_parse(AmNames N, AmChunk C) {
    __shared__ uint4 s_text4[AM_LDS / 16];
    __shared__ unsigned short s_start[AM_TILE_LINES + 1];
    __shared__ u32 s_w[4];
    unsigned char* s_text = reinterpret_cast<unsigned char*>(s_text4);
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 tile0 = (u64)blockIdx.x * AM_TILE;
    // the tile and what may hold the end of its last line, 16 B per load
    const uint4 mine = am_load16(C.text, tile0 + (u64)tid * 16, C.n);
    s_text4[tid] = mine;
    if (tid < AM_MAX_LINE / 16) s_text4[256 + tid] = am_load16(C.text, tile0 + AM_TILE + (u64)tid * 16, C.n);
    const bool tile_at_line_start = tile0 == 0 || C.text[tile0 - 1] == '\n';
    __syncthreads();
    // line starts among my 16 bytes: behind every newline, inside the chunk
    const u64 base = tile0 + (u64)tid * 16;
    const u32 nlm = am_newlines(mine);
    const u32 valid = base >= C.n ? 0u : (C.n - base >= 16 ? 0xFFFFu : (1u << (u32)(C.n - base)) - 1u);
    const u32 prev = tid == 0 ? (u32)tile_at_line_start : (u32)(s_text[tid * 16 - 1] == '\n');
    const u32 lsm = ((nlm << 1) | prev) & valid;
    const u32 c = (u32)__builtin_popcount(lsm);
    const u32 incl = wave_incl_scan_dpp(c);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u32 woff = 0, total = 0;
    for (u32 w = 0; w < 4; ++w) { if (w < wave) woff += s_w[w]; total += s_w[w]; }
    if (total > AM_TILE_LINES) { if (tid == 0) *C.status = 1; return; }       // (uniform: a line shorter than any strict one)
    u32 at = woff + incl - c;
    for (u32 m = lsm; m; m &= m - 1) s_start[at++] = (unsigned short)(tid * 16 + (u32)__builtin_ctz(m));
    __syncthreads();
    const u64 line0 = C.tile_off[blockIdx.x] + (tile_at_line_start ? 0 : 1);  // index of the tile's first line start
    bool bad = false;
    for (u32 j = tid; j < total; j += 256) {
        const u32 p = s_start[j];
        const u64 left = C.n - (tile0 + p);
        const u32 scan = left < AM_MAX_LINE ? (u32)left : AM_MAX_LINE;
        const unsigned char* s = s_text + p;
        u32 fbeg[4] = {0, 0, 0, 0}, flen[4] = {0, 0, 0, 0}, f = 0, i = 0;
        u64 taxid = 0;
        bool ok = true, ended = false;
        for (; i < scan; ++i) {
            const unsigned char ch = s[i];
            if (ch == '\n') { ended = true; break; }
            if (ch == '\t') {
                if (flen[f] == 0 || f == 3) { ok = false; break; }
                ++f; fbeg[f] = i + 1;
            } else if (ch == '\r') {
                if (!(f == 3 && i + 1 < scan && s[i + 1] == '\n')) { ok = false; break; }
                ended = true; break;
            } else if (ch == ' ' || ch == '\v' || ch == '\f') { ok = false; break; }
            else {
                ++flen[f];
                if (f == 2) {
                    if (ch < '0' || ch > '9' || flen[2] > 19) { ok = false; break; }
                    taxid = taxid * 10 + (u64)(ch - '0');
                }
            }
        }
        ok = ok && ended && f == 3 && flen[3] > 0;                            // (fields 0..2 were closed non-empty)
        const u64 li = line0 + j;
        if (!ok || li >= C.line_cap) { bad = true; continue; }
        u64 k;
        if constexpr (RULE == MCQ_ACCMAP_RULE_TARGETS) {
            k = am_find(N, s + fbeg[1], flen[1]);
            if (k == N.n) k = am_similar(N, s + fbeg[0], flen[0]);
            if (k == N.n) k = am_find(N, s + fbeg[3], flen[3]);
        } else {
            constexpr u32 col = RULE == MCQ_ACCMAP_RULE_ACC ? 0u : (RULE == MCQ_ACCMAP_RULE_ACCVER ? 1u : 3u);
            k = am_find(N, s + fbeg[col], flen[col]);
        }
        u32 t = AM_NONE;
        if (k != N.n) { t = N.target[k]; if (!N.unranked[t]) t = AM_NONE; }   // (no falling through when the target is ranked)
        C.line_tgt[li] = t;
        C.line_tax[li] = taxid;
    }
    if (bad) *C.status = 1;
}

__global__ __launch_bounds__(256) void k_am_claim(AmChunk C, unsigned long long* key) {
    if (*C.status) return;
    const u64 li = (u64)blockIdx.x * 256 + threadIdx.x, n_lines = C.tile_off[C.n_tiles];
    if (li >= n_lines || li >= C.line_cap) return;
    const u32 t = C.line_tgt[li];
    if (t != AM_NONE) atomicMin(&key[t], (unsigned long long)(C.key0 + li));
}
__global__ __launch_bounds__(256) void k_am_write(AmChunk C, const unsigned long long* key, u64* taxid) {
    if (*C.status) return;
    const u64 li = (u64)blockIdx.x * 256 + threadIdx.x, n_lines = C.tile_off[C.n_tiles];
    if (li >= n_lines || li >= C.line_cap) return;
    const u32 t = C.line_tgt[li];
    if (t != AM_NONE && key[t] == C.key0 + li) taxid[t] = C.line_tax[li];
}

template <class T> struct DevArr {
    T* p = nullptr; u64 cap = 0;
    ~DevArr() { if (p) (void)hipFree(p); }
    int grow(u64 n) {
        if (n <= cap) return MCQ_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        HIPCHK(hipMalloc((void**)&p, std::max<u64>(1, n) * sizeof(T)));
        cap = n;
        return MCQ_OK;
    }
};

}  // namespace

struct mcq_accmap {
    int device = 0;
    u32 rule = MCQ_ACCMAP_RULE_TARGETS;
    u64 n_names = 0; u32 n_targets = 0;
    DevArr<unsigned char> blob, unranked;
    DevArr<u64> name_off, taxid, tile_cnt, tile_off, line_tax;
    DevArr<u32> name_target, line_tgt, status;
    DevArr<unsigned long long> key;
};

extern "C" int mcq_accmap_create(const char* names_blob, const uint64_t* name_off, uint64_t n_names, const uint32_t* name_target,
                                 const uint8_t* unranked, uint32_t n_targets, int device, mcq_accmap** out) {
    return mcq_accmap_create_rule(names_blob, name_off, n_names, name_target, unranked, n_targets, MCQ_ACCMAP_RULE_TARGETS, device, out);
}

extern "C" int mcq_accmap_create_rule(const char* names_blob, const uint64_t* name_off, uint64_t n_names, const uint32_t* name_target,
                                      const uint8_t* unranked, uint32_t n_targets, uint32_t rule, int device, mcq_accmap** out) {
    if (rule > MCQ_ACCMAP_RULE_GI) return fail(MCQ_E_ARG, "the rule is one of MCQ_ACCMAP_RULE_*");
    if (!out || !name_off || (n_names && (!name_target || !names_blob)) || (n_targets && !unranked)) return fail(MCQ_E_ARG, "null argument");
    if (name_off[0] != 0) return fail(MCQ_E_ARG, "name_off[0] must be 0");
    for (u64 k = 0; k < n_names; ++k) {
        if (name_off[k + 1] < name_off[k]) return fail(MCQ_E_ARG, "name_off must not decrease");
        if (name_target[k] >= n_targets) return fail(MCQ_E_ARG, "a name's target is outside the targets");
        if (k) {                                                 // strictly ascending: unsigned bytes, then length
            const u64 a = name_off[k - 1], la = name_off[k] - a, b = name_off[k], lb = name_off[k + 1] - b;
            const int d = memcmp(names_blob + a, names_blob + b, (size_t)std::min(la, lb));
            if (d > 0 || (d == 0 && la >= lb)) return fail(MCQ_E_ARG, "the names must be sorted bytewise and distinct");
        }
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<mcq_accmap> h(new mcq_accmap());
    h->device = device; h->rule = rule; h->n_names = n_names; h->n_targets = n_targets;
    const u64 nb = name_off[n_names];
    int rc;
    if ((rc = h->blob.grow(nb)) || (rc = h->name_off.grow(n_names + 1)) || (rc = h->name_target.grow(n_names)) ||
        (rc = h->unranked.grow(n_targets)) || (rc = h->key.grow(n_targets)) || (rc = h->taxid.grow(n_targets)) || (rc = h->status.grow(1))) return rc;
    if (nb) HIPCHK(hipMemcpy(h->blob.p, names_blob, nb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->name_off.p, name_off, (n_names + 1) * 8, hipMemcpyHostToDevice));
    if (n_names) HIPCHK(hipMemcpy(h->name_target.p, name_target, n_names * 4, hipMemcpyHostToDevice));
    if (n_targets) {
        HIPCHK(hipMemcpy(h->unranked.p, unranked, n_targets, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(h->key.p, 0xFF, (size_t)n_targets * 8));
        HIPCHK(hipMemset(h->taxid.p, 0, (size_t)n_targets * 8));
    }
    *out = h.release();
    return MCQ_OK;
}

extern "C" int mcq_accmap_chunk(mcq_accmap* h, const char* text, uint64_t n_bytes, uint32_t file_ordinal, uint64_t first_line_no,
                                uint32_t* strict, void* stream) {
    if (!h || !strict || (n_bytes && !text)) return fail(MCQ_E_ARG, "null argument");
    if (n_bytes >= (1ull << 32)) return fail(MCQ_E_UNSUPPORTED, "a chunk holds fewer than 2^32 bytes");
    if (file_ordinal >= (1u << 23) || first_line_no >= (1ull << 40) || first_line_no + n_bytes >= (1ull << 40))
        return fail(MCQ_E_UNSUPPORTED, "file ordinals below 2^23 and line numbers below 2^40");
    *strict = 1;
    if (!n_bytes) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const u64 n_tiles = (n_bytes + AM_TILE - 1) / AM_TILE, line_cap = n_bytes / AM_MIN_LINE + 1;
    int rc;
    if ((rc = h->tile_cnt.grow(n_tiles)) || (rc = h->tile_off.grow(n_tiles + 1)) || (rc = h->line_tgt.grow(line_cap)) || (rc = h->line_tax.grow(line_cap))) return rc;
    HIPCHK(hipMemsetAsync(h->status.p, 0, 4, st));
    hipLaunchKernelGGL(k_am_count, dim3((u32)n_tiles), dim3(256), 0, st, text, n_bytes, h->tile_cnt.p);
    if ((rc = device_exclusive_scan<u64>((const u64*)h->tile_cnt.p, h->tile_off.p, n_tiles, st, 256))) return rc;
    AmNames N; N.blob = h->blob.p; N.off = h->name_off.p; N.target = h->name_target.p; N.n = h->n_names; N.unranked = h->unranked.p; N.n_targets = h->n_targets;
    AmChunk C; C.text = text; C.n = n_bytes; C.n_tiles = n_tiles; C.tile_off = h->tile_off.p; C.line_tgt = h->line_tgt.p; C.line_tax = h->line_tax.p;
    C.line_cap = line_cap; C.status = h->status.p; C.key0 = ((u64)file_ordinal << 40) | first_line_no;
    switch (h->rule) {
        case MCQ_ACCMAP_RULE_ACC:    hipLaunchKernelGGL(k_am_parse<MCQ_ACCMAP_RULE_ACC>, dim3((u32)n_tiles), dim3(256), 0, st, N, C); break;
        case MCQ_ACCMAP_RULE_ACCVER: hipLaunchKernelGGL(k_am_parse<MCQ_ACCMAP_RULE_ACCVER>, dim3((u32)n_tiles), dim3(256), 0, st, N, C); break;
        case MCQ_ACCMAP_RULE_GI:     hipLaunchKernelGGL(k_am_parse<MCQ_ACCMAP_RULE_GI>, dim3((u32)n_tiles), dim3(256), 0, st, N, C); break;
        default:                     hipLaunchKernelGGL(k_am_parse<MCQ_ACCMAP_RULE_TARGETS>, dim3((u32)n_tiles), dim3(256), 0, st, N, C); break;
    }
    const u32 line_blocks = (u32)((line_cap + 255) / 256);
    hipLaunchKernelGGL(k_am_claim, dim3(line_blocks), dim3(256), 0, st, C, h->key.p);
    hipLaunchKernelGGL(k_am_write, dim3(line_blocks), dim3(256), 0, st, C, (const unsigned long long*)h->key.p, h->taxid.p);
    HIPCHK(hipGetLastError());
    u32 status = 0;
    HIPCHK(hipMemcpyAsync(&status, h->status.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *strict = status ? 0u : 1u;
    return MCQ_OK;
}

extern "C" int mcq_accmap_finish(mcq_accmap* h, int64_t* parent, uint8_t* found) {
    if (!h || (h->n_targets && (!parent || !found))) return fail(MCQ_E_ARG, "null argument");
    if (!h->n_targets) return MCQ_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> key(h->n_targets);
    HIPCHK(hipMemcpy(key.data(), h->key.p, (size_t)h->n_targets * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(parent, h->taxid.p, (size_t)h->n_targets * 8, hipMemcpyDeviceToHost));      // (uint64 as read -> taxon_id, as reset_parent takes it)
    for (u32 t = 0; t < h->n_targets; ++t) { found[t] = key[t] != AM_NO_KEY; if (!found[t]) parent[t] = 0; }
    return MCQ_OK;
}

extern "C" int mcq_accmap_free(mcq_accmap* h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;
    return MCQ_OK;
}
