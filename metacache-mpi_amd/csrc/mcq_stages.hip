// mcq_stages.hip -- the query path as separate stages behind the C ABI (see include/mcq.h), and batch preparation:
// mcq_count_windows, mcq_sketch, mcq_lookup_*, mcq_assemble (rows 1-7 one call each; mcq_reduce, rows 8-11, is in
// mcq_engine.hip), feature routing for sharded runs (mcq_owner, mcq_bucket_features), FASTQ/FASTA indexing, chunks of
// read files into compacted batches (mcq_reads_prepare), base packing, and the exclusive scan that these and table creation use.
#include "mcq_internal.hpp"

// ------------------------------------------------------------------ exclusive scan
// exclusive scan of u64 array (single workgroup of 256 or 1024 threads)
template <class InT>
__global__ __launch_bounds__(1024) void k_scan_u64(const InT* in, u64* out, u64 n) {
    __shared__ u64 s_w[16];
    __shared__ u64 s_carry;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < n; base += NT) {
        u64 i = base + tid;
        u64 v = (i < n) ? in[i] : 0, x = v;
        for (int d = 1; d < 64; d <<= 1) {
            u64 t = __shfl_up(x, d, 64);
            if (lane >= (u32)d) x += t;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        u64 woff = 0;
        for (u32 w = 0; w < wave; ++w) woff += s_w[w];
        u64 carry = s_carry;
        if (i < n) out[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == NT - 1) s_carry = carry + woff + x;
        __syncthreads();
    }
    if (tid == 0) out[n] = s_carry;
}

// exclusive scan of n u64 values in three launches: per-tile scan + tile sums, scan of the
// tile sums (one workgroup), add.  out has n + 1 entries (out[n] = total).
#define MCQ_SCAN_TILE 8192
template <class InT>
__global__ __launch_bounds__(1024) void k_scan_tiles(const InT* in, u64* out, u64 n, u64* tile_sums) {
    __shared__ u64 s_w[16];
    __shared__ u64 s_carry;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    const u64 t0 = (u64)blockIdx.x * MCQ_SCAN_TILE;
    for (u64 base = t0; base < t0 + MCQ_SCAN_TILE; base += NT) {
        const u64 i = base + tid;
        u64 v = (i < n) ? in[i] : 0, x = v;
        for (int d = 1; d < 64; d <<= 1) { u64 t = __shfl_up(x, d, 64); if (lane >= (u32)d) x += t; }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        u64 woff = 0;
        for (u32 w = 0; w < wave; ++w) woff += s_w[w];
        const u64 carry = s_carry;
        if (i < n) out[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == NT - 1) s_carry = carry + woff + x;
        __syncthreads();
    }
    if (tid == 0) tile_sums[blockIdx.x] = s_carry;
}
__global__ void k_scan_add(u64* out, u64 n, const u64* tile_off) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += tile_off[i / MCQ_SCAN_TILE];
    if (i == 0) out[n] = tile_off[(n + MCQ_SCAN_TILE - 1) / MCQ_SCAN_TILE];
}

// nt: threads per workgroup, 256 or 1024.  A 1024-thread workgroup needs 16 free wave slots on ONE CU at once: enqueued
// beside a grid of smaller workgroups that fills the GPU (the sharded path's second stream) it waits until that grid has
// drained; 256-thread workgroups slip in as the others retire.
template <class InT>
int mcq::device_exclusive_scan(const InT* in, u64* out, u64 n, hipStream_t st, u32 nt) {
    const u64 ntiles = (n + MCQ_SCAN_TILE - 1) / MCQ_SCAN_TILE;
    if (ntiles <= 1) { hipLaunchKernelGGL(k_scan_u64<InT>, dim3(1), dim3(nt), 0, st, in, out, n); return MCQ_OK; }
    u64 *sums = nullptr, *offs = nullptr;
    HIPCHK(hipMallocAsync((void**)&sums, ntiles * 8, st));
    HIPCHK(hipMallocAsync((void**)&offs, (ntiles + 1) * 8, st));
    hipLaunchKernelGGL(k_scan_tiles<InT>, dim3((u32)ntiles), dim3(nt), 0, st, in, out, n, sums);
    hipLaunchKernelGGL(k_scan_u64<u64>, dim3(1), dim3(nt), 0, st, (const u64*)sums, offs, ntiles);
    hipLaunchKernelGGL(k_scan_add, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, out, n, (const u64*)offs);
    HIPCHK(hipFreeAsync(sums, st));
    HIPCHK(hipFreeAsync(offs, st));
    return MCQ_OK;
}
template int mcq::device_exclusive_scan<u32>(const u32*, u64*, u64, hipStream_t, u32);
template int mcq::device_exclusive_scan<u64>(const u64*, u64*, u64, hipStream_t, u32);

// ------------------------------------------------------------------ staged kernels (sharded path, DB build)
__global__ void k_count_windows(const u64* seq_off, u32 ranges, u64 n_seqs, u32 W, u32 S, u64* cnt) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seqs) { u64 bg, en; seq_bounds(seq_off, ranges, i, bg, en); cnt[i] = num_windows64(en - bg, W, S); }
}

// one wave per window: window w belongs to the last sequence i with win_off[i] <= w
__global__ __launch_bounds__(256) void k_sketch_windows(DbDev db, const char* bases, const u64* seq_off, u32 ranges, u64 n_seqs,
                                                        const u64* win_off, u32* features, u32* n_feat) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 n_win = win_off[n_seqs];
    const u64 nwaves = (u64)gridDim.x * 4;
    __shared__ u32 s_sk[4][128];
    u32* sk = s_sk[wave];
    for (u64 w = (u64)blockIdx.x * 4 + wave; w < n_win; w += nwaves) {
        u64 lo = 0, hi = n_seqs;
        while (hi - lo > 1) { u64 mid = (lo + hi) >> 1; if (win_off[mid] <= w) lo = mid; else hi = mid; }
        u64 o0, oe; seq_bounds(seq_off, ranges, lo, o0, oe);
        const u64 n = oe - o0;
        u64 beg; u32 wl;
        window_of(n, db.winlen, db.winstride, (u32)(w - win_off[lo]), beg, wl);
        u32 m = wave_sketch(bases + o0 + beg, wl, db.k, db.s, lane, sk, sk + 64);
        if (lane < db.s) features[w * db.s + lane] = (lane < m) ? sk[64 + lane] : MCQ_EMPTY;
        if (lane == 0) n_feat[w] = m;
        wave_sync();
    }
}

// one wave per sequence, looping over its (few) windows: no search, window math in 32 bits
__global__ __launch_bounds__(256) void k_sketch_seqs(DbDev db, const char* bases, const u64* seq_off, u32 ranges, u64 n_seqs,
                                                     const u64* win_off, u32* features, u32* n_feat) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 nwaves = (u64)gridDim.x * 4;
    __shared__ u32 s_sk[4][128];
    u32* sk = s_sk[wave];
    for (u64 i = (u64)blockIdx.x * 4 + wave; i < n_seqs; i += nwaves) {
        u64 o0, oe; seq_bounds(seq_off, ranges, i, o0, oe);
        const u32 n = (u32)(oe - o0);
        const u64 w0 = win_off[i];
        const u32 nw = (u32)(win_off[i + 1] - w0);
        for (u32 j = 0; j < nw; ++j) {
            u32 beg, wl;
            window_of32(n, db.winlen, db.winstride, db.magic_stride, j, beg, wl);
            u32 m = wave_sketch(bases + o0 + beg, wl, db.k, db.s, lane, sk, sk + 64);
            if (lane < db.s) features[(w0 + j) * db.s + lane] = (lane < m) ? sk[64 + lane] : MCQ_EMPTY;
            if (lane == 0) n_feat[w0 + j] = m;
            wave_sync();
        }
    }
}

__global__ void k_lookup_count(DbDev db, const u32* features, u64 n, u32* list_len, u64* list_src) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 off; u32 len;
    probe(db, features[i], off, len);
    list_len[i] = len;
    if (list_src) list_src[i] = off;
}

// one wave per 64 consecutive features: (probe again unless the list starts were kept), then
// copy the lists cooperatively, in the handle's native location width
template <class KeyT>
__global__ __launch_bounds__(256) void k_lookup_gather(DbDev db, const u32* features, u64 n, const u32* list_len,
                                                       const u64* list_src, const u64* out_off, KeyT* out_locs) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 ngroups = (n + 63) / 64, nwaves = (u64)gridDim.x * 4;
    const KeyT* __restrict__ locs = static_cast<const KeyT*>(db.locs);
    for (u64 g = (u64)blockIdx.x * 4 + wave; g < ngroups; g += nwaves) {
        const u64 i = g * 64 + lane;
        u64 off = 0; u32 len = 0;
        if (i < n) {
            if (list_src) { off = list_src[i]; len = list_len[i]; }
            else probe(db, features[i], off, len);
        }
        const u64 obase = out_off[g * 64];
        u32 incl = wave_incl_scan_dpp(len);
        u32 pos = incl - len;
        const u32 T = bcast(incl, 63);
        for (u32 base = 0; base < T; base += 256) {           // four 64-element chunks in flight per round trip
            KeyT v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = 0;
                if (base + (u32)(u * 64) < T) {
                    const u32 t = base + u * 64 + lane;
                    const u32 tt = t < T ? t : T - 1;
                    u32 lo = 0;
#pragma unroll
                    for (u32 step = 32; step > 0; step >>= 1) {
                        u32 c = lo + step;
                        u32 pc = __shfl(pos, (int)(c & 63), 64);
                        if (c < 64 && pc <= tt) lo = c;
                    }
                    u32 pj = __shfl(pos, (int)lo, 64);
                    u32 olo = __shfl((u32)off, (int)lo, 64), ohi = __shfl((u32)(off >> 32), (int)lo, 64);
                    if (t < T) v[u] = locs[(((u64)ohi << 32) | olo) + (tt - pj)];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u32 t = base + u * 64 + lane;
                if (t < T) out_locs[obase + t] = v[u];
            }
        }
    }
}

// ------------------------------------------------------------------ sharded-path routing kernels
// Bucket features by owning shard (mcq_owner); EMPTY features are dropped.  Counting sort
// over workgroup tiles: (1) every workgroup counts its tile per shard, (2) one workgroup
// turns the [shard][workgroup] counts into start offsets (shard-major), (3) every workgroup
// places its features; waves of a workgroup claim their slice with an LDS atomic.
#define MCQ_BUCKET_MAX_SHARDS 64
__device__ __forceinline__ u32 owner_of(u32 f, u32 n_shards) {
    return f == MCQ_EMPTY ? 0xFFFFFFFFu : (u32)(((u64)tmh(f) * n_shards) >> 32);
}
__global__ __launch_bounds__(256) void k_bucket_count(const u32* features, u64 n, u32 n_shards, u64 tile,
                                                      unsigned long long* blk_counts /* [n_shards][gridDim.x] */) {
    __shared__ u32 s_c[MCQ_BUCKET_MAX_SHARDS];
    const u32 lane = threadIdx.x & 63;
    if (threadIdx.x < MCQ_BUCKET_MAX_SHARDS) s_c[threadIdx.x] = 0;
    __syncthreads();
    const u64 t0 = (u64)blockIdx.x * tile, t1 = t0 + tile < n ? t0 + tile : n;
    for (u64 i0 = t0 + (threadIdx.x & ~63u); i0 < t1; i0 += 256) {
        const u64 i = i0 + lane;
        const u32 own = owner_of(i < t1 ? features[i] : MCQ_EMPTY, n_shards);
        for (u32 o = 0; o < n_shards; ++o) {
            u32 c = (u32)__builtin_popcountll(__ballot(own == o));
            if (lane == 0 && c) atomicAdd(&s_c[o], c);
        }
    }
    __syncthreads();
    if (threadIdx.x < n_shards) blk_counts[(u64)threadIdx.x * gridDim.x + blockIdx.x] = s_c[threadIdx.x];
}
// exclusive scan over the [shard][workgroup] matrix in shard-major order; totals per shard to counts[]
__global__ __launch_bounds__(1024) void k_bucket_scan(unsigned long long* blk_counts, u32 n_shards, u32 n_blocks, unsigned long long* counts) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long s_carry;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 n = (u64)n_shards * n_blocks;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < n; base += 1024) {
        const u64 i = base + tid;
        unsigned long long v = i < n ? blk_counts[i] : 0, x = v;
        for (int d = 1; d < 64; d <<= 1) { unsigned long long t = __shfl_up(x, d, 64); if (lane >= (u32)d) x += t; }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        unsigned long long woff = 0;
        for (u32 w = 0; w < wave; ++w) woff += s_w[w];
        const unsigned long long carry = s_carry;
        if (i < n) blk_counts[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = carry + woff + x;
        __syncthreads();
    }
    // per-shard totals = difference of the shard's first offsets
    if (tid < n_shards) {
        unsigned long long b0 = blk_counts[(u64)tid * n_blocks];
        unsigned long long b1 = (tid + 1 < n_shards) ? blk_counts[(u64)(tid + 1) * n_blocks] : s_carry;
        counts[tid] = b1 - b0;
    }
}
__global__ __launch_bounds__(256) void k_bucket_fill(const u32* features, u64 n, u32 n_shards, u64 tile,
                                                     const unsigned long long* blk_off, u32* bucketed, u32* src_index) {
    __shared__ unsigned long long s_cur[MCQ_BUCKET_MAX_SHARDS];
    const u32 lane = threadIdx.x & 63;
    if (threadIdx.x < n_shards) s_cur[threadIdx.x] = blk_off[(u64)threadIdx.x * gridDim.x + blockIdx.x];
    __syncthreads();
    const u64 t0 = (u64)blockIdx.x * tile, t1 = t0 + tile < n ? t0 + tile : n;
    for (u64 i0 = t0 + (threadIdx.x & ~63u); i0 < t1; i0 += 256) {
        const u64 i = i0 + lane;
        const u32 f = i < t1 ? features[i] : MCQ_EMPTY;
        const u32 own = owner_of(f, n_shards);
        for (u32 o = 0; o < n_shards; ++o) {
            const u64 m = __ballot(own == o);
            const u32 c = (u32)__builtin_popcountll(m);
            unsigned long long start = 0;
            if (lane == 0 && c) start = atomicAdd(&s_cur[o], (unsigned long long)c);
            start = ((unsigned long long)__builtin_amdgcn_readfirstlane((u32)(start >> 32)) << 32) | __builtin_amdgcn_readfirstlane((u32)start);
            if (own == o) {
                const u64 d = start + lane_rank(m);
                bucketed[d] = f; src_index[d] = (u32)i;
            }
        }
    }
}

// list i = src_locs[src_off[i] .. src_off[i+1]) goes to dst_locs[dst_off[dst_slot[i]] ..); one wave per 64 lists
template <class KeyT>
__global__ __launch_bounds__(256) void k_scatter_lists(u64 n_lists, const u64* src_off, const u32* dst_slot, const u64* dst_off,
                                                       const KeyT* src_locs, KeyT* dst_locs) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 ngroups = (n_lists + 63) / 64, nwaves = (u64)gridDim.x * 4;
    for (u64 g = (u64)blockIdx.x * 4 + wave; g < ngroups; g += nwaves) {
        const u64 i = g * 64 + lane;
        u64 so = 0, d = 0; u32 len = 0;
        if (i < n_lists) { so = src_off[i]; len = (u32)(src_off[i + 1] - so); d = dst_off[dst_slot[i]]; }
        const u64 sbase = src_off[g * 64];
        u32 incl = wave_incl_scan_dpp(len);
        u32 pos = incl - len;
        const u32 T = bcast(incl, 63);
        for (u32 base = 0; base < T; base += 64) {
            const u32 t = base + lane;
            const u32 tt = t < T ? t : T - 1;
            u32 lo = 0;
#pragma unroll
            for (u32 step = 32; step > 0; step >>= 1) {
                u32 c = lo + step;
                u32 pc = __shfl(pos, (int)(c & 63), 64);
                if (c < 64 && pc <= tt) lo = c;
            }
            u32 pj = __shfl(pos, (int)lo, 64);
            u32 dlo = __shfl((u32)d, (int)lo, 64), dhi = __shfl((u32)(d >> 32), (int)lo, 64);
            if (t < T) dst_locs[(((u64)dhi << 32) | dlo) + (tt - pj)] = src_locs[sbase + t];
        }
    }
}
__global__ void k_scatter_len(const u32* list_len, const u32* slot, u64 n, u32* slot_len) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slot_len[slot[i]] = list_len[i];
}
// per query: location segment start = offset of its first feature slot; length = sum of its mates
__global__ void k_query_offsets(u64 nq, u32 qstep, u32 s, const u64* win_off, const u64* seq_off, u32 ranges, const u64* dst_off, u64 n_slots,
                                u64* loc_off, u32* query_len) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) {
        loc_off[q] = dst_off[win_off[q * qstep] * s];
        u64 len = 0;
        for (u32 m = 0; m < qstep; ++m) { u64 bg, en; seq_bounds(seq_off, ranges, q * qstep + m, bg, en); len += en - bg; }
        query_len[q] = (u32)len;
    }
    if (q == 0) loc_off[nq] = dst_off[n_slots];
}

// ------------------------------------------------------------------ row f4: FASTQ text -> sequence ranges on the GPU
// FASTQ is four lines per record and the reference reads it exactly so (fastq_reader::read_next,
// src/sequence_io.cpp:251-285: getline header, getline data, getline '+', getline qualities), so
// the sequence of record r is line 4r+1.  Workgroup tiles of 4 KiB count their newlines, a scan
// gives every newline its line number, and the newline that ends line 4r (4r+1) writes the
// begin (end) of sequence r.  The text is not copied: mcq_query reads the bases in place
// (MCQ_BATCH_RANGES).  Like getline, a '\r' before the newline stays part of the line.
#define MCQ_FQ_TILE 4096
// 16-bit mask of the newlines among text[base .. base+16): one 16-B load and exact per-byte zero detection of
// (word ^ 0x0A0A0A0A) when the address is aligned and inside the buffer, a byte loop otherwise
__device__ __forceinline__ u32 fq_newline_mask(const char* __restrict__ text, u64 base, u64 n) {
    u32 mask = 0;
    if (base + 16 <= n && ((reinterpret_cast<uintptr_t>(text) + base) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32 m = w[i] ^ 0x0A0A0A0Au;
            const u32 z = ~(((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u;     // bit 7 of every zero byte
            mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * i);
        }
    } else {
        for (u32 j = 0; j < 16; ++j) mask |= (u32)(base + j < n && text[base + j] == '\n') << j;
    }
    return mask;
}
__global__ __launch_bounds__(256) void k_fq_count(const char* text, u64 n, u64* tile_cnt) {
    __shared__ u32 s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * MCQ_FQ_TILE + (u64)threadIdx.x * 16;
    u32 c = (u32)__builtin_popcount(fq_newline_mask(text, base, n));
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_c;
}
// L: lines per record (4: FASTQ; 2: FASTA with the sequence on one line); the sequence is the record's second line
__global__ __launch_bounds__(256) void k_fq_ranges(const char* text, u64 n, const u64* tile_off, u64 n_tiles, u64* ranges, u64 max_seqs,
                                                   u64* n_seqs_out, u32 L) {
    __shared__ u32 s_w[4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * MCQ_FQ_TILE + (u64)tid * 16;
    u32 mask = fq_newline_mask(text, base, n);
    const u32 c = (u32)__builtin_popcount(mask);
    u32 incl = wave_incl_scan_dpp(c);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u32 woff = 0;
    for (u32 w = 0; w < wave; ++w) woff += s_w[w];
    u64 line = tile_off[blockIdx.x] + woff + incl - c;         // index of the line my first newline terminates
    while (mask) {
        const u32 j = (u32)__builtin_ctz(mask);
        mask &= mask - 1;
        const u64 p = base + j;
        const u64 rec = L == 4 ? line >> 2 : line >> 1;
        const u32 li = (u32)(line & (L - 1));
        if (rec < max_seqs) {
            if (li == 0) ranges[2 * rec] = p + 1;
            else if (li == 1) ranges[2 * rec + 1] = p;
        }
        ++line;
    }
    if (blockIdx.x == 0 && tid == 0) {
        const u64 total = tile_off[n_tiles];
        u64 ns = total >= 2 ? (total - 2) / L + 1 : 0;          // records whose sequence line is complete
        *n_seqs_out = ns < max_seqs ? ns : max_seqs;
    }
}

extern "C" uint32_t mcq_owner(uint32_t feature, uint32_t n_shards) {
    u32 x = feature;
    x = ((x >> 16) ^ x) * 0x45d9f3bu; x = ((x >> 16) ^ x) * 0x45d9f3bu; x = (x >> 16) ^ x;
    return (u32)(((u64)x * (n_shards ? n_shards : 1)) >> 32);
}

// [ceil(n/32) words of ambiguity bits][1 zero pad word]
static u64 packed_words2(u64 n) { return (n + 15) / 16; }
static u64 packed_wordsA(u64 n) { return (n + 31) / 32; }
extern "C" uint64_t mcq_packed_bytes(uint64_t n_bases) { return (packed_words2(n_bases) + 1 + packed_wordsA(n_bases) + 1) * 4; }

// device-side view of a batch whose buffers are (already) in device memory
int mcq::batch_dev(const mcq_batch* in, const char* d_bases, const u64* d_seq_off, BatchDev& b) {
    memset(&b, 0, sizeof(b));
    b.bases = d_bases; b.seq_off = d_seq_off; b.n_seq = in->n_seqs; b.nq = in->paired ? in->n_seqs / 2 : in->n_seqs;
    b.paired = in->paired ? 1 : 0;
    b.ranges = (in->flags & MCQ_BATCH_RANGES) ? 1 : 0;
    if (in->flags & MCQ_BATCH_PACKED) {
        if (b.ranges) return fail(MCQ_E_ARG, "MCQ_BATCH_PACKED and MCQ_BATCH_RANGES exclude each other");
        if (in->n_bases >= (1ull << 35)) return fail(MCQ_E_UNSUPPORTED, "packed batches hold fewer than 2^35 bases");
        b.packed = 1;
        b.last_word = (u32)packed_words2(in->n_bases);
        b.amb_off = b.last_word + 1;
        b.amb_last = (u32)packed_wordsA(in->n_bases);
    }
    return MCQ_OK;
}

// ASCII bases -> MCQ_BATCH_PACKED words; one thread per 32 bases
__global__ void k_pack_bases(const char* __restrict__ src, u64 n, u32* __restrict__ dst, u64 n2, u64 amb_off, u64 nA) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > nA) return;
    u32 w0 = 0, w1 = 0, am = 0;
    for (u32 j = 0; j < 32; ++j) {
        const u64 i = g * 32 + j;
        u32 code = 0, amb = 0;                                  // behind the end: code 0, not ambiguous (never looked at)
        if (i < n) {
            const u32 u = (u32)(unsigned char)src[i] & 0xDFu;
            code = (u >> 1) & 3u; code ^= code >> 1;
            amb = !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
            if (amb) code = 0;
        }
        if (j < 16) w0 |= code << (30 - 2 * j); else w1 |= code << (30 - 2 * (j - 16));
        am |= amb << (31 - j);
    }
    if (2 * g <= n2) dst[2 * g] = (2 * g < n2) ? w0 : 0u;      // index n2 is the zero pad word
    if (2 * g + 1 <= n2) dst[2 * g + 1] = (2 * g + 1 < n2) ? w1 : 0u;
    dst[amb_off + g] = g < nA ? am : 0u;
}

extern "C" int mcq_pack_bases(const char* bases, uint64_t n_bases, void* out, uint32_t flags, void* stream) {
    if (!out || (n_bases && !bases)) return fail(MCQ_E_ARG, "null argument");
    const u64 n2 = packed_words2(n_bases), nA = packed_wordsA(n_bases), amb_off = n2 + 1;
    if (flags & MCQ_DEVICE_PTRS) {
        hipLaunchKernelGGL(k_pack_bases, dim3((u32)((nA + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bases, n_bases, (u32*)out, n2, amb_off, nA);
        HIPCHK(hipGetLastError());
        return MCQ_OK;
    }
    u32* dst = (u32*)out;
    memset(dst, 0, mcq_packed_bytes(n_bases));
    for (u64 i = 0; i < n_bases; ++i) {
        const u32 u = (u32)(unsigned char)bases[i] & 0xDFu;
        u32 code = (u >> 1) & 3u; code ^= code >> 1;
        const bool amb = !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
        if (amb) dst[amb_off + (i >> 5)] |= 1u << (31 - (i & 31));
        else dst[i >> 4] |= code << (30 - 2 * (i & 15));
    }
    return MCQ_OK;
}

// ------------------------------------------------------------------ staged entry points (device pointers only)
extern "C" int mcq_count_windows(const mcq_db* db, const mcq_batch* in, uint64_t* win_off, void* stream) {
    if (!db || !in || !win_off) return fail(MCQ_E_ARG, "null argument");
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "staged entry points take device pointers");
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    const u64 n = in->n_seqs;
    u64* cnt = nullptr;
    HIPCHK(hipMallocAsync((void**)&cnt, std::max<u64>(1, n) * 8, st));
    if (n) hipLaunchKernelGGL(k_count_windows, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, in->seq_off, (in->flags & MCQ_BATCH_RANGES) ? 1u : 0u, n, db->d.winlen, db->d.winstride, cnt);
    { int rcs = device_exclusive_scan<u64>((const u64*)cnt, win_off, n, st, 256); if (rcs) return rcs; }
    HIPCHK(hipFreeAsync(cnt, st));
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_sketch(const mcq_db* db, const mcq_batch* in, const uint64_t* win_off,
                          uint32_t* features, uint32_t* n_feat, void* stream) {
    if (!db || !in || !win_off || !features || !n_feat) return fail(MCQ_E_ARG, "null argument");
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "staged entry points take device pointers");
    if (in->flags & MCQ_BATCH_PACKED) return fail(MCQ_E_ARG, "mcq_sketch takes ASCII batches");
    HIPCHK(hipSetDevice(db->device));
    if (in->n_seqs == 0) return MCQ_OK;
    // many short sequences (reads): one wave per sequence; few long ones (genomes): one wave per window
    if (in->n_seqs >= 4096) {
        const u32 grid = (u32)std::min<u64>((in->n_seqs + 3) / 4, 256ull * 32);    // short items: several rounds balance better
        hipLaunchKernelGGL(k_sketch_seqs, dim3(grid), dim3(256), 0, (hipStream_t)stream, db->d, in->bases, in->seq_off,
                           (in->flags & MCQ_BATCH_RANGES) ? 1u : 0u, in->n_seqs, win_off, features, n_feat);
    } else {
        hipLaunchKernelGGL(k_sketch_windows, dim3(256 * 16), dim3(256), 0, (hipStream_t)stream, db->d, in->bases, in->seq_off,
                           (in->flags & MCQ_BATCH_RANGES) ? 1u : 0u, in->n_seqs, win_off, features, n_feat);
    }
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_lookup_count(const mcq_db* db, const uint32_t* features, uint64_t n_features,
                                uint32_t* list_len, uint64_t* list_src, void* stream) {
    if (!db || (n_features && (!features || !list_len))) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(db->device));
    if (n_features == 0) return MCQ_OK;
    hipLaunchKernelGGL(k_lookup_count, dim3((u32)((n_features + 255) / 256)), dim3(256), 0, (hipStream_t)stream, db->d, features,
                       n_features, list_len, list_src);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_lookup_gather(const mcq_db* db, const uint32_t* features, uint64_t n_features,
                                 const uint32_t* list_len, const uint64_t* list_src,
                                 const uint64_t* out_off, void* out_locs, void* stream) {
    if (!db || (n_features && (!features || !out_off))) return fail(MCQ_E_ARG, "null argument");
    if (list_src && !list_len) return fail(MCQ_E_ARG, "list_src needs list_len");
    HIPCHK(hipSetDevice(db->device));
    if (n_features == 0) return MCQ_OK;
    u64 groups = (n_features + 63) / 64;
    const u32 grid = (u32)std::min<u64>((groups + 3) / 4, 256ull * 32);
    with_loc_form(db, [&](auto L) {
        using Key = typename decltype(L)::Key;
        hipLaunchKernelGGL(k_lookup_gather<Key>, dim3(grid), dim3(256), 0, (hipStream_t)stream, db->d, features, n_features, list_len, list_src, out_off, (Key*)out_locs);
    });
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

extern "C" int mcq_assemble(const mcq_db* db, uint64_t n_lists, const uint32_t* list_len, const uint32_t* src_slot,
                            uint64_t n_slots, const void* src_locs, const mcq_batch* in, const uint64_t* win_off,
                            uint64_t* loc_off, uint32_t* query_len, void* dst_locs, void* stream) {
    if (!db || !in || !win_off || !loc_off || !query_len) return fail(MCQ_E_ARG, "null argument");
    if (!(in->flags & MCQ_DEVICE_PTRS)) return fail(MCQ_E_ARG, "staged entry points take device pointers");
    if (n_lists && (!list_len || !src_slot)) return fail(MCQ_E_ARG, "null argument");
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    const u64 nq = in->paired ? in->n_seqs / 2 : in->n_seqs;
    u32* slot_len = nullptr; u64 *dst_off = nullptr, *src_off = nullptr;
    HIPCHK(hipMallocAsync((void**)&slot_len, std::max<u64>(1, n_slots) * 4, st));
    HIPCHK(hipMallocAsync((void**)&dst_off, (n_slots + 1) * 8, st));
    HIPCHK(hipMallocAsync((void**)&src_off, (n_lists + 1) * 8, st));
    HIPCHK(hipMemsetAsync(slot_len, 0, std::max<u64>(1, n_slots) * 4, st));
    if (n_lists) hipLaunchKernelGGL(k_scatter_len, dim3((u32)((n_lists + 255) / 256)), dim3(256), 0, st, list_len, src_slot, n_lists, slot_len);
    int rc = device_exclusive_scan<u32>(slot_len, dst_off, n_slots, st); if (rc) return rc;
    rc = device_exclusive_scan<u32>(list_len, src_off, n_lists, st); if (rc) return rc;
    if (n_lists) {
        u64 groups = (n_lists + 63) / 64;
        const u32 grid = (u32)std::min<u64>((groups + 3) / 4, 256ull * 32);
        with_loc_form(db, [&](auto L) {
            using Key = typename decltype(L)::Key;
            hipLaunchKernelGGL(k_scatter_lists<Key>, dim3(grid), dim3(256), 0, st, n_lists, (const u64*)src_off, src_slot, (const u64*)dst_off, (const Key*)src_locs, (Key*)dst_locs);
        });
    }
    hipLaunchKernelGGL(k_query_offsets, dim3((u32)((nq + 256) / 256)), dim3(256), 0, st, nq, in->paired ? 2u : 1u, db->d.s, win_off,
                       in->seq_off, (in->flags & MCQ_BATCH_RANGES) ? 1u : 0u, (const u64*)dst_off, n_slots, loc_off, query_len);
    HIPCHK(hipFreeAsync(slot_len, st)); HIPCHK(hipFreeAsync(dst_off, st)); HIPCHK(hipFreeAsync(src_off, st));
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

// ------------------------------------------------------------------ sharded-path routing entry points
extern "C" int mcq_bucket_features(const uint32_t* features, uint64_t n, uint32_t n_shards,
                                   uint64_t* counts, uint32_t* bucketed, uint32_t* src_index, void* stream) {
    if (!counts || (n && (!features || !bucketed || !src_index))) return fail(MCQ_E_ARG, "null argument");
    if (n_shards < 1 || n_shards > MCQ_BUCKET_MAX_SHARDS) return fail(MCQ_E_ARG, "n_shards must be 1..64");
    if (n >= (1ull << 32)) return fail(MCQ_E_UNSUPPORTED, "more than 2^32 feature slots in one batch");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { HIPCHK(hipMemsetAsync(counts, 0, (u64)n_shards * 8, st)); return MCQ_OK; }
    const u32 grid = (u32)std::min<u64>((n + 4095) / 4096, 2048);
    const u64 tile = ((n + grid - 1) / grid + 255) / 256 * 256;
    unsigned long long* blk = nullptr;
    HIPCHK(hipMallocAsync((void**)&blk, (u64)n_shards * grid * 8, st));
    hipLaunchKernelGGL(k_bucket_count, dim3(grid), dim3(256), 0, st, features, n, n_shards, tile, blk);
    hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(1024), 0, st, blk, n_shards, grid, (unsigned long long*)counts);
    hipLaunchKernelGGL(k_bucket_fill, dim3(grid), dim3(256), 0, st, features, n, n_shards, tile, (const unsigned long long*)blk, bucketed, src_index);
    HIPCHK(hipFreeAsync(blk, st));
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

// ------------------------------------------------------------------ row f4 entry point
static int text_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs, uint64_t* n_seqs_out, void* stream, u32 L);
extern "C" int mcq_fastq_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs,
                               uint64_t* n_seqs_out, void* stream) {
    return text_index(text, n_bytes, seq_ranges, max_seqs, n_seqs_out, stream, 4);
}
extern "C" int mcq_fasta_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs,
                               uint64_t* n_seqs_out, void* stream) {
    return text_index(text, n_bytes, seq_ranges, max_seqs, n_seqs_out, stream, 2);
}
static int text_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs, uint64_t* n_seqs_out, void* stream, u32 L) {
    if (!seq_ranges || !n_seqs_out || (n_bytes && !text)) return fail(MCQ_E_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const u64 n_tiles = std::max<u64>(1, (n_bytes + MCQ_FQ_TILE - 1) / MCQ_FQ_TILE);
    if (n_tiles >= (1ull << 31)) return fail(MCQ_E_UNSUPPORTED, "text too large for one call");
    u64 *cnt = nullptr, *off = nullptr;
    HIPCHK(hipMallocAsync((void**)&cnt, n_tiles * 8, st));
    HIPCHK(hipMallocAsync((void**)&off, (n_tiles + 1) * 8, st));
    hipLaunchKernelGGL(k_fq_count, dim3((u32)n_tiles), dim3(256), 0, st, text, n_bytes, cnt);
    int rc = device_exclusive_scan<u64>((const u64*)cnt, off, n_tiles, st); if (rc) return rc;
    hipLaunchKernelGGL(k_fq_ranges, dim3((u32)n_tiles), dim3(256), 0, st, text, n_bytes, (const u64*)off, n_tiles, seq_ranges, max_seqs, n_seqs_out, L);
    HIPCHK(hipFreeAsync(cnt, st)); HIPCHK(hipFreeAsync(off, st));
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}

// ------------------------------------------------------------------ read files: one chunk of text -> a compacted batch
// mcq_reads_prepare (include/mcq.h).  Per text: workgroup tiles of 4 KiB count their newlines and their header starts
// (a line that begins with '>') from 16-B loads; two scans number them; a second pass over the tiles writes the position of
// every newline and the line index of every header, and checks the strict form at every line start.  Then one thread per
// record measures its sequence, one workgroup scans the lengths into seq_off and applies max_queries / max_bases, and one
// wave per (query, mate) copies the sequence lines (a wave ballot finds the header's first ' ').  Byte positions are u32:
// a chunk is below 4 GiB.
// MCQ_READS_INTERLEAVED (P.inter): one text, numbered as above; record 2q + m is mate m of query q.  rlen then holds one
// length per PAIR (so the scratch of the single-text call is enough), the scan runs over pairs and writes seq_off[2q], and
// the copy kernel, which walks the mates' lines anyway, places mate 1 behind mate 0 and writes seq_off[2q + 1].
struct RdText {
    const char* t; u64 L; u32 eof, pad;
    u64 n_tiles, rcap;
    u64 *cnt_nl, *off_nl, *cnt_h, *off_h;   // [n_tiles] per-tile counts, [n_tiles + 1] exclusive offsets
    u32* nl;                                // [L + 1]     byte position of newline l
    u32* hl;                                // [L / 2 + 2] FASTA: line index of header r
    u32* rlen;                              // [rcap]      sequence length of record r
};
struct RdPair { RdText x[2]; u32 mates, inter; u64* info; };   // mates: texts; inter: mates are records 2q, 2q+1 of x[0]

__device__ __forceinline__ u32 rd_zero_bytes(u32 m) {                  // bit i = byte i of m is zero (exact)
    const u32 z = ~(((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u;
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
// among t[base .. base+16): newlines (nlm), line starts (lsm) and line starts on a '>' (hsm)
__device__ __forceinline__ void rd_masks(const char* __restrict__ t, u64 base, u64 n, u32& nlm, u32& lsm, u32& hsm) {
    nlm = 0; hsm = 0;
    if (base + 16 <= n && ((reinterpret_cast<uintptr_t>(t) + base) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(t + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nlm |= rd_zero_bytes(w[i] ^ 0x0A0A0A0Au) << (4 * i);
            hsm |= rd_zero_bytes(w[i] ^ 0x3E3E3E3Eu) << (4 * i);
        }
    } else {
        for (u32 j = 0; j < 16; ++j)
            if (base + j < n) { const char c = t[base + j]; nlm |= (u32)(c == '\n') << j; hsm |= (u32)(c == '>') << j; }
    }
    const u32 valid = base >= n ? 0u : (n - base >= 16 ? 0xFFFFu : (1u << (n - base)) - 1u);
    const u32 prev = base == 0 ? 1u : (base < n ? (u32)(t[base - 1] == '\n') : 0u);
    lsm = ((nlm << 1) | prev) & valid;
    hsm &= lsm;
}
__device__ __forceinline__ const RdText& rd_pick(const RdPair& P, u32 y) { return y ? P.x[1] : P.x[0]; }

__global__ __launch_bounds__(256) void k_rd_count(RdPair P) {
    const RdText X = rd_pick(P, blockIdx.y);
    if (blockIdx.x >= X.n_tiles) return;
    __shared__ u32 s_c[2];
    if (threadIdx.x == 0) { s_c[0] = 0; s_c[1] = 0; }
    __syncthreads();
    u32 nlm, lsm, hsm;
    rd_masks(X.t, (u64)blockIdx.x * MCQ_FQ_TILE + (u64)threadIdx.x * 16, X.L, nlm, lsm, hsm);
    u32 a = (u32)__builtin_popcount(nlm), b = (u32)__builtin_popcount(hsm);
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { if (a) atomicAdd(&s_c[0], a); if (b) atomicAdd(&s_c[1], b); }
    __syncthreads();
    if (threadIdx.x == 0) { X.cnt_nl[blockIdx.x] = s_c[0]; X.cnt_h[blockIdx.x] = s_c[1]; }
}

__global__ __launch_bounds__(256) void k_rd_lines(RdPair P) {
    const RdText X = rd_pick(P, blockIdx.y);
    if (blockIdx.x >= X.n_tiles) return;
    __shared__ u32 s_w[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 base = (u64)blockIdx.x * MCQ_FQ_TILE + (u64)tid * 16;
    u32 nlm, lsm, hsm;
    rd_masks(X.t, base, X.L, nlm, lsm, hsm);
    const u32 cn = (u32)__builtin_popcount(nlm), ch = (u32)__builtin_popcount(hsm);
    const u32 in = wave_incl_scan_dpp(cn), ih = wave_incl_scan_dpp(ch);
    if (lane == 63) { s_w[0][wave] = in; s_w[1][wave] = ih; }
    __syncthreads();
    u32 wn = 0, wh = 0;
    for (u32 w = 0; w < wave; ++w) { wn += s_w[0][w]; wh += s_w[1][w]; }
    const u64 line0 = X.off_nl[blockIdx.x] + wn + in - cn;             // the line that text[base] belongs to
    const u64 hdr0 = X.off_h[blockIdx.x] + wh + ih - ch;
    bool bad = false;
    for (u32 m = nlm, l = 0; m; m &= m - 1, ++l) {
        const u64 at = base + (u32)__builtin_ctz(m);
        X.nl[line0 + l] = (u32)at;
        bad |= P.inter && at > 0 && X.t[at - 1] == '\r';               // (interleaved: a line that ends in '\r' goes to the host, include/mcq.h)
    }
    const char f = X.L ? X.t[0] : 0;
    for (u32 m = lsm; m; m &= m - 1) {
        const u32 j = (u32)__builtin_ctz(m), below = (1u << j) - 1u;
        const u64 li = line0 + (u32)__builtin_popcount(nlm & below);
        const char c = X.t[base + j];
        if (f == '@') {                                                 // FASTQ: line 4r starts with '@', line 4r+2 with '+'
            const u32 role = (u32)(li & 3);
            bad |= (role == 0 && c != '@') || (role == 2 && c != '+');
        } else if (f == '>') {                                          // FASTA: no empty line, no FASTQ record
            bad |= c == '\n' || c == '@';
            if (c == '>') X.hl[hdr0 + (u32)__builtin_popcount(hsm & below)] = (u32)li;
        } else bad = true;
    }
    if (bad) P.info[MCQ_READS_STATUS] = MCQ_READS_NOT_STRICT;
}

struct RdCounts { u64 nnl, n_lines, n_rec; bool fq; };
__device__ __forceinline__ RdCounts rd_counts(const RdText& X) {
    RdCounts c;
    c.nnl = X.off_nl[X.n_tiles];
    c.n_lines = c.nnl + (X.L && X.t[X.L - 1] != '\n' ? 1 : 0);
    const char f = X.L ? X.t[0] : 0;
    c.fq = f == '@';
    c.n_rec = c.fq ? (c.n_lines + 3) / 4 : (f == '>' ? X.off_h[X.n_tiles] : 0);
    return c;
}
__device__ __forceinline__ u64 rd_line_start(const RdText& X, u64 l) { return l ? (u64)X.nl[l - 1] + 1 : 0; }
__device__ __forceinline__ u64 rd_line_end(const RdText& X, const RdCounts& c, u64 l) { return l < c.nnl ? (u64)X.nl[l] : X.L; }
__device__ __forceinline__ u64 rd_hdr_line(const RdText& X, const RdCounts& c, u64 r) { return c.fq ? 4 * r : (u64)X.hl[r]; }
// lines [a, b) that hold the sequence of record r
__device__ __forceinline__ void rd_seq_lines(const RdText& X, const RdCounts& c, u64 r, u64& a, u64& b) {
    if (c.fq) { a = 4 * r + 1; b = a + 1; }
    else { a = (u64)X.hl[r] + 1; b = r + 1 < c.n_rec ? (u64)X.hl[r + 1] : c.n_lines; }
    if (b > c.n_lines) b = c.n_lines;
    if (a > b) a = b;
}

// sequence length of record r (0 for a record the text does not hold)
__device__ __forceinline__ u32 rd_rec_len(const RdText& X, const RdCounts& c, u64 r) {
    if (r >= c.n_rec) return 0u;
    u64 a, b;
    rd_seq_lines(X, c, r, a, b);
    return b > a ? (u32)(rd_line_end(X, c, b - 1) - rd_line_start(X, a) - (b - 1 - a)) : 0u;
}

// rlen[i]: the length of record i, or (interleaved) of the pair of records 2i, 2i+1
__global__ __launch_bounds__(256) void k_rd_recs(RdPair P) {
    const RdText X = rd_pick(P, blockIdx.y);
    const RdCounts c = rd_counts(X);
    const u64 items = P.inter ? (c.n_rec + 1) / 2 : c.n_rec;
    const u64 n = items < X.rcap ? items : X.rcap;
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (u64)gridDim.x * blockDim.x)
        X.rlen[r] = P.inter ? rd_rec_len(X, c, 2 * r) + rd_rec_len(X, c, 2 * r + 1) : rd_rec_len(X, c, r);
}

// one workgroup: complete records per text, the queries taken, seq_off, the cut points
#define MCQ_RD_PER_THREAD 8
__global__ __launch_bounds__(1024) void k_rd_offsets(RdPair P, u64 max_queries, u64 max_bases, u64* seq_off) {
    __shared__ u64 s_w[16];
    __shared__ u64 s_carry, s_endmax, s_end0;
    __shared__ u32 s_k;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 mates = P.mates;                                         // items of the scan per query (interleaved: one, a pair's length)
    const u32 ostride = P.inter ? 2u : 1u;                             // ... and seq_off entries per item
    RdCounts c[2];
    u64 complete[2] = {0, 0};
    bool bad = false;
#pragma unroll
    for (u32 m = 0; m < 2; ++m) {                                      // (unrolled: c[] and complete[] stay in registers)
        if (m >= mates) break;
        const RdText& X = P.x[m];
        c[m] = rd_counts(X);
        if (c[m].n_rec == 0) continue;
        bool last = X.eof != 0;                                        // FASTA: the last record ends with the file
        if (c[m].fq) {                                                 // FASTQ: its fourth line, and the byte after it, are here
            const u64 l3 = 4 * (c[m].n_rec - 1) + 3;
            last = X.eof ? l3 < c[m].n_lines : (l3 < c[m].nnl && (u64)X.nl[l3] + 1 < X.L);
            bad |= X.eof && (c[m].n_lines & 3) != 0;                   // a cut last record
        }
        bad |= P.inter && X.eof && X.t[X.L - 1] == '\r';                // (interleaved: a last line that ends in '\r' as well, see k_rd_lines)
        complete[m] = c[m].n_rec - (last ? 0 : 1);
    }
    // interleaved: a query is two complete records, or the last record alone where the file ends (the second next() of
    // sequence_pair_reader::next, src/sequence_io.cpp:442-462, then gives an empty sequence)
    if (P.inter) complete[0] = complete[0] / 2 + ((P.x[0].eof && complete[0] == c[0].n_rec) ? (complete[0] & 1) : 0);
    u64 nq = complete[0];
    if (mates == 2 && complete[1] < nq) nq = complete[1];
    if (P.x[0].rcap < nq) nq = P.x[0].rcap;
    if (mates == 2 && P.x[1].rcap < nq) nq = P.x[1].rcap;
    if (max_queries < nq) nq = max_queries;
    const u64 ns = nq * mates;
    if (tid == 0) { s_carry = 0; s_endmax = 0; s_end0 = 0; s_k = 0; }
    __syncthreads();
    const u32* rlen0 = P.x[0].rlen;
    const u32* rlen1 = P.x[1].rlen;
    for (u64 base = 0; base < ns; base += 1024 * MCQ_RD_PER_THREAD) {
        const u64 i0 = base + (u64)tid * MCQ_RD_PER_THREAD;
        u32 len[MCQ_RD_PER_THREAD];
        u64 tot = 0;
#pragma unroll
        for (int k = 0; k < MCQ_RD_PER_THREAD; ++k) {
            const u64 i = i0 + k;
            len[k] = i >= ns ? 0u : (mates == 1 ? rlen0[i] : ((i & 1) ? rlen1 : rlen0)[i >> 1]);
            tot += len[k];
        }
        u64 x = tot;
        for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_up(x, d, 64); if (lane >= (u32)d) x += t; }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        u64 off = s_carry;
        for (u32 w = 0; w < wave; ++w) off += s_w[w];
        off += x - tot;
        u32 k_fit = 0; u64 end_fit = 0;                                // this thread's last query that ends within max_bases
#pragma unroll
        for (int k = 0; k < MCQ_RD_PER_THREAD; ++k) {
            const u64 i = i0 + k;
            if (i < ns) {
                seq_off[i * ostride] = off;
                const u64 end = off + len[k];
                if (i % mates == mates - 1) {                          // the end of query q
                    const u64 q = i / mates;
                    if (end <= max_bases) { k_fit = (u32)(q + 1); end_fit = end; }
                    if (q == 0) s_end0 = end;
                }
            }
            off += len[k];
        }
        for (int d = 32; d > 0; d >>= 1) {                             // (the ends grow with q: the largest q has the largest end)
            const u32 ko = __shfl_xor(k_fit, d, 64);
            const u64 eo = __shfl_xor(end_fit, d, 64);
            if (ko > k_fit) { k_fit = ko; end_fit = eo; }
        }
        if (lane == 0 && k_fit) { atomicMax(&s_k, k_fit); atomicMax((unsigned long long*)&s_endmax, (unsigned long long)end_fit); }
        __syncthreads();
        if (tid == 1023) s_carry = off;
        __syncthreads();
    }
    if (tid == 0) {
        u64 n = s_k, nb = s_endmax;
        if (n == 0 && nq) { n = 1; nb = s_end0; }                      // one query larger than max_bases goes alone
        seq_off[n * mates * ostride] = nb;
        u64* info = P.info;
        info[MCQ_READS_N] = n; info[MCQ_READS_BASES] = nb;
#pragma unroll
        for (u32 m = 0; m < 2; ++m) {
            if (m >= mates) break;
            const RdText& X = P.x[m];
            const u64 rn = n * ostride;                                 // the first record not taken
            info[MCQ_READS_CUT1 + m] = rn < c[m].n_rec ? rd_line_start(X, rd_hdr_line(X, c[m], rn)) : X.L;
            info[MCQ_READS_COMPLETE1 + m] = complete[m] < max_queries ? complete[m] : max_queries;
        }
        if (bad) info[MCQ_READS_STATUS] = MCQ_READS_NOT_STRICT;
    }
}

// one wave per (query, mate): the sequence lines into bases, and (mate 0) the header's first token
__global__ __launch_bounds__(256) void k_rd_copy(RdPair P, u64* seq_off, char* bases, u64* hdr) {
    const u32 m = blockIdx.y, lane = threadIdx.x & 63, inter = P.inter, mates = inter ? 2u : P.mates;
    const RdText X = rd_pick(P, inter ? 0u : m);
    const RdCounts c = rd_counts(X);
    const u64 n = P.info[MCQ_READS_N];
    for (u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (u64)gridDim.x * 4) {
        const u64 r = inter ? 2 * q + m : q;                           // the record that is mate m of query q
        char* dst;
        if (inter) {                                                   // the scan placed the pair: mate 1 lies behind mate 0
            const u64 o1 = seq_off[2 * q] + rd_rec_len(X, c, 2 * q);
            if (m == 0 && lane == 0) seq_off[2 * q + 1] = o1;
            dst = bases + (m ? o1 : seq_off[2 * q]);
        } else dst = bases + seq_off[q * mates + m];
        u64 a = 0, b = 0;
        if (r < c.n_rec) rd_seq_lines(X, c, r, a, b);                  // (an unpaired last record has no second mate)
        for (u64 l = a; l < b; ++l) {
            const u64 s = rd_line_start(X, l), len = rd_line_end(X, c, l) - s;
            for (u64 i = lane; i < len; i += 64) dst[i] = X.t[s + i];
            dst += len;
        }
        if (m == 0) {
            const u64 h = rd_hdr_line(X, c, r), hs = rd_line_start(X, h) + 1, he = rd_line_end(X, c, h);
            u64 end = he;
            for (u64 p = hs; p < he; p += 64) {
                const unsigned long long sp = __ballot(p + lane < he && X.t[p + lane] == ' ');
                if (sp) { end = p + (u64)__builtin_ctzll(sp); break; }
            }
            if (lane == 0) { hdr[2 * q] = hs; hdr[2 * q + 1] = end; }
        }
    }
}

static u64 rd_align(u64 x) { return (x + 255) & ~255ull; }
static u64 rd_tiles(u64 L) { return std::max<u64>(1, (L + MCQ_FQ_TILE - 1) / MCQ_FQ_TILE); }
static u64 rd_rcap(u64 L, u64 max_queries) { return std::min<u64>(max_queries, L / 2 + 2); }
static u64 rd_text_bytes(u64 L, u64 max_queries) {
    const u64 nt = rd_tiles(L);
    return 2 * rd_align(nt * 8) + 2 * rd_align((nt + 1) * 8) + rd_align((L + 1) * 4) + rd_align((L / 2 + 2) * 4) + rd_align(rd_rcap(L, max_queries) * 4);
}
extern "C" uint64_t mcq_reads_scratch_bytes(uint64_t len1, uint64_t len2, uint64_t max_queries) {
    return rd_text_bytes(len1, max_queries) + rd_text_bytes(len2, max_queries);
}

extern "C" int mcq_reads_prepare(const char* text1, uint64_t len1, const char* text2, uint64_t len2, uint32_t flags,
                                 uint64_t max_queries, uint64_t max_bases, void* scratch, uint64_t scratch_bytes,
                                 char* bases, uint64_t* seq_off, uint64_t* hdr, uint64_t* info, void* stream) {
    if ((len1 && !text1) || (len2 && !text2) || !scratch || !bases || !seq_off || !hdr || !info) return fail(MCQ_E_ARG, "null argument");
    if (max_queries < 1) return fail(MCQ_E_ARG, "max_queries must be >= 1");
    if (len1 >= 0xFFFFFFFFull || len2 >= 0xFFFFFFFFull) return fail(MCQ_E_UNSUPPORTED, "a chunk of read text is below 4 GiB");
    if (scratch_bytes < mcq_reads_scratch_bytes(len1, len2, max_queries)) return fail(MCQ_E_ARG, "scratch smaller than mcq_reads_scratch_bytes");
    const bool inter = (flags & MCQ_READS_INTERLEAVED) != 0;
    if (inter && (text2 || len2)) return fail(MCQ_E_ARG, "MCQ_READS_INTERLEAVED is given with text2 == NULL");
    hipStream_t st = (hipStream_t)stream;
    RdPair P; memset(&P, 0, sizeof(P));
    P.mates = text2 ? 2 : 1; P.inter = inter ? 1 : 0; P.info = info;
    char* s = (char*)scratch;
    auto take = [&](u64 bytes) { char* p = s; s += rd_align(bytes); return p; };
    const char* tx[2] = {text1, text2};
    const u64 lx[2] = {len1, len2};
    u64 tiles = 1, qcap = max_queries;
    for (u32 m = 0; m < 2; ++m) {
        RdText& X = P.x[m];
        X.t = tx[m]; X.L = lx[m]; X.eof = (flags >> m) & 1u;
        X.n_tiles = rd_tiles(X.L); X.rcap = rd_rcap(X.L, max_queries);
        X.cnt_nl = (u64*)take(X.n_tiles * 8); X.cnt_h = (u64*)take(X.n_tiles * 8);
        X.off_nl = (u64*)take((X.n_tiles + 1) * 8); X.off_h = (u64*)take((X.n_tiles + 1) * 8);
        X.nl = (u32*)take((X.L + 1) * 4); X.hl = (u32*)take((X.L / 2 + 2) * 4); X.rlen = (u32*)take(X.rcap * 4);
        if (m < P.mates) { tiles = std::max(tiles, X.n_tiles); qcap = std::min(qcap, X.rcap); }
    }
    if (tiles >= (1ull << 31)) return fail(MCQ_E_UNSUPPORTED, "text too large for one call");
    HIPCHK(hipMemsetAsync(info, 0, MCQ_READS_INFO_WORDS * 8, st));
    hipLaunchKernelGGL(k_rd_count, dim3((u32)tiles, P.mates), dim3(256), 0, st, P);
    for (u32 m = 0; m < P.mates; ++m) {
        int rc = device_exclusive_scan<u64>((const u64*)P.x[m].cnt_nl, P.x[m].off_nl, P.x[m].n_tiles, st); if (rc) return rc;
        rc = device_exclusive_scan<u64>((const u64*)P.x[m].cnt_h, P.x[m].off_h, P.x[m].n_tiles, st); if (rc) return rc;
    }
    hipLaunchKernelGGL(k_rd_lines, dim3((u32)tiles, P.mates), dim3(256), 0, st, P);
    const u64 rmax = std::max(P.x[0].rcap, P.mates == 2 ? P.x[1].rcap : 0);
    hipLaunchKernelGGL(k_rd_recs, dim3((u32)std::min<u64>((rmax + 255) / 256, 1024), P.mates), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_rd_offsets, dim3(1), dim3(1024), 0, st, P, max_queries, max_bases, seq_off);
    hipLaunchKernelGGL(k_rd_copy, dim3((u32)std::min<u64>((qcap + 3) / 4, 2048), inter ? 2 : P.mates), dim3(256), 0, st, P, seq_off, bases, hdr);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}
