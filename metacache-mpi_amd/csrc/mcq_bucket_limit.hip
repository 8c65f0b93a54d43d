// mcq_bucket_limit.hip -- the reference's query-time bucket rules on a chunk of (feature, target, window) triples
// (mcq_bucket_limit of include/mcq.h).
//
// Restates, per (feature, rank) bucket, what `metacache_mpi query` does to every rank's table right after reading it
// (src/mode_query.cpp:354-377): remove_features_with_more_locations_than (src/sketch_database.h:381-395: a bucket of more than
// `remove_above` locations is cleared) and then max_locations_per_feature (src/sketch_database.h:356-368: a bucket of more
// than `keep_first` locations is shrunk to its first `keep_first`).  A chunk is what mcq_shard_stream_next hands out -- whole key
// records of one shard file --, so a maximal run of equal features is one bucket of one rank.
//
// Shape: memory-bound, 12 B read and at most 12 B written per triple; three launches over tiles of BL_TILE triples.
//   k_bl_mark     per triple the start and the end of its run: the run heads of the tile as a bit mask in LDS, the nearest head at
//                 or below / above the triple by a bit scan; a run that crosses the tile's edge is followed into the neighbouring
//                 tiles by the tile's first wave, 64 triples a step (runs are at most 255 long in real files, any length is right).
//                 From (position in run, run length) the keep flag; a wave's 64 flags are one 64-bit word (a ballot), the tile's
//                 kept triples one count; the run's first triple counts its bucket as shrunk or removed.
//   k_bl_scan     exclusive scan of the tile counts (one workgroup; a 4 M chunk has 2048 tiles), the total is n_out.
//   k_bl_compact  a tile's kept triples to tile offset + rank inside the tile (popcounts of the flag words): the reads are
//                 coalesced, the writes of a wave go to one contiguous stretch.
// Out of place into scratch, then (device pointers) k_bl_copy_back brings the n_out triples to the front of the caller's
// arrays.  Counters take one ordinary atomic add per tile; every store is a plain vector store.
// The scratch is the caller's (mcq_bucket_limit_ws: what the streaming loader calls, with a buffer the builder owns) or comes
// from the device's stream-ordered pool (mcq_bucket_limit); DESIGN.md section 31 says why the builder does not use the pool.
#include "mcq_internal.hpp"

namespace {
constexpr u32 BL_TB = 256;                 // threads per workgroup: 4 waves
constexpr u32 BL_TILE = 2048;              // triples per workgroup: every wave takes 512 contiguous ones, 64 a step
constexpr u32 BL_WORDS = BL_TILE / 64;     // flag words per tile
constexpr u32 BL_WAVE_SPAN = BL_TILE / (BL_TB / 64);

// counts[0] = n_out, [1] = buckets shrunk, [2] = buckets removed
__global__ __launch_bounds__(BL_TB) void k_bl_mark(const u32* __restrict__ feat, u64 n, u32 keep_first, u32 remove_above,
                                                    unsigned long long* __restrict__ mask, u32* __restrict__ tile_cnt,
                                                    unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long heads[BL_WORDS];     // bit j of word w: triple w * 64 + j of the tile starts a run
    __shared__ u64 ext[2];                              // triples of the tile's first run before the tile, of its last run behind it
    __shared__ u32 blk[3];                              // kept triples, buckets shrunk, buckets removed
    const u64 t0 = (u64)blockIdx.x * BL_TILE;
    const u64 t1 = (t0 + BL_TILE < n) ? t0 + BL_TILE : n;     // (t0 < n: the grid has ceil(n / BL_TILE) workgroups)
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) blk[threadIdx.x] = 0;
    // the run heads of the tile
    for (u32 it = 0; it < BL_WAVE_SPAN / 64; ++it) {
        const u64 i = t0 + wave * BL_WAVE_SPAN + it * 64 + lane;
        const bool head = i < t1 && (i == 0 || feat[i - 1] != feat[i]);
        const unsigned long long m = __ballot(head);
        if (lane == 0) heads[wave * (BL_WAVE_SPAN / 64) + it] = m;
    }
    // the runs that cross the tile's edges, followed by the first wave
    if (wave == 0) {
        const u32 f0 = feat[t0], fl = feat[t1 - 1];
        u64 back = 0, fwd = 0;
        for (u64 j = t0; j > 0;) {                      // triples j - 1, j - 2, ... equal to the tile's first
            const bool eq = (j > lane) && feat[j - 1 - lane] == f0;
            const unsigned long long m = __ballot(eq);
            if (m == ~0ull) { back += 64; j -= 64; continue; }      // (all 64 equal: j >= 64)
            back += (u32)__builtin_ctzll(~m);
            break;
        }
        for (u64 j = t1; j < n;) {                      // triples j, j + 1, ... equal to the tile's last
            const bool eq = (j + lane < n) && feat[j + lane] == fl;
            const unsigned long long m = __ballot(eq);
            if (m == ~0ull) { fwd += 64; j += 64; continue; }
            fwd += (u32)__builtin_ctzll(~m);
            break;
        }
        if (lane == 0) { ext[0] = back; ext[1] = fwd; }
    }
    __syncthreads();
    u32 kept = 0, shrunk = 0, removed = 0;
    for (u32 it = 0; it < BL_WAVE_SPAN / 64; ++it) {
        const u32 w = wave * (BL_WAVE_SPAN / 64) + it;
        const u64 i = t0 + (u64)w * 64 + lane;
        bool keep = false;
        if (i < t1) {
            // start: the nearest head at or below the triple; none in the tile: the run began ext[0] triples before it
            u64 start;
            {
                unsigned long long m = heads[w] & (~0ull >> (63 - lane));
                int ww = (int)w;
                while (!m && ww > 0) m = heads[--ww];
                start = m ? t0 + (u64)ww * 64 + (63 - (u32)__builtin_clzll(m)) : t0 - ext[0];
            }
            // end (exclusive): the nearest head above it; none in the tile: the run goes on ext[1] triples behind it
            u64 end;
            {
                unsigned long long m = lane == 63 ? 0ull : heads[w] & (~0ull << (lane + 1));
                u32 ww = w;
                while (!m && ww + 1 < BL_WORDS) m = heads[++ww];
                end = m ? t0 + (u64)ww * 64 + (u32)__builtin_ctzll(m) : t1 + ext[1];
            }
            const u64 len = end - start, pos = i - start;
            const bool rem = remove_above && len > remove_above;
            const bool cut = !rem && keep_first && len > keep_first;
            keep = !rem && !(cut && pos >= keep_first);
            if (pos == 0) { shrunk += cut; removed += rem; }
        }
        const unsigned long long km = __ballot(keep);
        if (lane == 0) { mask[t0 / 64 + w] = km; kept += (u32)__builtin_popcountll(km); }
    }
    if (kept) atomicAdd(&blk[0], kept);
    if (shrunk) atomicAdd(&blk[1], shrunk);
    if (removed) atomicAdd(&blk[2], removed);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = blk[0];
        if (blk[1]) atomicAdd(&counts[1], (unsigned long long)blk[1]);
        if (blk[2]) atomicAdd(&counts[2], (unsigned long long)blk[2]);
    }
}

// tile_off[t] = sum of tile_cnt[0 .. t), counts[0] = the total; one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void k_bl_scan(const u32* __restrict__ tile_cnt, u64 n_tiles, u64* __restrict__ tile_off,
                                                   unsigned long long* __restrict__ counts) {
    __shared__ u64 wsum[16];
    __shared__ u64 carry_s;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (u64 base = 0; base < n_tiles; base += 1024) {
        const u64 t = base + threadIdx.x;
        const u64 v = t < n_tiles ? tile_cnt[t] : 0;
        u64 incl = v;
        for (u32 d = 1; d < 64; d <<= 1) { const u64 o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u64 before = carry_s;
        for (u32 w = 0; w < wave; ++w) before += wsum[w];
        if (t < n_tiles) tile_off[t] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[0] = carry_s;
}

__global__ __launch_bounds__(BL_TB) void k_bl_compact(const u32* __restrict__ feat, const u32* __restrict__ tgt, const u32* __restrict__ win,
                                                       u64 n, const unsigned long long* __restrict__ mask, u64 n_words,
                                                       const u64* __restrict__ tile_off, u32* __restrict__ of, u32* __restrict__ ot,
                                                       u32* __restrict__ ow) {
    const u64 t0 = (u64)blockIdx.x * BL_TILE;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // every wave: lane l < BL_WORDS holds flag word l of the tile and the kept triples before it
    const u64 wi = t0 / 64 + lane;
    const unsigned long long word = (lane < BL_WORDS && wi < n_words) ? mask[wi] : 0ull;
    const u32 pc = (u32)__builtin_popcountll(word);
    u32 incl = pc;
    for (u32 d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    const u32 excl = incl - pc;
    const u64 base = tile_off[blockIdx.x];
    for (u32 it = 0; it < BL_WAVE_SPAN / 64; ++it) {
        const u32 w = wave * (BL_WAVE_SPAN / 64) + it;
        const unsigned long long m = __shfl(word, (int)w, 64);
        const u32 before = __shfl(excl, (int)w, 64);
        const u64 i = t0 + (u64)w * 64 + lane;
        if (i < n && ((m >> lane) & 1ull)) {
            const u64 dst = base + before + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));    // < n_out <= n
            of[dst] = feat[i]; ot[dst] = tgt[i]; ow[dst] = win[i];
        }
    }
}

__global__ void k_bl_copy_back(const u32* __restrict__ sf, const u32* __restrict__ st, const u32* __restrict__ sw,
                               const unsigned long long* __restrict__ counts, u64 n, u32* __restrict__ feat, u32* __restrict__ tgt,
                               u32* __restrict__ win) {
    u64 m = counts[0]; if (m > n) m = n;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) { feat[i] = sf[i]; tgt[i] = st[i]; win[i] = sw[i]; }
}

// the scratch of one call: stream-ordered, given back on every way out
struct BlScratch {
    hipStream_t s; std::vector<void*> live;
    explicit BlScratch(hipStream_t s_) : s(s_) {}
    template <class T> hipError_t get(T** p, u64 bytes) {
        void* q = nullptr;
        const hipError_t e = hipMallocAsync(&q, bytes ? bytes : 1, s);
        if (e == hipSuccess) { live.push_back(q); *p = static_cast<T*>(q); }
        return e;
    }
    ~BlScratch() { for (void* p : live) (void)hipFreeAsync(p, s); }
};


// the buffers of one run besides the caller's arrays; bl_enqueue launches the three kernels into them
struct BlBuffers { u32 *of, *ot, *ow, *tile_cnt; unsigned long long *mask, *counts; u64* tile_off; };
inline u64 bl_align(u64 b) { return (b + 255) & ~255ull; }
inline u64 bl_tiles(u64 n) { return (n + BL_TILE - 1) / BL_TILE; }
int bl_enqueue(const u32* df, const u32* dt, const u32* dw, u64 n, u32 keep_first, u32 remove_above, const BlBuffers& b, hipStream_t s) {
    const u64 n_tiles = bl_tiles(n);
    HIPCHK(hipMemsetAsync(b.counts, 0, 3 * 8, s));
    hipLaunchKernelGGL(k_bl_mark, dim3((u32)n_tiles), dim3(BL_TB), 0, s, df, n, keep_first, remove_above, b.mask, b.tile_cnt, b.counts);
    hipLaunchKernelGGL(k_bl_scan, dim3(1), dim3(1024), 0, s, (const u32*)b.tile_cnt, n_tiles, b.tile_off, b.counts);
    hipLaunchKernelGGL(k_bl_compact, dim3((u32)n_tiles), dim3(BL_TB), 0, s, df, dt, dw, n, (const unsigned long long*)b.mask, n_tiles * BL_WORDS,
                       (const u64*)b.tile_off, b.of, b.ot, b.ow);
    HIPCHK(hipGetLastError());
    return MCQ_OK;
}
int bl_check(const void* feat, const void* tgt, const void* win, u64 n, u32 keep_first, const void* a, const void* b, const void* c) {
    if (!a || !b || !c) return fail(MCQ_E_ARG, "null argument");
    if (n && (!feat || !tgt || !win)) return fail(MCQ_E_ARG, "null argument");
    if (keep_first > 255) return fail(MCQ_E_ARG, "keep_first must be in 0..255");
    if (n >= (1ull << 40)) return fail(MCQ_E_UNSUPPORTED, "a chunk holds fewer than 2^40 triples");
    return MCQ_OK;
}
}  // namespace

extern "C" uint64_t mcq_bucket_limit_scratch_bytes(uint64_t n) {
    const u64 n_tiles = bl_tiles(n);
    return 3 * bl_align(n * 4) + bl_align(n_tiles * BL_WORDS * 8) + bl_align(n_tiles * 4) + bl_align(n_tiles * 8) + 256;
}

extern "C" int mcq_bucket_limit_ws(uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t n, uint32_t keep_first, uint32_t remove_above,
                                   int32_t device, void* stream, void* scratch, uint64_t scratch_bytes, uint64_t* counts_out) {
    { const int rc = bl_check(feat, tgt, win, n, keep_first, counts_out, counts_out, counts_out); if (rc) return rc; }
    if (!n || (!keep_first && !remove_above)) { counts_out[0] = n; counts_out[1] = counts_out[2] = 0; return MCQ_OK; }
    if (!scratch || scratch_bytes < mcq_bucket_limit_scratch_bytes(n)) return fail(MCQ_E_ARG, "scratch smaller than mcq_bucket_limit_scratch_bytes(n)");
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const u64 n_tiles = bl_tiles(n);
    char* p = (char*)scratch;
    BlBuffers b;
    b.of = (u32*)p; p += bl_align(n * 4); b.ot = (u32*)p; p += bl_align(n * 4); b.ow = (u32*)p; p += bl_align(n * 4);
    b.mask = (unsigned long long*)p; p += bl_align(n_tiles * BL_WORDS * 8);          // (whole tiles: k_bl_mark writes every word of its tile)
    b.tile_cnt = (u32*)p; p += bl_align(n_tiles * 4);
    b.tile_off = (u64*)p; p += bl_align(n_tiles * 8);
    b.counts = (unsigned long long*)p;
    { const int rc = bl_enqueue(feat, tgt, win, n, keep_first, remove_above, b, s); if (rc) return rc; }
    const u64 g = (n + 255) / 256;
    hipLaunchKernelGGL(k_bl_copy_back, dim3((u32)(g < 4096 ? g : 4096)), dim3(256), 0, s, (const u32*)b.of, (const u32*)b.ot, (const u32*)b.ow,
                       (const unsigned long long*)b.counts, n, feat, tgt, win);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts_out, b.counts, 3 * 8, hipMemcpyDeviceToHost, s));     // (in stream order: the caller synchronises)
    return MCQ_OK;
}

extern "C" int mcq_bucket_limit(uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t n, uint32_t keep_first, uint32_t remove_above,
                                uint32_t flags, int32_t device, void* stream, uint64_t* n_out, uint64_t* n_shrunk, uint64_t* n_removed) {
    { const int rc = bl_check(feat, tgt, win, n, keep_first, n_out, n_shrunk, n_removed); if (rc) return rc; }
    *n_out = n; *n_shrunk = 0; *n_removed = 0;
    if (!n || (!keep_first && !remove_above)) return MCQ_OK;
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const bool dev = (flags & MCQ_DEVICE_PTRS) != 0;
    const u64 n_tiles = bl_tiles(n);
    BlScratch tmp(s);
    u32 *df = feat, *dt = tgt, *dw = win;
    BlBuffers b;
    if (!dev) {
        HIPCHK(tmp.get(&df, n * 4)); HIPCHK(tmp.get(&dt, n * 4)); HIPCHK(tmp.get(&dw, n * 4));
        HIPCHK(hipMemcpyAsync(df, feat, n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dt, tgt, n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dw, win, n * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(tmp.get(&b.of, n * 4)); HIPCHK(tmp.get(&b.ot, n * 4)); HIPCHK(tmp.get(&b.ow, n * 4));
    HIPCHK(tmp.get(&b.mask, n_tiles * BL_WORDS * 8));        // (whole tiles: k_bl_mark writes every word of its tile)
    HIPCHK(tmp.get(&b.tile_cnt, n_tiles * 4)); HIPCHK(tmp.get(&b.tile_off, n_tiles * 8));
    HIPCHK(tmp.get(&b.counts, 3 * 8));
    { const int rc = bl_enqueue(df, dt, dw, n, keep_first, remove_above, b, s); if (rc) return rc; }
    if (dev) {
        const u64 g = (n + 255) / 256;
        hipLaunchKernelGGL(k_bl_copy_back, dim3((u32)(g < 4096 ? g : 4096)), dim3(256), 0, s, (const u32*)b.of, (const u32*)b.ot, (const u32*)b.ow,
                           (const unsigned long long*)b.counts, n, feat, tgt, win);
        HIPCHK(hipGetLastError());
        // the counts travel in stream order: the caller synchronises the stream before reading them
        HIPCHK(hipMemcpyAsync(n_out, b.counts, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_shrunk, b.counts + 1, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_removed, b.counts + 2, 8, hipMemcpyDeviceToHost, s));
        return MCQ_OK;
    }
    unsigned long long c[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(c, b.counts, sizeof(c), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (c[0] > n) return fail(MCQ_E_HIP, "mcq_bucket_limit: more triples kept than given");
    HIPCHK(hipMemcpyAsync(feat, b.of, c[0] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(tgt, b.ot, c[0] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(win, b.ow, c[0] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = c[0]; *n_shrunk = c[1]; *n_removed = c[2];
    return MCQ_OK;
}
