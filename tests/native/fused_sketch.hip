// wave_sketch_two_windows (mcq_device.hpp) on the GPU against wave_sketch per window on the same bytes: the number of features and
// every feature, with the threshold's expectation E as shipped, at 64 (nearly every read's window A leaves more than 32 hashes
// below the threshold: the 64-lane sort, or the exact selection beyond 64) and at 4 (fewer than 16 below it: the exact selection)
// (tests/test_gpu_fused_sketch_native.py builds and runs this; exit code 0 = all equal and every forced path was taken)
#include <hip/hip_runtime.h>
#include "mcq_device.hpp"
using namespace mcq;
#define ROW 72u      // per read: [0] fused count, [1] path, [2] reference count, [4..36) fused features, [36..68) reference features
template <u32 E>
__global__ void k_fused(const char* bases, const u64* off, u32 nreads, u32* out) {
    __shared__ u32 tmp[64], dst[64], rdst[64];
    const u32 lane = threadIdx.x & 63;
    const u32 r = blockIdx.x;
    if (r >= nreads) return;
    const u64 o = off[r];
    const u32 n = (u32)(off[r + 1] - o);
    dst[lane] = 0xDEADBEEFu; rdst[lane] = 0xDEADBEEFu;
    wave_sync();
    u32 path = 9;
    const u32 nf = wave_sketch_two_windows<E>(bases + o, n, lane, tmp, dst, path);
    wave_sync();
    u32 nr = wave_sketch(bases + o, MCQ_GEOM_DEFAULT_WINLEN, MCQ_GEOM_DEFAULT_K, MCQ_GEOM_DEFAULT_S, lane, tmp, rdst);
    nr += wave_sketch(bases + o + MCQ_GEOM_DEFAULT_STRIDE, n - MCQ_GEOM_DEFAULT_STRIDE, MCQ_GEOM_DEFAULT_K, MCQ_GEOM_DEFAULT_S, lane, tmp, rdst + nr);
    wave_sync();
    u32* row = out + (u64)r * ROW;
    if (lane == 0) { row[0] = nf; row[1] = path; row[2] = nr; }
    if (lane < 32) { row[4 + lane] = dst[lane]; row[36 + lane] = rdst[lane]; }
}
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
static u32 g_x = 2463534242u;
static u32 rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }
static std::string random_read(u32 n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() & 3]; return s; }
static const char CODES[] = "NRYKMSWBDHVnacgtryX-";      // ambiguity codes in both cases, lower-case bases, bytes that are neither
static const u32 NCODES = sizeof(CODES) - 1;

template <u32 E>
static int run(const char* name, const char* d_bases, const u64* d_off, u32* d_out, const std::vector<u64>& off, u32 n_random, int forced, u32& bad_total) {
    const u32 nr = (u32)off.size() - 1;
    CK(hipMemset(d_out, 0, (size_t)nr * ROW * 4));
    hipLaunchKernelGGL(k_fused<E>, dim3(nr), dim3(64), 0, 0, d_bases, d_off, nr, d_out);
    CK(hipDeviceSynchronize());
    std::vector<u32> out((size_t)nr * ROW);
    CK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    u32 bad = 0, paths[3] = {0, 0, 0}, rpaths[3] = {0, 0, 0};
    for (u32 r = 0; r < nr; ++r) {
        const u32* row = &out[(size_t)r * ROW];
        bool ok = row[0] == row[2] && row[0] <= 32 && row[1] <= 2;
        for (u32 i = 0; ok && i < 32; ++i) ok = row[4 + i] == row[36 + i] || i >= row[0];
        if (!ok) { if (bad < 5) std::printf("  read %u (%u bases): fused %u features, path %u; per window %u\n", r, (u32)(off[r + 1] - off[r]), row[0], row[1], row[2]); ++bad; }
        if (row[1] <= 2) { paths[row[1]] += 1; if (r < n_random) rpaths[row[1]] += 1; }
    }
    std::printf("E = %-3s %u reads: one sort %u, 64-lane sort %u, exact %u; of the %u random reads %u / %u / %u; %s (%u reads differ)\n", name, nr, paths[0],
                paths[1], paths[2], n_random, rpaths[0], rpaths[1], rpaths[2], bad ? "FAILED" : "ok", bad);
    if (forced >= 0 && 2 * rpaths[forced] < n_random) { std::printf("  FAILED: the forced path %d took fewer than half of the random reads\n", forced); ++bad; }
    bad_total += bad;
    return 0;
}

int main() {
    std::vector<std::string> reads;
    // random reads, every length 129..160 (129..143: window B has fewer than 16 k-mers)
    const u32 n_random = 4096;
    for (u32 i = 0; i < n_random; ++i) reads.push_back(random_read(129 + i % 32));
    for (u32 n = 129; n <= 160; ++n) {
        // a code in the last k-mer of window A (bases 112..127), in the k-mer at 113 (113..128), in the read's last k-mer
        for (u32 rep = 0; rep < 3; ++rep) {
            std::string a = random_read(n); a[112 + rnd() % 16] = CODES[rnd() % NCODES]; reads.push_back(a);
            std::string b = random_read(n); b[113 + rnd() % 16] = CODES[rnd() % NCODES]; reads.push_back(b);
            std::string c = random_read(n); c[n - 1 - rnd() % 16] = CODES[rnd() % NCODES]; reads.push_back(c);
        }
        { std::string a = random_read(n); a[112] = 'N'; reads.push_back(a); }
        { std::string a = random_read(n); a[127] = 'n'; reads.push_back(a); }
        { std::string a = random_read(n); a[128] = 'R'; reads.push_back(a); }
        { std::string a = random_read(n); a[n - 1] = 'N'; reads.push_back(a); }
        { std::string a = random_read(n); a[n - 16] = 'y'; reads.push_back(a); }
        // lower case everywhere; a third of the bases
        { std::string a = random_read(n); for (auto& ch : a) ch |= 0x20; reads.push_back(a); }
        { std::string a = random_read(n); for (auto& ch : a) if (rnd() % 3 == 0) ch |= 0x20; reads.push_back(a); }
        // Ns leave window A one clean stretch of 16..95 bases: c_A = 1..80 (<= 32: all in; 33..64; above)
        for (u32 rep = 0; rep < 4; ++rep) {
            std::string a = random_read(n);
            const u32 len = 16 + rnd() % 80, at = rnd() % (128 - len + 1);
            for (u32 p = 0; p < 128; ++p) if (p < at || p >= at + len) a[p] = 'N';
            reads.push_back(a);
        }
        // c_A exactly 32, 33, 64, 65
        for (u32 ca : {32u, 33u, 64u, 65u}) { std::string a = random_read(n); for (u32 p = ca + 15; p < 128; ++p) a[p] = 'N'; reads.push_back(a); }
        // tandem repeats: 113 k-mers, a handful of distinct hashes (the exact selection at any E)
        { std::string a(n, 'A'); for (u32 p = 0; p < n; ++p) a[p] = "ACGT"[p & 3]; reads.push_back(a); }
        { std::string a(n, 'A'); for (u32 p = 0; p < n; ++p) a[p] = "AACCGTT"[p % 7]; reads.push_back(a); }
        { std::string a(n, 'A'); reads.push_back(a); }
        // window A repeats, window B does not, and the other way round
        { std::string a = random_read(n); for (u32 p = 0; p < 113; ++p) a[p] = "ACGT"[p & 3]; reads.push_back(a); }
        { std::string a = random_read(n); for (u32 p = 113; p < n; ++p) a[p] = "AC"[p & 1]; reads.push_back(a); }
        // nothing: all N; bytes 0x00 and 0xFF
        { std::string a(n, 'N'); reads.push_back(a); }
        { std::string a(n, '\0'); reads.push_back(a); }
        { std::string a(n, '\xFF'); reads.push_back(a); }
        // only window B has k-mers; only window A has
        { std::string a = random_read(n); for (u32 p = 0; p < 113; ++p) a[p] = 'N'; reads.push_back(a); }
        { std::string a = random_read(n); for (u32 p = 128; p < n; ++p) a[p] = 'N'; reads.push_back(a); }
    }
    // back to back (a byte loaded from outside a read is a neighbour's base and would show), the last read ends with the allocation
    std::vector<u64> off(1, 0);
    std::string all;
    for (auto& s : reads) { all += s; off.push_back(all.size()); }
    char* d_bases; u64* d_off; u32* d_out;
    CK(hipMalloc(&d_bases, all.size()));
    CK(hipMalloc(&d_off, off.size() * 8));
    CK(hipMalloc(&d_out, (size_t)reads.size() * ROW * 4));
    CK(hipMemcpy(d_bases, all.data(), all.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    u32 bad = 0;
    int rc;
    if ((rc = run<MCQ_SKETCH_EXPECT_FUSED>("as shipped", d_bases, d_off, d_out, off, n_random, -1, bad))) return rc;
    // E = 64: half of the random reads leave 33..64 hashes below the threshold and half more than 64 -- every one is a retry
    if ((rc = run<64>("64", d_bases, d_off, d_out, off, n_random, 1, bad))) return rc;
    if ((rc = run<4>("4", d_bases, d_off, d_out, off, n_random, 2, bad))) return rc;
    return bad ? 1 : 0;
}
