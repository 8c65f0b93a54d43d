#pragma once
// mcq_internal.hpp -- what more than one unit of libmcq_hip.so needs on the host side: the handle structs behind the
// C ABI, the owners of their GPU resources, error reporting, a few inline helpers, and the declarations of the functions that
// cross a unit boundary (hidden visibility: none is part of the ABI).  The units: mcq_engine.hip (workspace, fused query, reduce),
// mcq_table.hip (mcq_db_*), mcq_stages.hip (staged and routing entry points, batch preparation), mcq_shard.hip (mcq_shard_*),
// mcq_target_hits.hip (mcq_target_*), mcq_align.hip (mcq_align), mcq_all_hits.hip (mcq_all_hits*), mcq_accmap.hip (mcq_accmap_*).  Kernels are not declared here: each is defined in the unit that launches it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include <algorithm>
#include <type_traits>

#include "../../include/mcq.h"
#include "mcq_device.hpp"
#include "mcq_classify.hpp"

using namespace mcq;

// ------------------------------------------------------------------ error handling
// one text per thread, kept in mcq_engine.hip behind mcq_last_error
static inline int fail(int code, const std::string& msg) { return mcq::set_error(code, msg.c_str()); }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail(MCQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// like HIPCHK inside a constructor-like function: releases what the half-built object already holds before returning
#define HIPCHK_OR(expr, cleanup) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup; \
    return fail(MCQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)

static u64 pow2ceil64(u64 x) { u64 p = 1; while (p < x) p <<= 1; return p; }

// ------------------------------------------------------------------ handles
struct mcq_db {
    DbDev d;
    int device;
    u64 nslots;
    u64 n_keys_local, n_locs_local;
    uint4* slots;             // one allocation: the buckets, then the lists too long for a bucket
    u32* tgt2tax;
    u32* gw_off; u32* gw_blk; // global-window form: first window of every target, block -> target (see LocGW)
    GwDev g;                  // ... as the kernels take them
    u32 n_shards, shard_id;
    u32 bucket_bytes, slots_per_key;
    u64 n_ext, n_windows;
    u64 bytes;
    bool seq_taxa;            // tgt2tax holds sequence-level taxa (bit 31; see make_opt)
    u64 fmt_sig;              // what the location words of this handle mean (format, field widths, window offsets of the targets, sketch
                              // parameters), hashed: the ranks of a sharded run compare it before the first words travel (mcq_shard.hip)
};

struct ScratchDev {
    u32* feat; u32* fpos; u64* foff; u64* gbuf; u64* ghits;
    u32 fmax; u32 lmax;
};

struct DebugDev {
    int mode;                 // 0 off, 1 = write match counts, 2 = write matches
    u64* match_cnt;           // [nq]
    const u64* match_off;     // [nq+1]
    u64* matches;
};

// ------------------------------------------------------------------ owners
// move-only; the destructor gives back what is held, so every way out of a function frees and a handle is destroyed by `delete`.
// Dev<T> has the shape of the build unit's (mcq_build.hip keeps its own for now: DESIGN.md 20)
template <class T> struct Dev {                 // n elements of T from hipMalloc, never fewer than one
    T* p = nullptr;
    Dev() = default;
    Dev(Dev&& o) noexcept : p(o.release()) {}
    Dev& operator=(Dev&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    ~Dev() { reset(); }
    hipError_t alloc(u64 n) { reset(); return hipMalloc(&p, (n ? n : 1) * sizeof(T)); }
    T* get() const { return p; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }
};
template <class T> struct Pinned {              // the same from hipHostMalloc
    T* p = nullptr;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : p(o.p) { o.p = nullptr; }
    Pinned& operator=(Pinned&& o) noexcept { std::swap(p, o.p); return *this; }
    ~Pinned() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(u64 n) { return p ? hipSuccess : hipHostMalloc(&p, (n ? n : 1) * sizeof(T)); }
    T* get() const { return p; }
};
struct Event {                                  // created once, on demand; converts to the runtime's handle
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};
struct Stream {                                 // a non-blocking stream of the workspace's own
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

#define MCQ_N_TIMED 3           // kernels of one batch that are timed separately: first wave stage, second wave stage, workgroup kernel
struct TimedLaunch { Event ev[MCQ_N_TIMED + 1]; };
struct mcq_ws;
// One staging set for calls with host pointers: the batch's bases and offsets, its candidate lists, and the slot a host array of
// clade keys goes through (mcq_ws_set_query_clades), guarded by the event behind its last upload.  The four arrays come with
// alloc(), at the first call that needs this set; the slot comes with the first host clade array (take_query_clades).
struct Staging {
    Event qc_ev; bool qc_used = false; Pinned<u32> qc_pinned; Dev<u32> qc_dev;
    Dev<char> d_bases; Dev<u64> d_seq_off; Dev<u32> d_cands, d_ncand;
    int alloc(const mcq_ws* ws);                // (mcq_engine.hip)
};
// Members are destroyed last to first, and the order matters: device memory goes first (the first hipFree is what waits for the
// work in flight), then the events, then the streams.  So streams are declared before events, events before device memory.
struct mcq_ws {
    int device = 0, n_block_wgs = 0;
    u64 max_queries = 0, max_bases = 0;
    u32 cap_wave = 0, cap_wave16 = 0, cap_reduce16 = 0, cap_wave32 = 0, cap_wave_many = 0;   // resident workgroups of the wave-per-query kernels on this device
    u64 last_nq = 0;
    // host-buffer pipeline (mcq_query_pipelined): staging sets 0 and 1, copy streams on both sides of the compute stream
    struct Pipe {
        Stream s_in, s_k, s_out;
        Event ev_in[2], ev_k[2], ev_out[2];
        u64 issued = 0;         // calls so far; call i uses set i & 1
        bool ready = false;
    } pipe;
    // optional per-launch timing of the path's kernels (events between them on the call's stream)
    int timing = 0;
    std::vector<TimedLaunch> ev_used, ev_free;
    double timed_ms[MCQ_N_TIMED] = {}; u64 timed_launches = 0;
    // classification of every batch while a taxonomy is attached (mcq_ws_set_classify): counts [cls_n] on the device,
    // cls_ev recorded behind the last batch that added into them
    const mcq_taxonomy* cls_tx = nullptr;
    mcq_classify_opts cls_opt = {};
    u32 cls_n = 0;
    Event cls_ev;
    // clade exclusion (mcq_ws_set_exclusion): the targets' clade keys on the device while attached (excl_tgt [excl_n]); the query
    // keys handed over for the NEXT batch (mcq_ws_set_query_clades: a device pointer as it came, or a copy of the host array)
    u32 excl_n = 0;
    const u32* qc_dev = nullptr; std::vector<u32> qc_host; u64 qc_n = 0; int qc_kind = 0;    // qc_kind: 0 nothing handed over, 1 device pointer, 2 host copy
    Staging staging[3];       // [0], [1]: the pipeline's; [2]: mcq_query's and mcq_debug_matches'
    // device and pinned memory, declared in the reverse of the order it is given back in
    Dev<unsigned short> align_scratch; u64 align_scratch_words = 0;   // mcq_align: predecessor matrices too large for LDS; made once, divided among a call's waves
    Dev<u32> excl_tgt;
    Dev<unsigned long long> cls_counts;
    ScratchDev sc = {};       // the five arrays below as the workgroup kernels take them
    Dev<u64> sc_ghits, sc_gbuf, sc_foff; Dev<u32> sc_fpos, sc_feat;
    Dev<unsigned long long> probe_buf;   // [(2 x max_queries + 3 x MCQ_OVF_TAIL) x 64]: rows of the back queue, then of the front queue; see CountersDev
    Dev<u32> ovf_list;        // [ovf_capacity(max_queries)]
    Pinned<CountersDev> ctr_host;
    Dev<CountersDev> ctr;
};

// ------------------------------------------------------------------ a handle's form as template arguments
// The only code that turns d.compact, g.on and d.bsh into the template arguments of the kernels a handle launches.  The location
// word: LocForm<u64, false> = 64-bit bit fields, <u32, false> = 32-bit bit fields, <u32, true> = the 32-bit global-window index.
// The bucket layout BSH: 2 = 64-B buckets, 0 = 16-B slots.  f gets the form as a value of the tag type.
template <class KeyT, bool GW> struct LocForm { using Key = KeyT; static constexpr bool gw = GW; };
template <int V> using IntC = std::integral_constant<int, V>;
template <class F> static auto with_loc_form(bool compact, bool gw, F&& f) {
    if (!compact) return f(LocForm<u64, false>{});
    return gw ? f(LocForm<u32, true>{}) : f(LocForm<u32, false>{});
}
template <class F> static auto with_loc_form(const mcq_db* db, F&& f) { return with_loc_form(db->d.compact != 0, db->g.on != 0, f); }
template <class F> static auto with_layout(const mcq_db* db, F&& f) {
    return db->d.bsh != 0 ? f(IntC<2>{}) : f(IntC<0>{});
}

// which form of the first wave stage a caller asked for (MCQ_FORCE_FULL_WAVE / MCQ_FORCE_LEAN_WAVE; make_opt rejects both at once)
enum class LeanReq { Auto, FullOnly, LeanOnly };
static inline LeanReq lean_request(u32 flags) { return (flags & MCQ_FORCE_LEAN_WAVE) ? LeanReq::LeanOnly : (flags & MCQ_FORCE_FULL_WAVE) ? LeanReq::FullOnly : LeanReq::Auto; }

// ------------------------------------------------------------------ defined in one unit, called from others
namespace mcq {
// mcq_engine.hip
__attribute__((visibility("hidden"))) int make_opt(const mcq_query_opts* o, OptDev& d, const mcq_db* db);
__attribute__((visibility("hidden"))) int launch_query(const mcq_db* db, mcq_ws* ws, const BatchDev& b, const OptDev& od_in, const OutDev& o,
                                                       hipStream_t st, LeanReq lean_req, const DebugDev& dbg, const ShardDev* shp = nullptr, const DbDev* dbd = nullptr,
                                                       const ExclDev* exp = nullptr /* clade exclusion: mcq_ws_set_exclusion */);
// mcq_stages.hip (instantiated for InT = u32 and u64)
__attribute__((visibility("hidden"))) int batch_dev(const mcq_batch* in, const char* d_bases, const u64* d_seq_off, BatchDev& b);
template <class InT>
__attribute__((visibility("hidden"))) int device_exclusive_scan(const InT* in, u64* out, u64 n, hipStream_t st, u32 nt = 1024);
}  // namespace mcq
