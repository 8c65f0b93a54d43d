// narrow_tail_lin (mcq_device.hpp: the lean first wave stage's tail without a sort) on the GPU against the chain it stands in for,
// dedup_finish -> sweep_targets_regs -> topk_lin_write, both behind dedup_insert on the same caller-made location lists, one wave per
// list: candidates, n_cand and the returned count must be equal word for word, and equal to a plain host selection as well.
// (tests/test_gpu_lean_tail_native.py builds and runs this; exit code 0 = all equal, every constructed table case occurred and the
// tie reduction was taken)
#include <hip/hip_runtime.h>
#include "mcq_device.hpp"
using namespace mcq;
#define MAXM 4u
#define WB 12u                  // window bits of the test's location words
#define NT 40u                  // targets of the test's table

__global__ void k_tails(const u32* words, const u32* off, const u32* nwin, u32 nlists, DbDev db, OptDev opt, OutDev outA, OutDev outB,
                        u32* ret, u32* tie) {
    __shared__ u32 buf[512], hits[512];
    const u32 lane = threadIdx.x & 63;
    const u32 l = blockIdx.x;
    if (l >= nlists) return;
    const u32 T = off[l + 1] - off[l], numWindows = nwin[l];
    const u32* src = words + off[l];
    LocShift<u32> lf; lf.wb = db.wb;
    u32 r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { const u32 t = e * 64 + lane; r[e] = t < T ? src[t] : MCQ_EMPTY; }
    // the present chain
    u32 k1, incl1, t1, tb1;
    u32 D = dedup_insert<4>(r, buf, hits, T, lane);
    const u32 D0 = D;
    D = dedup_finish(D, buf, hits, lane, lf, k1, incl1, t1, tb1);
    u32 na = ~0u;
    if (D <= 64) {
        sweep_targets_regs(k1, incl1, tb1, buf, D, numWindows, lf, lane);
        na = topk_lin_write<u32, 9, false>(db, opt, outA, dedup_sk(hits), buf, D, lf, (u64)l, lane, t1);
    }
    wave_sync();
    // the sort-free tail
    const u32 D2 = dedup_insert<4>(r, buf, hits, T, lane);
    u32 nb = ~0u;
    if (D2 <= 64) nb = narrow_tail_lin<true>(db, opt, outB, buf, hits, D2, numWindows, lf, (u64)l, lane, &tie[l]);
    wave_sync();
    if (lane == 0) { ret[4 * l] = na; ret[4 * l + 1] = nb; ret[4 * l + 2] = D0; ret[4 * l + 3] = D2; }
}

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
static u32 g_x = 2463534242u;
static u32 rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }
static u32 hslot(u32 key) { return (key * 0x9E3779B1u) >> 23; }        // dedup_slot, restated
static u32 key_of(u32 t, u32 w) { return (t << WB) | w; }

struct List { std::vector<u32> w; u32 nw; std::string what; };

// the table dedup_insert builds, inserted register by register (words 0..63, then 64..127, ...).  Which slots are taken does not
// depend on the order inside a register; the constructed cases put the key they are about into a later register than its rivals
static std::vector<u32> table_of(const std::vector<u32>& w) {
    std::vector<u32> tab(512, MCQ_EMPTY);
    for (u32 k : w) {
        u32 s = hslot(k);
        while (tab[s] != MCQ_EMPTY && tab[s] != k) s = (s + 1) & 511u;
        tab[s] = k;
    }
    return tab;
}
// slots a look-up of word k walks past before it ends (on k or on an empty slot); wrapped: it went from 511 to 0
static u32 walk_of(const std::vector<u32>& tab, u32 k, bool& found, bool& wrapped) {
    u32 s = hslot(k), n = 0;
    wrapped = false;
    while (tab[s] != MCQ_EMPTY && tab[s] != k) { if (s == 511u) wrapped = true; s = (s + 1) & 511u; ++n; }
    found = tab[s] == k;
    return n;
}
// a word of another target than `not_t`, not in `used`, whose home slot is `slot`
static u32 foreign_at(u32 slot, u32 not_t, std::set<u32>& used) {
    for (u32 t = 0; t < NT; ++t)
        for (u32 w = 100; w < (1u << WB) - 100; w += 7) {      // (far from the windows the cases use, no two of them adjacent)
            const u32 k = key_of(t, w);
            if (t != not_t && hslot(k) == slot && !used.count(k)) { used.insert(k); return k; }
        }
    std::fprintf(stderr, "no foreign word for slot %u\n", slot);
    std::exit(3);
}
// rivals first (register 0, padded to 64 words by repeating them), then the words the case is about
static List staged(const std::vector<u32>& rivals, const std::vector<u32>& later, u32 nw, const char* what) {
    List L; L.nw = nw; L.what = what;
    for (u32 i = 0; i < 64; ++i) L.w.push_back(rivals[i % rivals.size()]);
    for (u32 k : later) L.w.push_back(k);
    return L;
}

// the plain selection: hits of a key = occurrences of its word and of the numWindows - 1 windows before it in its target; first M
// distinct taxa in the order (hits descending, rank ascending, key ascending) over the keys of the ranks below keep
static void host_select(const List& L, const std::vector<u32>& t2t, u32 P, u32 keep, u32 M, std::vector<u32>& cand, u32& n) {
    std::map<u32, u32> cnt;
    for (u32 k : L.w) cnt[k] += 1;
    struct E { u32 hits, rank, key, tax; };
    std::vector<E> es;
    for (auto& kv : cnt) {
        const u32 k = kv.first, t = k >> WB, win = k & ((1u << WB) - 1);
        u32 h = 0;
        for (u32 i = 0; i < L.nw && i <= win; ++i) { auto it = cnt.find(k - i); if (it != cnt.end()) h += it->second; }
        const u32 tax = t < NT ? t2t[t] : MCQ_EMPTY, rank = t % P;
        if (tax != MCQ_EMPTY && rank < keep) es.push_back({h, rank, k, tax});
    }
    std::sort(es.begin(), es.end(), [](const E& a, const E& b) {
        if (a.hits != b.hits) return a.hits > b.hits;
        if (a.rank != b.rank) return a.rank < b.rank;
        return a.key < b.key; });
    cand.assign(MAXM * 4, 0); n = 0;
    std::set<u32> seen;
    for (auto& e : es) {
        if (n == M) break;
        if (seen.count(e.tax)) continue;
        seen.insert(e.tax);
        cand[4 * n] = e.tax; cand[4 * n + 1] = e.hits; ++n;
    }
}

int main() {
    // taxa: targets 0..7 one taxon each, 8..15 in pairs, 16..23 all one taxon, 24..38 one each, 39 has none
    std::vector<u32> t2t(NT);
    for (u32 t = 0; t < NT; ++t) t2t[t] = t < 8 ? 100 + t : t < 16 ? 200 + t / 2 : t < 24 ? 300 : 400 + t;
    t2t[39] = MCQ_EMPTY;
    std::vector<List> lists;
    u32 case_disp1 = 0, case_disp3 = 0, case_absent2 = 0, case_wrap = 0;
    for (u32 nw = 2; nw <= 4; ++nw) {
        // D = 1, 2, 32, 33, 63, 64: runs of adjacent windows on a few targets, every key once to three times
        for (u32 D : {1u, 2u, 32u, 33u, 63u, 64u})
            for (u32 rep = 0; rep < 6; ++rep) {
                List L; L.nw = nw; L.what = "D = " + std::to_string(D);
                std::set<u32> ks;
                while (ks.size() < D) ks.insert(key_of(rnd() % 12, rnd() % (D < 8 ? 3 : 9)));
                for (u32 k : ks) for (u32 m = 1 + rnd() % 3; m; --m) L.w.push_back(k);
                for (u32 i = (u32)L.w.size(); i > 1; --i) std::swap(L.w[i - 1], L.w[rnd() % i]);
                lists.push_back(L);
            }
        // multiplicities 1 .. 200 on one key, neighbours around it
        for (u32 m : {1u, 2u, 3u, 17u, 64u, 65u, 128u, 200u}) {
            List L; L.nw = nw; L.what = "multiplicity " + std::to_string(m);
            for (u32 i = 0; i < m; ++i) L.w.push_back(key_of(5, 7));
            for (u32 w : {4u, 5u, 6u, 8u, 9u, 10u}) for (u32 i = 0; i < 1 + w % 3; ++i) L.w.push_back(key_of(5, w));
            for (u32 i = 0; i < 9; ++i) L.w.push_back(key_of(6, 7));
            lists.push_back(L);
        }
        // windows 0, 1, 2 of a target: a range stops at the target's start, whatever the target before holds at its end
        for (u32 t : {0u, 1u, 9u})
            for (u32 mask = 1; mask < 8; ++mask) {
                List L; L.nw = nw; L.what = "windows 0..2 of target " + std::to_string(t);
                for (u32 w = 0; w < 3; ++w) if (mask >> w & 1) for (u32 i = 0; i < 2 + w; ++i) L.w.push_back(key_of(t, w));
                if (t > 0) for (u32 w = (1u << WB) - 3; w < (1u << WB); ++w) for (u32 i = 0; i < 4; ++i) L.w.push_back(key_of(t - 1, w));
                lists.push_back(L);
            }
        // numerically adjacent words of different targets: (t << wb) | 0 and ((t - 1) << wb) | (2^wb - 1)
        for (u32 t : {1u, 2u, 17u}) {
            List L; L.nw = nw; L.what = "adjacent words, different targets";
            for (u32 i = 0; i < 3; ++i) L.w.push_back(key_of(t, 0));
            for (u32 i = 0; i < 5; ++i) L.w.push_back(key_of(t - 1, (1u << WB) - 1));
            lists.push_back(L);
        }
        // a target index >= n_targets; a target without a taxon -- each alone, and with more hits than a real target beside it
        for (u32 t : {NT, NT + 3, 39u}) {
            List a; a.nw = nw; a.what = "target " + std::to_string(t) + " alone";
            for (u32 i = 0; i < 4; ++i) a.w.push_back(key_of(t, 3));
            lists.push_back(a);
            for (u32 i = 0; i < 2; ++i) { a.w.push_back(key_of(3, 3)); a.w.push_back(key_of(t, 2)); }
            a.what = "target " + std::to_string(t) + " beside a real one";
            lists.push_back(a);
        }
        // equal hits: different taxa with the same rank (targets 0, 8 / 0, 24: same t % P for P = 2, 4, 8 / P = 2, 3, 4, 8), with
        // different ranks (0, 1, 2: rank 2 is dropped under P = 3), the same taxon (16..23), three ways; in every order of the list
        const std::vector<std::vector<u32>> tie_sets = {{0, 8}, {0, 24}, {24, 0, 8}, {0, 1}, {1, 2}, {0, 1, 2}, {2, 1, 0}, {16, 17}, {16, 17, 18}, {8, 9}, {9, 8, 0},
                                                        {16, 0, 24}, {3, 6, 9}, {6, 3}, {12, 24, 36}};
        for (const auto& ts : tie_sets)
            for (u32 rep = 0; rep < 2; ++rep) {
                List L; L.nw = nw; L.what = "equal hits";
                for (u32 t : ts) { L.w.push_back(key_of(t, 5)); L.w.push_back(key_of(t, 5)); L.w.push_back(key_of(t, 4)); }
                if (rep) { std::reverse(L.w.begin(), L.w.end()); L.w.push_back(key_of(30, 1)); }
                lists.push_back(L);
            }
        // (a) a present predecessor displaced by one and by three slots, (b) an absent predecessor whose walk passes two foreign keys,
        // (c) walks that wrap from slot 511 to 0 -- present and absent
        for (u32 t = 2; t < 10; ++t) {
            const u32 k = key_of(t, 20 + t), p = k - 1;
            for (u32 nf : {1u, 3u}) {
                std::set<u32> used;
                std::vector<u32> riv;
                for (u32 i = 0; i < nf; ++i) riv.push_back(foreign_at(hslot(p), t, used));
                lists.push_back(staged(riv, {p, p, k, k, k}, nw, nf == 1 ? "present predecessor displaced by one" : "present predecessor displaced by three"));
            }
            std::set<u32> used;
            std::vector<u32> riv{foreign_at(hslot(p), t, used), foreign_at((hslot(p) + 1) & 511u, t, used)};
            lists.push_back(staged(riv, {k, k, k}, nw, "absent predecessor behind two foreign keys"));
        }
        for (u32 t = 0, made = 0; t < NT - 1 && made < 4; ++t)
            for (u32 w = 1; w < 2000 && made < 4; ++w) {
                const u32 p = key_of(t, w), k = p + 1;
                if (hslot(p) != 511u) continue;
                std::set<u32> used;
                std::vector<u32> riv{foreign_at(511u, t, used)};
                lists.push_back(staged(riv, {p, k, k}, nw, "present predecessor wraps"));
                lists.push_back(staged(riv, {k, k}, nw, "absent predecessor wraps"));
                ++made;
                break;
            }
    }
    // random lists: up to 64 distinct keys on few targets and windows, small multiplicities -- ties everywhere
    for (u32 i = 0; i < 1500; ++i) {
        List L; L.nw = 2 + i % 3; L.what = "random";
        const u32 D = 1 + rnd() % 64, nt = 1 + rnd() % 24, nwin = 1 + rnd() % 12;
        std::set<u32> ks;
        for (u32 tries = 0; ks.size() < D && tries < 4 * D; ++tries) ks.insert(key_of(rnd() % nt, rnd() % nwin));
        const u32 mm = 1 + rnd() % 3;
        for (u32 k : ks) for (u32 m = 1 + rnd() % mm; m; --m) L.w.push_back(k);
        for (u32 j = (u32)L.w.size(); j > 1; --j) std::swap(L.w[j - 1], L.w[rnd() % j]);
        lists.push_back(L);
    }
    // what the constructed lists do in the table
    for (auto& L : lists) {
        if (L.w.size() > 256) { std::printf("FAILED: a list of %zu words (%s)\n", L.w.size(), L.what.c_str()); return 1; }
        std::set<u32> ks(L.w.begin(), L.w.end());
        if (ks.size() > 64) { std::printf("FAILED: a list of %zu distinct keys (%s)\n", ks.size(), L.what.c_str()); return 1; }
        const std::vector<u32> tab = table_of(L.w);
        for (u32 k : ks) {
            const u32 win = k & ((1u << WB) - 1);
            for (u32 i = 1; i < L.nw && i <= win; ++i) {
                bool found, wrapped;
                const u32 n = walk_of(tab, k - i, found, wrapped);
                if (found && n == 1) ++case_disp1;
                if (found && n == 3) ++case_disp3;
                if (!found && n == 2) ++case_absent2;
                if (wrapped) ++case_wrap;
            }
        }
    }
    std::printf("%zu lists; look-ups: present and displaced by one %u, by three %u; absent behind two foreign keys %u; wrapped %u\n",
                lists.size(), case_disp1, case_disp3, case_absent2, case_wrap);
    u32 bad = 0;
    if (!case_disp1 || !case_disp3 || !case_absent2 || !case_wrap) { std::printf("FAILED: a table case did not occur\n"); ++bad; }

    std::vector<u32> words, off(1, 0), nwin;
    for (auto& L : lists) { words.insert(words.end(), L.w.begin(), L.w.end()); off.push_back((u32)words.size()); nwin.push_back(L.nw); }
    const u32 nl = (u32)lists.size();
    u32 *d_words, *d_off, *d_nwin, *d_t2t, *d_ca, *d_cb, *d_na, *d_nb, *d_ret, *d_tie;
    CK(hipMalloc(&d_words, words.size() * 4)); CK(hipMalloc(&d_off, off.size() * 4)); CK(hipMalloc(&d_nwin, nl * 4)); CK(hipMalloc(&d_t2t, NT * 4));
    CK(hipMalloc(&d_ca, (size_t)nl * MAXM * 16)); CK(hipMalloc(&d_cb, (size_t)nl * MAXM * 16));
    CK(hipMalloc(&d_na, nl * 4)); CK(hipMalloc(&d_nb, nl * 4)); CK(hipMalloc(&d_ret, nl * 16)); CK(hipMalloc(&d_tie, nl * 4));
    CK(hipMemcpy(d_words, words.data(), words.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_nwin, nwin.data(), nl * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_t2t, t2t.data(), NT * 4, hipMemcpyHostToDevice));
    DbDev db = {};
    db.wb = WB; db.compact = 1; db.tgt2tax = d_t2t; db.n_targets = NT;
    u32 ties_total = 0;
    for (u32 P : {2u, 3u, 4u, 8u})
        for (u32 M : {1u, 2u, 4u}) {
            OptDev opt = {};
            opt.max_cand = M; opt.P = P; opt.seg = 64; opt.lin = 1;
            opt.keep = 1; while (opt.keep * 2 <= P) opt.keep *= 2;
            OutDev oa = {d_ca, d_na}, ob = {d_cb, d_nb};
            CK(hipMemset(d_ca, 0xEE, (size_t)nl * MAXM * 16)); CK(hipMemset(d_cb, 0xEE, (size_t)nl * MAXM * 16));
            CK(hipMemset(d_na, 0xEE, nl * 4)); CK(hipMemset(d_nb, 0xEE, nl * 4)); CK(hipMemset(d_ret, 0xEE, nl * 16)); CK(hipMemset(d_tie, 0, nl * 4));
            hipLaunchKernelGGL(k_tails, dim3(nl), dim3(64), 0, 0, d_words, d_off, d_nwin, nl, db, opt, oa, ob, d_ret, d_tie);
            CK(hipDeviceSynchronize());
            std::vector<u32> ca((size_t)nl * M * 4), cb((size_t)nl * M * 4), na(nl), nb(nl), ret(nl * 4), tie(nl);
            CK(hipMemcpy(ca.data(), d_ca, ca.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(cb.data(), d_cb, cb.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(na.data(), d_na, nl * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(nb.data(), d_nb, nl * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(ret.data(), d_ret, nl * 16, hipMemcpyDeviceToHost)); CK(hipMemcpy(tie.data(), d_tie, nl * 4, hipMemcpyDeviceToHost));
            u32 differ = 0, ties = 0;
            for (u32 l = 0; l < nl; ++l) {
                std::vector<u32> hc; u32 hn;
                host_select(lists[l], t2t, P, opt.keep, M, hc, hn);
                const u32 D = (u32)std::set<u32>(lists[l].w.begin(), lists[l].w.end()).size();
                bool ok = na[l] == nb[l] && na[l] == hn && ret[4 * l] == na[l] && ret[4 * l + 1] == nb[l] && ret[4 * l + 2] == D && ret[4 * l + 3] == D && na[l] <= M;
                for (u32 i = 0; ok && i < 4 * na[l]; ++i) ok = ca[(size_t)l * M * 4 + i] == cb[(size_t)l * M * 4 + i] && ca[(size_t)l * M * 4 + i] == hc[i];
                for (u32 i = 4 * std::min(na[l], M); ok && i < 4 * M; ++i) ok = cb[(size_t)l * M * 4 + i] == 0xEEEEEEEEu;      // nothing written behind n_cand
                if (!ok) {
                    if (differ < 5) std::printf("  list %u (%s, %zu words, %u distinct, numWindows %u): n_cand present %u, sort-free %u, host %u; first candidate %u:%u / %u:%u / %u:%u\n",
                                                l, lists[l].what.c_str(), lists[l].w.size(), D, lists[l].nw, na[l], nb[l], hn, ca[(size_t)l * M * 4], ca[(size_t)l * M * 4 + 1],
                                                cb[(size_t)l * M * 4], cb[(size_t)l * M * 4 + 1], hc[0], hc[1]);
                    ++differ;
                }
                ties += tie[l] != 0;
            }
            std::printf("P = %u (keep %u) M = %u: %u lists took the tie reduction; %s (%u lists differ)\n", P, opt.keep, M, ties, differ ? "FAILED" : "ok", differ);
            bad += differ; ties_total += ties;
        }
    std::printf("%u lists took the tie reduction in all\n", ties_total);
    if (!ties_total) { std::printf("FAILED: no list took the tie reduction\n"); ++bad; }
    return bad ? 1 : 0;
}
