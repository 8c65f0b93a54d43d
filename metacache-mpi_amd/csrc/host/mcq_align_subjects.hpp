#pragma once
// mcq_align_subjects.hpp -- the host side of mcq_query_cli's -align: the sequences a read can be aligned to, and one batch's jobs.
//
// The reference opens the top candidate's source file for every classified read and skips to its record (show_alignment,
// src/classification.cpp:437-477).  Here the distinct source files that the database's sequence-level taxa name are read once at
// start-up through mcq_genome_reader_* (file names as stored, relative to the working directory, as the reference resolves them)
// and stay in host memory with a map (file, record index) -> (offset, length): HOST MEMORY GROWS WITH THE GENOMES THE DATABASE
// NAMES.  A file that cannot be read gets one line on stderr and its targets get no block; a target whose record index lies
// beyond the file's records gets none either.  Per batch the slices the jobs name are gathered into a pinned buffer that goes to
// the device in front of mcq_align; the buffers are owned as in mcq_cli_buffers.hpp.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../../../include/mcq.h"
#include "../../../include/mcq_host.h"
#include "mcq_cli_buffers.hpp"

struct AlignSubjects {
    struct Where { uint64_t off = 0, len = 0; bool known = false; };
    std::vector<char> bases;                  // every sequence read, back to back
    std::vector<Where> of_target;             // [n_targets]
    std::vector<uint32_t> tax2tgt;            // [n_taxa]: target of a sequence-level taxon index, MCQ_NO_TAXON otherwise
    uint32_t winlen = 0, winstride = 0;       // of the targets

    bool load(mcq_refdb* rdb) {
        mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
        winlen = info.winlen; winstride = info.winstride;
        tax2tgt.assign(info.n_taxa, MCQ_NO_TAXON);
        if (mcq_refdb_tax2tgt(rdb, tax2tgt.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        of_target.assign(info.n_targets, Where());
        std::map<std::string, std::map<uint64_t, Where>> files;             // file -> record index -> where
        for (uint32_t t = 0; t < info.n_targets; ++t) {
            const uint32_t key = mcq_refdb_target_key(rdb, t);
            if (key != MCQ_NO_TAXON) files[mcq_refdb_taxon_file(rdb, key)];
        }
        for (auto& f : files) {
            if (f.first.empty() || !std::ifstream(f.first).good()) {
                std::fprintf(stderr, "-align: can't open file %s: its sequences get no alignment\n", f.first.c_str());
                continue;
            }
            const char* name = f.first.c_str();
            mcq_genome_reader* r = nullptr;
            if (mcq_genome_reader_open(&name, 1, 4u << 20, &r)) {
                std::fprintf(stderr, "-align: %s: %s: its sequences get no alignment\n", name, mcq_host_last_error());
                continue;
            }
            const uint64_t base = bases.size();
            const uint64_t step = 16u << 20;
            int32_t done = 0; bool ok = true;
            while (!done) {
                const uint64_t used = bases.size();
                bases.resize(used + step);
                uint64_t n = 0;
                if (mcq_genome_reader_next(r, bases.data() + used, step, &n, &done)) { ok = false; bases.resize(used); break; }
                bases.resize(used + n);
            }
            if (!ok) {
                std::fprintf(stderr, "-align: %s: %s: its sequences get no alignment\n", name, mcq_host_last_error());
                bases.resize(base);
            } else {
                uint64_t off = base;
                for (uint32_t t = 0; t < mcq_genome_reader_n_targets(r); ++t) {
                    mcq_taxon_rec rec; uint64_t len = 0;
                    if (mcq_genome_reader_target(r, t, &rec, &len)) break;
                    Where w; w.off = off; w.len = len; w.known = true;
                    f.second[rec.index] = w;
                    off += len;
                }
            }
            mcq_genome_reader_close(r);
        }
        bases.shrink_to_fit();
        for (uint32_t t = 0; t < info.n_targets; ++t) {
            const uint32_t key = mcq_refdb_target_key(rdb, t);
            if (key == MCQ_NO_TAXON) continue;
            const auto& recs = files[mcq_refdb_taxon_file(rdb, key)];
            const auto it = recs.find(mcq_refdb_taxon_index(rdb, key));
            if (it != recs.end()) of_target[t] = it->second;
        }
        return true;
    }

    // target of a candidate's taxon key if it is a sequence whose bases are here, MCQ_NO_TAXON otherwise
    uint32_t target_of(uint32_t key) const {
        if (key == MCQ_NO_TAXON || !(key & 0x80000000u)) return MCQ_NO_TAXON;
        const uint32_t idx = key & 0x7FFFFFFFu;
        const uint32_t t = idx < tax2tgt.size() ? tax2tgt[idx] : MCQ_NO_TAXON;
        return (t != MCQ_NO_TAXON && t < of_target.size() && of_target[t].known) ? t : MCQ_NO_TAXON;
    }
    // the subject of windows [beg, end] of target t: bases [stride * beg, min(len, stride * end + winlen)) (make_view_from_window_range,
    // src/classification.cpp:60-68)
    void slice(uint32_t t, uint32_t beg, uint32_t end, uint64_t& off, uint64_t& len) const {
        const Where& w = of_target[t];
        const uint64_t a = std::min<uint64_t>(w.len, (uint64_t)winstride * beg);
        const uint64_t e = std::max<uint64_t>(a, std::min<uint64_t>(w.len, (uint64_t)winstride * end + winlen));
        off = w.off + a; len = e - a;
    }
};

// one batch's alignment: the jobs and the gathered subjects going in, the results coming back
struct AlignSlot {
    PinnedBuf<char> sub, text_q, text_s; DeviceBuf<char> d_sub, d_text_q, d_text_s;
    PinnedBuf<mcq_align_job> jobs; DeviceBuf<mcq_align_job> d_jobs;
    PinnedBuf<mcq_alignment> res; DeviceBuf<mcq_alignment> d_res;
    std::vector<uint32_t> beg, end;           // the window range each job was cut from
    // -align-candidate-range: the top target of every read, its range and window counts (mcq_target_slots / mcq_target_hits, one slot)
    DeviceBuf<uint32_t> d_tgt, d_cnt, d_hst; DeviceBuf<mcq_target_range> d_rng; PinnedBuf<mcq_target_range> rng; PinnedBuf<uint32_t> hst;
    uint32_t text_cap = 0; bool on = false;   // on: this batch ran the kernel
};
