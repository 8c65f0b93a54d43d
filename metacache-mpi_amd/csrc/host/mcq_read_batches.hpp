#pragma once
// mcq_read_batches.hpp -- the input stage of mcq_query_cli: a list of units (mcq_read_unit.hpp: a file, a
// pair of files, an interleaved file) -> batches of queries on the device.  ReadBatcher owns the files of the unit it is in
// (mcq_read_stream_* of the host library; only they are open), what is asked of and carried between their chunks, and the stream
// the batches are prepared on; the caller owns the slots it fills, as many as it keeps in flight.
//
// The units go through in order and A BATCH NEVER MIXES UNITS: the end of a unit ends the batch, and slot.unit is the index of
// the unit all of the batch's queries come from.  It never decreases; a caller that writes a line per unit writes, in front of
// a batch, the lines of every unit up to slot.unit it has not written yet (a unit without records has no batch), and after
// END those of the rest.  Every unit of a list has the same number of mates.
//
// next(slot) returns BATCH, END (from then on always) or ERROR (reported on stderr).  After BATCH, slot.n > 0 queries lie in
// slot.d_bases / .d_seq_off as mcq_query takes them with MCQ_DEVICE_PTRS, ordered on stream(); query q's header is the pinned
// text[0] + hdr[2q] .. hdr[2q+1], hdr being slot.hdr if slot.host_parsed, else slot.d_hdr on the device; slot.info holds the 8
// words of mcq_reads_prepare / mcq_reads_parse.  All of it stays so until the slot is passed to next() again.
#include <algorithm>
#include <future>
#include <string>
#include <vector>

#include "../../../include/mcq.h"
#include "../../../include/mcq_host.h"
#include "mcq_cli_buffers.hpp"
#include "mcq_read_unit.hpp"

struct ReadSlot {
    PinnedBuf<char> text[2]; uint64_t len[2] = {0, 0};              // a chunk per file: the bytes the last batch left, then read()s
    DeviceBuf<char> d_text[2], d_bases, d_scratch;
    DeviceBuf<uint64_t> d_seq_off, d_hdr, d_info;
    PinnedBuf<uint64_t> hdr, info;
    std::vector<char> h_bases; std::vector<uint64_t> h_seq_off;     // a chunk parsed on the host
    uint64_t n = 0; bool host_parsed = false;
    size_t unit = 0;                                                // the unit the batch comes from
};

class ReadBatcher {
public:
    enum Status { BATCH, END, ERROR };
    // read_chunk: bytes per file and chunk; batch / batch_bases: most queries / bases of a batch; host_reader: every chunk is
    // parsed on the host.  A file of any unit that does not open (all are tried here, before anything is read) or a stream that
    // cannot be made: !ok().
    ReadBatcher(const std::vector<ReadUnit>& units, uint64_t read_chunk, uint64_t batch, uint64_t batch_bases, bool host_reader, int device)
        : units_(units), chunk_(read_chunk), batch_(batch), batch_bases_(batch_bases), host_reader_(host_reader) {
        for (size_t u = units_.size(); u-- > 0;) { if (!open_unit(u)) return; }       // (ends with the first unit open)
        MCQ_HIP(hipSetDevice(device), return);
        ok_ = s_in_.create();
    }
    ~ReadBatcher() { close_unit(); }
    bool ok() const { return ok_; }
    hipStream_t stream() const { return s_in_; }
    Status next(ReadSlot& S) {
        for (;;) {
            if (!ok_) return ERROR;
            if (unit_ >= units_.size()) return END;
            while (!at_end_) {
                if (!fill(S) || !prepare(S) || !take_or_enlarge(S)) { ok_ = false; return ERROR; }
                if (S.n) { S.unit = unit_; return BATCH; }
            }
            if (++unit_ < units_.size() && !open_unit(unit_)) { ok_ = false; return ERROR; }
        }
    }

private:
    void close_unit() { for (mcq_read_stream*& s : rs_) { if (s) mcq_read_stream_close(s); s = nullptr; } }
    // the files of unit u instead of those open now; chunks start over
    bool open_unit(size_t u) {
        close_unit();
        const ReadUnit& U = units_[u];
        mates_ = U.files(); inter_ = U.interleaved;
        for (int m = 0; m < mates_; ++m) {
            const std::string& f = m ? U.f2 : U.f1;
            if (mcq_read_stream_open(f.c_str(), &rs_[m])) { std::fprintf(stderr, "FAIL: can't open file %s\n", f.c_str()); return false; }
            want_[m] = chunk_; carry_[m] = 0; eof_[m] = 0;
        }
        at_end_ = false;
        return true;
    }
    // a chunk of each file into the slot's pinned text, the two files side by side.  A buffer too small for what is asked is
    // replaced; the one it replaces may hold the carried bytes, so it lives until the fill has moved them (the end of this function).
    bool fill(ReadSlot& S) {
        PinnedBuf<char> old[2];
        for (int m = 0; m < mates_; ++m) {
            const uint64_t need = std::max(want_[m], carry_[m]);
            if (S.text[m].cap < need) { old[m] = std::move(S.text[m]); if (!S.text[m].grow(need)) return false; }
        }
        auto fill1 = [&](int m) { return mcq_read_stream_fill(rs_[m], S.text[m].p, S.text[m].cap, std::max(want_[m], carry_[m]), &S.len[m], &eof_[m]); };
        std::future<int> second;
        if (mates_ == 2) second = std::async(std::launch::async, fill1, 1);
        int rc = fill1(0);
        if (mates_ == 2 && second.get()) rc = -1;
        if (rc) std::fprintf(stderr, "FAIL: reading the read files\n");
        return rc == 0;
    }
    // the chunks -> S.n queries in d_bases / d_seq_off, header ranges, info.  The GPU parses (mcq_reads_prepare) unless -reader host
    // was given; a chunk it finds not in the strict form (MCQ_READS_NOT_STRICT) goes to the host parser, as every chunk does then.
    bool prepare(ReadSlot& S) {
        const bool paired = mates_ == 2;
        const uint64_t L1 = S.len[0], L2 = paired ? S.len[1] : 0;
        const uint32_t flags = (eof_[0] ? MCQ_READS_EOF1 : 0) | (paired && eof_[1] ? MCQ_READS_EOF2 : 0) | (inter_ ? MCQ_READS_INTERLEAVED : 0);
        const int out_mates = (paired || inter_) ? 2 : 1;
        const uint64_t qcap = std::min<uint64_t>(batch_, std::min(L1, paired ? L2 : L1) / 2 + 2);
        if (!S.hdr.grow(2 * qcap) || !S.info.grow(MCQ_READS_INFO_WORDS) || !S.d_bases.grow(L1 + L2 + 1) || !S.d_seq_off.grow(2 * qcap + 1)) return false;
        S.host_parsed = host_reader_;
        if (!host_reader_) {
            const uint64_t sb = mcq_reads_scratch_bytes(L1, L2, qcap);
            if (!S.d_scratch.grow(sb) || !S.d_hdr.grow(2 * qcap) || !S.d_info.grow(MCQ_READS_INFO_WORDS)) return false;
            for (int m = 0; m < mates_; ++m) {
                if (!S.d_text[m].grow(S.len[m] + 1)) return false;
                if (S.len[m]) MCQ_HIP(hipMemcpyAsync(S.d_text[m].p, S.text[m].p, S.len[m], hipMemcpyHostToDevice, s_in_), return false);
            }
            if (mcq_reads_prepare(S.d_text[0].p, L1, paired ? S.d_text[1].p : nullptr, L2, flags, qcap, batch_bases_, S.d_scratch.p, sb,
                                  S.d_bases.p, S.d_seq_off.p, S.d_hdr.p, S.d_info.p, s_in_)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
            MCQ_HIP(hipMemcpyAsync(S.info.p, S.d_info.p, MCQ_READS_INFO_WORDS * 8, hipMemcpyDeviceToHost, s_in_), return false);
            MCQ_HIP(hipStreamSynchronize(s_in_), return false);
            S.host_parsed = (S.info.p[MCQ_READS_STATUS] & MCQ_READS_NOT_STRICT) != 0;
        }
        if (S.host_parsed) {
            S.h_bases.resize(L1 + L2 + 1); S.h_seq_off.resize(2 * qcap + 1);
            if (mcq_reads_parse(S.text[0].p, L1, paired ? S.text[1].p : nullptr, L2, flags, qcap, batch_bases_, S.h_bases.data(),
                                S.h_seq_off.data(), S.hdr.p, S.info.p)) { std::fprintf(stderr, "FAIL: %s\n", mcq_host_last_error()); return false; }
            if (const uint64_t n = S.info.p[MCQ_READS_N]) {
                MCQ_HIP(hipMemcpyAsync(S.d_bases.p, S.h_bases.data(), S.info.p[MCQ_READS_BASES] + 1, hipMemcpyHostToDevice, s_in_), return false);
                MCQ_HIP(hipMemcpyAsync(S.d_seq_off.p, S.h_seq_off.data(), (n * out_mates + 1) * 8, hipMemcpyHostToDevice, s_in_), return false);
                MCQ_HIP(hipStreamSynchronize(s_in_), return false);
            }
        }
        S.n = S.info.p[MCQ_READS_N];
        return true;
    }
    // Queries were taken: each file is cut behind its last one, the rest is carried into the next chunk.  None was taken: all is carried,
    // and a file without a complete record in its chunk has ended (so has the input) or is asked for twice the bytes, for the next fill only.
    bool take_or_enlarge(ReadSlot& S) {
        for (int m = 0; m < mates_; ++m) {
            const uint64_t cut = S.n ? S.info.p[MCQ_READS_CUT1 + m] : 0;
            if (mcq_read_stream_consume(rs_[m], cut)) { std::fprintf(stderr, "FAIL: %s\n", mcq_host_last_error()); return false; }
            carry_[m] = S.len[m] - cut;
            if (S.n) want_[m] = chunk_;
            else if (S.info.p[MCQ_READS_COMPLETE1 + m] == 0 && eof_[m]) at_end_ = true;
            else if (S.info.p[MCQ_READS_COMPLETE1 + m] == 0) want_[m] = std::max<uint64_t>(1, 2 * S.len[m]);
        }
        return true;
    }

    const std::vector<ReadUnit> units_; const uint64_t chunk_, batch_, batch_bases_; const bool host_reader_;
    size_t unit_ = 0;                                              // the unit whose files are open
    int mates_ = 1; bool inter_ = false;                           // its files; its file is interleaved
    mcq_read_stream* rs_[2] = {nullptr, nullptr}; Stream s_in_;
    uint64_t want_[2] = {chunk_, chunk_}, carry_[2] = {0, 0};      // bytes asked of the next fill; bytes the last batch left
    int32_t eof_[2] = {0, 0};                                      // the last fill reached the end of its file
    bool at_end_ = false, ok_ = false;
};
