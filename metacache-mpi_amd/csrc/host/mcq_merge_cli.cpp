// mcq_merge_cli -- the reference's `metacache merge` (src/mode_merge.cpp): result files of queries against several databases, written
// with -tophits -queryids -lowest species, are merged per read and classified from the union of the top hits.
//   mcq_merge_cli <results file|directory>... -taxonomy DIR [options]
// The files stream through two pinned buffers into mcq_merge_chunk (include/mcq.h), cut at line ends: the read of the next chunk
// runs beside the parse of this one (the parse itself waits for its chunk: it reads the strict-form word back).  A chunk that is
// not strict goes through mcq_merge_host (include/mcq_host.h) and mcq_merge_lines.  The merged lists are classified on the device
// (mcq_merge_finish: the per-taxon counts) and written by the writers of mcq_query_cli (mcq_cli_common.hpp).
// Divergences from the reference: all files must hold the same number of mapping lines; id 0 and ids beyond
// that number are errors; a line the reference does not return from ends the run with file and line; unknown taxids are counted.
#include <fcntl.h>
#include <unistd.h>

#include "mcq_cli_common.hpp"
#include "mcq_cli_buffers.hpp"

namespace {

const char* const kMergeUsage =
    "usage: mcq_merge_cli <results file|directory>... -taxonomy DIR [options]\n"
    "Merges result files that mcq_query_cli (or the reference) wrote with -tophits -queryids -lowest species.\n"
    "  -taxonomy DIR        directory with nodes.dmp and names.dmp (merged.dmp if there)\n"
    "  -out FILE            where the mapping lines, tables and summary go (default: stdout)\n"
    "  -lowest R, -highest R   ranks of the classification (lowest is at least species)\n"
    "  -hitmin N            hits a classification needs (default 5)\n"
    "  -maxcand N           candidates kept per read, 1..16 (default 2)\n"
    "  -tophits -queryids -taxids -taxids-only -omit-ranks -lineage -mapped-only -nomap\n"
    "  -abundances [FILE], -abundance-per R\n"
    "  -parser gpu|host     who parses the mapping lines (default gpu; text that is not strict always goes to the host parser)\n"
    "  -read-chunk BYTES    bytes of a file per chunk (default 8 MiB; about 16 B of device memory per byte)\n"
    "  -threads N           accepted; the lines are written by one thread\n";

struct Source { std::string name; uint32_t column = 0; uint64_t begin = 0, lines = 0; };
struct MergeOpts { std::string taxonomy; bool host_parser = false; };

bool parse(int argc, char** argv, Options& o, MergeOpts& m, std::vector<std::string>& named) {
    o.lowest = MCQ_RANK_SPECIES; o.maxcand = 0; o.threads = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "-help" || a == "--help" || a == "-h") { std::fputs(kMergeUsage, stdout); return false; }
        else if (a.empty() || a[0] != '-' || a == "-") named.push_back(a);
        else if (a == "-taxonomy") m.taxonomy = next();
        else if (a == "-out") o.outfile = next();
        else if (a == "-lowest") { const uint32_t r = mcq_rank_from_name(next()); if (r < MCQ_RANK_ROOT) o.lowest = r; }
        else if (a == "-highest") { const uint32_t r = mcq_rank_from_name(next()); if (r <= MCQ_RANK_ROOT) o.highest = r; }
        else if (a == "-hitmin") o.hitmin = (uint32_t)std::atoi(next());
        else if (a == "-hitdiff") { o.hitdiff = (float)std::atof(next()); if (o.hitdiff > 1) o.hitdiff *= 0.01; }
        else if (a == "-maxcand" || a == "-max-cand") o.maxcand = (uint32_t)std::max(0, std::atoi(next()));
        else if (a == "-tophits" || a == "-top-hits") o.tophits = true;
        else if (opt_named(a, {"-queryids", "-query-ids", "-query_ids", "-queryid", "-query-id", "-query_id"})) o.query_ids = true;
        else if (a == "-taxids" || a == "-taxid") o.taxids = true;
        else if (a == "-taxids-only" || a == "-taxidsonly" || a == "-taxid-only") o.taxids_only = true;
        else if (a == "-omit-ranks" || a == "-omitranks") o.show_ranks = false;
        else if (a == "-lineage") o.lineage = true;
        else if (a == "-mapped-only" || a == "-mappedonly") o.mapped_only = true;
        else if (a == "-nomap" || a == "-no-map") o.nomap = true;
        else if (a == "-abundances") { o.abundances = true; if (i + 1 < argc && argv[i + 1][0] != '-') o.abundance_file = argv[++i]; }
        else if (a == "-abundance-per" || a == "-abundances-per" || a == "-abundance_per" || a == "-abundances_per") {
            const uint32_t r = mcq_rank_from_name(next()); if (r < MCQ_RANK_ROOT) o.abundance_rank = r;
        }
        else if (a == "-threads") (void)next();
        else if (a == "-read-chunk") o.read_chunk = std::max<uint64_t>(1, std::strtoull(next(), nullptr, 10));
        else if (a == "-parser") {
            const std::string w = next();
            if (w != "gpu" && w != "host") { std::fprintf(stderr, "ABORT: -parser takes gpu or host\n"); return false; }
            m.host_parser = w == "host";
        }
        else { std::fprintf(stderr, "ABORT: option %s is not supported by mcq_merge_cli\n", a.c_str()); return false; }
    }
    if (o.hitmin == 0) o.hitmin = 5;                                         // get_merge_options, src/mode_merge.cpp:84-89
    if (o.lowest < MCQ_RANK_SPECIES) o.lowest = MCQ_RANK_SPECIES;
    if (o.lowest > o.highest) o.lowest = o.highest;
    if (o.maxcand == 0) o.maxcand = 2;                                       // rules.maxCandidates, src/mode_merge.cpp:284-286
    if (o.maxcand > 16) { std::fprintf(stderr, "ABORT: -maxcand is at most 16\n"); return false; }
    if (o.abundance_file == o.outfile) o.abundance_file.clear();
    if (o.nomap && o.tophits) { o.nomap = false; o.mapped_only = true; }
    if (m.taxonomy.empty()) { std::fprintf(stderr, "ABORT: -taxonomy DIR is needed\n"); return false; }
    return true;
}

// the lines of a chunk that is not strict (or of every chunk under -parser host): the reference's token parser, then the apply kernel,
// one call per run of distinct queries
bool host_chunk(mcq_merge* mg, const char* text, uint64_t n, const Source& s, uint32_t ordinal, uint64_t offset, uint64_t line_no,
                uint64_t n_queries, hipStream_t st) {
    uint64_t line_cap = 1, item_cap = 1;
    for (uint64_t i = 0; i < n; ++i) { line_cap += text[i] == '\n'; item_cap += text[i] == ':'; }
    std::vector<uint32_t> q(line_cap), hits(item_cap), hl(line_cap);
    std::vector<uint64_t> off(line_cap + 1), ho(line_cap), cut;
    std::vector<int64_t> tid(item_cap);
    uint64_t nl = 0, ni = 0;
    if (mcq_merge_host(text, n, s.column, n_queries, s.name.c_str(), line_no, offset, q.data(), off.data(), tid.data(), hits.data(), ho.data(),
                       hl.data(), line_cap, item_cap, &nl, &ni)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
    std::vector<uint8_t> seen(n_queries, 0);
    std::vector<uint32_t> touched;
    for (uint64_t first = 0, l = 0; l <= nl; ++l) {
        if (l == nl || seen[q[l]]) {
            if (l > first) {
                cut.assign(off.begin() + first, off.begin() + l + 1);
                const uint64_t a = cut[0];
                for (uint64_t& x : cut) x -= a;
                if (mcq_merge_lines(mg, q.data() + first, cut.data(), tid.data() + a, hits.data() + a, ho.data() + first, hl.data() + first, l - first,
                                    ordinal, 0, st)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
            }
            for (uint32_t t : touched) seen[t] = 0;
            touched.clear(); first = l;
        }
        if (l < nl) { seen[q[l]] = 1; touched.push_back(q[l]); }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    Options p; MergeOpts mo; std::vector<std::string> named;
    if (!parse(argc, argv, p, mo, named)) return 1;
    std::vector<std::string> files;                                          // expanded like read files, then sorted (src/mode_merge.cpp:411-420)
    for (const std::string& n : named) {
        const std::vector<std::string> in = files_in_directory(n);
        if (in.empty()) files.push_back(n); else files.insert(files.end(), in.begin(), in.end());
    }
    std::sort(files.begin(), files.end());
    if (files.size() < 2) { std::fprintf(stderr, "ABORT: a merge needs two result files or more (%zu given)\n", files.size()); return 1; }
    std::vector<Source> src(files.size());
    for (size_t k = 0; k < files.size(); ++k) {
        src[k].name = files[k];
        if (mcq_results_properties(files[k].c_str(), &src[k].column, &src[k].begin, &src[k].lines)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return 1; }
        if (src[k].lines != src[0].lines) {
            std::fprintf(stderr, "ABORT: file %s holds %llu mapping lines, file %s holds %llu: the files of a merge are results of the same reads\n",
                         files[k].c_str(), (unsigned long long)src[k].lines, files[0].c_str(), (unsigned long long)src[0].lines);
            return 1;
        }
    }
    const uint64_t nq = src[0].lines;
    mcq_taxdump* dump = nullptr; mcq_refdb* rdb = nullptr;
    if (mcq_taxdump_read(mo.taxonomy.c_str(), &dump) || mcq_refdb_from_taxdump(dump, &rdb)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return 1; }
    mcq_taxdump_free(dump);
    mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
    std::vector<int64_t> ids(info.n_taxa); std::vector<uint32_t> idx(info.n_taxa); uint64_t n_ids = 0;
    if (mcq_refdb_taxid_table(rdb, ids.data(), idx.data(), &n_ids)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return 1; }
    const int device = 0;
    MCQ_HIP(hipSetDevice(device), return 1);
    mcq_taxonomy* tx = make_taxonomy(rdb, device);
    if (!tx) return 1;
    mcq_merge* mg = nullptr;
    if (mcq_merge_create(tx, ids.data(), idx.data(), n_ids, nq, p.maxcand, p.lowest, device, &mg)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1; }
    Stream st, copy; Event copied[2];
    if (!st.create() || !copy.create() || !copied[0].create() || !copied[1].create()) return 1;

    std::ofstream file;
    std::ostream& os = open_out(p, file);
    if (!p.outfile.empty()) {
        if (!file.good()) { std::fprintf(stderr, "ABORT: Could not write to file %s\n", p.outfile.c_str()); return 1; }
        std::cout << "Per-Read mappings will be written to file: " << p.outfile << std::endl;
    }
    const Out out = make_out(rdb, p);
    write_head(os, out, p.hitmin, false);                                    // (no TABLE_LAYOUT line: map_candidates_to_targets prints none)
    os << out.comment << "Merging " << files.size() << " files:\n";
    for (const std::string& f : files) os << out.comment << f << '\n';
    typedef std::chrono::steady_clock Clock;
    auto ms_since = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
    const auto t0 = Clock::now();
    double ms_read = 0, ms_parse = 0;                                        // in pread; in mcq_merge_chunk / the host parser and mcq_merge_lines

    // every file: chunks of whole lines through two pinned and two device buffers
    PinnedBuf<char> host[2]; DeviceBuf<char> dev[2];
    const uint64_t want = std::max<uint64_t>(p.read_chunk, 1);
    uint64_t strict_chunks = 0, host_chunks = 0;
    for (size_t k = 0; k < files.size(); ++k) {
        const int fd = open(files[k].c_str(), O_RDONLY);
        if (fd < 0) { std::fprintf(stderr, "ABORT: could not re-open file %s\n", files[k].c_str()); return 1; }
        uint64_t at = src[k].begin, line_no = 1;
        {   // the number of the first results line
            std::ifstream head(files[k], std::ios::binary); std::string l; uint64_t pos = 0;
            while (pos < at && std::getline(head, l)) { pos += l.size() + 1; ++line_no; }
        }
        std::string carry;                                                   // the bytes behind the last line end of the chunk before
        bool eof = false;
        for (int b = 0; !eof; b ^= 1) {
            if (copied[b].h) MCQ_HIP(hipEventSynchronize(copied[b]), return 1);      // (the buffer's last copy to the device is done)
            const uint64_t chunk_at = at - carry.size(), cap = carry.size() + want;
            if (cap >= (1ull << 32)) { std::fprintf(stderr, "ABORT: a line of 4 GiB in file %s\n", files[k].c_str()); return 1; }
            if (!host[b].grow(cap) || !dev[b].grow(cap)) return 1;
            uint64_t n = carry.size();
            std::memcpy(host[b].p, carry.data(), n);
            const auto tr = Clock::now();
            while (n < cap) {
                const ssize_t got = pread(fd, host[b].p + n, cap - n, (off_t)at);
                if (got < 0) { std::fprintf(stderr, "ABORT: read error in file %s\n", files[k].c_str()); return 1; }
                if (got == 0) { eof = true; break; }
                n += (uint64_t)got; at += (uint64_t)got;
            }
            ms_read += ms_since(tr);
            uint64_t use = n;                                                // whole lines; at the end of the file all that is left
            if (!eof) while (use > 0 && host[b].p[use - 1] != '\n') --use;
            carry.assign(host[b].p + use, n - use);
            if (use == 0) continue;                                          // (no line end yet: read on behind what is carried)
            bool strict = false;
            const auto tp = Clock::now();
            if (!mo.host_parser) {
                MCQ_HIP(hipMemcpyAsync(dev[b].p, host[b].p, use, hipMemcpyHostToDevice, copy), return 1);
                MCQ_HIP(hipEventRecord(copied[b], copy), return 1);
                MCQ_HIP(hipStreamWaitEvent(st, copied[b], 0), return 1);
                int32_t s = 0;
                if (mcq_merge_chunk(mg, dev[b].p, use, (uint32_t)k, chunk_at, src[k].column, &s, st)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1; }
                strict = s != 0;
            }
            if (strict) ++strict_chunks;
            else {
                ++host_chunks;
                if (!host_chunk(mg, host[b].p, use, src[k], (uint32_t)k, chunk_at, line_no, nq, st)) return 1;
            }
            ms_parse += ms_since(tp);
            for (uint64_t i = 0; i < use; ++i) line_no += host[b].p[i] == '\n';
        }
        close(fd);
    }

    // classify on the device (the per-taxon counts), copy the lists and the header references out
    const auto tf = Clock::now();
    std::vector<uint64_t> counts(info.n_taxa + 1, 0);
    DeviceBuf<uint64_t> dcounts;
    if (!dcounts.grow(info.n_taxa + 1)) return 1;
    MCQ_HIP(hipMemsetAsync(dcounts.p, 0, (info.n_taxa + 1) * 8, st), return 1);
    const mcq_classify_opts co = classify_opts(p, p.hitmin);
    if (mcq_merge_finish(mg, &co, nullptr, dcounts.p, st)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1; }
    MCQ_HIP(hipMemcpyAsync(counts.data(), dcounts.p, (info.n_taxa + 1) * 8, hipMemcpyDeviceToHost, st), return 1);
    MCQ_HIP(hipStreamSynchronize(st), return 1);
    std::vector<uint32_t> ncand(nq), pairs((size_t)nq * p.maxcand * 2), hfile(nq), hlen(nq);
    std::vector<uint64_t> hoff(nq);
    uint64_t unknown = 0;
    if (mcq_merge_lists(mg, ncand.data(), pairs.data(), &unknown) || mcq_merge_headers(mg, hfile.data(), hoff.data(), hlen.data())) {
        std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1;
    }
    if (unknown) std::cerr << "taxid not found: " << unknown << " top_hits items name a taxon the taxonomy does not have" << std::endl;

    const double ms_finish = ms_since(tf);
    const auto tw = Clock::now();
    // the mapping lines for query 1 .. n, the tables, the summary
    std::vector<int> fds(files.size(), -1);
    for (size_t k = 0; k < files.size(); ++k) fds[k] = open(files[k].c_str(), O_RDONLY);
    uint64_t assigned[MCQ_RANK_NONE + 1] = {0};
    std::vector<mcq_cand> cands(p.maxcand);
    std::string token;
    for (uint64_t q = 0; q < nq; ++q) {
        token.assign(hlen[q], '\0');
        if (hlen[q] && pread(fds[hfile[q]], &token[0], hlen[q], (off_t)hoff[q]) != (ssize_t)hlen[q]) { std::fprintf(stderr, "ABORT: read error in file %s\n", files[hfile[q]].c_str()); return 1; }
        for (uint32_t i = 0; i < ncand[q]; ++i) { cands[i].tax = pairs[((size_t)q * p.maxcand + i) * 2]; cands[i].hits = pairs[((size_t)q * p.maxcand + i) * 2 + 1]; cands[i].win_beg = cands[i].win_end = 0; }
        write_query(os, out, p.hitmin, token.data(), token.size(), cands.data(), ncand[q], assigned, MCQ_NO_TAXON, nullptr, q + 1);
    }
    for (int fd : fds) if (fd >= 0) close(fd);
    const double ms = ms_since(t0);
    if (p.tax_counts() && !write_abundances(os, rdb, p, counts, assigned)) return 1;
    write_summary(os, out, assigned, ms);
    os.flush();
    std::cerr << "chunks parsed on the GPU: " << strict_chunks << ", on the host: " << host_chunks << std::endl;
    std::cerr << "phases ms: read " << ms_read << ", parse+apply " << ms_parse << ", finish " << ms_finish << ", write " << ms_since(tw)
              << ", all " << ms_since(t0) << std::endl;
    mcq_merge_free(mg); mcq_taxonomy_destroy(tx); mcq_refdb_close(rdb);
    return os.good() ? 0 : 1;
}
