#pragma once
// mcq_read_unit.hpp -- one unit of read input, what `metacache query` opens one sequence_pair_reader for
// (src/querying.h:1329-1343): a single-end file, a pair of files read side by side (-pairfiles), or one file whose
// consecutive records are the mates of a query (-pairseq).  The options make the list (mcq_cli_common.hpp), ReadBatcher
// (mcq_read_batches.hpp) and mcq_query_mpi's whole-file reader run through it in order.
#include <string>

struct ReadUnit {
    std::string f1, f2;              // f2 empty: one file
    bool interleaved = false;        // records 2q, 2q+1 of f1 are the mates of query q (f2 empty)
    int files() const { return f2.empty() ? 1 : 2; }
    int mates() const { return (interleaved || !f2.empty()) ? 2 : 1; }
    // what the reference writes in front of the unit's mapping lines (showInfo, src/querying.h:1336-1340)
    std::string display() const { return f2.empty() ? f1 : f1 + " + " + f2; }
};
