#pragma once
// mcq_host_internal.hpp -- what the units of libmcq_host.so share besides include/mcq_host.h; not exported
// sets the library's error text (mcq_host_last_error) and returns -1
#include <stdint.h>
#include <string>
__attribute__((visibility("hidden"))) int mcq_host_set_error(const char* text);
// what a sequence header names (mcq_host_build.cpp): extract_ncbi_accession_version_number, extract_ncbi_accession_number and
// extract_taxon_id of src/sequence_io.cpp:600-677, :724-748
__attribute__((visibility("hidden"))) std::string mcq_header_accession_version(const std::string& header);
__attribute__((visibility("hidden"))) std::string mcq_header_accession(const std::string& header);
__attribute__((visibility("hidden"))) int64_t mcq_header_taxid(const std::string& header);
