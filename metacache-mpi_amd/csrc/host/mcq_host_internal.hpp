#pragma once
// mcq_host_internal.hpp -- what the units of libmcq_host.so share besides include/mcq_host.h; not exported
// sets the library's error text (mcq_host_last_error) and returns -1
__attribute__((visibility("hidden"))) int mcq_host_set_error(const char* text);
