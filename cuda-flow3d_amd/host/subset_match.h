// The table of the records of f3d_subset_match and the grid it is laid on (include/f3d_host.h, f3d_subset_match_table and
// f3d_subset_match_layout): host code, binary64 in a fixed order, every operation rounded on its own.  tests/subset_match_ref.py
// restates it and the results match bit for bit; tests/subset_match_table_main.cpp runs it under sanitizers.  Nothing but the two
// public headers is needed.
#pragma once
#include <string>

#include "f3d_host.h"

// false with *error set (nothing written) for a grid f3d_subset_match refuses on its own numbers or a min_zncc that is NaN
bool TableSubsetMatch(const f3d_subset_match_record* records, const f3d_subset_match_grid* grid, double min_zncc,
                      const float* const* compare, f3d_subset_match_node* nodes, f3d_subset_match_summary* summary, std::string* error);

// false with *error set (nothing written) when a window leaves the volume or an argument is out of the range f3d_subset_match takes
bool LayoutSubsetMatch(size_t width, size_t height, size_t depth, int step, int window, f3d_subset_match_grid* grid, std::string* error);
