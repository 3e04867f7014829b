// The solve from the records of f3d_block_match to one row per node (include/f3d_host.h, f3d_block_match_solve): host code, integers
// and binary64 in a fixed order, every operation rounded on its own.  tests/block_match_ref.py restates it and the results match bit
// for bit; tests/block_match_solve_main.cpp runs it under sanitizers.  Nothing but the two public headers is needed.
#pragma once
#include <string>

#include "f3d_host.h"

// false with *error set (nothing written) for a grid f3d_block_match refuses or a min_zncc that is NaN
bool SolveBlockMatch(const f3d_block_match_record* records, const f3d_block_match_grid* grid, const int* centre, double min_zncc,
                     f3d_block_match_node* nodes, f3d_block_match_summary* summary, std::string* error);

// f3d_block_match_layout of include/f3d_host.h: false with *error set (nothing written) when a window leaves the volume or an argument
// is out of the range f3d_block_match takes
bool LayoutBlockMatch(size_t width, size_t height, size_t depth, int step, int window, int rx, int ry, int rz, f3d_block_match_grid* grid,
                      std::string* error);
