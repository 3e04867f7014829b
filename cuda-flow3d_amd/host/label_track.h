// The solve from the overlap rows of two labelled volumes to the tracks of their bodies (include/f3d_host.h, f3d_overlap_solve): host
// code, integers and binary64, a fixed order.  tests/overlap_ref.py restates it and the results match bit for bit.
#pragma once
#include <cstddef>
#include <string>

#include "f3d_host.h"

// f3d_overlap_solve of include/f3d_host.h: one row of `a` per body of A, one of `b` and one entry of map_b per body of B.  False with
// *error set (nothing written) when a row lies outside 0 .. n_a x -1 .. n_b, is (0, 0) or (0, -1), or min_fraction is not in (0, 1].
bool SolveOverlaps(const struct f3d_overlap* rows, size_t count, size_t n_a, size_t n_b, double min_fraction, f3d_track_a* a, f3d_track_b* b,
                   int* map_b, f3d_track_summary* summary, std::string* error);
