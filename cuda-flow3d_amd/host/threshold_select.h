// Exact selection on a histogram of f3d_histogram (include/f3d_host.h has the definitions): the float32 edge of a bin, the Otsu cuts
// of two or three classes and the bin of a rank.  Host code, no device needed; it includes nothing of the driver, so that a
// stand-alone program can be built from it (tests/histogram_host_main.cpp).
#ifndef THRESHOLD_SELECT_H_
#define THRESHOLD_SELECT_H_

#include <cstddef>
#include <string>

#include "f3d_host.h"

// Each returns false with *why set when its arguments are refused (nothing is written then).
bool HistogramEdge(float lo, float hi, size_t bins, size_t k, float* edge, std::string* why);
bool OtsuCuts(const unsigned long long* counts, size_t bins, int classes, unsigned* cuts, f3d_otsu_info* info, std::string* why);
bool HistogramRank(const unsigned long long* counts, size_t bins, unsigned long long r, unsigned* bin, std::string* why);

#endif  // THRESHOLD_SELECT_H_
