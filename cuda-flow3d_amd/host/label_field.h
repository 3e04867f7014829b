// The solve from the per-label sums of a scalar field to its statistics (include/f3d_host.h, f3d_label_field_solve): host code,
// binary64 from exact integers, a fixed order.  It needs the two public headers and threshold_select.h alone, so it also builds into
// a stand-alone program (tests/label_field_solve_main.cpp).
//
// Order of evaluation, per label from its row r and its `bins` counts c:
//   status    EMPTY when r.n == 0, else SMALL when r.n < min_voxels, else OK; everything below is filled for SMALL as for OK
//   min, max  the floats whose ordered key (csrc/f3d_histogram_bin.h) is r.min_key, r.max_key, widened to binary64; NaN when EMPTY
//   mean      ldexp((double)r.iq / (double)r.n, -shift): both conversions and the division rounded once each
//   variance  V = n * iqq - iq^2 with iqq = iqq_hi * 2^32 + iqq_lo, exactly, in unsigned __int128 (below 2^111, never negative by
//             Cauchy-Schwarz); vq = ((double)V / (double)n) / (double)n, the conversion rounding once; variance = ldexp(vq, -2 * shift)
//   std       ldexp(sqrt(vq), -shift): the population form
//   quantiles m = sum c in 64 bits.  With bins > 0 and m > 0 the ranks (m - 1) / 20, (m - 1) / 2 and (m - 1) - (m - 1) / 20 in integer
//             arithmetic; HistogramRank gives the bin k of a rank; the value is ((double)e_k + (double)e_(k+1)) / 2.0 with
//             e_k = HistogramEdge(lo, hi, bins, k) and e_bins = hi.  Otherwise the values are NaN and the bins -1.
// The summary counts the labels of every status and gives sum(n * mean) / sum(n) over the OK labels in label order: both sums in
// binary64 from 0.0, every product, add and the division rounded on its own; NaN without an OK label.
#ifndef LABEL_FIELD_H_
#define LABEL_FIELD_H_
#include <cstddef>
#include <string>

#include "f3d_host.h"

// false with *why set when the arguments are refused (nothing is written then): a null sums or stats, counts given with bins == 0
// or missing with bins > 0, shift outside -100 .. 100, bins above 256, what f3d_histogram refuses of lo, hi, bins
bool SolveLabelField(const struct f3d_label_field_sums* sums, const unsigned* counts, size_t n_labels, int shift, float lo, float hi,
                     size_t bins, unsigned long long min_voxels, f3d_label_field_stat* stats, f3d_label_field_summary* summary,
                     std::string* why);


// f3d_label_field_shift of include/f3d_host.h: the shift for a field whose finite values lie in [lo, hi] (`finite` of them)
int LabelFieldShift(float lo, float hi, unsigned long long finite);

#endif
