// The solve from the shape sums of labelled bodies to their shape table (include/f3d_host.h, f3d_label_shape_solve): host code,
// binary64, a fixed order.  It needs nothing but the two public headers, so it also builds into a stand-alone program.
#ifndef LABEL_SHAPE_H_
#define LABEL_SHAPE_H_
#include <cstddef>

#include "f3d_host.h"

// f3d_label_shape_solve of include/f3d_host.h: one row of `out` per label.  Nothing can fail: the arguments are checked by the caller.
void SolveLabelShapes(const struct f3d_label_shape_sums* sums, size_t n_labels, f3d_label_shape* out);

// The eigenvalues (descending) and unit axes (axes[3 * i + a]: component a of axis i, signs as in the header) of the symmetric matrix
// c (xx yy zz xy xz yz): cyclic Jacobi, kLabelShapeSweeps sweeps over the pairs (0,1) (0,2) (1,2).
constexpr int kLabelShapeSweeps = 12;
void LabelShapeAxes(const double c[6], double values[3], double axes[9]);

#endif
