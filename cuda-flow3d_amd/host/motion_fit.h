// The solve between f3d_motion_sums and f3d_remove_motion (include/f3d.h): from the moment sums of a displacement the translation, the
// rigid motion or the affine map d ~ t + M (x - centre) that fits it best in the least-squares sense.  Plain binary64 C++, no device,
// no LAPACK; f3d_motion_solve of include/f3d_host.h is the C entry and has the definition.
#ifndef F3D_HOST_MOTION_FIT_H_
#define F3D_HOST_MOTION_FIT_H_

#include <string>

#include "f3d.h"

// false with `error` set when the model cannot be determined from the sums (the fit is then untouched)
bool SolveMotion(const struct f3d_motion_sums& sums, int model, f3d_motion_fit* fit, std::string* error);

// f3d_motion_solve_labels of include/f3d_host.h: one SolveMotion per label about the volume centre, the status F3D_LABEL_* of each, and
// an OK fit moved to the label's centroid.  false with `error` set for an unknown model only.
bool SolveLabelMotions(const struct f3d_motion_sums* sums, size_t n_labels, int model, unsigned long long min_voxels,
                       const double volume_centre[3], f3d_motion_fit* fits, int* status, std::string* error);

#endif
