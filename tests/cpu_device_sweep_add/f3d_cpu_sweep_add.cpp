// TEST INFRASTRUCTURE: f3d_solve_sweep_add for the host-memory stand-in of tests/cpu_device, in a file of its own so that the
// stand-in can be built with the entry (this directory's Makefile) and without it (tests/cpu_device: the host library must load
// and solve either way).  Made of the stand-in's own entries: the sweep into the outputs, then outputs += flow on the same box and
// window -- binary32 addition commutes on numbers, so these are the bits of flow + new increments.
#include "f3d.h"

extern "C" int f3d_solve_sweep_add(f3d_devptr f0, f3d_devptr f1, f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr du, f3d_devptr dv,
                                   f3d_devptr dw, f3d_devptr phi, f3d_devptr ksi, size_t width, size_t height, size_t depth, float hx,
                                   float hy, float hz, float alpha, f3d_devptr su, f3d_devptr sv, f3d_devptr sw, const f3d_slab* slab)
{
  const f3d_devptr in[10] = {f0, f1, u, v, w, du, dv, dw, phi, ksi}, out[3] = {su, sv, sw};
  for (f3d_devptr o : out)
    for (f3d_devptr i : in)
      if (o == i) return 1;  // an output that is also an input is refused
  if (int e = f3d_solve_sweep(f0, f1, u, v, w, du, dv, dw, phi, ksi, width, height, depth, hx, hy, hz, alpha, su, sv, sw, slab)) return e;
  if (slab && slab->z_lo == slab->z_hi) return 0;
  for (int c = 0; c < 3; ++c)
    if (int e = f3d_add(out[c], in[2 + c], width, height, depth, slab)) return e;
  return 0;
}
