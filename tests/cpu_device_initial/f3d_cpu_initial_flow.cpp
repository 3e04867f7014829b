// TEST INFRASTRUCTURE: f3d_initial_flow for the host-memory stand-in of tests/cpu_device, in a file of its own so that the stand-in
// can be built with the entry (this directory's Makefile) and without it (tests/cpu_device: the host library links the entry weakly
// and must say so when it is asked for).  Plain loops over the box, the definition of include/f3d.h word for word; the geometry comes
// from the stand-in's own f3d_get_container.  f3d_compose_flow is here as well, because the driver cannot start a trajectory
// without it and one of the sources of an initial flow is the trajectory: acc += inc sampled trilinearly at x + acc, with the
// products and sums of the device's gather in the same order.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "f3d.h"

namespace {

template <typename T>
T* P(f3d_devptr p) { return reinterpret_cast<T*>(static_cast<uintptr_t>(p)); }

// the box fits the current container; pitch in floats and rows per plane out
bool geometry(size_t w, size_t h, size_t d, size_t* pitch_f, size_t* rows)
{
  f3d_size4 c;
  if (f3d_get_container(&c) != 0 || c.pitch == 0 || c.height == 0) return false;
  if (w == 0 || h == 0 || d == 0 || w > c.width || h > c.height || d > c.depth || w * sizeof(float) > c.pitch) return false;
  *pitch_f = c.pitch / sizeof(float);
  *rows = c.height;
  return true;
}

bool inside(float x, float y, float z, size_t w, size_t h, size_t d)
{
  return !(std::isnan(x) || std::isnan(y) || std::isnan(z) || x < 0.f || x > static_cast<float>(w - 1) || y < 0.f ||
           y > static_cast<float>(h - 1) || z < 0.f || z > static_cast<float>(d - 1));
}

}  // namespace

extern "C" int f3d_initial_flow(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w,
                                size_t width, size_t height, size_t depth, f3d_initial_info* info)
{
  if (!u || !v || !w || !out_u || !out_v || !out_w) return 1;
  const f3d_devptr in[3] = {u, v, w}, out[3] = {out_u, out_v, out_w};
  for (int i = 0; i < 3; ++i)
    for (int o = 0; o < 3; ++o)
      if (i != o && (in[i] == out[o] || out[i] == out[o])) return 1;
  size_t pitch_f = 0, rows = 0;
  if (!geometry(width, height, depth, &pitch_f, &rows)) return 1;
  unsigned long long replaced = 0, leaving = 0;
  uint32_t largest = 0;  // the bits of the largest |component|: non-negative floats order like their bits
  for (size_t z = 0; z < depth; ++z)
    for (size_t y = 0; y < height; ++y) {
      const size_t row = (z * rows + y) * pitch_f;
      for (size_t x = 0; x < width; ++x) {
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = P<const float>(in[k])[row + x];
        if (std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2])) {
          if (!inside(static_cast<float>(x) + c[0], static_cast<float>(y) + c[1], static_cast<float>(z) + c[2], width, height, depth))
            ++leaving;
          for (int k = 0; k < 3; ++k) {
            uint32_t bits;
            std::memcpy(&bits, &c[k], sizeof(bits));
            bits &= 0x7fffffffu;
            if (bits > largest) largest = bits;
          }
        } else {
          c[0] = c[1] = c[2] = 0.f;
          ++replaced;
        }
        for (int k = 0; k < 3; ++k) P<float>(out[k])[row + x] = c[k];
      }
    }
  if (info) {
    info->voxels = static_cast<unsigned long long>(width) * height * depth;
    info->replaced = replaced;
    info->leaving = leaving;
    std::memcpy(&info->max_abs, &largest, sizeof(float));
  }
  return 0;
}

extern "C" int f3d_compose_flow(f3d_devptr acc_u, f3d_devptr acc_v, f3d_devptr acc_w, f3d_devptr inc_u, f3d_devptr inc_v, f3d_devptr inc_w,
                                size_t width, size_t height, size_t depth, unsigned long long* lost)
{
  if (!acc_u || !acc_v || !acc_w || !inc_u || !inc_v || !inc_w) return 1;
  const f3d_devptr acc[3] = {acc_u, acc_v, acc_w}, inc[3] = {inc_u, inc_v, inc_w};
  for (f3d_devptr a : acc)
    for (f3d_devptr i : inc)
      if (a == i) return 1;
  size_t pitch_f = 0, rows = 0;
  if (!geometry(width, height, depth, &pitch_f, &rows)) return 1;
  const int W = static_cast<int>(width), H = static_cast<int>(height), D = static_cast<int>(depth);
  // the update is in place and a voxel's sample reads inc only, so the scan order does not matter
  unsigned long long n_lost = 0;
  for (int z = 0; z < D; ++z)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t c = (static_cast<size_t>(z) * rows + y) * pitch_f + x;
        float a[3];
        for (int k = 0; k < 3; ++k) a[k] = P<const float>(acc[k])[c];
        const float xf = static_cast<float>(x) + a[0], yf = static_cast<float>(y) + a[1], zf = static_cast<float>(z) + a[2];
        if (!inside(xf, yf, zf, width, height, depth)) {
          a[0] = a[1] = a[2] = std::nanf("");
        } else {
          const int xi = static_cast<int>(std::floor(xf)), yi = static_cast<int>(std::floor(yf)), zi = static_cast<int>(std::floor(zf));
          const float dx = xf - static_cast<float>(xi), dy = yf - static_cast<float>(yi), dz = zf - static_cast<float>(zi);
          const int x1 = xi + 1 < W ? xi + 1 : W - 1, y1 = yi + 1 < H ? yi + 1 : H - 1, z1 = zi + 1 < D ? zi + 1 : D - 1;
          auto row = [&](int yy, int zz) { return (static_cast<size_t>(zz) * rows + yy) * pitch_f; };
          const size_t r00 = row(yi, zi), r10 = row(y1, zi), r01 = row(yi, z1), r11 = row(y1, z1);
          for (int k = 0; k < 3; ++k) {
            const float* f = P<const float>(inc[k]);
            const float v0 = (1.f - dx) * (1.f - dy) * f[r00 + xi] + (dx) * (1.f - dy) * f[r00 + x1] + (1.f - dx) * (dy)*f[r10 + xi] +
                             (dx) * (dy)*f[r10 + x1];
            const float v1 = (1.f - dx) * (1.f - dy) * f[r01 + xi] + (dx) * (1.f - dy) * f[r01 + x1] + (1.f - dx) * (dy)*f[r11 + xi] +
                             (dx) * (dy)*f[r11 + x1];
            a[k] = a[k] + ((1.f - dz) * v0 + dz * v1);
          }
        }
        if (std::isnan(a[0])) ++n_lost;
        for (int k = 0; k < 3; ++k) P<float>(acc[k])[c] = a[k];
      }
  if (lost) *lost = n_lost;
  return 0;
}
