// TEST PROGRAM: the host-memory f3d_initial_flow of tests/cpu_device_initial at its boundary cases, built with its own main under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpu_device_initial/Makefile, target main).  Widths 1, 63, 64, 65 in containers
// allocated to the byte, out of place and in place, with values that are not finite at the first and the last voxel; every result is
// checked against what the definition of include/f3d.h says.  Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "f3d.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, size_t w)
{
  if (!ok) {
    std::printf("FAILED: %s (width %zu)\n", what, w);
    ++failures;
  }
}

f3d_devptr dev(std::vector<float>& v) { return static_cast<f3d_devptr>(reinterpret_cast<uintptr_t>(v.data())); }

void run(size_t w, size_t h, size_t d, bool in_place)
{
  // the container is the box: the last voxel of the box is the last float of the allocation
  const f3d_size4 c = {w, h, d, w * sizeof(float)};
  expect(f3d_set_container(&c) == 0, "f3d_set_container", w);
  const size_t n = w * h * d;
  std::vector<float> in[3], out[3];
  for (int k = 0; k < 3; ++k) {
    in[k].assign(n, 0.25f * static_cast<float>(k + 1));
    out[k].assign(n, -7.f);
  }
  const float inf = std::numeric_limits<float>::infinity();
  in[0][0] = std::nanf("");    // the first voxel
  in[2][n - 1] = -inf;         // the last one (the same voxel when n == 1: still one replaced voxel)
  if (n > 2) in[1][1] = -0.f;
  const std::vector<float> u0 = in[0], v0 = in[1], w0 = in[2];
  std::vector<float>* dst = in_place ? in : out;
  f3d_initial_info info;
  std::memset(&info, 0xff, sizeof(info));
  expect(f3d_initial_flow(dev(in[0]), dev(in[1]), dev(in[2]), dev(dst[0]), dev(dst[1]), dev(dst[2]), w, h, d, &info) == 0, "the call", w);
  const unsigned long long holes = n == 1 ? 1 : 2;
  expect(info.voxels == n && info.replaced == holes, "voxels / replaced", w);
  // x + 0.25 leaves only where x = w - 1 (0.25 past the last sample); y + 0.5 and z + 0.75 likewise on the last row and plane
  unsigned long long leaving = 0;
  for (size_t z = 0; z < d; ++z)
    for (size_t y = 0; y < h; ++y)
      for (size_t x = 0; x < w; ++x) {
        const size_t i = (z * h + y) * w + x;
        const bool finite = std::isfinite(u0[i]) && std::isfinite(v0[i]) && std::isfinite(w0[i]);
        if (finite && (x == w - 1 || y == h - 1 || z == d - 1)) ++leaving;
        const float e[3] = {finite ? u0[i] : 0.f, finite ? v0[i] : 0.f, finite ? w0[i] : 0.f};
        for (int k = 0; k < 3; ++k) expect(std::memcmp(&dst[k][i], &e[k], sizeof(float)) == 0, "a component's bits", w);
      }
  expect(info.leaving == leaving, "leaving", w);
  expect(info.max_abs == (n > holes ? 0.75f : 0.f), "max_abs", w);
  // info is optional
  expect(f3d_initial_flow(dev(in[0]), dev(in[1]), dev(in[2]), dev(dst[0]), dev(dst[1]), dev(dst[2]), w, h, d, nullptr) == 0, "without info", w);
}

}  // namespace

int main()
{
  f3d_init(-1);
  for (size_t w : {size_t(1), size_t(63), size_t(64), size_t(65)})
    for (bool in_place : {false, true}) {
      run(w, 1, 1, in_place);
      run(w, 3, 2, in_place);
    }
  // refusals: a null container, a zero dimension, a box larger than the container, an output that is another component's input
  std::vector<float> a(8, 0.f), b(8, 0.f), c(8, 0.f);
  const f3d_size4 box = {2, 2, 2, 2 * sizeof(float)};
  f3d_set_container(&box);
  expect(f3d_initial_flow(0, dev(b), dev(c), dev(a), dev(b), dev(c), 2, 2, 2, nullptr) != 0, "a null input is refused", 2);
  expect(f3d_initial_flow(dev(a), dev(b), dev(c), dev(a), dev(b), 0, 2, 2, 2, nullptr) != 0, "a null output is refused", 2);
  expect(f3d_initial_flow(dev(a), dev(b), dev(c), dev(a), dev(b), dev(c), 0, 2, 2, nullptr) != 0, "a zero width is refused", 2);
  expect(f3d_initial_flow(dev(a), dev(b), dev(c), dev(a), dev(b), dev(c), 3, 2, 2, nullptr) != 0, "a box wider than the container is refused", 2);
  expect(f3d_initial_flow(dev(a), dev(b), dev(c), dev(a), dev(b), dev(c), 2, 2, 3, nullptr) != 0, "a box deeper than the container is refused", 2);
  expect(f3d_initial_flow(dev(a), dev(b), dev(c), dev(b), dev(a), dev(c), 2, 2, 2, nullptr) != 0, "swapped components are refused", 2);
  f3d_shutdown();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
