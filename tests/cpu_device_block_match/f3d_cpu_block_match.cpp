// TEST INFRASTRUCTURE: f3d_block_match and f3d_expand_nodes (include/f3d_block_match.h) for the host-memory stand-in of
// tests/cpu_device, and the two other entries the driver's block matching path calls and no stand-in had: f3d_value_range and
// f3d_validate_displacement (include/f3d.h).  Plain loops, the definitions of the headers word for word; the geometry comes from the
// stand-in's own f3d_get_container.  This directory's Makefile builds the stand-in with these, tests/cpu_device_initial's
// f3d_initial_flow beside them, the product's host library against it and the command-line tool on top.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "f3d_block_match.h"
#include "../../cuda-flow3d_amd/csrc/f3d_histogram_bin.h"

namespace {

template <typename T>
T* P(f3d_devptr p) { return reinterpret_cast<T*>(static_cast<uintptr_t>(p)); }

struct Box {
  size_t w, h, d, pitch_f, rows;
  size_t at(size_t x, size_t y, size_t z) const { return (z * rows + y) * pitch_f + x; }
};

// the box fits the current container
bool geometry(size_t w, size_t h, size_t d, Box* box)
{
  f3d_size4 c;
  if (f3d_get_container(&c) != 0 || c.pitch == 0 || c.height == 0) return false;
  if (w == 0 || h == 0 || d == 0 || w > c.width || h > c.height || d > c.depth || w * sizeof(float) > c.pitch) return false;
  *box = {w, h, d, c.pitch / sizeof(float), c.height};
  return true;
}

int code_of(const f3d_hist::Rule& r, float s)
{
  if (s != s || s < r.lo) return 0;
  if (s > r.hi) return r.bins - 1;
  return f3d_hist::bin_of(r, s);
}

struct Sums {
  long long sb, sbb, sab;
};

// the median of the first k of 26 ascending values by index, as the definition has it: the middle one, or half the sum of the two
float median_by_index(const float* sorted, int k)
{
  if (k == 0) return 0.f;
  const float lo = sorted[(k - 1) / 2], hi = sorted[k / 2];
  return k % 2 == 1 ? hi : 0.5f * (lo + hi);
}

}  // namespace

extern "C" int f3d_value_range(f3d_devptr src, f3d_devptr mask, size_t width, size_t height, size_t depth, float* min, float* max,
                               f3d_range_info* info)
{
  Box b;
  if (!src || !min || !max || !geometry(width, height, depth, &b)) return 1;
  unsigned lo_key = 0xffffffffu, hi_key = 0u;
  unsigned long long finite = 0;
  for (size_t z = 0; z < depth; ++z)
    for (size_t y = 0; y < height; ++y)
      for (size_t x = 0; x < width; ++x) {
        const size_t c = b.at(x, y, z);
        if (mask && P<const int>(mask)[c] == 0) continue;
        const float s = P<const float>(src)[c];
        if (!std::isfinite(s)) continue;
        ++finite;
        const unsigned key = f3d_hist::key_of(s);
        lo_key = std::min(lo_key, key);
        hi_key = std::max(hi_key, key);
      }
  *min = finite ? f3d_hist::float_of_key(lo_key) : std::numeric_limits<float>::infinity();
  *max = finite ? f3d_hist::float_of_key(hi_key) : -std::numeric_limits<float>::infinity();
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->finite = finite;  // the only counter the driver's block matching path reads
  }
  return 0;
}

extern "C" int f3d_validate_displacement(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight, float weight_min, unsigned step,
                                         float eps, float threshold, unsigned min_neighbours, unsigned mode, const f3d_devptr out[4],
                                         unsigned fields, size_t width, size_t height, size_t depth, f3d_validate_stats* stats)
{
  Box b;
  if (!u || !v || !w || !out || step < 1 || !geometry(width, height, depth, &b)) return 1;
  if (mode != F3D_VALIDATE_MARK && mode != F3D_VALIDATE_REPLACE) return 1;
  if (fields == 0 || (fields & ~(F3D_VALIDATE_R | F3D_VALIDATE_D))) return 1;
  if ((fields & F3D_VALIDATE_R) && !out[0]) return 1;
  if ((fields & F3D_VALIDATE_D) && (!out[1] || !out[2] || !out[3])) return 1;
  const float* in[3] = {P<const float>(u), P<const float>(v), P<const float>(w)};
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const long long W = static_cast<long long>(width), H = static_cast<long long>(height), D = static_cast<long long>(depth);
  auto present = [&](long long x, long long y, long long z) {
    const size_t c = b.at(x, y, z);
    if (std::isnan(in[0][c]) || std::isnan(in[1][c]) || std::isnan(in[2][c])) return false;
    return !weight || P<const float>(weight)[c] >= weight_min;  // a NaN weight fails the comparison
  };
  // results first, stores afterwards: an output is never an input, but every voxel reads its neighbours' inputs
  const size_t n = width * height * depth;
  std::vector<float> r_out(n), d_out[3] = {std::vector<float>(n), std::vector<float>(n), std::vector<float>(n)};
  f3d_validate_stats st = {};
  float r_max = nan;
  size_t at = 0;
  for (long long z = 0; z < D; ++z)
    for (long long y = 0; y < H; ++y)
      for (long long x = 0; x < W; ++x, ++at) {
        const size_t c = b.at(x, y, z);
        float med[3], r = 0.f;
        int k = 0;
        for (int comp = 0; comp < 3; ++comp) {
          float list[26], res[26];
          int slot = 0;
          k = 0;
          for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx) {
                if (!dx && !dy && !dz) continue;
                const long long xx = x + dx * static_cast<long long>(step), yy = y + dy * static_cast<long long>(step),
                                zz = z + dz * static_cast<long long>(step);
                float value = inf;
                if (xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D && present(xx, yy, zz)) value = in[comp][b.at(xx, yy, zz)];
                list[slot++] = value;
                if (std::isfinite(value)) ++k;
              }
          std::sort(list, list + 26);
          med[comp] = median_by_index(list, k);
          for (int i = 0; i < 26; ++i) res[i] = std::fabs(list[i] - med[comp]);
          std::sort(res, res + 26);
          const float rm = median_by_index(res, k);
          const float part = std::fabs(in[comp][c] - med[comp]) / (rm + eps);
          r = comp == 0 ? part : std::fmax(r, part);
        }
        const bool is_present = present(x, y, z), enough = k >= static_cast<int>(min_neighbours);
        const bool tested = is_present && enough, outlier = tested && r > threshold;
        const bool kept = is_present && !outlier, median = !kept && enough && mode == F3D_VALIDATE_REPLACE;
        for (int comp = 0; comp < 3; ++comp) d_out[comp][at] = kept ? in[comp][c] : (median ? med[comp] + 0.f : nan);
        r_out[at] = tested ? r : nan;
        st.present += is_present;
        st.tested += tested;
        st.outliers += outlier;
        st.replaced += median;
        st.undefined += std::isnan(d_out[0][at]);
        if (tested && !(r_max >= r)) r_max = r;
      }
  st.r_max = r_max;
  at = 0;
  for (size_t z = 0; z < depth; ++z)
    for (size_t y = 0; y < height; ++y)
      for (size_t x = 0; x < width; ++x, ++at) {
        const size_t c = b.at(x, y, z);
        if (fields & F3D_VALIDATE_R) P<float>(out[0])[c] = r_out[at];
        if (fields & F3D_VALIDATE_D)
          for (int comp = 0; comp < 3; ++comp) P<float>(out[1 + comp])[c] = d_out[comp][at];
      }
  if (stats) *stats = st;
  return 0;
}

extern "C" int f3d_block_match(f3d_devptr a, f3d_devptr b, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                               const f3d_block_match_grid* grid, const int* centre, f3d_block_match_record* records,
                               f3d_block_match_info* info)
{
  Box box;
  f3d_hist::Rule rule;
  if (!a || !b || !grid || !records || bins < 2 || bins > F3D_BLOCK_MATCH_MAX_BINS) return 1;
  if (f3d_hist::make_rule(lo, hi, static_cast<long long>(bins), &rule)) return 1;
  const f3d_block_match_grid& q = *grid;
  if (q.step < 1 || q.nx < 1 || q.ny < 1 || q.nz < 1 || static_cast<unsigned long long>(q.nx) * q.ny * q.nz > F3D_BLOCK_MATCH_MAX_NODES)
    return 1;
  if (q.window < 1 || q.window > F3D_BLOCK_MATCH_MAX_WINDOW || q.rx < 0 || q.ry < 0 || q.rz < 0) return 1;
  if (q.window + std::max(q.rx, std::max(q.ry, q.rz)) > F3D_BLOCK_MATCH_MAX_REACH) return 1;
  if (!geometry(width, height, depth, &box)) return 1;
  const long long dims[3] = {static_cast<long long>(width), static_cast<long long>(height), static_cast<long long>(depth)};
  const long long first[3] = {q.ox, q.oy, q.oz}, counts[3] = {q.nx, q.ny, q.nz};
  for (int axis = 0; axis < 3; ++axis)
    if (first[axis] - q.window < 0 || first[axis] + (counts[axis] - 1) * q.step + q.window > dims[axis] - 1) return 1;
  const size_t nodes = static_cast<size_t>(q.nx) * q.ny * q.nz;
  if (centre)
    for (size_t i = 0; i < 3 * nodes; ++i)
      if (centre[i] < -(1 << 20) || centre[i] > (1 << 20)) return 1;

  const int W = q.window, side = 2 * W + 1, radius[3] = {q.rx, q.ry, q.rz};
  const long long n = static_cast<long long>(side) * side * side;
  const float* fa = P<const float>(a);
  const float* fb = P<const float>(b);
  std::vector<f3d_block_match_record> found(nodes);
  std::vector<int> win(static_cast<size_t>(n));
  size_t node = 0;
  for (int k = 0; k < q.nz; ++k)
    for (int j = 0; j < q.ny; ++j)
      for (int i = 0; i < q.nx; ++i, ++node) {
        f3d_block_match_record rec = {};
        const long long p[3] = {q.ox + static_cast<long long>(i) * q.step, q.oy + static_cast<long long>(j) * q.step,
                                q.oz + static_cast<long long>(k) * q.step};
        const long long c[3] = {centre ? centre[3 * node] : 0, centre ? centre[3 * node + 1] : 0, centre ? centre[3 * node + 2] : 0};
        long long sa = 0, saa = 0;
        size_t t = 0;
        for (int z = -W; z <= W; ++z)
          for (int y = -W; y <= W; ++y)
            for (int x = -W; x <= W; ++x, ++t) {
              const float s = fa[box.at(p[0] + x, p[1] + y, p[2] + z)];
              rec.nan += s != s;
              win[t] = code_of(rule, s);
              sa += win[t];
              saa += static_cast<long long>(win[t]) * win[t];
            }
        rec.sa = static_cast<int>(sa);
        rec.saa = static_cast<int>(saa);
        // the sums of a shift d from the centre; false when its window leaves the box
        auto sums = [&](const long long d[3], Sums* s) {
          long long lo3[3];
          for (int axis = 0; axis < 3; ++axis) {
            lo3[axis] = p[axis] + c[axis] + d[axis] - W;
            if (lo3[axis] < 0 || lo3[axis] + side > dims[axis]) return false;
          }
          *s = {0, 0, 0};
          size_t tt = 0;
          for (int z = 0; z < side; ++z)
            for (int y = 0; y < side; ++y)
              for (int x = 0; x < side; ++x, ++tt) {
                const long long code = code_of(rule, fb[box.at(lo3[0] + x, lo3[1] + y, lo3[2] + z)]);
                s->sb += code;
                s->sbb += code * code;
                s->sab += code * win[tt];
              }
          return true;
        };
        if (n * saa - sa * sa == 0) {
          rec.status = F3D_BLOCK_MATCH_FLAT;
          found[node] = rec;
          continue;
        }
        bool have = false;
        double best_score = 0.0;
        long long best[3] = {0, 0, 0};
        Sums best_sums = {0, 0, 0};
        for (long long dz = -q.rz; dz <= q.rz; ++dz)
          for (long long dy = -q.ry; dy <= q.ry; ++dy)
            for (long long dx = -q.rx; dx <= q.rx; ++dx) {
              const long long d[3] = {dx, dy, dz};
              Sums s;
              if (!sums(d, &s)) {
                ++rec.outside;
                continue;
              }
              const long long db = n * s.sbb - s.sb * s.sb;
              if (db == 0) {
                ++rec.flat;
                continue;
              }
              ++rec.evaluated;
              const double num = static_cast<double>(n * s.sab - sa * s.sb);
              const double squared = num * std::fabs(num);
              const double score = squared / static_cast<double>(db);
              if (!have || score > best_score) {  // ties keep the earlier, smaller index
                have = true;
                best_score = score;
                best_sums = s;
                for (int axis = 0; axis < 3; ++axis) best[axis] = d[axis];
              }
            }
        if (!have) {
          rec.status = F3D_BLOCK_MATCH_NONE;
          found[node] = rec;
          continue;
        }
        rec.status = F3D_BLOCK_MATCH_OK;
        for (int axis = 0; axis < 3; ++axis) rec.shift[axis] = static_cast<int>(c[axis] + best[axis]);
        rec.best[0] = static_cast<int>(best_sums.sb), rec.best[1] = static_cast<int>(best_sums.sbb), rec.best[2] = static_cast<int>(best_sums.sab);
        for (int face = 0; face < 6; ++face) {
          long long d[3] = {best[0], best[1], best[2]};
          d[face / 2] += face % 2 ? 1 : -1;
          Sums s;
          if (d[face / 2] < -radius[face / 2] || d[face / 2] > radius[face / 2] || !sums(d, &s) || n * s.sbb - s.sb * s.sb == 0) continue;
          rec.neighbour[face][0] = static_cast<int>(s.sb), rec.neighbour[face][1] = static_cast<int>(s.sbb);
          rec.neighbour[face][2] = static_cast<int>(s.sab);
          rec.valid |= 1 << face;
        }
        found[node] = rec;
      }
  std::memcpy(records, found.data(), nodes * sizeof(f3d_block_match_record));
  if (info) {
    f3d_block_match_info t = {};
    t.nodes = nodes;
    for (const f3d_block_match_record& r : found) {
      t.ok += r.status == F3D_BLOCK_MATCH_OK;
      t.flat_nodes += r.status == F3D_BLOCK_MATCH_FLAT;
      t.none_nodes += r.status == F3D_BLOCK_MATCH_NONE;
      t.evaluated += static_cast<unsigned long long>(r.evaluated);
      t.outside += static_cast<unsigned long long>(r.outside);
      t.flat += static_cast<unsigned long long>(r.flat);
      t.nan += static_cast<unsigned long long>(r.nan);
    }
    *info = t;
  }
  return 0;
}

extern "C" int f3d_expand_nodes(const float* u, const float* v, const float* w, int ox, int oy, int oz, int step, int nx, int ny, int nz,
                                f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height, size_t depth)
{
  Box b;
  if (!u || !v || !w || !out_u || !out_v || !out_w || out_u == out_v || out_u == out_w || out_v == out_w) return 1;
  if (step < 1 || nx < 1 || ny < 1 || nz < 1 || static_cast<unsigned long long>(nx) * ny * nz > F3D_BLOCK_MATCH_MAX_NODES) return 1;
  const int limit = 1 << 20;
  if (ox < -limit || ox > limit || oy < -limit || oy > limit || oz < -limit || oz > limit) return 1;
  if (!geometry(width, height, depth, &b)) return 1;
  auto cell = [&](size_t x, int origin, int count, int* i, float* f) {
    const float t = (static_cast<float>(x) - static_cast<float>(origin)) / static_cast<float>(step);
    int lower = static_cast<int>(std::floor(t));
    lower = std::min(std::max(lower, 0), std::max(count - 2, 0));
    const float fraction = t - static_cast<float>(lower);
    *i = lower;
    *f = fraction < 0.f ? 0.f : (fraction > 1.f ? 1.f : fraction);
  };
  auto lerp = [](float p, float q, float f) {
    const float step_pq = q - p;
    const float part = f * step_pq;
    return p + part;
  };
  const float* node[3] = {u, v, w};
  const f3d_devptr out[3] = {out_u, out_v, out_w};
  for (size_t z = 0; z < depth; ++z)
    for (size_t y = 0; y < height; ++y)
      for (size_t x = 0; x < width; ++x) {
        int i, j, k;
        float fx, fy, fz;
        cell(x, ox, nx, &i, &fx);
        cell(y, oy, ny, &j, &fy);
        cell(z, oz, nz, &k, &fz);
        for (int comp = 0; comp < 3; ++comp) {
          const float* f = node[comp];
          auto along_x = [&](int jj, int kk) {
            const size_t row = (static_cast<size_t>(kk) * ny + jj) * nx;
            return nx > 1 ? lerp(f[row + i], f[row + i + 1], fx) : f[row];
          };
          auto along_y = [&](int kk) { return ny > 1 ? lerp(along_x(j, kk), along_x(j + 1, kk), fy) : along_x(0, kk); };
          P<float>(out[comp])[b.at(x, y, z)] = nz > 1 ? lerp(along_y(k), along_y(k + 1), fz) : along_y(0);
        }
      }
  return 0;
}
