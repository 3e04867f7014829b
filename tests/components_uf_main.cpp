// The union-find of f3d_label_components (cuda-flow3d_amd/csrc/f3d_union_find.h) on the host: the header's find, unite and flatten with
// std::atomic behind its three primitives, run by several threads over the faces of a volume in an interleaved order, and compared with
// a sequential flood fill -- every voxel's parent must end as the smallest linear index of its component.  A stand-alone program, built
// with -fsanitize=address,undefined by tests/test_components_cpu.py; it takes no arguments and prints one line per case.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "f3d_union_find.h"

namespace {

struct Parents {
  std::atomic<unsigned>* p;
  unsigned load(unsigned i) const { return p[i].load(std::memory_order_relaxed); }
  unsigned fetch_min(unsigned i, unsigned v) const
  {
    unsigned seen = p[i].load(std::memory_order_relaxed);
    while (v < seen && !p[i].compare_exchange_weak(seen, v, std::memory_order_relaxed)) {
    }
    return seen;
  }
  void store(unsigned i, unsigned v) const { p[i].store(v, std::memory_order_relaxed); }
};

struct Volume {
  int w, h, d;
  std::vector<char> mask;
  unsigned index(int x, int y, int z) const { return static_cast<unsigned>(x + w * (y + h * z)); }
};

// tests/components_ref.py, serpentine
Volume serpentine(int w, int h, int d, bool mirrored)
{
  Volume v{w, h, d, std::vector<char>(static_cast<size_t>(w) * h * d, 0)};
  const int last = h - 1;
  const int end_x = (((last % 2 == 0 ? last : last - 1) / 2) % 2 == 0) ? w - 1 : 0;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        bool on;
        if (z % 2 == 0)
          on = y % 2 == 0 || x == ((((y - 1) / 2) % 2 == 0) ? w - 1 : 0);
        else
          on = (((z - 1) / 2) % 2 == 0) ? (y == last && x == end_x) : (y == 0 && x == 0);
        const unsigned i = mirrored ? v.index(w - 1 - x, h - 1 - y, d - 1 - z) : v.index(x, y, z);
        v.mask[i] = on ? 1 : 0;
      }
  return v;
}

Volume noise(int w, int h, int d, double p, uint64_t state)
{
  Volume v{w, h, d, std::vector<char>(static_cast<size_t>(w) * h * d, 0)};
  for (char& m : v.mask) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    m = static_cast<double>(state >> 11) / 9007199254740992.0 < p ? 1 : 0;
  }
  return v;
}

// the smallest linear index of every voxel's component (kBackground for background), by a sequential flood fill
std::vector<unsigned> flood(const Volume& v)
{
  const size_t n = v.mask.size();
  std::vector<unsigned> root(n, f3d_uf::kBackground);
  std::vector<unsigned> stack;
  for (unsigned s = 0; s < n; ++s) {
    if (!v.mask[s] || root[s] != f3d_uf::kBackground) continue;
    root[s] = s;
    stack.push_back(s);
    while (!stack.empty()) {
      const unsigned i = stack.back();
      stack.pop_back();
      const int x = static_cast<int>(i % v.w), y = static_cast<int>(i / v.w % v.h), z = static_cast<int>(i / v.w / v.h);
      const int step[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
      for (const int* s3 : step) {
        const int nx = x + s3[0], ny = y + s3[1], nz = z + s3[2];
        if (nx < 0 || ny < 0 || nz < 0 || nx >= v.w || ny >= v.h || nz >= v.d) continue;
        const unsigned j = v.index(nx, ny, nz);
        if (v.mask[j] && root[j] == f3d_uf::kBackground) {
          root[j] = s;
          stack.push_back(j);
        }
      }
    }
  }
  return root;
}

bool run(const char* name, const Volume& v, int n_threads)
{
  const unsigned n = static_cast<unsigned>(v.mask.size());
  std::unique_ptr<std::atomic<unsigned>[]> cells(new std::atomic<unsigned>[n]);
  Parents parent{cells.get()};
  for (unsigned i = 0; i < n; ++i) parent.store(i, v.mask[i] ? i : f3d_uf::kBackground);
  auto in_parallel = [&](auto&& body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < n_threads; ++t) pool.emplace_back([&, t] { body(t); });
    for (std::thread& t : pool) t.join();
  };
  // the merge pass: thread t takes voxels t, t + T, ... -- neighbours in x go to different threads -- and thread t walks them from the
  // far end when t is odd, so that long chains are met from both sides
  in_parallel([&](int t) {
    const unsigned first = static_cast<unsigned>(t), stride = static_cast<unsigned>(n_threads);
    const unsigned count = first < n ? (n - first + stride - 1) / stride : 0;
    for (unsigned k = 0; k < count; ++k) {
      const unsigned i = first + stride * (t % 2 ? count - 1 - k : k);
      if (!v.mask[i]) continue;
      const int x = static_cast<int>(i % v.w), y = static_cast<int>(i / v.w % v.h), z = static_cast<int>(i / v.w / v.h);
      if (x + 1 < v.w && v.mask[i + 1]) f3d_uf::unite(parent, i, i + 1);
      if (y + 1 < v.h && v.mask[i + v.w]) f3d_uf::unite(parent, i, i + static_cast<unsigned>(v.w));
      if (z + 1 < v.d && v.mask[i + static_cast<unsigned>(v.w * v.h)]) f3d_uf::unite(parent, i, i + static_cast<unsigned>(v.w * v.h));
    }
  });
  // the flatten pass, after every unite has returned
  in_parallel([&](int t) {
    for (unsigned i = static_cast<unsigned>(t); i < n; i += static_cast<unsigned>(n_threads))
      if (v.mask[i]) f3d_uf::flatten(parent, i);
  });
  const std::vector<unsigned> want = flood(v);
  size_t wrong = 0, bodies = 0;
  for (unsigned i = 0; i < n; ++i) {
    wrong += parent.load(i) != want[i];
    bodies += want[i] == i;
  }
  std::printf("%s %dx%dx%d threads %d: %zu bodies, %zu wrong\n", name, v.w, v.h, v.d, n_threads, bodies, wrong);
  return wrong == 0;
}

}  // namespace

int main()
{
  bool good = true;
  for (int threads : {1, 2, 7}) {
    good &= run("serpentine", serpentine(33, 9, 7, false), threads);
    good &= run("serpentine-mirrored", serpentine(33, 9, 7, true), threads);
    good &= run("serpentine-flat", serpentine(130, 6, 1, false), threads);
    good &= run("noise-0.31", noise(65, 17, 19, 0.31, 7), threads);
    good &= run("noise-0.6", noise(40, 20, 10, 0.6, 11), threads);
  }
  std::printf(good ? "ok union-find\n" : "FAILED union-find\n");
  return good ? 0 : 1;
}
