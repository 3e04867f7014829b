// csrc/f3d_envelope.h on the host: the line routine of f3d_nearest_seed over plain vectors behind its primitives, against the brute-force
// minimum of (f(v) + (i - v)^2, v) over the line, and its separator against plain 64-bit floor division.  Built with
// -fsanitize=address,undefined by tests/test_nearest_cpu.py; the stack and the outputs are vectors of exactly the line's length, so a
// push or an emit past the line is an error the sanitizer reports.  Prints one line per case and "ok envelope" at the end.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "f3d_envelope.h"

namespace {

constexpr unsigned kNone = 0xffffffffu;  // no parabola at this position

struct Line {
  const std::vector<unsigned>& f;
  std::vector<unsigned> stack;
  std::vector<int> owner;
  std::vector<unsigned> height, tags;
  long samples = 0, pushes = 0;
  explicit Line(const std::vector<unsigned>& heights) : f(heights), stack(heights.size()), owner(heights.size(), -2), height(heights.size()), tags(heights.size()) {}
  bool sample(int v, unsigned* out, unsigned* tag)
  {
    ++samples;
    if (f.at(v) == kNone) return false;
    *out = f[v];
    *tag = static_cast<unsigned>(v) * 7u + 1u;
    return true;
  }
  void push(int k, unsigned e)
  {
    ++pushes;
    stack.at(k) = e;
  }
  unsigned entry(int k) { return stack.at(k); }
  void emit(int i, int v, unsigned fv, unsigned tag)
  {
    owner.at(i) = v;
    height.at(i) = fv;
    tags.at(i) = tag;
  }
};

long check(const std::string& name, const std::vector<unsigned>& f)
{
  const int n = static_cast<int>(f.size());
  Line io(f);
  f3d_env::line(io, n);
  long wrong = 0;
  for (int i = 0; i < n; ++i) {
    int best = -1;
    unsigned long long best_d = 0;
    for (int v = 0; v < n; ++v) {
      if (f[v] == kNone) continue;
      const unsigned long long d = static_cast<unsigned long long>(f[v]) + static_cast<unsigned long long>((i - v) * (i - v));
      if (best < 0 || d < best_d) best = v, best_d = d;  // strictly: the smaller v keeps a tie
    }
    if (io.owner[i] != best) ++wrong;
    if (best >= 0 && (io.height[i] != f[best] || io.tags[i] != static_cast<unsigned>(best) * 7u + 1u)) ++wrong;
  }
  // linear work: a position is sampled once in the first loop, once more per pop or step, and pushed at most once
  if (io.pushes > n || io.samples > 4L * n + 4) ++wrong;
  std::printf("%s n=%d: %ld wrong\n", name.c_str(), n, wrong);
  return wrong;
}

long check_separator(std::mt19937& rng)
{
  long wrong = 0;
  const unsigned top = 0x7fffffffu - 2u * 32767u * 32767u;  // heights as large as two full axes leave
  for (int trial = 0; trial < 200000; ++trial) {
    const int n = 32768;
    int u = static_cast<int>(rng() % n), v = static_cast<int>(rng() % n);
    if (u == v) continue;
    if (u > v) std::swap(u, v);
    unsigned fu, fv;
    switch (trial % 4) {
      case 0: fu = rng() % 100, fv = rng() % 100; break;
      case 1: fu = 0x7fffffffu - rng() % 3, fv = rng() % 3; break;  // the most negative numerator
      case 2: fu = rng() % 3, fv = 0x7fffffffu - rng() % 3; break;  // the most positive one: 2^31 + v^2 - u^2
      default: fu = rng() % top, fv = rng() % top; break;
    }
    const long long num = static_cast<long long>(fv) - static_cast<long long>(fu) + static_cast<long long>(v) * v - static_cast<long long>(u) * u;
    const long long den = 2LL * (v - u);
    long long q = num / den;
    if (num % den != 0 && num < 0) --q;
    long long s = q + 1;
    s = s < 0 ? 0 : (s > n ? n : s);
    if (f3d_env::first_win(u, fu, v, fv, n) != s) ++wrong;
  }
  std::printf("separator: %ld wrong\n", wrong);
  return wrong;
}

}  // namespace

int main()
{
  std::mt19937 rng(11);
  long wrong = 0;
  for (int n : {1, 2, 63, 64, 65, 300}) {
    std::vector<unsigned> f(n);
    for (int i = 0; i < n; ++i) f[i] = 0;
    wrong += check("all-seeds", f);
    for (int i = 0; i < n; ++i) f[i] = kNone;
    wrong += check("none", f);
    f[0] = 0;
    wrong += check("first", f);
    f[0] = kNone;
    f[n - 1] = 5;
    wrong += check("last", f);
    f[0] = 5;
    wrong += check("both-ends", f);
    for (int i = 0; i < n; ++i) f[i] = i % 2 ? kNone : 0u;
    wrong += check("alternating", f);
    for (int i = 0; i < n; ++i) f[i] = i % 2 ? 0u : 1u;
    wrong += check("alternating-heights", f);
    // every separator an exact tie: the parabolas at u and u + 2 with equal heights meet exactly at u + 1, and
    // f(v) = c - v^2 + 2 v m puts every pair's separator on the integer m
    for (int i = 0; i < n; ++i) f[i] = i % 2 ? kNone : 9u;
    wrong += check("ties-midway", f);
    for (int m : {0, n / 2, n - 1}) {
      for (int i = 0; i < n; ++i) f[i] = static_cast<unsigned>(100000 + (i - m) * (i - m) - 2 * (i - m) * (i - m));  // c - (i - m)^2
      wrong += check("ties-all-at-" + std::to_string(m), f);
    }
    for (int i = 0; i < n; ++i) f[i] = static_cast<unsigned>(i * i);  // ever steeper: nothing is ever popped
    wrong += check("rising", f);
    for (int i = 0; i < n; ++i) f[i] = static_cast<unsigned>((n - i) * (n - i) * 4);  // every push pops what is there
    wrong += check("falling", f);
    for (int i = 0; i < n; ++i) f[i] = i == n / 2 ? 0u : 0x7ffe0000u;  // one pore in a solid line
    wrong += check("one-low", f);
    for (double density : {0.02, 0.1, 0.5, 1.0})
      for (unsigned range : {1u, 4u, 50u, 100000u, 0x7ffe0000u}) {
        for (int i = 0; i < n; ++i) f[i] = (rng() % 1000) < density * 1000 ? rng() % range : kNone;
        wrong += check("random-" + std::to_string(density) + "-" + std::to_string(range), f);
      }
  }
  wrong += check_separator(rng);
  if (wrong) {
    std::printf("FAILED: %ld\n", wrong);
    return 1;
  }
  std::printf("ok envelope\n");
  return 0;
}
