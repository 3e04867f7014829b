// The line routine of f3d_nearest_seed (include/f3d.h): the lower envelope of the parabolas f(v) + (i - v)^2 along one
// line of a volume, kept with a stack (Felzenszwalb-Huttenlocher / Meijster), written against one primitive set so that the same text
// runs in the kernels and in a host program under a sanitizer (tests/nearest_line_main.cpp).  Nothing else is included here.
//
// L is the line as the caller sees it and supplies
//   bool     sample(int v, unsigned* f, unsigned* tag)   whether position v carries a parabola; its height f < 2^31 and a word the
//                                                         caller wants back with it (which seed it stands for)
//   void     push(int k, unsigned e)                     entry k of the line's stack := e
//   unsigned entry(int k)                                entry k as pushed
//   void     emit(int i, int v, unsigned f, unsigned tag) position i belongs to the parabola at v (v < 0: the line has none)
//
// Definition.  Position i goes to the v that minimises the pair (f(v) + (i - v)^2, v): at equal height the smaller coordinate keeps it.
// Work.  Every position is pushed at most once and popped at most once, and the second loop moves forward only: linear in n whatever
// the input (a line with one parabola costs n emits and nothing else).  No loop waits for anything.
// Widths.  n <= 32768, so a coordinate and the start of a region fit 15 bits each and a stack entry is one word, v | start << 15.  The
// separator of the parabolas at u < v is the floor of num / den with num = f(v) - f(u) + v^2 - u^2 and den = 2 (v - u): f < 2^31 and
// 0 < v^2 - u^2 < 2^30 put num in (-2^31, 2^31 + 2^30), which a 32-bit word does not hold, so num is formed in 64 bits.  Its magnitude
// is below 2^32 on the positive side and below 2^31 on the negative side, and den <= 65534: floor(num / den) is one unsigned 32-bit
// division either way (-ceil(|num| / den) for a negative num, and |num| + den - 1 < 2^32).
#ifndef F3D_ENVELOPE_H_
#define F3D_ENVELOPE_H_

#ifndef F3D_ENV_FN
#define F3D_ENV_FN inline
#endif

namespace f3d_env {

constexpr int kCoordBits = 15;
constexpr unsigned kCoordMask = (1u << kCoordBits) - 1u;

// the first position at which the parabola at v (height fv) lies strictly below the one at u < v (height fu), cut to [0, n]
F3D_ENV_FN int first_win(int u, unsigned fu, int v, unsigned fv, int n)
{
  const long long num = static_cast<long long>(fv) - static_cast<long long>(fu) + static_cast<long long>(v * v - u * u);
  const unsigned den = 2u * static_cast<unsigned>(v - u);
  if (num < 0) {
    const unsigned up = (static_cast<unsigned>(-num) + den - 1u) / den;  // ceil(|num| / den) <= 2^30
    const int s = 1 - static_cast<int>(up);                             // floor(num / den) + 1
    return s < 0 ? 0 : s;
  }
  const unsigned q = static_cast<unsigned>(num) / den;  // floor, below 2^31
  return q >= static_cast<unsigned>(n) ? n : static_cast<int>(q) + 1;
}

template <typename L>
F3D_ENV_FN void line(L& io, int n)
{
  // the top of the stack stays in registers: its coordinate, height, tag and the start of its region
  int top = 0, u = 0, start_u = 0;
  unsigned fu = 0, tag_u = 0;
  for (int v = 0; v < n; ++v) {
    unsigned fv, tag_v;
    if (!io.sample(v, &fv, &tag_v)) continue;
    int s = 0;
    while (top > 0) {
      s = first_win(u, fu, v, fv, n);
      if (s > start_u) break;  // u keeps [start_u, s)
      --top;                   // v is strictly below u on all of u's region
      if (top > 0) {
        const unsigned e = io.entry(top - 1);
        u = static_cast<int>(e & kCoordMask);
        start_u = static_cast<int>(e >> kCoordBits);
        io.sample(u, &fu, &tag_u);
      }
    }
    if (top == 0) s = 0;
    if (s < n) {  // otherwise v wins nowhere on the line
      io.push(top, static_cast<unsigned>(v) | static_cast<unsigned>(s) << kCoordBits);
      ++top;
      u = v;
      fu = fv;
      tag_u = tag_v;
      start_u = s;
    }
  }
  if (top == 0) {
    for (int i = 0; i < n; ++i) io.emit(i, -1, 0u, 0u);
    return;
  }
  // the starts along the stack increase strictly and the first is 0: one step forward at a time
  int k = 0;
  u = static_cast<int>(io.entry(0) & kCoordMask);
  io.sample(u, &fu, &tag_u);
  int next = top > 1 ? static_cast<int>(io.entry(1) >> kCoordBits) : n;
  for (int i = 0; i < n; ++i) {
    if (i == next) {
      ++k;
      u = static_cast<int>(io.entry(k) & kCoordMask);
      io.sample(u, &fu, &tag_u);
      next = k + 1 < top ? static_cast<int>(io.entry(k + 1) >> kCoordBits) : n;
    }
    io.emit(i, u, fu, tag_u);
  }
}

}  // namespace f3d_env
#endif  // F3D_ENVELOPE_H_
