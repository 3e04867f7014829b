// The bin rule of f3d_histogram (include/f3d.h) and the ordered integer key of a float32, written once so that the same
// text runs in the kernels and on the host: in the device library's argument checks, in host/threshold_select.cpp (the bisection of
// f3d_histogram_edge) and in a stand-alone program under a sanitizer (tests/histogram_host_main.cpp).  Nothing but <cmath> and
// <cstring> is included here.
//
// The rule.  With lo < hi both finite, bins in 1 .. kMaxBins and scale = (float)bins / (hi - lo) formed once in float32, a value s
// takes part when lo <= s && s <= hi (a NaN never does) and its bin is min((int)((s - lo) * scale), bins - 1).  The subtraction and
// the product are each rounded to float32 -- every translation unit that includes this is built with contraction off, and a
// subtraction followed by a product has nothing to contract anyway -- and the conversion truncates.  Each step is monotone in s, so
// every bin is an interval of floats, and s == hi lands in the last bin.  For s in [lo, hi] the product lies in [0, bins * (1 + 2^-22)],
// far inside int.
#ifndef F3D_HISTOGRAM_BIN_H_
#define F3D_HISTOGRAM_BIN_H_

#include <cmath>
#include <cstring>

#ifndef F3D_HIST_FN
#define F3D_HIST_FN inline
#endif

namespace f3d_hist {

constexpr int kMaxBins = 4096;

struct Rule {
  float lo, hi, scale;
  int bins;
};

// the classes of f3d_histogram_info, in the order in which a voxel is tried against them (kMasked is decided by the caller)
enum Class { kMasked = 0, kNan = 1, kBelow = 2, kAbove = 3, kUsed = 4, kClasses = 5 };

// null when (lo, hi, bins) is a rule, which is then in *rule; otherwise what is wrong with it
inline const char* make_rule(float lo, float hi, long long bins, Rule* rule)
{
  if (!std::isfinite(lo) || !std::isfinite(hi)) return "lo and hi must be finite";
  if (!(lo < hi)) return "lo must be below hi";
  if (bins < 1 || bins > kMaxBins) return "bins must be 1 .. 4096";
  const float width = hi - lo;
  if (!std::isfinite(width) || !(width > 0.f)) return "hi - lo is not finite and positive in float32";
  const float scale = static_cast<float>(bins) / width;
  if (!std::isfinite(scale) || !(scale > 0.f)) return "bins / (hi - lo) is not finite and positive in float32";
  rule->lo = lo;
  rule->hi = hi;
  rule->scale = scale;
  rule->bins = static_cast<int>(bins);
  return nullptr;
}

F3D_HIST_FN int class_of(const Rule& r, float s)
{
  if (s != s) return kNan;
  if (s < r.lo) return kBelow;
  if (s > r.hi) return kAbove;
  return kUsed;
}

// the bin of a value of class kUsed
F3D_HIST_FN int bin_of(const Rule& r, float s)
{
  const float offset = s - r.lo;
  const float scaled = offset * r.scale;
  const int b = static_cast<int>(scaled);
  return b < r.bins - 1 ? b : r.bins - 1;
}

// The totally ordered key of a float's bits: a < b as floats gives key(a) < key(b), -0.0f lies directly below +0.0f, a denormal keeps
// its place, the negative NaNs lie below -inf and the positive ones above +inf.
F3D_HIST_FN unsigned key_of_bits(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
F3D_HIST_FN unsigned bits_of_key(unsigned key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

inline unsigned key_of(float s)
{
  unsigned bits;
  std::memcpy(&bits, &s, sizeof(bits));
  return key_of_bits(bits);
}
inline float float_of_key(unsigned key)
{
  const unsigned bits = bits_of_key(key);
  float s;
  std::memcpy(&s, &bits, sizeof(s));
  return s;
}

}  // namespace f3d_hist
#endif  // F3D_HISTOGRAM_BIN_H_
