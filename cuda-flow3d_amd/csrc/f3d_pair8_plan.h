// How a fused solver launch (k_pair8, f3d_solve_pair8.h) is cut into workgroups: the plan (host, pure arithmetic) and the decode of
// a workgroup number into its tile and its planes (host AND device: ONE function, pair8_decode, compiled into the kernel's prologue
// and into the host C API, host/host_capi.cpp: f3d_pair8_plan / f3d_pair8_decode -- so the tests walk the very decode the kernel runs
// without a GPU).  Nothing here touches a voxel: every plan gives the same bits (each plane of each tile is computed once, from
// inputs only), plans differ in time alone.
#pragma once

#include <algorithm>
#include <cstdlib>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define F3D_PAIR8_PLAN_OWN_QUALIFIERS
#endif

constexpr int kPair8Lanes = 64;   // columns of a tile

// Tiles of a level, numbered x first.  With a folded last column (`fold`) a pair of tile rows (ty, ty + 1), ty even, is numbered: the
// ntx - 1 regular tiles of row ty, the folded tile, the regular tiles of row ty + 1 -- so the folded tile marches in step with its y
// neighbours; with nty odd the last row is alone with its folded tile (whose band B is empty).
__host__ __device__ inline int pair8_tiles_per_chunk(int ntx, int nty, bool fold)
{
  return fold ? (ntx - 1) * nty + (nty + 1) / 2 : ntx * nty;
}
// F3D_PAIR8_FOLD=0 keeps one band per tile everywhere (A/B timing and the tests; read per call like F3D_PAIR8_TY): the same results
inline bool pair8_folds(int width, int rows, int ty)
{
  const char* e = std::getenv("F3D_PAIR8_FOLD");
  if (e && e[0] == '0') return false;
  const int rem = width % kPair8Lanes;
  return rem >= 1 && rem <= kPair8Lanes / 2 && width > kPair8Lanes && rows > ty;   // ntx >= 2, nty >= 2
}

// The cut of a launch: two classes of tiles, in the tile numbering above.  Class A -- tiles 0 .. tiles_a-1 -- is cut into chunks_a
// chunks of zc_a planes per tile, class B -- the other tiles_b tiles -- into chunks_b chunks of zc_b planes.  The uniform cut every
// level had before is tiles_a = 0.  Handed to the kernel by value.
struct Pair8Cut {
  int tiles_a, chunks_a, zc_a;
  int tiles_b, chunks_b, zc_b;
};
__host__ __device__ inline int pair8_cut_wgs(const Pair8Cut& c) { return c.tiles_a * c.chunks_a + c.tiles_b * c.chunks_b; }
// Workgroups are dealt to the eight XCDs round-robin; with `xcd_remap` every XCD works on a contiguous run of a class (see
// pair8_decode), which pads each class to a multiple of eight workgroup numbers.
__host__ __device__ inline int pair8_cut_grid(const Pair8Cut& c, int xcd_remap)
{
  if (!xcd_remap) return pair8_cut_wgs(c);
  return 8 * ((c.tiles_a * c.chunks_a + 7) / 8 + (c.tiles_b * c.chunks_b + 7) / 8);
}

struct Pair8Wg {
  int tile;          // in the numbering of pair8_tiles_per_chunk
  int tx, ty;        // tile column and tile row
  bool folded;       // two row bands (rows of ty and of ty + 1) in the last tile column
  int z0, z1;        // planes [z0, z1) of the window [m_lo, m_hi)
};

// Workgroup number -> tile and planes; false for the padding numbers of an XCD's run.
// Order.  Class A first, then class B; inside a class chunk-major (all tiles of the class at their first chunk, then the second
// ...), tiles x first: workgroups that run together march the same planes of neighbouring tiles, so the rows of a plane are swept
// across all memory channels and the halo rows and columns a tile fetches are its neighbours' core data of the same moment.
// With xcd_remap, workgroup i runs on XCD i % 8: XCD x gets the x-th eighth of class A (a contiguous run, ceil(nA / 8) numbers) and
// then the x-th eighth of class B -- its share of a round of whole columns first, as before its share of a round of chunks.
// `more`: planes a chunk marches beyond its own (timing builds of the lab only).
__host__ __device__ inline bool pair8_decode(int wg, const Pair8Cut& c, int ntx, int nty, bool fold, int xcd_remap, int m_lo,
                                             int m_hi, int more, Pair8Wg& w)
{
  const int n_a = c.tiles_a * c.chunks_a, n_b = c.tiles_b * c.chunks_b;
  bool in_a;
  int item;
  if (xcd_remap) {
    const int per_a = (n_a + 7) / 8, per_b = (n_b + 7) / 8;
    const int xcd = wg % 8, s = wg / 8;
    in_a = s < per_a;
    item = in_a ? xcd * per_a + s : xcd * per_b + (s - per_a);
  } else {
    in_a = wg < n_a;
    item = in_a ? wg : wg - n_a;
  }
  if (item >= (in_a ? n_a : n_b)) return false;
  const int tiles = in_a ? c.tiles_a : c.tiles_b, zc = in_a ? c.zc_a : c.zc_b;
  const int chunk = item / tiles;
  w.tile = item % tiles + (in_a ? 0 : c.tiles_a);
  w.z0 = m_lo + chunk * zc;
  w.z1 = w.z0 + zc + more < m_hi ? w.z0 + zc + more : m_hi;
  if (fold) {
    const int pair = w.tile / (2 * ntx - 1), k = w.tile % (2 * ntx - 1);
    w.folded = k == ntx - 1;
    w.tx = k < ntx ? k : k - ntx;
    w.ty = k < ntx ? 2 * pair : 2 * pair + 1;
  } else {
    w.folded = false;
    w.tx = w.tile % ntx;
    w.ty = w.tile / ntx;
  }
  return true;
}

// One workgroup per CU at a time: the round model of k_sweep7 -- a chunk costs its planes plus ~7 steps of prologue and repeated
// stage-1 planes, `per_round` workgroups (256: one per CU) run per round.  `cost` is in plane steps of ONE workgroup; a step of a
// 16-wave workgroup (TY = 12) takes ~1.28 x a step of a 12-wave one (TY = 8) -- measured at 128^3 ... 512^3 (tools/kbench.py with
// F3D_PAIR8_TY): 12 rows win where the rows divide well (384^3: -9.5 %, 512^3: -4 %), 8 rows where one round of workgroups covers the
// level (256^3: +6 %, 128^3: +6 %) -- so the caller compares cost x step.
//
// Two classes (levels with more tiles than a round holds).  A uniform cut of such a level chunks EVERY tile so that the tiles beyond
// the last full round fill a round of their own: 512^3 is 344 tiles x 5 chunks of 103 planes, five cold starts per tile column for the
// sake of 88 tiles.  Instead the first tiles_a tiles -- whole rounds of them -- march (nearly) their whole column in lock-step and
// only the remainder is cut, as finely as fills the machine: cost = rounds(A) x (zc_a + extra) + rounds(B) x (zc_b + extra).
struct Pair8Plan {
  int zchunk;      // chunk length of the uniform plan (tiles_a == 0: == cut.zc_b)
  long cost;
  long wgs = 0;
  Pair8Cut cut = {};
};
inline Pair8Cut pair8_uniform_cut(int tiles, int planes, int zchunk)
{
  return Pair8Cut{0, 0, 0, tiles, (planes + zchunk - 1) / zchunk, zchunk};
}
// F3D_PAIR8_ROUND=<n> overrides the workgroups per round (the tests reach both classes on tiny shapes with it); read per call
inline long pair8_per_round(long standard)
{
  const char* e = std::getenv("F3D_PAIR8_ROUND");
  const long v = e ? std::atol(e) : 0;
  return v > 0 ? v : standard;
}
// `rows` / `planes`: extent along the tile rows and along the march (H and the z window; D and H for a y march)
// `fold`: the last tile column holds two row bands per tile (pair8_folds; never for a y march)
// `two_class`: false keeps the uniform plan (the y-marching builds); F3D_PAIR8_PLAN=0 does so everywhere (A/B timing, tests; read per call)
inline Pair8Plan pair8_plan_dims(int width, int rows, int planes, int ty, int zc_limit, long per_round = 256, bool fold = false,
                                 bool two_class = true)
{
  const long tiles = pair8_tiles_per_chunk((width + kPair8Lanes - 1) / kPair8Lanes, (rows + ty - 1) / ty, fold);
  const int max_chunks = planes > 0 ? planes : 1;  // down to one plane per chunk: three steps instead of four where one round covers it
  // what a chunk costs beside its planes, in plane steps (F3D_PAIR8_CHUNK_STEPS: launch-geometry experiments)
  static const int extra = std::getenv("F3D_PAIR8_CHUNK_STEPS") ? std::atoi(std::getenv("F3D_PAIR8_CHUNK_STEPS")) : 7;
  auto rounds = [&](long wgs) { return (wgs + per_round - 1) / per_round; };
  Pair8Plan p = {std::min(planes, zc_limit), -1};
  for (int nzc = 1; nzc <= max_chunks; ++nzc) {
    const int zc = (planes + nzc - 1) / nzc;
    if (zc > zc_limit) continue;
    const long wgs = tiles * ((planes + zc - 1) / zc);
    const long cost = rounds(wgs) * (zc + extra);
    if (p.cost < 0 || cost < p.cost) {
      p.cost = cost;
      p.zchunk = zc;
      p.wgs = wgs;
    }
  }
  if (p.cost < 0) {
    p.cost = static_cast<long>(rounds(tiles)) * (p.zchunk + extra);
    p.wgs = tiles;
  }
  if (p.zchunk < 1) p.zchunk = 1;
  p.cut = pair8_uniform_cut(static_cast<int>(tiles), planes, p.zchunk);
  const char* pe = std::getenv("F3D_PAIR8_PLAN");
  if (!two_class || (pe && pe[0] == '0') || tiles <= per_round || planes < 1 || zc_limit < 1) return p;
  // class A: whole rounds of tiles (A x a a multiple of per_round) in as few chunks as the chunk limit allows, or one or two more;
  // class B: the other tiles in 1 .. planes chunks.  A strictly cheaper cut wins; on a tie the uniform plan stays.
  const int a0 = (planes + zc_limit - 1) / zc_limit;
  int zc_a_seen = 0;
  for (int na = a0; na <= a0 + 2 && na <= planes; ++na) {
    const int zc_a = (planes + na - 1) / na;
    if (zc_a > zc_limit || zc_a == zc_a_seen) continue;
    zc_a_seen = zc_a;
    const int a = (planes + zc_a - 1) / zc_a;
    long g = a, r = per_round;
    while (r) { const long t = g % r; g = r; r = t; }   // g = gcd(a, per_round)
    const long stride = per_round / g;
    for (long A = stride; A < tiles; A += stride) {
      const long cost_a = rounds(A * a) * (zc_a + extra);
      if (cost_a >= p.cost) break;
      int zc_b_seen = 0;
      for (int nb = 1; nb <= planes; ++nb) {
        const int zc_b = (planes + nb - 1) / nb;
        if (zc_b > zc_limit || zc_b == zc_b_seen) continue;
        zc_b_seen = zc_b;
        const int b = (planes + zc_b - 1) / zc_b;
        const long cost = cost_a + rounds((tiles - A) * b) * (zc_b + extra);
        if (cost < p.cost) {
          p.cost = cost;
          p.wgs = A * a + (tiles - A) * b;
          p.cut = Pair8Cut{static_cast<int>(A), a, zc_a, static_cast<int>(tiles - A), b, zc_b};
        }
      }
    }
  }
  return p;
}

#ifdef F3D_PAIR8_PLAN_OWN_QUALIFIERS
#undef __host__
#undef __device__
#undef F3D_PAIR8_PLAN_OWN_QUALIFIERS
#endif
