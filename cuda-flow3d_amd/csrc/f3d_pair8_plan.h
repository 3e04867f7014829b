// How a fused solver launch (k_pair8, f3d_solve_pair8.h) is cut into workgroups: the plan (host, pure arithmetic) and the decode of
// a workgroup number into its tile and its planes (host AND device: ONE function, pair8_decode, compiled into the kernel's prologue
// and into the host C API, host/host_capi.cpp: f3d_pair8_plan / f3d_pair8_decode -- so the tests walk the very decode the kernel runs
// without a GPU).  Nothing here touches a voxel: every plan gives the same bits (each plane of each tile is computed once, from
// inputs only), plans differ in time alone.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define F3D_PAIR8_PLAN_OWN_QUALIFIERS
#endif

constexpr int kPair8Lanes = 64;   // columns of a tile

// a value that is the same in every lane of a wave, as a value (device: held in a scalar register; host: itself)
#if defined(__HIP_DEVICE_COMPILE__)
#define PAIR8_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define PAIR8_UNIFORM(x) (x)
#endif

// The solver kernels address a z-chunk with unsigned 32-bit byte offsets from the lowest plane the chunk touches: its own planes and
// `reach` halo planes on either side (1 for one sweep or the weights, 2 for the two-stage launches, 3 for the three-stage ones) must
// span at most 2^32 bytes of one array.  Returns the planes a chunk may hold at most -- eight planes of slack below 2^32 wherever
// that leaves a plane; where it does not (planes above 2^32 / 9 bytes), 1 as long as one plane with its halo still fits -- or 0:
// no chunk fits, the launch must be refused.  The entries and their planners ask with the reach of the launch.
inline int solver_chunk_limit(unsigned long long plane_bytes, int reach)
{
  if (plane_bytes == 0 || plane_bytes > 0x100000000ull || reach < 0) return 0;
  const long long planes = static_cast<long long>(0xffffffffull / plane_bytes) - 8;
  if (planes >= 1) return planes > 0x3fffffff ? 0x3fffffff : static_cast<int>(planes);
  return (1ull + 2ull * static_cast<unsigned long long>(reach)) * plane_bytes <= 0x100000000ull ? 1 : 0;
}

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

// The cut of a launch: up to three classes of tiles, in the tile numbering above.  Class A -- tiles 0 .. tiles_a-1 -- is cut into chunks_a
// chunks of zc_a planes per tile, class B -- the next tiles_b tiles -- into chunks_b chunks of zc_b planes, class C -- the last tiles_c
// tiles -- into chunks_c chunks of zc_c planes.  An empty class has no tiles: the uniform cut is class B alone, the two-class cut A and B.
// Handed to the kernel by value.
struct Pair8Cut {
  int tiles_a, chunks_a, zc_a;
  int tiles_b, chunks_b, zc_b;
  int tiles_c, chunks_c, zc_c;
};
__host__ __device__ inline int pair8_cut_wgs(const Pair8Cut& c)
{
  return c.tiles_a * c.chunks_a + c.tiles_b * c.chunks_b + c.tiles_c * c.chunks_c;
}
// Workgroups are dealt to the eight XCDs round-robin; with `xcd_remap` every XCD works on a contiguous run of a class (see
// pair8_decode), which pads each class to a multiple of eight workgroup numbers.
__host__ __device__ inline int pair8_cut_grid(const Pair8Cut& c, int xcd_remap)
{
  if (!xcd_remap) return pair8_cut_wgs(c);
  return 8 * ((c.tiles_a * c.chunks_a + 7) / 8 + (c.tiles_b * c.chunks_b + 7) / 8 + (c.tiles_c * c.chunks_c + 7) / 8);
}

struct Pair8Wg {
  int tile;          // in the numbering of pair8_tiles_per_chunk
  int tx, ty;        // tile column and tile row
  bool folded;       // two row bands (rows of ty and of ty + 1) in the last tile column
  int z0, z1;        // planes [z0, z1) of the window [m_lo, m_hi)
};

// Workgroup number -> tile and planes; false for the padding numbers of an XCD's run.
// Order.  The classes in order (A, B, C); inside a class chunk-major (all tiles of the class at their first chunk, then the second
// ...), tiles x first: workgroups that run together march the same planes of neighbouring tiles, so the rows of a plane are swept
// across all memory channels and the halo rows and columns a tile fetches are its neighbours' core data of the same moment.
// With xcd_remap, workgroup i runs on XCD i % 8: XCD x gets the x-th eighth of class A (a contiguous run, ceil(nA / 8) numbers),
// then the x-th eighth of class B, then that of class C -- its share of each round of a class, the classes in the order they run.
// `more`: planes a chunk marches beyond its own (timing builds of the lab only).
__host__ __device__ inline bool pair8_decode(int wg, const Pair8Cut& c, int ntx, int nty, bool fold, int xcd_remap, int m_lo,
                                             int m_hi, int more, Pair8Wg& w)
{
  // (the nine numbers as values first: a choice among three fields of `c` by class number is otherwise compiled into an indexed read of
  // a copy of `c` in scratch memory, per lane)
  const int tiles_a = PAIR8_UNIFORM(c.tiles_a), tiles_b = PAIR8_UNIFORM(c.tiles_b), tiles_c = PAIR8_UNIFORM(c.tiles_c);
  const int zc_a = PAIR8_UNIFORM(c.zc_a), zc_b = PAIR8_UNIFORM(c.zc_b), zc_c = PAIR8_UNIFORM(c.zc_c);
  const int n_a = tiles_a * PAIR8_UNIFORM(c.chunks_a), n_b = tiles_b * PAIR8_UNIFORM(c.chunks_b), n_c = tiles_c * PAIR8_UNIFORM(c.chunks_c);
  int cls;    // 0, 1, 2 = A, B, C
  int item;   // chunk-major position inside the class
  if (xcd_remap) {
    const int per_a = (n_a + 7) / 8, per_b = (n_b + 7) / 8, per_c = (n_c + 7) / 8;
    const int xcd = wg % 8, s = wg / 8;
    cls = s < per_a ? 0 : (s < per_a + per_b ? 1 : 2);
    item = cls == 0 ? xcd * per_a + s : (cls == 1 ? xcd * per_b + (s - per_a) : xcd * per_c + (s - per_a - per_b));
  } else {
    cls = wg < n_a ? 0 : (wg < n_a + n_b ? 1 : 2);
    item = cls == 0 ? wg : (cls == 1 ? wg - n_a : wg - n_a - n_b);
  }
  if (item >= (cls == 0 ? n_a : (cls == 1 ? n_b : n_c))) return false;
  const int tiles = cls == 0 ? tiles_a : (cls == 1 ? tiles_b : tiles_c);
  const int zc = cls == 0 ? zc_a : (cls == 1 ? zc_b : zc_c);
  const int chunk = item / tiles;
  w.tile = item % tiles + (cls == 0 ? 0 : (cls == 1 ? tiles_a : tiles_a + tiles_b));
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

// ---- the x neighbours of a row wave's lanes, read from the ring (weights-first launch, tile with one band) ----
// A ring slot holds one plane: `ns` arrays of `nj` rows of 64 floats, behind them the 16-byte x-halo pieces [array][side][row] (side 0:
// columns x0-4 .. x0-1, side 1: x0+64 .. x0+67), rounded up to whole DMA instructions of 64 pieces.
__host__ __device__ constexpr int pair8_slot_halo_off(int ns, int nj) { return ns * nj * kPair8Lanes; }
__host__ __device__ constexpr int pair8_slot_floats(int ns, int nj)
{
  return pair8_slot_halo_off(ns, nj) + (ns * 2 * nj + kPair8Lanes - 1) / kPair8Lanes * 4 * kPair8Lanes;
}
// Lane -> the row elements that hold its left and its right neighbour; -1 is the last float of the left halo piece, 64 the first of
// the right one.  The reference's mirror rule (index -1 -> 1, W -> W-2) is part of the rule: at x = 0 the left neighbour IS the right
// one, at x = W-1 the right one is the left one -- in this order, so a volume one column wide names element 1 twice, as the selects
// that this replaces did.  Lanes beyond the volume (x >= W) name their geometric neighbours: nobody looks at what they read.
struct Pair8XNeighbours {
  int left, right;
};
__host__ __device__ inline Pair8XNeighbours pair8_x_neighbours(int lane, int x0, int width)
{
  const int x = x0 + lane;
  Pair8XNeighbours n = {lane - 1, lane + 1};
  if (x == 0) n.left = n.right;
  if (x == width - 1) n.right = n.left;
  return n;
}
// float offset inside a slot of element `elem` (-1 .. 64, as above) of ring row `row` of array `array`
__host__ __device__ inline int pair8_x_neighbour_offset(int elem, int array, int row, int ns, int nj)
{
  const int halo = pair8_slot_halo_off(ns, nj) + (array * 2 * nj + row) * 4;
  if (elem < 0) return halo + 3;
  if (elem >= kPair8Lanes) return halo + nj * 4;
  return (array * nj + row) * kPair8Lanes + elem;
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
  return Pair8Cut{0, 0, 0, tiles, (planes + zchunk - 1) / zchunk, zchunk, 0, 0, 0};
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
// what a chunk costs beside its planes, in plane steps (F3D_PAIR8_CHUNK_STEPS: launch-geometry experiments)
inline int pair8_chunk_steps()
{
  static const int extra = std::getenv("F3D_PAIR8_CHUNK_STEPS") ? std::atoi(std::getenv("F3D_PAIR8_CHUNK_STEPS")) : 7;
  return extra;
}
// `two_class`: false gives the uniform plan.  Reads no switch: the same arguments give the same plan.
inline Pair8Plan pair8_plan_two(int width, int rows, int planes, int ty, int zc_limit, long per_round, bool fold, bool two_class)
{
  const long tiles = pair8_tiles_per_chunk((width + kPair8Lanes - 1) / kPair8Lanes, (rows + ty - 1) / ty, fold);
  const int max_chunks = planes > 0 ? planes : 1;  // down to one plane per chunk: three steps instead of four where one round covers it
  const int extra = pair8_chunk_steps();
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
  if (!two_class || tiles <= per_round || planes < 1 || zc_limit < 1) return p;
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
          p.cut = Pair8Cut{static_cast<int>(A), a, zc_a, static_cast<int>(tiles - A), b, zc_b, 0, 0, 0};
        }
      }
    }
  }
  return p;
}

// `two_class`: false keeps the uniform plan (the y-marching builds); F3D_PAIR8_PLAN=0 does so everywhere (A/B timing, tests; read per call)
inline Pair8Plan pair8_plan_dims(int width, int rows, int planes, int ty, int zc_limit, long per_round = 256, bool fold = false,
                                 bool two_class = true)
{
  const char* pe = std::getenv("F3D_PAIR8_PLAN");
  return pair8_plan_two(width, rows, planes, ty, zc_limit, per_round, fold, two_class && !(pe && pe[0] == '0'));
}

// The wide plan: up to three classes, also on levels one round covers.  The two-class plan above leaves two kinds of waste in the
// round model.  A level of at most per_round tiles keeps one chunk length for every tile, although "most tiles in two chunks, the few
// left over cut finely" fills the rounds better (307^3: 130 tiles in 3 chunks of 103 planes are two rounds of 110 steps less a
// few; 128 tiles x 2 chunks of 154 planes are ONE full round of 161 steps and the two tiles left over one round of 10).  And what is
// left beside class A is itself a level with a remainder (512^3: 88 tiles left, of which 64 x 4 chunks fill a round exactly).
//   classes  up to three, in tile order; every class but the last fills whole rounds (tiles_i x chunks_i a multiple of per_round),
//            the last class is the cheapest uniform cut of the tiles left;
//   cost     sum over the classes of rounds(tiles_i x chunks_i) x (zc_i + extra);
//   leading  a leading class takes one of the 16 smallest chunk counts the chunk limit allows;
//   tie      taken only where strictly cheaper than pair8_plan_two's plan for the same arguments, which is returned otherwise --
//            among wide plans the first found stays (fewer classes first, then fewer chunks, then fewer tiles in the leading class).
// Pure arithmetic on its arguments: F3D_PAIR8_ROUND and F3D_PAIR8_PLAN are read by the callers, per call.
inline Pair8Plan pair8_plan_wide(int width, int rows, int planes, int ty, int zc_limit, long per_round = 256, bool fold = false)
{
  Pair8Plan best = pair8_plan_two(width, rows, planes, ty, zc_limit, per_round, fold, true);
  const int tiles = pair8_tiles_per_chunk((width + kPair8Lanes - 1) / kPair8Lanes, (rows + ty - 1) / ty, fold);
  if (tiles < 2 || planes < 1 || zc_limit < 1 || per_round < 1) return best;
  const int extra = pair8_chunk_steps();
  auto rounds = [&](long wgs) { return (wgs + per_round - 1) / per_round; };

  struct Class { int tiles, chunks, zc; };
  // the chunkings a leading class may take, and the tile counts that fill whole rounds with each (multiples of `stride`)
  struct Lead { int chunks, zc; long stride; };
  Lead leads[16];
  int n_leads = 0;
  const int a0 = (planes + zc_limit - 1) / zc_limit;
  for (int na = a0, seen = 0; na < a0 + 16 && na <= planes; ++na) {
    const int zc = (planes + na - 1) / na;
    if (zc > zc_limit || zc == seen) continue;
    seen = zc;
    const int a = (planes + zc - 1) / zc;
    long g = a, r = per_round;
    while (r) { const long t = g % r; g = r; r = t; }   // g = gcd(a, per_round)
    leads[n_leads++] = Lead{a, zc, per_round / g};
  }
  // the cheapest uniform cut of n tiles (the first cheapest of 1 .. planes chunks, as in the uniform plan), and the cheapest cut of n
  // tiles into a leading class and that; both remembered per n -- the tile counts left over are few (tiles minus multiples of a stride)
  struct Tail { long cost = -1; Class lead = {0, 0, 0}, last = {0, 0, 0}; };
  std::vector<Tail> one(tiles + 1), two(tiles + 1);
  auto uniform = [&](int n) -> const Tail& {
    Tail& t = one[n];
    if (t.cost >= 0) return t;
    for (int nzc = 1, seen = 0; nzc <= planes; ++nzc) {
      const int zc = (planes + nzc - 1) / nzc;
      if (zc > zc_limit || zc == seen) continue;
      seen = zc;
      const int b = (planes + zc - 1) / zc;
      const long cost = rounds(static_cast<long>(n) * b) * (zc + extra);
      if (t.cost < 0 || cost < t.cost) {
        t.cost = cost;
        t.last = Class{n, b, zc};
      }
    }
    return t;
  };
  auto lead_and_uniform = [&](int n) -> const Tail& {
    Tail& t = two[n];
    if (t.cost >= 0) return t;
    t = uniform(n);
    for (int i = 0; i < n_leads; ++i) {
      for (long A = leads[i].stride; A < n; A += leads[i].stride) {
        const long cost_a = rounds(A * leads[i].chunks) * (leads[i].zc + extra);
        if (cost_a >= t.cost) break;
        const Tail& rest = uniform(n - static_cast<int>(A));
        if (cost_a + rest.cost < t.cost) {
          t.cost = cost_a + rest.cost;
          t.lead = Class{static_cast<int>(A), leads[i].chunks, leads[i].zc};
          t.last = rest.last;
        }
      }
    }
    return t;
  };
  auto take = [&](long cost, const Class& a, const Class& b, const Class& c) {
    best.cost = cost;
    best.cut = Pair8Cut{a.tiles, a.chunks, a.zc, b.tiles, b.chunks, b.zc, c.tiles, c.chunks, c.zc};
    best.wgs = pair8_cut_wgs(best.cut);
  };
  {   // one or two classes
    const Tail& t = lead_and_uniform(tiles);
    if (t.cost < best.cost) take(t.cost, t.lead, t.last, Class{0, 0, 0});
  }
  for (int i = 0; i < n_leads; ++i) {   // three
    for (long A = leads[i].stride; A < tiles; A += leads[i].stride) {
      const long cost_a = rounds(A * leads[i].chunks) * (leads[i].zc + extra);
      if (cost_a >= best.cost) break;
      const Tail& rest = lead_and_uniform(tiles - static_cast<int>(A));
      if (rest.lead.tiles && cost_a + rest.cost < best.cost)
        take(cost_a + rest.cost, Class{static_cast<int>(A), leads[i].chunks, leads[i].zc}, rest.lead, rest.last);
    }
  }
  return best;
}

// The plan a z-marching product launch takes: F3D_PAIR8_PLAN (read per call) unset or 2 = the wide plan, 1 = the two-class plan,
// 0 = the uniform plan.
inline Pair8Plan pair8_plan_launch(int width, int rows, int planes, int ty, int zc_limit, long per_round = 256, bool fold = false)
{
  const char* pe = std::getenv("F3D_PAIR8_PLAN");
  if (pe && (pe[0] == '0' || pe[0] == '1')) return pair8_plan_two(width, rows, planes, ty, zc_limit, per_round, fold, pe[0] == '1');
  return pair8_plan_wide(width, rows, planes, ty, zc_limit, per_round, fold);
}

#ifdef F3D_PAIR8_PLAN_OWN_QUALIFIERS
#undef __host__
#undef __device__
#undef F3D_PAIR8_PLAN_OWN_QUALIFIERS
#endif
