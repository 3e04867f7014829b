/*
 * f3d_block_match.h -- the two device entries of the coarse block matching stage: the integer shift that maximises
 * the zero-normalised cross-correlation of a small window of frame 0 against frame 1 on a grid of nodes, and the expansion of node
 * vectors to a dense field.  Part of the C ABI of libf3d_hip.so; the conventions are those of f3d.h, which this header includes
 * (f3d.h does not include it: the entries move there when the tests that pin the declarations of f3d.h are next revised).
 */
#ifndef F3D_BLOCK_MATCH_H_
#define F3D_BLOCK_MATCH_H_

#include "f3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define F3D_BLOCK_MATCH_MAX_WINDOW 8   /* the largest half-window */
#define F3D_BLOCK_MATCH_MAX_REACH 16   /* the largest window + search radius */
#define F3D_BLOCK_MATCH_MAX_BINS 256
#define F3D_BLOCK_MATCH_MAX_NODES (1u << 22)

/* status of a node's record */
#define F3D_BLOCK_MATCH_OK 0
#define F3D_BLOCK_MATCH_FLAT 1 /* the window of a is constant (da == 0): nothing was searched */
#define F3D_BLOCK_MATCH_NONE 2 /* every candidate was outside the box or flat */

/* The node grid and the search.  Node (i, j, k), i fastest, lies at (ox + i step, oy + j step, oz + k step). */
typedef struct f3d_block_match_grid {
  int ox, oy, oz;
  int step;       /* >= 1 */
  int nx, ny, nz; /* >= 1, nx ny nz <= F3D_BLOCK_MATCH_MAX_NODES */
  int window;     /* half-window W, 1 .. 8: the window of a node is (2W+1)^3 voxels */
  int rx, ry, rz; /* search radii >= 0, window + max(r) <= 16 */
} f3d_block_match_grid;

/* The record of one node: 32 int32.  Codes: a voxel s of a or b has code bin_of(s) of the rule (lo, hi, bins) of f3d_histogram when
 * lo <= s <= hi, 0 below lo or NaN, bins - 1 above hi.  With p the window voxels, n = (2W+1)^3:
 *   sa = sum a_p, saa = sum a_p^2;  for a shift d: sb = sum b_{p+d}, sbb = sum b_{p+d}^2, sab = sum a_p b_{p+d}
 *   num = n sab - sa sb, da = n saa - sa^2, db = n sbb - sb^2   (int64)
 * Candidates are centre + (dx, dy, dz), |dx| <= rx ..., index ((dz + rz) (2 ry + 1) + (dy + ry)) (2 rx + 1) + (dx + rx).  One whose
 * window leaves the box counts in `outside`; of the others one with db == 0 counts in `flat`; the rest count in `evaluated` and have
 * the score (double)num * fabs((double)num) / (double)db, each operation rounded on its own.  The best is the largest score, the
 * smallest index among equals.  neighbour[f] holds sb, sbb, sab at best - x, + x, - y, + y, - z, + z; bit f of `valid` says that this
 * shift lies in the search range, its window inside the box and db != 0 (the three words are 0 otherwise).
 * status FLAT (da == 0): nothing is searched, all but sa, saa, nan is 0.  status NONE: all but sa, saa, nan and the counts is 0. */
typedef struct f3d_block_match_record {
  int shift[3];         /* the best shift, the centre included */
  int status;
  int evaluated, outside, flat;
  int sa, saa;
  int best[3];          /* sb, sbb, sab at the best shift */
  int neighbour[6][3];
  int valid;
  int nan;              /* the NaN voxels of a in this node's window */
} f3d_block_match_record;

typedef struct f3d_block_match_info {
  unsigned long long nodes, ok, flat_nodes, none_nodes; /* nodes = ok + flat_nodes + none_nodes */
  unsigned long long evaluated, outside, flat;          /* candidates, over all nodes */
  unsigned long long nan;                               /* NaN voxels of a, every window counted separately */
} f3d_block_match_info;

/* a, b: float32 containers of the current geometry holding frame 0 and frame 1 over the box width x height x depth.  centre
 * (nullable: all zero): nx ny nz int32 triples in host memory, the middle of each node's search.  records: nx ny nz records in host
 * memory.  info: nullable.  Whole volume, library stream; the call waits for the stream.  Padding outside the box is never read.
 * The same arguments give the same bytes whatever the schedule.  Refused, with nothing written: a null a, b, grid or records; lo, hi,
 * bins that f3d_histogram refuses, bins below 2 or above 256; step, counts, window or radii out of range; a centre component beyond
 * +-(1 << 20); a node whose own window leaves the box; a zero dimension or a box beyond the container. */
int f3d_block_match(f3d_devptr a, f3d_devptr b, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                    const f3d_block_match_grid* grid, const int* centre, f3d_block_match_record* records,
                    f3d_block_match_info* info);

/* Node vectors to a dense field.  u, v, w: nx ny nz float32 each in host memory (node (i, j, k) at [(k ny + j) nx + i]); the entry
 * uploads them.  Per voxel (x, y, z) of the box and per axis, in float32 with every operation rounded on its own:
 *   t = ((float)x - (float)ox) / (float)step;  i = clamp((int)floorf(t), 0, nx - 2);  f = clamp(t - (float)i, 0, 1)
 * and the value is p + f * (q - p) along x between nodes i and i + 1, then along y, then along z.  An axis with one node is constant
 * (no interpolation is done along it).  Outside the hull of the nodes the field is held constant.  A NaN node gives NaN wherever it
 * takes part.  Padding outside the box is not written.  Library stream; the call waits for the stream (the node arrays may be reused
 * on return).  Refused: null arguments, out_* that share a container, step < 1, a count < 1, more than F3D_BLOCK_MATCH_MAX_NODES
 * nodes, an origin beyond +-(1 << 20), a zero dimension or a box beyond the container. */
int f3d_expand_nodes(const float* u, const float* v, const float* w, int ox, int oy, int oz, int step, int nx, int ny, int nz,
                     f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height, size_t depth);

#ifdef __cplusplus
}
#endif
#endif /* F3D_BLOCK_MATCH_H_ */
