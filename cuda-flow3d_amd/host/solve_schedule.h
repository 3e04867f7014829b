// Launch schedule of the solver: how the K inner sweeps of one outer iteration are cut into launches, and which launch also
// writes the weights (phi / ksi) of the next outer iteration.  Pure host arithmetic (no device call, no environment read, no
// state), shared by the resident operator, the piecemeal operator, the z-slab driver and the CPU tests.  Which entry point a
// launch maps to, on which window it runs and what happens when a launch declines stays with each driver.
#ifndef F3D_HOST_SOLVE_SCHEDULE_H_
#define F3D_HOST_SOLVE_SCHEDULE_H_

#include <vector>

// The fused launches apply the face weights alpha / h^2 by selection, which equals the reference's (float)(flag) * w only for a
// finite w that is not negative (include/f3d.h).  False for a solve with other parameters -- the reference would propagate NaN
// or -0 --: such a solve takes the one-sweep launches, whose kernels multiply as the reference does.  Every solve asks once and
// hands `fused = FusedSweepsEnabled() && SolveWeightsPlain(...)` to whatever cuts or chooses its launches.
bool SolveWeightsPlain(float equation_alpha, float hx, float hy, float hz);

struct SweepLaunch {
  int first;          // index of the launch's first sweep within the outer iteration
  int sweeps;         // 1, 2 or 3 sweeps in this launch
  bool next_weights;  // the launch also computes the phi / ksi of the NEXT outer iteration (into the second weight pair)
  bool weights_first = false;  // the launch computes the phi / ksi of THIS outer iteration in front of its sweep (CutSweepsWeightsFirst)
};

// The K sweeps of ONE outer iteration (the same bit pattern whichever way they are cut), one buffer swap per launch:
//   !fused  one sweep per launch, none takes the weights along;
//   fused   two sweeps per launch and a single one for an odd K; with `tri` (the three-stage launches, small and mid-size levels
//           of the resident operator) three per launch, then two, then one.
// `carry` = another outer iteration follows AND the driver can take its weights along (a second weight pair is there, the switches
// allow it).  Then the last launch carries them when it is a single sweep -- without `tri` only an odd K ends that way -- or, with
// `tri`, two sweeps: the tail is arranged to end in (S, S, P), so 3 remaining are cut 1 + 2 and 4 remaining 2 + 2, and the default
// five sweeps are (S, S, S) + (S, S, P).  Whether an outer iteration hands the weights over is therefore a property of K, fused and
// tri alone: a level of `outer` iterations makes outer - 1 hand-overs when CutSweeps(K, fused, tri, true) ends in a launch that
// carries, and none otherwise.
std::vector<SweepLaunch> CutSweeps(int K, bool fused, bool tri, bool carry);

// The same K sweeps cut the other way, for a driver that has the weights-first launch: the first launch of EVERY outer iteration is
// (P, S) -- the phi / ksi of this iteration and its first sweep --, then two sweeps per launch, then a single one for an even K.  No
// launch takes the next weights along (they are made where they are used, into the caller's pair: no second pair, no swap parity), so
// the cut is the same whether or not another outer iteration follows.  K < 1: empty.
std::vector<SweepLaunch> CutSweepsWeightsFirst(int K);

#endif
