// osot_qp_tol.h -- the tolerances of the dual active-set rule, once, for every solver that promises that rule: the wavefront core
// (osot_qp_core.h), the workgroup solver for 65 .. 128 variables (osot_qp_big.h) and the wide cascade built on it
// (osot_cascade_wide.h).  Plain C++ (no HIP): osot_qp_big.h is also compiled by the host compiler for tests/emu.
// OSOT_RATIO_TOL and OSOT_REFINE_FLOOR are build-variant knobs (tools/build_variant.sh); a build that overrides one moves BOTH
// solvers -- on purpose: the wide cascade's rule is the wavefront cascade's rule, whatever a variant makes of it.
// (The oracle keeps tolerances of its own: an independent checker does not share a header with what it checks.)
#pragma once

namespace osot {

constexpr double kInfty = 1.0e20;      // QPOasesBackEnd::checkINFTY clamp (QPOasesBackEnd.cpp:339-356)
constexpr double kDepTol2 = 1.0e-24;   // |d2|^2 <= kDepTol2 |d|^2  -> normal is in the span of the working set.
                                       // |d|^2 is dominated by the 1/eps-scaled directions (6e10 at the default eps), the
                                       // round-off floor of |d2|^2 is ~1e-29 |d|^2, and a genuine last free direction was seen
                                       // at 6e-19 |d|^2 (tests/stress_parity.py): 1e-18 called it dependent -> false INFEASIBLE
constexpr double kDepFloor2 = 1.0e-13; // second test, only when |d2|^2 <= 1e-12 |d|^2: max over the free columns c of J of
                                       // d2_c^2 / (|J_c|^2 |n|^2) <= kDepFloor2 -> dependent (see direction_is_independent).
                                       // That ratio is the cos^2 of the angle between the normal and the column: about the
                                       // sine^2 of its angle with the span of the working set.  A row at 1e-8 .. 1e-12 of that span is a direction on paper, but
                                       // taking it puts |d2| on the diagonal of R (condition 1e8+: the dual directions r lose
                                       // their signs) and moves x by violation / |d2|.  Seen on hardware (closed-loop
                                       // self-collision tests, H ~ I): sine^2 = 3e-23 with a bound violated by 4e-11 -> x jumped
                                       // by 26; sine^2 = 1.5e-17 with 1e-7 -> by 14; both ended as false INFEASIBLE.  The genuine
                                       // last direction quoted above sits at 9.4e-9 on this scale.  tests/stress_closed_loop.py:
                                       // 5.3 M closed-loop solves at eps factor 1e6 without an unsolved instance (346 in
                                       // 921 k with a floor of 1e-19); at the default eps 5 distinct instances in 3 x 307 k
constexpr double kViolTol = 1.0e-11;   // a slack below -kViolTol*max(1,|bound|) counts as violated
constexpr double kEqTol = 1.0e-9;      // consistency of a linearly dependent equality row
constexpr double kSlackTol = 1.0e-6;   // a violation below this (relative) with no direction left is round-off: with the
                                       // default eps (4.4e-11) an upper level's x carries O(1e-16 / eps) = 1e-6 of noise and
                                       // its active bound re-appears violated by that much where no freedom is left
                                       // (found by tests/stress_parity.py; qpOASES accepts the same point)
constexpr double kSlackCap = 1.0e-5;   // ... but never more than this in absolute terms (torque / acceleration limits of 1e2 .. 1e3)

#ifndef OSOT_RATIO_TOL
#define OSOT_RATIO_TOL 1.0e-14
#endif
constexpr double kRatioTol = OSOT_RATIO_TOL;  // (1e-10 cost a genuine trade at the default eps, where the entries of r span ten decades; the noise seen was < 1e-15)  // dual ratio test: r_k counts as positive only above this fraction of max |r| (see gi_inequalities)

#ifndef OSOT_REFINE_FLOOR
#define OSOT_REFINE_FLOOR 1.0e-9
#endif
constexpr double kRefineFloor = OSOT_REFINE_FLOOR;   // violations below this (relative to max(1, |bound|)) are accepted without a refinement
constexpr int kRefineMax = 2;             // refinements per level
constexpr double kSpanAccept = 1.0e-8;    // (see gi_inequalities: a violation below this with the normal in the span of the working set is not exchanged)

}  // namespace osot
