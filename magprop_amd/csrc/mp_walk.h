// mp_walk.h — what the walk kernels of the resident drivers share, device only: the stepping-out and shrinkage slice update
// (Neal 2003) as a state machine that names one point per round (slice_half_kernel of mp_slice.hip; nest_slice_kernel of
// mp_nest.hip states the same machine itself, measured 2.2 % faster that way: its file says so), and the DE step of a constrained
// random walk (nest_walk_kernel, smc_move_kernel of mp_smc.hip).  A caller keeps what is its own: where the partners and the
// scale come from, the Philox key, what "inside" means, how many slices a launch runs, and its counters of moves and
// evaluations.  Every product and sum is rounded on its own (mul_rn / add_rn / sub_rn), in the order the restatement of the
// tests states (tests/walk_restated.py: slice_rounds, de_step).
#pragma once
#include "mp_math.hpp"

namespace mp {

// One slice along dir through cur, between rounds (in LDS; only lane 0 reads or writes it).  phase: kSliceLeft / kSliceRight step
// out (budgets left / right), kSliceShrink draws shrink point i of [lo, hi], kSliceEnded: no slice is open (the zero state).
// The counts run on over the slices a caller opens on one state.
enum { kSliceEnded = 0, kSliceLeft = 1, kSliceRight = 2, kSliceShrink = 3 };
struct SliceCore {
    double lo, hi, t;   // the interval along dir; the parameter of the named point
    int phase, left, right, i, n_exp, n_con, n_fail;
};

// What a round of slice_step came to: a point to evaluate in prop, or the slice has ended, moved to prop or failed at the cap.
enum { kSliceNamed = 0, kSliceMoved = 1, kSliceFailed = 2 };

// Opens a slice of scale mu: the interval of length mu placed by u_lo, the max_steps_out - 1 steps out split by u_left.
MP_DEV void slice_open(SliceCore &z, double mu, double u_lo, double u_left, int max_steps_out) {
    z.lo = -mul_rn(mu, u_lo);
    z.hi = add_rn(z.lo, mu);
    z.left = (int)(u_left * (double)max_steps_out);
    z.right = max_steps_out - 1 - z.left;
    z.i = 0;
    z.phase = kSliceLeft;
}

// Lane 0, once per round of an open slice: takes the outcome of the point named last round (have: there is one; in: it was
// inside), then advances until it names the next point in the box (prop = cur + t dir; kSliceNamed) or the slice ends: a shrink
// point was inside (kSliceMoved, the point still in prop) or max_shrink of them were not (kSliceFailed: the slice fails where it
// starts).  shrink_u(i): the uniform of shrink point i; in_box(d, q): coordinate d of a point may be q.  A point outside the box
// is outside without an evaluation.
template <class Shrink, class Box>
MP_DEV int slice_step(SliceCore &z, double mu, int max_shrink, bool have, bool in, const double *cur, const double *dir, double *prop,
                      int nd, Shrink &&shrink_u, Box &&in_box) {
    for (;;) {
        if (have) {   // the named point's outcome (evaluated, or outside the box)
            have = false;
            if (z.phase == kSliceLeft) {
                if (in) { z.lo = sub_rn(z.lo, mu); --z.left; ++z.n_exp; } else z.phase = kSliceRight;
            } else if (z.phase == kSliceRight) {
                if (in) { z.hi = add_rn(z.hi, mu); --z.right; ++z.n_exp; } else z.phase = kSliceShrink;
            } else if (in) {
                z.phase = kSliceEnded;
                return kSliceMoved;
            } else {
                ++z.n_con;
                if (z.t < 0.0) z.lo = z.t;
                else z.hi = z.t;
            }
        }
        double t;
        if (z.phase == kSliceLeft) {
            if (z.left == 0) { z.phase = kSliceRight; continue; }
            t = z.lo;
        } else if (z.phase == kSliceRight) {
            if (z.right == 0) { z.phase = kSliceShrink; continue; }
            t = z.hi;
        } else {
            if (z.i == max_shrink) {   // the cap
                ++z.n_fail;
                z.phase = kSliceEnded;
                return kSliceFailed;
            }
            t = add_rn(z.lo, mul_rn(shrink_u(z.i), sub_rn(z.hi, z.lo)));
            ++z.i;
        }
        z.t = t;
        int box = 1;
        for (int d = 0; d < nd; ++d) {
            const double q = add_rn(cur[d], mul_rn(t, dir[d]));
            box &= in_box(d, q) ? 1 : 0;
            prop[d] = q;
        }
        if (box) return kSliceNamed;
        have = true;   // outside the box: outside, not evaluated
        in = false;
    }
}

// The DE step of a constrained walk: prop = cur + gamma (x1 - x2), gamma = g (1 + sig3 (2 u - 1)); returns whether prop lies in
// the box [lower, upper].
MP_DEV int de_walk_step(const double *cur, const double *x1, const double *x2, double g, double sig3, double u, const double *lower,
                        const double *upper, int nd, double *prop) {
    const double gamma = mul_rn(g, add_rn(1.0, mul_rn(sig3, sub_rn(mul_rn(2.0, u), 1.0))));
    int in = 1;
    for (int d = 0; d < nd; ++d) {
        const double q = add_rn(cur[d], mul_rn(gamma, sub_rn(x1[d], x2[d])));
        in &= (q >= lower[d] && q <= upper[d]) ? 1 : 0;
        prop[d] = q;
    }
    return in;
}

}  // namespace mp
