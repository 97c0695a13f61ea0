// mp_normal_pair.h — the one Box-Muller step of the device code: two standard normals from the four words of one Philox draw.
// Shared by the Gaussian and walk moves of the sampler (mp_normal.hip) and the proposal draws of the bridge-sampling evidence
// (mp_bridge.hip), so that both form their normals with the same separately rounded operations.  Device only: included from .hip
// sources, never from a header a host compiler reads.
#pragma once
#include "mp_math.hpp"

namespace mp {

// Box-Muller on the four words of one draw (the KDE move's formula): sqrt(-2 ln(1 - u_a)) cos, sin (2 pi u_b)
MP_DEV void normal_pair(const uint32_t (&s4)[4], double &n0, double &n1) {
    const double rad = sqrt(mul_rn(-2.0, log(sub_rn(1.0, u01(s4[0], s4[1])))));
    const double ang = mul_rn(6.283185307179586, u01(s4[2], s4[3]));
    n0 = mul_rn(rad, cos(ang));
    n1 = mul_rn(rad, sin(ang));
}

}  // namespace mp
