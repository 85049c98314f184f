// arith/arith_launch.hpp -- what arith.hip (the entry points) and the two builds of arith_kernels.hip (the kernels and their launch)
// share: the launch request and the two launchers.  Host side.
#pragma once

#include "../ctx.hpp"
#include "arith.hpp"

namespace mi355 {

struct ArithLaunch {
    ArithArgs k;
    LaunchEnv env;
};

// arith_exact_kernel<co> / arith_checked_kernel<co> on a persistent grid; co outside 1..32 -> hipErrorInvalidValue
hipError_t launch_arith_exact(unsigned co, const ArithLaunch &r);
hipError_t launch_arith_checked(unsigned co, const ArithLaunch &r);

} // namespace mi355
