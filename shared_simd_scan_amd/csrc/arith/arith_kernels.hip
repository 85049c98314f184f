// arith_kernels.hip -- the 32 output widths of ONE of the two kernels of arith/arith.hpp and their launch, compiled twice:
// -DMI355_ARITH_CHECKED=0 (arith_exact_kernel, launch_arith_exact) and =1 (arith_checked_kernel, launch_arith_checked), so the two
// halves of the device code build side by side.  The launch itself is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp), shared
// with semijoin/, lookup/ and compact/.
#include "../ctx.hpp"

#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "arith_launch.hpp"

#ifndef MI355_ARITH_CHECKED
#error "build with -DMI355_ARITH_CHECKED=0 or 1"
#endif

namespace mi355 {

namespace {

// all of a block's LDS is dynamic, sized to the two input widths: the waves' two images of each column
template <int CO> hipError_t launch_arith(const ArithLaunch &r)
{
    const uint64_t ntiles = rt_ntiles(r.k.n);
    const size_t lds = arith_block_lds(r.k.c1, r.k.c2);
    const int max_dyn = (int)arith_block_lds(32, 32);
#if MI355_ARITH_CHECKED
    launch_tier<arith_checked_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
#else
    launch_tier<arith_exact_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
#endif
    return hipGetLastError();
}

} // namespace

#if MI355_ARITH_CHECKED
hipError_t launch_arith_checked(unsigned co, const ArithLaunch &r)
#else
hipError_t launch_arith_exact(unsigned co, const ArithLaunch &r)
#endif
{
    return launch_by_width<1, 32>(co, r, [](auto w, const ArithLaunch &q) { return launch_arith<decltype(w)::value>(q); });
}

} // namespace mi355
