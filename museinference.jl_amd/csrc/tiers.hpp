// tiers.hpp -- the tiers of a model family and the ONE rule that gives a launch its tier (muse_kernels.hip: for_family, launch_solver,
// loop_dispatch, launch_loglike).  Plain C++ without a HIP type: tests/native/tiers_driver.cpp compiles the lists and the rule as
// they stand, over stand-in types that carry MAXB alone.
#pragma once
#include "../../include/muse_hip.h"

namespace muse {

constexpr int kMaxTheta = MUSE_MAX_THETA;
constexpr int kBigTheta = MUSE_MAX_THETA_EXT;  // ntheta in (kMaxTheta, kBigTheta]: the "big" tier (args.hpp, BigTheta)

// A family's tiers in rising order of MAXB, the components one instantiation holds; at most the last one is big (MAXB > kMaxTheta).
template <class... Ms>
struct Tiers {};
template <class M>
struct ModelTag { using type = M; };
template <template <int> class M>
using FunnelTiers = Tiers<M<1>, M<2>, M<4>, M<kMaxTheta>, M<kBigTheta>>;   // the built-in funnel
template <template <int> class M>
using StencilTiers = Tiers<M<2>, M<4>, M<kMaxTheta>, M<kBigTheta>>;        // every stencil variant, a response header
template <template <int> class M>
using ElementwiseTiers = Tiers<M<1>, M<kMaxTheta>, M<kBigTheta>>;          // a user's elementwise header
template <template <int> class M>
using PairTiers = Tiers<M<2>, M<4>, M<kMaxTheta>>;                         // the two-parameter family: no big tier

// The rule.  `big` (muse_engine.cpp, tier_big: ntheta > kMaxTheta, or 2 .. kMaxTheta components in a streaming placement): the big
// tier.  Otherwise the first small tier that holds ntheta components -- TIER_WIDEST: the last small tier alone, for the
// per-simulation operators, which have one kernel for all small tiers.  f(ModelTag<M>) is called for the tier picked, `refused`
// returned where the family has none.  The policy is a template parameter and a tier it rules out is never named: a generic f that
// launches a kernel instantiates that kernel for every tier f is COMPILED for, taken or not.
enum TierPolicy { TIER_FIRST_FIT, TIER_WIDEST };
template <TierPolicy P, class R, class F>
R pick_tier(Tiers<>, int, bool, R refused, F&&) { return refused; }
template <TierPolicy P, class R, class F, class M, class... Rest>
R pick_tier(Tiers<M, Rest...>, int ntheta, bool big, R refused, F&& f) {
    constexpr bool kBig = M::MAXB > kMaxTheta;
    constexpr bool kLastSmall = !kBig && (... && (Rest::MAXB > kMaxTheta));
    if constexpr (kBig || kLastSmall || P == TIER_FIRST_FIT)
        if (big == kBig && ntheta <= M::MAXB) return f(ModelTag<M>{});
    return pick_tier<P>(Tiers<Rest...>{}, ntheta, big, refused, f);
}

}  // namespace muse
