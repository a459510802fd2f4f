// tiers_driver.cpp -- csrc/tiers.hpp on the host: the families' tier lists and the tier rule as the library compiles them, over
// stand-in model types that carry MAXB alone.  Prints, for every family, policy, `big` off and on, the MAXB picked for every ntheta
// from 1 to kBigTheta ("-": refused); tests/test_dispatch_tiers.py holds the table this must equal.
//   g++ -std=c++17 -o tiers_driver tiers_driver.cpp && ./tiers_driver
#include <stdio.h>

#include "../../museinference.jl_amd/csrc/tiers.hpp"

using namespace muse;

template <int B>
struct Stand { static constexpr int MAXB = B; };
struct StandNoise { static constexpr int MAXB = 1; };   // (models.hpp, NoiseModel: one type, one component)

// How many tiers a generic visitor is COMPILED for under a policy: a tier the policy rules out must not be named, taken or not (a
// kernel launched from the visitor would be instantiated for it).  The static member exists once per body the compiler instantiated.
static int g_compiled[2];
template <class Tag, TierPolicy P>
struct Compiled { static inline const int reg = ++g_compiled[P]; };
template <TierPolicy P, class T>
static void table(const char* family, T tiers) {
    for (int big = 0; big <= 1; ++big) {
        printf("%s %s big=%d:", family, P == TIER_WIDEST ? "widest" : "first", big);
        for (int nt = 1; nt <= kBigTheta; ++nt) {
            const int picked = pick_tier<P>(tiers, nt, big != 0, -1, [](auto m) { return decltype(m)::type::MAXB; });
            if (picked < 0) printf(" -");
            else printf(" %d", picked);
        }
        printf("\n");
    }
}
template <TierPolicy P, class T>
static void name_tiers(T tiers) {
    (void)pick_tier<P>(tiers, 1, false, -1, [](auto m) { return Compiled<decltype(m), P>::reg & 0; });
}
template <class T>
static void family(const char* name, T tiers) {
    table<TIER_FIRST_FIT>(name, tiers);
    table<TIER_WIDEST>(name, tiers);
}

int main() {
    printf("kMaxTheta %d kBigTheta %d\n", kMaxTheta, kBigTheta);
    family("funnel", FunnelTiers<Stand>{});
    family("stencil", StencilTiers<Stand>{});
    family("elementwise", ElementwiseTiers<Stand>{});
    family("pair", PairTiers<Stand>{});
    family("noise", Tiers<StandNoise>{});
    name_tiers<TIER_FIRST_FIT>(FunnelTiers<Stand>{});   // (the funnel's five tiers: all of them under first-fit, <8> and <64> under widest)
    name_tiers<TIER_WIDEST>(FunnelTiers<Stand>{});
    printf("compiled funnel first %d widest %d\n", g_compiled[TIER_FIRST_FIT], g_compiled[TIER_WIDEST]);
    printf("tiers driver ok\n");
    return 0;
}
