// muse::model_exp (museinference.jl_amd/csrc/model_math.hpp: the per-element exponential of device code) on the CPU, beside
// muse::muse_exp (step.hpp): reads arguments as 16 hex digits (the bits of a double), one per line, from stdin and prints
// "<bits of muse_exp> <bits of model_exp>" per line.  On the host the reciprocal's seed is what -DSEED_BITS=n leaves of 1/d (the top
// n bits of its significand, rounded down or -- SEED_UP -- up by one unit of that precision): the refinement has to turn every
// such seed into the correctly rounded quotient.  "-q" instead checks the division alone: lines "<bits n> <bits d>", output the
// bits of n / d and of model_div_unscaled(n, d).  Compiled without floating-point contraction, as the library compiles both files.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#ifndef SEED_BITS
#define SEED_BITS 20
#endif
static inline double coarse_rcp(double d) {
    double y = 1.0 / d;
    uint64_t u;
    memcpy(&u, &y, 8);
    u &= ~((UINT64_C(1) << (52 - SEED_BITS)) - 1);
#ifdef SEED_UP
    u += UINT64_C(1) << (52 - SEED_BITS);
#endif
    memcpy(&y, &u, 8);
    return y;
}
#define MUSE_MM_RCP_SEED(d) coarse_rcp(d)

#include "../../museinference.jl_amd/csrc/step.hpp"
#include "../../museinference.jl_amd/csrc/model_math.hpp"

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

int main(int argc, char** argv) {
    uint64_t u, w;
    if (argc > 1 && strcmp(argv[1], "-q") == 0) {
        while (scanf("%" SCNx64 " %" SCNx64, &u, &w) == 2) {
            double n, d;
            memcpy(&n, &u, 8);
            memcpy(&d, &w, 8);
            printf("%016" PRIx64 " %016" PRIx64 "\n", bits(n / d), bits(muse::model_div_unscaled(n, d)));
        }
        return 0;
    }
    while (scanf("%" SCNx64, &u) == 1) {
        double x;
        memcpy(&x, &u, 8);
        printf("%016" PRIx64 " %016" PRIx64 "\n", bits(muse::muse_exp(x)), bits(muse::model_exp(x)));
    }
    return 0;
}
