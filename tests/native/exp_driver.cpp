// muse_exp (museinference.jl_amd/csrc/step.hpp) on the CPU: reads arguments as 16 hex digits (the bits of a double), one per line,
// from stdin and prints the bits of muse_exp of each, one per line.  Compiled without floating-point contraction, as the
// library compiles step.hpp on both sides.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../museinference.jl_amd/csrc/step.hpp"

int main() {
    uint64_t u;
    while (scanf("%" SCNx64, &u) == 1) {
        double x, y;
        memcpy(&x, &u, 8);
        y = muse::muse_exp(x);
        memcpy(&u, &y, 8);
        printf("%016" PRIx64 "\n", u);
    }
    return 0;
}
