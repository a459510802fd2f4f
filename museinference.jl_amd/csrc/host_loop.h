// host_loop.h -- the host-driven muse! loop (src/muse.jl:159-232): ONE copy for muse_run (muse_engine.cpp) and for the
// host loop of muse_run_sharded (muse_comm.cpp).  Host code only, no HIP call in it: the caller supplies the map, the loop
// owns the StepParams set-up, the convergence test, the step (step.hpp), the records and the step's error messages
// (tests/native/host_loop_driver.cpp runs it on a CPU).
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "../../include/muse_hip.h"
#include "step.hpp"

extern "C" int muse_set_error(int code, const char* msg);   // muse_engine.cpp (the message of muse_last_error)

namespace muse {

inline void step_params(int ntheta, const muse_run_options* o, StepParams& sp) {
    memset(&sp, 0, sizeof sp);
    sp.ntheta = ntheta;
    sp.nsims = o->nsims;
    sp.prior_kind = o->prior_kind;
    sp.alpha = o->alpha;
    sp.theta_rtol = o->theta_rtol;
    for (int k = 0; k < ntheta; ++k) {
        sp.prior_mean[k] = o->prior_mean[k];
        sp.prior_sigma[k] = o->prior_sigma[k];
    }
}

// A step.hpp error code (from the host step, or from the loop kernel's status word) as return code + message; `who` is the
// entry point whose convergence test it was.
inline int step_error(int err, const char* who = "muse_run") {
    switch (err) {
        case STEP_SINGULAR_LIKE: return muse_set_error(MUSE_ERR_INVALID, "muse_run: singular H^-1_like (zero score variance)");
        case STEP_SINGULAR_POST: return muse_set_error(MUSE_ERR_INVALID, "muse_run: singular posterior Hessian");
        case STEP_DOMAIN:
            // sqrt of a negative argument is a DomainError in the reference (an H^-1_post' that is not negative definite)
            return muse_set_error(MUSE_ERR_INVALID, (std::string(who) + ": DomainError in the convergence test: dtheta' H^-1_post' dtheta > 0 "
                                                                        "(H^-1_post' is not negative definite)").c_str());
        default: return MUSE_OK;
    }
}

inline double steady_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The loop: launch, wait, step, launch again.  run_map(i, theta, z0_mode, g, info) runs iteration i's map at theta and fills
// g [nsims + 1][ntheta], the scores in the reference's order (the data element first), and the caller's `ninfo` info rows; what
// it returns other than MUSE_OK ends the loop and is returned unchanged.  info_out (may be NULL): [maxsteps][ninfo].
template <class RunMap>
int host_muse_loop(const char* who, int nt, const double* theta0, const muse_run_options* o, int64_t ninfo, RunMap&& run_map,
                   int32_t* niter_out, double* theta_out, double* hist_out, double* gsims_out, muse_info* info_out) {
    const int S = o->nsims;
    const int64_t H = MUSE_RUN_HIST(nt);
    StepParams sp;
    step_params(nt, o, sp);
    StepWork work;
    double theta[kMaxTheta], theta_next[kMaxTheta], mean[kMaxTheta], var[kMaxTheta];
    for (int k = 0; k < nt; ++k) theta[k] = theta0[k];
    std::vector<double> g((size_t)(S + 1) * nt);
    std::vector<muse_info> info((size_t)ninfo);
    int n = 0;
    for (int i = 1; i <= o->maxsteps; ++i) {
        const double t_start = steady_s();
        if (i > 2) {  // convergence on the last two records (src/muse.jl:163-166); a NaN compares false and the loop goes on
            const int cv = step_converged(nt, hist_out + (int64_t)(i - 2) * H, hist_out + (int64_t)(i - 3) * H, o->theta_rtol);
            if (cv < 0) return step_error(STEP_DOMAIN, who);
            if (cv > 0) break;
        }
        const int z0_mode = (i > 1 || o->z0_warm) ? MUSE_Z0_WARM : MUSE_Z0_ZERO;
        const int rc = run_map(i, (const double*)theta, z0_mode, g.data(), info.data());
        if (rc) return rc;
        double* h = hist_out + (int64_t)(i - 1) * H;
        double* gs = gsims_out + (int64_t)(i - 1) * S * nt;
        memcpy(gs, g.data() + nt, (size_t)S * nt * sizeof(double));
        if (info_out) memcpy(info_out + (int64_t)(i - 1) * ninfo, info.data(), (size_t)ninfo * sizeof(muse_info));
        for (int k = 0; k < nt; ++k) step_moments(k, nt, S, gs, mean[k], var[k]);
        const int err = step_record(sp, theta, g.data(), mean, var, h, theta_next, work);
        if (err != STEP_OK) return step_error(err, who);
        for (int k = 0; k < nt; ++k) theta[k] = theta_next[k];
        h[7 * nt + nt * nt] = steady_s() - t_start;
        n = i;
    }
    *niter_out = n;
    for (int k = 0; k < nt; ++k) theta_out[k] = theta[k];
    return MUSE_OK;
}

}  // namespace muse
