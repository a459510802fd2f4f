// The host-driven muse! loop (museinference.jl_amd/csrc/host_loop.h: host_muse_loop, the one copy muse_run and
// muse_run_sharded share) on a CPU, with a synthetic map -- scores that are a fixed function of theta and the element's
// index.  Checked: the z0 mode the map is called with; where the loop stops (step_converged on the last two records,
// otherwise maxsteps); every record, score block, info row and the final theta against a replay that calls step_moments +
// step_record itself on the same scores, bit for bit; a map's return code comes back unchanged; zero score variance is the
// "singular" error; the DomainError message carries the caller's name.  Exit 0 = all of it holds.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../museinference.jl_amd/csrc/host_loop.h"

using namespace muse;

static std::string g_msg;
extern "C" int muse_set_error(int code, const char* msg) {
    g_msg = msg ? msg : "";
    return code;
}

static int bad = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond) && bad++ < 20) {                        \
            fprintf(stderr, "line %d: ", __LINE__);         \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

// element e (0: the data) of the synthetic problem at theta: the data pulls theta to `target`, the simulations scatter with
// a variance between one and two (whatever their number: +-1 in turn, and a little noise) around a mean that moves a little
// with theta -- so the step contracts and the loop converges
static double noise(int e, int k) {
    unsigned long long x = (unsigned long long)(e * 131 + k * 7919 + 12345) * 6364136223846793005ull + 1442695040888963407ull;
    x ^= x >> 29;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 32;
    return ((e & 1) ? 1.0 : -1.0) + 0.2 * (((double)(x >> 11) + 0.5) / 9007199254740992.0 - 0.5);
}
static void scores_at(int nt, int S, const double* theta, bool flat_sims, double* g) {
    for (int k = 0; k < nt; ++k) g[k] = -(theta[k] - (0.5 + 0.25 * k));
    for (int e = 1; e <= S; ++e)
        for (int k = 0; k < nt; ++k) g[(size_t)e * nt + k] = flat_sims ? 0.125 : noise(e, k) + 0.05 * theta[k];
}

struct Case {
    int nt, S, maxsteps, prior_kind, z0_warm;
    double rtol;
    int ninfo;
    int fail_at, fail_rc;   // the map returns fail_rc at iteration fail_at (0: never)
    bool flat_sims;
};

static int run_case(const Case& c, bool want_info, int* niter_seen = nullptr) {
    const int nt = c.nt, S = c.S;
    const int64_t H = MUSE_RUN_HIST(nt);
    muse_run_options o;
    memset(&o, 0, sizeof o);
    o.nsims = S;
    o.maxsteps = c.maxsteps;
    o.prior_kind = c.prior_kind;
    o.alpha = 0.7;
    o.theta_rtol = c.rtol;
    o.z0_warm = c.z0_warm;
    o.atol = 1e-2;
    double theta0[kMaxTheta];
    for (int k = 0; k < nt; ++k) {
        o.prior_mean[k] = 0.1 * k;
        o.prior_sigma[k] = 2.0 + k;
        theta0[k] = 3.0 - k;
    }
    std::vector<double> hist((size_t)c.maxsteps * H, -7.0), gsims((size_t)c.maxsteps * S * nt, -7.0);
    std::vector<muse_info> info((size_t)c.maxsteps * c.ninfo + 1);
    memset(info.data(), 0x5a, info.size() * sizeof(muse_info));
    std::vector<int> modes;
    std::vector<std::vector<double>> thetas;
    auto run_map = [&](int i, const double* theta, int z0_mode, double* g, muse_info* inf) {
        CHECK(i == (int)modes.size() + 1, "iteration %d after %d calls", i, (int)modes.size());
        modes.push_back(z0_mode);
        thetas.emplace_back(theta, theta + nt);
        if (c.fail_at == i) return c.fail_rc;
        scores_at(nt, S, theta, c.flat_sims, g);
        for (int r = 0; r < c.ninfo; ++r) memset(&inf[r], (i * 16 + r) & 0xff, sizeof(muse_info));
        return (int)MUSE_OK;
    };
    int32_t niter = -1;
    double theta_out[kMaxTheta];
    g_msg.clear();
    const int rc = host_muse_loop("driver_loop", nt, theta0, &o, c.ninfo, run_map, &niter, theta_out, hist.data(), gsims.data(),
                                  want_info ? info.data() : nullptr);
    // the z0 mode: zero(z) on the first iteration of a cold start, the resident MAPs otherwise
    for (size_t i = 0; i < modes.size(); ++i)
        CHECK(modes[i] == ((i > 0 || c.z0_warm) ? MUSE_Z0_WARM : MUSE_Z0_ZERO), "z0 mode %d at iteration %d", modes[i], (int)i + 1);
    if (c.fail_at) {
        CHECK(rc == c.fail_rc, "map error %d came back as %d", c.fail_rc, rc);
        CHECK((int)modes.size() == c.fail_at, "%d map calls before the error at %d", (int)modes.size(), c.fail_at);
        return rc;
    }
    if (c.flat_sims) return rc;
    CHECK(rc == MUSE_OK, "rc %d (%s)", rc, g_msg.c_str());
    if (rc != MUSE_OK) return rc;
    // the replay: the same scores through step_moments + step_record, stopping where step_converged says
    StepParams sp;
    memset(&sp, 0, sizeof sp);
    sp.ntheta = nt; sp.nsims = S; sp.prior_kind = c.prior_kind; sp.alpha = o.alpha; sp.theta_rtol = o.theta_rtol;
    for (int k = 0; k < nt; ++k) { sp.prior_mean[k] = o.prior_mean[k]; sp.prior_sigma[k] = o.prior_sigma[k]; }
    StepWork w;
    std::vector<double> g((size_t)(S + 1) * nt), rec((size_t)c.maxsteps * H, 0.0);
    double theta[kMaxTheta], next[kMaxTheta], mean[kMaxTheta], var[kMaxTheta];
    memcpy(theta, theta0, sizeof(double) * nt);
    int n = 0;
    for (int i = 1; i <= c.maxsteps; ++i) {
        if (i > 2 && step_converged(nt, &rec[(size_t)(i - 2) * H], &rec[(size_t)(i - 3) * H], o.theta_rtol) > 0) break;
        CHECK(i <= niter, "the loop stopped after %d iterations, the replay goes on", niter);
        if (i > niter) break;
        CHECK(memcmp(thetas[i - 1].data(), theta, sizeof(double) * nt) == 0, "theta handed to the map at iteration %d", i);
        scores_at(nt, S, theta, false, g.data());
        const double* gs = g.data() + nt;
        for (int k = 0; k < nt; ++k) step_moments(k, nt, S, gs, mean[k], var[k]);
        double* h = &rec[(size_t)(i - 1) * H];
        const int err = step_record(sp, theta, g.data(), mean, var, h, next, w);
        CHECK(err == STEP_OK, "replay: step error %d", err);
        CHECK(memcmp(h, &hist[(size_t)(i - 1) * H], (size_t)(H - 1) * sizeof(double)) == 0, "record %d differs", i);
        const double t = hist[(size_t)(i - 1) * H + (H - 1)];
        CHECK(t >= 0.0 && t < 60.0, "record %d: time field %g", i, t);
        CHECK(memcmp(gs, &gsims[(size_t)(i - 1) * S * nt], (size_t)S * nt * sizeof(double)) == 0, "simulation scores of iteration %d", i);
        if (want_info)
            for (int r = 0; r < c.ninfo; ++r) {
                muse_info expect;
                memset(&expect, (i * 16 + r) & 0xff, sizeof expect);
                CHECK(memcmp(&expect, &info[(size_t)(i - 1) * c.ninfo + r], sizeof expect) == 0, "info row %d of iteration %d", r, i);
            }
        memcpy(theta, next, sizeof(double) * nt);
        n = i;
    }
    CHECK(n == niter, "niter %d, replay %d", niter, n);
    CHECK((int)modes.size() == niter, "%d map calls for %d iterations", (int)modes.size(), niter);
    CHECK(memcmp(theta, theta_out, sizeof(double) * nt) == 0, "theta_out");
    if (niter < c.maxsteps) CHECK(hist[(size_t)niter * H] == -7.0 && gsims[(size_t)niter * S * nt] == -7.0, "wrote behind the last iteration");
    {   // nothing written behind the info rows of the iterations that ran
        const unsigned char* p = (const unsigned char*)&info[want_info ? (size_t)niter * c.ninfo : 0];
        CHECK(p[0] == 0x5a && p[sizeof(muse_info) - 1] == 0x5a, "wrote behind the info rows");
    }
    if (niter_seen) *niter_seen = niter;
    return rc;
}

int main() {
    int cases = 0, converged = 0, ran_out = 0;
    for (int nt = 1; nt <= kMaxTheta; ++nt)
        for (int S : {2, 5, 64, 100, 257})
            for (int prior = 0; prior <= 1; ++prior)
                for (int warm = 0; warm <= 1; ++warm)
                    for (double rtol : {1e-3, 0.0, 0.2}) {
                        const int maxsteps = rtol == 0.0 ? 12 : 40;
                        int n = 0;
                        run_case({nt, S, maxsteps, prior, warm, rtol, (S % 3) + (warm ? S : 0), 0, 0, false}, (S + nt) % 2 == 0 || warm, &n);
                        cases += 1;
                        converged += n >= 3 && n < maxsteps;
                        ran_out += n == maxsteps;
                        if (rtol == 0.0) CHECK(n == maxsteps, "theta_rtol 0 stopped after %d of %d", n, maxsteps);
                    }
    // (theta_rtol 0 never converges; the other two thirds of the cases do)
    CHECK(converged == cases - cases / 3 && ran_out == cases / 3, "%d converged, %d ran to maxsteps of %d cases", converged, ran_out, cases);
    run_case({2, 8, 1, 0, 0, 1e-3, 9, 0, 0, false}, true);
    run_case({2, 8, 2, 0, 1, 1e-3, 9, 0, 0, false}, true);
    run_case({2, 8, 5, 0, 0, 0.0, 0, 0, 0, false}, false);   // no info rows at all
    // a map that fails: its code, negative or positive, comes back unchanged and nothing runs after it
    for (int at : {1, 2, 5})
        for (int code : {MUSE_ERR_HIP, MUSE_ERR_RCCL, -77, 1001}) run_case({3, 16, 10, 1, 0, 0.0, 4, at, code, false}, true);
    // zero score variance: the step is singular
    for (int nt = 1; nt <= kMaxTheta; ++nt) {
        const int rc = run_case({nt, 32, 10, 0, 0, 1e-3, 1, 0, 0, true}, false);
        CHECK(rc == MUSE_ERR_INVALID && g_msg.find("singular") != std::string::npos && g_msg.rfind("muse_run:", 0) == 0, "rc %d, \"%s\"", rc, g_msg.c_str());
    }
    CHECK(step_error(STEP_DOMAIN, "muse_run_sharded") == MUSE_ERR_INVALID && g_msg.rfind("muse_run_sharded: DomainError", 0) == 0, "\"%s\"", g_msg.c_str());
    CHECK(step_error(STEP_SINGULAR_LIKE) == MUSE_ERR_INVALID && g_msg.find("singular") != std::string::npos, "\"%s\"", g_msg.c_str());
    CHECK(step_error(STEP_OK) == MUSE_OK, "STEP_OK is no error");
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    printf("host loop driver ok: %d cases (%d converged, %d ran to maxsteps)\n", cases, converged, ran_out);
    return 0;
}
