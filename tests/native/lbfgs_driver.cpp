// lbfgs_driver.cpp -- the scalar machine of libmuse_lbfgs.so (museinference.jl_amd/lbfgs/lbfgs_control.hpp, lbfgs_advance.hpp) on the
// CPU: the same headers the advance kernel compiles, over a vector backend of naive loops, driven round by round as the host drives
// the kernel (evaluate at z, advance, until the problem is no longer active).  Prints one line per case:
//     name iterations f_calls status f_min gnorm x[0] [x[1]]
// tests/test_lbfgs_control.py compares every line with optim.lbfgs on the same function in torch.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <vector>

#include "../../museinference.jl_amd/lbfgs/lbfgs_advance.hpp"

using namespace muse_lbfgs;

struct HostVectors {
    int n;
    std::vector<double> g, z, x, s, gp, dx, dg, rho_, alpha_;
    explicit HostVectors(int n_) : n(n_), g(n_), z(n_), x(n_), s(n_, 0.0), gp(n_), dx(kM * n_), dg(kM * n_), rho_(kM, 0.0), alpha_(kM, 0.0) {}
    void intake(double& gs, double& absmax, double& nanc) {
        gs = 0.0, absmax = 0.0, nanc = 0.0;
        for (int e = 0; e < n; ++e) {
            gs += g[e] * s[e];
            nanc += g[e] != g[e] ? 1.0 : 0.0;
            absmax = fmax(absmax, fabs(g[e]));
        }
    }
    void start() {
        for (int e = 0; e < n; ++e) s[e] = gp[e] = g[e];
    }
    void write_trial(double c) {
        for (int e = 0; e < n; ++e) z[e] = x[e] + c * s[e];
    }
    void step_to(double c) {
        for (int e = 0; e < n; ++e) z[e] = x[e] = x[e] + c * s[e];
    }
    void pass_accept(double alpha, int slot, double& x_diff, double& dxdg, double& dgdg, double& dxg) {
        x_diff = dxdg = dgdg = dxg = 0.0;
        for (int e = 0; e < n; ++e) {
            const double d = alpha * s[e], xn = x[e] + d, y = g[e] - gp[e];
            x_diff = fmax(x_diff, fabs(xn - x[e]));
            dxdg += d * y;
            dgdg += y * y;
            dxg += d * g[e];
            x[e] = xn;
            dx[slot * n + e] = d;
            dg[slot * n + e] = y;
            gp[e] = g[e];
            s[e] = g[e];
        }
    }
    double stage_down(double a, int i, int inext) {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            s[e] = s[e] - a * dg[i * n + e];
            acc += dx[inext * n + e] * s[e];
        }
        return acc;
    }
    double stage_down_last(double a, int i, double scale) {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            const double q = s[e] - a * dg[i * n + e];
            s[e] = scale * q;
            acc += dg[i * n + e] * s[e];
        }
        return acc;
    }
    double stage_up(double coef, int i, int inext) {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            s[e] = s[e] + dx[i * n + e] * coef;
            acc += dg[inext * n + e] * s[e];
        }
        return acc;
    }
    double stage_up_last(double coef, int i) {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            s[e] = -(s[e] + dx[i * n + e] * coef);
            acc += g[e] * s[e];
        }
        return acc;
    }
    double negate_first() {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            s[e] = -s[e];
            acc += g[e] * s[e];
        }
        return acc;
    }
    double steepest() {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            s[e] = -g[e];
            acc += g[e] * s[e];
        }
        return acc;
    }
    double rho(int i) const { return rho_[i]; }
    double alpha(int i) const { return alpha_[i]; }
    void set_rho(int i, double v) { rho_[i] = v; }
    void set_alpha(int i, double v) { alpha_[i] = v; }
};

typedef std::function<double(const double*, double*)> Objective;   // value; writes the gradient

static void run(const char* name, int n, const Objective& fg, const double* x0, double g_tol) {
    HostVectors v(n);
    Problem p;
    problem_init(p, g_tol, 1000);
    for (int e = 0; e < n; ++e) v.x[e] = v.z[e] = x0[e];     // muse_lbfgs_begin
    int rounds = 0;
    for (;;) {
        const double f = fg(v.z.data(), v.g.data());
        rounds += 1;
        if (!advance_problem(p, v, f)) break;
        if (rounds > 100000) { printf("%s did not end\n", name); return; }
    }
    // a finished problem's evaluation point is its final point
    for (int e = 0; e < n; ++e)
        if (memcmp(&v.z[e], &v.x[e], 8) != 0 && !(p.status == STATUS_NONFINITE)) { printf("%s z != x\n", name); return; }
    printf("%s %d %d %d %.17g %.17g", name, p.iterations, p.f_calls, p.status, p.f, p.gnorm);
    for (int e = 0; e < n; ++e) printf(" %.17g", v.x[e]);
    printf("\n");
    // ... and a further round changes nothing
    const Problem before = p;
    advance_problem(p, v, 0.0);
    if (memcmp(&before, &p, sizeof(Problem)) != 0) printf("%s record changed after the end\n", name);
}

int main() {
    const Objective rosen = [](const double* z, double* g) {
        g[0] = -2 * (1 - z[0]) - 400 * z[0] * (z[1] - z[0] * z[0]);
        g[1] = 200 * (z[1] - z[0] * z[0]);
        return (1 - z[0]) * (1 - z[0]) + 100 * ((z[1] - z[0] * z[0]) * (z[1] - z[0] * z[0]));
    };
    const Objective bowl = [](const double* z, double* g) {
        g[0] = z[0];
        g[1] = z[1];
        return 0.5 * (z[0] * z[0] + z[1] * z[1]);
    };
    const Objective nan_f = [](const double* z, double* g) {
        g[0] = z[0];
        return (double)NAN;
    };
    // not finite beyond 2.5: the first trial from 0 (at 2.6) is, so the search shrinks it by psi3
    const Objective barrier = [](const double* z, double* g) {
        g[0] = (z[0] - 3) + 1 / (2.5 - z[0]);
        return 0.5 * ((z[0] - 3) * (z[0] - 3)) - log(2.5 - z[0]);
    };
    const Objective quartic = [](const double* z, double* g) {
        const double u = z[0] - 1;
        g[0] = 4 * (u * u * u) + z[0];
        return (u * u) * (u * u) + 0.5 * (z[0] * z[0]);
    };
    const double zero2[2] = {0.0, 0.0}, classic[2] = {-1.2, 1.0}, three[1] = {3.0}, one[1] = {1.0};
    run("rosenbrock_origin", 2, rosen, zero2, 1e-8);
    run("rosenbrock_classic", 2, rosen, classic, 1e-8);
    run("converged_at_start", 2, bowl, zero2, 1e-8);
    run("nan_objective", 1, nan_f, one, 1e-8);
    run("nonfinite_first_trial", 1, barrier, zero2, 1e-8);
    run("quartic", 1, quartic, three, 1e-8);
    printf("lbfgs driver ok\n");
    return 0;
}
