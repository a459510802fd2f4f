// pcg_driver.cpp -- the diagonally preconditioned lock-step conjugate gradients of libmuse_lbfgs.so
// (museinference.jl_amd/lbfgs/pcg_control.hpp, pcg_advance.hpp) on the CPU: the same headers the preconditioned round kernel compiles,
// over a vector backend of naive loops, driven round by round as the host drives the kernel (apply M to p, advance, until the row is
// no longer active).  Prints one line per case:
//     name count rounds resnorm true_residual |b| max|y|
// tests/test_pcg_control.py compares every line with simple._pcg and tests/pcg_reference.py on the same operator, diagonal and
// right-hand side.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../museinference.jl_amd/lbfgs/pcg_advance.hpp"

using namespace muse_lbfgs;

struct HostVectors {
    int n;
    std::vector<double> b, d, p, y, r;     // b: the right-hand side in begin, M p in a round;  d: the diagonal
    explicit HostVectors(int n_) : n(n_), b(n_), d(n_), p(n_, 7.0), y(n_, 1.0), r(n_, 1.0) {}
    void start(double& rr, double& rho, double& bad) {
        rr = rho = bad = 0.0;
        for (int e = 0; e < n; ++e) {
            const double c = b[e] / d[e];
            y[e] = 0.0;
            r[e] = b[e];
            p[e] = c;
            rr += b[e] * b[e];
            rho += c * b[e];
            bad += pcg_bad_entry(d[e]) ? 1.0 : 0.0;
        }
    }
    void direction_is_rhs() {
        for (int e = 0; e < n; ++e) p[e] = b[e];
    }
    double dot_p_Mp() {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) acc += p[e] * b[e];
        return acc;
    }
    void update(double alpha, double& rr, double& rho) {
        rr = rho = 0.0;
        for (int e = 0; e < n; ++e) {
            y[e] = y[e] + alpha * p[e];
            r[e] = r[e] - alpha * b[e];
            rr += r[e] * r[e];
            rho += (r[e] / d[e]) * r[e];
        }
    }
    void next_direction(double beta) {
        for (int e = 0; e < n; ++e) p[e] = r[e] / d[e] + beta * p[e];
    }
};

typedef std::function<void(int, const double*, double*)> Operator;   // out = M in

// The right-hand side of a case of size n: the first n doubles of the file named by the first argument; the weights W of the scaled
// family: the first n doubles of the file named by the second (the test's own vectors, the same bits on both sides).
static std::vector<double> master, weights;
static double rhs_at(int i) { return i < (int)master.size() ? master[i] : (double)((i * 7919 + 13) % 1009) / 1009.0 - 0.5; }
static double weight_at(int i) { return i < (int)weights.size() ? weights[i] : exp(2.0 * sin(1.7 * (double)i + 0.3)); }

static int failures = 0;

static void run(const std::string& name, int n, const Operator& M, const std::vector<double>& rhs, const std::vector<double>& diag,
                double reltol, double abstol, int maxiter) {
    HostVectors v(n);
    v.b = rhs;
    v.d = diag;
    CgRecord c;
    bool active = pcg_begin_row(c, v, reltol, abstol, maxiter);      // muse_lbfgs_pcg_begin
    bool finite_p = true;
    for (int e = 0; e < n; ++e) finite_p = finite_p && (isfinite(v.p[e]) || !isfinite(rhs[e]));
    if (!active && c.count < 0 && !finite_p) { printf("%s left a direction that is not finite\n", name.c_str()); failures += 1; }
    std::vector<double> Mp(n);
    int rounds = 0;
    while (active) {
        M(n, v.p.data(), v.b.data());
        rounds += 1;
        active = pcg_advance_row(c, v);
        if (rounds > 100000) { printf("%s did not end\n", name.c_str()); failures += 1; return; }
    }
    // the true residual |rhs - M y|
    M(n, v.y.data(), Mp.data());
    double res = 0.0, bb = 0.0, ymax = 0.0;
    for (int e = 0; e < n; ++e) {
        res += (rhs[e] - Mp[e]) * (rhs[e] - Mp[e]);
        bb += rhs[e] * rhs[e];
        ymax = fmax(ymax, fabs(v.y[e]));
    }
    printf("%s %d %d %.17g %.17g %.17g %.17g\n", name.c_str(), c.count, rounds, sqrt(c.rr), sqrt(res), sqrt(bb), ymax);
    // ... and a further round changes nothing: not the record, not y, not the direction the operator is given
    const CgRecord before = c;
    const std::vector<double> p0 = v.p, y0 = v.y;
    for (int e = 0; e < n; ++e) v.b[e] = NAN;
    pcg_advance_row(c, v);
    if (memcmp(&before, &c, sizeof(CgRecord)) != 0 || memcmp(p0.data(), v.p.data(), 8 * n) != 0 || memcmp(y0.data(), v.y.data(), 8 * n) != 0) {
        printf("%s changed after the end\n", name.c_str());
        failures += 1;
    }
}

static std::vector<double> rhs_of(int n) {
    std::vector<double> b(n);
    for (int i = 0; i < n; ++i) b[i] = rhs_at(i);
    return b;
}

static void read_doubles(const char* path, std::vector<double>& into) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("cannot read %s\n", path); exit(2); }
    double buf[512];
    size_t got;
    while ((got = fread(buf, sizeof(double), 512, f)) > 0) into.insert(into.end(), buf, buf + got);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc > 1) read_doubles(argv[1], master);
    if (argc > 2) read_doubles(argv[2], weights);
    const double reltol = sqrt(2.220446049250313e-16);
    const int ns[5] = {1, 5, 255, 257, 4097}, ks[4] = {1, 2, 3, 5};
    // the diagonal operator of the plain driver with its own diagonal as d: one iteration, whatever k
    for (int n : ns)
        for (int k : ks) {
            const Operator diag = [k](int m, const double* in, double* out) {
                for (int i = 0; i < m; ++i) out[i] = (1.0 + 0.75 * (double)(i % k)) * in[i];
            };
            std::vector<double> d(n), one(n, 1.0);
            for (int i = 0; i < n; ++i) d[i] = 1.0 + 0.75 * (double)(i % k);
            run("diag_n" + std::to_string(n) + "_k" + std::to_string(k), n, diag, rhs_of(n), d, reltol, 0.0, 100);
            run("unit_diag_n" + std::to_string(n) + "_k" + std::to_string(k), n, diag, rhs_of(n), one, reltol, 0.0, 100);   // d = 1: plain CG
        }
    const auto periodic = [](double s) {
        return Operator([s](int m, const double* in, double* out) {
            for (int i = 0; i < m; ++i) out[i] = (2.0 + s) * in[i] - in[(i + m - 1) % m] - in[(i + 1) % m];
        });
    };
    const auto ones = [](int n) { return std::vector<double>(n, 1.0); };
    run("unit_periodic_n33_s1", 33, periodic(1.0), rhs_of(33), ones(33), reltol, 0.0, 100);
    run("unit_periodic_n257_s1", 257, periodic(1.0), rhs_of(257), ones(257), reltol, 0.0, 100);
    run("unit_periodic_n257_s025", 257, periodic(0.25), rhs_of(257), ones(257), reltol, 0.0, 100);
    // the scaled periodic family: M = W T W, T p = 3 p - roll(p, 1) - roll(p, -1), d = 3 W^2
    const Operator scaled = [](int m, const double* in, double* out) {
        std::vector<double> q(m);
        for (int i = 0; i < m; ++i) q[i] = weight_at(i) * in[i];
        for (int i = 0; i < m; ++i) out[i] = weight_at(i) * (3.0 * q[i] - q[(i + m - 1) % m] - q[(i + 1) % m]);
    };
    const auto scaled_diag = [](int n) {
        std::vector<double> d(n);
        for (int i = 0; i < n; ++i) d[i] = 3.0 * (weight_at(i) * weight_at(i));
        return d;
    };
    const int sns[5] = {5, 33, 255, 257, 4097};
    for (int n : sns) run("scaled_n" + std::to_string(n), n, scaled, rhs_of(n), scaled_diag(n), reltol, 0.0, 100);
    run("zero_rhs", 5, scaled, std::vector<double>(5, 0.0), scaled_diag(5), reltol, 0.0, 100);
    run("maxiter0", 257, scaled, rhs_of(257), scaled_diag(257), reltol, 0.0, 0);
    run("maxiter3", 257, scaled, rhs_of(257), scaled_diag(257), reltol, 0.0, 3);
    run("abstol", 257, scaled, rhs_of(257), scaled_diag(257), reltol, 1e-4, 100);
    const Operator indefinite = [](int, const double* in, double* out) {
        out[0] = in[0];
        out[1] = -in[1];
    };
    run("indefinite", 2, indefinite, std::vector<double>{1.0, 2.0}, std::vector<double>{1.0, 1.0}, reltol, 0.0, 100);
    const Operator nan_op = [](int m, const double*, double* out) {
        for (int i = 0; i < m; ++i) out[i] = NAN;
    };
    run("nan_operator", 5, nan_op, rhs_of(5), ones(5), reltol, 0.0, 100);
    // a diagonal that is not positive definite: the guard stops the row in begin, count -1, y = 0
    const double bads[4] = {0.0, -1.0, INFINITY, NAN};
    const char* bad_names[4] = {"zero", "negative", "infinite", "nan"};
    for (int i = 0; i < 4; ++i) {
        std::vector<double> d = scaled_diag(33);
        d[7] = bads[i];
        run(std::string("bad_diag_") + bad_names[i], 33, scaled, rhs_of(33), d, reltol, 0.0, 100);
    }
    // ... and a row that needs no iteration never uses its diagonal
    run("zero_rhs_bad_diag", 5, scaled, std::vector<double>(5, 0.0), std::vector<double>(5, 0.0), reltol, 0.0, 100);
    if (failures) return 1;
    printf("pcg driver ok\n");
    return 0;
}
