// cg_driver.cpp -- the lock-step conjugate gradients of libmuse_lbfgs.so (museinference.jl_amd/lbfgs/cg_control.hpp, cg_advance.hpp) on
// the CPU: the same headers the CG step kernel compiles, over a vector backend of naive loops, driven round by round as the host
// drives the kernel (apply M to p, advance, until the row is no longer active).  Prints one line per case:
//     name count rounds resnorm true_residual |b| max|y|
// tests/test_cg_control.py compares every line with simple._cg on the same operator and right-hand side in torch.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../museinference.jl_amd/lbfgs/cg_advance.hpp"

using namespace muse_lbfgs;

struct HostVectors {
    int n;
    std::vector<double> b, p, y, r;     // b: the right-hand side in begin, M p in a round
    explicit HostVectors(int n_) : n(n_), b(n_), p(n_), y(n_, 1.0), r(n_, 1.0) {}
    double start() {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            y[e] = 0.0;
            r[e] = p[e] = b[e];
            acc += b[e] * b[e];
        }
        return acc;
    }
    double dot_p_Mp() {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) acc += p[e] * b[e];
        return acc;
    }
    double update(double alpha) {
        double acc = 0.0;
        for (int e = 0; e < n; ++e) {
            y[e] = y[e] + alpha * p[e];
            r[e] = r[e] - alpha * b[e];
            acc += r[e] * r[e];
        }
        return acc;
    }
    void next_direction(double beta) {
        for (int e = 0; e < n; ++e) p[e] = r[e] + beta * p[e];
    }
};

typedef std::function<void(int, const double*, double*)> Operator;   // out = M in

// The right-hand side of a case of size n: the first n doubles of the file named by the first argument (the test's own vector, the
// same bits on both sides); without a file, a sequence that is exact in double arithmetic.
static std::vector<double> master;
static double rhs_at(int i) { return i < (int)master.size() ? master[i] : (double)((i * 7919 + 13) % 1009) / 1009.0 - 0.5; }

static int failures = 0;

static void run(const std::string& name, int n, const Operator& M, const std::vector<double>& rhs, double reltol, double abstol, int maxiter) {
    HostVectors v(n);
    v.b = rhs;
    CgRecord c;
    bool active = cg_begin_row(c, v, reltol, abstol, maxiter);      // muse_lbfgs_cg_begin
    std::vector<double> Mp(n);
    int rounds = 0;
    while (active) {
        M(n, v.p.data(), v.b.data());
        rounds += 1;
        active = cg_advance_row(c, v);
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
    cg_advance_row(c, v);
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

int main(int argc, char** argv) {
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
        double buf[512];
        size_t got;
        while ((got = fread(buf, sizeof(double), 512, f)) > 0) master.insert(master.end(), buf, buf + got);
        fclose(f);
    }
    const double reltol = sqrt(2.220446049250313e-16);
    const int ns[5] = {1, 5, 255, 257, 4097}, ks[4] = {1, 2, 3, 5};
    for (int n : ns)
        for (int k : ks) {
            const Operator diag = [k](int m, const double* in, double* out) {
                for (int i = 0; i < m; ++i) out[i] = (1.0 + 0.75 * (double)(i % k)) * in[i];
            };
            run("diag_n" + std::to_string(n) + "_k" + std::to_string(k), n, diag, rhs_of(n), reltol, 0.0, 100);
        }
    const auto periodic = [](double s) {
        return Operator([s](int m, const double* in, double* out) {
            for (int i = 0; i < m; ++i) out[i] = (2.0 + s) * in[i] - in[(i + m - 1) % m] - in[(i + 1) % m];
        });
    };
    run("periodic_n33_s1", 33, periodic(1.0), rhs_of(33), reltol, 0.0, 100);
    run("periodic_n257_s1", 257, periodic(1.0), rhs_of(257), reltol, 0.0, 100);
    run("periodic_n257_s025", 257, periodic(0.25), rhs_of(257), reltol, 0.0, 100);
    run("zero_rhs", 5, periodic(1.0), std::vector<double>(5, 0.0), reltol, 0.0, 100);
    run("maxiter0", 257, periodic(0.25), rhs_of(257), reltol, 0.0, 0);
    run("maxiter3", 257, periodic(0.25), rhs_of(257), reltol, 0.0, 3);
    run("abstol", 257, periodic(0.25), rhs_of(257), reltol, 1e-4, 100);
    const Operator indefinite = [](int, const double* in, double* out) {
        out[0] = in[0];
        out[1] = -in[1];
    };
    run("indefinite", 2, indefinite, std::vector<double>{1.0, 2.0}, reltol, 0.0, 100);
    const Operator nan_op = [](int m, const double*, double* out) {
        for (int i = 0; i < m; ++i) out[i] = NAN;
    };
    run("nan_operator", 5, nan_op, rhs_of(5), reltol, 0.0, 100);
    if (failures) return 1;
    printf("cg driver ok\n");
    return 0;
}
