// test_trial.cpp -- GPU: cpi_host::retract, cpi_host::local_coordinates and ImuFactorCPI::error end to end, product only, against
// values the Python test (tests/test_gpu_trial_cpp.py) wrote out with Engine.retract / local_coordinates / factor_cost_host: the same
// kernels behind another front, so every number must come back bit for bit.  Checks itself.
//   test_trial <file>
// file (whitespace-separated, %.17g): S, then states [S*16], delta [S*15], other [S*16], retract [S*16], local [S*15]; then NF and per
// factor: model, DT, alpha, beta, q, J_q, J_b, J_a, H_b, H_a, q_k_lin, O_b, O_a, P [225], grav, ba_lin, bg_lin, state_i, state_j, error.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../cpi_amd/csrc/cpi_host.hpp"

using namespace cpi_host;

static std::vector<double> take(std::ifstream &g, size_t n) {
    std::vector<double> v(n);
    for (size_t i = 0; i < n; i++)
        if (!(g >> v[i])) throw std::runtime_error("input file too short");
    return v;
}
template <class A> static A arr(std::ifstream &g) {
    A a;
    const std::vector<double> v = take(g, a.size());
    for (size_t i = 0; i < a.size(); i++) a[i] = v[i];
    return a;
}
static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    try {
        std::ifstream g(argv[1]);
        Context ctx;
        int bad = 0;
        const size_t S = (size_t)take(g, 1)[0];
        const std::vector<double> states = take(g, S * 16), delta = take(g, S * 15), other = take(g, S * 16), want_r = take(g, S * 16),
                                  want_l = take(g, S * 15);
        if (!same(retract(ctx, states, delta), want_r)) { printf("retract differs from the device form\n"); bad++; }
        if (!same(local_coordinates(ctx, states, other), want_l)) { printf("local_coordinates differs from the device form\n"); bad++; }
        try { retract(ctx, states, std::vector<double>(3)); printf("a short delta was accepted\n"); bad++; } catch (const std::invalid_argument &) {}
        const size_t NF = (size_t)take(g, 1)[0];
        for (size_t f = 0; f < NF; f++) {
            const int model = (int)take(g, 1)[0];
            const double DT = take(g, 1)[0];
            const Vec3 alpha = arr<Vec3>(g), beta = arr<Vec3>(g);
            const Vec4 q = arr<Vec4>(g);
            const Mat3 J_q = arr<Mat3>(g), J_b = arr<Mat3>(g), J_a = arr<Mat3>(g), H_b = arr<Mat3>(g), H_a = arr<Mat3>(g);
            const Vec4 qk = arr<Vec4>(g);
            const Mat3 O_b = arr<Mat3>(g), O_a = arr<Mat3>(g);
            const Mat15 P = arr<Mat15>(g);
            const Vec3 grav = arr<Vec3>(g), ba = arr<Vec3>(g), bg = arr<Vec3>(g);
            const std::vector<double> xi = take(g, 16), xj = take(g, 16);
            const double want = take(g, 1)[0];
            ImuFactorCPI fac = model == 1 ? ImuFactorCPI(P, DT, grav, alpha, beta, q, ba, bg, J_q, J_b, J_a, H_b, H_a)
                                          : ImuFactorCPI(P, DT, grav, alpha, beta, q, qk, ba, bg, J_q, J_b, J_a, H_b, H_a, O_b, O_a);
            const double got = fac.error(ctx, xi.data(), xj.data());
            double e15[15];
            fac.evaluateError(ctx, xi.data(), xj.data(), e15);      // the factor still evaluates
            if (memcmp(&got, &want, sizeof got) != 0 || !(got >= 0)) { printf("factor %zu (model %d): error %.17g, expected %.17g\n", f, model, got, want); bad++; }
        }
        if (bad) return 1;
        printf("test_trial ok %zu %zu\n", S, NF);
    } catch (const std::exception &e) {
        printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
