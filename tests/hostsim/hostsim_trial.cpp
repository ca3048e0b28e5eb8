// hostsim_trial.cpp -- HOST restatement of the arithmetic of cpi_retract_kernel / cpi_local_kernel / cpi_factor_cost_kernel
// (cpi_amd/csrc/cpi_trial_kernels.hpp): the CPI_HD functions of cpi_math.hpp those kernels call -- retract_state, local_coordinates,
// factor_shared_core, whiten_row, chi2_of -- one state / one factor at a time.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off: chi2_of documents a summation without fused multiply-adds, and the device keeps to it by other
// means.  With -DHOSTSIM_TRIAL_MAIN the file is a stand-alone program (seeded inputs, self-checks), the one to build with
// -fsanitize=address,undefined.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <string.h>
using namespace cpi;

namespace {
NavState load_state(const double *p) {
    NavState s;
    s.q = ldq(p); s.bg = ldv(p + 4); s.v = ldv(p + 7); s.ba = ldv(p + 10); s.p = ldv(p + 13);
    return s;
}
void store_state(double *d, const NavState &o) {
    d[0] = o.q.x; d[1] = o.q.y; d[2] = o.q.z; d[3] = o.q.w;
    put3(d + 4, o.bg); put3(d + 7, o.v); put3(d + 10, o.ba); put3(d + 13, o.p);
}
}  // namespace

extern "C" {

int hst_retract(long long S, const double *states, const double *delta, double *out) {
    for (long long s = 0; s < S; s++) store_state(out + s * 16, retract_state(load_state(states + s * 16), delta + s * 15));
    return 0;
}

int hst_local(long long S, const double *x, const double *other, double *xi) {
    for (long long s = 0; s < S; s++) local_coordinates(load_state(x + s * 16), load_state(other + s * 16), xi + s * 15);
    return 0;
}

// fields: SoA arrays of F rows in the cpi_outputs layouts (column-major 3x3); R [F][225] dense column-major or [F][120] packed (tri)
int hst_cost(int model, long long F, const double *grav, const double *DT, const double *alpha, const double *beta, const double *q,
             const double *J_q, const double *J_b, const double *J_a, const double *H_b, const double *H_a, const double *O_b,
             const double *O_a, const double *lin, const double *qk, const double *xi, const double *xj, const double *R, int tri,
             double *werr, double *chi2) {
    if (model != 1 && model != 2) return 1;
    for (long long f = 0; f < F; f++) {
        FactorMeas m;
        m.alpha = alpha + f * 3; m.beta = beta + f * 3; m.q_KtoK1 = q + f * 4; m.lin = lin + f * 6; m.J_q = J_q + f * 9;
        m.J_beta = J_b + f * 9; m.J_alpha = J_a + f * 9; m.H_beta = H_b + f * 9; m.H_alpha = H_a + f * 9; m.dt = DT + f;
        m.q_K_lin = qk ? qk + f * 4 : q + f * 4; m.O_beta = O_b ? O_b + f * 9 : J_b + f * 9; m.O_alpha = O_a ? O_a + f * 9 : J_a + f * 9;
        m.xi = xi + f * 16; m.xj = xj + f * 16;
        m.grav = mk(grav[0], grav[1], grav[2]);
        FactorShared S;
        V3 e5[5];
        if (model == 1) factor_shared_core<1>(m, S, e5); else factor_shared_core<2>(m, S, e5);
        double e[15], w[15];
        for (int a = 0; a < 5; a++) put3(e + 3 * a, e5[a]);
        const double *Rf = R + f * (tri ? 120 : 225);
        for (int i = 0; i < 15; i++) w[i] = tri ? whiten_row<true>(Rf, e, i) : whiten_row<false>(Rf, e, i);
        memcpy(werr + f * 15, w, sizeof w);
        chi2[f] = chi2_of(w);
    }
    return 0;
}

}  // extern "C"

#ifdef HOSTSIM_TRIAL_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(7);
    const long long S = 257;
    std::vector<double> x(S * 16), d(S * 15), o(S * 16), back(S * 15);
    for (long long s = 0; s < S; s++) {
        double n = 0;
        for (int i = 0; i < 4; i++) { x[s * 16 + i] = rnd(); n += x[s * 16 + i] * x[s * 16 + i]; }
        for (int i = 0; i < 4; i++) x[s * 16 + i] /= sqrt(n);
        for (int i = 4; i < 16; i++) x[s * 16 + i] = 10 * rnd();
        for (int i = 0; i < 15; i++) d[s * 15 + i] = (s % 7 == 0) ? 0.0 : 0.3 * rnd();
    }
    hst_retract(S, x.data(), d.data(), o.data());
    hst_local(S, x.data(), o.data(), back.data());
    double worst = 0;
    for (long long s = 0; s < S; s++)
        for (int i = 3; i < 15; i++) worst = fmax(worst, fabs(back[s * 15 + i] - d[s * 15 + i]));   // additive part: local undoes retract
    // one model-1 factor with identity-like fields and R = I: chi2 = |e|^2 by the documented order
    std::vector<double> z9(9, 0.0), R(225, 0.0), we(15), c2(1);
    for (int i = 0; i < 15; i++) R[i * 15 + i] = 1.0;
    const double grav[3] = {0, 0, 9.81}, DT = 0.1, al[3] = {0, 0, 0}, be[3] = {0, 0, 0}, q[4] = {0, 0, 0, 1}, lin[6] = {0, 0, 0, 0, 0, 0};
    if (hst_cost(1, 1, grav, &DT, al, be, q, z9.data(), z9.data(), z9.data(), z9.data(), z9.data(), nullptr, nullptr, lin, nullptr,
                 x.data(), x.data() + 16, R.data(), 0, we.data(), c2.data()) != 0) return 2;
    double acc = we[0] * we[0];
    for (int i = 1; i < 15; i++) acc = acc + we[i] * we[i];
    printf("additive round trip %.3g, chi2 %.17g (order %s)\n", worst, c2[0], acc == c2[0] ? "ok" : "DIFFERS");
    return (worst < 1e-9 && acc == c2[0]) ? 0 : 1;
}
#endif
