// hostsim_between.cpp -- HOST restatement of the arithmetic of cpi_between_kernel<kind> (cpi_amd/csrc/cpi_between_kernels.hpp): the CPI_HD
// functions of cpi_math.hpp that kernel calls -- chn::between_geometry, between_residual, between_jcol, between_acol, between_term,
// composed by chn::factor_between -- one factor at a time in the layout of cpi_state_between_batch, ranges and indices clamped as the
// kernel clamps them.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma(), and chi2
// documents squares that are NOT fused.  With -DHOSTSIM_BETWEEN_MAIN the file is a stand-alone program (seeded states and
// measurements, self-checks), the one to build with -fsanitize=address,undefined.
#include "../../cpi_amd/csrc/cpi_math.hpp"
#include <stdint.h>
#include <string.h>
#include <vector>
using namespace cpi;

namespace {
NavState load_state(const double *p) {
    NavState s;
    s.q = ldq(p); s.bg = ldv(p + 4); s.v = ldv(p + 7); s.ba = ldv(p + 10); s.p = ldv(p + 13);
    return s;
}
long long clampM(long long v, long long M) { return v < 0 ? 0 : (v > M ? M : v); }
long long state_of(const int *idx, long long f, long long off, long long S) { return clampM(idx ? (long long)idx[f] : f + off, S - 1); }

template <int K>
void run(long long F, long long M, const long long *mfirst, const double *states, long long S, const int *idx_i, const int *idx_j, const double *z,
         const double *R, const double *weight, const double *hess_base, const double *chi2_base, double *hess, double *chi2, double *chi2_m) {
    typedef chn::Between<K> T;
    for (long long f = 0; f < F; f++) {
        const long long m0 = clampM(mfirst[f], M);
        long long m1 = clampM(mfirst[f + 1], M);
        if (m1 < m0) m1 = m0;
        chn::factor_between<K>(load_state(states + state_of(idx_i, f, 0, S) * 16), load_state(states + state_of(idx_j, f, 1, S) * 16), m1 - m0,
                               z + m0 * T::ZN, R + m0 * T::RN, weight ? weight + m0 : nullptr, hess_base ? hess_base + f * 496 : nullptr,
                               chi2_base ? chi2_base[f] : 0.0, hess ? hess + f * 496 : nullptr, chi2 ? chi2 + f : nullptr,
                               chi2_m ? chi2_m + m0 : nullptr);
    }
}

// e [d] and J [d][30] (row-major, the 30 tangent columns of the pair) of one measurement
template <int K>
void jac(const double *xi, const double *xj, const double *z, double *e, double *J) {
    typedef chn::Between<K> T;
    const chn::BetweenGeo g = chn::between_geometry<K>(load_state(xi), load_state(xj));
    chn::between_residual<K>(g, z, e);
    for (int i = 0; i < T::D * 30; i++) J[i] = 0.0;
    for (int c = 0; c < T::NC - 1; c++) {
        double Jc[T::D];
        chn::between_jcol<K>(g, c, Jc);
        for (int r = 0; r < T::D; r++) J[r * 30 + T::col(c)] = Jc[r];
    }
}
}  // namespace

extern "C" {

// cpi_state_between_batch on host arrays.  Returns 0, or 1 for an unknown kind.
int hsb_state_between(long long F, long long M, int kind, const long long *mfirst, const double *states, long long S, const int *idx_i,
                      const int *idx_j, const double *z, const double *R, const double *weight, const double *hess_base, const double *chi2_base,
                      double *hess, double *chi2, double *chi2_m) {
    switch (kind) {
        case chn::BETWEEN_POSITION: run<chn::BETWEEN_POSITION>(F, M, mfirst, states, S, idx_i, idx_j, z, R, weight, hess_base, chi2_base, hess, chi2, chi2_m); return 0;
        case chn::BETWEEN_ORIENTATION: run<chn::BETWEEN_ORIENTATION>(F, M, mfirst, states, S, idx_i, idx_j, z, R, weight, hess_base, chi2_base, hess, chi2, chi2_m); return 0;
        case chn::BETWEEN_POSE: run<chn::BETWEEN_POSE>(F, M, mfirst, states, S, idx_i, idx_j, z, R, weight, hess_base, chi2_base, hess, chi2, chi2_m); return 0;
    }
    return 1;
}

// the residual e [d] and the Jacobian J [d][30] of ONE measurement z between the states xi, xj [16] (what the documented-order
// restatement of the tests starts from, and what the finite differences are held against)
int hsb_jacobian(int kind, const double *xi, const double *xj, const double *z, double *e, double *J) {
    switch (kind) {
        case chn::BETWEEN_POSITION: jac<chn::BETWEEN_POSITION>(xi, xj, z, e, J); return 0;
        case chn::BETWEEN_ORIENTATION: jac<chn::BETWEEN_ORIENTATION>(xi, xj, z, e, J); return 0;
        case chn::BETWEEN_POSE: jac<chn::BETWEEN_POSE>(xi, xj, z, e, J); return 0;
    }
    return 1;
}

}  // extern "C"

#ifdef HOSTSIM_BETWEEN_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(11);
    bool ok = true;
    // five factors with 0, 1, 2, 17 and 0 measurements over six chained states; every array ends where its rows end
    const long long F = 5, S = 6, cnt[5] = {0, 1, 2, 17, 0};
    std::vector<long long> mf(F + 1, 0);
    for (int f = 0; f < F; f++) mf[f + 1] = mf[f] + cnt[f];
    const long long M = mf[F];
    std::vector<double> st(S * 16), base(F * 496), cb(F);
    for (long long s = 0; s < S; s++) {
        double n = 0;
        for (int i = 0; i < 4; i++) { st[s * 16 + i] = rnd(); n += st[s * 16 + i] * st[s * 16 + i]; }
        for (int i = 0; i < 4; i++) st[s * 16 + i] /= sqrt(n);
        for (int i = 4; i < 16; i++) st[s * 16 + i] = rnd();
    }
    for (auto &v : base) v = rnd();
    for (auto &v : cb) v = fabs(rnd());
    const int ZN[3] = {3, 4, 7}, RN[3] = {6, 6, 21}, NT[3] = {55, 28, 91};
    for (int kind = 0; kind < 3; kind++) {
        std::vector<double> z(M * ZN[kind]), R(M * RN[kind]), w(M), out(F * 496, -7.0), c2(F, -7.0), cm(M, -7.0);
        for (auto &v : z) v = rnd();
        for (auto &v : R) v = rnd();
        for (auto &v : w) v = fabs(rnd());
        if (hsb_state_between(F, M, kind, mf.data(), st.data(), S, nullptr, nullptr, z.data(), R.data(), w.data(), base.data(), cb.data(), out.data(), c2.data(), cm.data())) return 2;
        bool kept = c2[0] == cb[0] && c2[4] == cb[4];
        for (int i = 0; i < 496; i++) kept = kept && out[i] == base[i] && out[4 * 496 + i] == base[4 * 496 + i];
        int changed = 0;
        for (int i = 0; i < 496; i++) changed += out[3 * 496 + i] != base[3 * 496 + i];
        // chi2 against the plain sum in long double, factor 3 (17 measurements)
        long double v = cb[3];
        for (long long m = mf[3]; m < mf[4]; m++) v += (long double)w[m] * cm[m];
        const bool sum = fabsl(v - c2[3]) < 1e-12L * (1 + fabsl(v));
        // in place: the same bits
        std::vector<double> in(base), cin(cb);
        if (hsb_state_between(F, M, kind, mf.data(), st.data(), S, nullptr, nullptr, z.data(), R.data(), w.data(), in.data(), cin.data(), in.data(), cin.data(), nullptr)) return 2;
        const bool same = memcmp(in.data(), out.data(), F * 496 * sizeof(double)) == 0 && memcmp(cin.data(), c2.data(), F * sizeof(double)) == 0;
        printf("kind %d: factors without measurements keep their base %d, %d of %d touched entries changed, chi2 is the weighted sum %d, in place %d\n",
               kind, (int)kept, changed, NT[kind], (int)sum, (int)same);
        ok = ok && kept && sum && same && changed == NT[kind];
    }
    // a broken mfirst and broken indices are clamped: nothing outside the arrays is touched (the sanitizer build is the check)
    std::vector<long long> broken = {-3, 40, 2, 1000, -1, 5};
    std::vector<int> bi = {-5, 100, 0, 7, 2}, bj = {6, -1, 3, 3, 1 << 30};
    std::vector<double> z(M * 3, 0.5), R(M * 6, 1.0), out(F * 496), c2(F);
    if (hsb_state_between(F, M, 0, broken.data(), st.data(), S, bi.data(), bj.data(), z.data(), R.data(), nullptr, nullptr, nullptr, out.data(), c2.data(), nullptr)) return 2;
    if (hsb_state_between(F, M, 9, mf.data(), st.data(), S, nullptr, nullptr, z.data(), R.data(), nullptr, nullptr, nullptr, out.data(), c2.data(), nullptr) != 1) ok = false;
    // the padded arrays of tests/between_edge_checks.py: z, R, weight and chi2_m with PAD measurements on either side, the states with
    // PADS states, NaN in the input pads and -7 in chi2_m; an mfirst and indices that leave their ranges by less than the pads.  The
    // clamp keeps every access inside the interiors: nothing comes back NaN and no pad of chi2_m is written.
    {
        const long long PAD = 4, PADS = 2;
        const double nan = NAN;
        std::vector<double> bz((M + 2 * PAD) * 7, nan), bR((M + 2 * PAD) * 21, nan), bw(M + 2 * PAD, nan), bs((S + 2 * PADS) * 16, nan), bm(M + 2 * PAD, -7.0);
        for (long long i = 0; i < M * 7; i++) bz[PAD * 7 + i] = (i % 7 == 3) ? 1.0 : 0.25;
        for (long long i = 0; i < M * 21; i++) bR[PAD * 21 + i] = 1.0;
        for (long long i = 0; i < M; i++) bw[PAD + i] = 0.5;
        for (long long i = 0; i < S * 16; i++) bs[PADS * 16 + i] = st[i];
        std::vector<long long> pm(mf);
        pm[0] = -3; pm[2] = pm[1] - 1; pm[F] = M + 3;
        std::vector<int> pi = {-1, 1, (int)S + 1, 3, 4}, pj = {1, (int)S, 3, -2, 5};
        std::vector<double> po(F * 496, nan), pc(F, nan);
        if (hsb_state_between(F, M, 2, pm.data(), bs.data() + PADS * 16, S, pi.data(), pj.data(), bz.data() + PAD * 7, bR.data() + PAD * 21, bw.data() + PAD,
                              nullptr, nullptr, po.data(), pc.data(), bm.data() + PAD)) return 2;
        bool inside = true;
        for (double v : po) inside = inside && v == v;
        for (double v : pc) inside = inside && v == v;
        for (long long i = 0; i < PAD; i++) inside = inside && bm[i] == -7.0 && bm[PAD + M + i] == -7.0;
        for (long long i = 0; i < M; i++) inside = inside && bm[PAD + i] == bm[PAD + i];
        printf("padded arrays, broken mfirst and indices: everything stays inside %d\n", (int)inside);
        ok = ok && inside;
    }
    return ok ? 0 : 1;
}
#endif
