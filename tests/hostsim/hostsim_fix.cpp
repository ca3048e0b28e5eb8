// hostsim_fix.cpp -- HOST restatement of the arithmetic of cpi_fix_kernel<kind> (cpi_amd/csrc/cpi_fix_kernels.hpp): the CPI_HD
// functions of cpi_math.hpp that kernel calls -- chn::fix_residual, fix_vectors, fix_term, composed by chn::state_fix -- one state at a
// time in the layout of cpi_state_fix_batch, ranges clamped as the kernel clamps them.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma(), and chi2
// documents squares that are NOT fused.  With -DHOSTSIM_FIX_MAIN the file is a stand-alone program (seeded states and fixes,
// self-checks), the one to build with -fsanitize=address,undefined.
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

template <int K>
void run(long long S, long long M, const long long *mfirst, const double *states, const double *z, const double *R, const double *weight,
         const double *base, const double *pcost_base, double *out, double *pcost, double *chi2) {
    typedef chn::Fix<K> T;
    for (long long s = 0; s < S; s++) {
        const long long m0 = clampM(mfirst[s], M);
        long long m1 = clampM(mfirst[s + 1], M);
        if (m1 < m0) m1 = m0;
        chn::state_fix<K>(load_state(states + s * 16), m1 - m0, z + m0 * T::ZN, R + m0 * T::RN, weight ? weight + m0 : nullptr,
                          base ? base + s * 136 : nullptr, pcost_base ? pcost_base[s] : 0.0, out ? out + s * 136 : nullptr,
                          pcost ? pcost + s : nullptr, chi2 ? chi2 + m0 : nullptr);
    }
}
}  // namespace

extern "C" {

// cpi_state_fix_batch on host arrays.  Returns 0, or 1 for an unknown kind.
int hsf_state_fix(long long S, long long M, int kind, const long long *mfirst, const double *states, const double *z, const double *R,
                  const double *weight, const double *base, const double *pcost_base, double *out, double *pcost, double *chi2) {
    switch (kind) {
        case chn::FIX_POSITION: run<chn::FIX_POSITION>(S, M, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2); return 0;
        case chn::FIX_VELOCITY: run<chn::FIX_VELOCITY>(S, M, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2); return 0;
        case chn::FIX_ORIENTATION: run<chn::FIX_ORIENTATION>(S, M, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2); return 0;
        case chn::FIX_POSE: run<chn::FIX_POSE>(S, M, mfirst, states, z, R, weight, base, pcost_base, out, pcost, chi2); return 0;
    }
    return 1;
}

// the residual e [M][d] of every fix alone (what the documented-order restatement of the tests starts from)
int hsf_residual(long long S, long long M, int kind, const long long *mfirst, const double *states, const double *z, double *e) {
    for (long long s = 0; s < S; s++)
        for (long long m = clampM(mfirst[s], M); m < clampM(mfirst[s + 1], M); m++) {
            const NavState x = load_state(states + s * 16);
            switch (kind) {
                case chn::FIX_POSITION: chn::fix_residual<chn::FIX_POSITION>(x, z + m * 3, e + m * 3); break;
                case chn::FIX_VELOCITY: chn::fix_residual<chn::FIX_VELOCITY>(x, z + m * 3, e + m * 3); break;
                case chn::FIX_ORIENTATION: chn::fix_residual<chn::FIX_ORIENTATION>(x, z + m * 4, e + m * 3); break;
                case chn::FIX_POSE: chn::fix_residual<chn::FIX_POSE>(x, z + m * 7, e + m * 6); break;
                default: return 1;
            }
        }
    return 0;
}

}  // extern "C"

#ifdef HOSTSIM_FIX_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(7);
    bool ok = true;
    // five states with 0, 1, 2, 17 and 0 fixes; every array ends where its rows end
    const long long S = 5, cnt[5] = {0, 1, 2, 17, 0};
    std::vector<long long> mf(S + 1, 0);
    for (int s = 0; s < S; s++) mf[s + 1] = mf[s] + cnt[s];
    const long long M = mf[S];
    std::vector<double> st(S * 16), base(S * 136), pb(S);
    for (long long s = 0; s < S; s++) {
        double n = 0;
        for (int i = 0; i < 4; i++) { st[s * 16 + i] = rnd(); n += st[s * 16 + i] * st[s * 16 + i]; }
        for (int i = 0; i < 4; i++) st[s * 16 + i] /= sqrt(n);
        for (int i = 4; i < 16; i++) st[s * 16 + i] = rnd();
        for (int i = 0; i < 136; i++) base[s * 136 + i] = rnd();
        pb[s] = rnd();
    }
    const int ZN[4] = {3, 3, 4, 7}, RN[4] = {6, 6, 6, 21}, D[4] = {3, 3, 3, 6};
    for (int kind = 0; kind < 4; kind++) {
        std::vector<double> z(M * ZN[kind]), R(M * RN[kind]), w(M), out(S * 136, -7.0), pc(S, -7.0), chi2(M, -7.0);
        for (auto &v : z) v = rnd();
        for (auto &v : R) v = rnd();
        for (auto &v : w) v = fabs(rnd());
        if (hsf_state_fix(S, M, kind, mf.data(), st.data(), z.data(), R.data(), w.data(), base.data(), pb.data(), out.data(), pc.data(), chi2.data())) return 2;
        bool kept = pc[0] == pb[0] && pc[4] == pb[4] && out[135] == 0.0;
        for (int i = 0; i < 135; i++) kept = kept && out[i] == base[i] && out[4 * 136 + i] == base[4 * 136 + i];
        // pcost against the plain sum in long double, state 3 (17 fixes)
        long double v = pb[3];
        for (long long m = mf[3]; m < mf[4]; m++) v += 0.5L * w[m] * chi2[m];
        const bool sum = fabsl(v - pc[3]) < 1e-12L * (1 + fabsl(v));
        // a zero weight leaves the row alone and still reports chi2
        std::vector<double> w0(M, 0.0), out0(S * 136), chi0(M);
        if (hsf_state_fix(S, M, kind, mf.data(), st.data(), z.data(), R.data(), w0.data(), base.data(), nullptr, out0.data(), nullptr, chi0.data())) return 2;
        bool zero = true;
        for (int i = 0; i < 135; i++) zero = zero && out0[3 * 136 + i] == base[3 * 136 + i];
        for (long long m = 0; m < M; m++) zero = zero && chi0[m] == chi2[m];
        printf("kind %d (d %d): states without fixes keep their base %d, pcost is the weighted sum %d, weight 0 leaves the row %d\n", kind, D[kind],
               (int)kept, (int)sum, (int)zero);
        ok = ok && kept && sum && zero;
    }
    // a broken mfirst is clamped: nothing outside the arrays is touched (the sanitizer build is the check)
    std::vector<long long> broken = {-3, 40, 2, 1000, -1, 5};
    std::vector<double> z(M * 3, 0.5), R(M * 6, 1.0), out(S * 136), pc(S);
    if (hsf_state_fix(S, M, 0, broken.data(), st.data(), z.data(), R.data(), nullptr, nullptr, nullptr, out.data(), pc.data(), nullptr)) return 2;
    if (hsf_state_fix(S, M, 9, mf.data(), st.data(), z.data(), R.data(), nullptr, nullptr, nullptr, out.data(), pc.data(), nullptr) != 1) ok = false;
    return ok ? 0 : 1;
}
#endif
