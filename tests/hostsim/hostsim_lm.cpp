// hostsim_lm.cpp -- HOST restatement of the arithmetic of cpi_lm_prior_kernel / cpi_lm_cost_kernel / cpi_lm_accept_kernel
// (cpi_amd/csrc/cpi_lm_kernels.hpp): the CPI_HD functions of cpi_math.hpp those kernels call -- local_coordinates,
// chn::prior_relinearize, chn::chain_cost, chn::lm_decide -- one record / one chain at a time in the layouts of
// cpi_prior_relinearize_batch, cpi_chain_cost_batch and cpi_chain_accept_batch.  TEST INFRASTRUCTURE ONLY.
//
// Compile with -ffp-contract=off like its siblings: every fused multiply-add of the restatement is written as fma(), and the chain
// cost documents sums and a product that are NOT fused.  With -DHOSTSIM_LM_MAIN the file is a stand-alone program (seeded records
// and chains, self-checks), the one to build with -fsanitize=address,undefined.
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
// the states and the factors of chain c, clamped or refused as the entries do it (cpi_chain_util.hpp: chain_states / chain_range)
struct Range { long long f, ff; int n; bool bad; };
Range range_of(long long c, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst) {
    Range r;
    long long f = first ? first[c] : c * G, n = count ? count[c] : G;
    n = n < 0 ? 0 : (n > G ? G : n);
    f = f < 0 ? 0 : (f > S ? S : f);
    if (S - f < n) n = S - f;
    r.f = f; r.n = (int)n;
    r.ff = ffirst ? ffirst[c] : f - c;
    r.bad = n > 1 && (r.ff < 0 || r.ff > F - (n - 1));
    return r;
}
double cost_of(const Range &r, const double *chi2, const double *pcost) {
    if (r.bad) return NAN;
    return chn::chain_cost(r.n, (chi2 && r.n > 1) ? chi2 + r.ff : nullptr, (pcost && r.n > 0) ? pcost + r.f : nullptr);
}
}  // namespace

extern "C" {

// the rows of cpi_prior_relinearize_batch from xi that something else computed (the device's cpi_local_batch): rows [P][136], pcost [P]
int hsl_prior_from_xi(long long P, const double *xi, const double *prior0, double *rows, double *pcost) {
    for (long long p = 0; p < P; p++)
        chn::prior_relinearize(xi + p * 15, prior0 + p * 136, rows ? rows + p * 136 : nullptr, pcost ? pcost + p : nullptr);
    return 0;
}

// xi [P][15] as hsl_prior_relinearize forms it for records in state order (idx = NULL)
int hsl_local(long long P, const double *states, const double *anchor, double *xi) {
    for (long long p = 0; p < P; p++) local_coordinates(load_state(states + p * 16), load_state(anchor + p * 16), xi + p * 15);
    return 0;
}

// cpi_prior_relinearize_batch on host arrays.  Returns 0.
int hsl_prior_relinearize(long long S, long long P, const int *idx, const double *states, const double *anchor, const double *prior0,
                          double *prior, double *pcost) {
    for (long long p = 0; p < P; p++) {
        const long long s = idx ? idx[p] : p;
        if (s < 0 || s >= S) continue;
        double xi[15];
        local_coordinates(load_state(states + s * 16), load_state(anchor + p * 16), xi);
        chn::prior_relinearize(xi, prior0 + p * 136, prior ? prior + s * 136 : nullptr, pcost ? pcost + s : nullptr);
    }
    return 0;
}

// cpi_chain_cost_batch on host arrays.  Returns 0.
int hsl_chain_cost(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                   const double *chi2, const double *pcost, double *cost) {
    for (long long c = 0; c < C; c++) cost[c] = cost_of(range_of(c, G, S, F, first, count, ffirst), chi2, pcost);
    return 0;
}

// cpi_chain_accept_batch on host arrays; params: six doubles in the order of cpi_lm_params, or NULL for the defaults.  Returns 0.
int hsl_chain_accept(long long C, long long G, long long S, long long F, const long long *first, const int *count, const long long *ffirst,
                     const double *params, const double *chi2_new, const double *pcost_new, const double *trial, double *cost,
                     double *states, double *chi2, double *lambda, int *phase, int *accepted) {
    chn::LmParams P = {0.1, 10.0, 0.0, 1e5, 1e-5, 1e-5};
    if (params) { P.lam_down = params[0]; P.lam_up = params[1]; P.lam_min = params[2]; P.lam_max = params[3]; P.abs_tol = params[4]; P.rel_tol = params[5]; }
    for (long long c = 0; c < C; c++) {
        if (accepted) accepted[c] = 0;
        if (phase[c] != 0) continue;
        const Range r = range_of(c, G, S, F, first, count, ffirst);
        if (r.n == 0) { phase[c] = 1; continue; }
        const double nw = cost_of(r, chi2_new, pcost_new);
        double lam = lambda[c];
        int ph = 0;
        const int acc = chn::lm_decide(cost[c], nw, P, lam, ph);
        if (acc) {
            memcpy(states + r.f * 16, trial + r.f * 16, sizeof(double) * 16 * r.n);
            if (chi2 && r.n > 1) memcpy(chi2 + r.ff, chi2_new + r.ff, sizeof(double) * (r.n - 1));
            cost[c] = nw;
        }
        lambda[c] = lam;
        if (ph) phase[c] = ph;
        if (accepted) accepted[c] = acc;
    }
    return 0;
}

}  // extern "C"

#ifdef HOSTSIM_LM_MAIN
#include <stdio.h>
#include <stdlib.h>
static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }
int main() {
    srand(5);
    bool ok = true;
    // ---- prior: records in reverse order with a skipped index at either end; the arrays end where the records end
    const long long S = 9, P = 7;
    std::vector<double> st(S * 16), an(P * 16), p0(P * 136), pr(S * 136, -7.0), pc(S, -7.0);
    std::vector<int> idx = {-1, 8, 6, 5, 3, 1, (int)S};
    auto unit_state = [](double *x) {
        double n = 0;
        for (int i = 0; i < 4; i++) { x[i] = rnd(); n += x[i] * x[i]; }
        for (int i = 0; i < 4; i++) x[i] /= sqrt(n);
        for (int i = 4; i < 16; i++) x[i] = rnd();
    };
    for (long long s = 0; s < S; s++) unit_state(&st[s * 16]);
    for (long long p = 0; p < P; p++) {
        unit_state(&an[p * 16]);
        for (int i = 0; i < 136; i++) p0[p * 136 + i] = rnd();
        p0[p * 136 + 135] = NAN;                              // never read
    }
    memcpy(&an[2 * 16], &st[6 * 16], 16 * sizeof(double));    // record 2 sits at its anchor
    if (hsl_prior_relinearize(S, P, idx.data(), st.data(), an.data(), p0.data(), pr.data(), pc.data())) return 2;
    bool kept = true, same = pc[6] == 0.0 && pr[6 * 136 + 135] == 0.0;
    for (long long s : {0LL, 2LL, 4LL, 7LL})
        for (int i = 0; i < 136; i++) kept = kept && pr[s * 136 + i] == -7.0 && pc[s] == -7.0;
    for (int i = 0; i < 135; i++) same = same && pr[6 * 136 + i] == p0[2 * 136 + i];
    double worst = 0;                                         // pcost against the plain quadratic form in long double
    for (long long p = 1; p < P - 1; p++) {
        const long long s = idx[p];
        double xi[15];
        local_coordinates(load_state(&st[s * 16]), load_state(&an[p * 16]), xi);
        long double v = 0, scale = 0;
        for (int i = 0; i < 15; i++) {
            v += (long double)p0[p * 136 + 120 + i] * xi[i];
            scale += fabsl((long double)p0[p * 136 + 120 + i] * xi[i]);
            for (int k = 0; k < 15; k++) {
                v += 0.5L * xi[i] * chn::sym_at(&p0[p * 136], i, k) * xi[k];
                scale += fabsl(0.5L * xi[i] * chn::sym_at(&p0[p * 136], i, k) * xi[k]);
            }
        }
        worst = fmax(worst, (double)(fabsl(v - pc[s]) / scale));
    }
    printf("prior: rows without a record kept %d, a record at its anchor passes prior0 through %d, |pcost - quadratic form| %.3g of sum |terms|\n",
           (int)kept, (int)same, worst);
    ok = ok && kept && same && worst < 1e-14;

    // ---- cost and accept: ragged chains, one with factor rows outside, one frozen, one empty
    const int cnt[6] = {1, 17, 0, 33, 5, 2};
    long long C = 6, G = 33, Sc = 0, Fc = 0;
    std::vector<long long> first(C), ffirst(C);
    std::vector<int> count(cnt, cnt + 6);
    for (int c = 0; c < C; c++) { first[c] = Sc; ffirst[c] = Fc; Sc += cnt[c]; Fc += cnt[c] > 1 ? cnt[c] - 1 : 0; }
    ffirst[4] = Fc - 3;                                       // four rows from F - 3 on: refused, nothing is read
    std::vector<double> chi2(Fc), pco(Sc), cost(C), cur(C), lam(C, 1.0), tr(Sc * 16), xs(Sc * 16, -7.0), c2(Fc, -7.0);
    std::vector<int> phase(C, 0), acc(C, 9);
    for (auto &v : chi2) v = fabs(rnd());
    for (auto &v : pco) v = rnd();
    for (auto &v : tr) v = rnd();
    if (hsl_chain_cost(C, G, Sc, Fc, first.data(), count.data(), ffirst.data(), chi2.data(), pco.data(), cost.data())) return 2;
    double plain = 0;
    for (int k = 0; k < 32; k++) plain += 0.5 * chi2[ffirst[3] + k];
    for (int s = 0; s < 33; s++) plain += pco[first[3] + s];
    const bool shape = cost[2] == 0.0 && !signbit(cost[2]) && cost[4] != cost[4] && cost[0] == pco[0] && fabs(cost[3] - plain) < 1e-12;
    printf("cost: empty chain +0.0, refused chain NaN, one state = its pcost, 33 states within rounding of the plain sum: %d\n", (int)shape);
    ok = ok && shape;
    phase[5] = 2;
    for (int c = 0; c < C; c++) cur[c] = cost[c] + (c == 1 ? -1.0 : 1.0);   // chain 1 is rejected, 0 and 3 accepted, 4 NaN, 5 frozen
    std::vector<double> was = cur;
    if (hsl_chain_accept(C, G, Sc, Fc, first.data(), count.data(), ffirst.data(), nullptr, chi2.data(), pco.data(), tr.data(), cur.data(),
                         xs.data(), c2.data(), lam.data(), phase.data(), acc.data())) return 2;
    bool rule = acc[0] == 1 && acc[1] == 0 && acc[2] == 0 && acc[3] == 1 && acc[4] == 0 && acc[5] == 0 && phase[2] == 1 && phase[5] == 2 &&
                lam[0] == 0.1 && lam[1] == 10.0 && lam[3] == 0.1 && lam[4] == 10.0 && lam[5] == 1.0 && cur[0] == cost[0] && cur[1] == was[1] &&
                cur[3] == cost[3] && cur[5] == was[5];
    for (long long s = 0; s < Sc; s++) {
        const bool moved = s == first[0] || (s >= first[3] && s < first[3] + 33);
        for (int i = 0; i < 16; i++) rule = rule && xs[s * 16 + i] == (moved ? tr[s * 16 + i] : -7.0);
    }
    printf("accept: the rule table holds on six chains: %d\n", (int)rule);
    ok = ok && rule;
    return ok ? 0 : 1;
}
#endif
