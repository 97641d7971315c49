// ASan/UBSan harness for the host logic of an encode to an error bound (csrc/wr_budget.h), compiled by g++: the start point
// against a scan of the grid, and the walk over synthetic error curves E(g) -- smooth, jagged, with plateaus, far from
// nominal, with a floor -- checked against the contract: what comes back holds, its coarser neighbour does not, no point is
// asked about twice or outside [g_min, kGMax], and a bound nobody meets is reported with E(g_min).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "wr_budget.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }
static double unit() { return (rnd() & 0xfffff) / 1048576.0; }

static int scan_start(double m, double absmax)
{
    if (!(m > 0) || !(absmax > 0) || m > DBL_MAX || absmax > DBL_MAX) return -1;
    int best = -1;
    for (int g = 0; g <= wrbud::kGMax; g++) if (wrbud::grid_tol(g) * absmax <= m) best = g;
    return best;
}

static int check_start(double m, double absmax)
{
    const int got = wrbud::bounded_start(m, absmax), want = scan_start(m, absmax);
    if (got != want) { printf("bounded_start(%.17g, %.17g) = %d, the scan gives %d\n", m, absmax, got, want); return 1; }
    return 0;
}

// one walk over the curve E (exactly kGMax + 1 values on the heap: an index outside is ASan's)
static int check_walk(const std::vector<double>& E, double m, int g_min, int start, const char* what, int* most)
{
    std::vector<int> asked((size_t)wrbud::kGMax + 1, 0);
    int trials = 0, out_of_range = 0;
    auto eval = [&](int g, double* e) {
        if (g < g_min || g > wrbud::kGMax) { out_of_range++; return 7; }
        asked[(size_t)g]++;
        trials++;
        *e = E[(size_t)g];
        return 0;
    };
    int g = -5;
    double e = -1;
    const int rc = wrbud::bounded_walk(m, g_min, start, eval, &g, &e);
    if (out_of_range) { printf("%s: a point outside [%d, %d] was asked about\n", what, g_min, wrbud::kGMax); return 1; }
    for (int k = 0; k <= wrbud::kGMax; k++) if (asked[(size_t)k] > 1) { printf("%s: point %d formed %d times\n", what, k, asked[(size_t)k]); return 1; }
    if (trials > *most) *most = trials;
    if (rc == wrbud::kBoundedMiss) {
        if (g != g_min || e != E[(size_t)g_min] || E[(size_t)g_min] <= m) { printf("%s: a miss that is none (g %d, g_min %d)\n", what, g, g_min); return 1; }
        return 0;
    }
    if (rc) { printf("%s: rc %d\n", what, rc); return 1; }
    if (g < g_min || g > wrbud::kGMax) { printf("%s: g = %d outside the grid\n", what, g); return 1; }
    if (e != E[(size_t)g] || !(e <= m)) { printf("%s: E(%d) = %g does not hold for %g\n", what, g, E[(size_t)g], m); return 1; }
    if (g < wrbud::kGMax && E[(size_t)g + 1] <= m) { printf("%s: %d is not tight\n", what, g); return 1; }
    if (!asked[(size_t)g] || (g < wrbud::kGMax && !asked[(size_t)g + 1])) { printf("%s: the verdict on %d was not formed\n", what, g); return 1; }
    return 0;
}

int main()
{
    int bad = 0;
    // ---- the start point
    const double absmaxes[] = {1.0, 3.0, 1e-300, 1e300, 0x1p-1022, 4.9e-324, DBL_MAX, 0.7};
    for (double a : absmaxes) {
        for (int g = 0; g <= wrbud::kGMax; g += 1 + (int)(rnd() % 5)) {
            const double m = wrbud::grid_tol(g) * a;
            bad += check_start(m, a) + check_start(nextafter(m, 0.0), a) + check_start(nextafter(m, INFINITY), a);
        }
        bad += check_start(DBL_MAX, a) + check_start(4.9e-324, a);
    }
    const double junk[] = {0.0, -0.0, -1.0, NAN, INFINITY, -INFINITY};
    for (double j : junk) {
        if (wrbud::bounded_start(j, 1.0) != -1 || wrbud::bounded_start(1.0, j) != -1) { printf("bounded_start takes %g\n", j); bad++; }
    }
    for (int it = 0; it < 2000; it++) bad += check_start(ldexp(unit() + 0.5, (int)(rnd() % 200) - 130), ldexp(unit() + 0.5, (int)(rnd() % 120) - 60));

    // ---- the walk
    int most = 0;
    for (int it = 0; it < 3000 && !bad; it++) {
        const int kind = it % 6;
        const double absmax = ldexp(unit() + 0.5, (int)(rnd() % 40) - 20);
        const double off = kind == 3 ? 0.02 + 30 * unit() : 0.6 + 0.6 * unit();  // (kind 3: far from nominal, either way)
        const double jag = kind == 1 ? 0.3 : kind == 2 ? 0.05 : kind == 5 ? 0.9 : 0.0;
        const double floor_e = kind == 4 ? absmax * ldexp(1.0, -(int)(rnd() % 50)) : 0.0;
        std::vector<double> E((size_t)wrbud::kGMax + 1);
        for (int g = 0; g <= wrbud::kGMax; g++) {
            double v = wrbud::grid_tol(kind == 2 ? (g & ~15) : g) * absmax * off * (1.0 + jag * (unit() - 0.5));
            if (v < floor_e) v = floor_e;
            E[(size_t)g] = v;
        }
        const int gq = (int)(rnd() % (wrbud::kGMax + 1));
        const double m = it % 7 == 0 ? E[(size_t)gq] : it % 7 == 1 ? nextafter(E[(size_t)gq], 0.0) : wrbud::grid_tol(gq) * absmax * (0.5 + unit());
        if (!(m > 0)) continue;
        const int g_min = it % 3 == 0 ? 0 : (int)(rnd() % (wrbud::kGMax + 1));
        bad += check_walk(E, m, g_min, wrbud::bounded_start(m, absmax), "from the start point", &most);
        bad += check_walk(E, m, g_min, (int)(rnd() % (wrbud::kGMax + 40)) - 20, "from anywhere", &most);
    }
    // all zero, all above the bound, a single point that holds
    {
        std::vector<double> E((size_t)wrbud::kGMax + 1, 0.0);
        bad += check_walk(E, 1.0, 0, 100, "all zero", &most);
        std::fill(E.begin(), E.end(), 2.0);
        bad += check_walk(E, 1.0, 17, 3000, "none holds", &most);
        E[17] = 0.5;
        bad += check_walk(E, 1.0, 17, 3000, "only g_min holds", &most);
        E[wrbud::kGMax] = 1.0;
        bad += check_walk(E, 1.0, 17, wrbud::kGMax, "the end holds, with equality", &most);
    }
    if (bad) return 1;
    printf("bounded search sanitizer run OK (%d trials at most)\n", most);
    return 0;
}
