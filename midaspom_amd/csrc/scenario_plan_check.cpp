// midaspom_amd/csrc/scenario_plan_check.cpp -- the exact scenario engine's
// host planner (spom_scenario_plan.cpp) over one survey row, without a device
// or the HIP runtime:
//   scenario_plan_check ROW M P D KIND "OPTIONS" NE NC NK ND [TS TDIS]
// ROW is one character per patch: '0' empty, '1' occupied, 'm' missing; any
// other digit is its value and '-' is -2 (both refused).  Prints the kernel
// the row and the options select, its counts and LDS bytes, FNV-1a digests of
// the tables it reads and of the source rows at distances 250, 500, ..., and
// the launches of both passes over an NE x NC x NK x ND grid (ts = 3,
// tdis = 2 unless given).  A count with a trailing '!' passes a null axis.
// Exit 0, or mdp_last_error() on stderr and exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spom_scenario_plan.h"

namespace {

uint64_t fnv(const void *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bit
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}

template <typename T>
unsigned long long dig(const std::vector<T> &v)
{
    return (unsigned long long)fnv(v.data(), v.size() * sizeof(T));
}

// an axis of `count` values; above 2^20 values it holds one (the planner
// reads the source distances alone)
struct Axis {
    uint32_t count = 0;
    std::vector<double> v;
    bool null = false;
    explicit Axis(const char *arg, double first, double step)
    {
        count = (uint32_t)strtoul(arg, nullptr, 10);
        null = arg[0] && arg[strlen(arg) - 1] == '!';
        v.resize(count <= (1u << 20) ? count : 1);
        for (size_t i = 0; i < v.size(); ++i) v[i] = first + step * (double)i;
    }
    const double *data() const { return null ? nullptr : v.data(); }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 11 && argc != 13) {
        fprintf(stderr, "usage: scenario_plan_check ROW M P D KIND \"OPTIONS\" NE NC NK ND [TS TDIS]\n");
        return 2;
    }
    auto fail = []() {
        fprintf(stderr, "scenario_plan_check: %s\n", mdp_last_error());
        return 1;
    };
    const uint32_t n = (uint32_t)strlen(argv[1]);
    std::vector<int32_t> row(n);
    for (uint32_t k = 0; k < n; ++k) row[k] = argv[1][k] == 'm' ? -1 : argv[1][k] == '-' ? -2 : argv[1][k] - '0';
    const double m = atof(argv[2]), d = atof(argv[4]);
    const float p = (float)atof(argv[3]);
    const int kind = atoi(argv[5]);
    const int ts = argc == 13 ? atoi(argv[11]) : 3, tdis = argc == 13 ? atoi(argv[12]) : 2;
    ScnOpts opts;
    if (scn_parse_opts(argv[6], &opts)) return fail();
    ScnPlan pl;
    if (scn_plan(row.data(), n, m, p, d, kind, opts, &pl)) return fail();
    printf("kernel %s\n", pl.kname);
    printf("plan n %u ns %u nsched %u btot %u lds %zu\n", pl.n, pl.ns, pl.nsched, pl.btot, pl.lds);
    printf("S %016llx w %016llx boff %016llx jsched %016llx jord %016llx\n", dig(pl.S), dig(pl.w), dig(pl.boff),
           dig(pl.jsched), dig(pl.jord));
    const Axis e(argv[7], 0.0, 0.01), c(argv[8], 0.0, 0.1), K(argv[9], 0.5, 0.25), ds(argv[10], 250.0, 250.0);
    if (kind == 1 && ds.count > ds.v.size()) {
        fprintf(stderr, "scenario_plan_check: ND <= 2^20 for the loss kind (the distances are read)\n");
        return 2;
    }
    ScnGrid g;
    if (scn_grid_plan(pl, ts, tdis, e.data(), e.count, c.data(), c.count, K.data(), K.count, ds.data(), ds.count, &g))
        return fail();
    printf("grid ne %u nc %u nK %u nd %u src %016llx nV %zu nY %zu big_pts %u\n", g.ne, g.nc, g.nK, g.nd, dig(g.src),
           g.nV, g.nY, g.big_pts);
    for (int mode = 0; mode < 2; ++mode)
        for (const ScnLaunch &l : g.launches[mode])
            printf("launch mode %d p0 %llu points %llu workgroups %u\n", mode, (unsigned long long)l.p0,
                   (unsigned long long)l.pts, l.nwg);
    return 0;
}
