// midaspom_amd/csrc/scnchain_plan_check.cpp -- the scenario chain's host
// planner (spom_scnchain_plan.cpp) over one survey row, without a device or
// the HIP runtime:
//   scnchain_plan_check ROW M P D KIND "OPTIONS" NK NREP DSRC
// ROW is one character per patch: '0' empty, '1' occupied, 'm' missing.
// Prints the kernel the options select, the row's counts, FNV-1a digests of
// the dispersal table, the default target and the source row at distance
// DSRC, the launches of a scenario table over NK grid points (one e, one c,
// one distance) and of the baseline table of its one (e, c), NREP replicates
// per class each, and the host evaluation (ts 2, tdis 1, default weights) of
// the one-point tables cnt[k][l] = (7k + 3l) % 5 + 1 and (k + 2l) % 3 + 1
// read as 10 replicates per class.
// Exit 0, or mdp_last_error() on stderr and exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spom_scnchain_plan.h"

namespace {

uint64_t fnv(const void *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bit
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}

void print_call(const char *what, const ChainCall &call)
{
    printf("%s points %llu tiles_per_class %llu tiles_per_point %llu cells %llu launches %zu\n", what,
           (unsigned long long)call.G, (unsigned long long)call.tiles_per_class,
           (unsigned long long)call.tiles_per_point, (unsigned long long)call.cells, call.launches.size());
    for (const ChainLaunch &l : call.launches)
        printf("launch p0 %llu npts %llu parts %llu units %llu nwg %u\n", (unsigned long long)l.p0,
               (unsigned long long)l.npts, (unsigned long long)l.parts, (unsigned long long)l.units, l.nwg);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 10) {
        fprintf(stderr, "usage: scnchain_plan_check ROW M P D KIND \"OPTIONS\" NK NREP DSRC\n");
        return 2;
    }
    auto fail = []() {
        fprintf(stderr, "scnchain_plan_check: %s\n", mdp_last_error());
        return 1;
    };
    const uint32_t n = (uint32_t)strlen(argv[1]);
    std::vector<int32_t> row(n);
    for (uint32_t k = 0; k < n; ++k) row[k] = argv[1][k] == 'm' ? -1 : argv[1][k] - '0';
    const double m = atof(argv[2]), d = atof(argv[4]), ds = atof(argv[9]);
    const float p = (float)atof(argv[3]);
    const int kind = atoi(argv[5]);
    const uint32_t nK = (uint32_t)strtoul(argv[7], nullptr, 10);
    const uint64_t nrep = strtoull(argv[8], nullptr, 10);
    ChainOpts opts;
    if (chain_parse_opts(argv[6], &opts)) return fail();
    ChainPlan pl;
    if (chain_plan(row.data(), n, m, p, d, kind, opts, &pl)) return fail();
    std::vector<double> src;
    chain_src(pl, false, &ds, 1, &src);
    printf("kernel k_scnchain<%u>\n", pl.nm);
    printf("row n %u nmiss %u n1 %u\n", pl.n, pl.nmiss, pl.n1);
    printf("M %016llx target %016llx src %016llx\n", (unsigned long long)fnv(pl.M.data(), pl.M.size() * sizeof(double)),
           (unsigned long long)fnv(pl.target.data(), pl.target.size() * sizeof(double)),
           (unsigned long long)fnv(src.data(), src.size() * sizeof(double)));
    const double e = 0.5, c = 0.5;
    std::vector<double> K(nK, 1.0);
    ChainCall call;
    if (chain_call(pl, false, &e, 1, &c, 1, K.data(), nK, &ds, 1, nrep, false, &call)) return fail();
    print_call("call", call);
    if (chain_call(pl, true, &e, 1, &c, 1, nullptr, 0, nullptr, 0, nrep, true, &call)) return fail();
    print_call("base", call);
    const uint32_t ncl = n + 1;
    std::vector<uint64_t> a((size_t)ncl * ncl), b((size_t)ncl * ncl);
    for (uint32_t k = 0; k < ncl; ++k)
        for (uint32_t l = 0; l < ncl; ++l) {
            a[(size_t)k * ncl + l] = (7 * k + 3 * l) % 5 + 1;
            b[(size_t)k * ncl + l] = (k + 2 * l) % 3 + 1;
        }
    double L = 0;
    std::vector<double> by(ncl);
    if (chain_eval(pl, 2, 1, 1, 1, 1, 1, a.data(), 10, b.data(), 10, nullptr, nullptr, &L, by.data())) return fail();
    printf("eval %a by_class %016llx\n", L, (unsigned long long)fnv(by.data(), by.size() * sizeof(double)));
    return 0;
}
