// midaspom_amd/csrc/future_plan_check.cpp -- the future engine's host planner
// (spom_future_plan.cpp) over one survey row, without a device or the HIP
// runtime:
//   future_plan_check ROW M D KD KS DS "OPTIONS" [TFUT]
// ROW is one character per patch: '0' empty, '1' occupied, 'm' missing.
// Prints the kernel the options select; for a lane kernel one line of its
// plan (the missing count, the occupied mask, FNV-1a digests of the missing
// bits, of M*K_D and of the source row); for k_future_wide the layout the
// kernel is given, after checking every entry the kernel can read of the
// distance image against the n x n table's expression, and the state layout
// against its inverse.  With TFUT, one more line: the summary path's window plan for
// that many years under the options.  Exit 0, or mdp_last_error() on stderr and exit 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spom_future_plan.h"

namespace {

uint64_t fnv(const void *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a, 64 bit
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 8 && argc != 9) {
        fprintf(stderr, "usage: future_plan_check ROW M D KD KS DS \"OPTIONS\" [TFUT]\n");
        return 2;
    }
    auto fail = []() {
        fprintf(stderr, "future_plan_check: %s\n", mdp_last_error());
        return 1;
    };
    const uint32_t n = (uint32_t)strlen(argv[1]);
    std::vector<int32_t> row(n);
    for (uint32_t k = 0; k < n; ++k) row[k] = argv[1][k] == 'm' ? -1 : argv[1][k] - '0';
    const double m = atof(argv[2]), d = atof(argv[3]), KD = atof(argv[4]), KS = atof(argv[5]), dS = atof(argv[6]);
    FutWideMode mode;
    uint32_t np = 0, sum_years = 0;
    if (fut_parse_opts(argv[7], &mode, &sum_years)) return fail();
    if (fut_select_kernel(n, mode, &np)) return fail();
    // the summary path's plan (argv[8] years), after everything else
    auto summary = [&](uint32_t wlen) {
        if (argc != 9) return 0;
        FutSumPlan sp;
        if (fut_sum_plan(n, np, wlen, (uint32_t)strtoul(argv[8], nullptr, 10), sum_years, &sp)) return 1;
        printf("summary cells %u years %u windows %u lds %u grid %u reps %llu\n", sp.cells, sp.years, sp.windows, sp.lds,
               sp.maxwg, (unsigned long long)sp.reps);
        // every LDS cell of a year of k_future_wide lands on its own global cell
        std::vector<char> hit(2 * (size_t)n + 1, 0);
        for (uint32_t c = 0; np && c < sp.cells; ++c) {
            const int32_t g = fut_sum_wide_cell(n, c);
            if (g < 0) continue;
            if ((uint32_t)g > 2 * n || hit[g]) {
                fprintf(stderr, "future_plan_check: LDS cell %u maps to global cell %d\n", c, g);
                return 2;
            }
            hit[g] = 1;
        }
        for (size_t g = 0; np && g < hit.size(); ++g)
            if (!hit[g]) {
                fprintf(stderr, "future_plan_check: global cell %zu has no LDS cell\n", g);
                return 2;
            }
        return 0;
    };
    if (np == 0) {
        FutLanePlan lp;
        if (fut_lane_plan(row.data(), n, m, d, KD, KS, dS, &lp)) return fail();
        printf("kernel k_future<%u>\n", lp.nm);
        printf("lane nmiss %u occ0 %llx miss %016llx MK %016llx src %016llx\n", lp.nmiss, (unsigned long long)lp.occ0,
               (unsigned long long)fnv(lp.miss.data(), lp.miss.size() * sizeof(uint64_t)),
               (unsigned long long)fnv(lp.MK.data(), lp.MK.size() * sizeof(double)),
               (unsigned long long)fnv(lp.src.data(), lp.src.size() * sizeof(double)));
        if (const int rc = summary(0)) return rc == 1 ? fail() : 1;
        return 0;
    }
    FutWidePlan p;
    if (fut_wide_plan(row.data(), n, np, m, d, KD, KS, dS, &p)) return fail();
    printf("kernel k_future_wide<%u>\n", np);
    printf("n %u len %u nmiss %u\n", p.n, p.len, p.nmiss);
    printf("occ0");
    for (uint32_t v : p.occ0) printf(" %x", v);
    printf("\nmiss");
    for (uint32_t v : p.miss) printf(" %x", v);
    printf("\nimage %016llx src %016llx\n", (unsigned long long)fnv(p.image.data(), p.image.size() * sizeof(double)),
           (unsigned long long)fnv(p.src.data(), p.src.size() * sizeof(double)));
    // every slot a lane reads for every survivor l: inside the image, and
    // the bits of the lane kernels' table entry exp(-a*|l-k|*d)*K_D
    const double a = 1.0 / m;
    for (uint32_t l = 0; l < n; ++l) {
        const uint32_t s0 = fut_wide_slot0(n, p.len, l);
        for (uint32_t pair = 0; pair < 64 * np; ++pair) {
            const size_t at = 2 * ((size_t)pair + s0);
            if (at + 1 >= p.image.size()) {
                fprintf(stderr, "future_plan_check: slot of pair %u, survivor %u outside the image\n", pair, l);
                return 1;
            }
            for (uint32_t q = 0; q < 2; ++q) {
                const uint32_t k = 2 * pair + q;
                if (k >= n) continue;
                const double want = k == l ? 0.0 : exp(-a * (k > l ? k - l : l - k) * d) * KD;
                if (memcmp(&want, &p.image[at + q], sizeof want)) {
                    fprintf(stderr, "future_plan_check: image entry of M[%u][%u] differs\n", l, k);
                    return 1;
                }
            }
        }
    }
    // layout round trip: the completion with every missing patch occupied,
    // through the lane words and back
    std::vector<uint32_t> lanes(p.occ0);
    for (uint32_t v : p.miss) lanes[v >> 8] |= 1u << (v & 0xffu);
    const uint32_t W = (n + 63) / 64;
    std::vector<uint64_t> words(W, ~0ull);
    fut_wide_unpack(lanes.data(), 1, n, np, words.data());
    for (uint32_t k = 0; k < W * 64; ++k) {
        const bool got = (words[k >> 6] >> (k & 63u)) & 1u, want = k < n && row[k] != 0;
        if (got != want) {
            fprintf(stderr, "future_plan_check: patch %u does not survive the layout round trip\n", k);
            return 1;
        }
    }
    printf("states");
    for (uint64_t w : words) printf(" %llx", (unsigned long long)w);
    printf("\ncheck ok\n");
    if (const int rc = summary(p.len)) return rc == 1 ? fail() : 1;
    return 0;
}
