// plan_download (manhattanslam_amd/csrc/msl_sf_plan.h: what msl_sf_fuse_ex sends back to the caller's vector) on the host, against a literal
// restatement of the loop msl_sf_fuse_ex carried inline before the planner was extracted.  Built with -fsanitize=address,undefined by
// tests/test_sf_hostvec_host.py; exit status 0 = every case agrees.
#include "msl_sf_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using msl::sf::DownloadPlan;
using msl::sf::plan_download;

namespace {

constexpr size_t SUB = 128;   // SUB_ITEMS of the library

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// the inline planner as it stood: blk holds the deleted counts, then -- blkHalf entries on -- the updated counts
struct Literal { struct Run { size_t b0, b1; }; std::vector<Run> runs; size_t touched = 0, runSurfels = 0, listLimit = 0; bool list = false; };
Literal literal(const unsigned *blk, size_t blkHalf, size_t nblk, size_t n_local) {
    Literal L;
    std::vector<Literal::Run> &runs = L.runs;
    size_t touched = 0, runSurfels = 0;
    for (size_t b = 0; b < nblk; b++) touched += (size_t)blk[b] + blk[blkHalf + b];
    for (size_t gapMax = 4; ; gapMax *= 4) {
        runs.clear();
        for (size_t b = 0; b < nblk; b++) {
            if (!(blk[b] | blk[blkHalf + b])) continue;
            if (!runs.empty() && b - runs.back().b1 <= gapMax) runs.back().b1 = b + 1;
            else runs.push_back({b, b + 1});
        }
        if (runs.size() <= 64) break;
    }
    for (const Literal::Run &r : runs) runSurfels += std::min(r.b1 * SUB, n_local) - r.b0 * SUB;
    const size_t listLimit = n_local / 8;
    const double costRuns = 56.0 * (double)runSurfels / 45e9, costList = (double)touched * (60.0 / 45e9 + 6e-9);
    L.touched = touched; L.runSurfels = runSurfels; L.listLimit = listLimit;
    L.list = touched && touched <= listLimit && costList < costRuns;
    return L;
}

int failures = 0, cases = 0;

// del / upd: nblk counts each.  Returns the plan (already compared with the literal loop).
DownloadPlan check(const char *what, const std::vector<unsigned> &del, const std::vector<unsigned> &upd, size_t n_local) {
    const size_t nblk = (n_local + SUB - 1) / SUB, blkHalf = nblk + 7;   // (the halves lie apart, as in the handle's pinned buffer)
    std::vector<unsigned> blk(2 * blkHalf, 0xDEADu);
    for (size_t b = 0; b < nblk; b++) { blk[b] = del[b]; blk[blkHalf + b] = upd[b]; }
    const Literal L = literal(blk.data(), blkHalf, nblk, n_local);
    // exactly nblk entries each, so that the sanitizer sees any read beyond them
    const std::vector<unsigned> d(del.begin(), del.begin() + nblk), u(upd.begin(), upd.begin() + nblk);
    const DownloadPlan P = plan_download(d.data(), u.data(), nblk, n_local, SUB);
    bool ok = P.touched == L.touched && P.runSurfels == L.runSurfels && P.listLimit == L.listLimit && P.tryList == L.list && P.runs.size() == L.runs.size() &&
              P.runs.size() <= 64;
    for (size_t i = 0; ok && i < P.runs.size(); i++) ok = P.runs[i].b0 == L.runs[i].b0 && P.runs[i].b1 == L.runs[i].b1;
    cases++;
    if (!ok) { failures++; printf("FAIL %s: n_local %zu, %zu runs against %zu, touched %zu / %zu, runSurfels %zu / %zu\n", what, n_local, P.runs.size(), L.runs.size(),
                                  P.touched, L.touched, P.runSurfels, L.runSurfels); }
    return P;
}
void expect(bool cond, const char *what) { if (!cond) { failures++; printf("FAIL %s\n", what); } }

// `count` touched sub-blocks `step` apart from `first` on, in a map of n_local surfels
DownloadPlan isolated(const char *what, size_t n_local, size_t first, size_t step, size_t count) {
    const size_t nblk = (n_local + SUB - 1) / SUB;
    std::vector<unsigned> del(nblk, 0), upd(nblk, 0);
    for (size_t k = 0; k < count; k++) { const size_t b = first + k * step; if (b < nblk) ((k & 1) ? del : upd)[b] = 1 + (unsigned)(k % 3); }
    return check(what, del, upd, n_local);
}

}  // namespace

int main() {
    {   // an empty map
        const DownloadPlan P = check("empty map", {}, {}, 0);
        expect(P.runs.empty() && P.touched == 0 && P.runSurfels == 0 && !P.tryList, "empty map: nothing to send");
    }
    {   // one touched block
        const DownloadPlan P = isolated("one block", 20 * SUB, 7, 1, 1);
        expect(P.runs.size() == 1 && P.runs[0].b0 == 7 && P.runs[0].b1 == 8 && P.runSurfels == SUB, "one block: one run of one sub-block");
    }
    {   // the last block partial, and touched
        const size_t n = 20 * SUB + 37;
        const DownloadPlan P = isolated("partial last block", n, 20, 1, 1);
        expect(P.runs.size() == 1 && P.runs[0].b0 == 20 && P.runs[0].b1 == 21 && P.runSurfels == 37, "partial last block: the run ends with the map");
        const DownloadPlan Q = isolated("partial last block, one surfel", 1, 0, 1, 1);
        expect(Q.runs.size() == 1 && Q.runSurfels == 1, "a map of one surfel");
    }
    {   // touched blocks exactly gapMax and gapMax + 1 apart (gapMax = 4: b - b1 of the run before)
        const DownloadPlan P = isolated("gap of 4", 64 * SUB, 3, 5, 2);    // blocks 3 and 8: 8 - 4 == 4
        expect(P.runs.size() == 1 && P.runs[0].b0 == 3 && P.runs[0].b1 == 9, "a gap of 4 sub-blocks is bridged");
        const DownloadPlan Q = isolated("gap of 5", 64 * SUB, 3, 6, 2);    // blocks 3 and 9: 9 - 4 == 5
        expect(Q.runs.size() == 2 && Q.runs[0].b1 == 4 && Q.runs[1].b0 == 9, "a gap of 5 sub-blocks is not");
    }
    {   // 65 isolated blocks 10 apart: more than 64 runs at gapMax 4, one at 16; 18 apart: 64 is needed
        const DownloadPlan P = isolated("65 isolated", 700 * SUB, 2, 10, 65);
        expect(P.runs.size() == 1 && P.runs[0].b0 == 2 && P.runs[0].b1 == 2 + 64 * 10 + 1, "65 isolated blocks: widened to 16");
        const DownloadPlan Q = isolated("65 isolated, wide", 1300 * SUB, 2, 18, 65);
        expect(Q.runs.size() == 1, "65 isolated blocks 18 apart: widened to 64");
        const DownloadPlan R = isolated("64 isolated", 700 * SUB, 2, 10, 64);
        expect(R.runs.size() == 64, "64 isolated blocks stay 64 runs");
    }
    {   // 300 isolated blocks 20 apart: 16 does not bridge them, 64 does; with a wide hole in the middle two runs are left
        const DownloadPlan P = isolated("300 isolated", 6100 * SUB + 5, 1, 20, 300);
        expect(P.runs.size() == 1 && P.runs.size() <= 64, "300 isolated blocks: widened to 64");
        const size_t n = 9000 * SUB, nblk = 9000;
        std::vector<unsigned> del(nblk, 0), upd(nblk, 0);
        for (size_t k = 0; k < 150; k++) { upd[k * 20] = 1; del[5000 + k * 20] = 2; }
        const DownloadPlan Q = check("300 isolated, two groups", del, upd, n);
        expect(Q.runs.size() == 2 && Q.touched == 450, "two groups of 150 isolated blocks: two runs");
    }
    {   // every block touched
        const size_t n = 333 * SUB + 1, nblk = 334;
        const DownloadPlan P = check("all touched", std::vector<unsigned>(nblk, 100), std::vector<unsigned>(nblk, 0), n);
        expect(P.runs.size() == 1 && P.runSurfels == n && P.touched == 100 * nblk && !P.tryList, "every block touched: the whole vector in one run");
    }
    {   // few surfels in many sub-blocks of a large map: the list is expected to be cheaper
        const DownloadPlan P = isolated("sparse", 4000 * SUB, 0, 3, 1300);
        expect(P.tryList, "sparse changes in a large map: the list is tried");
    }
    for (int t = 0; t < 400; t++) {   // random patterns: density from a few blocks to most, counts up to a whole sub-block
        const size_t n = 1 + rnd() % (t < 200 ? 5000 : 200000), nblk = (n + SUB - 1) / SUB;
        const unsigned dens = 1 + rnd() % 200;
        std::vector<unsigned> del(nblk, 0), upd(nblk, 0);
        for (size_t b = 0; b < nblk; b++) {
            if (rnd() % 200 < dens) del[b] = rnd() % 4 ? 0 : 1 + rnd() % SUB;
            if (rnd() % 200 < dens) upd[b] = rnd() % 4 ? 0 : 1 + rnd() % SUB;
        }
        check("random", del, upd, n);
    }
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
