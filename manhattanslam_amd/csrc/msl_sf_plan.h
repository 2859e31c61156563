// msl_sf_plan.h -- what msl_sf_fuse_ex sends back to the caller's vector, planned from the per-sub-block counts of the call's k_fuse launch
// (internal; plain C++, no HIP and no handle: tests/sf_hostvec_host.cpp builds it with a host compiler).
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace msl {
namespace sf {

struct DownloadPlan {
    struct Run { size_t b0, b1; };   // sub-blocks [b0, b1)
    std::vector<Run> runs;           // the stretches of the vector that hold every touched sub-block, at most 64
    size_t touched = 0;              // surfels deleted + updated
    size_t runSurfels = 0;           // surfels the runs cover
    size_t listLimit = 0;            // the most records the sparse list may carry
    bool tryList = false;            // the sparse {index, record} list is expected to be cheaper than the runs
};

// del / upd: deleted and updated surfels per sub-block of subItems surfels, nblk = ceil(n_local / subItems) entries each.  Sub-blocks with neither
// are byte-identical to the caller's copy and are not sent back: runs of touched sub-blocks travel as one copy each, gaps of up to 4 sub-blocks
// bridged; more than 64 runs collapse into fewer by bridging larger gaps (16, 64, ...).
inline DownloadPlan plan_download(const unsigned *del, const unsigned *upd, size_t nblk, size_t n_local, size_t subItems) {
    DownloadPlan p;
    for (size_t b = 0; b < nblk; b++) p.touched += (size_t)del[b] + upd[b];
    for (size_t gapMax = 4; ; gapMax *= 4) {
        p.runs.clear();
        for (size_t b = 0; b < nblk; b++) {
            if (!(del[b] | upd[b])) continue;
            if (!p.runs.empty() && b - p.runs.back().b1 <= gapMax) p.runs.back().b1 = b + 1;
            else p.runs.push_back({b, b + 1});
        }
        if (p.runs.size() <= 64) break;
    }
    for (const DownloadPlan::Run &r : p.runs) p.runSurfels += std::min(r.b1 * subItems, n_local) - r.b0 * subItems;
    // Two ways back.  Runs of touched sub-blocks copied straight into the caller's vector (~45 GB/s), or -- when few surfels in many sub-blocks
    // changed (a map in no particular order) -- a compact {index, record} list scattered by the CPU (~6 ns per record on top of its 60 bytes).
    p.listLimit = n_local / 8;
    const double costRuns = 56.0 * (double)p.runSurfels / 45e9, costList = (double)p.touched * (60.0 / 45e9 + 6e-9);
    p.tryList = p.touched && p.touched <= p.listLimit && costList < costRuns;
    return p;
}

}  // namespace sf
}  // namespace msl
