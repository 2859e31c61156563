// A plain C++ host program for the index checks of msl_cull_keyframes / msl_cull_recent (manhattanslam_amd/csrc/msl_index_check.h, the
// observation table with obs_idx through csr_ok included, as the entry calls it): every array is heap-allocated at exactly
// its size, so a read past an end is the address sanitizer's to find; valid random arrays must pass, each single defect must be refused
// with a message that names the field, and a count outside its capacity must be refused before any entry behind it is read.
// Prints "<n> failures".
#include "msl_index_check.h"

#include <stdlib.h>
#include <string.h>

#include <random>

using namespace msl::check;

namespace {

int failures = 0;
char err[256];

void expect(bool got, bool want, const char *field, const char *what) {
    const bool named = want || strstr(err, field) != nullptr;
    if (got != want || !named) { printf("FAIL %s: returned %d, message '%s'\n", what, (int)got, err); failures++; }
    err[0] = 0;
}

int below(std::mt19937 &g, int n) { return (int)(g() % (unsigned)n); }

}  // namespace

int main() {
    std::mt19937 g(17);
    for (int round = 0; round < 60; round++) {
        const int n_items = 1 + below(g, 4), n_tab = 2 + below(g, 40), ccap = 1 + below(g, n_tab), cap = 1 + below(g, 12), n_pts = 1 + below(g, 30);
        // the candidate rows: distinct keyframes, the slots beyond the count never read
        std::vector<int32_t> cand((size_t)n_items * ccap), n_cand((size_t)n_items);
        for (int f = 0; f < n_items; f++) {
            std::vector<int32_t> all((size_t)n_tab);
            for (int k = 0; k < n_tab; k++) all[(size_t)k] = k;
            for (int k = n_tab - 1; k > 0; k--) std::swap(all[(size_t)k], all[(size_t)below(g, k + 1)]);
            n_cand[(size_t)f] = round % 3 == 0 ? ccap : below(g, ccap + 1);
            for (int r = 0; r < ccap; r++) cand[(size_t)f * ccap + r] = r < n_cand[(size_t)f] ? all[(size_t)r] : 1 << 30;
        }
        auto cand_ok_ = [&] { return kf_rows_ok("cand", "n_cand", "ccap", n_items, n_tab, ccap, cand.data(), n_cand.data(), err, sizeof(err)); };
        expect(cand_ok_(), true, "", "valid candidate rows (a keyframe may be in the rows of two items)");
        const int f = below(g, n_items);
        const int32_t keep_n = n_cand[(size_t)f];
        n_cand[(size_t)f] = ccap + 1; expect(cand_ok_(), false, "n_cand[", "count above ccap");   // the last item's row ends the array
        n_cand[(size_t)f] = -1; expect(cand_ok_(), false, "n_cand[", "count below 0");
        n_cand[(size_t)f] = keep_n;
        if (keep_n > 0) {
            int32_t &e = cand[(size_t)f * ccap + below(g, keep_n)];
            const int32_t keep = e;
            e = n_tab; expect(cand_ok_(), false, "cand[", "entry == n_tab");
            e = -1; expect(cand_ok_(), false, "cand[", "entry -1 inside the row");
            e = keep;
        }
        if (keep_n > 1) {
            int32_t &e = cand[(size_t)f * ccap + keep_n - 1];
            const int32_t keep = e;
            e = cand[(size_t)f * ccap]; expect(cand_ok_(), false, "twice", "repeated candidate");
            e = keep;
        }
        // the origin
        expect(origin_ok(n_tab, -1, err, sizeof(err)), true, "", "no origin");
        expect(origin_ok(n_tab, below(g, n_tab), err, sizeof(err)), true, "", "origin inside the table");
        expect(origin_ok(n_tab, n_tab, err, sizeof(err)), false, "origin", "origin == n_tab");
        expect(origin_ok(n_tab, -2, err, sizeof(err)), false, "origin", "origin -2");
        // the observation table with obs_idx, which msl_cull_keyframes reads
        std::vector<int32_t> n_kps((size_t)n_tab), off((size_t)n_pts + 1, 0);
        for (int k = 0; k < n_tab; k++) n_kps[(size_t)k] = below(g, cap + 1);
        n_kps[(size_t)below(g, n_tab)] = cap;                                     // at least one keyframe can be observed
        std::vector<int32_t> okf, oidx;
        for (int p = 0; p < n_pts; p++) {
            for (int o = below(g, 5); o > 0; o--) {
                const int k = below(g, n_tab);
                if (n_kps[(size_t)k] == 0) continue;
                okf.push_back(k); oidx.push_back(below(g, n_kps[(size_t)k]));
            }
            off[(size_t)p + 1] = (int32_t)okf.size();
        }
        const int n_obs = (int)okf.size();
        auto csr_ok_ = [&] { return csr_ok(n_tab, cap, n_pts, n_obs, off.data(), okf.data(), oidx.data(), n_kps.data(), err, sizeof(err)); };
        expect(csr_ok_(), true, "", "valid observation table");
        if (n_obs > 0) {
            const int o = below(g, n_obs);
            const int32_t keep_i = oidx[(size_t)o], keep_k = okf[(size_t)o];
            oidx[(size_t)o] = n_kps[(size_t)keep_k]; expect(csr_ok_(), false, "obs_idx[", "obs_idx == n_kps");
            oidx[(size_t)o] = -1; expect(csr_ok_(), false, "obs_idx[", "obs_idx -1");
            oidx[(size_t)o] = keep_i;
            okf[(size_t)o] = n_tab; expect(csr_ok_(), false, "obs_kf[", "obs_kf == n_tab");   // refused before n_kps[n_tab] is read
            okf[(size_t)o] = keep_k;
        }
        // the recent elements
        const int n = 1 + below(g, 40);
        std::vector<int32_t> found((size_t)n), visible((size_t)n), first((size_t)n);
        std::vector<uint8_t> flags((size_t)n);
        for (int i = 0; i < n; i++) {
            flags[(size_t)i] = (uint8_t)below(g, 4);
            found[(size_t)i] = below(g, 9); first[(size_t)i] = below(g, 100);
            visible[(size_t)i] = flags[(size_t)i] & 1 ? 1 + below(g, 9) : below(g, 3);      // 0 only where the element is bad
        }
        auto recent_ok_ = [&](bool int_form) { return recent_ok(n, int_form, found.data(), visible.data(), first.data(), flags.data(), err, sizeof(err)); };
        expect(recent_ok_(false), true, "", "valid recent elements, float form");
        expect(recent_ok_(true), true, "", "valid recent elements, integer form (visible == 0 of a bad element is never divided by)");
        const int i = below(g, n);
        const int32_t keep_f = found[(size_t)i], keep_v = visible[(size_t)i], keep_id = first[(size_t)i];
        const uint8_t keep_fl = flags[(size_t)i];
        found[(size_t)i] = -1; expect(recent_ok_(false), false, "found[", "found below 0"); found[(size_t)i] = keep_f;
        visible[(size_t)i] = -1; expect(recent_ok_(true), false, "visible[", "visible below 0"); visible[(size_t)i] = keep_v;
        first[(size_t)i] = -1; expect(recent_ok_(false), false, "first_kf_id[", "first_kf_id below 0"); first[(size_t)i] = keep_id;
        flags[(size_t)i] = 1; visible[(size_t)i] = 0;
        expect(recent_ok_(true), false, "visible[", "visible == 0 of a live element in the integer form");
        expect(recent_ok_(false), true, "", "visible == 0 of a live element in the float form");
        flags[(size_t)i] = keep_fl; visible[(size_t)i] = keep_v;
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
