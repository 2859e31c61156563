// A plain C++ host program for the index checks of msl_refresh_map_points / msl_covisibility (manhattanslam_amd/csrc/msl_index_check.h):
// every array is heap-allocated at exactly its size, so a read past an end is the address sanitizer's to find; a valid random table must
// pass, and each single defect must be refused with a message that names the field.  Prints "<n> failures".
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

struct Table {
    int n_tab, cap, n_pts, n_obs;
    std::vector<int32_t> off, kf, idx, n_kps, ref, ids;
    bool csr(bool with_idx = true) { return csr_ok(n_tab, cap, n_pts, n_obs, off.data(), kf.data(), with_idx ? idx.data() : nullptr, n_kps.data(), err, sizeof(err)); }
};

Table make(std::mt19937 &g, int n_tab, int cap, int n_pts, int max_obs) {
    Table t;
    t.n_tab = n_tab; t.cap = cap; t.n_pts = n_pts;
    t.n_kps.resize(n_tab);
    for (int k = 0; k < n_tab; k++) t.n_kps[k] = 1 + (int)(g() % (unsigned)cap);
    t.off.assign(1, 0);
    for (int p = 0; p < n_pts; p++) {
        const int n = (int)(g() % (unsigned)(max_obs + 1));
        for (int j = 0; j < n; j++) {
            const int k = (int)(g() % (unsigned)n_tab);
            t.kf.push_back(k); t.idx.push_back((int)(g() % (unsigned)t.n_kps[k]));
        }
        t.off.push_back((int32_t)t.kf.size());
        t.ref.push_back((int)(g() % (unsigned)n_tab));
    }
    t.n_obs = (int)t.kf.size();
    t.kf.shrink_to_fit(); t.idx.shrink_to_fit(); t.off.shrink_to_fit();
    for (int p = 0; p < n_pts; p++) t.ids.push_back(n_pts - 1 - p);
    return t;
}

}  // namespace

int main() {
    std::mt19937 g(7);
    for (int round = 0; round < 50; round++) {
        const int n_tab = 1 + (int)(g() % 40), cap = 1 + (int)(g() % 30), n_pts = 1 + (int)(g() % 200);
        Table t = make(g, n_tab, cap, n_pts, round % 5 == 0 ? 0 : 12);
        expect(t.csr(), true, "", "valid table");
        expect(t.csr(false), true, "", "valid table without obs_idx");
        expect(items_ok("ids", n_pts, n_pts, t.ids.data(), true, err, sizeof(err)), true, "", "valid ids");
        expect(refs_ok(n_tab, n_pts, t.ids.data(), t.ref.data(), err, sizeof(err)), true, "", "valid refs");
        {   // the total
            Table b = t; b.n_obs += 1;
            // obs_kf has n_obs entries only: the check must stop at the mismatch before it reads them
            expect(b.csr(), false, "n_obs_total", "n_obs_total one too large");
        }
        {   // a descending offset
            Table b = t; const int p = (int)(g() % (unsigned)n_pts);
            b.off[p + 1] = b.off[p] - 1;
            expect(b.csr(), false, "obs_off", "descending obs_off");
        }
        {   // a negative start
            Table b = t; b.off[0] = -1;
            expect(b.csr(), false, "obs_off", "negative obs_off[0]");
        }
        if (t.n_obs > 0) {
            const int o = (int)(g() % (unsigned)t.n_obs);
            { Table b = t; b.kf[o] = n_tab; expect(b.csr(), false, "obs_kf", "obs_kf == n_tab"); }
            { Table b = t; b.kf[o] = -1; expect(b.csr(false), false, "obs_kf", "obs_kf == -1"); }
            { Table b = t; b.idx[o] = b.n_kps[b.kf[o]]; expect(b.csr(), false, "obs_idx", "obs_idx == n_kps"); expect(b.csr(false), true, "", "obs_idx not read"); }
            { Table b = t; b.idx[o] = -3; expect(b.csr(), false, "obs_idx", "negative obs_idx"); }
            { Table b = t; b.n_kps[b.kf[o]] = cap + 5; b.idx[o] = cap; expect(b.csr(), false, "obs_idx", "obs_idx == cap under a too large n_kps"); }
        }
        {   // the items
            std::vector<int32_t> ids = t.ids;
            ids[0] = n_pts;
            expect(items_ok("ids", n_pts, n_pts, ids.data(), true, err, sizeof(err)), false, "ids", "id == n_pts");
            ids[0] = -1;
            expect(items_ok("ids", n_pts, n_pts, ids.data(), true, err, sizeof(err)), false, "ids", "id == -1");
            if (n_pts > 1) {
                ids[0] = ids[n_pts - 1];
                expect(items_ok("ids", n_pts, n_pts, ids.data(), true, err, sizeof(err)), false, "twice", "a repeated id");
                expect(items_ok("kf", n_pts, n_pts, ids.data(), false, err, sizeof(err)), true, "", "a repeated kf is allowed");
            }
            std::vector<int32_t> ref = t.ref;
            ref[t.ids[0]] = n_tab;
            expect(refs_ok(n_tab, 1, t.ids.data(), ref.data(), err, sizeof(err)), false, "pt_ref", "pt_ref == n_tab");
            ref[t.ids[0]] = -1;
            expect(refs_ok(n_tab, 1, t.ids.data(), ref.data(), err, sizeof(err)), false, "pt_ref", "pt_ref == -1");
            expect(refs_ok(n_tab, n_pts - 1, t.ids.data() + 1, ref.data(), err, sizeof(err)), true, "", "a bad pt_ref of a point that is not named");
        }
    }
    {   // no observation at all: the index arrays are empty
        Table t; t.n_tab = 1; t.cap = 1; t.n_pts = 3; t.n_obs = 0; t.off.assign(4, 0); t.n_kps.assign(1, 1);
        expect(csr_ok(1, 1, 3, 0, t.off.data(), nullptr, nullptr, t.n_kps.data(), err, sizeof(err)), true, "", "empty table");
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
