// A plain C++ host program for the index checks of msl_observations_apply (manhattanslam_amd/csrc/msl_index_check.h: obs_ascending_ok
// and obs_ops_ok, behind csr_ok as the entry calls them): every array is heap-allocated at exactly its size, so a read past an end is the
// address sanitizer's to find; valid random tables and logs must pass, each single defect must be refused with a message that names the
// field, and an op whose keyframe is outside the table must be refused before n_kps of that keyframe is read.
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
    std::mt19937 g(23);
    for (int round = 0; round < 80; round++) {
        const int n_tab = 2 + below(g, 30), cap = 1 + below(g, 12), n_pts = 1 + below(g, 30);
        std::vector<int32_t> n_kps((size_t)n_tab), off((size_t)n_pts + 1, 0), okf, oidx;
        for (int k = 0; k < n_tab; k++) n_kps[(size_t)k] = 1 + below(g, cap);
        // every range ascending: each keyframe joins with probability 1/3
        for (int p = 0; p < n_pts; p++) {
            for (int k = 0; k < n_tab; k++)
                if (below(g, 3) == 0) { okf.push_back(k); oidx.push_back(below(g, n_kps[(size_t)k])); }
            off[(size_t)p + 1] = (int32_t)okf.size();
        }
        const int n_obs = (int)okf.size();
        auto table_ok = [&] {
            return csr_ok(n_tab, cap, n_pts, n_obs, off.data(), okf.data(), oidx.data(), n_kps.data(), err, sizeof(err)) &&
                   obs_ascending_ok(n_pts, off.data(), okf.data(), err, sizeof(err));
        };
        expect(table_ok(), true, "", "valid ascending table");
        for (int p = 0; p < n_pts; p++)
            if (off[(size_t)p + 1] - off[(size_t)p] >= 2) {
                const int o = off[(size_t)p] + 1 + below(g, off[(size_t)p + 1] - off[(size_t)p] - 1);
                const int32_t keep = okf[(size_t)o], keep_i = oidx[(size_t)o];
                okf[(size_t)o] = okf[(size_t)o - 1]; oidx[(size_t)o] = 0; expect(table_ok(), false, "obs_kf[", "a keyframe twice in a range");
                okf[(size_t)o] = 0; expect(table_ok(), false, "obs_kf[", "a range that descends");
                okf[(size_t)o] = keep; oidx[(size_t)o] = keep_i;
                break;
            }
        // the log: MSL_OBS_KF_ERASE in front, then the other four
        const int n_ops = 1 + below(g, 40), n_kf = round % 4 == 0 ? 0 : below(g, n_ops + 1);
        std::vector<int32_t> ops(4 * (size_t)n_ops);
        int n_add = 0;
        for (int o = 0; o < n_ops; o++) {
            int32_t *r = &ops[4 * (size_t)o];
            r[0] = o < n_kf ? OBS_KF_ERASE : OBS_ADD + below(g, 4);
            r[1] = r[0] == OBS_KF_ERASE ? -7 : below(g, n_pts);                // a field an op does not read may hold anything
            r[2] = r[0] == OBS_REPLACE ? below(g, n_pts) : r[0] == OBS_SET_BAD ? 1 << 30 : below(g, n_tab);
            r[3] = r[0] == OBS_ADD ? below(g, n_kps[(size_t)r[2]]) : -1;
            n_add += r[0] == OBS_ADD;
        }
        int ocap = n_obs + n_add;
        auto ops_ok = [&] { return obs_ops_ok(n_tab, cap, n_pts, n_obs, n_ops, ocap, n_kps.data(), ops.data(), err, sizeof(err)); };
        expect(ops_ok(), true, "", "valid log");
        if (n_add) { ocap--; expect(ops_ok(), false, "ocap", "ocap one below n_obs_total + the ADD ops"); ocap++; }
        const int o = below(g, n_ops);
        int32_t *r = &ops[4 * (size_t)o];
        const int32_t keep[4] = {r[0], r[1], r[2], r[3]};
        char at[32];
        snprintf(at, sizeof(at), "ops[%d].", o);
        r[0] = 0; expect(ops_ok(), false, at, "op code 0");
        r[0] = OBS_KF_ERASE + 1; expect(ops_ok(), false, at, "op code 6");
        r[0] = keep[0];
        if (keep[0] != OBS_KF_ERASE) {
            r[1] = n_pts; expect(ops_ok(), false, at, "a == n_pts");
            r[1] = -1; expect(ops_ok(), false, at, "a -1");
            r[1] = keep[1];
        }
        if (keep[0] != OBS_SET_BAD) {
            r[2] = keep[0] == OBS_REPLACE ? n_pts : n_tab; expect(ops_ok(), false, at, "b == its table's size");   // before n_kps[n_tab] is read
            r[2] = -1; expect(ops_ok(), false, at, "b -1");
            r[2] = keep[2];
        }
        if (keep[0] == OBS_ADD) {
            r[3] = n_kps[(size_t)keep[2]]; expect(ops_ok(), false, at, "c == n_kps");
            r[3] = -1; expect(ops_ok(), false, at, "c -1");
            r[3] = keep[3];
        }
        if (n_kf < n_ops) {                                                    // an MSL_OBS_KF_ERASE behind another op
            int32_t *last = &ops[4 * (size_t)(n_ops - 1)];
            const int32_t keep_op = last[0], keep_b = last[2];
            last[0] = OBS_KF_ERASE; last[2] = 0;
            if (n_ops - 1 > n_kf) expect(ops_ok(), false, "behind another op", "late MSL_OBS_KF_ERASE");
            last[0] = keep_op; last[2] = keep_b;
        }
    }
    {   // one more MSL_OBS_KF_ERASE than the limit
        const int n_ops = OBS_MAX_KF_ERASE + 1;
        std::vector<int32_t> ops(4 * (size_t)n_ops, 0), n_kps(1, 1);
        for (int o = 0; o < n_ops; o++) ops[4 * (size_t)o] = OBS_KF_ERASE;
        expect(obs_ops_ok(1, 1, 1, 0, n_ops - 1, 0, n_kps.data(), ops.data(), err, sizeof(err)), true, "", "256 MSL_OBS_KF_ERASE");
        expect(obs_ops_ok(1, 1, 1, 0, n_ops, 0, n_kps.data(), ops.data(), err, sizeof(err)), false, "MSL_OBS_KF_ERASE number 257", "257 MSL_OBS_KF_ERASE");
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
