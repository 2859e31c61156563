// A plain C++ host program for the index checks of msl_connections_apply and msl_fuse_targets (manhattanslam_amd/csrc/msl_index_check.h:
// weights_ok, conn_rows_ok, parents_ok, conn_ops_ok, with origin_ok and items_ok as the entries call them): every array is heap-allocated
// at exactly its size, so a read past an end is the address sanitizer's to find; valid random graphs and logs must pass, each single
// defect must be refused with a message that names the field, an n_conn above ccap must not take the walk beyond the row of ccap, and a
// zero-row weight array (a null pointer) must not be read.
// Prints "<n> failures".
#include "msl_index_check.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
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
    std::mt19937 g(29);
    for (int round = 0; round < 80; round++) {
        const int n_tab = 1 + below(g, 30), ccap = 1 + below(g, n_tab), n_rows = round % 5 == 0 ? 0 : 1 + below(g, n_tab);
        std::vector<int32_t> cw((size_t)n_tab * n_tab), conn((size_t)n_tab * ccap), n_conn((size_t)n_tab), parent((size_t)n_tab);
        std::vector<int32_t> weight((size_t)n_rows * n_tab);
        for (auto &w : cw) w = below(g, 3) ? 0 : below(g, 50);
        for (auto &w : weight) w = below(g, 2) ? 0 : below(g, 50);
        if (!cw.empty()) cw.back() = 0x7FFFFFFF;
        for (int k = 0; k < n_tab; k++) {
            n_conn[(size_t)k] = below(g, n_tab + 1);                           // the full count: may exceed ccap
            for (int r = 0; r < ccap; r++) conn[(size_t)k * ccap + r] = r < n_conn[(size_t)k] ? below(g, n_tab) : -1;
            parent[(size_t)k] = below(g, n_tab + 1) - 1;
        }
        const int32_t *wp = n_rows ? weight.data() : nullptr;
        auto state_ok = [&] {
            return conn_rows_ok(n_tab, ccap, conn.data(), n_conn.data(), err, sizeof(err)) && parents_ok(n_tab, parent.data(), err, sizeof(err)) &&
                   weights_ok("weight", n_rows, n_tab, wp, err, sizeof(err)) && weights_ok("cw", n_tab, n_tab, cw.data(), err, sizeof(err));
        };
        expect(state_ok(), true, "", "valid graph");
        const int k = below(g, n_tab);
        char at[48];
        int32_t keep = n_conn[(size_t)k];
        snprintf(at, sizeof(at), "n_conn[%d]", k);
        n_conn[(size_t)k] = -1; expect(state_ok(), false, at, "n_conn -1");
        n_conn[(size_t)k] = n_tab + 1; expect(state_ok(), false, at, "n_conn n_tab + 1");
        n_conn[(size_t)k] = n_tab;                                             // every slot of the row is read, and none beyond
        {
            std::vector<int32_t> row(conn.begin() + (size_t)k * ccap, conn.begin() + (size_t)(k + 1) * ccap);
            for (int r = 0; r < ccap; r++) conn[(size_t)k * ccap + r] = below(g, n_tab);
            expect(state_ok(), true, "", "n_conn == n_tab over a row of ccap");
            const int r = below(g, ccap);
            snprintf(at, sizeof(at), "conn[%d][%d]", k, r);
            conn[(size_t)k * ccap + r] = n_tab; expect(state_ok(), false, at, "conn entry == n_tab");
            conn[(size_t)k * ccap + r] = -1; expect(state_ok(), false, at, "conn entry -1 below the count");
            std::copy(row.begin(), row.end(), conn.begin() + (size_t)k * ccap);
        }
        n_conn[(size_t)k] = keep;
        keep = parent[(size_t)k];
        snprintf(at, sizeof(at), "parent[%d]", k);
        parent[(size_t)k] = -2; expect(state_ok(), false, at, "parent -2");
        parent[(size_t)k] = n_tab; expect(state_ok(), false, at, "parent == n_tab");
        parent[(size_t)k] = keep;
        const int j = below(g, n_tab);
        keep = cw[(size_t)k * n_tab + j];
        snprintf(at, sizeof(at), "cw[%d][%d]", k, j);
        cw[(size_t)k * n_tab + j] = -1; expect(state_ok(), false, at, "negative cw");
        cw[(size_t)k * n_tab + j] = keep;
        if (n_rows) {
            const int f = below(g, n_rows);
            keep = weight[(size_t)f * n_tab + j];
            snprintf(at, sizeof(at), "weight[%d][%d]", f, j);
            weight[(size_t)f * n_tab + j] = (int32_t)0x80000000; expect(state_ok(), false, at, "negative weight");
            weight[(size_t)f * n_tab + j] = keep;
        }
        expect(origin_ok(n_tab, -1, err, sizeof(err)) && origin_ok(n_tab, n_tab - 1, err, sizeof(err)), true, "", "origin -1 and n_tab - 1");
        expect(origin_ok(n_tab, n_tab, err, sizeof(err)), false, "origin", "origin == n_tab");
        expect(origin_ok(n_tab, -2, err, sizeof(err)), false, "origin", "origin -2");

        // the log: with no weight row only MSL_CONN_KF_BAD is valid
        const int n_ops = 1 + below(g, 40);
        std::vector<int32_t> ops(4 * (size_t)n_ops);
        for (int o = 0; o < n_ops; o++) {
            int32_t *r = &ops[4 * (size_t)o];
            r[0] = n_rows && below(g, 2) ? CONN_UPDATE : CONN_KF_BAD;
            r[1] = below(g, n_tab);
            r[2] = r[0] == CONN_UPDATE ? below(g, n_rows) : 1 << 30;           // a field an op does not read may hold anything
            r[3] = -7;
        }
        auto ops_ok = [&] { return conn_ops_ok(n_tab, n_rows, n_ops, ops.data(), err, sizeof(err)); };
        expect(ops_ok(), true, "", "valid log");
        const int o = below(g, n_ops);
        int32_t *r = &ops[4 * (size_t)o];
        const int32_t was[3] = {r[0], r[1], r[2]};
        snprintf(at, sizeof(at), "ops[%d].", o);
        r[0] = 0; expect(ops_ok(), false, at, "op code 0");
        r[0] = CONN_KF_BAD + 1; expect(ops_ok(), false, at, "op code 3");
        r[0] = was[0];
        r[1] = n_tab; expect(ops_ok(), false, at, "a == n_tab");
        r[1] = -1; expect(ops_ok(), false, at, "a -1");
        r[1] = was[1];
        r[0] = CONN_UPDATE;
        r[2] = n_rows; expect(ops_ok(), false, at, "b == n_rows");
        r[2] = -1; expect(ops_ok(), false, at, "b -1");
        r[0] = was[0]; r[2] = was[2];

        // the current keyframes of msl_fuse_targets: in the table, repeats allowed
        const int n_items = 1 + below(g, 12);
        std::vector<int32_t> cur((size_t)n_items);
        for (auto &c : cur) c = below(g, n_tab);
        cur.back() = cur.front();
        expect(items_ok("cur", n_tab, n_items, cur.data(), false, err, sizeof(err)), true, "", "valid cur");
        cur[(size_t)below(g, n_items)] = n_tab;
        expect(items_ok("cur", n_tab, n_items, cur.data(), false, err, sizeof(err)), false, "cur[", "cur == n_tab");
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
