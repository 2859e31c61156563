// A plain C++ host program for the index checks of msl_plane_clouds / msl_map_plane_merge (manhattanslam_amd/csrc/msl_index_check.h:
// offsets_ok, vertex_indices_ok, merge_into_ok): every array is heap-allocated at exactly its size, so a read past an end is the address
// sanitizer's to find; valid random arrays must pass, each single defect must be refused with a message that names the field, and counts
// outside their capacity are clamped before any row behind them is read.  Prints "<n> failures".
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
        const int F = 1 + below(g, 3), P = 1 + below(g, 6), V = 4 + below(g, 60), mcap = 1 + below(g, 9);
        // detector planes: offsets over the frame's index array, indices inside the cloud
        std::vector<int32_t> off((size_t)F * (P + 1)), idx((size_t)F * V), n((size_t)F), n_map((size_t)F), into((size_t)F * P);
        for (int f = 0; f < F; f++) {
            n[(size_t)f] = round % 4 == 0 ? P + 5 : (round % 4 == 1 ? -2 : below(g, P + 1));       // counts beyond the capacity are clamped
            int o = below(g, 3);
            for (int r = 0; r <= P; r++) { off[(size_t)f * (P + 1) + r] = o; o += below(g, (V - o) / (P - r + 1) + 1); }
            for (int q = 0; q < V; q++) idx[(size_t)f * V + q] = below(g, V);
            n_map[(size_t)f] = round % 5 == 0 ? mcap + 3 : 1 + below(g, mcap);
            const int nm = n_map[(size_t)f] > mcap ? mcap : n_map[(size_t)f];
            for (int k = 0; k < P; k++) into[(size_t)f * P + k] = below(g, nm + 1) - 1;
        }
        auto off_ok = [&] { return offsets_ok("vertex_offsets", "n_planes", F, P, V, off.data(), n.data(), err, sizeof(err)); };
        auto idx_ok = [&] { return vertex_indices_ok(F, P, V, off.data(), idx.data(), n.data(), err, sizeof(err)); };
        auto into_ok = [&] { return merge_into_ok(F, P, mcap, into.data(), n.data(), n_map.data(), err, sizeof(err)); };
        expect(off_ok(), true, "", "valid offsets");
        expect(idx_ok(), true, "", "valid vertex indices");
        expect(into_ok(), true, "", "valid merge_into");
        const int f = below(g, F);
        const int m = n[(size_t)f] < 0 ? 0 : (n[(size_t)f] > P ? P : n[(size_t)f]);
        int32_t *o = off.data() + (size_t)f * (P + 1);
        {
            const int32_t keep = o[0];
            o[0] = -1; expect(off_ok(), false, "vertex_offsets[", "first offset below 0");
            o[0] = keep;
        }
        {
            const int32_t keep = o[m];
            o[m] = V + 1; expect(off_ok(), false, "vertex_offsets[", "last read offset beyond the index array");
            o[m] = keep;
        }
        if (m >= 1 && o[m] > 0) {
            const int32_t keep = o[m - 1];
            o[m - 1] = o[m] + 1; expect(off_ok(), false, "descends", "offsets descend");
            o[m - 1] = keep;
        }
        if (m < P) {                                                               // rows beyond the count are not read
            const int32_t keep = o[P];
            o[P] = -7; expect(off_ok(), true, "", "an offset beyond the count");
            o[P] = keep;
        }
        if (o[m] > o[0]) {
            int32_t &e = idx[(size_t)f * V + o[0] + below(g, o[m] - o[0])];
            const int32_t keep = e;
            e = V; expect(idx_ok(), false, "vertex_indices[", "index == n_vertices");
            e = -1; expect(idx_ok(), false, "vertex_indices[", "index below 0");
            e = keep;
        }
        if (o[m] < V) {                                                            // entries outside every plane are not read
            int32_t &e = idx[(size_t)f * V + o[m]];
            const int32_t keep = e;
            e = 1 << 30; expect(idx_ok(), true, "", "an index behind the last plane");
            e = keep;
        }
        if (m >= 1) {
            const int nm = n_map[(size_t)f] > mcap ? mcap : n_map[(size_t)f];
            int32_t &e = into[(size_t)f * P + below(g, m)];
            const int32_t keep = e;
            e = nm; expect(into_ok(), false, "merge_into[", "row == n_map");
            e = -2; expect(into_ok(), false, "merge_into[", "row below -1");
            e = -1; expect(into_ok(), true, "", "row -1");
            e = keep;
        }
        if (m < P) {
            int32_t &e = into[(size_t)f * P + m];
            const int32_t keep = e;
            e = 1 << 20; expect(into_ok(), true, "", "a row beyond the count");
            e = keep;
        }
    }
    printf("%d failures\n", failures);
    return failures != 0;
}
