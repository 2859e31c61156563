// A plain C++ host program for the index checks of msl_local_keyframes / msl_local_points / msl_local_lines
// (manhattanslam_amd/csrc/msl_index_check.h): every array is heap-allocated at exactly its size, so a read past an end is the address
// sanitizer's to find; valid random arrays must pass, each single defect must be refused with a message that names the field, and a count
// outside its capacity must be refused before any entry behind it is read.  Prints "<n> failures".
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

// n distinct keyframes of n_tab in random order
std::vector<int32_t> distinct(std::mt19937 &g, int n_tab, int n) {
    std::vector<int32_t> all((size_t)n_tab);
    for (int k = 0; k < n_tab; k++) all[(size_t)k] = k;
    for (int k = n_tab - 1; k > 0; k--) std::swap(all[(size_t)k], all[(size_t)below(g, k + 1)]);
    all.resize((size_t)n);
    return all;
}

}  // namespace

int main() {
    std::mt19937 g(11);
    for (int round = 0; round < 60; round++) {
        const int n_frames = 1 + below(g, 4), cap = 1 + below(g, 20), n_ids = 1 + below(g, 50), n_tab = 2 + below(g, 40), ccap = 1 + below(g, n_tab);
        // the ids the frames hold
        std::vector<int32_t> held((size_t)n_frames * cap), n((size_t)n_frames);
        for (int f = 0; f < n_frames; f++) {
            n[(size_t)f] = round % 7 == 0 ? cap : below(g, cap + 1);
            for (int i = 0; i < cap; i++) held[(size_t)f * cap + i] = i < n[(size_t)f] ? below(g, n_ids + 1) - 1 : 1 << 30;   // beyond the count: not read
        }
        auto held_ok_ = [&] { return held_ok("cur_held", "n_cur", n_frames, cap, n_ids, held.data(), n.data(), err, sizeof(err)); };
        expect(held_ok_(), true, "", "valid held ids");
        const int f = below(g, n_frames);
        if (n[(size_t)f] > 0) {
            int32_t &slot = held[(size_t)f * cap + below(g, n[(size_t)f])];
            const int32_t keep = slot;
            slot = n_ids; expect(held_ok_(), false, "cur_held[", "id == n_ids");
            slot = -2; expect(held_ok_(), false, "cur_held[", "id -2");
            slot = keep;
        }
        const int32_t keep_n = n[(size_t)f];
        n[(size_t)f] = cap + 1; expect(held_ok_(), false, "n_cur[", "count above cap");      // refused before slot cap of the last frame is read
        n[(size_t)f] = -1; expect(held_ok_(), false, "n_cur[", "count below 0");
        n[(size_t)f] = keep_n;
        // the covisibility rows and the parent links
        std::vector<int32_t> conn((size_t)n_tab * ccap), n_conn((size_t)n_tab), parent((size_t)n_tab);
        for (int k = 0; k < n_tab; k++) {
            n_conn[(size_t)k] = round % 5 == 0 ? ccap : below(g, ccap + 1);
            for (int r = 0; r < ccap; r++) conn[(size_t)k * ccap + r] = r < n_conn[(size_t)k] ? below(g, n_tab) : -1;
            parent[(size_t)k] = k == 0 || below(g, 4) == 0 ? -1 : below(g, k);
        }
        auto graph_ok_ = [&] { return graph_ok(n_tab, ccap, conn.data(), n_conn.data(), parent.data(), err, sizeof(err)); };
        expect(graph_ok_(), true, "", "valid graph");
        const int k = below(g, n_tab);
        const int32_t keep_p = parent[(size_t)k], keep_c = n_conn[(size_t)k];
        parent[(size_t)k] = n_tab; expect(graph_ok_(), false, "parent[", "parent == n_tab");
        parent[(size_t)k] = -2; expect(graph_ok_(), false, "parent[", "parent -2");
        parent[(size_t)k] = k; expect(graph_ok_(), false, "parent[", "self-parent");
        parent[(size_t)k] = keep_p;
        n_conn[(size_t)k] = ccap + 1; expect(graph_ok_(), false, "n_conn[", "n_conn above ccap");   // the last keyframe's row ends the array
        n_conn[(size_t)k] = -1; expect(graph_ok_(), false, "n_conn[", "n_conn below 0");
        n_conn[(size_t)k] = keep_c;
        if (keep_c > 0) {
            int32_t &c = conn[(size_t)k * ccap + below(g, keep_c)];
            const int32_t keep = c;
            c = n_tab; expect(graph_ok_(), false, "conn[", "neighbour == n_tab");
            c = -1; expect(graph_ok_(), false, "conn[", "neighbour -1");
            c = keep;
        }
        // a list of local keyframes per frame
        std::vector<int32_t> list((size_t)n_frames * n_tab, -1), n_list((size_t)n_frames);
        for (int q = 0; q < n_frames; q++) {
            n_list[(size_t)q] = round % 3 == 0 ? n_tab : below(g, n_tab + 1);
            const std::vector<int32_t> d = distinct(g, n_tab, n_list[(size_t)q]);
            for (size_t r = 0; r < d.size(); r++) list[(size_t)q * n_tab + r] = d[r];
        }
        auto list_ok_ = [&] { return kf_rows_ok("local_kf", "n_local_kf", "n_tab", n_frames, n_tab, n_tab, list.data(), n_list.data(), err, sizeof(err)); };
        expect(list_ok_(), true, "", "valid lists (a keyframe may be in the lists of two frames)");
        const int32_t keep_l = n_list[(size_t)f];
        n_list[(size_t)f] = n_tab + 1; expect(list_ok_(), false, "n_local_kf[", "length above n_tab");
        n_list[(size_t)f] = -1; expect(list_ok_(), false, "n_local_kf[", "length below 0");
        n_list[(size_t)f] = keep_l;
        if (keep_l > 0) {
            int32_t &e = list[(size_t)f * n_tab + below(g, keep_l)];
            const int32_t keep = e;
            e = n_tab; expect(list_ok_(), false, "local_kf[", "entry == n_tab");
            e = -1; expect(list_ok_(), false, "local_kf[", "entry -1 inside the list");
            e = keep;
        }
        if (keep_l > 1) {
            int32_t &e = list[(size_t)f * n_tab + keep_l - 1];
            const int32_t keep = e;
            e = list[(size_t)f * n_tab]; expect(list_ok_(), false, "twice", "repeated entry");
            e = keep;
        }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
