// A plain C++ host program for the index and sort checks of msl_keyframe_planes / msl_manhattan_observe
// (manhattanslam_amd/csrc/msl_index_check.h: counts_ok, plane_match_ok, kf_slots_ok, tables_sorted_ok, as the entries call them): every array
// is heap-allocated at exactly its size, so a read past an end is the address sanitizer's to find; valid random arrays must pass, each
// single defect must be refused with a message that names the field, and a count outside its capacity must be refused before any entry
// behind it is read; tables_sorted_ok on its own, as msl_manhattan_detect calls it, clamps such a count and reads no entry beyond the
// capacity.  Prints "<n> failures".
#include "msl_index_check.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <random>
#include <set>

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

// n_frames tables of cap entries of 2 w + 1 ints, n[f] of them sorted by distinct ascending keys over `rows` map rows; the rest is junk
std::vector<int32_t> tables(std::mt19937 &g, int n_frames, int cap, int w, int rows, const std::vector<int32_t> &n) {
    const int st = 2 * w + 1;
    std::vector<int32_t> tab((size_t)n_frames * cap * st, 1 << 30);
    for (int f = 0; f < n_frames; f++) {
        std::set<std::array<int, 3>> keys;
        while ((int)keys.size() < n[(size_t)f]) {
            std::array<int, 3> k = {below(g, rows), below(g, rows), w == 3 ? below(g, rows) : 0};
            std::sort(k.begin(), k.begin() + w);
            keys.insert(k);
        }
        int e = 0;
        for (const auto &k : keys) {
            int32_t *x = tab.data() + ((size_t)f * cap + e++) * st;
            for (int q = 0; q < w; q++) x[q] = k[(size_t)q];
            for (int q = w; q < st; q++) x[q] = below(g, 64);
        }
    }
    return tab;
}

}  // namespace

int main() {
    std::mt19937 g(23);
    for (int round = 0; round < 60; round++) {
        const int n_frames = 1 + below(g, 4), pcap = 1 + below(g, 64), mcap = 1 + below(g, 50), kcap = 1 + below(g, 9);
        // the counts and the held planes: the rows at and beyond n_planes[f] are never read
        std::vector<int32_t> n_planes((size_t)n_frames), n_map((size_t)n_frames), match((size_t)n_frames * pcap * 3);
        for (int f = 0; f < n_frames; f++) {
            n_planes[(size_t)f] = round % 3 == 0 ? pcap : below(g, pcap + 1);
            n_map[(size_t)f] = round % 4 == 0 ? mcap : below(g, mcap + 1);
            for (int k = 0; k < pcap; k++)
                for (int s = 0; s < 3; s++)
                    match[3 * ((size_t)f * pcap + k) + s] = k < n_planes[(size_t)f] ? below(g, n_map[(size_t)f] + 1) - 1 : 1 << 30;
        }
        auto planes_ok_ = [&] { return counts_ok("n_planes", "pcap", n_frames, pcap, n_planes.data(), err, sizeof(err)); };
        auto map_ok_ = [&] { return counts_ok("n_map", "mcap", n_frames, mcap, n_map.data(), err, sizeof(err)); };
        auto match_ok_ = [&](int slots) {
            return planes_ok_() && map_ok_() && plane_match_ok("plane_match", n_frames, pcap, slots, match.data(), n_planes.data(), n_map.data(), err, sizeof(err));
        };
        expect(match_ok_(3), true, "", "valid counts and held planes, three slots");
        expect(match_ok_(1), true, "", "valid counts and held planes, slot 0 alone");
        const int f = below(g, n_frames);
        const int32_t keep_n = n_planes[(size_t)f], keep_m = n_map[(size_t)f];
        n_planes[(size_t)f] = pcap + 1; expect(match_ok_(3), false, "n_planes[", "n_planes above pcap");   // refused before row pcap of the last frame is read
        n_planes[(size_t)f] = -1; expect(match_ok_(3), false, "n_planes[", "n_planes below 0");
        n_planes[(size_t)f] = keep_n;
        n_map[(size_t)f] = mcap + 1; expect(match_ok_(3), false, "n_map[", "n_map above mcap");
        n_map[(size_t)f] = -1; expect(match_ok_(3), false, "n_map[", "n_map below 0");
        n_map[(size_t)f] = keep_m;
        if (keep_n > 0) {
            const int k = below(g, keep_n), s = 1 + below(g, 2);
            int32_t &e = match[3 * ((size_t)f * pcap + k) + s];
            const int32_t keep = e;
            e = keep_m; expect(match_ok_(3), false, "plane_match[", "a parallel / vertical plane == n_map");
            expect(match_ok_(1), true, "", "the same defect where only slot 0 is read");
            e = keep;
            int32_t &e0 = match[3 * ((size_t)f * pcap + k)];
            const int32_t keep0 = e0;
            e0 = -2; expect(match_ok_(1), false, "plane_match[", "a held plane -2");
            e0 = keep_m; expect(match_ok_(3), false, "plane_match[", "a held plane == n_map");
            e0 = keep0;
        }
        // the keyframe of every frame, read out of records of four ints
        std::vector<int32_t> rec((size_t)n_frames * 4);
        for (int q = 0; q < n_frames; q++) { rec[4 * (size_t)q] = below(g, 2); rec[4 * (size_t)q + 1] = below(g, kcap); rec[4 * (size_t)q + 2] = below(g, 1000); rec[4 * (size_t)q + 3] = 0; }
        auto slots_ok_ = [&] { return kf_slots_ok(n_frames, kcap, rec.data() + 1, rec.data() + 2, 4, err, sizeof(err)); };
        expect(slots_ok_(), true, "", "valid keyframe rows");
        const int32_t keep_s = rec[4 * (size_t)f + 1], keep_i = rec[4 * (size_t)f + 2];
        rec[4 * (size_t)f + 1] = kcap; expect(slots_ok_(), false, "kf_slot", "kf_slot == kcap");
        rec[4 * (size_t)f + 1] = -1; expect(slots_ok_(), false, "kf_slot", "kf_slot -1");
        rec[4 * (size_t)f + 1] = keep_s;
        rec[4 * (size_t)f + 2] = -1; expect(slots_ok_(), false, "kf_id", "kf_id below 0");
        rec[4 * (size_t)f + 2] = keep_i;
        // the two Manhattan tables
        for (int w = 2; w <= 3; w++) {
            const int cap = 1 + below(g, 40), st = 2 * w + 1, rows = 12;
            const char *name = w == 3 ? "full_tab" : "part_tab", *count = w == 3 ? "n_full" : "n_part", *limit = w == 3 ? "fcap" : "qcap";
            std::vector<int32_t> n((size_t)n_frames);
            for (int q = 0; q < n_frames; q++) n[(size_t)q] = round % 3 == 1 ? cap : below(g, cap + 1);
            std::vector<int32_t> tab = tables(g, n_frames, cap, w, rows, n);
            auto sorted_ok_ = [&] {
                return counts_ok(count, limit, n_frames, cap, n.data(), err, sizeof(err)) &&
                       tables_sorted_ok(name, n_frames, cap, st, w, tab.data(), n.data(), err, sizeof(err));
            };
            expect(sorted_ok_(), true, "", "valid sorted tables");
            const int32_t keep_c = n[(size_t)f];
            n[(size_t)f] = cap + 1; expect(sorted_ok_(), false, count, "a count above the capacity");
            n[(size_t)f] = -1; expect(sorted_ok_(), false, count, "a count below 0");
            n[(size_t)f] = keep_c;
            if (keep_c > 0) {
                int32_t *x = tab.data() + ((size_t)f * cap + below(g, keep_c)) * st;
                const int32_t a = x[0];
                x[0] = rows + 1; expect(sorted_ok_(), false, name, "a key that descends inside its entry");
                x[0] = a;
            }
            if (keep_c > 1) {
                const int e = 1 + below(g, keep_c - 1);
                int32_t *x = tab.data() + ((size_t)f * cap + e) * st;
                std::vector<int32_t> keep(x, x + st);
                for (int q = 0; q < w; q++) x[q] = x[q - st];
                expect(sorted_ok_(), false, name, "a key twice");
                for (int q = 0; q < st; q++) x[q] = keep[(size_t)q];
                std::vector<int32_t> prev(x - st, x);
                for (int q = 0; q < st; q++) { x[q - st] = keep[(size_t)q]; x[q] = prev[(size_t)q]; }
                expect(sorted_ok_(), false, name, "two entries swapped");
                for (int q = 0; q < st; q++) { x[q - st] = prev[(size_t)q]; x[q] = keep[(size_t)q]; }
                expect(sorted_ok_(), true, "", "the tables restored");
            }
            // msl_manhattan_detect's use: no counts_ok in front; a count outside 0 .. cap is clamped, so no entry at or beyond cap is read
            std::vector<int32_t> all((size_t)n_frames, cap);
            std::vector<int32_t> whole = tables(g, n_frames, cap, w, rows, all);
            auto clamped_ok_ = [&] { return tables_sorted_ok(name, n_frames, cap, st, w, whole.data(), all.data(), err, sizeof(err)); };
            all[(size_t)f] = cap + 3; expect(clamped_ok_(), true, "", "a count above the capacity over cap sorted entries");
            int32_t *last = whole.data() + ((size_t)f * cap + cap - 1) * st;
            const int32_t keep_l = last[0];
            last[0] = rows + 1; expect(clamped_ok_(), false, name, "a defect at entry cap - 1 under a count above the capacity");
            all[(size_t)f] = -2; expect(clamped_ok_(), true, "", "a count below 0: no entry of the frame is read");
            last[0] = keep_l;
        }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
