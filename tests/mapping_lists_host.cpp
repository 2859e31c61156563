// A plain C++ host program for the item checks of msl_fuse_map_points / msl_fuse_map_lines (lists_ok), msl_triangulate_new_points
// (neighbours_ok) and msl_fuse_candidates (targets_ok) in manhattanslam_amd/csrc/msl_index_check.h: every array is heap-allocated at exactly
// its size, so a read past an end is the address sanitizer's to find; a valid set must pass, and each single defect must be refused with
// exactly the message the library has always given behind its "<entry point>: ".  Prints "<n> failures".
#include "msl_index_check.h"

#include <string.h>

using namespace msl::check;

namespace {

int failures = 0;
char err[256];

// want: the whole message of a refusal, or null for an accepted set
void expect(bool got, const char *want, const char *what) {
    if (got != (want == nullptr) || (want && strcmp(err, want) != 0)) { printf("FAIL %s: returned %d, message '%s'\n", what, (int)got, err); failures++; }
    err[0] = 0;
}

typedef std::vector<int32_t> V;

// 2 keyframes, a table of 3 rows, 2 lists of at most 3, 2 items
bool lists(const char *noun, const V &tgt, const V &list, const V &cand, const V &n_cand) {
    return lists_ok(noun, 2, 3, 2, 2, 3, tgt.data(), list.data(), cand.data(), n_cand.data(), err, sizeof(err));
}

// 3 keyframes, at most 2 neighbours, 2 items
bool neighbours(const V &cur, const V &neigh, const V &n_neigh) {
    return neighbours_ok(3, 2, 2, cur.data(), neigh.data(), n_neigh.data(), err, sizeof(err));
}

// 3 keyframes, at most 2 targets, 2 items
bool targets(const V &tg, const V &n_targets) { return targets_ok(3, 2, 2, tg.data(), n_targets.data(), err, sizeof(err)); }

}  // namespace

int main() {
    const V tgt{0, 1}, list{1, 0}, cand{0, 1, 2, 2, 0, -1}, n_cand{3, 2};
    expect(lists("point", tgt, list, cand, n_cand), nullptr, "valid lists");
    expect(lists("point", tgt, list, {-1, 1, -1, -1, -1, -1}, {3, 3}), nullptr, "-1 repeated within a list");
    expect(lists("point", tgt, list, {1, 0, 2, 1, 2, 0}, {3, 3}), nullptr, "one id in two lists");
    expect(lists("point", tgt, list, {1, 0, 1, 2, 0, -1}, n_cand), "list 0 holds point 1 twice (pass -1 for a later duplicate)", "one id twice in a list");
    expect(lists("line", tgt, list, {1, 0, 1, 2, 0, -1}, n_cand), "list 0 holds line 1 twice (pass -1 for a later duplicate)", "one line twice in a list");
    expect(lists("point", tgt, list, {0, 1, 2, 2, 0, 3}, {3, 3}), "list 1 entry 2 is point 3 of 3", "id == n");
    expect(lists("line", tgt, list, {0, -2, 2, 2, 0, -1}, n_cand), "list 0 entry 1 is line -2 of 3", "id == -2");
    // the last list's length is wrong and its row is not there at all: it must be refused before any entry of it is read
    expect(lists("point", tgt, list, {0, 1, 2}, {3, 4}), "list 1 has n_cand 4 outside 0 .. 3", "n_cand == lcap + 1");
    expect(lists("point", tgt, list, {0, 1, 2}, {3, -1}), "list 1 has n_cand -1 outside 0 .. 3", "n_cand == -1");
    expect(lists("point", {0, 2}, list, cand, n_cand), "item 1 names keyframe 2 of 2 or list 0 of 2", "tgt == n_tab");
    expect(lists("point", {-1, 1}, list, cand, n_cand), "item 0 names keyframe -1 of 2 or list 1 of 2", "tgt == -1");
    expect(lists("line", tgt, {1, 2}, cand, n_cand), "item 1 names keyframe 1 of 2 or list 2 of 2", "list == n_lists");

    const char *tri0 = "item 0 names a keyframe outside the table of 3, repeats a neighbour, lists its current keyframe as a neighbour, or has "
                       "n_neigh outside 0 .. 2";
    const char *tri1 = "item 1 names a keyframe outside the table of 3, repeats a neighbour, lists its current keyframe as a neighbour, or has "
                       "n_neigh outside 0 .. 2";
    expect(neighbours({0, 2}, {1, 2, 0, -7}, {2, 1}), nullptr, "valid neighbours (the entry past n_neigh is not read as one)");
    expect(neighbours({0, 2}, {1, 0, 0, 1}, {2, 2}), tri0, "a neighbour equal to cur");
    expect(neighbours({0, 2}, {1, 2, 1, 1}, {2, 2}), tri1, "a repeated neighbour");
    expect(neighbours({0, 2}, {1, 3, 0, 1}, {2, 2}), tri0, "a neighbour == n_tab");
    expect(neighbours({0, 2}, {1, 2, 0, 1}, {2, 3}), tri1, "n_neigh == ncap + 1");   // entry 2 of item 1 would be past the end
    expect(neighbours({0, -1}, {1, 2, 0, 1}, {2, 2}), tri1, "cur == -1");

    expect(targets({0, 2, 1, -7}, {2, 1}), nullptr, "valid targets");
    expect(targets({0, 2, 1, 0}, {2, 3}), "item 1 names a keyframe outside the table of 3, or has n_targets outside 0 .. 2", "n_targets == tcap + 1");
    expect(targets({0, 3, 1, 0}, {2, 2}), "item 0 names a keyframe outside the table of 3, or has n_targets outside 0 .. 2", "a target == n_tab");
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
