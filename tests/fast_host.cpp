// The integer pieces of k_fast (manhattanslam_amd/csrc/msl_orb_fast.h) on the host, against a literal scalar FAST written here: the packed
// quick test of four adjacent pixels (words assembled from a 7 x 10 neighbourhood the way the kernel assembles them from its tile) and the
// FAST-9/16 score.  Built with -fsanitize=address,undefined by tests/test_fast_host.py; exit status 0 = every case agrees.
#include "msl_orb_fast.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace msl::orb;

namespace {

// ring position k -> (dx, dy), clockwise from three rows down (the order of the kernel's ring[])
const int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
const int RY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

struct Patch { uint8_t p[7][12]; };   // rows y - 3 .. y + 3, columns x0 - 3 .. x0 + 8 of four pixels x0 .. x0 + 3 on row y (two spare bytes: whole words)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// literal: is the pixel a FAST-9 corner at threshold t (nine contiguous ring pixels all brighter than v + t or all darker than v - t)
bool corner9(int v, const int *ring, int t) {
    for (int k = 0; k < 16; k++) {
        bool bright = true, dark = true;
        for (int j = 0; j < 9; j++) { const int r = ring[(k + j) & 15]; bright = bright && r > v + t; dark = dark && r < v - t; }
        if (bright || dark) return true;
    }
    return false;
}
int score_literal(int v, const int *ring) {   // the largest threshold at which the pixel is a corner, -1 = none (a corner at t is one at every t' < t: bisection)
    int lo = -1, hi = 255;   // corner at lo (or lo = -1), none at hi
    while (hi - lo > 1) { const int t = (lo + hi) / 2; if (corner9(v, ring, t)) lo = t; else hi = t; }
    return lo;
}
// literal high-speed test: each of the four even opposite pairs has a member brighter than v + th, or each has one darker than v - th
bool quick_literal(int v, const int *ring, int th) {
    bool bright = true, dark = true;
    for (int k = 0; k < 8; k += 2) {
        const int a = ring[k], b = ring[k + 8];
        bright = bright && (a < v - th || b < v - th);   // d = v - ring > th
        dark = dark && (a > v + th || b > v + th);       // d = v - ring < -th
    }
    return bright || dark;
}

uint32_t word(const uint8_t *b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }

long checked = 0;
int failures = 0;

void check_patch(const Patch &P, int th) {
    // the kernel's reads: aligned words from the tile column of the first centre - 3
    const uint32_t u0 = word(&P.p[0][0]), u1 = word(&P.p[0][4]);
    const uint32_t a0 = word(&P.p[1][0]), a1 = word(&P.p[1][4]), a2 = word(&P.p[1][8]);
    const uint32_t b0 = word(&P.p[3][0]), b1 = word(&P.p[3][4]), b2 = word(&P.p[3][8]);
    const uint32_t d0 = word(&P.p[5][0]), d1 = word(&P.p[5][4]), d2 = word(&P.p[5][8]);
    const uint32_t e0 = word(&P.p[6][0]), e1 = word(&P.p[6][4]);
    const unsigned m4 = fast_quick4(fast_bytes(b0, b1, 3), fast_bytes(e0, e1, 3), fast_bytes(u0, u1, 3), fast_bytes(b1, b2, 2), b0, fast_bytes(d1, d2, 1),
                                    fast_bytes(a0, a1, 1), fast_bytes(a1, a2, 1), fast_bytes(d0, d1, 1), th);
    for (int e = 0; e < 4; e++) {
        const int v = P.p[3][3 + e];
        int ring[16];
        for (int k = 0; k < 16; k++) ring[k] = P.p[3 + RY[k]][3 + e + RX[k]];
        const bool q = quick_literal(v, ring, th), got = (m4 >> e) & 1u;
        const int s = score_literal(v, ring), sg = fast_score16(v, ring);
        checked++;
        bool bad = false;
        if (q != got) { bad = true; std::fprintf(stderr, "quick test: th %d pixel %d: literal %d, packed %d\n", th, e, (int)q, (int)got); }
        if ((sg < -1 ? -1 : sg) != s) { bad = true; std::fprintf(stderr, "score: pixel %d: literal %d, network %d\n", e, s, sg); }
        if (s >= th && !q) { bad = true; std::fprintf(stderr, "a pixel that scores %d fails the quick test at %d\n", s, th); }
        if (bad && failures++ < 5) {
            for (int y = 0; y < 7; y++) { for (int x = 0; x < 12; x++) std::fprintf(stderr, "%4d", P.p[y][x]); std::fprintf(stderr, "\n"); }
        }
    }
}

}  // namespace

int main() {
    const int ths[] = {7, 20, 0, 1, 25, 100, 254, 255};
    Patch P;
    for (int th : ths) {
        // all equal, at several levels (0 / 255 extremes included)
        for (int v : {0, 1, 90, 254, 255}) { std::memset(&P, v, sizeof P); check_patch(P, th); }
        // the ring at exactly v +- th and v +- (th + 1) around every centre (clamped to the byte range), the same for all 16 or for arcs of 8, 9 and 10
        for (int v : {0, 30, 128, 225, 255})
            for (int off : {th, th + 1, -th, -(th + 1), th - 1, -(th - 1)})
                for (int arc : {16, 10, 9, 8})
                    for (int start = 0; start < 16; start++) {
                        std::memset(&P, v, sizeof P);
                        const int other = v + off < 0 ? 0 : v + off > 255 ? 255 : v + off;
                        for (int j = 0; j < arc; j++) { const int k = (start + j) & 15; P.p[3 + RY[k]][3 + RX[k]] = (uint8_t)other; }   // (pixel 0's ring; the other three see a shifted pattern)
                        check_patch(P, th);
                        if (arc == 16 && start > 0) break;
                    }
        // 0 / 255 checkerboards and stripes
        for (int kind = 0; kind < 4; kind++) {
            for (int y = 0; y < 7; y++) for (int x = 0; x < 12; x++) P.p[y][x] = (kind == 0 ? (x + y) & 1 : kind == 1 ? x & 1 : kind == 2 ? y & 1 : ((x >> 1) + (y >> 1)) & 1) ? 255 : 0;
            check_patch(P, th);
        }
        // random: full range, and low contrast around the threshold (differences within about +-(th + 2))
        for (int i = 0; i < 2000; i++) {
            for (int y = 0; y < 7; y++) for (int x = 0; x < 12; x++) P.p[y][x] = (uint8_t)rnd();
            check_patch(P, th);
            const int base = (int)(rnd() % 256), span = 2 * (th > 120 ? 120 : th) + 5;
            for (int y = 0; y < 7; y++) for (int x = 0; x < 12; x++) { int v = base + (int)(rnd() % span) - span / 2; P.p[y][x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
            check_patch(P, th);
            // a few levels only: many exact ties and exact +-th steps
            for (int y = 0; y < 7; y++) for (int x = 0; x < 12; x++) { int v = base + ((int)(rnd() % 3) - 1) * (th + (int)(rnd() % 2)); P.p[y][x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
            check_patch(P, th);
        }
    }
    std::printf("fast_host: %ld pixels checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
