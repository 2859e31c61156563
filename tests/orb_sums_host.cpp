// The integer pieces of k_describe and k_pyramid (manhattanslam_amd/csrc/msl_orb_sums.h) on the host, against literal loops written here.
//   IC_Angle   the double loop over the circular patch (m10 = sum u I, m01 = sum v I for |u| <= umax[|v|]).  The words are handed over the way the
//              kernel's lanes hold them: lane L has the patch words L, L + 64, L + 128, L + 192 (row i / 8, columns 4 (i % 8) - 16 .. + 3 around the
//              keypoint; words >= 248 do not exist and are 0), and the lanes' partial sums are added up.
//   resize     the run of four adjacent pixels of one row (source pairs cut from aligned words of a source image with a pitch that is a multiple of
//              four) against the per-pixel expression  r0[s0] c0 + r0[s1] c1 ..., for every row tap and every run of column taps of the 640 x 480
//              and 641 x 479 pyramids (8 levels, scale 1.2; the tables by cv::resize's rule), on random bytes.
// Built with -fsanitize=address,undefined by tests/test_orb_sums_host.py; exit status 0 = every case agrees.
#include "msl_orb_sums.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace msl::orb;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// circular patch row ends as the extractor computes them (the reference's constructor)
void make_umax(int *umax) {
    const int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
    for (int v = 0; v < 16; v++) umax[v] = 0;
    for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::lrint(std::sqrt(225.0 - v * v));
    for (int v = 15, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
}

long checked = 0;
int failures = 0;

// img: 31 rows of 32 bytes, row v + 15, column u + 16
void check_patch(const uint8_t (&img)[31][32], const int *umax, const char *what) {
    int m10 = 0, m01 = 0;
    for (int v = -15; v <= 15; v++) {
        const int d = umax[v < 0 ? -v : v];
        for (int u = -d; u <= d; u++) { m10 += u * img[v + 15][u + 16]; m01 += v * img[v + 15][u + 16]; }
    }
    const uint64_t nib = ic_pack_umax(umax);
    int g10 = 0, g01 = 0;
    for (int lane = 0; lane < 64; lane++) {
        uint32_t sI = 0, sCI = 0;
        int sVI = 0;
        for (int k = 0; k < 4; k++) {
            const int i = lane + 64 * k;
            uint32_t w = 0;
            if (i < IC_WORDS) std::memcpy(&w, &img[i / 8][4 * (i % 8)], 4);
            ic_add_word(w, i < IC_WORDS ? i : IC_WORDS - 1, nib, sI, sCI, sVI);
        }
        g10 += ic_m10(sI, sCI); g01 += sVI;
    }
    checked++;
    if (g10 != m10 || g01 != m01) {
        if (failures++ < 5) std::fprintf(stderr, "%s: literal m10 %d m01 %d, by words m10 %d m01 %d\n", what, m10, m01, g10, g01);
    }
}

struct Tap { short s0, s1, c0, c1; };
int fl(double v) { int i = (int)v; return i - (i > v); }
int clamp16(long v) { return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }
// cv::resize INTER_LINEAR 8U tables (the rule of the extractor's host plan): x zeroes the fraction at both borders and overrides the last tap, y clamps the indices
void make_taps(int dn, int sn, bool isX, std::vector<Tap> &t) {
    const double scale = 1. / ((double)dn / sn);
    t.resize(dn);
    for (int d = 0; d < dn; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = fl(f);
        f -= s;
        if (isX) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= sn - 1) { f = 0; s = sn - 1; }
            t[d].s0 = (short)s; t[d].s1 = (short)(s + 1 < sn - 1 ? s + 1 : sn - 1);
        } else {
            t[d].s0 = (short)(s < 0 ? 0 : s > sn - 1 ? sn - 1 : s); t[d].s1 = (short)(s + 1 < 0 ? 0 : s + 1 > sn - 1 ? sn - 1 : s + 1);
        }
        t[d].c0 = (short)clamp16(std::lrintf((1.f - f) * 2048)); t[d].c1 = (short)clamp16(std::lrintf(f * 2048));
        if (isX && s + 1 >= sn) { t[d].c0 = 2048; t[d].c1 = 0; }
    }
}

void check_pyramid(int W, int H, int levels, double factor) {
    float scale = 1.0f;
    int sw = W, sh = H;
    for (int l = 1; l < levels; l++) {
        scale = (float)(scale * factor);
        const float inv = 1.0f / scale;
        const int dw = (int)std::lrintf((float)W * inv), dh = (int)std::lrintf((float)H * inv);
        std::vector<Tap> tx, ty;
        make_taps(dw, sw, true, tx); make_taps(dh, sh, false, ty);
        for (const Tap &t : tx)
            if (t.c0 < 0 || t.c1 < 0 || !(t.s1 == t.s0 + 1 || t.c1 == 0)) { if (failures++ < 5) std::fprintf(stderr, "column tap %d %d %d %d breaks the pair rule\n", t.s0, t.s1, t.c0, t.c1); }
        // the source level the way the kernel holds it: rows of a pitch that is a multiple of four, eight spare bytes behind the last
        const int pitch = (sw + 3) & ~3;
        std::vector<uint8_t> src((size_t)pitch * sh + 8);
        for (uint8_t &b : src) b = (uint8_t)rnd();
        auto word = [&](int a) { uint32_t w; std::memcpy(&w, &src[a], 4); return w; };
        for (int dy = 0; dy < dh; dy++)
            for (int dx = 0; dx < dw; dx += 4) {
                uint32_t run = 0;
                for (int k = 0; k < 4 && dx + k < dw; k++) {
                    const Tap &x = tx[dx + k], &y = ty[dy];
                    const int a0 = y.s0 * pitch + x.s0, a1 = y.s1 * pitch + x.s0;
                    const uint32_t cx = (uint32_t)(uint16_t)x.c0 | ((uint32_t)(uint16_t)x.c1 << 16);
                    run |= resize_px(resize_pair(word(a0 & ~3), word((a0 & ~3) + 4), a0 & 3), resize_pair(word(a1 & ~3), word((a1 & ~3) + 4), a0 & 3), cx, y.c0, y.c1) << (8 * k);
                }
                for (int k = 0; k < 4 && dx + k < dw; k++) {
                    const Tap &x = tx[dx + k], &y = ty[dy];
                    const uint8_t *r0 = &src[(size_t)y.s0 * pitch], *r1 = &src[(size_t)y.s1 * pitch];
                    const int h0 = r0[x.s0] * x.c0 + r0[x.s1] * x.c1, h1 = r1[x.s0] * x.c0 + r1[x.s1] * x.c1;
                    int v = (((y.c0 * (h0 >> 4)) >> 16) + ((y.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    v = v < 0 ? 0 : v > 255 ? 255 : v;
                    checked++;
                    if ((int)((run >> (8 * k)) & 255u) != v && failures++ < 5)
                        std::fprintf(stderr, "resize %dx%d level %d pixel (%d, %d): literal %d, run %d\n", W, H, l, dx + k, dy, v, (int)((run >> (8 * k)) & 255u));
                }
            }
        sw = dw; sh = dh;
    }
}

}  // namespace

int main() {
    check_pyramid(640, 480, 8, (double)1.2f);
    check_pyramid(641, 479, 8, (double)1.2f);

    int umax[16];
    make_umax(umax);
    const int want[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    for (int v = 0; v < 16; v++) if (umax[v] != want[v]) { std::fprintf(stderr, "umax[%d] = %d\n", v, umax[v]); failures++; }
    // the weight words against the circle, pixel by pixel
    for (int i = 0; i < IC_WORDS; i++) {
        uint32_t one, col;
        ic_weights(i, ic_pack_umax(umax), one, col);
        for (int e = 0; e < 4; e++) {
            const int v = i / 8 - 15, u = 4 * (i % 8) + e - 16, in = (u < 0 ? -u : u) <= umax[v < 0 ? -v : v];
            checked++;
            if ((int)((one >> (8 * e)) & 255u) != in || (int)((col >> (8 * e)) & 255u) != (in ? u + 16 : 0)) {
                if (failures++ < 5) std::fprintf(stderr, "weights of word %d byte %d: one %08x col %08x\n", i, e, one, col);
            }
        }
    }
    uint8_t img[31][32];
    std::memset(img, 0, sizeof img); check_patch(img, umax, "all 0");
    std::memset(img, 255, sizeof img); check_patch(img, umax, "all 255");
    // 255 inside the circle only / outside only (the bytes outside, column u = -16 included, must not count), halves, single pixels
    for (int kind = 0; kind < 6; kind++) {
        for (int r = 0; r < 31; r++)
            for (int c = 0; c < 32; c++) {
                const int v = r - 15, u = c - 16, in = (u < 0 ? -u : u) <= umax[v < 0 ? -v : v];
                img[r][c] = (uint8_t)(kind == 0 ? (in ? 255 : 0) : kind == 1 ? (in ? 0 : 255) : kind == 2 ? (u > 0 ? 255 : 0) : kind == 3 ? (v < 0 ? 255 : 0)
                                      : kind == 4 ? (u < 0 ? 255 : 1) : ((r + c) & 1 ? 255 : 0));
            }
        check_patch(img, umax, "pattern");
    }
    for (int r = 0; r < 31; r++)
        for (int c = 0; c < 32; c++) { std::memset(img, 0, sizeof img); img[r][c] = 255; check_patch(img, umax, "single pixel"); }
    for (int n = 0; n < 20000; n++) {
        for (int r = 0; r < 31; r++) for (int c = 0; c < 32; c++) img[r][c] = (uint8_t)rnd();
        check_patch(img, umax, "random");
    }
    std::printf("orb_sums_host: %ld cases checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
