// msl_bow.hip -- device vocabulary, batched BoW transform and the two descriptor searches of the reference-keyframe paths, for gfx950.
//
// msl_vocab_create / _load_text    DBoW2::TemplatedVocabulary::loadFromTextFile (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420)
// msl_bow_transform                TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) (:1126-1192, :1217-1255),
//                                  i.e. Frame::ComputeBoW / KeyFrame::ComputeBoW
// msl_match_by_bow                 ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:146-247)
// msl_match_lines_by_descriptor    LSDmatcher::SearchByDescriptor (src/LSDmatcher.cpp:201-234)
//
// Vocabulary on the device: every node's children packed contiguously, in the reference's order (file order), as 32-byte descriptor records
// (plus a node-id table), so one tree level is one coalesced read of <= k records.
//
// Launches, all on the matcher handle's stream:
//   k_bow_descend<G>   one group of G lanes (16 or 32, from the widest node) per (frame, feature).  Lane j scores child j (j + G, ... for a
//                      node wider than G) with the shared popcount and keeps its first minimum; the group's minimum of (dist << 32 | ordinal)
//                      is the reference's pick (the first child holds the initial best, only a strictly smaller distance replaces it).  The
//                      descent stops at a node without children.  Writes word_out / node_out (-1 = stopped) and, for the BowVector, the weight.
//   k_bow_vector       one workgroup per frame, only when the BowVector is wanted: (word << 32 | feature) keys bitonic-sorted in LDS, one
//                      ordered sum per word (feature order: v[id] += w for TF / TF_IDF, the first weight for IDF / BINARY), then the
//                      division by v.size() or the one sequential norm pass in ascending word order, as BowVector::normalize.
//   k_match_bow        one workgroup per pair: both sides' (node << 13 | index) keys sorted in LDS, one wave per node present on the keyframe
//                      side, its keyframe features in ascending order, the frame features of the node over the lanes; best / second best
//                      by a two-minimum wave reduction of (dist << 13 | index); then the rotation histogram and ComputeThreeMaxima.
//   k_match_ldesc      one workgroup per pair: knnMatch(kf, cur, 2) per query as a two-minimum of (dist << 9 | train), the ratio test, and
//                      the "last query wins" overwrite as a maximum.
#include "msl_match_handle.h"
#include "msl_match_math.h"

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace msl;

// The vocabulary: node tables on the device (children packed per parent), plus the header fields.
struct msl_vocab {
    int device = 0;
    int k = 0, L = 0, scoring = 0, weighting = 0, nNodes = 0, nWords = 0, maxChildren = 0;
    DevBuf rec, recNode, child, word, weight;   // [positions][32 B], [positions] node id, [nodes] {start, count}, [nodes] word id, [nodes] weight
};

namespace {

constexpr int MAX_K = 20, MAX_L = 10;
constexpr int IDX_BITS = 13;                       // feature index < MAX_CAP
constexpr int VEC_NT = 1024, BOW_NT = 1024, LD_NT = 256;
constexpr unsigned long long KEY_NONE = ~0ull;

enum { TF_IDF = 0, TF = 1, IDF = 2, BINARY = 3 };             // DBoW2::WeightingType
enum { L1_NORM = 0, L2_NORM = 1, DOT_PRODUCT = 5 };           // DBoW2::ScoringType (CHI_SQUARE, KL, BHATTACHARYYA normalise with L1)

struct VocabDev {
    const uint4 *rec; const int32_t *recNode; const int2 *child; const int32_t *word; const double *weight;
    int nWords;
};

struct BowDev {
    int cap, nidLevel, weighting, scoring;
    VocabDev V;
    const uint8_t *desc; const int32_t *nDesc;
    int32_t *wordOut, *nodeOut;
    double *fw;                                    // [n][cap] weight of the stopped node (BowVector only)
    int32_t *bowWord, *nWordsOut; double *bowValue;
};

struct BowMatchDev {
    int cap;
    float nnRatio; int checkOrientation;
    const uint8_t *kfDesc; const float *kfAngle; const int32_t *kfNode; const uint8_t *kfFlags; const int32_t *nKf;
    const msl_keypoint *curKps; const uint8_t *curDesc; const int32_t *curNode; const int32_t *nCur;
    int32_t *matchOut, *nmatches;
};

struct LdescDev {
    int lcap, klcap;
    const uint8_t *kfLdesc, *kfFlags; const double *kfXyz; const int32_t *nKf;
    const uint8_t *curLdesc; const int32_t *nCur;
    int32_t *matchOut, *nmatches; double *lineXyz; uint8_t *lineHas;
};

// ==== Transform: the descent ===============================================================================================================
template <int G>
__global__ __launch_bounds__(256) void k_bow_descend(BowDev D) {
    constexpr int FPB = 256 / G;
    const int f = blockIdx.y, sub = threadIdx.x % G;
    const int i = blockIdx.x * FPB + threadIdx.x / G;
    if (i >= D.cap) return;                                    // uniform per group
    const size_t fi = (size_t)f * D.cap + i;
    const int n = clampi(D.nDesc[f], 0, D.cap);
    if (i >= n || D.V.nWords == 0) {                           // padding, or an empty() vocabulary: the reference returns before any feature
        if (sub == 0) { D.wordOut[fi] = -1; D.nodeOut[fi] = -1; if (D.fw) D.fw[fi] = 0.0; }
        return;
    }
    uint4 a0, a1;
    load_desc(D.desc + fi * 32, a0, a1);
    int node = 0, level = 0, nid = D.nidLevel <= 0 ? 0 : -1;
    int2 ch = D.V.child[0];
    while (ch.y > 0) {
        ++level;
        unsigned long long best = KEY_NONE;
        for (int j = sub; j < ch.y; j += G) {                  // ascending ordinals per lane: the first minimum is kept by the strict <
            const uint4 *r = D.V.rec + 2 * ((size_t)ch.x + j);
            const unsigned d = (unsigned)hamming256(a0, a1, r[0], r[1]);
            const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)j;
            if (key < best) best = key;
        }
        for (int o = 1; o < G; o <<= 1) { const unsigned long long b = __shfl_xor(best, o, G); best = b < best ? b : best; }
        node = D.V.recNode[(size_t)ch.x + (unsigned)(best & 0xFFFFFFFFu)];
        if (level == D.nidLevel) nid = node;
        ch = D.V.child[node];
    }
    if (nid < 0) nid = node;                                   // the descent stopped above L - levelsup: the reference leaves nid unset
    const double w = D.V.weight[node];
    if (sub == 0) {
        const bool kept = w > 0.0;                             // `if (w > 0)`: a NaN or non-positive weight is a stopped word
        D.wordOut[fi] = kept ? D.V.word[node] : -1;
        D.nodeOut[fi] = kept ? nid : -1;
        if (D.fw) D.fw[fi] = w;
    }
}

// ==== Transform: the BowVector ==============================================================================================================
__global__ __launch_bounds__(VEC_NT) void k_bow_vector(BowDev D) {
    extern __shared__ unsigned long long s_key[];              // [P] (word << 32 | feature), then the per-word values (double)
    __shared__ unsigned s_wave[17];
    __shared__ double s_norm;
    const int f = blockIdx.x, n = clampi(D.nDesc[f], 0, D.cap), P = pow2_at_least(max(D.cap, 2));
    const size_t base = (size_t)f * D.cap;
    for (int i = threadIdx.x; i < P; i += VEC_NT) {
        const int w = i < n ? D.wordOut[base + i] : -1;
        s_key[i] = w >= 0 ? ((unsigned long long)(unsigned)w << 32) | (unsigned)i : KEY_NONE;
    }
    bitonic_sort(s_key, P);
    // each thread owns E consecutive sorted entries; a head starts a word
    const int E = P / VEC_NT > 0 ? P / VEC_NT : 1;
    const int b = threadIdx.x * E;
    unsigned heads = 0;
    for (int e = 0; e < E; e++) {
        const int j = b + e;
        if (j < P && s_key[j] != KEY_NONE && (j == 0 || (s_key[j] >> 32) != (s_key[j - 1] >> 32))) heads++;
    }
    unsigned total;
    unsigned pos = block_excl_scan(heads, s_wave, &total);
    const int nw = (int)total;
    const bool tf = D.weighting == TF || D.weighting == TF_IDF;
    double val[8]; int wid[8]; unsigned at[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        val[e] = 0.0; wid[e] = -1; at[e] = 0;
        const int j = b + e;
        if (e < E && j < P && s_key[j] != KEY_NONE && (j == 0 || (s_key[j] >> 32) != (s_key[j - 1] >> 32))) {
            const unsigned w = (unsigned)(s_key[j] >> 32);
            double v = D.fw[base + (unsigned)(s_key[j] & 0xFFFFFFFFu)];
            if (tf)                                            // BowVector::addWeight in feature order
                for (int q = j + 1; q < P && s_key[q] != KEY_NONE && (unsigned)(s_key[q] >> 32) == w; q++)
                    v += D.fw[base + (unsigned)(s_key[q] & 0xFFFFFFFFu)];
            val[e] = v; wid[e] = (int)w; at[e] = pos++;        // IDF / BINARY: addIfNotExist keeps the first
        }
    }
    __syncthreads();                                           // the keys are read for the last time above
    double *s_val = reinterpret_cast<double *>(s_key);
#pragma unroll
    for (int e = 0; e < 8; e++)
        if (wid[e] >= 0) { s_val[at[e]] = val[e]; D.bowWord[base + at[e]] = wid[e]; }
    __syncthreads();
    const bool must = D.scoring != DOT_PRODUCT;
    if (must) {
        if (threadIdx.x == 0) {                                // BowVector::normalize: one ordered pass
            double norm = 0.0;
            if (D.scoring == L2_NORM) {
                for (int j = 0; j < nw; j++) norm += s_val[j] * s_val[j];
                norm = sqrt(norm);
            } else {
                for (int j = 0; j < nw; j++) norm += fabs(s_val[j]);
            }
            s_norm = norm;
        }
        __syncthreads();
    }
    const double norm = must ? s_norm : 0.0, nd = (double)nw;
    for (int j = threadIdx.x; j < D.cap; j += VEC_NT) {
        if (j < nw) {
            double v = s_val[j];
            if (tf && !must) v /= nd;
            if (must && norm > 0.0) v /= norm;
            D.bowValue[base + j] = v;
        } else {
            D.bowWord[base + j] = -1;
            D.bowValue[base + j] = 0.0;
        }
    }
    if (threadIdx.x == 0) D.nWordsOut[f] = nw;
}

// ==== SearchByBoW(KeyFrame*, Frame&) =======================================================================================================
__global__ __launch_bounds__(BOW_NT) void k_match_bow(BowMatchDev M) {
    extern __shared__ unsigned long long s_dyn[];
    __shared__ int s_hist[ROT_HISTO_LENGTH], s_keep[3], s_nm;
    const int f = blockIdx.x, cap = M.cap, P = pow2_at_least(max(cap, 2));
    unsigned long long *s_kf = s_dyn, *s_cur = s_dyn + P;
    short *s_m = reinterpret_cast<short *>(s_dyn + 2 * P);    // [cap] keyframe index matched to frame feature i, -1 = NULL
    const size_t base = (size_t)f * cap;
    const int nKf = clampi(M.nKf[f], 0, cap), nCur = clampi(M.nCur[f], 0, cap);
    for (int i = threadIdx.x; i < P; i += BOW_NT) {
        const int nk = i < nKf && (M.kfFlags[base + i] & 1) ? M.kfNode[base + i] : -1;   // only keyframe features holding a good map point
        const int nc = i < nCur ? M.curNode[base + i] : -1;
        s_kf[i] = nk >= 0 ? ((unsigned long long)(unsigned)nk << IDX_BITS) | (unsigned)i : KEY_NONE;
        s_cur[i] = nc >= 0 ? ((unsigned long long)(unsigned)nc << IDX_BITS) | (unsigned)i : KEY_NONE;
        if (i < cap) s_m[i] = -1;
    }
    if (threadIdx.x < ROT_HISTO_LENGTH) s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_nm = 0;
    bitonic_sort(s_kf, P);
    bitonic_sort(s_cur, P);
    const int lane = lane_id(), wave = threadIdx.x >> 6, nWaves = BOW_NT / 64;
    // one wave per keyframe node (the nodes are disjoint in frame features, so they are independent)
    for (int p = wave; p < P; p += nWaves) {
        const unsigned long long kp = s_kf[p];
        if (kp == KEY_NONE || (p > 0 && (s_kf[p - 1] >> IDX_BITS) == (kp >> IDX_BITS))) continue;
        const unsigned long long node = kp >> IDX_BITS;
        int lo = 0, hi = P;                                    // lower_bound of the node in the frame keys
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_cur[mid] < (node << IDX_BITS)) lo = mid + 1; else hi = mid; }
        const int cb = lo;
        int ce = cb;
        while (ce < P && s_cur[ce] != KEY_NONE && (s_cur[ce] >> IDX_BITS) == node) ce++;
        if (ce == cb) continue;
        for (int q = p; q < P && s_kf[q] != KEY_NONE && (s_kf[q] >> IDX_BITS) == node; q++) {
            const int iKF = (int)(s_kf[q] & (MAX_CAP - 1));
            uint4 k0, k1;
            load_desc(M.kfDesc + (base + iKF) * 32, k0, k1);
            unsigned long long m1 = KEY_NONE, m2 = KEY_NONE;
            for (int c = cb + lane; c < ce; c += 64) {         // position c always belongs to lane (c - cb) % 64: s_m of it is this lane's
                const int iF = (int)(s_cur[c] & (MAX_CAP - 1));
                if (s_m[iF] >= 0) continue;                    // matched earlier in this node
                uint4 c0, c1;
                load_desc(M.curDesc + (base + iF) * 32, c0, c1);
                const unsigned d = (unsigned)hamming256(k0, k1, c0, c1);
                two_smallest(((unsigned long long)d << IDX_BITS) | (unsigned)iF, m1, m2);
            }
            two_min(m1, m2, 64);
            // bestDist1 / bestDist2 start at 256, and a distance of 256 never replaces them
            const int d1 = m1 == KEY_NONE ? 256 : (int)(m1 >> IDX_BITS), d2 = m2 == KEY_NONE ? 256 : (int)(m2 >> IDX_BITS);
            if (d1 <= TH_LOW && (float)d1 < M.nnRatio * (float)d2) {
                const int iF = (int)(m1 & (MAX_CAP - 1));
                for (int c = cb + lane; c < ce; c += 64)
                    if ((int)(s_cur[c] & (MAX_CAP - 1)) == iF) s_m[iF] = (short)iKF;
            }
        }
    }
    __syncthreads();
    int nm = 0;
    for (int i = threadIdx.x; i < nCur; i += BOW_NT) nm += s_m[i] >= 0;
    if (nm) atomicAdd(&s_nm, nm);
    __syncthreads();
    if (M.checkOrientation)                                    // rotation histogram, three maxima, NULLing (:199-206, :226-243)
        rotation_cull<BOW_NT>(nCur, s_hist, s_keep,
                              [&](int i) { return s_m[i] >= 0 ? rot_bin(M.kfAngle[base + s_m[i]] - M.curKps[base + i].angle) : -1; },
                              [&](int i) { s_m[i] = -1; atomicSub(&s_nm, 1); });
    for (int i = threadIdx.x; i < cap; i += BOW_NT) M.matchOut[base + i] = i < nCur ? s_m[i] : -1;
    if (threadIdx.x == 0) M.nmatches[f] = s_nm;
}

// ==== LSDmatcher::SearchByDescriptor =======================================================================================================
__global__ __launch_bounds__(LD_NT) void k_match_ldesc(LdescDev L) {
    __shared__ uint4 s_kd[2 * MAX_KLCAP];
    __shared__ int s_best[MAX_KLCAP], s_m[MAX_KLCAP], s_nm;
    const int f = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    const int nKf = clampi(L.nKf[f], 0, L.klcap), nCur = clampi(L.nCur[f], 0, L.lcap);
    const size_t kb = (size_t)f * L.klcap, cb = (size_t)f * L.lcap;
    const bool run = nKf > 0 && nCur >= 2;                     // otherwise the reference reads past a vector's end: defined as no match
    for (int q = threadIdx.x; q < nKf; q += LD_NT) load_desc(L.kfLdesc + (kb + q) * 32, s_kd[2 * q], s_kd[2 * q + 1]);
    for (int t = threadIdx.x; t < MAX_KLCAP; t += LD_NT) { s_best[t] = -1; s_m[t] = -1; }
    if (threadIdx.x == 0) s_nm = 0;
    uint4 c[4][2];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int t = lane + 64 * r;
        if (t < nCur) load_desc(L.curLdesc + (cb + t) * 32, c[r][0], c[r][1]);
        else c[r][0] = c[r][1] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    if (run)
        for (int q = wave; q < nKf; q += LD_NT / 64) {
            const uint4 k0 = s_kd[2 * q], k1 = s_kd[2 * q + 1];
            unsigned m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int t = lane + 64 * r;
                if (t >= nCur) continue;
                two_smallest(((unsigned)hamming256(k0, k1, c[r][0], c[r][1]) << 9) | (unsigned)t, m1, m2);   // lowest train index first on ties
            }
            two_min(m1, m2, 64);
            if (lane == 0) {
                const float d0 = (float)(m1 >> 9), d1 = (float)(m2 >> 9);
                const bool ok = d0 / d1 < (float)(1.0f / 1.5f);    // 0 / 0 is NaN: rejected
                s_best[q] = ok && (L.kfFlags[kb + q] & 1) ? (int)(m1 & 511u) : -1;
            }
        }
    __syncthreads();
    for (int q = threadIdx.x; q < nKf; q += LD_NT)
        if (s_best[q] >= 0) { atomicMax(&s_m[s_best[q]], q); atomicAdd(&s_nm, 1); }   // later queries overwrite; every write counts
    __syncthreads();
    for (int t = threadIdx.x; t < L.lcap; t += LD_NT) {
        const int q = t < nCur ? s_m[t] : -1;
        L.matchOut[cb + t] = q;
        if (L.lineHas && t < nCur) {
            L.lineHas[cb + t] = q >= 0 ? 1 : 0;
            if (q >= 0)
                for (int e = 0; e < 6; e++) L.lineXyz[(cb + t) * 6 + e] = L.kfXyz[(kb + q) * 6 + e];
        }
    }
    if (threadIdx.x == 0) L.nmatches[f] = s_nm;
}

// ==== host side ============================================================================================================================
int vocab_check(const msl_vocab *v, int device, const char *who) {
    if (!v) { set_error("%s: null vocabulary", who); return MSL_ERR_INVALID; }
    if (v->device != device) {
        set_error("%s: the vocabulary lives on device %d, the handle on device %d", who, v->device, device);
        return MSL_ERR_INVALID;
    }
    return MSL_OK;
}

msl_vocab *vocab_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf,
                        const uint8_t *desc32, const double *weight) {
    if (k < 2 || k > MAX_K || L < 1 || L > MAX_L || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3 || n_nodes < 1 ||
        (n_nodes > 1 && (!parent || !is_leaf || !desc32 || !weight))) {
        set_error("msl_vocab_create: invalid argument (2 <= k <= %d, 1 <= L <= %d, scoring 0..5, weighting 0..3, n_nodes >= 1)", MAX_K, MAX_L);
        return nullptr;
    }
    // children per parent in file order; a parent must precede its child (the reference indexes m_nodes[pid] as it grows)
    std::vector<int32_t> count((size_t)n_nodes, 0), start((size_t)n_nodes, 0), word((size_t)n_nodes, 0);
    std::vector<double> w((size_t)n_nodes, 0.0);
    int nWords = 0;
    for (int i = 1; i < n_nodes; i++) {
        if (parent[i] < 0 || parent[i] >= i) { set_error("msl_vocab_create: node %d names parent %d (must be in [0, %d))", i, parent[i], i); return nullptr; }
        count[parent[i]]++;
        w[i] = weight[i];
        if (is_leaf[i]) word[i] = nWords++;
    }
    int maxChildren = 0;
    size_t pos = 0;
    for (int i = 0; i < n_nodes; i++) { start[i] = (int32_t)pos; pos += count[i]; maxChildren = std::max(maxChildren, count[i]); }
    std::vector<uint8_t> rec(32 * std::max<size_t>(pos, 1));
    std::vector<int32_t> recNode(std::max<size_t>(pos, 1)), fill((size_t)n_nodes, 0);
    for (int i = 1; i < n_nodes; i++) {
        const size_t p = (size_t)start[parent[i]] + fill[parent[i]]++;
        memcpy(rec.data() + 32 * p, desc32 + 32 * (size_t)i, 32);
        recNode[p] = i;
    }
    std::vector<int2> child((size_t)n_nodes);
    for (int i = 0; i < n_nodes; i++) child[i] = make_int2(start[i], count[i]);
    if (bind_device(device) != MSL_OK) return nullptr;
    msl_vocab *v = new (std::nothrow) msl_vocab();
    if (!v) { set_error("msl_vocab_create: out of memory"); return nullptr; }
    v->device = device; v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting; v->nNodes = n_nodes; v->nWords = nWords;
    v->maxChildren = maxChildren;
    struct Up { DevBuf &b; const void *src; size_t bytes; };
    const Up ups[5] = {{v->rec, rec.data(), rec.size()}, {v->recNode, recNode.data(), 4 * recNode.size()}, {v->child, child.data(), 8 * child.size()},
                       {v->word, word.data(), 4 * word.size()}, {v->weight, w.data(), 8 * w.size()}};
    for (const Up &u : ups) {
        hipError_t e = u.b.grow(u.bytes, nullptr);
        if (e == hipSuccess) e = hipMemcpy(u.b.p, u.src, u.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("msl_vocab_create: %s", hipGetErrorString(e)); delete v; return nullptr; }
    }
    return v;
}

// One node line: parent isLeaf d0..d31 weight.  Returns false on a malformed line.
bool parse_node(const char *s, int32_t &pid, uint8_t &leaf, uint8_t *d, double &w) {
    char *e = nullptr;
    errno = 0;
    long x = strtol(s, &e, 10);
    if (e == s || errno) return false;
    pid = (int32_t)x; s = e;
    x = strtol(s, &e, 10);
    if (e == s) return false;
    leaf = x > 0 ? 1 : 0; s = e;
    for (int j = 0; j < 32; j++) {
        x = strtol(s, &e, 10);
        if (e == s) return false;
        d[j] = (uint8_t)(unsigned)x; s = e;                     // FORB::fromString: (unsigned char) of the int read
    }
    w = strtod(s, &e);
    return e != s;
}

msl_vocab *vocab_load_text(int device, const char *path) {
    if (!path) { set_error("msl_vocab_load_text: null path"); return nullptr; }
    FILE *fp = fopen(path, "rb");
    if (!fp) { set_error("msl_vocab_load_text: cannot open %s", path); return nullptr; }
    std::string line;
    std::vector<int32_t> parent(1, 0);
    std::vector<uint8_t> leaf(1, 0), desc(32, 0);
    std::vector<double> weight(1, 0.0);
    int k = -1, L = -1, sc = -1, wt = -1;
    bool header = true, bad = false;
    auto take = [&](const std::string &s) {
        if (header) {
            header = false;
            if (sscanf(s.c_str(), "%d %d %d %d", &k, &L, &sc, &wt) != 4) bad = true;
            return;
        }
        if (s.find_first_not_of(" \t\r") == std::string::npos) return;   // blank lines (a trailing newline) are no nodes
        int32_t p; uint8_t lf, d[32]; double w;
        if (!parse_node(s.c_str(), p, lf, d, w)) { bad = true; return; }
        parent.push_back(p); leaf.push_back(lf); desc.insert(desc.end(), d, d + 32); weight.push_back(w);
    };
    int c;
    while (!bad && (c = fgetc(fp)) != EOF) {
        if (c == '\n') { take(line); line.clear(); } else line.push_back((char)c);
    }
    if (!bad && !line.empty()) take(line);
    fclose(fp);
    if (bad || header) { set_error("msl_vocab_load_text: %s is not a DBoW2 text vocabulary", path); return nullptr; }
    if (parent.size() >= (size_t)INT32_MAX) { set_error("msl_vocab_load_text: too many nodes"); return nullptr; }
    return vocab_create(device, k, L, sc, wt, (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data());
}

constexpr const char *WHO_TRANSFORM = "msl_bow_transform", *WHO_BOW = "msl_match_by_bow", *WHO_LDESC = "msl_match_lines_by_descriptor";

// The vocabulary is compared with the handle's device, so it is launch_transform's to test.
int check_transform(const msl_vocab *, int n_frames, int cap, int, const uint8_t *desc, const int32_t *n_desc, msl_mem, int32_t *word_out,
                    int32_t *node_out, int32_t *bow_word, double *bow_value, int32_t *n_words, msl_mem) {
    const char *who = WHO_TRANSFORM;
    if (!none_null(who, {MSL_NAMED(desc), MSL_NAMED(n_desc), MSL_NAMED(word_out), MSL_NAMED(node_out)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_frames", n_frames) || !in_range(who, "cap", cap, 1, MAX_CAP)) return MSL_ERR_INVALID;
    if ((bow_word || bow_value || n_words) && !(bow_word && bow_value && n_words)) {
        set_error("%s: bow_word, bow_value and n_words are given all or none", who);
        return MSL_ERR_INVALID;
    }
    return MSL_OK;
}

int launch_transform(msl_match *h, const msl_vocab *v, int n_frames, int cap, int levelsup, const uint8_t *desc, const int32_t *n_desc, msl_mem mem,
                     int32_t *word_out, int32_t *node_out, int32_t *bow_word, double *bow_value, int32_t *n_words, msl_mem out_mem) {
    const bool vec = bow_word != nullptr;                                   // the three arrays of the vector: all or none
    int rc = vocab_check(v, h->device, WHO_TRANSFORM);
    if (rc != MSL_OK) return rc;
    rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, n = F * cap;
    BowDev D{};
    D.cap = cap; D.weighting = v->weighting; D.scoring = v->scoring;
    D.nidLevel = (int)std::min<long long>((long long)v->L - levelsup, INT_MAX);   // <= 0: the root
    D.V = VocabDev{(const uint4 *)v->rec.p, (const int32_t *)v->recNode.p, (const int2 *)v->child.p, (const int32_t *)v->word.p,
                   (const double *)v->weight.p, v->nWords};
    Stage S(h, mem, out_mem);
    D.desc = S.in(desc, 32 * n); D.nDesc = S.in(n_desc, F);
    D.wordOut = S.out(word_out, n); D.nodeOut = S.out(node_out, n);
    D.bowWord = S.out(bow_word, n); D.bowValue = S.out(bow_value, n); D.nWordsOut = S.out(n_words, F);   // all three or none
    MSL_HIP_TRY(S.error());
    if (vec) {
        MSL_HIP_TRY(h->bowW.grow(8 * n, st));
        D.fw = (double *)h->bowW.p;
        MSL_HIP_TRY(allow_lds(h, LDS_BOW_VECTOR, k_bow_vector, 8 * MAX_CAP));
    }
    if (v->maxChildren <= 16)
        hipLaunchKernelGGL(k_bow_descend<16>, dim3((unsigned)((cap + 15) / 16), (unsigned)n_frames), dim3(256), 0, st, D);
    else
        hipLaunchKernelGGL(k_bow_descend<32>, dim3((unsigned)((cap + 7) / 8), (unsigned)n_frames), dim3(256), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    if (vec) {
        hipLaunchKernelGGL(k_bow_vector, dim3((unsigned)n_frames), dim3(VEC_NT), 8 * (size_t)pow2_at_least(std::max(cap, 2)), st, D);
        MSL_HIP_TRY(hipGetLastError());
    }
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_match_bow(int n_pairs, int cap, const msl_bow_match_params *params, const uint8_t *kf_desc, const float *kf_angle, const int32_t *kf_node,
                    const uint8_t *kf_flags, const int32_t *n_kf, const msl_keypoint *cur_kps, const uint8_t *cur_desc, const int32_t *cur_node,
                    const int32_t *n_cur, msl_mem, int32_t *match_out, int32_t *nmatches, msl_mem) {
    const char *who = WHO_BOW;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kf_desc), MSL_NAMED(kf_angle), MSL_NAMED(kf_node), MSL_NAMED(kf_flags), MSL_NAMED(n_kf),
                         MSL_NAMED(cur_kps), MSL_NAMED(cur_desc), MSL_NAMED(cur_node), MSL_NAMED(n_cur), MSL_NAMED(match_out), MSL_NAMED(nmatches)}))
        return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_pairs", n_pairs) || !in_range(who, "cap", cap, 1, MAX_CAP)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_match_bow(msl_match *h, int n_pairs, int cap, const msl_bow_match_params *prm, const uint8_t *kf_desc, const float *kf_angle,
                     const int32_t *kf_node, const uint8_t *kf_flags, const int32_t *n_kf, const msl_keypoint *cur_kps, const uint8_t *cur_desc,
                     const int32_t *cur_node, const int32_t *n_cur, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_pairs, n = F * cap;
    BowMatchDev M{};
    M.cap = cap; M.nnRatio = prm->nn_ratio; M.checkOrientation = prm->check_orientation;
    Stage S(h, mem, out_mem);
    M.kfDesc = S.in(kf_desc, 32 * n); M.kfAngle = S.in(kf_angle, n); M.kfNode = S.in(kf_node, n); M.kfFlags = S.in(kf_flags, n); M.nKf = S.in(n_kf, F);
    M.curKps = S.in(cur_kps, n); M.curDesc = S.in(cur_desc, 32 * n); M.curNode = S.in(cur_node, n); M.nCur = S.in(n_cur, F);
    M.matchOut = S.out(match_out, n); M.nmatches = S.out(nmatches, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(allow_lds(h, LDS_MATCH_BOW, k_match_bow, 18 * MAX_CAP));
    const size_t P = (size_t)pow2_at_least(std::max(cap, 2));
    hipLaunchKernelGGL(k_match_bow, dim3((unsigned)n_pairs), dim3(BOW_NT), 16 * P + 2 * P, st, M);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

// kf_line_xyz, line_xyz and line_has are optional: the last two together, and then with the first.
int check_match_ldesc(int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc, const uint8_t *kf_line_flags, const double *kf_line_xyz,
                      const int32_t *n_kf_lines, const uint8_t *cur_ldesc, const int32_t *n_cur_lines, msl_mem, int32_t *match_out, int32_t *nmatches,
                      double *line_xyz, uint8_t *line_has, msl_mem) {
    const char *who = WHO_LDESC;
    if (!none_null(who, {MSL_NAMED(kf_ldesc), MSL_NAMED(kf_line_flags), MSL_NAMED(n_kf_lines), MSL_NAMED(cur_ldesc), MSL_NAMED(n_cur_lines),
                         MSL_NAMED(match_out), MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_pairs", n_pairs) || !in_range(who, "lcap", lcap, 1, MAX_KLCAP) || !in_range(who, "klcap", klcap, 1, MAX_KLCAP))
        return MSL_ERR_INVALID;
    if (!line_xyz != !line_has) { set_error("%s: line_xyz and line_has are given together", who); return MSL_ERR_INVALID; }
    if (line_xyz && !none_null(who, {MSL_NAMED(kf_line_xyz)})) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_match_ldesc(msl_match *h, int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc, const uint8_t *kf_line_flags, const double *kf_line_xyz,
                       const int32_t *n_kf_lines, const uint8_t *cur_ldesc, const int32_t *n_cur_lines, msl_mem mem, int32_t *match_out,
                       int32_t *nmatches, double *line_xyz, uint8_t *line_has, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_pairs, nk = F * klcap, nc = F * lcap;
    LdescDev L{};
    L.lcap = lcap; L.klcap = klcap;
    Stage S(h, mem, out_mem);
    L.kfLdesc = S.in(kf_ldesc, 32 * nk); L.kfFlags = S.in(kf_line_flags, nk); L.nKf = S.in(n_kf_lines, F); L.curLdesc = S.in(cur_ldesc, 32 * nc);
    L.nCur = S.in(n_cur_lines, F); L.kfXyz = S.in(kf_line_xyz, 6 * nk);
    L.lineXyz = S.inout(line_xyz, 6 * nc);                     // in/out: a slot without a match keeps its bytes
    L.lineHas = S.out(line_has, nc); L.matchOut = S.out(match_out, nc); L.nmatches = S.out(nmatches, F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_match_ldesc, dim3((unsigned)n_pairs), dim3(LD_NT), 0, st, L);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

msl_vocab *msl_vocab_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf,
                            const uint8_t *desc32, const double *weight) noexcept {
    try {
    return vocab_create(device, k, L, scoring, weighting, n_nodes, parent, is_leaf, desc32, weight);
    } MSL_ABI_CATCH_PTR
}

msl_vocab *msl_vocab_load_text(int device, const char *path) noexcept {
    try {
    return vocab_load_text(device, path);
    } MSL_ABI_CATCH_PTR
}

void msl_vocab_destroy(msl_vocab *v) noexcept {
    try {
    if (!v) return;
    (void)bind_device(v->device);
    delete v;                                    // frees the buffers
    } MSL_ABI_CATCH_VOID
}

int msl_vocab_info(const msl_vocab *v, int32_t info[7]) noexcept {
    try {
    if (!v || !info) { set_error("msl_vocab_info: null argument"); return MSL_ERR_INVALID; }
    info[0] = v->k; info[1] = v->L; info[2] = v->scoring; info[3] = v->weighting; info[4] = v->nNodes; info[5] = v->nWords; info[6] = v->device;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_bow_transform(msl_match *h, const msl_vocab *v, int n_frames, int cap, int levelsup, const uint8_t *desc, const int32_t *n_desc, msl_mem mem,
                      int32_t *word_out, int32_t *node_out, int32_t *bow_word, double *bow_value, int32_t *n_words, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_TRANSFORM, check_transform, launch_transform, h, v, n_frames, cap, levelsup, desc, n_desc, mem, word_out, node_out, bow_word,
                       bow_value, n_words, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_bow_transform_batch(int device, const msl_vocab *v, int n_frames, int cap, int levelsup, const uint8_t *desc, const int32_t *n_desc,
                            msl_mem mem, int32_t *word_out, int32_t *node_out, int32_t *bow_word, double *bow_value, int32_t *n_words,
                            msl_mem out_mem) noexcept {
    try {
    return batch_form(check_transform, launch_transform, device, mem == MSL_MEM_DEVICE, v, n_frames, cap, levelsup, desc, n_desc, mem, word_out, node_out,
                      bow_word, bow_value, n_words, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_by_bow(msl_match *h, int n_pairs, int cap, const msl_bow_match_params *params, const uint8_t *kf_desc, const float *kf_angle,
                     const int32_t *kf_node, const uint8_t *kf_flags, const int32_t *n_kf, const msl_keypoint *cur_kps, const uint8_t *cur_desc,
                     const int32_t *cur_node, const int32_t *n_cur, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_BOW, check_match_bow, launch_match_bow, h, n_pairs, cap, params, kf_desc, kf_angle, kf_node, kf_flags, n_kf, cur_kps, cur_desc,
                       cur_node, n_cur, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_by_bow_batch(int device, int n_pairs, int cap, const msl_bow_match_params *params, const uint8_t *kf_desc, const float *kf_angle,
                           const int32_t *kf_node, const uint8_t *kf_flags, const int32_t *n_kf, const msl_keypoint *cur_kps,
                           const uint8_t *cur_desc, const int32_t *cur_node, const int32_t *n_cur, msl_mem mem, int32_t *match_out,
                           int32_t *nmatches, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_match_bow, launch_match_bow, device, mem == MSL_MEM_DEVICE, n_pairs, cap, params, kf_desc, kf_angle, kf_node, kf_flags, n_kf,
                      cur_kps, cur_desc, cur_node, n_cur, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_lines_by_descriptor(msl_match *h, int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc, const uint8_t *kf_line_flags,
                                  const double *kf_line_xyz, const int32_t *n_kf_lines, const uint8_t *cur_ldesc, const int32_t *n_cur_lines,
                                  msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz, uint8_t *line_has,
                                  msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LDESC, check_match_ldesc, launch_match_ldesc, h, n_pairs, lcap, klcap, kf_ldesc, kf_line_flags, kf_line_xyz, n_kf_lines,
                       cur_ldesc, n_cur_lines, mem, match_out, nmatches, line_xyz, line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_lines_by_descriptor_batch(int device, int n_pairs, int lcap, int klcap, const uint8_t *kf_ldesc, const uint8_t *kf_line_flags,
                                        const double *kf_line_xyz, const int32_t *n_kf_lines, const uint8_t *cur_ldesc,
                                        const int32_t *n_cur_lines, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz,
                                        uint8_t *line_has, msl_mem out_mem) noexcept {
    // line_xyz is in/out: device-memory outputs are read as well
    try {
    return batch_form(check_match_ldesc, launch_match_ldesc, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_pairs, lcap, klcap, kf_ldesc,
                      kf_line_flags, kf_line_xyz, n_kf_lines, cur_ldesc, n_cur_lines, mem, match_out, nmatches, line_xyz, line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"
