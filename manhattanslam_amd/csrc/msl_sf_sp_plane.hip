// msl_sf_sp_plane.hip -- superpixel stage for gfx950 (MI355X): the plane fit that ends the stage, and what the map stage reads of a keyframe
// (stage overview: msl_sf_superpixel.hip).
//     kb_seed_plane<STRADDLE>             16 lanes per seed: back-projection, pixel normals, Huber plane fit with FP64 4x4 normal
//                                         equations; the tex words of the seed's cell         (reference src/SurfelFusion.cpp:91-165, :597-773)
//     kb_seed_finish                      one thread per seed: plane normalisation, FuseRec, the candidate surfel (:744-773, :291-329)
//     kb_tex_strips                       the tex words outside the whole cells (sizes that are not multiples of 8)
//     k_debug_group_sums                  test hook of the transposed FP64 group sums

#include "msl_sf_sp_dev.h"

namespace {

// kb_seed_plane: calculateNorms (:775-803) fused per seed, 16 lanes per seed, 4 seeds per wave/workgroup.
// Pixel positions and cross-product normals are recomputed from depth instead of materialising spaceMap
// (7.4 MB f64) / normMap.  Also prepares the surfel the seed would spawn (initializeSurfels, :285-331).
__device__ __forceinline__ void pixel_normal(const SfDev &P, int row, int col, float myX, float myY, float myZ, float rightDepth,
                                             float downDepth, float cxr, float cx1, float ryr, float ry1,
                                             float &nX, float &nY, float &nZ) {
    nX = nY = nZ = 0.0f;
    if (row < 1 || row > P.H - 2 || col < 1 || col > P.W - 2) return;  // never written (:620-625)
    // back_project of the right / down neighbours with the tabulated quotients: (col+1, row) and (col, row+1)
    float rightX = cx1 * rightDepth, rightY = ryr * rightDepth, rightZ = rightDepth;
    float downX = cxr * downDepth, downY = ry1 * downDepth, downZ = downDepth;
    if (myZ < DEPTH_01_F || rightZ < DEPTH_01_F || downZ < DEPTH_01_F) return;   // `< 0.1` (:628): float form, see msl_sf_sp_dev.h
    rightX = rightX - myX; rightY = rightY - myY; rightZ = rightZ - myZ;
    downX = downX - myX; downY = downY - myY; downZ = downZ - myZ;
    float normX = rightY * downZ - rightZ * downY;
    float normY = rightZ * downX - rightX * downZ;
    float normZ = rightX * downY - rightY * downX;
    const float normLength = sqrtf(normX * normX + normY * normY + normZ * normZ);
    normX /= normLength; normY /= normLength; normZ /= normLength;
    const float viewAngle = (normX * myX + normY * myY + normZ * myZ) / sqrtf(myX * myX + myY * myY + myZ * myZ);
    if (viewAngle > -MAX_ANGLE_COS_F && viewAngle < MAX_ANGLE_COS_F) return;
    nX = normX; nY = normY; nZ = normZ;
}

// FuseRec: the 48 bytes of a seed that fuseSurfelsKernel reads (three 16-byte loads instead of the 64-byte msl_seed), with the terms
// that depend on the seed alone evaluated once per seed instead of once per fused surfel -- same expressions, same operands:
//   [0] normX, normY, normZ (camera frame), meanDepth
//   [1] pose * (posX, posY, posZ, 1) (:240-245), getWeight(meanDepth) (:236)
//   [2] size * fabs(meanDepth / (cameraF * viewCos)) (:270-271), meanIntensity, r | g << 8 | b << 16, valid
// valid = !(norm == 0) && !(viewCos < MAX_ANGLE_COS), the two seed tests of :214-219.
//
// LDS: one pool per wave.  The four seeds of a wave form a 2x2 block of the seed lattice, so their 16x16 windows cover
// 24x24 = 576 distinct pixels; every pixel belongs to one seed, hence the four ordered lists hold <= 576 entries in total
// (+ 3 x 3 for 16-byte alignment of each list) instead of 4 x 256.  14 KB per wave: 11 waves per CU instead of 5.
struct PlaneFit { int active; float nx, ny, nz, nb, sumX, sumY, sumZ, maxDist; };   // kb_seed_plane -> kb_seed_finish, in the seed's slot of SfDev::cand
static_assert(sizeof(PlaneFit) <= sizeof(msl_surfel), "the hand-over record fits a candidate slot");
constexpr int PLANE_POOL = 24 * 24 + 12 + 2 * 28;   // + the bank-phase gaps in front of the second list of each half
template <bool STRADDLE>   // STRADDLE: W mod 8 in {1, 2, 3} -- a window quad can stick out over the right edge (instantiated separately: the common
                           // geometry carries none of that code)
__global__ __launch_bounds__(64) void kb_seed_plane(SfDev P, int nSlots) {
    __shared__ __attribute__((aligned(16))) float s_pool[6][PLANE_POOL];   // position x y z, normal x y z
    __shared__ __attribute__((aligned(16))) double s_h[4][16];
    int slot, blk;
    const int bW = (P.spW + 1) / 2, bH = (P.spH + 1) / 2;
    if (!xcd_slot(bW * bH, nSlots, slot, blk)) return;
#ifdef MSL_FUSE_STAMPS   // section cycle counts of the waves of slot 0, summed into delList[64 ..] (tools/fuse_stamps.py)
    unsigned long long sst[14]; int ssn = 0;
#define SECTION_STAMP() sst[ssn++] = __builtin_amdgcn_s_memtime()
#else
#define SECTION_STAMP()
#endif
    SECTION_STAMP();
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15, lane = threadIdx.x;
    const int spX = (blk % bW) * 2 + (g & 1), spY = (blk / bW) * 2 + (g >> 1);
    const bool inRange = spX < P.spW && spY < P.spH;
    const int seedI = inRange ? spY * P.spW + spX : 0;
    const FrameDev F = P.frames[slot];   // by value: one load up front instead of re-reading fields around every store
#ifdef MSL_FUSE_STAMPS
    { unsigned long long a = (unsigned long long)F.depth; asm volatile("" :: "s"(a)); }
    SECTION_STAMP();   // 0a: kernel arguments + frame record
#endif
    const unsigned short *index = P.index + (size_t)slot * P.pxStride;
    // (unconditionally: a group outside the lattice reads seed 0 -- seedI = 0 above -- and never uses or stores it; the zero-filled record the
    // conditional load needed cost 84 select instructions)
    const msl_seed S = P.seeds[(size_t)slot * P.nseeds + seedI];
#ifdef MSL_FUSE_STAMPS
    asm volatile("" :: "v"(S.x), "v"(S.meanDepth));
    SECTION_STAMP();   // 0b: seed record
#endif
    const int xb = spX * SP + SP / 2 - SP, yb = spY * SP + SP / 2 - SP;
    // ---- gather: lane = (row r of a group of four window rows, quad q of four window columns), four iterations; the
    // unclipped window is guarded by the flat index range (:680-684).  16 wide loads per lane: 8 B of index, 16 B of depth,
    // 16 B of the row below, 4 B right of the quad (the other right neighbours are the quad's own elements). ----
    float maxDist = 0;
    int nvalid = 0, base = 0, poolUsed = 0;
    {
        const int rq = l >> 2, cq = l & 3;
        // wrapped pixels (App. B.6) without an integer division: a quad left / right of the image (window columns start at a multiple
        // of 4) belongs to the previous / next row of the flat index.  When W is not a multiple of 4 the last quad of a window in the last
        // lattice column can straddle the right edge: its elements beyond W - 1 are the first pixels of the next row (`straddle`, rare:
        // element-wise loads).
        const int cx0 = xb + 4 * cq;
        const int wrapRow = cx0 < 0 ? -1 : (cx0 >= P.W ? 1 : 0), wcol0 = cx0 - wrapRow * P.W;
        const bool straddle = STRADDLE && cx0 < P.W && cx0 + 3 >= P.W;
        auto elem_wrap = [&](int e) -> int { return (straddle && cx0 + e >= P.W) ? 1 : 0; };   // extra row wrap of element e of a straddling quad
        Quad<unsigned short> idq[4];
        Quad<float> dq[4], ddq[4];
        float dr3[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int wr = yb + 4 * m + rq + wrapRow;
            const int row = min(max(wr, 0), P.H - 1);     // rows outside the image fail the flat-index test below
            if (!straddle) {
                idq[m] = load_quad(byte_off(index, 2u * (unsigned)(row * P.W + wcol0)));
                dq[m] = load_quad(byte_off(F.depthG(), (unsigned)row * P.dsB + 4u * (unsigned)wcol0));
                ddq[m] = load_quad(byte_off(F.depthG(), (unsigned)min(row + 1, P.H - 1) * P.dsB + 4u * (unsigned)wcol0));
                dr3[m] = *byte_off(F.depthG(), (unsigned)row * P.dsB + 4u * (unsigned)min(wcol0 + 4, P.W - 1));
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int we = elem_wrap(e), col = cx0 + e - we * P.W, rowe = min(max(wr + we, 0), P.H - 1);
                    idq[m].v[e] = index[(size_t)rowe * P.W + col];
                    dq[m].v[e] = F.depthG()[(size_t)rowe * P.dstride + col];
                    ddq[m].v[e] = F.depthG()[(size_t)min(rowe + 1, P.H - 1) * P.dstride + col];
                }
                dr3[m] = 0.0f;
            }
        }
        // Texel map for k_fuse: every pixel's {depth, final index} as one 8-byte word.  The seed's own 8x8 cell is rows / columns
        // [4, 12) of its window (iterations 1, 2; column quads 1, 2), and the cells tile the image, so each pixel is written exactly
        // once from values this lane holds anyway: two 16-byte stores per iteration for half of the lanes.
        if (inRange && (cq == 1 || cq == 2)) {
            uint2 *tex = P.tex + (size_t)slot * P.pxStride;
#pragma unroll
            for (int m = 1; m <= 2; m++) {
                uint4 *t4 = reinterpret_cast<uint4 *>(tex + (size_t)(yb + 4 * m + rq) * P.W + cx0);
                t4[0] = make_uint4(__float_as_uint(dq[m].v[0]), idq[m].v[0], __float_as_uint(dq[m].v[1]), idq[m].v[1]);
                t4[1] = make_uint4(__float_as_uint(dq[m].v[2]), idq[m].v[2], __float_as_uint(dq[m].v[3]), idq[m].v[3]);
            }
        }
        unsigned vm = 0;   // bit 4 m + e: pixel e of the quad in iteration m is a valid-depth pixel of the seed
        // Branch-free (sixteen per-lane branches per wave otherwise; one or two waves per SIMD cannot hide their bubbles): the two squares of `dist` are the
        // same products whichever pixel of a column / row they are computed for, so each is evaluated once per column and once per row of the lane's quads.
        float xd2[4], yd2[4];
#pragma unroll
        for (int e = 0; e < 4; e++) { const float xDiff = (xb + 4 * cq + e) - S.x; xd2[e] = xDiff * xDiff; }
#pragma unroll
        for (int m = 0; m < 4; m++) { const float yDiff = (yb + 4 * m + rq) - S.y; yd2[m] = yDiff * yDiff; }
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = xb + 4 * cq + e, jrow = yb + 4 * m + rq;
                const int pixelIndex = jrow * P.W + i;
                const bool own = inRange & (pixelIndex >= 0) & (pixelIndex < P.npx) & (idq[m].v[e] == seedI);   // (`&`: no short-circuit branch around the compare of the loaded index)
                const float dist = xd2[e] + yd2[m];   // xDiff * xDiff + yDiff * yDiff (:680-683)
                maxDist = (own & (dist > maxDist)) ? dist : maxDist;
                vm |= ((own & (dq[m].v[e] >= DEPTH_005_F)) ? 1u : 0u) << (4 * m + e);   // `> 0.05` (:686)
            }
        nvalid = __popc(vm);
        SECTION_STAMP();   // 1a: window loads arrived, ownership tests
        nvalid = row_sum_i32(nvalid);
        {   // list bases inside the pool: multiples of 4 entries (16-byte reads of the sequential sums), and the second list of each 32-lane half
            // 16 banks away from the first one (mod 32) -- the loops below read entry base + l + 16 t with ds_read_b32, whose lane groups are the two
            // halves of the wave and whose bank is the word address mod 32: with arbitrary bases the two seeds of a half collided on every access
            // (round 4: 27 % of the kernel's LDS cycles were bank conflicts)
            const int pad = (nvalid + 3) & ~3;
            const int n0 = __builtin_amdgcn_readlane(pad, 0), n1 = __builtin_amdgcn_readlane(pad, 16), n2 = __builtin_amdgcn_readlane(pad, 32), n3 = __builtin_amdgcn_readlane(pad, 48);
            const int b1 = n0 + ((16 - n0) & 31), b2 = b1 + n1, b3 = b2 + n2 + ((16 - n2) & 31);   // b1 = 16 (mod 32) relative to b0 = 0; b3 likewise to b2
            base = g == 0 ? 0 : g == 1 ? b1 : g == 2 ? b2 : b3;
            poolUsed = b3 + n3;
            // the padding entries behind a list (<= 3 + 28) take part in the wave-wide pass below: give them a valid pixel (row 0, column 0)
            const int padEnd = g == 0 ? b1 : g == 1 ? b2 : g == 2 ? b3 : b3 + n3;
            for (int q = base + nvalid + l; q < padEnd; q += 16) { s_pool[2][q] = 0.0f; s_pool[3][q] = 0.0f; s_pool[4][q] = 0.0f; s_pool[5][q] = 0.0f; }
        }
        int run = base;
#pragma unroll
        for (int m = 0; m < 4; m++) {   // ordered compaction in window raster order = (iteration, lane, element)
            const unsigned q = (vm >> (4 * m)) & 0xFu;
            const int c = __popc(q);
            const int incl = row_incl_scan(c);
            int o = run + incl - c;
            const int rc = ((yb + 4 * m + rq + wrapRow) << 16) | wcol0;   // a valid pixel lies inside the image
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (q & (1u << e)) {   // depth, right depth, down depth, (row, col)
                    float right = e < 3 ? dq[m].v[e < 3 ? e + 1 : 3] : dr3[m];
                    int rce = rc + e;
                    if (straddle) {   // (row, col) and the right neighbour of an element of a straddling quad, fetched here (rare)
                        const int we = elem_wrap(e), col = cx0 + e - we * P.W, rowe = yb + 4 * m + rq + we;
                        rce = (rowe << 16) | col;
                        right = F.depthG()[(size_t)rowe * P.dstride + min(col + 1, P.W - 1)];
                    }
                    s_pool[2][o] = dq[m].v[e]; s_pool[3][o] = right;
                    s_pool[4][o] = ddq[m].v[e]; s_pool[5][o] = __int_as_float(rce);
                    o++;
                }
            run += row_lane_i32<15>(incl);
        }
    }
    SECTION_STAMP();   // 1: gather + ordered lists
    float *const pX = s_pool[0] + base, *const pY = s_pool[1] + base, *const pZ = s_pool[2] + base;
    float *const qX = s_pool[3] + base, *const qY = s_pool[4] + base, *const qZ = s_pool[5] + base;
    maxDist = row_max_f32(maxDist);
    __builtin_amdgcn_wave_barrier();
    // entry e -> position + cross-product normal, written back in place (order preserved).  The work per entry does not depend on the seed, so
    // the 64 lanes walk the whole pool together: ceil(pool / 64) rounds instead of ceil(longest list / 16) -- the four superpixels of a wave
    // rarely have the same size.
    for (int e = lane; e < poolUsed; e += 64) {
        const int rc = __float_as_int(s_pool[5][e]);
        const int row = rc >> 16, col = rc & 0xFFFF;     // a valid pixel lies inside the image: (row, col) of its flat index
        const float myDepth = s_pool[2][e], rightD = s_pool[3][e], downD = s_pool[4][e];
        const float cxr = P.colX[col], cx1 = P.colX[col + 1], ryr = P.rowY[row], ry1 = P.rowY[row + 1];
        const float x = cxr * myDepth, y = ryr * myDepth;   // back_project(col, row, myDepth)
        float nX, nY, nZ;
        pixel_normal(P, row, col, x, y, myDepth, rightD, downD, cxr, cx1, ryr, ry1, nX, nY, nZ);
        s_pool[0][e] = x; s_pool[1][e] = y;
        s_pool[3][e] = nX; s_pool[4][e] = nY; s_pool[5][e] = nZ;
    }
    __builtin_amdgcn_wave_barrier();
    SECTION_STAMP();   // 2: positions + pixel normals
    bool active = inRange && nvalid >= 16;   // validDepthNum < 16 -> continue (:702)
    float meanDepth = S.meanDepth;
    // ---- inliers, kept in order (:707-720).  Count first: when every valid pixel is an inlier (the common case)
    // the list is already in place; otherwise in-place ordered compaction, 16 entries per round. ----
    int ninl = 0;
    {
        int c = 0;
        if (active)
            for (int o = l; o < nvalid; o += 16) {
                const float residual = meanDepth - pZ[o];
                c += in_huber_band(residual) ? 1 : 0;
            }
        ninl = row_sum_i32(c);
    }
    const bool needCompact = active && ninl != nvalid;
    if (__ballot(needCompact)) {
        int w0 = 0;
        for (int t = 0; t < 16; t++) {
            const int o = t * 16 + l;
            bool inl = false;
            float a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
            if (needCompact && o < nvalid) {
                const float residual = meanDepth - pZ[o];
                inl = in_huber_band(residual);
                a0 = pX[o]; a1 = pY[o]; a2 = pZ[o];
                b0 = qX[o]; b1 = qY[o]; b2 = qZ[o];
            }
            const unsigned gm = (unsigned)((__ballot(inl) >> (g * 16)) & 0xFFFFull);
            __builtin_amdgcn_wave_barrier();   // every lane has read its slot before anyone overwrites (w <= o)
            if (inl) {
                const int w = w0 + __popc(gm & ((1u << l) - 1u));
                pX[w] = a0; pY[w] = a1; pZ[w] = a2;
                qX[w] = b0; qY[w] = b1; qZ[w] = b2;
            }
            w0 += __popc(gm);
            __builtin_amdgcn_wave_barrier();
        }
    }
    SECTION_STAMP();   // 3: inlier count / compaction
    if (active && (float)ninl / (float)nvalid < 0.8) active = false;
    // Six strictly sequential f32 sums (inlier normals x,y,z and positions x,y,z, :709-713 and :95-99) run side by side:
    // lane q < 6 of the group walks array q in list order, so the serial latency is one chain instead of six.
    float normX, normY, normZ, sumX, sumY, sumZ;
    {
        float acc = 0.0f;
        if (active && l < 6) acc = seq_sum_f32(s_pool[l < 3 ? 3 + l : l - 3] + base, ninl, 0.0f);
        normX = row_lane_f32<0>(acc); normY = row_lane_f32<1>(acc); normZ = row_lane_f32<2>(acc);
        sumX = row_lane_f32<3>(acc); sumY = row_lane_f32<4>(acc); sumZ = row_lane_f32<5>(acc);
        const float normLength = sqrtf(normX * normX + normY * normY + normZ * normZ);
        normX = normX / normLength; normY = normY / normLength; normZ = normZ / normLength;
        sumX /= ninl; sumY /= ninl; sumZ /= ninl;
    }
    SECTION_STAMP();   // 4: six sequential sums
    // ---- getHuberNorm (:91-165): 5 Gauss-Newton steps, FP64 normal equations reduced over the 16 lanes ----
    float nx = normX, ny = normY, nz = normZ, nb = 0.0f;
    // The Hessian depends only on WHICH points lie inside the Huber band; while that set is unchanged between
    // iterations (the common case: all of them) its sums -- and the inverse -- are bit-identical and are reused.
    unsigned prevMask = 0xFFFFFFFFu;   // impossible mask: forces the first evaluation
    // Cooperative 4x4 inverse: lane l = 4a+b of the group evaluates cofactor (a,b) with exactly the DET3 expression of
    // inverse4(), so lane l ends up holding inv[l] (column-major) -- 1/16 of the work and 2 instead of 32 registers.
    double invl = 0;
    const int ca = l >> 2, cb = l & 3;
    const int r0 = ca == 0 ? 1 : 0, r1 = ca <= 1 ? 2 : 1, r2 = ca <= 2 ? 3 : 2;
    const int c0 = cb == 0 ? 1 : 0, c1 = cb <= 1 ? 2 : 1, c2 = cb <= 2 ? 3 : 2;
    const int tRounds = rows_max_i32(active ? (ninl + 15) >> 4 : 0);   // (ninl and active are uniform inside a group of 16 lanes)
    // The centred points (`points[i] -= sum`, :107-111, once in the reference) of the first RREG rounds stay in registers through the five steps: the
    // loops re-read and re-centred every point from the LDS in every step (three reads and three subtractions per point and step, and an LDS round trip
    // per round that one or two waves per SIMD do not hide); rounds beyond RREG (lists longer than 96 points) still do.
    constexpr int RREG = 6;
    float cpx[RREG], cpy[RREG], cpz[RREG];
#pragma unroll
    for (int t = 0; t < RREG; t++) {
        const int o = l + 16 * t, oc = (active && o < ninl) ? o : 0;
        cpx[t] = cpy[t] = cpz[t] = 0.0f;
        if (t < tRounds) { cpx[t] = pX[oc] - sumX; cpy[t] = pY[oc] - sumY; cpz[t] = pZ[oc] - sumZ; }
    }
    for (int gnI = 0; gnI < 5; gnI++) {
        double J0 = 0, J1 = 0, J2 = 0, J3 = 0;
        unsigned mask = 0;
        // One round of the Jacobian.  Branch-free for the common case (every point inside the Huber band): a lane without a point in this round, or whose
        // point is outside the band, adds +0.0 to its four sums -- exact: a sum that starts at +0.0 never becomes -0.0 -- with the coordinates replaced by
        // zeros BEFORE the products (a NaN / infinite coordinate of a point outside the band must not reach them).  The nested per-lane branches of the
        // literal form cost four taken branches per round, which one or two waves per SIMD cannot hide.  Points outside the band take the reference's two
        // tail cases behind ONE wave-uniform test.
        auto jstep = [&](int t, float px, float py, float pz) {
            const bool has = l + 16 * t < ninl;
            const float residual = px * nx + py * ny + pz * nz + nb;
            const bool inb = has && in_huber_band(residual);
            mask |= (inb ? 1u : 0u) << t;
            const float r2 = inb ? 2 * residual : 0.0f;
            const float qx = inb ? px : 0.0f, qy = inb ? py : 0.0f, qz = inb ? pz : 0.0f;
            J0 += r2 * qx; J1 += r2 * qy; J2 += r2 * qz; J3 += r2;
            if (__builtin_expect(__ballot(has && !inb) != 0ull, 0)) {
                if (has && residual >= HUBER_RANGE_F) {
                    J0 += HUBER_RANGE * px; J1 += HUBER_RANGE * py; J2 += HUBER_RANGE * pz; J3 += HUBER_RANGE;
                } else if (has && residual <= -HUBER_RANGE_F) {
                    J0 += -1 * HUBER_RANGE * px; J1 += -1 * HUBER_RANGE * py; J2 += -1 * HUBER_RANGE * pz; J3 += -1 * HUBER_RANGE;
                }
            }
        };
        if (active) {
#pragma unroll
            for (int t = 0; t < RREG; t++)
                if (t < tRounds) jstep(t, cpx[t], cpy[t], cpz[t]);   // (a wave-uniform bound: the longest inlier list of the four seeds, typically 4-6 of the 16 rounds)
#pragma unroll 1
            for (int t = RREG; t < tRounds; t++) {
                const int o = l + 16 * t, oc = o < ninl ? o : 0;
                jstep(t, pX[oc] - sumX, pY[oc] - sumY, pZ[oc] - sumZ);
            }
        }
        // the four sums over the group's lanes, transposed: lane 4 a + b receives J_a, which is all the update below reads (msl_sf_sp_arith.h)
        const double Jg = sp_group_sum4<RowOpsD>(J0, J1, J2, J3);
        const bool sameSet = mask == prevMask;
        const unsigned diffGroups = (unsigned)((__ballot(!sameSet) >> (g * 16)) & 0xFFFFull);   // uniform per group
        prevMask = mask;
        if (__ballot(diffGroups != 0)) {
            double H00 = 0, H01 = 0, H02 = 0, H03 = 0, H11 = 0, H12 = 0, H13 = 0, H22 = 0, H23 = 0, H33 = 0;
            if (active && diffGroups) {
                auto hstep = [&](int t, float rx, float ry, float rz) {   // (branch-free like the Jacobian: a lane without an in-band point in this round adds zeros)
                    const bool inb = (mask >> t) & 1u;
                    const float px = inb ? rx : 0.0f, py = inb ? ry : 0.0f, pz = inb ? rz : 0.0f;
                    H00 += 2 * px * px; H01 += 2 * px * py; H02 += 2 * px * pz; H03 += 2 * px;
                    H11 += 2 * py * py; H12 += 2 * py * pz; H13 += 2 * py;
                    H22 += 2 * pz * pz; H23 += 2 * pz; H33 += inb ? 2.0 : 0.0;
                };
#pragma unroll
                for (int t = 0; t < RREG; t++)
                    if (t < tRounds) hstep(t, cpx[t], cpy[t], cpz[t]);
#pragma unroll 1
                for (int t = RREG; t < tRounds; t++) {
                    const int oc = ((mask >> t) & 1u) ? l + 16 * t : 0;
                    hstep(t, pX[oc] - sumX, pY[oc] - sumY, pZ[oc] - sumZ);
                }
            }
            // the ten sums, transposed: each total arrives in one bank of the group, whose first lane stores it -- the (symmetric) Hessian + 5 I,
            // column-major (msl_sf_sp_arith.h)
            const SpHessSums<double> hs = sp_group_sum10<RowOpsD>(H00, H01, H02, H03, H11, H12, H13, H22, H23, H33);
            sp_hessian_store(s_h[g], l, hs.c0, hs.c1, hs.c2);
            __builtin_amdgcn_wave_barrier();
            {
                const double *m = s_h[g];
#define M_(r, c) m[(c) * 4 + (r)]
                const double d3 = M_(r0, c0) * (M_(r1, c1) * M_(r2, c2) - M_(r1, c2) * M_(r2, c1)) -
                                  M_(r0, c1) * (M_(r1, c0) * M_(r2, c2) - M_(r1, c2) * M_(r2, c0)) +
                                  M_(r0, c2) * (M_(r1, c0) * M_(r2, c1) - M_(r1, c1) * M_(r2, c0));
                const double cof = ((ca + cb) & 1) ? -d3 : d3;
                const double f0 = dpp_mov_d<0x150>(cof), f1 = dpp_mov_d<0x151>(cof), f2 = dpp_mov_d<0x152>(cof), f3 = dpp_mov_d<0x153>(cof);   // lanes 0..3 of the group
                const double det = ((M_(0, 0) * f0 + M_(0, 1) * f1) + M_(0, 2) * f2) + M_(0, 3) * f3;
#undef M_
                if (diffGroups) invl = cof / det;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // upd[r] = ((inv[0*4+r] J0 + inv[1*4+r] J1) + inv[2*4+r] J2) + inv[3*4+r] J3; lane l holds inv[l], its column is l >> 2
        const double prod = invl * Jg;   // (lane l holds J of its column l >> 2)
        // lanes r = 0..3 of the group (column 0, row r) collect their row: lane r + 4 a holds the term of column a -- row_ror:n hands lane i the value of
        // lane i - n (mod 16), so n = 12, 8, 4 fetch the lanes 4, 8, 12 ahead; the other lanes compute sums nobody reads
        const double q0 = prod, q1 = dpp_mov_d<0x12C>(prod), q2 = dpp_mov_d<0x128>(prod), q3 = dpp_mov_d<0x124>(prod);
        const double updr = ((q0 + q1) + q2) + q3;            // lane r < 4 of the group now holds upd[r]
        const double u0 = dpp_mov_d<0x150>(updr), u1 = dpp_mov_d<0x151>(updr), u2 = dpp_mov_d<0x152>(updr), u3 = dpp_mov_d<0x153>(updr);
        nx = (float)((double)nx - u0); ny = (float)((double)ny - u1); nz = (float)((double)nz - u2); nb = (float)((double)nb - u3);
        SECTION_STAMP();   // 5-9: Gauss-Newton steps
    }
#ifdef MSL_FUSE_STAMPS
    if (slot == 0 && lane == 0) {
        for (int q = 1; q < ssn; q++) atomicAdd(&P.delList[64 + q], (unsigned)(sst[q] - sst[q - 1]));
        atomicAdd(&P.delList[64], 1u);
    }
#endif
    // The per-seed rest -- the plane's normalisation, the seed record, FuseRec and the candidate surfel: ~310 instructions that only ONE lane of a
    // seed's sixteen would execute here (4 of 64 lanes busy) -- runs in kb_seed_finish, one thread per seed.  What it needs of this kernel travels in the
    // seed's slot of the candidate array, which kb_seed_finish itself overwrites afterwards.
    if (!inRange || l != 0) return;
    PlaneFit T;
    T.active = active ? 1 : 0; T.nx = nx; T.ny = ny; T.nz = nz; T.nb = nb; T.sumX = sumX; T.sumY = sumY; T.sumZ = sumZ; T.maxDist = maxDist;
    __builtin_memcpy(reinterpret_cast<char *>(P.cand + ((size_t)slot * P.nseeds + seedI)), &T, sizeof(T));
}

// kb_seed_finish: the end of calculateNorms for one seed (:744-773: plane normalisation, the seed's position on the plane, viewCos, size), then what the
// map stage reads of the seed (FuseRec) and the surfel it would spawn (initializeSurfels, :291-329).  One thread per seed; same expressions, same
// operands as the reference, fed by the fit kb_seed_plane left in the seed's candidate slot.
__global__ __launch_bounds__(256) void kb_seed_finish(SfDev P) {
    const int slot = blockIdx.y;
    const int seedI = blockIdx.x * 256 + threadIdx.x;
    if (seedI >= P.nseeds) return;
    const FrameDev &F = P.frames[slot];
    msl_seed S = P.seeds[(size_t)slot * P.nseeds + seedI];
    PlaneFit T;
    __builtin_memcpy(&T, reinterpret_cast<const char *>(P.cand + ((size_t)slot * P.nseeds + seedI)), sizeof(T));
    const bool active = T.active != 0;
    float nx = T.nx, ny = T.ny, nz = T.nz, nb = T.nb;
    const float sumX = T.sumX, sumY = T.sumY, sumZ = T.sumZ, maxDist = T.maxDist;
    float normX, normY, normZ, meanDepth = S.meanDepth;
    if (active) {
        nb = nb - (nx * sumX + ny * sumY + nz * sumZ);
        {
            const float normLength = sqrtf(nx * nx + ny * ny + nz * nz);
            nx /= normLength; ny /= normLength; nz /= normLength; nb /= normLength;
        }
        normX = nx; normY = ny; normZ = nz;
        const float normB = nb;
        float ax, ay, az;
        back_project(P, S.x, S.y, meanDepth, ax, ay, az);
        double avgX = ax, avgY = ay, avgZ = az;
        {
            const float k = (float)(-1 * (avgX * (double)normX + avgY * (double)normY + avgZ * (double)normZ) - (double)normB);
            avgX += (double)(k * normX); avgY += (double)(k * normY); avgZ += (double)(k * normZ);
            meanDepth = (float)avgZ;
        }
        float viewCos = (float)(-1.0 * ((double)normX * avgX + (double)normY * avgY + (double)normZ * avgZ) / sqrt(avgX * avgX + avgY * avgY + avgZ * avgZ));
        if (viewCos < 0) { viewCos = -viewCos; normX = -normX; normY = -normY; normZ = -normZ; }
        S.normX = normX; S.normY = normY; S.normZ = normZ;
        S.posX = (float)avgX; S.posY = (float)avgY; S.posZ = (float)avgZ;
        S.meanDepth = meanDepth; S.viewCos = viewCos; S.size = sqrtf(maxDist);
        P.seeds[(size_t)slot * P.nseeds + seedI] = S;
    }
    // what the map stage reads of this seed (FuseRec) and the candidate new surfel (:291-329, everything except the `fused` test,
    // which needs the map stage); both use the same per-seed terms
    const bool valid = !(S.viewCos < MAX_ANGLE_COS) && !(S.normX == 0 && S.normY == 0 && S.normZ == 0);
    const bool ok = valid && !(S.meanDepth == 0);
    P.candOk[(size_t)slot * P.flagStride + seedI] = ok ? 1 : 0;
    if (!ok) P.fused[(size_t)slot * P.flagStride + seedI] = 2;   // "spawns nothing" for the deferred map stage's one-array scan (kb_seed_init cleared the byte; a fusion writes 1)
    float pw[4] = {0, 0, 0, 0};
    float seedWeight = 0, seedSize = 0;
    if (valid) {
        mul4(F.pose, S.posX, S.posY, S.posZ, 1.0f, pw);
        const float cameraF = (float)(((double)fabsf(P.fx) + (double)fabsf(P.fy)) / 2.0);
        seedSize = S.size * fabsf(S.meanDepth / (cameraF * S.viewCos));
        seedWeight = get_weight(S.meanDepth);
    }
    {
        float4 *fr = P.fuseRec + (size_t)slot * P.nseeds * 3;
        fr[fuserec_index(P.nseeds, seedI, 0)] = make_float4(S.normX, S.normY, S.normZ, S.meanDepth);
        fr[fuserec_index(P.nseeds, seedI, 1)] = make_float4(pw[0], pw[1], pw[2], seedWeight);
        fr[fuserec_index(P.nseeds, seedI, 2)] = make_float4(seedSize, S.meanIntensity, __uint_as_float(rgb_pack(S.r, S.g, S.b)), __uint_as_float(valid ? 1u : 0u));
    }
    if (ok) {
        float nw[3];
        mul3(F.pose, S.normX, S.normY, S.normZ, nw);
        msl_surfel e;
        e.px = pw[0]; e.py = pw[1]; e.pz = pw[2];
        e.r = S.r; e.g = S.g; e.b = S.b;
        e.nx = nw[0]; e.ny = nw[1]; e.nz = nw[2];
        e.size = seedSize;
        e.color = S.meanIntensity;
        e.weight = seedWeight;
        e.updateTimes = 1;
        e.lastUpdate = F.ref;
        P.cand[(size_t)slot * P.nseeds + seedI] = e;
    }
}

// Image sizes that are not multiples of 8: the strips right of / below the last whole 8x8 cell belong to no cell, so kb_seed_plane does not
// write their texels; this (tiny, rarely launched) kernel does.
__global__ __launch_bounds__(256) void kb_tex_strips(SfDev P) {
    const int slot = blockIdx.y;
    const int wStrip = P.W - P.spW * SP, hStrip = P.H - P.spH * SP;
    const int nRight = wStrip * P.spH * SP, nBottom = P.W * hStrip;   // right strip over the cell rows, bottom strip over the full width
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nRight + nBottom) return;
    int x, y;
    if (i < nRight) { y = i / wStrip; x = P.spW * SP + i % wStrip; }
    else { const int j = i - nRight; y = P.spH * SP + j / P.W; x = j % P.W; }
    const FrameDev F = P.frames[slot];
    const size_t p = (size_t)y * P.W + x;
    P.tex[(size_t)slot * P.pxStride + p] = make_uint2(__float_as_uint(F.depthG()[(size_t)y * P.dstride + x]), P.index[(size_t)slot * P.pxStride + p]);
}

// Test hook of the FP64 group sums: group q (the 16 lanes of row q & 3 of wave q >> 2) holds nvals (4 or 10) values per lane, x[(q nvals + k) 16 + l], and
// reduces them exactly the way kb_seed_plane reduces its Jacobian (4: out[16 q + l] = what lane l holds afterwards, J_(l >> 2)) or its Hessian (10: out[16 q
// ..] = the matrix sp_hessian_store leaves in the LDS, over a NaN fill).  ref[(q nvals + k) 16 + l] = the one-value butterfly of value k in lane l.
__global__ __launch_bounds__(64) void k_debug_group_sums(const double *x, double *out, double *ref, int groups, int nvals) {
    __shared__ __attribute__((aligned(16))) double s_m[4][16];
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15, q = blockIdx.x * 4 + g;
    const bool in = q < groups;   // (no lane leaves early: the row operations need all sixteen)
    double v[10];
#pragma unroll
    for (int k = 0; k < 10; k++) v[k] = (in && k < nvals) ? x[((size_t)q * nvals + k) * 16 + l] : 0.0;
    double res;
    if (nvals == 4) {
        res = sp_group_sum4<RowOpsD>(v[0], v[1], v[2], v[3]);
    } else {
        const SpHessSums<double> hs = sp_group_sum10<RowOpsD>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
        s_m[g][l] = __builtin_nan("");
        __builtin_amdgcn_wave_barrier();
        sp_hessian_store(s_m[g], l, hs.c0, hs.c1, hs.c2);
        __builtin_amdgcn_wave_barrier();
        res = s_m[g][l];
    }
    if (in) out[(size_t)q * 16 + l] = res;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const double r = sp_group_sum<RowOpsD>(v[k]);
        if (in && k < nvals) ref[((size_t)q * nvals + k) * 16 + l] = r;
    }
}

}  // namespace

namespace msl {
namespace sf {

void sp_launch_plane(KernelProfiler &prof, hipStream_t sp, const SfDev &P, int n) {
    const int W = P.W, H = P.H;
    // 4 KB of (unused) dynamic LDS cap kb_seed_plane at 8 waves per CU (it could run 10).  Alone it is fastest uncapped -- its waves are VALU-latency
    // bound -- but the wave slots, registers and LDS it leaves go to the ORB kernels and the map stage beside it: the front end is fastest at this cap
    // (sweeps of rounds 3, 5 and 6: DESIGN.md sections 6.0 and 6.2).
    constexpr unsigned planePad = 4096;
    if (sp_quad_straddles(W)) MSL_SF_LAUNCH_LDS(prof, SK_SEED_PLANE, sp, kb_seed_plane<true>, dim3(xcd_grid(((P.spW + 1) / 2) * ((P.spH + 1) / 2), n)), dim3(64), planePad, P, n);
    else MSL_SF_LAUNCH_LDS(prof, SK_SEED_PLANE, sp, kb_seed_plane<false>, dim3(xcd_grid(((P.spW + 1) / 2) * ((P.spH + 1) / 2), n)), dim3(64), planePad, P, n);
    hipLaunchKernelGGL(kb_seed_finish, sp_seed_grid(P, n), dim3(256), 0, sp, P);
    if ((W % SP) || (H % SP)) {   // pixels outside the whole cells (sizes that are not multiples of 8)
        const int nStrip = (W - P.spW * SP) * P.spH * SP + W * (H - P.spH * SP);
        hipLaunchKernelGGL(kb_tex_strips, dim3((unsigned)((nStrip + 255) / 256), (unsigned)n), dim3(256), 0, sp, P);
    }
}

int sp_debug_group_sums(const double *x_host, int groups, int nvals, double *out_host, double *ref_host) {
    if (groups <= 0) return MSL_OK;
    if (!x_host || !out_host || !ref_host || (nvals != 4 && nvals != 10)) return MSL_ERR_INVALID;
    const size_t nx = sizeof(double) * 16 * (size_t)nvals * (size_t)groups, no = sizeof(double) * 16 * (size_t)groups;
    DevBuf x, out, ref;
    MSL_HIP_TRY(grow_all(0, {{x, nx}, {out, no}, {ref, nx}}));
    MSL_HIP_TRY(hipMemcpy(x.p, x_host, nx, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_group_sums, dim3((unsigned)((groups + 3) / 4)), dim3(64), 0, 0, (const double *)x.p, (double *)out.p, (double *)ref.p, groups, nvals);
    MSL_HIP_TRY(hipMemcpy(out_host, out.p, no, hipMemcpyDeviceToHost));
    MSL_HIP_TRY(hipMemcpy(ref_host, ref.p, nx, hipMemcpyDeviceToHost));
    return MSL_OK;
}

}  // namespace sf
}  // namespace msl
