// msl_fuse_list.h -- what the two halves of LocalMapping::SearchInNeighbors share (msl_fuse.hip for points, msl_line_fuse.hip for lines;
// internal): the limits of their items and candidate lists, the list of an item, and the first two matched candidates of every slot, on
// which both slot walks have their closed form.
#pragma once

#include "msl_match_handle.h"
#include "msl_match_math.h"

namespace msl {

constexpr int MAX_LCAP = 65536, MAX_ITEMS = 4096;
// No id, no position, no j: above every valid one, so an atomicMin keeps whatever it meets
constexpr unsigned NO_ENTRY = 0xFFFFFFFFu;

// The limits of a call's items and candidate lists; false with the error set.
inline bool item_limits(const char *who, int n_items, int lcap) {
    if (n_items < 1 || n_items > MAX_ITEMS) { set_error("%s: n_items %d outside 1 .. %d", who, n_items, MAX_ITEMS); return false; }
    if (lcap < 1 || lcap > MAX_LCAP) { set_error("%s: lcap %d outside 1 .. %d", who, lcap, MAX_LCAP); return false; }
    return true;
}

// The list of item f: its row of cand and its length (0 for a list outside the lists).  Dev: a FuseDev or an LfDev, whose list fields
// (nLists, lcap, list, cand, nCand) keep their places in the struct: the kernels' text holds the kernarg offsets.
template <class Dev>
__device__ __forceinline__ int item_list(const Dev &D, int f, const int32_t *&row) {
    const int li = D.list[f];
    if (li < 0 || li >= D.nLists) { row = D.cand; return 0; }
    row = D.cand + (size_t)li * D.lcap;
    return clampi(D.nCand[li], 0, D.lcap);
}

// The first and the second matched j of every slot of one item, by two LDS atomicMin passes of a workgroup of NT threads.  status and
// bestIdx are the call's arrays after the search and fb the item's offset in them (bestIdx of a matched candidate is its slot), `matched`
// the status of a match; skip(j, s) says that candidate j does not count for slot s.  first and second hold NO_ENTRY on entry, behind a barrier; a barrier ends each pass.
template <int NT, class Skip>
__device__ __forceinline__ void first_two_hits(const uint8_t *status, const int32_t *bestIdx, size_t fb, int matched, int nc, unsigned *first,
                                               unsigned *second, Skip skip) {
    for (int j = threadIdx.x; j < nc; j += NT)
        if (status[fb + j] == matched) { const int s = bestIdx[fb + j]; if (!skip(j, s)) atomicMin(&first[s], (unsigned)j); }
    __syncthreads();
    for (int j = threadIdx.x; j < nc; j += NT)
        if (status[fb + j] == matched) {
            const int s = bestIdx[fb + j];
            if (!skip(j, s) && first[s] != (unsigned)j) atomicMin(&second[s], (unsigned)j);
        }
    __syncthreads();
}

}  // namespace msl
